// Host layer behind the C ABI (include/mavlm.h): the context, the workspace plan and what the host translation units share
// (mavlm_context.hip, mavlm_step.hip, mavlm_emit.hip, mavlm_ops.hip).  No allocation, no synchronisation: every entry point
// only enqueues kernels on the caller's stream.
#pragma once
#include "../../include/mavlm.h"

#include <math.h>

#include "mavlm_kernels.h"

extern int g_mavlm_fused_ln;    // process-wide hook (mavlm_set_fused_layernorm); contexts snapshot it at mavlm_create
extern int g_mavlm_cache_q0;    // the first step's first Q projection is made once per weight binding (mavlm_set_cache_initial_q)
extern int g_mavlm_splitk_ln;   // dense + LayerNorm over a split contraction: planes -> reduce + LayerNorm in one kernel (mavlm_set_splitk_layernorm)

#pragma GCC visibility push(hidden)   // (internal to the library: the exported symbols are include/mavlm.h and the hooks above)

// The workspace layout of one video count (plan_of, mavlm_context.hip): a pure function of the config and, at the time of the call, of the two
// LayerNorm hooks it snapshots.  Byte offsets into mavlm_buffers.workspace; sizes in floats / bytes as named.
struct mavlm_plan {
  size_t o_kv = 0, o_q = 0, o_ctx = 0, o_a = 0, o_h = 0, o_pre = 0, o_mA = 0, o_mB = 0, o_lse = 0, o_part = 0, o_split = 0, o_gsplit = 0,
         gsplit_floats = 0, total = 0;
  size_t o_fscr = 0, o_fout = 0;   // frame-score variant of the last layer's forward (0 = not available for this config)
  bool ftiles_ok = false;          // ... and the carve covers its tile-entry form (attention3.hip FR = 2)
  size_t fscr_floats = 0, fout_floats = 0;
  size_t split_floats = 0;         // floats carved at o_split (attention partials: split-KV / stream-K)
  size_t o_lnx = 0, lnx_bytes = 0; // scratch of the fused dense + residual + LayerNorm GEMM epilogue (0 = not used for this config)
  size_t o_stage = 0, stage_bytes = 0;   // fused memory rows of a gapped token layout where the fuser's last writer has no row map (fuse_stage_bytes)
  size_t o_kv2 = 0;                // second chunk K/V buffer (0 = none: row batches)
  size_t o_kvsplit = 0, kvsplit_floats = 0;   // split-K scratch of the projections made ahead (project_for), never shared with a step
  size_t o_q0 = 0;                 // the cached first-step Q (mavlm_ctx::q0_valid), behind every other region of the plan
  int fuse_mems = 1;   // cached memories the Memory-Fuser MLP takes per GEMM launch (mavlm_fuse_emit)
  int fused_ln = 1;    // snapshot of the process-wide hook at mavlm_create (0 = two-kernel form, 1 / 2 = fused where supported)
  int ln_wide = 0;     // ... and of its "rows of up to 4096 columns" test mode
};

// Ragged row batch (mavlm_step_batch_active): a step serves the first nb videos.  view[v] holds what the plan of a context
// created with batch = v decides by - a step over v videos takes the schedule of that context (v = 1: the row-batch rules at
// one video).  view[B] is this context's own plan.  Where a view needs more scratch than the region of the own plan, the
// steps with nb < B use a region of their own BEHIND o_q0 (o_x*: 0 = the own region covers every view).
struct mavlm_nb_view { size_t gsplit_floats = 0, split_floats = 0, lnx_bytes = 0, fscr_floats = 0, fout_floats = 0; bool fscr = false, ftiles_ok = false; };
struct mavlm_carve : mavlm_plan {
  mavlm_nb_view view[MAVLM_MAX_BATCH + 1];
  size_t o_xsplit = 0, o_xgsplit = 0, o_xfscr = 0, o_xfout = 0;
  size_t o_vlpart = 0, vlpart_floats = 0;   // column-sum planes of a step with per-video frame counts (mavlm_step_batch_frames)
};
mavlm_carve mavlm_carve_of(const mavlm_config& c);

struct mavlm_ctx : mavlm_carve {
  mavlm_config cfg;
  mavlm_weights w;
  mavlm_buffers b;
  bool has_w = false, has_b = false;
  int steps = 0;
  // K/V projections of chunks ahead of their step (mavlm_project_chunk: the next step; mavlm_project_chunk_ahead: the one after it,
  // on another stream): two chunk K/V buffers (o_kv, o_kv2; single videos), a slot per buffer
  struct pre_slot {
    const void* seg = nullptr;     // the chunk whose K/V the buffer holds / will hold (0 = none)
    int F = 0, step = -1;          // ... for the step with this index
    void* stream = nullptr;        // the stream the projection was enqueued on
    bool pending = false;          // a projection into this buffer may still be in flight on `stream` (ev_pre not waited for yet)
  } pre[2];
  hipEvent_t ev_pre[2] = {nullptr, nullptr};    // recorded behind a projection into buffer b
  hipEvent_t ev_done[2] = {nullptr, nullptr};   // recorded behind the last step that read buffer b
  bool done_rec[2] = {false, false};
  int pre_hits = 0;                // steps that reused a projection (mavlm_prefetch_hits: tests)
  ~mavlm_ctx() {
    for (int i = 0; i < 2; ++i) {
      if (ev_pre[i]) (void)hipEventDestroy(ev_pre[i]);
      if (ev_done[i]) (void)hipEventDestroy(ev_done[i]);
    }
  }
  float* maps = nullptr;    // attention maps of every step (mavlm_bind_attention_maps): the caller's buffer, null = off
  bool lnx_clean = false;   // the exchange scratch of this workspace has been zero-filled since the last mavlm_bind_buffers
  // Q of the first step's first formation layer, mem0 . Wq^T + bq: a function of the bound weights alone.  Projected once
  // per binding into its own region (o_q0); cleared by mavlm_bind_weights (other weights) and mavlm_bind_buffers (another workspace)
  bool q0_valid = false;
  int q0_nb = 0;                  // videos whose rows the projection covers (a prefix of a larger one is valid: the rows of B
                                  // copies of mem0), and whether it split its contraction (then only the same count reads it)
  bool q0_split = false;
  const void* q_used = nullptr;   // the Q the last attn_block ran on (o_q, or o_q0): what the passes behind it read
  int nb = 1;                     // videos of the step / emit launch in flight (B outside mavlm_step_batch_active)
  int n_active = 0;               // videos of the last step since mavlm_reset (0 = none yet)
  int vsteps[MAVLM_MAX_BATCH] = {};   // steps of each video since mavlm_reset
};

inline int nbatch(const mavlm_config& c) { return c.batch > 1 ? c.batch : 1; }
// row shard (mavlm_config.q_tokens): memory tokens this context computes per step, and the first of them
inline int q_tokens(const mavlm_config& c) { return c.q_tokens > 0 ? c.q_tokens : c.mem_tokens; }
inline int q_row0(const mavlm_config& c) { return c.q_tokens > 0 ? c.q_token0 * c.patches : 0; }
inline bool wide_heads(const mavlm_config& c) { return c.hidden / c.heads > 128; }
inline int padded_width(const mavlm_config& c) { return wide_heads(c) ? c.hidden : c.heads * 128; }
inline float attn_scale(const mavlm_config& c) { return 1.0f / sqrtf((float)(c.hidden / c.heads)); }

inline char* ws(mavlm_ctx* x, size_t off) { return (char*)x->b.workspace + off; }
// what the step in flight decides by and where its count-dependent scratch lies (mavlm_carve::view; the own plan for all B videos)
inline const mavlm_nb_view& vw(const mavlm_ctx* x) { return x->view[x->nb]; }
inline bool prefix_step(const mavlm_ctx* x) { return x->nb < nbatch(x->cfg); }
inline float* p_gsplit(mavlm_ctx* x) { return (float*)ws(x, prefix_step(x) && x->o_xgsplit ? x->o_xgsplit : x->o_gsplit); }
inline float* p_split(mavlm_ctx* x) { return (float*)ws(x, prefix_step(x) && x->o_xsplit ? x->o_xsplit : x->o_split); }
inline float* p_fscr(mavlm_ctx* x) { return (float*)ws(x, prefix_step(x) && x->o_xfscr ? x->o_xfscr : x->o_fscr); }
inline float* p_fout(mavlm_ctx* x) { return (float*)ws(x, prefix_step(x) && x->o_xfout ? x->o_xfout : x->o_fout); }

#define MAVLM_TRY(expr)                       \
  do {                                        \
    hipError_t _e = (expr);                   \
    if (_e != hipSuccess) return (int)_e;     \
  } while (0)

// the launchers refuse bad arguments with hipErrorInvalidValue: the ABI's MAVLM_E_ARG; every other HIP error travels as it is
inline int api_rc(hipError_t e) { return e == hipErrorInvalidValue ? MAVLM_E_ARG : (int)e; }

// mavlm_context.hip
bool cfg_ok(const mavlm_config* c);
bool shape_ok(const mavlm_config* c);
// The fuser's second GEMM of a launch over `rows` memory rows of a single video, as mavlm_fuse_emit issues it (C / split_ws: only
// their being set and 16-byte aligned matters to the dispatch)
mavlm_gemm_args fuser_out_gemm(const mavlm_config& c, int rows, void* C, float* split_ws, size_t split_floats);
bool maps_supported(const mavlm_config& c);
size_t maps_floats(const mavlm_config& c);      // the caller's whole buffer: every video's maps + the scratch of the pass

// mavlm_ops.hip
mavlm_gemm_args gemm_args(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res, int ldr, void* C,
                          int ldc, int M, int N, int K, int epi);
hipError_t gemm(int dtype, hipStream_t s, const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc,
                int M, int N, int K, int epi, const void* res = nullptr, int ldr = 0, float* split_ws = nullptr,
                size_t split_floats = 0);
// GEMM of the fused step: the split-K workspace of the context rides along, so that every launch takes the same plan
// as the stand-alone operator (mavlm_linear_ws) would for its shape
inline hipError_t gemm_x(mavlm_ctx* x, hipStream_t s, const void* A, int lda, const void* W, int ldw, const float* bias, void* C,
                         int ldc, int M, int N, int K, int epi) {
  return gemm(x->cfg.dtype, s, A, lda, W, ldw, bias, C, ldc, M, N, K, epi, nullptr, 0,
              vw(x).gsplit_floats ? p_gsplit(x) : nullptr, vw(x).gsplit_floats);
}
mavlm_attn_args attn_args(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, float* lse2,
                          int R, int S, int H, float scale);
mavlm_colsum_args colsum_args(const void* Q, int ldq, const void* K, int ldk, const float* lse2, float* part, int R, int S, int H,
                              float scale);

// mavlm_emit.hip
int layout_gap(const mavlm_config& c, int32_t layout);
int64_t block_rows(int64_t rows, int32_t layout, int gap);

// ---- attention maps (mavlm_bind_attention_maps): layout of the caller's buffer.  Per video: the formation maps of a step
// [depth, H, M, F] (compact for the step's F) in a region sized for max_chunk_frames, then the evolution map [H, M, n] in a region
// sized for cache_cap; behind the last video the scratch of the pass.
inline size_t maps_form_floats(const mavlm_config& c) { return (size_t)c.depth * c.heads * q_tokens(c) * c.max_chunk_frames; }
inline size_t maps_video_floats(const mavlm_config& c) { return maps_form_floats(c) + (size_t)c.heads * q_tokens(c) * c.cache_cap; }

#pragma GCC visibility pop
