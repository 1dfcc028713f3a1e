// The per-chunk launch sequence (mavlm_step*) and the chunk K/V prefetch protocol (mavlm_project_chunk*).
#include "mavlm_ctx.h"

int g_mavlm_cache_q0 = 1;
int g_mavlm_splitk_ln = 1;

namespace {

// Is a graph capture running on `s`?  A failed query reads as `if_unknown`: the call sites that must not run inside a capture
// (the exchange-scratch memset, the attention maps, the cached first-step Q) pass true; the prefetch protocol, which only skips
// its event traffic inside a capture, passes false.
inline bool capturing(hipStream_t s, bool if_unknown) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) return if_unknown;
  return cs != hipStreamCaptureStatusNone;
}

// Residual block (MemoryController.py:26-29): out = LayerNorm(A . W^T + bias + res) * gamma + beta.  One kernel where the
// 256-column-tile GEMM fills the chip (EPI_LN: the fp32 dense output never goes through HBM), else the GEMM with its
// fp32 epilogue + the row LayerNorm kernel.  Same fp32 values into the normalisation either way; the two forms add the
// row statistics in different orders (a pure function of the shape which one runs: mavlm_linear_ln_fused).
int dense_ln(mavlm_ctx* x, hipStream_t s, const void* A, int lda, const void* W, int ldw, const float* bias, const void* res,
             const float* gamma, const float* beta, void* out, int rows, int N, int K) {
  const mavlm_config& c = x->cfg;
  if (x->fused_ln && vw(x).lnx_bytes && mavlm_gemm_ln_supported(rows, N, K, x->ln_wide) && mavlm_gemm_ln_ws_bytes(rows, N) <= vw(x).lnx_bytes &&
      mavlm_gemm_ln_ws_bytes(rows, N) <= x->lnx_bytes) {
    if (!x->lnx_clean) {
      // the library owns the "zero before the first launch" invariant of the exchange scratch: one asynchronous memset on
      // the stream of the first step after mavlm_bind_buffers.  Not inside a capture: a replayed memset would reset the
      // launch counter under the granules of the previous replay.
      if (capturing(s, true)) return MAVLM_E_STATE;
      MAVLM_TRY(hipMemsetAsync(ws(x, x->o_lnx), 0, x->lnx_bytes, s));
      x->lnx_clean = true;
    }
    mavlm_gemm_args g = gemm_args(A, lda, W, ldw, bias, res, N, out, N, rows, N, K, MAVLM_EPI_LN);
    g.ln.gamma = gamma; g.ln.beta = beta; g.ln.eps = c.eps; g.ln.wide = x->ln_wide;
    // (control words FIRST: their place must not depend on the shape - the launch counter is what keeps epochs unique)
    g.ln.ctl = (unsigned*)ws(x, x->o_lnx);
    g.ln.gran = (unsigned long long*)(ws(x, x->o_lnx) + 64);
    MAVLM_TRY(mavlm_launch_gemm(g, c.dtype, s));
    return 0;
  }
  // small grids whose contraction is split (the 4D -> D projection at few memory tokens): the fp32 planes go straight into a
  // reduce + bias + residual + LayerNorm kernel - no reduction pass, no fp32 round trip of the dense output (same bits)
  if (g_mavlm_splitk_ln && vw(x).gsplit_floats && (N & 7) == 0 && N <= MAVLM_LN_MAX_D &&
      mavlm_gemm_split_ws_floats(rows, N, K, MAVLM_EPI_F32, N) != 0 &&
      mavlm_gemm_split_ws_floats(rows, N, K, MAVLM_EPI_F32, N) <= vw(x).gsplit_floats) {
    int planes = 0;
    mavlm_gemm_args g = gemm_args(A, lda, W, ldw, bias, nullptr, 0, ws(x, x->o_pre), N, rows, N, K, MAVLM_EPI_F32);
    g.splitk_ws = p_gsplit(x); g.planes_only = 1; g.planes_out = &planes;
    MAVLM_TRY(mavlm_launch_gemm(g, c.dtype, s));
    if (planes > 0) {
      MAVLM_TRY(mavlm_launch_layernorm_planes(p_gsplit(x), planes, bias, res, N, gamma, beta, out, rows, N,
                                              c.eps, c.dtype, s));
      return 0;
    }
    // (the launch did not split after all - a tuning hook: it wrote the dense output to `pre`)
    MAVLM_TRY(mavlm_launch_layernorm((const float*)ws(x, x->o_pre), res, N, gamma, beta, out, rows, N, c.eps, c.dtype, s));
    return 0;
  }
  MAVLM_TRY(gemm_x(x, s, A, lda, W, ldw, bias, ws(x, x->o_pre), N, rows, N, K, MAVLM_EPI_F32));
  MAVLM_TRY(mavlm_launch_layernorm((const float*)ws(x, x->o_pre), res, N, gamma, beta, out, rows, N, c.eps, c.dtype, s));
  return 0;
}

// One `Attention` block given projected K/V:  out = LN(dense(attn(q_proj(xq), K, V)) + xq).  All videos of the row batch
// at once: xq / out are [B R, D]; video b's S keys start kv_bs elements after video b-1's.
// frame_rows (out): rows of the partial frame sums per video when `frames` (argument of the finish kernel)
int attn_block(mavlm_ctx* x, hipStream_t s, const mavlm_attn_weights& aw, const void* xq, const void* K, int ldk,
               const void* V, int ldv, long long kv_bs, int S, void* out, float* lse2, int frames = 0,
               int* frame_rows = nullptr, const void* q_pre = nullptr, const int* vl_S = nullptr,
               const long long* vl_off = nullptr) {
  // vl_S / vl_off (a step whose videos bring different frame counts; never with `frames`): video b has vl_S[b] keys that start
  // vl_off[b] elements into K / V - S and kv_bs are not read
  const mavlm_config& c = x->cfg;
  // (B: the videos of this step - all of the context's, or the active prefix; Bc > 1: the row-batch rules)
  const int B = x->nb, Bc = nbatch(c), R1 = q_tokens(c) * c.patches, R = R1 * B, D = c.hidden, H = c.heads, dt = c.dtype,
            Dp = padded_width(c);
  // q_pre: the projection of xq made earlier (the initial memory of a first step): no GEMM
  if (!q_pre) MAVLM_TRY(gemm_x(x, s, xq, D, aw.wq, D, aw.bq, ws(x, x->o_q), Dp, R, Dp, D, MAVLM_EPI_BIAS));
  x->q_used = q_pre ? q_pre : ws(x, x->o_q);
  mavlm_attn_args a = attn_args(x->q_used, Dp, K, ldk, V, ldv, ws(x, x->o_ctx), Dp, lse2, R1, S, H * B, attn_scale(c));
  a.nb = B; a.kv_bstride = kv_bs;
  if (frames) {       // forward + probability masses per (row, frame) or per (row, tile) in one pass (no column-sum pass)
    a.frame_scr = p_fscr(x);
    a.frame_out = p_fout(x);
    a.frame_keys = c.patches;
  }
  if (vl_S && wide_heads(c) && g_mavlm_attn_hd_varlen && c.hidden / c.heads == 448 && g_mavlm_attn_hd_qg != 1) {
    // opt-in (mavlm_set_attention_hd_varlen): ONE plain-grid launch over the B active videos - the bits of the loop below
    a.vl_S = vl_S; a.vl_off = vl_off; a.split_ws = nullptr;
    MAVLM_TRY(mavlm_launch_attention_hd_varlen(a, 448, dt, s));
  } else if (vl_S && wide_heads(c)) {
    // the default at head_dim 448 (and the only form of the 16-query-wave kernel): one launch of the forward per video, plain
    // grid (the stacked GEMMs around it are where a row batch gains at this width)
    for (int b = 0; b < B; ++b) {
      mavlm_attn_args a1 = a;
      a1.Q = (const char*)a.Q + (size_t)b * R1 * Dp * 2;
      a1.O = (char*)a.O + (size_t)b * R1 * Dp * 2;
      a1.K = (const char*)K + (size_t)vl_off[b] * 2;
      a1.V = (const char*)V + (size_t)vl_off[b] * 2;
      a1.lse2 = lse2 ? lse2 + (size_t)b * H * R1 : nullptr;
      a1.S = vl_S[b]; a1.H = H; a1.nb = 1; a1.kv_bstride = 0; a1.split_ws = nullptr;
      MAVLM_TRY(mavlm_launch_attention_hd(a1, c.hidden / c.heads, dt, s));
    }
  } else if (vl_S) {
    a.vl_S = vl_S; a.vl_off = vl_off;
    MAVLM_TRY(mavlm_launch_attention3_varlen(a, dt, s));
  } else if (wide_heads(c)) {
    // wide heads (448: the OneVision-7B width): the row batch is the grid's z dimension, or - when its units exceed the 256
    // workgroups of one-per-CU - the levelled stream-K plan over the (video, head) pairs; a single video with a small grid takes
    // the kernel's split-KV form.  The schedule is part of the result: the plan is taken only when the carved workspace covers
    // it under the CURRENT tuning hooks.
    const int hd = c.hidden / c.heads;
    const bool sk = mavlm_attention_hd_streamk(R1, S, H * B, hd, nullptr) > 0;
    if (sk) a.split_ws = mavlm_attention_hd_split_ws_floats(R1, S, H * B, hd) <= vw(x).split_floats ? p_split(x) : nullptr;
    else a.split_ws = (Bc == 1 && vw(x).split_floats) ? p_split(x) : nullptr;
    if (frames) {
      if (frame_rows) *frame_rows = mavlm_attention_hd_frames_rows_per_video(R1, H);
      MAVLM_TRY(mavlm_launch_attention_hd_frames(a, hd, dt, s));
    } else {
      MAVLM_TRY(mavlm_launch_attention_hd(a, hd, dt, s));
    }
  } else {
    // the schedule is part of the result: take it only when the carved workspace covers this shape's plan under the
    // CURRENT tuning hooks (they may have changed since mavlm_create) - never write past the carve
    // (a row batch never takes the split-KV form of the small grids: attention3.hip)
    const size_t need = (Bc == 1 || mavlm_attention_streamk_wgs(R1, S, H * B) > 0) ? mavlm_attention_split_ws_floats(R1, S, H * B) : 0;
    if (need > vw(x).split_floats) return MAVLM_E_STATE;
    a.split_ws = vw(x).split_floats ? p_split(x) : nullptr;
    if (frames == 2) {                      // per-(row, tile) masses: any schedule, incl. the split-KV small grids
      if (frame_rows) *frame_rows = H * ((R1 + 63) / 64);
      MAVLM_TRY(mavlm_launch_attention3_frame_tiles(a, dt, s));
    } else if (frames) {                    // per-frame probability mass
      if (frame_rows) *frame_rows = mavlm_attention_frames_rows_per_video(a);
      MAVLM_TRY(mavlm_launch_attention3_frames(a, dt, s));
    } else {
      MAVLM_TRY(mavlm_launch_attention(a, dt, s));
    }
  }
  // Residual: dense + bias + residual in fp32, LayerNorm (MemoryController.py:26-29)
  return dense_ln(x, s, ws(x, x->o_ctx), Dp, aw.wo, Dp, aw.bo, xq, aw.ln_g, aw.ln_b, out, R, D, Dp);
}

// does the step take the fused frame scores for a last-layer attention over S keys?  (single videos: not the small grids
// that split their keys - mavlm_frame_scores_fused; a row batch never splits)
// 0 = no (column-sum pass), 1 = per-(row, frame) masses (attention3.hip FR = 1) or the wide heads' tile entries, 2 = the tile-entry
// form of the 128-wide kernel (FR = 2: the small grids that split their keys; everywhere under mavlm_set_frame_score_mode(2))
int step_frames_fused(const mavlm_ctx* x, int S) {
  const mavlm_config& c = x->cfg;
  const int B = x->nb, Bc = nbatch(c), R1 = q_tokens(c) * c.patches;
  if (!vw(x).fscr || g_mavlm_frame_score_mode == 0) return 0;
  const bool fits = S <= (c.max_chunk_frames < 64 ? c.max_chunk_frames : 64) * c.patches;
  if (wide_heads(c))       // (any schedule: a (row, tile) entry has one writer under all of them)
    return fits && mavlm_attention_hd_frames_supported(R1, S, c.heads * B, c.hidden / c.heads, c.patches) ? 1 : 0;
  if (g_mavlm_attn_impl == 2) return 0;
  const bool tiles = vw(x).ftiles_ok && fits && mavlm_attention_frame_tiles_supported(R1, S, c.heads * B, c.patches);
  if (g_mavlm_frame_score_mode == 2) return tiles ? 2 : 0;
  if (Bc == 1) return mavlm_frame_scores_fused(R1, S, c.heads, c.patches) != 0 ? 1 : (tiles ? 2 : 0);
  return mavlm_attention_frames_supported(R1, S, c.heads * B, c.patches) ? 1 : 0;
}

// the attention-maps pass behind one attention of the step: Q of the block sits in the workspace (q_used), lse2 in o_lse; one
// launch per video
int step_maps(mavlm_ctx* x, hipStream_t s, const char* K, int ldk, long long kv_bs, int S, int k_group, int k_rot, size_t out_off) {
  const mavlm_config& c = x->cfg;
  const int B = x->nb, Bc = nbatch(c), Rq1 = q_tokens(c) * c.patches, H = c.heads, Dp = padded_width(c);
  for (int b = 0; b < B; ++b) {          // (the active videos; the scratch sits behind the maps of ALL the context's videos)
    mavlm_group_mass_args g;
    g.Q = (const char*)x->q_used + (size_t)b * Rq1 * Dp * 2; g.ldq = Dp; g.K = K + (size_t)b * kv_bs * 2; g.ldk = ldk;
    g.lse2 = (const float*)ws(x, x->o_lse) + (size_t)b * H * Rq1;
    g.out = x->maps + (size_t)b * maps_video_floats(c) + out_off;
    g.scratch = x->maps + (size_t)Bc * maps_video_floats(c);
    g.R = Rq1; g.S = S; g.H = H; g.scale = attn_scale(c); g.q_group = c.patches; g.k_group = k_group; g.k_rot = k_rot;
    MAVLM_TRY(mavlm_launch_group_mass(g, wide_heads(c) ? c.hidden / c.heads : 128, c.dtype, s));
  }
  return 0;
}

// Frame scores of the last formation layer by the column-sum pass over its Q (q_used) / K / lse2, for the B videos of the step.
// Video b's scores land ld_scores entries behind video b-1's.  Fv null: every video has F frames, its S keys b * S * ldkv elements
// into Kl.  Fv set (mavlm_step_batch_frames): video b has Fv[b] frames, its vl_S[b] keys vl_off[b] elements into Kl.
int colsum_frame_scores(mavlm_ctx* x, hipStream_t s, const char* Kl, int ldkv, float* lse, int S, int F, const int32_t* Fv,
                        const int* vl_S, const long long* vl_off, void* frame_scores, int scores_f32, long long ld_scores) {
  const mavlm_config& c = x->cfg;
  const int B = x->nb, Rq1 = q_tokens(c) * c.patches, H = c.heads, Dp = padded_width(c), dt = c.dtype;
  const size_t fs_stride = (size_t)ld_scores * (scores_f32 ? 4 : 2);        // bytes between two videos' scores
  auto scores_of = [&](int b) { return (void*)((char*)frame_scores + (size_t)b * fs_stride); };
  if (Fv && !wide_heads(c)) {
    // one column-sum launch for all videos, each on the schedule of its own key count, its planes at its prefix offset; the
    // finishing kernel adds a video's planes in order (as behind a single video's pass)
    mavlm_colsum_args ca = colsum_args(x->q_used, Dp, Kl, ldkv, lse, (float*)ws(x, x->o_vlpart), Rq1, 0, H, attn_scale(c));
    ca.nb = B; ca.keep_planes = 1; ca.vl_S = vl_S; ca.vl_kv_off = vl_off;
    size_t need = 0;
    for (int b = 0; b < B; ++b) need += mavlm_colsum_part_floats(Rq1, vl_S[b], H);
    if (!x->o_vlpart || need > x->vlpart_floats) return MAVLM_E_STATE;
    MAVLM_TRY(mavlm_launch_colsum3_varlen(ca, dt, s));
    size_t po = 0;
    for (int b = 0; b < B; ++b) {
      int planes = 1;
      mavlm_colsum_plan(Rq1, vl_S[b], H, &planes);
      MAVLM_TRY(mavlm_launch_frame_scores(ca.part + po, planes, H, vl_S[b], Fv[b], c.patches, scores_of(b), scores_f32, dt, s));
      po += mavlm_colsum_part_floats(Rq1, vl_S[b], H);
    }
    return 0;
  }
  // one pass per video through o_part (the column-sum kernels of a single key count know nothing of the row batch; head_dim 448
  // has no variable-length kernel)
  for (int b = 0; b < B; ++b) {
    const int Sb = Fv ? vl_S[b] : S, Fb = Fv ? Fv[b] : F;
    const size_t k_off = Fv ? (size_t)vl_off[b] : (size_t)b * S * ldkv;
    mavlm_colsum_args ca = colsum_args((const char*)x->q_used + (size_t)b * Rq1 * Dp * 2, Dp, Kl + k_off * 2, ldkv,
                                       lse + (size_t)b * H * Rq1, (float*)ws(x, x->o_part), Rq1, Sb, H, attn_scale(c));
    int planes = 1;
    if (wide_heads(c)) {
      MAVLM_TRY(mavlm_launch_colsum_hd(ca, c.hidden / c.heads, dt, s));
    } else {
      ca.keep_planes = 1;                   // frame_scores_kernel adds the planes (same order as the reduce kernel)
      planes = mavlm_colsum_planes(Rq1, Sb, H);
      MAVLM_TRY(mavlm_launch_colsum(ca, dt, s));
    }
    MAVLM_TRY(mavlm_launch_frame_scores(ca.part, planes, H, Sb, Fb, c.patches, scores_of(b), scores_f32, dt, s));
  }
  return 0;
}

// ---- the chunk K/V prefetch protocol of a single video: two buffers (o_kv, o_kv2), project_for writes one ahead of its step,
// chunk_kv_buffer picks the one a step reads.
//
// Which chunk K/V buffer the upcoming step reads: the one a projection made ahead for exactly this step and chunk sits in (*pre:
// the step then waits for it, nothing else); otherwise buffer 0 - or buffer 1 while a projection for a LATER step owns buffer 0.  A
// projection made for this step but another chunk is discarded (its buffer is waited for before anything overwrites it).
int chunk_kv_buffer(mavlm_ctx* x, const void* seg, int F, hipStream_t s, int* rb, bool* pre) {
  *rb = 0;
  *pre = false;
  if (nbatch(x->cfg) != 1) return 0;
  const bool cap = capturing(s, false);
  for (int b = 0; b < 2; ++b)
    if (x->pre[b].seg && x->pre[b].step == x->steps) {
      if (!*pre && !cap && x->pre[b].seg == seg && x->pre[b].F == F) { *pre = true; *rb = b; }
      x->pre[b].seg = nullptr;
    }
  if (!*pre) *rb = (x->pre[0].seg && x->pre[0].step > x->steps && x->o_kv2) ? 1 : 0;
  if (x->pre[*rb].pending) {
    // a projection into this buffer may still be running on its stream (one that was discarded, or left behind by an error):
    // an eager step waits for it; a captured one cannot (the event belongs to work outside the graph) - run an eager step first
    if (cap) return MAVLM_E_STATE;
    if (x->pre[*rb].stream != (void*)s || !*pre) MAVLM_TRY(hipStreamWaitEvent(s, x->ev_pre[*rb], 0));
    x->pre[*rb].pending = false;
  }
  return 0;
}

// K/V projection of chunk `seg` for the step with index `for_step` (>= x->steps), enqueued on `stream`
int project_for(mavlm_ctx* x, const void* seg, int32_t F, void* stream, int for_step) {
  if (!x || !seg) return MAVLM_E_ARG;
  if (!x->has_w || !x->has_b || nbatch(x->cfg) != 1) return MAVLM_E_STATE;
  const mavlm_config& c = x->cfg;
  if (F <= 0 || F > c.max_chunk_frames) return MAVLM_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (capturing(s, false)) return MAVLM_E_STATE;         // (events across streams: not inside a graph capture)
  for (int i = 0; i < 2; ++i) {
    if (!x->ev_pre[i]) MAVLM_TRY(hipEventCreateWithFlags(&x->ev_pre[i], hipEventDisableTiming));
    if (!x->ev_done[i]) MAVLM_TRY(hipEventCreateWithFlags(&x->ev_done[i], hipEventDisableTiming));
  }
  // The buffer.  For the upcoming step (index n = x->steps): buffer 0, or 1 while buffer 0 holds a projection for a later step.
  // For the step after it: buffer 1 - the upcoming step reads (or projects inline into) buffer 0 - unless buffer 1 holds the
  // projection the upcoming step is going to read, then 0.
  int tb = 0;
  if (x->o_kv2) {
    const int n = x->steps;
    if (for_step == n) tb = (x->pre[0].seg && x->pre[0].step > n) ? 1 : 0;
    else tb = (x->pre[1].seg && x->pre[1].step == n) ? 0 : 1;
  }
  if (x->pre[tb].pending && x->pre[tb].stream != stream) MAVLM_TRY(hipStreamWaitEvent(s, x->ev_pre[tb], 0));   // an older projection
  if (x->done_rec[tb]) MAVLM_TRY(hipStreamWaitEvent(s, x->ev_done[tb], 0));     // the last step that read this buffer has finished
  const int D = c.hidden, Dp = padded_width(c), ldkv = 2 * c.depth * Dp, S = F * c.patches;
  // The plan of the inline projection (gemm_x: split-K where the plan fits the step's scratch), on the projections' own scratch:
  // the step this projection overlaps uses o_gsplit on its stream.  A projection into the other buffer on another stream shares
  // this scratch: wait for it.
  const size_t need = mavlm_gemm_split_ws_floats(S, ldkv, D, MAVLM_EPI_BIAS, ldkv);
  const bool split = need > 0 && need <= x->gsplit_floats;
  if (split && need > x->kvsplit_floats) return MAVLM_E_STATE;      // (the plan covers every chunk size up to max_chunk_frames)
  if (split && x->pre[1 - tb].pending && x->pre[1 - tb].stream != stream) MAVLM_TRY(hipStreamWaitEvent(s, x->ev_pre[1 - tb], 0));
  MAVLM_TRY(gemm(c.dtype, s, seg, D, x->w.w_kv_seg, D, x->w.b_kv_seg, ws(x, tb ? x->o_kv2 : x->o_kv), ldkv, S, ldkv, D, MAVLM_EPI_BIAS,
                 nullptr, 0, split ? (float*)ws(x, x->o_kvsplit) : nullptr, split ? x->kvsplit_floats : 0));
  MAVLM_TRY(hipEventRecord(x->ev_pre[tb], s));
  x->pre[tb].seg = seg;
  x->pre[tb].F = F;
  x->pre[tb].step = for_step;
  x->pre[tb].stream = stream;
  x->pre[tb].pending = true;
  return 0;
}

// Fv (mavlm_step_batch_frames; null = every video brings F frames): video b's chunk is [Fv[b], P, D].  The chunk K/V of the videos
// then lie back to back in the chunk K/V buffer (prefix offsets), every formation layer runs the variable-length forward, and the
// frame scores of the last layer come from the variable-length column-sum launch (never fused into the forward: the memory is
// the same bits with and without scores, under every frame-score mode); video b's Fv[b] scores land at frame_scores + b * ld_scores.
int step_impl(mavlm_ctx* x, const void* const* segs, int32_t F, void* frame_scores, int32_t scores_f32, hipStream_t s,
              const int32_t* Fv = nullptr, long long ld_scores = 0) {
  const mavlm_config& c = x->cfg;
  // R1: memory rows of one video (keys of the evolution, ring strides); Rq1: the rows of them this context computes (row
  // shard: q_tokens memory tokens from row r0 on; else all); R: rows of the row-wise operators
  // B: the videos this step serves (x->nb: all Bc videos of the context, or the active prefix of a ragged row batch - their
  // rows come first in every stacked operand and in a ring slot); Bc: the videos of the context (ring strides, row-batch rules)
  const int B = x->nb, Bc = nbatch(c), R1 = c.mem_tokens * c.patches, Rq1 = q_tokens(c) * c.patches, r0 = q_row0(c), R = Rq1 * B,
            D = c.hidden, I = c.inter, L = c.depth, H = c.heads;
  const int Dp = padded_width(c);
  const int S = F * c.patches;
  const size_t slot_bytes = (size_t)R1 * Bc * D * 2;          // one FIFO slot: the newest memory of every video, [Bc, R1, D]
  const int cap = c.cache_cap;
  const int n = x->steps < cap ? x->steps : cap;
  // evolution K/V ring: [B][cap][R1][2 Dp] - the keys of ONE video are contiguous over its slots
  const long long evo_bs = (long long)cap * R1 * 2 * Dp;
  // attention maps: every attention of the step hands its lse2 to the pass behind it (same O: the forward only stores it too)
  float* const maps_lse = x->maps ? (float*)ws(x, x->o_lse) : nullptr;
  // (a replayed graph would keep writing the maps of the captured step into the caller's buffer)
  if (x->maps && capturing(s, true)) return MAVLM_E_STATE;

  const void* cur = x->w.mem0;
  if (x->steps > 0) {
    // ---- memory evolution (MemoryController.py:89-97): q = newest memory, kv = every cached memory.
    const int newest = (x->steps - 1) % cap;
    const char* mem_new = (const char*)x->b.mem_ring + (size_t)newest * slot_bytes;     // ALL rows (row shard: gathered)
    char* kv_new = (char*)x->b.evo_kv_ring + (size_t)newest * R1 * 2 * Dp * 2;
    // K/V of a cached memory are row-independent -> project each memory once, when it becomes the newest.  Row batch: ONE
    // GEMM over the stacked rows, block b of R1 rows lands in video b's ring
    {
      mavlm_gemm_args g = gemm_args(mem_new, D, x->w.w_kv_evo, D, x->w.b_kv_evo, nullptr, 0, kv_new, 2 * Dp, R1 * B, 2 * Dp, D, MAVLM_EPI_BIAS);
      if (Bc > 1) { g.c_rpb = R1; g.c_nb = B; g.c_bstride = evo_bs; }
      else if (x->gsplit_floats && mavlm_gemm_split_ws_floats(R1, 2 * Dp, D, MAVLM_EPI_BIAS, 2 * Dp) <= x->gsplit_floats)
        g.splitk_ws = (float*)ws(x, x->o_gsplit);
      MAVLM_TRY(mavlm_launch_gemm(g, c.dtype, s));
    }
    const char* kv = (const char*)x->b.evo_kv_ring;
    int rc = attn_block(x, s, x->w.evo, mem_new + (size_t)r0 * D * 2, kv, 2 * Dp, kv + (size_t)Dp * 2, 2 * Dp, evo_bs, n * R1,
                        ws(x, x->o_mA), maps_lse);
    if (rc) return rc;
    if (x->maps) {        // [H, M, n]: key group = one cached memory, oldest first (the ring's oldest slot once it is full)
      rc = step_maps(x, s, kv, 2 * Dp, evo_bs, n * R1, R1, x->steps > cap ? x->steps % cap : 0, maps_form_floats(c));
      if (rc) return rc;
    }
    cur = ws(x, x->o_mA);
  }

  // ---- memory formation (MemoryController.py:132-133): K/V of the chunk for all L layers in one GEMM per video (the shape
  // does not depend on the memory rows: nothing to gain from stacking, and the videos' frames stay where they are)
  const int ldkv = 2 * L * Dp;
  int vl_S[MAVLM_VBASE_MAX];
  long long vl_off[MAVLM_VBASE_MAX];         // elements into the chunk K/V buffer
  if (Fv) {
    if (B > MAVLM_VBASE_MAX || x->maps) return MAVLM_E_STATE;
    long long o = 0;
    for (int b = 0; b < B; ++b) {
      vl_S[b] = Fv[b] * c.patches;
      vl_off[b] = o;
      o += (long long)vl_S[b] * ldkv;
    }
  }
  int rb = 0;
  bool pre = false;
  {
    const int rc = chunk_kv_buffer(x, segs[0], F, s, &rb, &pre);
    if (rc) return rc;
  }
  x->pre_hits += pre ? 1 : 0;       // a projection made ahead for exactly this chunk
  char* kvs = ws(x, rb ? x->o_kv2 : x->o_kv);
  for (int b = 0; b < B && !pre; ++b)
    MAVLM_TRY(gemm_x(x, s, segs[b], D, x->w.w_kv_seg, D, x->w.b_kv_seg, kvs + (Fv ? (size_t)vl_off[b] : (size_t)b * S * ldkv) * 2, ldkv,
                     Fv ? vl_S[b] : S, ldkv, D, MAVLM_EPI_BIAS));
  for (int l = 0; l < L; ++l) {
    const bool last = l == L - 1;
    const bool want_scores = last && frame_scores != nullptr;
    const char* Kl = kvs + (size_t)(2 * l) * Dp * 2;
    const char* Vl = Kl + (size_t)Dp * 2;
    // frame scores: fused into this layer's forward (default), or the column-sum pass over its Q / K / lse2
    const int fused_scores = want_scores && !Fv ? step_frames_fused(x, S) : 0;
    float* lse = want_scores ? (float*)ws(x, x->o_lse) : maps_lse;     // (the fused form does not need it; kept for inspection)
    int frows = 0;
    // First step, first layer: cur is the packed initial memory and Q = mem0 . Wq^T + bq depends on the bound weights alone -
    // projected once per binding into o_q0.  A capture that starts before any eager first step keeps the GEMM inside the
    // graph (into o_q, flag untouched): the graph stays self-contained.  A graph captured with the flag set reads o_q0, which
    // goes stale exactly when the packed mem0 it also reads does.
    const void* q_pre = nullptr;
    if (l == 0 && x->steps == 0 && g_mavlm_cache_q0) {
      // (a prefix step reads the rows of a projection made for more videos where neither splits its contraction: the GEMM is
      //  row-independent then; otherwise it projects its own rows again, as a context of that many videos would)
      const size_t qneed = mavlm_gemm_split_ws_floats(R, Dp, D, MAVLM_EPI_BIAS, Dp);
      const bool qsplit = qneed != 0 && qneed <= vw(x).gsplit_floats;
      bool hit = x->q0_valid && (B == x->q0_nb || (B < x->q0_nb && !x->q0_split && !qsplit));
      if (!hit && !capturing(s, true)) {
        MAVLM_TRY(gemm_x(x, s, cur, D, x->w.layer_attn[0].wq, D, x->w.layer_attn[0].bq, ws(x, x->o_q0), Dp, R, Dp, D, MAVLM_EPI_BIAS));
        x->q0_valid = hit = true;
        x->q0_nb = B;
        x->q0_split = qsplit;
      }
      if (hit) q_pre = ws(x, x->o_q0);
    }
    int rc = attn_block(x, s, x->w.layer_attn[l], cur, Kl, ldkv, Vl, ldkv, (long long)S * ldkv, S, ws(x, x->o_a), lse,
                        fused_scores, &frows, q_pre, Fv ? vl_S : nullptr, Fv ? vl_off : nullptr);
    if (rc) return rc;
    if (x->maps) {        // [H, M, F] of layer l: query group = one memory token, key group = one frame
      rc = step_maps(x, s, Kl, ldkv, (long long)S * ldkv, S, c.patches, 0, (size_t)l * H * q_tokens(c) * F);
      if (rc) return rc;
    }
    if (fused_scores) {
      MAVLM_TRY(mavlm_launch_frame_finish(p_fout(x), frows, B, F, c.patches, frame_scores, scores_f32, c.dtype, s));
    } else if (want_scores) {
      rc = colsum_frame_scores(x, s, Kl, ldkv, lse, S, F, Fv, vl_S, vl_off, frame_scores, scores_f32, Fv ? ld_scores : F);
      if (rc) return rc;
    }
    // MLP: Linear(D,I)+ReLU -> Residual(I->D)  (MemoryController.py:63-67,71)
    MAVLM_TRY(gemm_x(x, s, ws(x, x->o_a), D, x->w.w_up[l], D, x->w.b_up[l], ws(x, x->o_h), I, R, I, D, MAVLM_EPI_RELU));
    // (row shard: this context's rows of the slot; the host all-gathers the other ranks' rows into it before the next step)
    void* dst = last ? (void*)((char*)x->b.mem_ring + (size_t)(x->steps % cap) * slot_bytes + (size_t)r0 * D * 2)
                     : (void*)ws(x, (l & 1) ? x->o_mA : x->o_mB);
    rc = dense_ln(x, s, ws(x, x->o_h), I, x->w.w_down[l], I, x->w.b_down[l], ws(x, x->o_a), x->w.ln2_g[l], x->w.ln2_b[l], dst, R, D, I);
    if (rc) return rc;
    cur = dst;
  }
  // the chunk K/V buffer this step read is free once the stream gets here
  if (Bc == 1 && x->o_kv2 && x->ev_done[rb] && !capturing(s, false)) {
    MAVLM_TRY(hipEventRecord(x->ev_done[rb], s));
    x->done_rec[rb] = true;
  }
  x->steps += 1;   // append; the slot written above evicts the oldest entry once the ring is full (:152-154)
  for (int b = 0; b < B; ++b) x->vsteps[b] += 1;
  x->n_active = B;
  return 0;
}

}  // namespace

extern "C" {

int mavlm_step(mavlm_ctx* x, const void* seg, int32_t F, void* frame_scores, int32_t scores_f32, void* stream) {
  if (!x || !seg) return MAVLM_E_ARG;
  if (!x->has_w || !x->has_b) return MAVLM_E_STATE;
  if (nbatch(x->cfg) != 1) return MAVLM_E_STATE;             // a row-batched context steps through mavlm_step_batch
  if (F <= 0 || F > x->cfg.max_chunk_frames) return MAVLM_E_SHAPE;
  return step_impl(x, &seg, F, frame_scores, scores_f32, (hipStream_t)stream);
}

int mavlm_step_batch(mavlm_ctx* x, const void* const* segs, int32_t F, void* frame_scores, int32_t scores_f32, void* stream) {
  if (!x || !segs) return MAVLM_E_ARG;
  if (!x->has_w || !x->has_b) return MAVLM_E_STATE;
  if (F <= 0 || F > x->cfg.max_chunk_frames) return MAVLM_E_SHAPE;
  for (int b = 0; b < nbatch(x->cfg); ++b)
    if (!segs[b]) return MAVLM_E_ARG;
  if (x->n_active != 0 && x->n_active < nbatch(x->cfg)) return MAVLM_E_STATE;      // (the prefix of a ragged batch never grows)
  x->nb = nbatch(x->cfg);
  return step_impl(x, segs, F, frame_scores, scores_f32, (hipStream_t)stream);
}

int mavlm_step_batch_active(mavlm_ctx* x, const void* const* segs, int32_t n_active, int32_t F, void* frame_scores,
                            int32_t scores_f32, void* stream) {
  if (!x || !segs) return MAVLM_E_ARG;
  if (n_active < 1 || n_active > nbatch(x->cfg)) return MAVLM_E_ARG;
  if (nbatch(x->cfg) < 2) return MAVLM_E_STATE;            // (a single video steps through mavlm_step)
  if (!x->has_w || !x->has_b) return MAVLM_E_STATE;
  if (F <= 0 || F > x->cfg.max_chunk_frames) return MAVLM_E_SHAPE;
  for (int b = 0; b < n_active; ++b)
    if (!segs[b]) return MAVLM_E_ARG;
  if (x->n_active != 0 && n_active > x->n_active) return MAVLM_E_STATE;            // all videos start together; the prefix only shrinks
  x->nb = n_active;
  const int rc = step_impl(x, segs, F, frame_scores, scores_f32, (hipStream_t)stream);
  x->nb = nbatch(x->cfg);
  return rc;
}

int mavlm_step_batch_frames(mavlm_ctx* x, const void* const* segs, const int32_t* F, int32_t n_active, void* frame_scores,
                            int64_t ld_scores, int32_t scores_f32, void* stream) {
  // every check comes before anything is enqueued
  if (!x || !segs || !F) return MAVLM_E_ARG;
  if (n_active < 1 || n_active > nbatch(x->cfg)) return MAVLM_E_ARG;
  if (nbatch(x->cfg) < 2) return MAVLM_E_STATE;            // (a single video steps through mavlm_step)
  bool equal = true;
  int fmax = 0;
  for (int b = 0; b < n_active; ++b) {
    if (!segs[b]) return MAVLM_E_ARG;
    if (F[b] < 1 || F[b] > x->cfg.max_chunk_frames) return MAVLM_E_ARG;
    equal = equal && F[b] == F[0];
    fmax = F[b] > fmax ? F[b] : fmax;
  }
  if (frame_scores && ld_scores < fmax) return MAVLM_E_ARG;
  if (!x->has_w || !x->has_b) return MAVLM_E_STATE;
  if (x->n_active != 0 && n_active > x->n_active) return MAVLM_E_STATE;            // the prefix only shrinks
  // all videos with the same frame count and scores packed [n_active, F]: the existing step, bit for bit
  if (equal && (!frame_scores || ld_scores == F[0]))
    return mavlm_step_batch_active(x, segs, n_active, F[0], frame_scores, scores_f32, stream);
  if (n_active > MAVLM_VBASE_MAX) return MAVLM_E_ARG;       // the per-video counts travel by value
  if (x->maps) return MAVLM_E_STATE;                       // attention maps of videos with different frame counts: not provided
  x->nb = n_active;
  const int rc = step_impl(x, segs, fmax, frame_scores, scores_f32, (hipStream_t)stream, F, ld_scores);
  x->nb = nbatch(x->cfg);
  return rc;
}

int mavlm_project_chunk(mavlm_ctx* x, const void* seg, int32_t F, void* stream) { return project_for(x, seg, F, stream, x ? x->steps : 0); }
int mavlm_project_chunk_ahead(mavlm_ctx* x, const void* seg, int32_t F, void* stream) {
  if (x && !x->o_kv2) return MAVLM_E_STATE;
  return project_for(x, seg, F, stream, x ? x->steps + 1 : 0);
}

}  // extern "C"
