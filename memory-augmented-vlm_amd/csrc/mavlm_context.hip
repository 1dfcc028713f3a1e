// Context and workspace: config checks, the workspace plan, create / bind / reset and the small getters (include/mavlm.h).
#include <new>

#include "mavlm_ctx.h"

int g_mavlm_fused_ln = 1;

bool cfg_ok(const mavlm_config* c) {
  if (!c) return false;
  if (c->hidden <= 0 || c->heads <= 0 || c->patches <= 0 || c->mem_tokens <= 0 || c->depth <= 0 ||
      c->depth > MAVLM_MAX_DEPTH || c->inter <= 0 || c->cache_cap <= 0 || c->max_chunk_frames <= 0)
    return false;
  if (c->dtype != 0 && c->dtype != 1) return false;
  if (c->batch < 0 || c->batch > MAVLM_MAX_BATCH) return false;
  if (c->q_tokens < 0 || c->q_token0 < 0 || c->q_token0 + c->q_tokens > c->mem_tokens || (c->q_tokens == 0 && c->q_token0 != 0))
    return false;
  if (c->q_tokens > 0 && c->batch > 1) return false;           // a row shard of ONE video, or a row batch of whole videos
  if (c->fused_ln != MAVLM_LN_AUTO && c->fused_ln != MAVLM_LN_NEVER) return false;
  return true;
}

// shapes the gfx950 kernels implement (DESIGN.md "Supported shapes"): head_dim <= 128 (heads are zero-padded to
// 128 columns in the Q/K/V/ctx buffers and in the packed weights), D and I multiples of 128, D <= MAVLM_MAX_HIDDEN (the
// widest row of the LayerNorm kernels, forward and backward: a wider context would fail inside its first step)
static_assert(MAVLM_MAX_HIDDEN == MAVLM_LN_MAX_D, "include/mavlm.h and mavlm_kernels.h state the same limit");
bool shape_ok(const mavlm_config* c) {
  if (c->hidden % 128 != 0 || c->hidden % c->heads != 0 || c->inter % 128 != 0 || c->hidden > MAVLM_MAX_HIDDEN) return false;
  const int hd = c->hidden / c->heads;
  return hd <= 128 || hd == 448;      // 448: wide-head kernels (attention_hd.hip), no padding
}

mavlm_gemm_args fuser_out_gemm(const mavlm_config& c, int rows, void* C, float* split_ws, size_t split_floats) {
  mavlm_gemm_args g = gemm_args(nullptr, c.inter, nullptr, c.inter, nullptr, nullptr, 0, C, c.hidden, rows, c.hidden, c.inter, MAVLM_EPI_BIAS);
  if (split_ws != nullptr && mavlm_gemm_split_ws_floats(rows, c.hidden, c.inter, MAVLM_EPI_BIAS, c.hidden) <= split_floats) g.splitk_ws = split_ws;
  return g;
}

namespace {

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// Memory-Fuser batching: the fuser MLP is row-independent, and the FIFO ring is one contiguous [cap, R, D] buffer, so
// cached memories that sit in consecutive slots go through ONE pair of GEMMs.  At the reference's 8 memory tokens
// (R = 1568) a launch per memory fills 7 of 256 CUs' worth of 256-row tiles; up to FUSE_ROWS rows per launch fill the chip.
constexpr int FUSE_ROWS = 32768;
inline int fuse_mems_per_launch(const mavlm_config& c) {
  const int R = c.mem_tokens * c.patches * nbatch(c);       // rows of one FIFO slot (all videos of the row batch)
  int k = FUSE_ROWS / R;
  if (k < 1) k = 1;
  return k > c.cache_cap ? c.cache_cap : k;
}

// floats of the split-K planes of the GEMMs with few output tiles and a long contraction (mavlm_gemm_splits): the I -> D
// projections (MLP down, fuser second layer) at small R - the scratch o_gsplit every GEMM of a step shares (on the step's stream)
size_t gemm_split_floats(const mavlm_config& c) {
  const size_t B = (size_t)nbatch(c);
  const size_t R1 = (size_t)q_tokens(c) * c.patches, R = (size_t)c.mem_tokens * c.patches * B;
  const int sk = c.max_chunk_frames * c.patches, d = c.hidden, dp = padded_width(c), in = c.inter, l2 = 2 * c.depth * dp;
  size_t fl = 0;
  const int rows_[2] = {(int)R, (int)(R1 * B)};              // every row of the memory / the rows of a row shard
  for (int r : rows_) {
    const size_t need[] = {mavlm_gemm_split_ws_floats(r, dp, d, MAVLM_EPI_BIAS, dp),      // q projection
                           mavlm_gemm_split_ws_floats(r, d, dp, MAVLM_EPI_F32, d),        // attention out dense
                           mavlm_gemm_split_ws_floats(r, in, d, MAVLM_EPI_RELU, in),      // MLP up / fuser first
                           mavlm_gemm_split_ws_floats(r, d, in, MAVLM_EPI_F32, d),        // MLP down / fuser second
                           mavlm_gemm_split_ws_floats(sk, l2, d, MAVLM_EPI_BIAS, l2),     // chunk K/V
                           mavlm_gemm_split_ws_floats(r, 2 * dp, d, MAVLM_EPI_BIAS, 2 * dp)};   // evolution K/V
    for (size_t n : need) fl = n > fl ? n : fl;
  }
  return fl;
}

// Token layouts with newline rows INSIDE the memory block (MAVLM_LAYOUT_FRAME / _GRID): the fuser's second GEMM scatters its
// rows itself where it runs on a 256-column-tile kernel (mavlm_gemm_args::c_gap).  The small grids of a single video that
// take the 128^2 kernel or the split-K reduce - writers of M x N contiguous elements - write here instead and one copy
// kernel places the rows: the bytes of the largest such launch (0 = every launch of this config maps its rows).
size_t fuse_stage_bytes(const mavlm_config& c, int fuse_mems, size_t gsplit_floats) {
  if (nbatch(c) > 1) return 0;                      // (a row batch only ever runs kernels with the row map)
  size_t rows_max = 0;
  for (int run = 1; run <= fuse_mems; ++run) {
    const int rows = run * c.mem_tokens * c.patches;
    const mavlm_gemm_args g = fuser_out_gemm(c, rows, (void*)(uintptr_t)256, gsplit_floats ? (float*)(uintptr_t)256 : nullptr, gsplit_floats);
    if (!mavlm_gemm_row_map_ok(g)) rows_max = (size_t)rows;
  }
  return rows_max * (size_t)c.hidden * 2;
}

// largest column-sum plane set of one video over every chunk size (attention3.hip: balanced schedule - the plane count depends on
// the chunk's key count)
size_t colsum_floats_max(const mavlm_config& c) {
  const int R1 = q_tokens(c) * c.patches;
  size_t fl = 0;
  for (int f = 1; f <= c.max_chunk_frames; ++f) {
    const size_t v = mavlm_colsum_part_floats(R1, f * c.patches, c.heads);
    if (v > fl) fl = v;
  }
  return fl;
}

// rb_one: the plan of ONE video under the row-batch rules (the nb = 1 view of a row-batched context): none of the single-video
// context's extras - no second chunk K/V buffer, no split-KV partials (the GEMMs of a step keep the plan of their shape; the
// evolution K/V projection goes through the row map, which never splits)
mavlm_plan plan_of(const mavlm_config& c, bool rb_one) {
  mavlm_plan p;
  const size_t B = (size_t)nbatch(c);
  const bool single = B == 1 && !rb_one;
  const size_t Rf = (size_t)c.mem_tokens * c.patches;          // memory rows of ONE video (row buffers: sized for all of them)
  const size_t R1 = (size_t)q_tokens(c) * c.patches;           // query rows of one video this context computes (row shard)
  const size_t R = Rf * B;                                     // rows of every row-wise operator (all videos stacked)
  const size_t S = (size_t)c.max_chunk_frames * c.patches, D = c.hidden, I = c.inter, L = c.depth, H = c.heads,
               Dp = (size_t)padded_width(c);
  size_t o = 0;
  p.o_kv = o;   o += al(B * S * 2 * L * Dp * 2);
  p.gsplit_floats = gemm_split_floats(c);
  if (single) {
    p.o_kv2 = o; o += al(S * 2 * L * Dp * 2);      // landing zone of mavlm_project_chunk_ahead
    // A projection made ahead runs on another stream than the step it overlaps, so it cannot borrow the step's split-K scratch
    // (o_gsplit: the planes of the step's own small-grid GEMMs).  It gets one of its own, sized for the plan the inline projection
    // takes (gemm_x: split where the plan fits the step's scratch) at every chunk size up to max_chunk_frames - same plan, same bits.
    const int l2 = (int)(2 * L * Dp);
    for (int f = 1; f <= c.max_chunk_frames; ++f) {
      const size_t need = mavlm_gemm_split_ws_floats(f * c.patches, l2, (int)D, MAVLM_EPI_BIAS, l2);
      if (need <= p.gsplit_floats && need > p.kvsplit_floats) p.kvsplit_floats = need;
    }
    if (p.kvsplit_floats) { p.o_kvsplit = o; o += al(p.kvsplit_floats * 4); }
  }
  p.o_q = o;    o += al(R * Dp * 2);
  p.o_ctx = o;  o += al(R * Dp * 2);
  p.o_a = o;    o += al(R * D * 2);
  p.fuse_mems = fuse_mems_per_launch(c);
  p.o_h = o;    o += al((size_t)p.fuse_mems * R * I * 2);     // MLP hidden of a step (R rows) / of a fuser batch
  p.o_pre = o;  o += al(R * D * 4);
  p.o_mA = o;   o += al(R * D * 2);
  p.o_mB = o;   o += al(R * D * 2);
  p.o_lse = o;  o += al(B * H * R1 * 4);
  {   // column-sum planes of one video
    const size_t fl = wide_heads(c) ? 0 : colsum_floats_max(c);
    p.o_part = o; o += al((fl > H * S ? fl : H * S) * 4);
  }
  // attention partials.  Single videos: split-KV of the small grids (mavlm_attention_splits), worst case over the key
  // count, or the levelled stream-K schedule (more units than workgroup slots; independent of the key count).  The
  // stream-K size is the maximum over both workgroup shapes (4 / 8 waves), so that mavlm_set_attention_streamk_waves
  // may change after the context exists; attn_block checks the carved size anyway.
  p.o_split = o;
  {
    const size_t items = ((R1 + 127) / 128) * H;
    size_t fl = 0;
    if (single) {
      size_t cap;
      if (!wide_heads(c)) cap = items < 320 ? (512 / items > 8 ? 8 : 512 / items) : 0;      // mavlm_attention_splits
      else cap = (size_t)mavlm_attention_hd_splits((int)R1, 1 << 20, (int)H, nullptr);       // (its maximum over the key count)
      fl = cap >= 2 ? cap * (R1 * Dp + H * R1) : 0;
    }
    const int s_long = 1 << 20;          // (the stream-K schedules only depend on "enough key tiles")
    if (!wide_heads(c)) {
      const size_t sk = mavlm_attention_split_ws_floats_max((int)R1, s_long, (int)(H * B));
      if (sk > fl) fl = sk;
    } else if (mavlm_attention_hd_streamk((int)R1, s_long, (int)(H * B), c.hidden / c.heads, nullptr) > 0) {
      const size_t sk = mavlm_attention_hd_split_ws_floats((int)R1, s_long, (int)(H * B), c.hidden / c.heads);
      if (sk > fl) fl = sk;
    }
    p.split_floats = fl;
    if (fl) o += al(fl * 4);
  }
  // split-K planes of the step's GEMMs (gemm_split_floats)
  p.o_gsplit = o;
  o += al(p.gsplit_floats * 4);
  // scratch of the frame-score variant of the last formation layer's forward (attention3.hip): (a, m) per (head, memory
  // row, frame) and the partial frame sums per (unit, 32-query group)
  {
    const int fc = c.max_chunk_frames < 64 ? c.max_chunk_frames : 64;      // chunks of more frames take the column-sum pass
    const bool sup1 = !wide_heads(c) && mavlm_attention_frames_supported((int)R1, fc * c.patches, (int)(H * B), c.patches);
    const bool sup2 = !wide_heads(c) && mavlm_attention_frame_tiles_supported((int)R1, fc * c.patches, (int)(H * B), c.patches) &&
                      mavlm_attention_frame_tiles_scr_floats((int)R1, fc * c.patches, (int)(H * B)) * 4 <= ((size_t)1 << 30);
    bool any = sup1 || sup2;
    if (any) {
      // the per-(row, frame) form and / or the per-(row, 64-key tile) form (the small grids that split their keys): the larger of both
      size_t scr = sup1 ? mavlm_attention_frames_scr_floats((int)R1, fc * c.patches, (int)(H * B), c.patches) : 0;
      size_t out = sup1 ? mavlm_attention_frames_out_floats((int)R1, fc * c.patches, (int)(H * B), c.patches) : 0;
      if (sup2) {
        const size_t s2 = mavlm_attention_frame_tiles_scr_floats((int)R1, fc * c.patches, (int)(H * B));
        const size_t o2 = mavlm_attention_frame_tiles_out_floats((int)R1, c.patches, (int)(H * B), c.patches) * 64;
        scr = s2 > scr ? s2 : scr;
        out = o2 > out ? o2 : out;
      }
      p.ftiles_ok = sup2;
      p.fscr_floats = scr; p.fout_floats = out;
    } else if (wide_heads(c) && mavlm_attention_hd_frames_supported((int)R1, fc * c.patches, (int)(H * B), c.hidden / c.heads, c.patches) &&
               mavlm_attention_hd_frames_scr_floats((int)R1, fc * c.patches, (int)(H * B)) * 4 <= ((size_t)1 << 30)) {
      // head_dim 448 (attention_hd.hip): one 8-byte entry per (head, memory row, 32-key tile) - up to 1 GiB, else the column-sum pass
      p.fscr_floats = mavlm_attention_hd_frames_scr_floats((int)R1, fc * c.patches, (int)(H * B));
      p.fout_floats = mavlm_attention_hd_frames_out_floats((int)R1, c.patches, (int)(H * B), c.patches) * 64;
      any = true;
    }
    if (any) {
      p.o_fscr = o; o += al(p.fscr_floats * 4);
      p.o_fout = o; o += al(p.fout_floats * 4);
    }
  }
  // scratch of the fused dense + residual + LayerNorm epilogue (gemm256.hip EPI_LN): {epoch, value} granules of the row
  // blocks + control words.  MUST be zero when the workspace is bound (mavlm_buffers.workspace).
  // the process-wide hook is SNAPSHOTTED here (the plan is made once per context, at mavlm_create): a live context keeps its form
  p.fused_ln = c.fused_ln == MAVLM_LN_NEVER ? 0 : g_mavlm_fused_ln;
  p.ln_wide = g_mavlm_gemm_ln_wide;
  if (p.fused_ln) {
    const int rows_[2] = {(int)R, (int)(R1 * B)};
    for (int r : rows_)
      if (mavlm_gemm_ln_supported(r, (int)D, (int)Dp, p.ln_wide) || mavlm_gemm_ln_supported(r, (int)D, (int)I, p.ln_wide)) {
        const size_t b = mavlm_gemm_ln_ws_bytes(r, (int)D);
        if (b > p.lnx_bytes) p.lnx_bytes = b;
      }
    if (p.lnx_bytes) { p.o_lnx = o; o += al(p.lnx_bytes); }
  }
  p.stage_bytes = fuse_stage_bytes(c, p.fuse_mems, p.gsplit_floats);
  if (p.stage_bytes) { p.o_stage = o; o += al(p.stage_bytes); }
  p.o_q0 = o; o += al(R * Dp * 2);       // (behind every region above: none of their offsets moves)
  p.total = o;
  return p;
}

inline mavlm_nb_view view_of(const mavlm_plan& t) {
  mavlm_nb_view v;
  v.gsplit_floats = t.gsplit_floats; v.split_floats = t.split_floats; v.lnx_bytes = t.lnx_bytes;
  v.fscr_floats = t.fscr_floats; v.fout_floats = t.fout_floats; v.fscr = t.o_fscr != 0; v.ftiles_ok = t.ftiles_ok;
  return v;
}

}  // namespace

// The context's own plan, then - row batches - the views of the smaller video counts and the scratch they need beyond it.
// The need is NOT monotone in the video count (the attention partials follow the plan): every count is planned and the
// largest taken.  The additional regions sit behind o_q0, so a context only ever stepped with all B videos finds every
// region where it was.
mavlm_carve mavlm_carve_of(const mavlm_config& c) {
  mavlm_carve x;
  static_cast<mavlm_plan&>(x) = plan_of(c, false);
  const int B = nbatch(c);
  x.view[B] = view_of(x);
  if (B < 2) return x;
  mavlm_nb_view mx;
  for (int v = 1; v < B; ++v) {
    mavlm_config cv = c;
    cv.batch = v;
    const mavlm_nb_view w = x.view[v] = view_of(plan_of(cv, v == 1));
    mx.gsplit_floats = w.gsplit_floats > mx.gsplit_floats ? w.gsplit_floats : mx.gsplit_floats;
    mx.split_floats = w.split_floats > mx.split_floats ? w.split_floats : mx.split_floats;
    mx.fscr_floats = w.fscr_floats > mx.fscr_floats ? w.fscr_floats : mx.fscr_floats;
    mx.fout_floats = w.fout_floats > mx.fout_floats ? w.fout_floats : mx.fout_floats;
  }
  size_t o = x.total;
  if (mx.split_floats > x.split_floats) { x.o_xsplit = o; o += al(mx.split_floats * 4); }
  if (mx.gsplit_floats > x.gsplit_floats) { x.o_xgsplit = o; o += al(mx.gsplit_floats * 4); }
  if (mx.fscr_floats > x.fscr_floats) { x.o_xfscr = o; o += al(mx.fscr_floats * 4); }
  if (mx.fout_floats > x.fout_floats) { x.o_xfout = o; o += al(mx.fout_floats * 4); }
  // (the exchange scratch of the fused Residual kernel grows with the rows: the own region covers every smaller count)
  // Steps whose videos bring different frame counts (mavlm_step_batch_frames): the column-sum planes of ALL videos of one launch,
  // video after video (o_part holds one video's).  Behind every other region; heads of <= 128 columns only (the wide heads run
  // their column sums video by video through o_part).
  if (!wide_heads(c)) {
    x.vlpart_floats = colsum_floats_max(c) * (size_t)(B < MAVLM_VBASE_MAX ? B : MAVLM_VBASE_MAX);
    x.o_vlpart = o;
    o += al(x.vlpart_floats * 4);
  }
  x.total = o;
  return x;
}

bool maps_supported(const mavlm_config& c) { return shape_ok(&c) && c.patches % 4 == 0; }
size_t maps_floats(const mavlm_config& c) {
  const int Rq1 = q_tokens(c) * c.patches, R1 = c.mem_tokens * c.patches, P = c.patches, H = c.heads;
  const size_t f = mavlm_group_mass_floats(Rq1, c.max_chunk_frames * P, H, P, P) - mavlm_group_mass_out_floats(Rq1, c.max_chunk_frames * P, H, P, P);
  const size_t e = mavlm_group_mass_floats(Rq1, c.cache_cap * R1, H, P, R1) - mavlm_group_mass_out_floats(Rq1, c.cache_cap * R1, H, P, R1);
  return (size_t)nbatch(c) * maps_video_floats(c) + (f > e ? f : e);
}

extern "C" {

int mavlm_abi_version(void) { return MAVLM_ABI_VERSION; }

size_t mavlm_workspace_bytes(const mavlm_config* cfg) { return cfg_ok(cfg) ? mavlm_carve_of(*cfg).total : 0; }

int64_t mavlm_workspace_ln_ctl_offset(const mavlm_config* cfg) {
  if (!cfg_ok(cfg)) return -1;
  const mavlm_carve t = mavlm_carve_of(*cfg);
  return t.lnx_bytes ? (int64_t)t.o_lnx : -1;
}

int64_t mavlm_ln_ctl_offset(const mavlm_ctx* x) { return x ? (x->lnx_bytes ? (int64_t)x->o_lnx : -1) : MAVLM_E_ARG; }

int mavlm_workspace_layout(const mavlm_config* cfg, size_t* offsets, int32_t n) {
  if (!cfg_ok(cfg) || !offsets || n < 10) return MAVLM_E_ARG;
  const mavlm_carve t = mavlm_carve_of(*cfg);
  const size_t o[14] = {t.o_kv, t.o_q, t.o_ctx, t.o_a, t.o_h, t.o_pre, t.o_mA, t.o_mB, t.o_lse, t.o_part,
                        t.o_gsplit, t.gsplit_floats * 4, t.o_kvsplit, t.kvsplit_floats * 4};
  for (int i = 0; i < (n < 14 ? n : 14); ++i) offsets[i] = o[i];
  return 0;
}

int64_t mavlm_attention_maps_floats(const mavlm_config* cfg) {
  return (cfg_ok(cfg) && maps_supported(*cfg)) ? (int64_t)maps_floats(*cfg) : 0;
}

int mavlm_create(const mavlm_config* cfg, mavlm_ctx** out) {
  if (!out || !cfg_ok(cfg)) return MAVLM_E_ARG;
  if (!shape_ok(cfg)) return MAVLM_E_SHAPE;
  mavlm_ctx* x = new (std::nothrow) mavlm_ctx();
  if (!x) return MAVLM_E_ARG;
  x->cfg = *cfg;
  static_cast<mavlm_carve&>(*x) = mavlm_carve_of(*cfg);
  x->nb = nbatch(*cfg);
  *out = x;
  return 0;
}

void mavlm_destroy(mavlm_ctx* ctx) { delete ctx; }

int mavlm_bind_weights(mavlm_ctx* x, const mavlm_weights* w) {
  if (!x || !w) return MAVLM_E_ARG;
  if (!w->mem0 || !w->w_kv_seg || !w->b_kv_seg || !w->w_kv_evo || !w->b_kv_evo) return MAVLM_E_ARG;
  // the fuser / token-type weights live outside TransformerProjector (llava_arch.py:132-150): optional here,
  // required by mavlm_fuse_emit
  const mavlm_attn_weights* e = &w->evo;
  if (!e->wq || !e->bq || !e->wo || !e->bo || !e->ln_g || !e->ln_b) return MAVLM_E_ARG;
  for (int l = 0; l < x->cfg.depth; ++l) {
    const mavlm_attn_weights* a = &w->layer_attn[l];
    if (!a->wq || !a->bq || !a->wo || !a->bo || !a->ln_g || !a->ln_b || !w->w_up[l] || !w->b_up[l] || !w->w_down[l] ||
        !w->b_down[l] || !w->ln2_g[l] || !w->ln2_b[l])
      return MAVLM_E_ARG;
  }
  x->w = *w;
  x->q0_valid = false;                          // (so is the projection of the previous initial memory)
  x->q0_nb = 0;
  x->pre[0].seg = x->pre[1].seg = nullptr;      // K/V projected with the previous weights are not this context's any more
  x->has_w = true;
  return 0;
}

int mavlm_bind_buffers(mavlm_ctx* x, const mavlm_buffers* b) {
  if (!x || !b || !b->mem_ring || !b->evo_kv_ring || !b->workspace) return MAVLM_E_ARG;
  if (b->workspace_bytes < x->total || ((uintptr_t)b->workspace & 255)) return MAVLM_E_ARG;
  x->b = *b;
  x->has_b = true;
  x->q0_valid = false;             // ... and the cached first-step Q lived in the old one
  x->lnx_clean = false;            // a new workspace: its exchange scratch is zero-filled at the first step
  x->pre[0] = x->pre[1] = mavlm_ctx::pre_slot();     // (a prefetched projection lived in the old workspace)
  x->done_rec[0] = x->done_rec[1] = false;
  return 0;
}

int mavlm_bind_attention_maps(mavlm_ctx* x, float* maps, int64_t maps_floats_) {
  if (!x) return MAVLM_E_ARG;
  if (!maps) { x->maps = nullptr; return 0; }
  if (!maps_supported(x->cfg)) return MAVLM_E_SHAPE;
  if (maps_floats_ < (int64_t)maps_floats(x->cfg) || ((uintptr_t)maps & 3)) return MAVLM_E_ARG;
  x->maps = maps;
  return 0;
}

int mavlm_ln_status_async(mavlm_ctx* x, void* host16, int32_t clear, void* stream) {
  if (!x || !host16) return MAVLM_E_ARG;
  if (!x->has_b) return MAVLM_E_STATE;
  if (!x->lnx_bytes || !x->lnx_clean) return 1;       // never fused / nothing launched yet: nothing to report
  hipStream_t s = (hipStream_t)stream;
  MAVLM_TRY(hipMemcpyAsync(host16, ws(x, x->o_lnx), 16, hipMemcpyDeviceToHost, s));
  if (clear) MAVLM_TRY(hipMemsetAsync(ws(x, x->o_lnx) + 8, 0, 4, s));
  return 0;
}

int mavlm_reset(mavlm_ctx* x) {
  if (!x) return MAVLM_E_ARG;
  x->steps = 0;
  x->n_active = 0;
  for (int b = 0; b < MAVLM_MAX_BATCH; ++b) x->vsteps[b] = 0;
  x->nb = nbatch(x->cfg);
  x->pre[0].seg = x->pre[1].seg = nullptr;      // (a projection still in flight keeps its `pending` mark: the next writer waits)
  return 0;
}

int mavlm_prefetch_hits(const mavlm_ctx* x) { return x ? x->pre_hits : MAVLM_E_ARG; }
int mavlm_cache_len(const mavlm_ctx* x) { return x ? (x->steps < x->cfg.cache_cap ? x->steps : x->cfg.cache_cap) : MAVLM_E_ARG; }
int mavlm_newest_slot(const mavlm_ctx* x) { return x ? (x->steps ? (x->steps - 1) % x->cfg.cache_cap : -1) : MAVLM_E_ARG; }
int mavlm_steps(const mavlm_ctx* x) { return x ? x->steps : MAVLM_E_ARG; }
int mavlm_batch(const mavlm_ctx* x) { return x ? nbatch(x->cfg) : MAVLM_E_ARG; }
int mavlm_video_steps(const mavlm_ctx* x, int32_t b) {
  if (!x || b < 0 || b >= nbatch(x->cfg)) return MAVLM_E_ARG;
  return x->vsteps[b];
}

}  // extern "C"
