// Token emit (mavlm_fuse_emit*): the cached memories through the Memory-Fuser MLP into the caller's token blocks, with the
// literal rows (prompts, newlines) and the fine frames of a video token layout around them.
#include "mavlm_ctx.h"

// newline period of a token layout (mavlm.h MAVLM_LAYOUT_*): 0 = no newline inside a block (_ONE: one behind it, _NONE: none),
// else one newline row after every `gap` rows of a block.  <0: MAVLM_E_*.
int layout_gap(const mavlm_config& c, int32_t layout) {
  switch (layout) {
    case MAVLM_LAYOUT_ONE:
    case MAVLM_LAYOUT_NONE: return 0;
    case MAVLM_LAYOUT_FRAME: return c.patches;
    case MAVLM_LAYOUT_GRID: {
      int g = (int)(sqrt((double)c.patches) + 0.5);
      return g > 0 && g * g == c.patches ? g : MAVLM_E_SHAPE;     // (add_token_per_grid views a frame as a square grid, :336-338)
    }
  }
  return MAVLM_E_ARG;
}
// rows a block of `rows` feature rows takes in a layout
int64_t block_rows(int64_t rows, int32_t layout, int gap) {
  return rows + (gap > 0 ? rows / gap : (layout == MAVLM_LAYOUT_ONE ? 1 : 0));
}

namespace {

// What both emit implementations take from the caller besides the videos' features and destinations
struct emit_in {
  const void* const* x_pe; const int64_t* fine_idx;
  const void* mem_prompt; int32_t n_mem_prompt; const void* frame_prompt; int32_t n_frame_prompt; const void* newline;
  int32_t with_frames, layout;
  void* out;
};

// The token block of every video: [memory prompt | memories (+ newlines) | frame prompt | fine frames (+ newlines)].  The memory
// block and the fine-frame block are laid out SEPARATELY (llava_arch.py:585-634 runs per feature).  The equal-length exports
// are the case where every entry is equal.
struct emit_plan {
  int nv = 0, gap = 0;
  int nm[MAVLM_MAX_BATCH], nf[MAVLM_MAX_BATCH];              // cached memories / fine frames of video b
  int64_t r_fine[MAVLM_MAX_BATCH], need[MAVLM_MAX_BATCH];    // first fine-frame row inside the block / rows of the block
  int64_t row0[MAVLM_MAX_BATCH];                             // first row of the block in `out`
  long long base[MAVLM_MAX_BATCH];                           // ... as an element offset (mavlm_gemm_args::c_vbase)
  // how the blocks' places travel to the kernels: a constant stride (elements; the equal-length exports), and / or per-video
  // bases by value (null = the stride alone)
  long long vstride = 0;
  const long long* vbase = nullptr;
  long long fine_ld = 0;                                     // index entries between two videos' rows of fine_idx (0 = shared)
};

bool fuser_weights_bound(const mavlm_ctx* x, int with_frames) {
  return x->w.w_f1 && x->w.b_f1 && x->w.w_f2 && x->w.b_f2_type0 && (!with_frames || x->w.type1);
}

// the argument checks common to both (n_fine: the largest count of any video); sets the plan's gap
int emit_args_check(const mavlm_config& c, const emit_in& in, int32_t n_fine, emit_plan* p) {
  if (in.n_mem_prompt < 0 || in.n_frame_prompt < 0 || n_fine < 0 || (in.n_mem_prompt && !in.mem_prompt) ||
      (in.with_frames && ((in.n_frame_prompt && !in.frame_prompt) || (n_fine && (!in.x_pe || !in.fine_idx)))))
    return MAVLM_E_ARG;
  p->gap = layout_gap(c, in.layout);
  if (p->gap < 0) return p->gap;
  if (in.layout != MAVLM_LAYOUT_NONE && !in.newline) return MAVLM_E_ARG;
  return 0;
}
// the rows the literal-row and fine-frame kernels read and write in 16-byte pieces
inline bool misaligned16(const emit_in& in, const void* extra = nullptr) {
  return (((uintptr_t)in.mem_prompt | (uintptr_t)in.newline | (uintptr_t)in.frame_prompt | (uintptr_t)in.out | (uintptr_t)extra) & 15) != 0;
}

// r_fine / need of every video from its nm / nf
void plan_blocks(const mavlm_config& c, const emit_in& in, emit_plan* p) {
  for (int b = 0; b < p->nv; ++b) {
    const int64_t r_fp = in.n_mem_prompt + block_rows((int64_t)p->nm[b] * c.mem_tokens * c.patches, in.layout, p->gap);
    p->r_fine[b] = r_fp + in.n_frame_prompt;
    p->need[b] = in.with_frames ? p->r_fine[b] + block_rows((int64_t)p->nf[b] * c.patches, in.layout, p->gap) : r_fp;
  }
}

// The destinations, on the host, before the first launch.  dst_row (null: video b's block starts b * vstride into `out`, its
// capacity is the caller's to check): inside the out_rows rows of `out`, pairwise disjoint.  Sets row0 / base.  A row batch at a
// hidden size the 256-column-tile kernels do not take: the fuser's second GEMM maps its rows with 32-bit byte offsets
// (MAVLM_GEMM_MAP_REACH) - a destination that reaches further is refused here.
int emit_dest_check(const mavlm_config& c, emit_plan* p, const int64_t* dst_row, int64_t out_rows) {
  const int D = c.hidden;
  for (int b = 0; b < p->nv; ++b) {
    if (dst_row) {
      if (dst_row[b] < 0 || dst_row[b] > out_rows - p->need[b]) return MAVLM_E_ARG;
      for (int a = 0; a < b; ++a)
        if (dst_row[a] < dst_row[b] + p->need[b] && dst_row[b] < dst_row[a] + p->need[a]) return MAVLM_E_ARG;
    }
    p->row0[b] = dst_row ? dst_row[b] : (int64_t)b * (p->vstride / D);
    p->base[b] = (long long)p->row0[b] * D;
  }
  if (nbatch(c) > 1 && D % 256 != 0)
    for (int b = 0; b < p->nv; ++b)
      if ((double)(p->row0[b] + p->need[b]) * D * 2.0 >= (double)MAVLM_GEMM_MAP_REACH) return MAVLM_E_SHAPE;
  return 0;
}

// The literal rows (memory prompt, newlines of the memory block, frame prompt, newlines of the fine block) of the videos
// b0 .. b0 + n - 1, which have one (memories, fine frames) pair: one launch, rows known up front.  gap > 0: a newline behind every
// `gap` rows, i.e. every gap + 1 output rows.
hipError_t emit_literal_rows(const mavlm_config& c, const emit_in& in, const emit_plan& p, int b0, int n, hipStream_t s) {
  const int gap = p.gap;
  const int64_t feat = (int64_t)p.nm[b0] * c.mem_tokens * c.patches, fine = (int64_t)p.nf[b0] * c.patches;
  const int64_t r_fp = p.r_fine[b0] - in.n_frame_prompt;
  const int nl_mem = (int)(r_fp - in.n_mem_prompt - feat), nl_fine = (int)(block_rows(fine, in.layout, gap) - fine);
  const void* src[4] = {in.mem_prompt, in.newline, in.frame_prompt, in.newline};
  const int cnt[4] = {in.n_mem_prompt, nl_mem, in.with_frames ? in.n_frame_prompt : 0, in.with_frames ? nl_fine : 0};
  const long long dst[4] = {0, in.n_mem_prompt + (gap > 0 ? gap : feat), r_fp, p.r_fine[b0] + (gap > 0 ? gap : fine)};
  const int rep[4] = {0, gap > 0 ? gap + 1 : 0, 0, gap > 0 ? gap + 1 : 0};
  return mavlm_launch_copy_rows(src, cnt, dst, 4, in.out, p.vstride, n, c.hidden, s, rep, p.vbase ? p.vbase + b0 : nullptr);
}

// The fine frames (+ type embedding) of the videos b0 .. b0 + n - 1, which have one fine-frame count: one launch.  With a stride the
// launch starts at the (equal) blocks' first fine row and the blocks' places travel as for the literal rows; without, every video's
// first fine row travels as its base and every video gathers through its own row of fine_idx.
hipError_t emit_fine_frames(mavlm_ctx* x, const emit_in& in, const emit_plan& p, int b0, int n, hipStream_t s) {
  const mavlm_config& c = x->cfg;
  const int D = c.hidden;
  if (p.vstride)
    return mavlm_launch_row_add_batch(in.x_pe + b0, in.fine_idx, x->w.type1, (char*)in.out + (size_t)p.r_fine[b0] * D * 2, p.vstride, n,
                                      p.nf[b0], c.patches, D, c.dtype, s, p.gap, p.vbase ? p.vbase + b0 : nullptr);
  long long fb[MAVLM_VBASE_MAX];
  for (int b = 0; b < n; ++b) fb[b] = p.base[b0 + b] + (long long)p.r_fine[b0 + b] * D;
  return mavlm_launch_row_add_batch(in.x_pe + b0, in.fine_idx + (size_t)b0 * p.fine_ld, x->w.type1, in.out, 0, n, p.nf[b0], c.patches, D,
                                    c.dtype, s, p.gap, fb, p.fine_ld);
}

// The equal-length exports: every video of the context has made every step.  cap_rows: rows between two videos' blocks, or - with
// dst_row (mavlm_fuse_emit_layout_batch_to) - the rows of `out`, video b's block starting at row dst_row[b].
int fuse_emit_impl(mavlm_ctx* x, const emit_in& in, int32_t n_fine, int64_t cap_rows, int64_t* rows, hipStream_t s,
                   const int64_t* dst_row = nullptr) {
  if (!fuser_weights_bound(x, in.with_frames)) return MAVLM_E_STATE;
  emit_plan p;
  { const int rc = emit_args_check(x->cfg, in, n_fine, &p); if (rc) return rc; }
  const mavlm_config& c = x->cfg;
  const int gap = p.gap;
  const int B = nbatch(c), R1 = c.mem_tokens * c.patches, R = R1 * B, D = c.hidden, I = c.inter, dt = c.dtype, cap = c.cache_cap;
  const int n = x->steps < cap ? x->steps : cap;
  if (n == 0) return MAVLM_E_STATE;
  for (int b = 0; b < B; ++b)       // (a ragged row batch - videos with fewer steps - emits through mavlm_fuse_emit_layout_ragged_to)
    if (x->vsteps[b] != x->steps) return MAVLM_E_STATE;
  p.nv = B;
  for (int b = 0; b < B; ++b) { p.nm[b] = n; p.nf[b] = n_fine; }
  plan_blocks(c, in, &p);
  const int64_t need = p.need[0];
  if (cap_rows < need) return MAVLM_E_ARG;
  if (dst_row && B > MAVLM_VBASE_MAX) return MAVLM_E_ARG;      // the bases go to the kernels by value
  p.vstride = (long long)cap_rows * D;
  { const int rc = emit_dest_check(c, &p, dst_row, cap_rows); if (rc) return rc; }
  if (dst_row) p.vbase = p.base;
  if (in.with_frames && n_fine)
    for (int b = 0; b < B; ++b)
      if (!in.x_pe[b]) return MAVLM_E_ARG;
  if (misaligned16(in)) return MAVLM_E_ARG;
  const size_t rowb = (size_t)D * 2;
  MAVLM_TRY(emit_literal_rows(c, in, p, 0, B, s));
  const int oldest = x->steps <= cap ? 0 : x->steps % cap;
  // torch.cat(memory_cache) order = oldest first (llava_arch.py:545) = ring slots oldest..cap-1, then 0..oldest-1: at most
  // two contiguous slot ranges, each fused in batches of up to fuse_mems memories per GEMM pair (llava_arch.py:546).  A
  // slot holds the memories of all B videos ([B, R1, D]): the second GEMM writes block b of a slot into video b's tokens.
  for (int done = 0; done < n;) {
    const int slot = (oldest + done) % cap;
    int run = n - done < cap - slot ? n - done : cap - slot;
    if (run > x->fuse_mems) run = x->fuse_mems;
    const int rows_ = run * R;
    const char* mem = (const char*)x->b.mem_ring + (size_t)slot * R * rowb;
    MAVLM_TRY(gemm_x(x, s, mem, D, x->w.w_f1, D, x->w.b_f1, ws(x, x->o_h), I, rows_, I, D, MAVLM_EPI_GELU));
    // first row of this launch inside a video's block (done * R1 is a multiple of the gap: whole frames)
    const int64_t v0 = (int64_t)done * R1;
    char* dstp = (char*)in.out + (size_t)(in.n_mem_prompt + v0 + (gap > 0 ? v0 / gap : 0)) * rowb;
    mavlm_gemm_args g = fuser_out_gemm(c, rows_, dstp, x->gsplit_floats ? (float*)ws(x, x->o_gsplit) : nullptr, x->gsplit_floats);
    g.A = ws(x, x->o_h); g.W = x->w.w_f2; g.bias = x->w.b_f2_type0;
    if (B > 1) {
      g.splitk_ws = nullptr;
      g.c_rpb = R1; g.c_nb = B; g.c_bstride = p.vstride;
      g.c_vbase = p.vbase;
    }
    if (gap > 0 && !mavlm_gemm_row_map_ok(g)) {
      // the writer this shape takes has no row map (128^2 kernel / split-K reduce; single videos on small grids): the same
      // launch into the scratch, then one copy places the rows
      if ((size_t)rows_ * rowb > x->stage_bytes) return MAVLM_E_STATE;      // (a tuning hook changed the dispatch after mavlm_create)
      g.C = ws(x, x->o_stage);
      MAVLM_TRY(mavlm_launch_gemm(g, dt, s));
      MAVLM_TRY(mavlm_launch_spread_rows(g.C, dstp, rows_, D, gap, s));
    } else {
      g.c_gap = gap;
      MAVLM_TRY(mavlm_launch_gemm(g, dt, s));
    }
    done += run;
  }
  if (in.with_frames && n_fine) MAVLM_TRY(emit_fine_frames(x, in, p, 0, B, s));
  *rows = need;
  return 0;
}

// mavlm_fuse_emit_layout_ragged_to.  Videos 0 .. nv-1 in the context's longest-first order: vsteps is non-increasing, so the
// videos that hold a ring slot, and the videos with one block length, are ranges that start at video 0 / are contiguous.
// n_fine_v (mavlm_fuse_emit_layout_frames_to; null = every video has n_fine fine frames and fine_ld = n_fine): video b has
// n_fine_v[b] fine frames, its index row starts b * fine_ld entries into fine_idx.  The literal rows and the fine frames then
// run per range of consecutive videos with one (memories, fine frames) pair - with a constant count the same launches as before.
int ragged_emit_impl(mavlm_ctx* x, int nv, const emit_in& in, int32_t n_fine, int64_t out_rows, const int64_t* dst_row, int64_t* rows,
                     hipStream_t s, const int32_t* n_fine_v = nullptr, int64_t fine_ld = 0) {
  const mavlm_config& c = x->cfg;
  const int Bc = nbatch(c), R1 = c.mem_tokens * c.patches, D = c.hidden, I = c.inter, dt = c.dtype, cap = c.cache_cap;
  if (nv < 1 || nv > Bc || nv > MAVLM_VBASE_MAX) return MAVLM_E_ARG;
  emit_plan p;
  p.nv = nv;
  for (int b = 0; b < nv; ++b) {
    p.nf[b] = n_fine_v ? n_fine_v[b] : n_fine;
    if (p.nf[b] < 0 || (n_fine_v && p.nf[b] > fine_ld)) return MAVLM_E_ARG;
    if (p.nf[b] > n_fine) n_fine = p.nf[b];                          // (from here on: the largest count)
  }
  p.fine_ld = n_fine_v ? fine_ld : n_fine;
  // (the per-video fine-frame counts stay with the row map of the 256-column-tile kernels: this export says so up front - the
  // equal-count exports also run at hidden sizes that are multiples of 128 only, on the row-mapped form of the 128^2 kernel)
  if (n_fine_v && D % 256 != 0) return MAVLM_E_SHAPE;
  { const int rc = emit_args_check(c, in, n_fine, &p); if (rc) return rc; }
  const int gap = p.gap;
  if (misaligned16(in, in.fine_idx) || (D & 7)) return MAVLM_E_ARG;
  for (int b = 0; b < nv; ++b) p.nm[b] = x->vsteps[b] < cap ? x->vsteps[b] : cap;
  plan_blocks(c, in, &p);
  { const int rc = emit_dest_check(c, &p, dst_row, out_rows); if (rc) return rc; }
  p.vbase = p.base;             // (no stride: the blocks' first rows travel as per-video bases)
  if (!x->has_w || !x->has_b) return MAVLM_E_STATE;
  if (!fuser_weights_bound(x, in.with_frames)) return MAVLM_E_STATE;
  for (int b = 0; b < nv; ++b) {
    if (p.nm[b] == 0 || (b > 0 && x->vsteps[b] > x->vsteps[b - 1])) return MAVLM_E_STATE;
    if (in.with_frames && p.nf[b] && !in.x_pe[b]) return MAVLM_E_ARG;
  }
  const size_t rowb = (size_t)D * 2;
  // ---- the literal rows: one launch per range of videos with the same number of memories and fine frames (the rows of
  // copy_rows_kernel's runs are the same for all of them)
  for (int b0 = 0; b0 < nv;) {
    int b1 = b0 + 1;
    while (b1 < nv && p.nm[b1] == p.nm[b0] && p.nf[b1] == p.nf[b0]) ++b1;
    MAVLM_TRY(emit_literal_rows(c, in, p, b0, b1 - b0, s));
    b0 = b1;
  }
  // ---- the fused memories, per ring slot: the videos that hold slot `sl` are 0 .. h-1; video b has it as the p-th memory of its
  // block.  Consecutive slots that all Bc videos hold at consecutive places share a GEMM pair, as in fuse_emit_impl (their
  // rows are contiguous in the ring then); a slot of fewer videos runs alone over its first h * R1 rows.
  auto holders = [&](int sl) { int h = 0; while (h < nv && sl < p.nm[h]) ++h; return h; };
  auto place = [&](int b, int sl) { return x->vsteps[b] <= cap ? sl : (sl - x->vsteps[b] % cap + cap) % cap; };
  const int nb_keep = x->nb;
  for (int sl = 0; sl < cap;) {
    const int h = holders(sl);
    if (h == 0) break;
    int run = 1;
    while (h == Bc && run < x->fuse_mems && sl + run < cap && holders(sl + run) == Bc) {
      bool next = true;
      for (int b = 0; b < h && next; ++b) next = place(b, sl + run) == place(b, sl) + run;
      if (!next) break;
      ++run;
    }
    const int rows_ = run * h * R1;
    long long vb[MAVLM_VBASE_MAX];
    for (int b = 0; b < h; ++b) {
      const int64_t v0 = (int64_t)place(b, sl) * R1;                 // (a multiple of the gap: whole frames)
      vb[b] = p.base[b] + (long long)(in.n_mem_prompt + v0 + (gap > 0 ? v0 / gap : 0)) * D;
    }
    const char* mem = (const char*)x->b.mem_ring + (size_t)sl * Bc * R1 * rowb;
    x->nb = h;                  // (the plan of a context of h videos: gemm_x, as mavlm_fuse_emit_layout_batch_to there)
    const hipError_t e1 = gemm_x(x, s, mem, D, x->w.w_f1, D, x->w.b_f1, ws(x, x->o_h), I, rows_, I, D, MAVLM_EPI_GELU);
    x->nb = nb_keep;
    MAVLM_TRY(e1);
    mavlm_gemm_args g = fuser_out_gemm(c, rows_, in.out, nullptr, 0);
    g.A = ws(x, x->o_h); g.W = x->w.w_f2; g.bias = x->w.b_f2_type0;
    g.c_rpb = R1; g.c_nb = h; g.c_bstride = 0; g.c_vbase = vb; g.c_gap = gap;
    MAVLM_TRY(mavlm_launch_gemm(g, dt, s));
    sl += run;
  }
  if (in.with_frames && n_fine)
    for (int b0 = 0; b0 < nv;) {            // (one launch per range of videos with one fine-frame count: all of them, when it is constant)
      int b1 = b0 + 1;
      while (b1 < nv && p.nf[b1] == p.nf[b0]) ++b1;
      MAVLM_TRY(emit_fine_frames(x, in, p, b0, b1 - b0, s));
      b0 = b1;
    }
  for (int b = 0; b < nv; ++b) rows[b] = p.need[b];
  return 0;
}

}  // namespace

extern "C" {

int mavlm_fuse_emit_layout(mavlm_ctx* x, const void* x_pe, const int64_t* fine_idx, int32_t n_fine, const void* mem_prompt,
                           int32_t n_mem_prompt, const void* frame_prompt, int32_t n_frame_prompt, const void* newline,
                           int32_t with_frames, int32_t layout, void* out, int64_t cap_rows, int64_t* rows, void* stream) {
  if (!x || !out || !rows) return MAVLM_E_ARG;
  if (!x->has_w || !x->has_b) return MAVLM_E_STATE;
  if (nbatch(x->cfg) != 1) return MAVLM_E_STATE;
  const emit_in in = {x_pe ? &x_pe : nullptr, fine_idx, mem_prompt, n_mem_prompt, frame_prompt, n_frame_prompt, newline, with_frames, layout, out};
  return fuse_emit_impl(x, in, n_fine, cap_rows, rows, (hipStream_t)stream);
}

int mavlm_fuse_emit_layout_batch(mavlm_ctx* x, const void* const* x_pe, const int64_t* fine_idx, int32_t n_fine,
                                 const void* mem_prompt, int32_t n_mem_prompt, const void* frame_prompt, int32_t n_frame_prompt,
                                 const void* newline, int32_t with_frames, int32_t layout, void* out, int64_t rows_per_video,
                                 int64_t* rows, void* stream) {
  if (!x || !out || !rows) return MAVLM_E_ARG;
  if (!x->has_w || !x->has_b) return MAVLM_E_STATE;
  const emit_in in = {x_pe, fine_idx, mem_prompt, n_mem_prompt, frame_prompt, n_frame_prompt, newline, with_frames, layout, out};
  return fuse_emit_impl(x, in, n_fine, rows_per_video, rows, (hipStream_t)stream);
}

int mavlm_fuse_emit_layout_batch_to(mavlm_ctx* x, const void* const* x_pe, const int64_t* fine_idx, int32_t n_fine,
                                    const void* mem_prompt, int32_t n_mem_prompt, const void* frame_prompt, int32_t n_frame_prompt,
                                    const void* newline, int32_t with_frames, int32_t layout, void* out, int64_t out_rows,
                                    const int64_t* dst_row, int64_t* rows, void* stream) {
  if (!x || !out || !rows || !dst_row || out_rows < 0) return MAVLM_E_ARG;
  if (!x->has_w || !x->has_b) return MAVLM_E_STATE;
  if (nbatch(x->cfg) < 2) return MAVLM_E_STATE;             // (a single video: mavlm_fuse_emit_layout writes where `out` points)
  const emit_in in = {x_pe, fine_idx, mem_prompt, n_mem_prompt, frame_prompt, n_frame_prompt, newline, with_frames, layout, out};
  return fuse_emit_impl(x, in, n_fine, out_rows, rows, (hipStream_t)stream, dst_row);
}

int mavlm_fuse_emit_layout_ragged_to(mavlm_ctx* x, int32_t n_videos, const void* const* x_pe, const int64_t* fine_idx,
                                     int32_t n_fine, const void* mem_prompt, int32_t n_mem_prompt, const void* frame_prompt,
                                     int32_t n_frame_prompt, const void* newline, int32_t with_frames, int32_t layout, void* out,
                                     int64_t out_rows, const int64_t* dst_row, int64_t* rows, void* stream) {
  if (!x || !out || !rows || !dst_row || out_rows < 0) return MAVLM_E_ARG;
  if (nbatch(x->cfg) < 2) return MAVLM_E_STATE;
  const emit_in in = {x_pe, fine_idx, mem_prompt, n_mem_prompt, frame_prompt, n_frame_prompt, newline, with_frames, layout, out};
  return ragged_emit_impl(x, n_videos, in, n_fine, out_rows, dst_row, rows, (hipStream_t)stream);
}

int mavlm_fuse_emit_layout_frames_to(mavlm_ctx* x, int32_t n_videos, const void* const* x_pe, const int64_t* fine_idx,
                                     int64_t fine_ld, const int32_t* n_fine, const void* mem_prompt, int32_t n_mem_prompt,
                                     const void* frame_prompt, int32_t n_frame_prompt, const void* newline, int32_t with_frames,
                                     int32_t layout, void* out, int64_t out_rows, const int64_t* dst_row, int64_t* rows,
                                     void* stream) {
  if (!x || !out || !rows || !dst_row || !n_fine || out_rows < 0 || fine_ld < 0) return MAVLM_E_ARG;
  if (nbatch(x->cfg) < 2) return MAVLM_E_STATE;
  const emit_in in = {x_pe, fine_idx, mem_prompt, n_mem_prompt, frame_prompt, n_frame_prompt, newline, with_frames, layout, out};
  return ragged_emit_impl(x, n_videos, in, 0, out_rows, dst_row, rows, (hipStream_t)stream, n_fine, fine_ld);
}

int mavlm_fuse_emit(mavlm_ctx* x, const void* x_pe, const int64_t* fine_idx, int32_t n_fine, const void* mem_prompt,
                    int32_t n_mem_prompt, const void* frame_prompt, int32_t n_frame_prompt, const void* newline,
                    int32_t with_frames, void* out, int64_t cap_rows, int64_t* rows, void* stream) {
  if (!newline) return MAVLM_E_ARG;
  return mavlm_fuse_emit_layout(x, x_pe, fine_idx, n_fine, mem_prompt, n_mem_prompt, frame_prompt, n_frame_prompt, newline, with_frames,
                                MAVLM_LAYOUT_ONE, out, cap_rows, rows, stream);
}

int mavlm_fuse_emit_batch(mavlm_ctx* x, const void* const* x_pe, const int64_t* fine_idx, int32_t n_fine, const void* mem_prompt,
                          int32_t n_mem_prompt, const void* frame_prompt, int32_t n_frame_prompt, const void* newline,
                          int32_t with_frames, void* out, int64_t rows_per_video, int64_t* rows, void* stream) {
  if (!newline) return MAVLM_E_ARG;
  return mavlm_fuse_emit_layout_batch(x, x_pe, fine_idx, n_fine, mem_prompt, n_mem_prompt, frame_prompt, n_frame_prompt, newline,
                                      with_frames, MAVLM_LAYOUT_ONE, out, rows_per_video, rows, stream);
}

int64_t mavlm_layout_rows(const mavlm_config* cfg, int32_t n_memories, int32_t n_fine, int32_t n_mem_prompt, int32_t n_frame_prompt,
                          int32_t with_frames, int32_t layout) {
  if (!cfg_ok(cfg) || n_memories < 0 || n_fine < 0 || n_mem_prompt < 0 || n_frame_prompt < 0) return MAVLM_E_ARG;
  const int gap = layout_gap(*cfg, layout);
  if (gap < 0) return gap;
  int64_t r = n_mem_prompt + block_rows((int64_t)n_memories * cfg->mem_tokens * cfg->patches, layout, gap);
  if (with_frames) r += n_frame_prompt + block_rows((int64_t)n_fine * cfg->patches, layout, gap);
  return r;
}

}  // extern "C"
