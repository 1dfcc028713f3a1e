// Tuning hooks (mavlm_set_*) and the stand-alone operator exports: one kernel family each, arguments checked before the launch.
// Unless an export says otherwise, a launcher's refusal of its arguments comes back as MAVLM_E_ARG (api_rc).
#include "mavlm_ctx.h"

mavlm_gemm_args gemm_args(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res, int ldr, void* C,
                          int ldc, int M, int N, int K, int epi) {
  mavlm_gemm_args g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.res = res; g.ldr = ldr; g.C = C; g.ldc = ldc;
  g.M = M; g.N = N; g.K = K; g.epilogue = epi;
  return g;
}

hipError_t gemm(int dtype, hipStream_t s, const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc,
                int M, int N, int K, int epi, const void* res, int ldr, float* split_ws, size_t split_floats) {
  mavlm_gemm_args g = gemm_args(A, lda, W, ldw, bias, res, ldr, C, ldc, M, N, K, epi);
  // split-K only when the caller's workspace covers this shape's plan (the plan is part of the result)
  if (split_ws != nullptr && mavlm_gemm_split_ws_floats(M, N, K, epi, ldc) <= split_floats) g.splitk_ws = split_ws;
  return mavlm_launch_gemm(g, dtype, s);
}

mavlm_attn_args attn_args(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, float* lse2,
                          int R, int S, int H, float scale) {
  mavlm_attn_args a;
  a.Q = Q; a.ldq = ldq; a.K = K; a.ldk = ldk; a.V = V; a.ldv = ldv; a.O = O; a.ldo = ldo; a.lse2 = lse2;
  a.R = R; a.S = S; a.H = H; a.scale = scale;
  return a;
}

mavlm_colsum_args colsum_args(const void* Q, int ldq, const void* K, int ldk, const float* lse2, float* part, int R, int S, int H,
                              float scale) {
  mavlm_colsum_args a;
  a.Q = Q; a.ldq = ldq; a.K = K; a.ldk = ldk; a.lse2 = lse2; a.part = part; a.R = R; a.S = S; a.H = H; a.scale = scale;
  return a;
}

namespace {

struct bwd_abi {   // the operands every attention-backward export takes
  const void* Q; int32_t ldq; const void* K; int32_t ldk; const void* V; int32_t ldv; const void* O; int32_t ldo;
  const void* dO; int32_t lddo; const float* lse2; float* delta; void* dQ; int32_t lddq; void* dK; int32_t lddk; void* dV; int32_t lddv;
};
// pointers, strides (w = columns of one video's heads) and the 16-byte alignment of the inputs
int bwd_abi_check(const bwd_abi& p, int w) {
  if ((p.ldq & 7) || (p.ldk & 7) || (p.ldv & 7) || (p.ldo & 7) || (p.lddo & 7) || (p.lddq & 3) || (p.lddk & 3) || (p.lddv & 3))
    return MAVLM_E_ARG;
  if (p.ldq < w || p.ldk < w || p.ldv < w || p.ldo < w || p.lddo < w || (p.dQ && p.lddq < w) || (p.dK && p.lddk < w) || (p.dV && p.lddv < w))
    return MAVLM_E_ARG;
  if (((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.V | (uintptr_t)p.O | (uintptr_t)p.dO) & 15) return MAVLM_E_ARG;
  return 0;
}
inline bool bwd_abi_null(const bwd_abi& p) { return !p.Q || !p.K || !p.V || !p.O || !p.dO || !p.lse2 || !p.delta; }
mavlm_attn_bwd_args attn_bwd_args(const bwd_abi& p, int R, int S, int H, float scale) {
  mavlm_attn_bwd_args a;
  a.Q = p.Q; a.ldq = p.ldq; a.K = p.K; a.ldk = p.ldk; a.V = p.V; a.ldv = p.ldv; a.O = p.O; a.ldo = p.ldo; a.dO = p.dO; a.lddo = p.lddo;
  a.lse2 = p.lse2; a.delta = p.delta; a.dQ = p.dQ; a.lddq = p.lddq; a.dK = p.dK; a.lddk = p.lddk; a.dV = p.dV; a.lddv = p.lddv;
  a.R = R; a.S = S; a.H = H; a.scale = scale;
  return a;
}
// launch under the profile scope of the backward (algorithmic flops: 3 products for dQ, 3 for dK, 2 for dV; the head_dim-448
// kernels run 5 / 5 / 2 - attention_bwd_hd.hip); hw = columns of a head
int attn_bwd_launch(const mavlm_attn_bwd_args& a, int hw, int dtype, void* stream) {
  const double units = (a.dQ ? 3.0 : 0.0) + (a.dK ? 3.0 : 0.0) + (a.dV ? 2.0 : 0.0);
  mavlm_prof_scope prof(MAVLM_K_ATTN_BWD, units * 2.0 * a.R * (double)a.S * a.H * hw, 2.0 * hw * a.H * (4.0 * a.R + 4.0 * a.S),
                        (hipStream_t)stream);
  return api_rc(hw == 128 ? mavlm_launch_attention_bwd(a, dtype, (hipStream_t)stream)
                          : mavlm_launch_attention_bwd_hd(a, hw, dtype, (hipStream_t)stream));
}

int batch_args_bad(int32_t H, int32_t nb) { return nb < 1 || nb > MAVLM_MAX_BATCH || H <= 0 || H % nb != 0; }

// per-video key ranges of a variable-length row batch: counts, alignment, pairwise disjoint [off, off + S * ld)
int varlen_ranges_bad(const int32_t* S, const int64_t* off, int32_t nb, int64_t ld) {
  if (!S || !off || nb < 1 || nb > MAVLM_VBASE_MAX) return 1;
  for (int b = 0; b < nb; ++b) {
    if (S[b] < 1 || off[b] < 0 || (off[b] & 7)) return 1;
    for (int a = 0; a < b; ++a)
      if (off[a] < off[b] + (int64_t)S[b] * ld && off[b] < off[a] + (int64_t)S[a] * ld) return 1;
  }
  return 0;
}

// mavlm_linear / mavlm_linear_ws: ws_ null = never split the contraction
int linear_impl(const void* A, int32_t lda, const void* W, int32_t ldw, const float* bias, const void* res, int32_t ldr, void* C,
                int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t epilogue, bool with_ws, float* ws_, int64_t ws_floats,
                int32_t dtype, void* stream) {
  if (!A || !W || !bias || !C || M < 0) return MAVLM_E_ARG;
  if (N % 128 || K % 64 || N <= 0 || K <= 0) return MAVLM_E_SHAPE;
  const int64_t need = with_ws ? (int64_t)mavlm_gemm_split_ws_floats(M, N, K, epilogue, ldc) : 0;
  if (need > 0 && (!ws_ || ws_floats < need)) return MAVLM_E_ARG;      // the plan is part of the result
  return api_rc(gemm(dtype, (hipStream_t)stream, A, lda, W, ldw, bias, C, ldc, M, N, K, epilogue, res, ldr,
                     need > 0 ? ws_ : nullptr, need > 0 ? (size_t)ws_floats : 0));
}

// mavlm_attention_hd / mavlm_attention_hd_ws.  Returns the launcher's hipError_t as it is (no MAVLM_E_ARG mapping): the
// established behaviour of these two exports.
int attention_hd_impl(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, void* O, int32_t ldo,
                      float* lse2, int32_t R, int32_t S, int32_t H, int32_t head_dim, float scale, bool with_ws, float* ws_,
                      int64_t ws_floats, int32_t dtype, void* stream) {
  if (!Q || !K || !V || !O || R <= 0 || S <= 0 || H <= 0 || (ldq & 7) || (ldk & 7) || (ldv & 7) || (ldo & 3) ||
      ldq < H * head_dim || ldk < head_dim || ldv < head_dim)
    return MAVLM_E_ARG;
  if (head_dim != 448 && head_dim != 128 && head_dim != 256 && head_dim != 224) return MAVLM_E_SHAPE;
  const int64_t need = with_ws ? (int64_t)mavlm_attention_hd_split_ws_floats(R, S, H, head_dim) : 0;
  if (need > 0 && (!ws_ || ws_floats < need)) return MAVLM_E_ARG;        // the plan is part of the result
  mavlm_attn_args a = attn_args(Q, ldq, K, ldk, V, ldv, O, ldo, lse2, R, S, H, scale);
  a.split_ws = need > 0 ? ws_ : nullptr;
  return (int)mavlm_launch_attention_hd(a, head_dim, dtype, (hipStream_t)stream);
}

}  // namespace

extern "C" {

// ---- tuning hooks: process-wide, read at the next launch (mavlm.h says what each one selects) --------------------------------
static int set_hook(int* hook, int32_t v, bool ok) {
  if (!ok) return MAVLM_E_ARG;
  *hook = v;
  return 0;
}
int mavlm_set_attention_impl(int32_t impl) { return set_hook(&g_mavlm_attn_impl, impl, impl == 0 || impl == 2 || impl == 3); }
int mavlm_set_attention_bwd_fused(int32_t on) { return set_hook(&g_mavlm_attn_bwd_fused, on ? 1 : 0, true); }
int mavlm_set_gemm_tile(int32_t tile) {
  return set_hook(&g_mavlm_gemm_tile, tile, tile == 0 || tile == 128 || tile == 129 || tile == 256 || tile == 257);
}
int mavlm_set_attention_unit_order(int32_t affine) { return set_hook(&g_mavlm_attn_unit_order, affine, affine == 0 || affine == 1); }
int mavlm_set_attention_streamk_min_tiles(int32_t tiles) { return set_hook(&g_mavlm_attn_sk_min_tiles, tiles, tiles >= 1); }
int mavlm_set_attention_streamk_waves(int32_t waves) { return set_hook(&g_mavlm_attn_sk_waves, waves, waves == 0 || waves == 4 || waves == 8); }
int mavlm_set_attention_colsum_wgs(int32_t wgs) { return set_hook(&g_mavlm_colsum_wgs, wgs, wgs == 0 || (wgs >= 64 && wgs <= 1024)); }
int mavlm_set_attention_wide_groups(int32_t groups) { return set_hook(&g_mavlm_attn_hd_qg, groups, groups >= 0 && groups <= 2); }
int mavlm_set_attention_hd_varlen(int32_t on) { return set_hook(&g_mavlm_attn_hd_varlen, on, on == 0 || on == 1); }
// (2: diagnostics - the tile-entry form wherever it is supported)
int mavlm_set_frame_score_mode(int32_t mode) { return set_hook(&g_mavlm_frame_score_mode, mode, mode >= 0 && mode <= 2); }
int mavlm_set_gemm_short_splits(int32_t splits) { return set_hook(&g_mavlm_gemm_f32_short_splits, splits, splits >= 1 && splits <= 8); }
int mavlm_set_frame_entries_lds(int32_t on) { return set_hook(&g_mavlm_frame_entries_lds, on, on == 0 || on == 1); }
int mavlm_set_cache_initial_q(int32_t on) { return set_hook(&g_mavlm_cache_q0, on, on == 0 || on == 1); }
int mavlm_set_splitk_layernorm(int32_t on) { return set_hook(&g_mavlm_splitk_ln, on, on == 0 || on == 1); }
int mavlm_set_fused_layernorm(int32_t on) {
  if (on < 0 || on > 2) return MAVLM_E_ARG;
  g_mavlm_fused_ln = on ? 1 : 0;
  g_mavlm_gemm_ln_wide = on == 2 ? 1 : 0;
  return 0;
}
int mavlm_set_gemm_order(int32_t order) { return set_hook(&g_mavlm_gemm_order, order, order == 0 || order == 1); }
int mavlm_set_gemm_rows(int32_t rows) { return set_hook(&g_mavlm_gemm_rows, rows, rows == 0 || rows == 224 || rows == 256); }

// ---- GEMM and LayerNorm --------------------------------------------------------------------------------------------------
int mavlm_linear(const void* A, int32_t lda, const void* W, int32_t ldw, const float* bias, const void* res, int32_t ldr,
                 void* C, int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t dtype, void* stream) {
  return linear_impl(A, lda, W, ldw, bias, res, ldr, C, ldc, M, N, K, epilogue, false, nullptr, 0, dtype, stream);
}

int64_t mavlm_linear_ws_floats(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t ldc) {
  return (int64_t)mavlm_gemm_split_ws_floats(M, N, K, epilogue, ldc);
}

int mavlm_linear_ws(const void* A, int32_t lda, const void* W, int32_t ldw, const float* bias, const void* res, int32_t ldr,
                    void* C, int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t epilogue, float* ws_, int64_t ws_floats,
                    int32_t dtype, void* stream) {
  return linear_impl(A, lda, W, ldw, bias, res, ldr, C, ldc, M, N, K, epilogue, true, ws_, ws_floats, dtype, stream);
}

int64_t mavlm_linear_ln_ws_bytes(int32_t M, int32_t N, int32_t K) {
  return (g_mavlm_fused_ln && mavlm_gemm_ln_supported(M, N, K, -1)) ? (int64_t)mavlm_gemm_ln_ws_bytes(M, N) : 0;
}

int mavlm_linear_ln(const void* A, int32_t lda, const void* W, int32_t ldw, const float* bias, const void* res, int32_t ldr,
                    const float* gamma, const float* beta, float eps, void* out, int32_t ldo, float* pre_out, int32_t M,
                    int32_t N, int32_t K, void* ws_, int64_t ws_bytes, int32_t dtype, void* stream) {
  if (!A || !W || !bias || !res || !gamma || !beta || !out || M < 0) return MAVLM_E_ARG;
  const int64_t need = mavlm_linear_ln_ws_bytes(M, N, K);
  if (need == 0) return MAVLM_E_SHAPE;
  if (!ws_ || ws_bytes < need || ((uintptr_t)ws_ & 15)) return MAVLM_E_ARG;
  mavlm_gemm_args g = gemm_args(A, lda, W, ldw, bias, res, ldr, out, ldo, M, N, K, MAVLM_EPI_LN);
  g.ln.gamma = gamma; g.ln.beta = beta; g.ln.eps = eps; g.ln.pre_out = pre_out;
  g.ln.ctl = (unsigned*)ws_;                               // control words first: a fixed place for every shape
  g.ln.gran = (unsigned long long*)((char*)ws_ + 64);
  return api_rc(mavlm_launch_gemm(g, dtype, (hipStream_t)stream));
}

int mavlm_linear_splitk(const void* A, int32_t lda, const void* W, int32_t ldw, void* C, int32_t M, int32_t N, int32_t K,
                        int32_t splits, float* ws, const float* zero_bias, int32_t dtype, void* stream) {
  if (!A || !W || !C || !ws || !zero_bias || M < 0 || splits < 1) return MAVLM_E_ARG;
  if (N % 128 || K % 64 || N <= 0 || K <= 0) return MAVLM_E_SHAPE;
  const mavlm_gemm_args g = gemm_args(A, lda, W, ldw, zero_bias, nullptr, 0, C, N, M, N, K, MAVLM_EPI_F32);
  return api_rc(mavlm_launch_gemm_splitk(g, splits, ws, zero_bias, dtype, (hipStream_t)stream));
}

int mavlm_layernorm(const float* xin, const void* res, int32_t ldr, const float* gamma, const float* beta, void* out,
                    int32_t rows, int32_t D, float eps, int32_t dtype, void* stream) {
  return api_rc(mavlm_launch_layernorm(xin, res, ldr, gamma, beta, out, rows, D, eps, dtype, (hipStream_t)stream));
}

int mavlm_layernorm_form(int32_t D, int32_t ldr) { return mavlm_layernorm_form_of(D, ldr); }

// ---- attention forward -------------------------------------------------------------------------------------------------
int mavlm_frame_scores_fused(int32_t R, int32_t S, int32_t H, int32_t patches) {
  // not for the small grids that split their keys (few query blocks x heads, e.g. 8 memory tokens): the frame masses ride on
  // the never-split grid, which would leave most of the chip idle there - those shapes keep the column-sum pass
  return (g_mavlm_frame_score_mode == 1 && g_mavlm_attn_impl != 2 && R > 0 && H > 0 &&
          mavlm_attention_frames_supported(R, S, H, patches) && mavlm_attention_splits(R, S, H, nullptr) <= 1) ? 1 : 0;
}

int mavlm_attention(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, void* O,
                    int32_t ldo, float* lse2, int32_t R, int32_t S, int32_t H, float scale, int32_t dtype, void* stream) {
  return api_rc(mavlm_launch_attention(attn_args(Q, ldq, K, ldk, V, ldv, O, ldo, lse2, R, S, H, scale), dtype, (hipStream_t)stream));
}

int64_t mavlm_attention_frames_ws_floats(int32_t R, int32_t S, int32_t H, int32_t patches) {
  if (R <= 0 || H <= 0 || !mavlm_attention_frames_supported(R, S, H, patches)) return 0;
  // [entries | partial frame sums | partials of the stream-K schedule, when this shape runs it]
  const size_t sk = mavlm_attention_streamk_wgs(R, S, H) > 0 ? mavlm_attention_split_ws_floats(R, S, H) : 0;
  return (int64_t)(mavlm_attention_frames_scr_floats(R, S, H, patches) + mavlm_attention_frames_out_floats(R, S, H, patches) + sk);
}

int mavlm_attention_frames(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, void* O,
                           int32_t ldo, float* lse2, int32_t R, int32_t S, int32_t H, float scale, int32_t patches,
                           float* ws_, int64_t ws_floats, float* frame_scores, int32_t dtype, void* stream) {
  const int64_t need = mavlm_attention_frames_ws_floats(R, S, H, patches);
  if (!Q || !K || !V || !O || !frame_scores || need == 0 || !ws_ || ws_floats < need) return MAVLM_E_ARG;
  mavlm_attn_args a = attn_args(Q, ldq, K, ldk, V, ldv, O, ldo, lse2, R, S, H, scale);
  a.frame_scr = ws_;
  a.frame_out = ws_ + mavlm_attention_frames_scr_floats(R, S, H, patches);
  a.frame_keys = patches;
  if (mavlm_attention_streamk_wgs(R, S, H) > 0)
    a.split_ws = a.frame_out + mavlm_attention_frames_out_floats(R, S, H, patches);
  const int frows = mavlm_attention_frames_rows_per_video(a);
  hipError_t e = mavlm_launch_attention3_frames(a, dtype, (hipStream_t)stream);
  if (e == hipSuccess)
    e = mavlm_launch_frame_finish(a.frame_out, frows, 1, S / patches, patches, frame_scores, 1, dtype, (hipStream_t)stream);
  return api_rc(e);
}

int64_t mavlm_attention_ws_floats(int32_t R, int32_t S, int32_t H) {
  return (R > 0 && S > 0 && H > 0) ? (int64_t)mavlm_attention_split_ws_floats(R, S, H) : 0;
}

int mavlm_attention_plan(int32_t R, int32_t S, int32_t H, int32_t info[4]) {
  if (!info || R <= 0 || S <= 0 || H <= 0) return MAVLM_E_ARG;
  int v[4];
  mavlm_attention_plan_info(R, S, H, v);
  for (int i = 0; i < 4; ++i) info[i] = v[i];
  return 0;
}

int mavlm_attention_plan_unit(int32_t R, int32_t S, int32_t H, int32_t level, int32_t a, int32_t b) {
  if (R <= 0 || S <= 0 || H <= 0) return MAVLM_E_ARG;
  return mavlm_attention_plan_unit_(R, S, H, level, a, b);
}

int mavlm_attention_ws(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, void* O,
                       int32_t ldo, float* lse2, int32_t R, int32_t S, int32_t H, float scale, float* ws,
                       int64_t ws_floats, int32_t dtype, void* stream) {
  mavlm_attn_args a = attn_args(Q, ldq, K, ldk, V, ldv, O, ldo, lse2, R, S, H, scale);
  if (R > 0 && S > 0 && H > 0) {
    const int64_t need = (int64_t)mavlm_attention_split_ws_floats(R, S, H);
    if (need > 0 && (!ws || ws_floats < need)) return MAVLM_E_ARG;     // the plan is part of the result: no silent change
    a.split_ws = need > 0 ? ws : nullptr;
  }
  return api_rc(mavlm_launch_attention(a, dtype, (hipStream_t)stream));
}

int mavlm_attention_hd(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, void* O,
                       int32_t ldo, float* lse2, int32_t R, int32_t S, int32_t H, int32_t head_dim, float scale,
                       int32_t dtype, void* stream) {
  return attention_hd_impl(Q, ldq, K, ldk, V, ldv, O, ldo, lse2, R, S, H, head_dim, scale, false, nullptr, 0, dtype, stream);
}

int mavlm_attention_hd_plan_info(int32_t R, int32_t S, int32_t H, int32_t head_dim, int32_t* info) {
  if (R <= 0 || S <= 0 || H <= 0 || !info) return MAVLM_E_ARG;
  int v[3] = {0, 0, 0};
  mavlm_attention_hd_streamk(R, S, H, head_dim, v);
  info[0] = v[0]; info[1] = v[1]; info[2] = v[2];
  info[3] = v[0] > 0 ? 1 : mavlm_attention_hd_splits(R, S, H, nullptr);
  return 0;
}

int64_t mavlm_attention_hd_ws_floats(int32_t R, int32_t S, int32_t H, int32_t head_dim) {
  return (R > 0 && S > 0 && H > 0 && head_dim > 0) ? (int64_t)mavlm_attention_hd_split_ws_floats(R, S, H, head_dim) : 0;
}

int mavlm_attention_hd_ws(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, void* O,
                          int32_t ldo, float* lse2, int32_t R, int32_t S, int32_t H, int32_t head_dim, float scale, float* ws_,
                          int64_t ws_floats, int32_t dtype, void* stream) {
  return attention_hd_impl(Q, ldq, K, ldk, V, ldv, O, ldo, lse2, R, S, H, head_dim, scale, true, ws_, ws_floats, dtype, stream);
}

// ---- row-batched operators (the training path of BatchedProjector): nb videos per launch, as attn_block runs them
int64_t mavlm_attention_batch_ws_floats(int32_t R, int32_t S, int32_t H, int32_t nb, int32_t head_dim) {
  if (R <= 0 || S <= 0 || head_dim <= 0 || batch_args_bad(H, nb)) return 0;
  // attn_block's rule: the stream-K plan over all H (video, head) pairs where it applies; the split-KV form of the small
  // grids for a single video only
  if (head_dim == 448)
    return (nb == 1 || mavlm_attention_hd_streamk(R, S, H, head_dim, nullptr) > 0) ? (int64_t)mavlm_attention_hd_split_ws_floats(R, S, H, head_dim) : 0;
  if (head_dim > 128) return 0;
  return (nb == 1 || mavlm_attention_streamk_wgs(R, S, H) > 0) ? (int64_t)mavlm_attention_split_ws_floats(R, S, H) : 0;
}

int mavlm_attention_batch(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, void* O,
                          int32_t ldo, float* lse2, int32_t R, int32_t S, int32_t H, float scale, float* ws_,
                          int64_t ws_floats, int32_t nb, int64_t kv_bstride, int32_t head_dim, int32_t dtype, void* stream) {
  if (!Q || !K || !V || !O || R <= 0 || S <= 0 || batch_args_bad(H, nb) || kv_bstride < 0) return MAVLM_E_ARG;
  if (head_dim != 448 && (head_dim <= 0 || head_dim > 128)) return MAVLM_E_SHAPE;
  const int hw = head_dim == 448 ? 448 : 128;                  // columns a head occupies (narrow heads: zero-padded to 128)
  const int Hv = H / nb;
  if ((ldq & 7) || (ldk & 7) || (ldv & 7) || (ldo & 3) || ldq < Hv * hw || ldk < Hv * hw || ldv < Hv * hw || ldo < Hv * hw ||
      (kv_bstride & 7))
    return MAVLM_E_ARG;
  const int64_t need = mavlm_attention_batch_ws_floats(R, S, H, nb, head_dim);
  if (need > 0 && (!ws_ || ws_floats < need)) return MAVLM_E_ARG;        // the plan is part of the result
  mavlm_attn_args a = attn_args(Q, ldq, K, ldk, V, ldv, O, ldo, lse2, R, S, H, scale);
  a.nb = nb; a.kv_bstride = kv_bstride;
  a.split_ws = need > 0 ? ws_ : nullptr;
  return api_rc(hw == 448 ? mavlm_launch_attention_hd(a, head_dim, dtype, (hipStream_t)stream)
                          : mavlm_launch_attention(a, dtype, (hipStream_t)stream));
}

int mavlm_attention_batch_varlen(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, void* O,
                                 int32_t ldo, float* lse2, int32_t R, const int32_t* S, const int64_t* kv_off, int32_t H,
                                 float scale, int32_t nb, int32_t head_dim, int32_t dtype, void* stream) {
  // every check comes before the launch
  if (!Q || !K || !V || !O || R <= 0 || nb < 1 || nb > MAVLM_VBASE_MAX || H <= 0 || H % nb != 0 || (dtype != 0 && dtype != 1))
    return MAVLM_E_ARG;
  if (head_dim <= 0 || head_dim > 128) return MAVLM_E_SHAPE;
  const int Hv = H / nb;
  if ((ldq & 7) || (ldk & 7) || (ldv & 7) || (ldo & 3) || ldq < Hv * 128 || ldk < Hv * 128 || ldv < Hv * 128 || ldo < Hv * 128)
    return MAVLM_E_ARG;
  if (varlen_ranges_bad(S, kv_off, nb, ldk) || varlen_ranges_bad(S, kv_off, nb, ldv)) return MAVLM_E_ARG;
  long long off[MAVLM_VBASE_MAX];
  for (int b = 0; b < nb; ++b) off[b] = kv_off[b];
  mavlm_attn_args a = attn_args(Q, ldq, K, ldk, V, ldv, O, ldo, lse2, R, 0, H, scale);
  a.nb = nb; a.vl_S = S; a.vl_off = off;
  return api_rc(mavlm_launch_attention3_varlen(a, dtype, (hipStream_t)stream));
}

// the same at head_dim 448 (32-query waves): ONE plain-grid launch over (video, head, 128-query block)
int mavlm_attention_hd_batch_varlen(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, void* O,
                                    int32_t ldo, float* lse2, int32_t R, const int32_t* S, const int64_t* kv_off, int32_t H,
                                    float scale, int32_t nb, int32_t head_dim, int32_t dtype, void* stream) {
  // every check comes before the launch
  if (!Q || !K || !V || !O || R <= 0 || nb < 1 || nb > MAVLM_VBASE_MAX || H <= 0 || H % nb != 0 || (dtype != 0 && dtype != 1))
    return MAVLM_E_ARG;
  if (head_dim != 448 || g_mavlm_attn_hd_qg == 1) return MAVLM_E_SHAPE;      // (the 16-query-wave kernel has no such form)
  const int Hv = H / nb;
  if ((ldq & 7) || (ldk & 7) || (ldv & 7) || (ldo & 3) || ldq < Hv * 448 || ldk < Hv * 448 || ldv < Hv * 448 || ldo < Hv * 448)
    return MAVLM_E_ARG;
  if ((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V) & 15) || ((uintptr_t)O & 7)) return MAVLM_E_ARG;   // 16-byte loads, 8-byte stores
  if (varlen_ranges_bad(S, kv_off, nb, ldk) || varlen_ranges_bad(S, kv_off, nb, ldv)) return MAVLM_E_ARG;
  for (int b = 0; b < nb; ++b)     // 32-bit byte offsets inside a video's keys, one 32-key tile past the ragged last one included
    if (((double)S[b] + 64.0) * ldk * 2.0 >= 2147483648.0 || ((double)S[b] + 64.0) * ldv * 2.0 >= 2147483648.0) return MAVLM_E_ARG;
  long long off[MAVLM_VBASE_MAX];
  for (int b = 0; b < nb; ++b) off[b] = kv_off[b];
  mavlm_attn_args a = attn_args(Q, ldq, K, ldk, V, ldv, O, ldo, lse2, R, 0, H, scale);
  a.nb = nb; a.vl_S = S; a.vl_off = off;
  return api_rc(mavlm_launch_attention_hd_varlen(a, head_dim, dtype, (hipStream_t)stream));
}

// ---- column sums and attention maps ------------------------------------------------------------------------------------------
// (returns the launcher's hipError_t as it is, no MAVLM_E_ARG mapping: the established behaviour of this export)
int mavlm_attention_colsum_hd(const void* Q, int32_t ldq, const void* K, int32_t ldk, const float* lse2, float* part,
                              int32_t R, int32_t S, int32_t H, int32_t head_dim, float scale, int32_t dtype, void* stream) {
  if (!Q || !K || !lse2 || !part || R <= 0 || S <= 0 || H <= 0 || (ldq & 7) || (ldk & 7)) return MAVLM_E_ARG;
  if (head_dim != 448 && head_dim != 128) return MAVLM_E_SHAPE;
  return (int)mavlm_launch_colsum_hd(colsum_args(Q, ldq, K, ldk, lse2, part, R, S, H, scale), head_dim, dtype, (hipStream_t)stream);
}

int64_t mavlm_attention_colsum_floats(int32_t R, int32_t S, int32_t H) {
  return (R > 0 && S > 0 && H > 0) ? (int64_t)mavlm_colsum_part_floats(R, S, H) : 0;
}

int mavlm_attention_colsum_plan(int32_t R, int32_t S, int32_t H, int32_t info[2]) {
  if (!info || R <= 0 || S <= 0 || H <= 0) return MAVLM_E_ARG;
  int planes = 1;
  info[0] = mavlm_colsum_plan(R, S, H, &planes);
  info[1] = mavlm_colsum_planes(R, S, H);
  return 0;
}

int mavlm_attention_colsum(const void* Q, int32_t ldq, const void* K, int32_t ldk, const float* lse2, float* part,
                           int64_t part_floats, int32_t R, int32_t S, int32_t H, float scale, int32_t dtype, void* stream) {
  if (R <= 0 || S <= 0 || H <= 0 || !part || part_floats < (int64_t)mavlm_colsum_part_floats(R, S, H)) return MAVLM_E_ARG;
  return api_rc(mavlm_launch_colsum(colsum_args(Q, ldq, K, ldk, lse2, part, R, S, H, scale), dtype, (hipStream_t)stream));
}

// row-batched column sums: nb videos per launch, every video on the single-video schedule (the bits of nb launches)
int64_t mavlm_attention_colsum_batch_floats(int32_t R, int32_t S, int32_t H, int32_t nb) {
  return (R > 0 && S > 0 && H > 0 && nb >= 1 && nb <= MAVLM_MAX_BATCH) ? (int64_t)nb * (int64_t)mavlm_colsum_part_floats(R, S, H) : 0;
}

int mavlm_attention_colsum_batch(const void* Q, int32_t ldq, const void* K, int32_t ldk, int64_t kv_bstride, const float* lse2,
                                 float* part, int64_t part_floats, int32_t R, int32_t S, int32_t H, int32_t nb, int32_t head_dim,
                                 float scale, int32_t dtype, void* stream) {
  // every check comes before any launch
  if (!Q || !K || !lse2 || !part || R <= 0 || S <= 0 || H <= 0 || nb < 1 || nb > MAVLM_MAX_BATCH || (dtype != 0 && dtype != 1))
    return MAVLM_E_ARG;
  if (head_dim != 448 && (head_dim <= 0 || head_dim > 128)) return MAVLM_E_SHAPE;
  const int hw = head_dim == 448 ? 448 : 128;                  // columns a head occupies (narrow heads: zero-padded to 128)
  if ((ldq & 7) || (ldk & 7) || (kv_bstride & 7) || ldq < H * hw || ldk < H * hw) return MAVLM_E_ARG;
  if (nb > 1 && kv_bstride < (int64_t)S * ldk) return MAVLM_E_ARG;           // a video's keys end before the next video's start
  const int64_t per = (int64_t)mavlm_colsum_part_floats(R, S, H);
  if (part_floats < (int64_t)nb * per) return MAVLM_E_ARG;
  if (hw == 128 && ((double)R * ldq * 2.0 >= 2147483648.0 || (double)((S + 127) / 128) * H * ((R + 63) / 64) >= 2.0e9))
    return MAVLM_E_ARG;                                         // the 32-bit offsets / schedule arithmetic of the pipelined kernel
  mavlm_colsum_args a = colsum_args(Q, ldq, K, ldk, lse2, part, R, S, H, scale);
  a.nb = nb; a.kv_bstride = kv_bstride; a.part_bstride = per;
  hipError_t e = hipSuccess;
  if (hw == 448) {
    e = mavlm_launch_colsum_hd(a, 448, dtype, (hipStream_t)stream);
  } else if (g_mavlm_attn_impl != 2) {
    e = mavlm_launch_colsum3(a, dtype, (hipStream_t)stream);
  } else {                                                     // the register-staged diagnostic kernel knows one video
    a.nb = 1;
    for (int b = 0; b < nb && e == hipSuccess; ++b) {
      a.Q = (const uint16_t*)Q + (size_t)b * R * ldq; a.K = (const uint16_t*)K + (size_t)b * kv_bstride;
      a.lse2 = lse2 + (size_t)b * H * R; a.part = part + (size_t)b * per;
      e = mavlm_launch_colsum(a, dtype, (hipStream_t)stream);
    }
  }
  return api_rc(e);
}

// the same with per-video key counts (head columns of 128): every video on the schedule of its own shape
int64_t mavlm_attention_colsum_batch_varlen_floats(int32_t R, const int32_t* S, int32_t H, int32_t nb) {
  if (R <= 0 || H <= 0 || !S || nb < 1 || nb > MAVLM_VBASE_MAX) return 0;
  int64_t n = 0;
  for (int b = 0; b < nb; ++b) {
    if (S[b] < 1) return 0;
    n += (int64_t)mavlm_colsum_part_floats(R, S[b], H);
  }
  return n;
}

int mavlm_attention_colsum_batch_varlen(const void* Q, int32_t ldq, const void* K, int32_t ldk, const int64_t* kv_off,
                                        const float* lse2, float* part, int64_t part_floats, int32_t R, const int32_t* S,
                                        int32_t H, int32_t nb, int32_t head_dim, float scale, int32_t dtype, void* stream) {
  // every check comes before any launch
  if (!Q || !K || !lse2 || !part || R <= 0 || H <= 0 || nb < 1 || nb > MAVLM_VBASE_MAX || (dtype != 0 && dtype != 1)) return MAVLM_E_ARG;
  if (head_dim <= 0 || head_dim > 128) return MAVLM_E_SHAPE;
  if ((ldq & 7) || (ldk & 7) || ldq < H * 128 || ldk < H * 128) return MAVLM_E_ARG;
  if (varlen_ranges_bad(S, kv_off, nb, ldk)) return MAVLM_E_ARG;
  const int64_t need = mavlm_attention_colsum_batch_varlen_floats(R, S, H, nb);
  if (need <= 0 || part_floats < need) return MAVLM_E_ARG;
  if ((double)R * ldq * 2.0 >= 2147483648.0) return MAVLM_E_ARG;            // the 32-bit offsets of the pipelined kernel
  for (int b = 0; b < nb; ++b)
    if ((double)((S[b] + 127) / 128) * H * ((R + 63) / 64) >= 2.0e9) return MAVLM_E_ARG;     // ... and its schedule arithmetic
  long long off[MAVLM_VBASE_MAX];
  for (int b = 0; b < nb; ++b) off[b] = kv_off[b];
  mavlm_colsum_args a = colsum_args(Q, ldq, K, ldk, lse2, part, R, 0, H, scale);
  a.nb = nb; a.vl_S = S; a.vl_kv_off = off;
  return api_rc(mavlm_launch_colsum3_varlen(a, dtype, (hipStream_t)stream));
}

int64_t mavlm_attention_group_mass_floats(int32_t R, int32_t S, int32_t H, int32_t q_group, int32_t k_group) {
  return (R > 0 && S > 0 && H > 0 && q_group > 0 && k_group > 0) ? (int64_t)mavlm_group_mass_floats(R, S, H, q_group, k_group) : 0;
}

int mavlm_attention_group_mass(const void* Q, int32_t ldq, const void* K, int32_t ldk, const float* lse2, float* out,
                               int64_t out_floats, int32_t R, int32_t S, int32_t H, int32_t head_dim, float scale,
                               int32_t q_group, int32_t k_group, int32_t dtype, void* stream) {
  // every check comes before any launch
  if (!Q || !K || !lse2 || !out || R <= 0 || S <= 0 || H <= 0 || (ldq & 7) || (ldk & 7) || (dtype != 0 && dtype != 1))
    return MAVLM_E_ARG;
  if (!mavlm_group_mass_supported(R, S, H, head_dim, q_group, k_group)) return MAVLM_E_SHAPE;
  if (ldq < H * head_dim || ldk < H * head_dim) return MAVLM_E_ARG;
  if (out_floats < (int64_t)mavlm_group_mass_floats(R, S, H, q_group, k_group)) return MAVLM_E_ARG;
  mavlm_group_mass_args a;
  a.Q = Q; a.ldq = ldq; a.K = K; a.ldk = ldk; a.lse2 = lse2; a.out = out;
  a.scratch = out + mavlm_group_mass_out_floats(R, S, H, q_group, k_group);
  a.R = R; a.S = S; a.H = H; a.scale = scale; a.q_group = q_group; a.k_group = k_group;
  return api_rc(mavlm_launch_group_mass(a, head_dim, dtype, (hipStream_t)stream));
}

// ---- row-wise operators ------------------------------------------------------------------------------------------------------
// (returns the launcher's hipError_t as it is, no MAVLM_E_ARG mapping: the established behaviour of this export)
int mavlm_pe_add(const void* xin, const int64_t* idx, const void* table, void* out, int32_t T, int32_t P, int32_t D,
                 int32_t dtype, void* stream) {
  if (!xin || !idx || !table || !out || T < 0) return MAVLM_E_ARG;
  return (int)mavlm_launch_row_add(xin, nullptr, table, idx, out, T, P, D, dtype, (hipStream_t)stream);
}

int mavlm_pool_bilinear(const void* xin, void* out, const void* pe_table, const int64_t* idx, int32_t F, int32_t side,
                        int32_t stride, int32_t D, int32_t dtype, void* stream) {
  return api_rc(mavlm_launch_pool_bilinear(xin, out, pe_table, idx, F, side, stride, D, dtype, (hipStream_t)stream));
}

int mavlm_row_add(const void* xin, const int64_t* src, const void* table, const int64_t* idx, void* out, int32_t T,
                  int32_t P, int32_t D, int32_t dtype, void* stream) {
  return api_rc(mavlm_launch_row_add(xin, src, table, idx, out, T, P, D, dtype, (hipStream_t)stream));
}

// ---- backward pass ------------------------------------------------------------------------
int mavlm_attention_bwd(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, const void* O,
                        int32_t ldo, const void* dO, int32_t lddo, const float* lse2, float* delta, void* dQ,
                        int32_t lddq, void* dK, int32_t lddk, void* dV, int32_t lddv, int32_t R, int32_t S, int32_t H,
                        float scale, int32_t dtype, void* stream) {
  const bwd_abi p = {Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse2, delta, dQ, lddq, dK, lddk, dV, lddv};
  if (bwd_abi_null(p) || R <= 0 || S <= 0 || H <= 0) return MAVLM_E_ARG;
  if (const int rc = bwd_abi_check(p, H * 128)) return rc;
  return attn_bwd_launch(attn_bwd_args(p, R, S, H, scale), 128, dtype, stream);
}

int mavlm_attention_bwd_hd(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, const void* O,
                           int32_t ldo, const void* dO, int32_t lddo, const float* lse2, float* delta, void* dQ,
                           int32_t lddq, void* dK, int32_t lddk, void* dV, int32_t lddv, int32_t R, int32_t S, int32_t H,
                           int32_t head_dim, float scale, int32_t dtype, void* stream) {
  const bwd_abi p = {Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse2, delta, dQ, lddq, dK, lddk, dV, lddv};
  if (bwd_abi_null(p) || R <= 0 || S <= 0 || H <= 0) return MAVLM_E_ARG;
  if (head_dim != 448) return MAVLM_E_SHAPE;
  if (const int rc = bwd_abi_check(p, H * head_dim)) return rc;
  if (((uintptr_t)dQ | (uintptr_t)dK | (uintptr_t)dV) & 7) return MAVLM_E_ARG;
  return attn_bwd_launch(attn_bwd_args(p, R, S, H, scale), head_dim, dtype, stream);
}

// row-batched backward: arguments checked before anything is enqueued (hw = columns of a head: 128 or 448)
static int attention_bwd_batch(const bwd_abi& p, int32_t R, int32_t S, int32_t H, int hw, float scale, int32_t nb, int64_t kv_bstride,
                               int64_t dkv_bstride, int32_t dtype, void* stream) {
  if (bwd_abi_null(p) || R <= 0 || S <= 0 || batch_args_bad(H, nb)) return MAVLM_E_ARG;
  if (hw != 128 && hw != 448) return MAVLM_E_SHAPE;
  if (kv_bstride < 0 || dkv_bstride < 0 || (kv_bstride & 7) || (dkv_bstride & 3)) return MAVLM_E_ARG;
  if (nb > 1 && (kv_bstride == 0 || ((p.dK || p.dV) && dkv_bstride == 0))) return MAVLM_E_ARG;     // (videos on top of each other)
  if (const int rc = bwd_abi_check(p, (H / nb) * hw)) return rc;
  if (((uintptr_t)p.dQ | (uintptr_t)p.dK | (uintptr_t)p.dV) & 7) return MAVLM_E_ARG;
  mavlm_attn_bwd_args a = attn_bwd_args(p, R, S, H, scale);
  a.nb = nb; a.kv_bstride = kv_bstride; a.dkv_bstride = dkv_bstride;
  return attn_bwd_launch(a, hw, dtype, stream);
}

int mavlm_attention_bwd_batch(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, const void* O,
                              int32_t ldo, const void* dO, int32_t lddo, const float* lse2, float* delta, void* dQ,
                              int32_t lddq, void* dK, int32_t lddk, void* dV, int32_t lddv, int32_t R, int32_t S, int32_t H,
                              float scale, int32_t nb, int64_t kv_bstride, int64_t dkv_bstride, int32_t dtype, void* stream) {
  const bwd_abi p = {Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse2, delta, dQ, lddq, dK, lddk, dV, lddv};
  return attention_bwd_batch(p, R, S, H, 128, scale, nb, kv_bstride, dkv_bstride, dtype, stream);
}

int mavlm_attention_bwd_hd_batch(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv,
                                 const void* O, int32_t ldo, const void* dO, int32_t lddo, const float* lse2, float* delta,
                                 void* dQ, int32_t lddq, void* dK, int32_t lddk, void* dV, int32_t lddv, int32_t R, int32_t S,
                                 int32_t H, int32_t head_dim, float scale, int32_t nb, int64_t kv_bstride, int64_t dkv_bstride,
                                 int32_t dtype, void* stream) {
  const bwd_abi p = {Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse2, delta, dQ, lddq, dK, lddk, dV, lddv};
  if (head_dim != 448 && !bwd_abi_null(p) && R > 0 && S > 0 && !batch_args_bad(H, nb)) return MAVLM_E_SHAPE;
  return attention_bwd_batch(p, R, S, H, head_dim, scale, nb, kv_bstride, dkv_bstride, dtype, stream);
}

// the same with per-video key counts (head columns of 128): always the dQ, dK and dV kernels, whatever the fused switch says
int mavlm_attention_bwd_batch_varlen(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, const void* O,
                                     int32_t ldo, const void* dO, int32_t lddo, const float* lse2, float* delta, void* dQ,
                                     int32_t lddq, void* dK, int32_t lddk, void* dV, int32_t lddv, int32_t R, const int32_t* S,
                                     const int64_t* kv_off, const int64_t* dkv_off, int32_t H, float scale, int32_t nb,
                                     int32_t head_dim, int32_t dtype, void* stream) {
  // every check comes before any launch
  const bwd_abi p = {Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse2, delta, dQ, lddq, dK, lddk, dV, lddv};
  if (bwd_abi_null(p) || R <= 0 || nb < 1 || nb > MAVLM_VBASE_MAX || H <= 0 || H % nb != 0 || (dtype != 0 && dtype != 1))
    return MAVLM_E_ARG;
  if (head_dim <= 0 || head_dim > 128) return MAVLM_E_SHAPE;
  if (const int rc = bwd_abi_check(p, (H / nb) * 128)) return rc;
  if (((uintptr_t)dQ | (uintptr_t)dK | (uintptr_t)dV) & 7) return MAVLM_E_ARG;
  if (varlen_ranges_bad(S, kv_off, nb, ldk) || varlen_ranges_bad(S, kv_off, nb, ldv)) return MAVLM_E_ARG;
  if ((dK && varlen_ranges_bad(S, dkv_off, nb, lddk)) || (dV && varlen_ranges_bad(S, dkv_off, nb, lddv))) return MAVLM_E_ARG;
  const double lim = 2147483648.0;                          // the 32-bit buffer offsets of the kernel, per video
  if (((double)R + 64) * ldq * 2.0 >= lim || ((double)R + 64) * lddo * 2.0 >= lim) return MAVLM_E_ARG;
  long long off[MAVLM_VBASE_MAX], doff[MAVLM_VBASE_MAX];
  double keys = 0.0;
  int smax = 0;
  for (int b = 0; b < nb; ++b) {
    if (((double)S[b] + 64) * ldk * 2.0 >= lim || ((double)S[b] + 64) * ldv * 2.0 >= lim) return MAVLM_E_ARG;
    off[b] = kv_off[b];
    doff[b] = (dK || dV) ? dkv_off[b] : 0;
    keys += S[b];
    smax = S[b] > smax ? S[b] : smax;
  }
  mavlm_attn_bwd_args a = attn_bwd_args(p, R, smax, H, scale);
  a.nb = nb; a.vl_S = S; a.vl_off = off; a.vl_doff = doff;
  const int Hv = H / nb;
  const double units = (dQ ? 3.0 : 0.0) + (dK ? 3.0 : 0.0) + (dV ? 2.0 : 0.0);
  mavlm_prof_scope prof(MAVLM_K_ATTN_BWD, units * 2.0 * R * keys * Hv * 128, 2.0 * 128 * Hv * (4.0 * R * nb + 4.0 * keys),
                        (hipStream_t)stream);
  return api_rc(mavlm_launch_attention_bwd_varlen(a, dtype, (hipStream_t)stream));
}

// the same at head columns of 448: dK and dV together run the fused kernel, as mavlm_attention_bwd_hd_batch does
int mavlm_attention_bwd_hd_batch_varlen(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv,
                                        const void* O, int32_t ldo, const void* dO, int32_t lddo, const float* lse2, float* delta,
                                        void* dQ, int32_t lddq, void* dK, int32_t lddk, void* dV, int32_t lddv, int32_t R,
                                        const int32_t* S, const int64_t* kv_off, const int64_t* dkv_off, int32_t H, float scale,
                                        int32_t nb, int32_t head_dim, int32_t dtype, void* stream) {
  // every check comes before any launch
  const bwd_abi p = {Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse2, delta, dQ, lddq, dK, lddk, dV, lddv};
  if (bwd_abi_null(p) || R <= 0 || nb < 1 || nb > MAVLM_VBASE_MAX || H <= 0 || H % nb != 0 || (dtype != 0 && dtype != 1))
    return MAVLM_E_ARG;
  if (head_dim != 448) return MAVLM_E_SHAPE;
  if (const int rc = bwd_abi_check(p, (H / nb) * 448)) return rc;
  if (((uintptr_t)dQ | (uintptr_t)dK | (uintptr_t)dV) & 7) return MAVLM_E_ARG;
  if (varlen_ranges_bad(S, kv_off, nb, ldk) || varlen_ranges_bad(S, kv_off, nb, ldv)) return MAVLM_E_ARG;
  if ((dK && varlen_ranges_bad(S, dkv_off, nb, lddk)) || (dV && varlen_ranges_bad(S, dkv_off, nb, lddv))) return MAVLM_E_ARG;
  const double lim = 2147483648.0;                          // the 32-bit buffer offsets of the kernel, per video
  if (((double)R + 64) * ldq * 2.0 >= lim || ((double)R + 64) * lddo * 2.0 >= lim) return MAVLM_E_ARG;
  long long off[MAVLM_VBASE_MAX], doff[MAVLM_VBASE_MAX];
  double keys = 0.0;
  int smax = 0;
  for (int b = 0; b < nb; ++b) {
    if (((double)S[b] + 64) * ldk * 2.0 >= lim || ((double)S[b] + 64) * ldv * 2.0 >= lim) return MAVLM_E_ARG;
    off[b] = kv_off[b];
    doff[b] = (dK || dV) ? dkv_off[b] : 0;
    keys += S[b];
    smax = S[b] > smax ? S[b] : smax;
  }
  mavlm_attn_bwd_args a = attn_bwd_args(p, R, smax, H, scale);
  a.nb = nb; a.vl_S = S; a.vl_off = off; a.vl_doff = doff;
  const int Hv = H / nb;
  const double units = (dQ ? 3.0 : 0.0) + (dK ? 3.0 : 0.0) + (dV ? 2.0 : 0.0);
  mavlm_prof_scope prof(MAVLM_K_ATTN_BWD, units * 2.0 * R * keys * Hv * 448, 2.0 * 448 * Hv * (4.0 * R * nb + 4.0 * keys),
                        (hipStream_t)stream);
  return api_rc(mavlm_launch_attention_bwd_hd_varlen(a, 448, dtype, (hipStream_t)stream));
}

int64_t mavlm_layernorm_bwd_ws_floats(int32_t D) { return (int64_t)mavlm_layernorm_bwd_partial_floats(D); }

int mavlm_layernorm_bwd(const void* dy, const float* xin, const void* res, int32_t ldr, const float* gamma, void* dz,
                        float* dgamma, float* dbeta, float* ws, int32_t rows, int32_t D, float eps, int32_t dtype,
                        void* stream) {
  if (!dy || !xin || !gamma || !dz || !dgamma || !dbeta || !ws) return MAVLM_E_ARG;
  return api_rc(mavlm_launch_layernorm_bwd(dy, xin, res, ldr, gamma, dz, dgamma, dbeta, ws, rows, D, eps, dtype, (hipStream_t)stream));
}

int mavlm_transpose(const void* in, int32_t ldi, int32_t rows, int32_t cols, void* out, int32_t ldo, void* stream) {
  if (!in || !out) return MAVLM_E_ARG;
  return api_rc(mavlm_launch_transpose(in, ldi, rows, cols, out, ldo, (hipStream_t)stream));
}

int mavlm_rowsum(const void* in, int32_t ld, int32_t rows, int32_t cols, float* out, int32_t dtype, void* stream) {
  if (!in || !out) return MAVLM_E_ARG;
  return api_rc(mavlm_launch_rowsum(in, ld, rows, cols, out, dtype, (hipStream_t)stream));
}

int mavlm_act(int32_t kind, const void* xin, const void* dy, void* out, int64_t n, int32_t dtype, void* stream) {
  if (!xin || !out || n < 0) return MAVLM_E_ARG;
  return api_rc(mavlm_launch_act(kind, xin, dy, out, (size_t)n, dtype, (hipStream_t)stream));
}

// wide-head attention backward: element-wise pieces between the per-head GEMMs (backward.hip)
int mavlm_attention_probs(const float* S, int32_t lds_, const float* lse2, void* P, int32_t ldp, int32_t R, int32_t cols,
                          int32_t valid, float scale, int32_t dtype, void* stream) {
  if (!S || !lse2 || !P) return MAVLM_E_ARG;
  return api_rc(mavlm_launch_attn_probs(S, lds_, lse2, P, ldp, R, cols, valid, scale * 1.44269504088896340736f, dtype, (hipStream_t)stream));
}

int mavlm_attention_dscores(const float* S, int32_t lds_, const float* dP, int32_t lddp, const float* lse2, const float* delta,
                            void* dS, int32_t ldds, int32_t R, int32_t cols, int32_t valid, float scale, int32_t dtype,
                            void* stream) {
  if (!S || !dP || !lse2 || !delta || !dS) return MAVLM_E_ARG;
  return api_rc(mavlm_launch_attn_dscores(S, lds_, dP, lddp, lse2, delta, dS, ldds, R, cols, valid, scale * 1.44269504088896340736f, scale,
                                          dtype, (hipStream_t)stream));
}

int mavlm_rowdot_heads(const void* a, int32_t lda, const void* b, int32_t ldb, float* out, int32_t R, int32_t H, int32_t head_dim,
                       int32_t dtype, void* stream) {
  if (!a || !b || !out) return MAVLM_E_ARG;
  return api_rc(mavlm_launch_rowdot(a, lda, b, ldb, out, R, H, head_dim, dtype, (hipStream_t)stream));
}

// ---- inactive variants of the reference -------------------------------------------------------
int mavlm_frame_mean(const void* xin, void* out16, float* out32, int32_t F, int32_t P, int32_t D, int32_t dtype,
                     void* stream) {
  if (!xin || (!out16 && !out32)) return MAVLM_E_ARG;
  return api_rc(mavlm_launch_frame_mean(xin, out16, out32, F, P, D, dtype, (hipStream_t)stream));
}

int mavlm_adjacent_cosine(const float* v, float* out, int32_t n, int32_t D, float eps, void* stream) {
  if (!v || !out) return MAVLM_E_ARG;
  return api_rc(mavlm_launch_adjacent_cosine(v, out, n, D, eps, (hipStream_t)stream));
}

// (the recurrence refuses a hidden size, not a pointer: hipErrorInvalidValue comes back as MAVLM_E_SHAPE here)
int mavlm_gru_sequence(const float* xg, const void* whh, const float* bhh, void* out, int32_t F, int32_t H, int32_t ndir,
                       int32_t dtype, void* stream) {
  if (!xg || !whh || !bhh || !out) return MAVLM_E_ARG;
  const hipError_t e = mavlm_launch_gru_seq(xg, whh, bhh, out, F, H, ndir, dtype, (hipStream_t)stream);
  return e == hipErrorInvalidValue ? MAVLM_E_SHAPE : (int)e;
}

}  // extern "C"
