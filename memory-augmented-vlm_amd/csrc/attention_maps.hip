// Attention maps: the mass of the normalised probabilities per (head, query group, key group),
//
//   mass[h][i][j] = sum over q in query group i, k in key group j of exp2(s[q][k] * c - lse2[h][q]),   s = Q.K^T,
//
// for query groups of q_group consecutive rows and key groups of k_group consecutive keys (k_group % 4 == 0; the last group of
// either side may be short).  A second pass over Q, K and the forward's lse2, like the column-sum pass - the probabilities are
// never stored.  Heads of 128 and of 448 columns (the staging and fragment layout of attn_colsum_hd_kernel, attention_hd.hip,
// with the operands' roles swapped: the QUERIES are stationary, the keys stream).
//
// Two stages, every scratch word has ONE writer and every sum a fixed order (no atomics, nothing to clear beforehand):
//   1. attn_group_mass_rows_kernel: a wave keeps 32 queries in registers (B operand of v_mfma_f32_32x32x16) and walks the keys
//      of its key-group range in 32-key tiles (A operand, LDS-DMA into a 2-stage ring shared by the workgroup's 4 waves).
//      The result tile has the query on the lane and 4 consecutive keys in each register quad; the lane pair (l, l^32)
//      holds the 8 quads of a tile.  One v_permlane32_swap per quad pair gives BOTH lanes all 8 quad sums, which they add
//      in key order into a running mass of the current key group.  Whether a quad opens a new group depends on the key
//      index alone - a scalar branch - and at a boundary the running mass goes to rowmass[h][j][q] (the bookkeeping of the
//      FR = 1 forward, attention3.hip).  blockIdx.y cuts the key GROUPS into ranges, so a (row, group) word still has one
//      writer; a range starts at a multiple of k_group, which is a multiple of 4, so the quads never straddle a group.
//   2. attn_group_mass_reduce_kernel: one wave per cell adds the rows of its query group: lane l takes rows l, l + 64, ...
//      in order, then the fixed xor tree.
#include "mavlm_common.h"
#include "mavlm_kernels.h"

namespace {

constexpr int GM_KT = 32;                                   // keys per tile
constexpr int GM_QB = 128;                                  // queries per workgroup (4 waves x 32)

__device__ __forceinline__ int gm_img_x(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

template <typename T, int HD>
__global__ __launch_bounds__(256, 1) void attn_group_mass_rows_kernel(const uint16_t* __restrict__ Q, int ldq,
                                                                      const uint16_t* __restrict__ K, int ldk,
                                                                      const float* __restrict__ lse2,
                                                                      float* __restrict__ rowmass, int R, int S, int H, float c,
                                                                      int kg, int nkg, int gps) {
  constexpr int NSUB = (HD + 127) / 128;                  // 128-column sub-images of a tile row: [32 keys][256 B], swizzled
  constexpr int SUB = GM_KT * 256;
  constexpr int TILE = NSUB * SUB;
  constexpr int KS = HD / 16;                             // k-steps of the 32x32x16 MFMA
  constexpr int NCH = HD / 8;                             // 16-byte chunks of a row
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 key-tile slots
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.x % H;
  const int q0 = (blockIdx.x / H) * GM_QB + wave * 32;
  const int r = lane & 31, hh = lane >> 5;
  // key groups [g_lo, g_hi) -> keys [kbeg, kend)
  const int g_lo = blockIdx.y * gps;
  const int g_hi = g_lo + gps < nkg ? g_lo + gps : nkg;
  const int kbeg = g_lo * kg;
  const int kend = (long long)g_hi * kg < S ? g_hi * kg : S;
  const int nk = kend - kbeg;
  const int nt = (nk + GM_KT - 1) / GM_KT;

  const int qidx = q0 + r;
  typename T::vec8 qf[KS];
  {
    const int qrow = qidx < R ? qidx : R - 1;
    const uint16_t* qp = Q + (size_t)qrow * ldq + h * HD + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const typename T::vec8*)(qp + 16 * ks);
  }
  const float l2 = qidx < R ? lse2[(size_t)h * R + qidx] : INFINITY;      // rows past R: exp2(-inf) = 0 (and never written)
  auto dma_k = [&](int t, char* dst) {                    // 4 waves: instruction ids wave, wave+4, ...
#pragma unroll
    for (int k = 0; k < 2 * NSUB; ++k) {
      const int id = wave + 4 * k;
      const int sub = id >> 3, rg = id & 7;
      const int row = 4 * rg + (lane >> 4);
      int gch = sub * 16 + ((lane & 15) ^ gm_img_x(row));
      gch = gch < NCH ? gch : (gch & 7);
      int krow = kbeg + t * GM_KT + row;
      krow = krow < kend ? krow : kend - 1;               // (the tail's keys are masked below)
      const uint16_t* p = K + (size_t)krow * ldk + h * HD + gch * 8;
      __builtin_amdgcn_global_load_lds((const MAVLM_GLOBAL void*)p, (MAVLM_LDS void*)(dst + sub * SUB + rg * 1024), 16, 0, 0);
    }
  };
  const int xr = gm_img_x(r);
  const int k_rd = 256 * r;
  float* const out = rowmass + (size_t)h * nkg * R + qidx;
  const bool writer = hh == 0 && qidx < R;

  float run = 0.f;                                        // mass of this lane's query in key group g_cur so far
  int g_cur = g_lo, left = kg;                            // (wave-uniform) keys of group g_cur not yet visited

  dma_k(0, smem);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  for (int t = 0; t < nt; ++t) {
    const char* kb = smem + (t & 1) * TILE;
    if (t + 1 < nt) dma_k(t + 1, smem + ((t + 1) & 1) * TILE);
    f32x16 st;
#pragma unroll
    for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int gch = 2 * ks;                             // + hh
      const typename T::vec8 kf = *(const typename T::vec8*)(kb + (gch >> 4) * SUB + k_rd + 16 * (((gch & 15) + hh) ^ xr));
      st = T::mfma32(kf, qf[ks], st);
    }
    // st[i]: key (i & 3) + 8 (i >> 2) + 4 hh of the tile, query r
    float p[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) p[i] = __builtin_amdgcn_exp2f(st[i] * c - l2);
    if (t == nt - 1 && (nk & (GM_KT - 1))) {              // ragged tail of the range
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (t * GM_KT + (i & 3) + 8 * (i >> 2) + 4 * hh >= nk) p[i] = 0.f;
    }
    float v[8];                                           // the tile's 8 quad sums in key order, on both lanes of a pair
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float qs = (p[4 * j] + p[4 * j + 1]) + (p[4 * j + 2] + p[4 * j + 3]);
      float a = qs, b = qs;
      permlane32_swap(a, b);                              // a = the hh = 0 lane's sum, b = the hh = 1 lane's, on both
      v[2 * j] = a;
      v[2 * j + 1] = b;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (t * GM_KT + 4 * e < nk) {                       // (uniform) a quad past the range opens no group
        if (left == 0) {                                  // (uniform) first quad of the next key group
          if (writer) out[(size_t)g_cur * R] = run;
          run = 0.f;
          ++g_cur;
          left = kg;
        }
        run += v[e];
        left -= 4;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  if (writer) out[(size_t)g_cur * R] = run;               // g_cur == g_hi - 1: the range's last group (short when S is ragged)
}

// out[h][i][j] = sum of rowmass[h][j][q] over the rows q of query group i, one wave per cell
__global__ __launch_bounds__(256) void attn_group_mass_reduce_kernel(const float* __restrict__ rowmass, float* __restrict__ out,
                                                                     int R, int qg, int nqg, int nkg, int k_rot, long long cells) {
  const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= cells) return;
  const int lane = threadIdx.x & 63;
  const int j = (int)(cell % nkg);
  const long long hi = cell / nkg;
  const int i = (int)(hi % nqg);
  const long long h = hi / nqg;
  const int qb = i * qg;
  const int qe = qb + qg < R ? qb + qg : R;
  const int js = j + k_rot < nkg ? j + k_rot : j + k_rot - nkg;      // output column j = key group (j + k_rot) mod nkg
  const float* src = rowmass + ((size_t)h * nkg + js) * R;
  float acc = 0.f;
  for (int q = qb + lane; q < qe; q += 64) acc += src[q];
  acc = wave_sum(acc);
  if (lane == 0) out[cell] = acc;
}

// key groups per blockIdx.y range: enough ranges for ~512 workgroups, at least 256 keys each.  Pure function of the shape.
int group_mass_gps(int R, int S, int H, int kg) {
  const long nkg = ((long)S + kg - 1) / kg;
  const long units = (long)((R + GM_QB - 1) / GM_QB) * H;
  long want = (512 + units - 1) / units;
  if (want < 1) want = 1;
  long gps = (nkg + want - 1) / want;
  const long min_g = (256 + (long)kg - 1) / kg;
  if (gps < min_g) gps = min_g;
  if (gps > nkg) gps = nkg;
  return (int)gps;
}

template <typename T, int HD>
hipError_t launch_rows(const mavlm_group_mass_args& a, float* rowmass, int nkg, hipStream_t s) {
  constexpr int LDS = 2 * ((HD + 127) / 128) * GM_KT * 256;
  auto kern = attn_group_mass_rows_kernel<T, HD>;
  static mavlm_per_device_once once;
  {
    hipError_t e = once.dyn_lds((const void*)kern, LDS);
    if (e != hipSuccess) return e;
  }
  const float c = a.scale * 1.44269504088896340736f;
  const int gps = group_mass_gps(a.R, a.S, a.H, a.k_group);
  const int ns = (nkg + gps - 1) / gps;
  mavlm_prof_scope prof(MAVLM_K_COLSUM, 2.0 * a.R * (double)a.S * a.H * HD, 2.0 * HD * a.H * ((double)a.R + (double)a.S * ns), s);
  hipLaunchKernelGGL(kern, dim3(((a.R + GM_QB - 1) / GM_QB) * a.H, ns), dim3(256), LDS, s, (const uint16_t*)a.Q, a.ldq,
                     (const uint16_t*)a.K, a.ldk, a.lse2, rowmass, a.R, a.S, a.H, c, a.k_group, nkg, gps);
  return hipGetLastError();
}

}  // namespace

bool mavlm_group_mass_supported(int R, int S, int H, int head_dim, int q_group, int k_group) {
  if (R <= 0 || S <= 0 || H <= 0 || q_group <= 0 || k_group <= 0 || (k_group & 3)) return false;
  if (head_dim != 128 && head_dim != 448) return false;
  // (the kernels index keys and rows with int)
  return (long long)((S + k_group - 1) / k_group) * k_group < (1ll << 31);
}

size_t mavlm_group_mass_out_floats(int R, int S, int H, int q_group, int k_group) {
  const size_t nqg = ((size_t)R + q_group - 1) / q_group, nkg = ((size_t)S + k_group - 1) / k_group;
  return (size_t)H * nqg * nkg;
}

size_t mavlm_group_mass_floats(int R, int S, int H, int q_group, int k_group) {
  const size_t nkg = ((size_t)S + k_group - 1) / k_group;
  return mavlm_group_mass_out_floats(R, S, H, q_group, k_group) + (size_t)H * nkg * R;      // result, then rowmass [H][nkg][R]
}

hipError_t mavlm_launch_group_mass(const mavlm_group_mass_args& a, int head_dim, int dtype, hipStream_t s) {
  if (!mavlm_group_mass_supported(a.R, a.S, a.H, head_dim, a.q_group, a.k_group)) return hipErrorInvalidValue;
  const int nqg = (a.R + a.q_group - 1) / a.q_group, nkg = (a.S + a.k_group - 1) / a.k_group;
  if (a.k_rot < 0 || a.k_rot >= nkg) return hipErrorInvalidValue;
  float* rowmass = a.scratch;
  const bool f16 = dtype == MAVLM_F16;
  hipError_t e;
  if (head_dim == 448) e = f16 ? launch_rows<F16, 448>(a, rowmass, nkg, s) : launch_rows<BF16, 448>(a, rowmass, nkg, s);
  else e = f16 ? launch_rows<F16, 128>(a, rowmass, nkg, s) : launch_rows<BF16, 128>(a, rowmass, nkg, s);
  if (e != hipSuccess) return e;
  const long long cells = (long long)a.H * nqg * nkg;
  mavlm_prof_scope prof(MAVLM_K_COLSUM, 0.0, 4.0 * a.H * (double)nkg * a.R, s);
  hipLaunchKernelGGL(attn_group_mass_reduce_kernel, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, s, rowmass, a.out, a.R,
                     a.q_group, nqg, nkg, a.k_rot, cells);
  return hipGetLastError();
}
