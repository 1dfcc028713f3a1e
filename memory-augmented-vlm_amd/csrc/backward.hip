// Row-wise / layout kernels of the backward pass of the memory path.  All HBM-bound.
//
//   layernorm_bwd_kernel   backward of Residual's LayerNorm(x + res) (MemoryController.py:24,28): recomputes the
//                          normalised row from the saved fp32 GEMM output and the residual, writes dz (the gradient
//                          of BOTH the dense output and the residual) and per-wave partial sums of dgamma / dbeta
//   colsum_partials_kernel [P][cols] fp32 partials -> [cols] (deterministic second stage)
//   transpose_kernel       16-bit [rows, cols] -> [cols, rows_pad] (zero-filled pad): turns the "contract over rows"
//                          products of the backward (dW = dY^T X) into the K-contiguous form the MFMA GEMMs read
//   rowsum_kernel          bias gradient: row sums of dY^T
//   act_kernel             GELU forward on a stored pre-activation, GELU / ReLU backward
//   splitk_reduce_kernel   fp32 split-K partials -> 16-bit
#include "mavlm_common.h"
#include "mavlm_kernels.h"

namespace {

constexpr int LNB_BLOCKS = 512;  // workgroups of the LayerNorm backward = partial rows of dgamma/dbeta (one per workgroup)

template <typename T, int NV>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const uint16_t* __restrict__ dy,
                                                            const float* __restrict__ x,
                                                            const uint16_t* __restrict__ res, int ldr,
                                                            const float* __restrict__ gamma, uint16_t* __restrict__ dz,
                                                            float* __restrict__ part, int rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = gridDim.x * 4;
  const int nvec = D >> 2;
  f32x4 g[NV], ag[NV], ab[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = i * 64 + lane;
    g[i] = j < nvec ? ((const f32x4*)gamma)[j] : f32x4{0.f, 0.f, 0.f, 0.f};
    ag[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    ab[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float invD = 1.0f / (float)D;
  for (int row = wv; row < rows; row += nw) {
    f32x4 v[NV], d[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j = i * 64 + lane;
      if (j < nvec) {
        v[i] = ((const f32x4*)(x + (size_t)row * D))[j];
        if (res != nullptr) {
          const u16x4 rv = *(const u16x4*)(res + (size_t)row * ldr + 4 * j);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[i][e] += T::to_f32(rv[e]);
        }
        const u16x4 dv = *(const u16x4*)(dy + (size_t)row * D + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[i][e] = T::to_f32(dv[e]);
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
      } else {
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        d[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    const float mean = wave_sum(s) * invD;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j = i * 64 + lane;
      if (j < nvec) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[i][e] -= mean;
          ss += v[i][e] * v[i][e];
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(ss) * invD + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = v[i][e] * rstd;
        const float gd = d[i][e] * g[i][e];
        ag[i][e] += d[i][e] * xh;
        ab[i][e] += d[i][e];
        v[i][e] = xh;
        d[i][e] = gd;
        s1 += gd;
        s2 += gd * xh;
      }
    }
    const float m1 = wave_sum(s1) * invD, m2 = wave_sum(s2) * invD;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j = i * 64 + lane;
      if (j < nvec)
        *(u32x2*)(dz + (size_t)row * D + 4 * j) =
            pack4<T>(rstd * (d[i][0] - m1 - v[i][0] * m2), rstd * (d[i][1] - m1 - v[i][1] * m2),
                     rstd * (d[i][2] - m1 - v[i][2] * m2), rstd * (d[i][3] - m1 - v[i][3] * m2));
    }
  }
  // the 4 waves of the workgroup add their sums through LDS (fixed order: deterministic), one partial row per workgroup
  extern __shared__ __attribute__((aligned(16))) float red[];      // [3][2][D]: waves 1..3
  const int w = threadIdx.x >> 6;
  if (w > 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j = i * 64 + lane;
      if (j < nvec) {
        ((f32x4*)(red + (size_t)(w - 1) * 2 * D))[j] = ag[i];
        ((f32x4*)(red + (size_t)(w - 1) * 2 * D + D))[j] = ab[i];
      }
    }
  }
  __syncthreads();
  if (w == 0) {
    float* pg = part + (size_t)blockIdx.x * 2 * D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j = i * 64 + lane;
      if (j < nvec) {
        f32x4 a = ag[i], b = ab[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const f32x4 ra = ((const f32x4*)(red + (size_t)k * 2 * D))[j];
          const f32x4 rb = ((const f32x4*)(red + (size_t)k * 2 * D + D))[j];
          a[0] += ra[0]; a[1] += ra[1]; a[2] += ra[2]; a[3] += ra[3];
          b[0] += rb[0]; b[1] += rb[1]; b[2] += rb[2]; b[3] += rb[3];
        }
        ((f32x4*)pg)[j] = a;
        ((f32x4*)(pg + D))[j] = b;
      }
    }
  }
}

// out[c] = sum_p part[p][c]; a workgroup owns 64 columns, its 16 waves take every 16th partial row (fixed order:
// deterministic), then add up through LDS
__global__ __launch_bounds__(1024) void colsum_partials_kernel(const float* __restrict__ part, int nparts, int cols,
                                                               float* __restrict__ out) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float s0 = 0.f, s1 = 0.f;
  if (c < cols) {
    int p = w;
    for (; p + 16 < nparts; p += 32) {       // two independent chains per thread
      s0 += part[(size_t)p * cols + c];
      s1 += part[(size_t)(p + 16) * cols + c];
    }
    if (p < nparts) s0 += part[(size_t)p * cols + c];
  }
  red[w][lane] = s0 + s1;
  __syncthreads();
  if (w == 0 && c < cols) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][lane];
    out[c] = t;
  }
}

// 64x64 tile through LDS; 8-byte global accesses on both sides.
__global__ __launch_bounds__(256) void transpose_kernel(const uint16_t* __restrict__ in, int ldi, int rows, int cols,
                                                        uint16_t* __restrict__ out, int ldo, int rows_pad) {
  __shared__ uint16_t tile[64][68];
  const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = tid + 256 * k;
    const int rr = v >> 4, cv = v & 15;
    u16x4 d = u16x4{0, 0, 0, 0};
    if (r0 + rr < rows && c0 + 4 * cv < cols) d = *(const u16x4*)(in + (size_t)(r0 + rr) * ldi + c0 + 4 * cv);
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[4 * cv + j][rr] = d[j];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = tid + 256 * k;
    const int cc = v >> 4, rv = v & 15;
    if (c0 + cc < cols && r0 + 4 * rv < rows_pad)
      *(u16x4*)(out + (size_t)(c0 + cc) * ldo + r0 + 4 * rv) = *(const u16x4*)&tile[cc][4 * rv];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void rowsum_kernel(const uint16_t* __restrict__ in, int ld, int rows, int cols,
                                                     float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint16_t* p = in + (size_t)row * ld;
  float s = 0.f;
  for (int j = lane * 8; j < cols; j += 512) {
    if (j + 8 <= cols) {
      const u16x8 v = *(const u16x8*)(p + j);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += T::to_f32(v[e]);
    } else {
      for (int e = j; e < cols; ++e) s += T::to_f32(p[e]);
    }
  }
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

// kind 0: out = gelu(x)   1: out = dy * gelu'(x)   2: out = x > 0 ? dy : 0   (x = the ReLU OUTPUT)
template <typename T, int KIND>
__global__ __launch_bounds__(256) void act_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy,
                                                  uint16_t* __restrict__ out, size_t nvec) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
    const u16x8 a = ((const u16x8*)x)[i];
    u16x8 b = a, o;
    if (KIND != 0) b = ((const u16x8*)dy)[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xv = T::to_f32(a[e]);
      float r;
      if (KIND == 0) {
        r = gelu_erf_fast(xv);
      } else if (KIND == 1) {
        const float cdf = 0.5f * (1.0f + erff(xv * 0.70710678118654752440f));
        const float pdf = 0.39894228040143267794f * __expf(-0.5f * xv * xv);
        r = T::to_f32(b[e]) * (cdf + xv * pdf);
      } else {
        r = xv > 0.f ? T::to_f32(b[e]) : 0.f;
      }
      o[e] = T::from_f32(r);
    }
    ((u16x8*)out)[i] = o;
  }
}

// out = epilogue(sum of the split-K planes + bias); EPI as the GEMM epilogues (bias may be null = 0); N % 4 == 0
template <typename T, int EPI>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int splits, size_t n4,
                                                            const float* __restrict__ bias, int N4, void* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 s = ((const f32x4*)part)[i];
    for (int k = 1; k < splits; ++k) {
      const f32x4 v = ((const f32x4*)part)[(size_t)k * n4 + i];
      s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
    if (bias != nullptr) {
      const f32x4 b = ((const f32x4*)bias)[i % (size_t)N4];
      s[0] += b[0]; s[1] += b[1]; s[2] += b[2]; s[3] += b[3];
    }
    if (EPI == MAVLM_EPI_RELU) {
      s[0] = fmaxf(s[0], 0.f); s[1] = fmaxf(s[1], 0.f); s[2] = fmaxf(s[2], 0.f); s[3] = fmaxf(s[3], 0.f);
    } else if (EPI == MAVLM_EPI_GELU) {
      s[0] = gelu_erf_fast(s[0]); s[1] = gelu_erf_fast(s[1]); s[2] = gelu_erf_fast(s[2]); s[3] = gelu_erf_fast(s[3]);
    }
    if (EPI == MAVLM_EPI_F32) ((f32x4*)out)[i] = s;
    else ((u32x2*)out)[i] = pack4<T>(s[0], s[1], s[2], s[3]);
  }
}

// ---- wide-head attention backward (head_dim 448: LLaVA-OneVision-7B, the shape scripts/train/finetune_long.sh trains):
// the register budget of the flash-style backward (attention_bwd.hip) does not stretch to 448-wide heads, so that
// case materialises the scores of ONE head at a time ([R,S] fp32 from the MFMA GEMM) and runs every product as a GEMM;
// these are the element-wise pieces in between.
//   prob_kernel     P[r,s]  = exp2(S[r,s]*c - lse2[r])  (0 for s >= S_valid)          -> 16-bit
//   dscore_kernel   dS[r,s] = exp2(S[r,s]*c - lse2[r]) * (dP[r,s] - delta[r]) * scale  (the UNROUNDED probability, as the
//                   flash-style kernels use; 0 for s >= S_valid)                       -> 16-bit
//   rowdot_kernel   delta[h][r] = sum_d a[r, h*hd+d] * b[r, h*hd+d]                   (any head_dim)
template <typename T>
__global__ __launch_bounds__(256) void prob_kernel(const float* __restrict__ S, int lds_, const float* __restrict__ lse2,
                                                   uint16_t* __restrict__ P, int ldp, int R, int cols, int valid, float c) {
  const int r = blockIdx.y;
  const float l = lse2[r];
  const float* sr = S + (size_t)r * lds_;
  uint16_t* pr = P + (size_t)r * ldp;
  for (int j = (blockIdx.x * 256 + threadIdx.x) * 4; j < cols; j += gridDim.x * 1024) {
    const f32x4 v = *(const f32x4*)(sr + j);
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (j + e < valid) ? __builtin_amdgcn_exp2f(v[e] * c - l) : 0.f;
    *(u32x2*)(pr + j) = pack4<T>(o[0], o[1], o[2], o[3]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dscore_kernel(const float* __restrict__ S, int lds_, const float* __restrict__ dP,
                                                     int lddp, const float* __restrict__ lse2, const float* __restrict__ delta,
                                                     uint16_t* __restrict__ dS, int ldds, int R, int cols, int valid, float c,
                                                     float scale) {
  const int r = blockIdx.y;
  const float d = delta[r], l = lse2[r];
  for (int j = (blockIdx.x * 256 + threadIdx.x) * 4; j < cols; j += gridDim.x * 1024) {
    const f32x4 sv = *(const f32x4*)(S + (size_t)r * lds_ + j);
    const f32x4 g = *(const f32x4*)(dP + (size_t)r * lddp + j);
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o[e] = (j + e < valid) ? __builtin_amdgcn_exp2f(sv[e] * c - l) * (g[e] - d) * scale : 0.f;
    *(u32x2*)(dS + (size_t)r * ldds + j) = pack4<T>(o[0], o[1], o[2], o[3]);
  }
}

// one wave per (row, head)
template <typename T>
__global__ __launch_bounds__(256) void rowdot_kernel(const uint16_t* __restrict__ a, int lda, const uint16_t* __restrict__ b,
                                                     int ldb, float* __restrict__ out, int R, int H, int hd) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= R * H) return;
  const int r = item / H, h = item % H;
  const uint16_t* pa = a + (size_t)r * lda + h * hd;
  const uint16_t* pb = b + (size_t)r * ldb + h * hd;
  float s = 0.f;
  for (int j = lane * 8; j < hd; j += 512) {
    const u16x8 x = *(const u16x8*)(pa + j);
    const u16x8 y = *(const u16x8*)(pb + j);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += T::to_f32(x[e]) * T::to_f32(y[e]);
  }
  s = wave_sum(s);
  if (lane == 0) out[(size_t)h * R + r] = s;
}

template <typename T>
hipError_t launch_ln_bwd(const uint16_t* dy, const float* x, const uint16_t* res, int ldr, const float* gamma,
                         uint16_t* dz, float* part, int rows, int D, float eps, hipStream_t s) {
  const dim3 grid(LNB_BLOCKS), block(256);
  const int nv = (D / 4 + 63) / 64;
  const size_t lds = (size_t)3 * 2 * D * sizeof(float);
#define LNB(NV)                                                                                                     \
  do {                                                                                                              \
    static mavlm_per_device_once once;                                                                              \
    if (lds > 65536) {                                                                                              \
      hipError_t ae = once.dyn_lds((const void*)layernorm_bwd_kernel<T, NV>, 3 * 2 * MAVLM_LN_MAX_D * 4);           \
      if (ae != hipSuccess) return ae;                                                                              \
    }                                                                                                               \
    hipLaunchKernelGGL((layernorm_bwd_kernel<T, NV>), grid, block, lds, s, dy, x, res, ldr, gamma, dz, part, rows,   \
                       D, eps);                                                                                     \
  } while (0)
  if (nv <= 1) LNB(1);
  else if (nv <= 2) LNB(2);
  else if (nv <= 4) LNB(4);
  else if (nv <= 8) LNB(8);
  else if (nv <= 16) LNB(16);
  else return hipErrorInvalidValue;
#undef LNB
  return hipGetLastError();
}

}  // namespace

size_t mavlm_layernorm_bwd_partial_floats(int D) { return (size_t)(LNB_BLOCKS + 1) * 2 * D; }

hipError_t mavlm_launch_layernorm_bwd(const void* dy, const float* x, const void* res, int ldr, const float* gamma,
                                      void* dz, float* dgamma, float* dbeta, float* part, int rows, int D, float eps,
                                      int dtype, hipStream_t s) {
  if (rows <= 0 || (D & 3) || D > MAVLM_LN_MAX_D) return hipErrorInvalidValue;
  mavlm_prof_scope prof(MAVLM_K_LN, 0.0, 12.0 * rows * (double)D, s);
  hipError_t e = dtype == MAVLM_F16
                     ? launch_ln_bwd<F16>((const uint16_t*)dy, x, (const uint16_t*)res, ldr, gamma, (uint16_t*)dz, part, rows, D, eps, s)
                     : launch_ln_bwd<BF16>((const uint16_t*)dy, x, (const uint16_t*)res, ldr, gamma, (uint16_t*)dz, part, rows, D, eps, s);
  if (e != hipSuccess) return e;
  // partial rows are [workgroup][2][D]: view as [LNB_BLOCKS][2D] and sum down the columns; dgamma = cols [0,D), dbeta = [D,2D)
  // of a 2D-wide result; write through a small two-step so that dgamma / dbeta may be separate allocations
  hipLaunchKernelGGL(colsum_partials_kernel, dim3((2 * D + 63) / 64), dim3(1024), 0, s, part, LNB_BLOCKS, 2 * D,
                     part + (size_t)LNB_BLOCKS * 2 * D);
  e = hipMemcpyAsync(dgamma, part + (size_t)LNB_BLOCKS * 2 * D, sizeof(float) * D, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(dbeta, part + (size_t)LNB_BLOCKS * 2 * D + D, sizeof(float) * D, hipMemcpyDeviceToDevice, s);
}

hipError_t mavlm_launch_transpose(const void* in, int ldi, int rows, int cols, void* out, int ldo, hipStream_t s) {
  if (rows <= 0 || cols <= 0 || (cols & 3) || (ldi & 3) || (ldo & 3)) return hipErrorInvalidValue;
  const int rows_pad = (rows + 63) / 64 * 64;
  if (ldo < rows_pad) return hipErrorInvalidValue;
  mavlm_prof_scope prof(MAVLM_K_TRANSPOSE, 0.0, 4.0 * rows * (double)cols, s);
  hipLaunchKernelGGL(transpose_kernel, dim3(rows_pad / 64, (cols + 63) / 64), dim3(256), 0, s, (const uint16_t*)in, ldi,
                     rows, cols, (uint16_t*)out, ldo, rows_pad);
  return hipGetLastError();
}

hipError_t mavlm_launch_rowsum(const void* in, int ld, int rows, int cols, float* out, int dtype, hipStream_t s) {
  if (rows <= 0 || cols <= 0 || (ld & 7)) return hipErrorInvalidValue;
  mavlm_prof_scope prof(MAVLM_K_MISC, 0.0, 2.0 * rows * (double)cols, s);
  if (dtype == MAVLM_F16)
    hipLaunchKernelGGL(rowsum_kernel<F16>, dim3((rows + 3) / 4), dim3(256), 0, s, (const uint16_t*)in, ld, rows, cols, out);
  else
    hipLaunchKernelGGL(rowsum_kernel<BF16>, dim3((rows + 3) / 4), dim3(256), 0, s, (const uint16_t*)in, ld, rows, cols, out);
  return hipGetLastError();
}

hipError_t mavlm_launch_act(int kind, const void* x, const void* dy, void* out, size_t n, int dtype, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if ((n & 7) || kind < 0 || kind > 2 || (kind != 0 && dy == nullptr)) return hipErrorInvalidValue;
  const size_t nvec = n >> 3;
  const int blocks = (int)((nvec + 255) / 256 < 8192 ? (nvec + 255) / 256 : 8192);
  mavlm_prof_scope prof(MAVLM_K_MISC, 0.0, (kind == 0 ? 4.0 : 6.0) * n, s);
#define ACT(TT, KK) hipLaunchKernelGGL((act_kernel<TT, KK>), dim3(blocks), dim3(256), 0, s, (const uint16_t*)x, (const uint16_t*)dy, (uint16_t*)out, nvec)
  if (dtype == MAVLM_F16) {
    if (kind == 0) ACT(F16, 0); else if (kind == 1) ACT(F16, 1); else ACT(F16, 2);
  } else {
    if (kind == 0) ACT(BF16, 0); else if (kind == 1) ACT(BF16, 1); else ACT(BF16, 2);
  }
#undef ACT
  return hipGetLastError();
}

hipError_t mavlm_launch_splitk_reduce(const float* part, int splits, size_t n, void* out, int dtype, hipStream_t s,
                                      const float* bias, int N, int epilogue) {
  if ((n & 3) || (bias != nullptr && (N <= 0 || (N & 3)))) return hipErrorInvalidValue;
  const size_t n4 = n >> 2;
  const int blocks = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
#define SKR(TT, EE) hipLaunchKernelGGL((splitk_reduce_kernel<TT, EE>), dim3(blocks), dim3(256), 0, s, part, splits, n4, bias, N / 4, out)
#define SKR_T(TT)                                                    \
  switch (epilogue) {                                                \
    case MAVLM_EPI_BIAS: SKR(TT, MAVLM_EPI_BIAS); break;             \
    case MAVLM_EPI_RELU: SKR(TT, MAVLM_EPI_RELU); break;             \
    case MAVLM_EPI_GELU: SKR(TT, MAVLM_EPI_GELU); break;             \
    case MAVLM_EPI_F32: SKR(TT, MAVLM_EPI_F32); break;               \
    default: return hipErrorInvalidValue;                            \
  }
  if (dtype == MAVLM_F16) { SKR_T(F16) } else { SKR_T(BF16) }
#undef SKR_T
#undef SKR
  return hipGetLastError();
}

hipError_t mavlm_launch_attn_probs(const float* S, int lds_, const float* lse2, void* P, int ldp, int R, int cols, int valid,
                                   float c, int dtype, hipStream_t s) {
  if (R <= 0 || cols <= 0 || (cols & 3) || (lds_ & 3) || (ldp & 3) || valid > cols) return hipErrorInvalidValue;
  mavlm_prof_scope prof(MAVLM_K_MISC, 0.0, 6.0 * R * (double)cols, s);
  const dim3 grid((cols / 4 + 255) / 256 < 8 ? (cols / 4 + 255) / 256 : 8, R);
  if (dtype == MAVLM_F16)
    hipLaunchKernelGGL(prob_kernel<F16>, grid, dim3(256), 0, s, S, lds_, lse2, (uint16_t*)P, ldp, R, cols, valid, c);
  else
    hipLaunchKernelGGL(prob_kernel<BF16>, grid, dim3(256), 0, s, S, lds_, lse2, (uint16_t*)P, ldp, R, cols, valid, c);
  return hipGetLastError();
}

hipError_t mavlm_launch_attn_dscores(const float* S, int lds_, const float* dP, int lddp, const float* lse2, const float* delta,
                                     void* dS, int ldds, int R, int cols, int valid, float c, float scale, int dtype,
                                     hipStream_t s) {
  if (R <= 0 || cols <= 0 || (cols & 3) || (lds_ & 3) || (lddp & 3) || (ldds & 3) || valid > cols) return hipErrorInvalidValue;
  mavlm_prof_scope prof(MAVLM_K_MISC, 0.0, 10.0 * R * (double)cols, s);
  const dim3 grid((cols / 4 + 255) / 256 < 8 ? (cols / 4 + 255) / 256 : 8, R);
  if (dtype == MAVLM_F16)
    hipLaunchKernelGGL(dscore_kernel<F16>, grid, dim3(256), 0, s, S, lds_, dP, lddp, lse2, delta, (uint16_t*)dS, ldds, R, cols,
                       valid, c, scale);
  else
    hipLaunchKernelGGL(dscore_kernel<BF16>, grid, dim3(256), 0, s, S, lds_, dP, lddp, lse2, delta, (uint16_t*)dS, ldds, R, cols,
                       valid, c, scale);
  return hipGetLastError();
}

hipError_t mavlm_launch_rowdot(const void* a, int lda, const void* b, int ldb, float* out, int R, int H, int hd, int dtype,
                               hipStream_t s) {
  if (R <= 0 || H <= 0 || hd <= 0 || (hd & 7) || (lda & 7) || (ldb & 7)) return hipErrorInvalidValue;
  if (dtype == MAVLM_F16)
    hipLaunchKernelGGL(rowdot_kernel<F16>, dim3((R * H + 3) / 4), dim3(256), 0, s, (const uint16_t*)a, lda, (const uint16_t*)b,
                       ldb, out, R, H, hd);
  else
    hipLaunchKernelGGL(rowdot_kernel<BF16>, dim3((R * H + 3) / 4), dim3(256), 0, s, (const uint16_t*)a, lda, (const uint16_t*)b,
                       ldb, out, R, H, hd);
  return hipGetLastError();
}
