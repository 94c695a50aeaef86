// moq_nvfp4.hip -- static NVFP4 weights: E2M1 elements under per-block (16) E4M3 scales relative to a tensor-wide amax.
//   moq_nvfp4_static_qdq          static_blockwise_fp4_fake_quant (kernels/quantization/gemm/fp4_kernel.py:217-318)
//   moq_nvfp4_fp8_sweep           _fp8_scale_sweep_kernel          (gemm/nvfp4_fp8_sweep.py:59-124)
//   moq_nvfp4_fp8_sweep_hessian   _fp8_scale_sweep_hessian_kernel  (gemm/nvfp4_fp8_sweep.py:174-226)
//
// The sweeps try the 126 positive finite E4M3 values c_k * 448 as block scales.  The reference rounds fl(|w| / s_k)
// onto the E2M1 grid (fp4_round_magnitude, common/nvfp4_quant.py).  fl(a / s) is monotone in a, so each of the seven
// rounding thresholds of one candidate is one exact boundary on |w|: U = the largest a whose quotient still rounds to
// the lower side.  The 126 x 7 boundaries and the 126 x 8 products fl(q * s) are computed (with IEEE divisions) once
// per workgroup into LDS; an element-candidate then costs seven compares / selects, a subtraction and a square --
// no division -- and gives the value of the correctly rounded quotient bit for bit.
#include "moq_common.h"

namespace moq {
namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int kCand = 126;   // positive finite E4M3 values (codes 1..126)
constexpr int kRow = 16;     // LDS floats per candidate: U[7], V[8], amax factor
constexpr int kNvBlock = 16;

// fp4_round_magnitude's thresholds: "<=" for the ties that round down (to the even code), "<" for those that round up
__device__ const float kT[7] = {0.25f, 0.75f, 1.25f, 1.75f, 2.5f, 3.5f, 5.0f};
__device__ const int kLe[7] = {1, 0, 1, 0, 1, 0, 1};
__device__ const float kQ[8] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 4.0f, 6.0f};

__device__ __forceinline__ float next_up(float a) { return __uint_as_float(__float_as_uint(a) + 1u); }
__device__ __forceinline__ float next_dn(float a) { return __uint_as_float(__float_as_uint(a) - 1u); }

// largest a >= 0 with fl(a / s) <= t   (s > 0 finite, t > 0; fl(t * s) is within a few ulps of it)
__device__ float bound_le(float t, float s) {
  float a = t * s;
  for (int i = 0; i < 64 && a / s > t; ++i) a = next_dn(a);
  for (int i = 0; i < 64 && __float_as_uint(a) < 0x7F7FFFFFu && next_up(a) / s <= t; ++i) a = next_up(a);
  return a;
}

// E4M3 (e4m3fn) value of code k in 1..126, exact
__device__ __forceinline__ float e4m3_value(int k) {
  const int e = k >> 3, m = k & 7;
  return e == 0 ? (float)m * 0x1p-9f : __builtin_ldexpf(1.0f + (float)m * 0.125f, e - 7);
}

// scaled_e4m3_impl(v, amax) on the eager path (tensor_quant.py:46-59): clamp(v * 448/amax) -> e4m3fn -> * amax/448
__device__ __forceinline__ float fp8_eager1(float v, const Fp8Scale& sc) {
  const float a = v * sc.s;
  float c = __builtin_fminf(__builtin_fmaxf(a, -448.0f), 448.0f);
  c = (a != a) ? a : c;
  float r, unused;
  e4m3_roundtrip2(c, 0.0f, r, unused);
  return r * sc.inv;
}

// the per-candidate table: row k = {U[0..6], V[0..7], fl(c_k * g)}.  two_level: the candidate scale goes through the
// FP8 round trip of compute_fp4_scales (the Hessian sweep); else s_k = fl(fl(c_k * g) / 6) (the plain sweep)
__device__ void build_table(float* tab, float g, bool two_level) {
  const Fp8Scale sc = fp8_scale(g / 6.0f);
  for (int i = threadIdx.x; i < kCand * 8; i += blockDim.x) {
    const int k = i >> 3, j = i & 7;
    const float amax_k = (e4m3_value(k + 1) / 448.0f) * g;
    float s = amax_k / 6.0f;
    if (two_level) s = fp8_eager1(s, sc);
    s = s == 0.0f ? 1.0f : s;  // scale_safe (only when g == 0 or the FP8 scale flushes to zero)
    float* row = tab + k * kRow;
    if (j < 7) {
      // "q > q_j" <=> fl(a/s) > T_j (kLe) or fl(a/s) >= T_j: the boundary of "<= T_j" or of "<= pred(T_j)"
      const float t = kLe[j] ? kT[j] : next_dn(kT[j]);
      row[j] = bound_le(t, s);
    } else {
      row[15] = amax_k;
    }
    row[7 + j] = kQ[j] * s;
  }
  __syncthreads();
}

// fl(q(a) * s) of one candidate: the last boundary that a exceeds picks the value (boundaries ascend)
__device__ __forceinline__ float qs_of(float a, const float* u, const float* v) {
  float r = v[0];
#pragma unroll
  for (int j = 0; j < 7; ++j) r = a > u[j] ? v[j + 1] : r;
  return r;
}

// numpy's pairwise order for a contiguous 16-term float32 sum (what the reference's tl.sum gives in the interpreter):
// r_j = p_j + p_{j+8}, then ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7))
__device__ __forceinline__ float sum16(const float* p) {
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = p[j] + p[j + 8];
  return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

// ------------------------------------------------------------------------------------------------ (a) static QDQ
// one 16-byte packet per lane and iteration; a block is 16 elements (2 packets of bf16/f16, 4 of f32)
template <int DT>
__global__ void __launch_bounds__(kBlock) nvfp4_static_qdq_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                                 const float* __restrict__ amax,
                                                                 const float* __restrict__ gamax, int64_t n_packets) {
  constexpr int V = Elem<DT>::kVec;
  constexpr int kPerBlock = kNvBlock / V;
  const Fp8Scale sc = fp8_scale(gamax[0] / 6.0f);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_packets; p += stride) {
    const float s = fp8_eager1(amax[p / kPerBlock] / 6.0f, sc);
    const bool zero = s == 0.0f;
    const float safe = (zero || s != s || __builtin_fabsf(s) == __builtin_inff()) ? 1.0f : s;
    const Pack16 in = load16_nt((const char*)x + p * 16);
    float f[8];
    unpack<DT>(in, f);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float r = __builtin_fabsf(f[i]) / safe;
      float q = 6.0f;  // fp4_round_magnitude, innermost condition first (a NaN quotient stays 6)
      q = r <= 5.0f ? 4.0f : q;
      q = r < 3.5f ? 3.0f : q;
      q = r <= 2.5f ? 2.0f : q;
      q = r < 1.75f ? 1.5f : q;
      q = r <= 1.25f ? 1.0f : q;
      q = r < 0.75f ? 0.5f : q;
      q = r <= 0.25f ? 0.0f : q;
      const float m = q * safe;
      f[i] = zero ? 0.0f : (f[i] >= 0.0f ? m : -m);
    }
    store16_nt((char*)y + p * 16, pack<DT>(f));
  }
}

// ------------------------------------------------------------------------------------------------ (b) plain sweep
// one lane per block: 16 |w| in registers, all 126 candidates, running argmin with strict "<" (lowest index wins ties)
template <int DT>
__global__ void __launch_bounds__(kBlock) nvfp4_sweep_kernel(const void* __restrict__ x, const float* __restrict__ gamax,
                                                            float* __restrict__ best_amax, int64_t n_blocks) {
  __shared__ float tab[kCand * kRow];
  build_table(tab, gamax[0], false);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += stride) {
    float a[16];
    constexpr int V = Elem<DT>::kVec;
#pragma unroll
    for (int c = 0; c < 16 / V; ++c) {
      const Pack16 in = load16_nt((const char*)x + (b * 16 + c * V) * (int64_t)sizeof(typename Elem<DT>::storage));
      unpack<DT>(in, a + c * V);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = __builtin_fabsf(a[i]);
    float best = __builtin_inff();
    int bi = 0;
    for (int k = 0; k < kCand; ++k) {
      const float* row = tab + k * kRow;
      float u[7], v[8];
#pragma unroll
      for (int j = 0; j < 7; ++j) u[j] = row[j];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = row[7 + j];
      float p[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float d = a[i] - qs_of(a[i], u, v);
        p[i] = d * d;
      }
      const float loss = sum16(p);
      if (loss < best) {
        best = loss;
        bi = k;
      }
    }
    best_amax[b] = tab[bi * kRow + 15];
  }
}

// ------------------------------------------------------------------------------------------------ (c) Hessian sweep
// One wave per tile of 16 output rows x one cin-block n.  The loss dw^T H dw of 16 blocks is one [16 x 16] x [16 x 16]
// product on v_mfma_f32_16x16x4_f32 (exact f32, bit-for-bit an fmaf chain in k order), computed as C = H^T-part x dw^T:
//   step s (0..3), lane l (g = l >> 4, col = l & 15):  A = H[k = 4g + s][j = col],  B = dw[row col][k = 4g + s]
//   C/D: lane l holds (dw H)[row col][j = 4g + r], r = 0..3  -- the same four elements 4g..4g+3 the lane holds as B,
// so hdw_j * dw_j needs no lane movement.  hdw_j is the fmaf chain over k = 0,4,8,12, 1,5,9,13, 2,6,10,14, 3,7,11,15
// started at +0; the 16 products are summed in the order of sum16 (lanes g, g^2 hold j and j + 8; g, g^1 the halves).
template <int DT>
__global__ void __launch_bounds__(kBlock) nvfp4_sweep_hessian_kernel(const void* __restrict__ x,
                                                                    const float* __restrict__ hess,
                                                                    const float* __restrict__ gamax,
                                                                    float* __restrict__ best_amax, int64_t cout,
                                                                    int64_t ncb) {
  __shared__ float tab[kCand * kRow];
  build_table(tab, gamax[0], true);
  const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
  const int64_t row_tiles = (cout + 15) / 16, tiles = row_tiles * ncb;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / 64);
  for (int64_t t = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); t < tiles; t += waves) {
    const int64_t n = t % ncb, row = (t / ncb) * 16 + col;
    const bool valid = row < cout;
    const int64_t base = (row * ncb + n) * 16 + 4 * g;
    float w[4], a[4], h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i] = valid ? load1<DT>(x, base + i) : 0.0f;
      a[i] = __builtin_fabsf(w[i]);
      h[i] = hess[n * 256 + (4 * g + i) * 16 + col];
    }
    float best = __builtin_inff();
    int bi = 0;
    for (int k = 0; k < kCand; ++k) {
      const float* rowp = tab + k * kRow;
      float u[7], v[8];
#pragma unroll
      for (int j = 0; j < 7; ++j) u[j] = rowp[j];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = rowp[7 + j];
      float dw[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = a[i] - qs_of(a[i], u, v);
        dw[i] = w[i] >= 0.0f ? d : -d;
      }
      f32x4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h[s], dw[s], acc, 0, 0, 0);
      float q[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = acc[r] * dw[r];
        q[r] = p + __shfl_xor(p, 32);
      }
      const float uh = (q[0] + q[1]) + (q[2] + q[3]);
      const float loss = uh + __shfl_xor(uh, 16);
      if (loss < best) {
        best = loss;
        bi = k;
      }
    }
    if (valid && g == 0) best_amax[row * ncb + n] = tab[bi * kRow + 15];
  }
}

int launch_grid(int64_t items_per_wg_iter, int64_t items) { return stream_grid(items_per_wg_iter, items); }

}  // namespace
}  // namespace moq

using namespace moq;

extern "C" int moq_nvfp4_static_qdq(const void* x, void* y, const float* amax, const float* global_amax,
                                    int64_t n_blocks, int block, int dt, void* stream) {
  if (n_blocks < 0 || (n_blocks > 0 && (!x || !y || !amax || !global_amax))) {
    set_error("moq_nvfp4_static_qdq: bad arguments");
    return MOQ_ERR_INVALID;
  }
  if (block != kNvBlock) {
    set_error("moq_nvfp4_static_qdq: block size %d (only 16)", block);
    return MOQ_ERR_UNSUPPORTED;
  }
  if (((uintptr_t)x | (uintptr_t)y) & 15u) {
    set_error("moq_nvfp4_static_qdq: x / y must be 16-byte aligned");
    return MOQ_ERR_UNSUPPORTED;
  }
  if (n_blocks == 0) return MOQ_OK;
  hipStream_t st = (hipStream_t)stream;
  MOQ_DISPATCH_DTYPE(dt, {
    const int64_t packets = n_blocks * (kNvBlock / Elem<DT>::kVec);
    hipLaunchKernelGGL(nvfp4_static_qdq_kernel<DT>, dim3(launch_grid(kBlock, packets)), dim3(kBlock), 0, st, x, y, amax,
                       global_amax, packets);
  });
  return check_launch("moq_nvfp4_static_qdq");
}

extern "C" int moq_nvfp4_fp8_sweep(const void* x, const float* global_amax, float* best_amax, int64_t n_blocks,
                                   int block, int dt, void* stream) {
  if (n_blocks < 0 || (n_blocks > 0 && (!x || !global_amax || !best_amax))) {
    set_error("moq_nvfp4_fp8_sweep: bad arguments");
    return MOQ_ERR_INVALID;
  }
  if (block != kNvBlock) {
    set_error("moq_nvfp4_fp8_sweep: block size %d (only 16)", block);
    return MOQ_ERR_UNSUPPORTED;
  }
  if ((uintptr_t)x & 15u) {
    set_error("moq_nvfp4_fp8_sweep: x must be 16-byte aligned");
    return MOQ_ERR_UNSUPPORTED;
  }
  if (n_blocks == 0) return MOQ_OK;
  hipStream_t st = (hipStream_t)stream;
  MOQ_DISPATCH_DTYPE(dt, {
    hipLaunchKernelGGL(nvfp4_sweep_kernel<DT>, dim3(launch_grid(kBlock, n_blocks)), dim3(kBlock), 0, st, x, global_amax,
                       best_amax, n_blocks);
  });
  return check_launch("moq_nvfp4_fp8_sweep");
}

extern "C" int moq_nvfp4_fp8_sweep_hessian(const void* x, const float* hessian, const float* global_amax,
                                           float* best_amax, int64_t n_blocks, int64_t n_cin_blocks, int block, int dt,
                                           void* stream) {
  if (n_blocks < 0 || n_cin_blocks <= 0 || (n_blocks > 0 && (!x || !hessian || !global_amax || !best_amax))) {
    set_error("moq_nvfp4_fp8_sweep_hessian: bad arguments");
    return MOQ_ERR_INVALID;
  }
  if (block != kNvBlock) {
    set_error("moq_nvfp4_fp8_sweep_hessian: block size %d (only 16)", block);
    return MOQ_ERR_UNSUPPORTED;
  }
  if (n_blocks % n_cin_blocks != 0) {
    set_error("moq_nvfp4_fp8_sweep_hessian: %lld blocks are not whole rows of %lld cin-blocks (cin %% 16 != 0?)",
              (long long)n_blocks, (long long)n_cin_blocks);
    return MOQ_ERR_UNSUPPORTED;
  }
  if (n_blocks == 0) return MOQ_OK;
  const int64_t cout = n_blocks / n_cin_blocks, tiles = (cout + 15) / 16 * n_cin_blocks;
  hipStream_t st = (hipStream_t)stream;
  MOQ_DISPATCH_DTYPE(dt, {
    hipLaunchKernelGGL(nvfp4_sweep_hessian_kernel<DT>, dim3(launch_grid(kBlock / 64, tiles)), dim3(kBlock), 0, st, x,
                       hessian, global_amax, best_amax, cout, n_cin_blocks);
  });
  return check_launch("moq_nvfp4_fp8_sweep_hessian");
}
