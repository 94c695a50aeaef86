// moq_nvfp4.hip -- static NVFP4 weights: E2M1 elements under per-block (16) E4M3 scales relative to a tensor-wide amax.
//   moq_nvfp4_static_qdq          static_blockwise_fp4_fake_quant (kernels/quantization/gemm/fp4_kernel.py:217-318)
//   moq_nvfp4_fp8_sweep           _fp8_scale_sweep_kernel          (gemm/nvfp4_fp8_sweep.py:59-124)
//   moq_nvfp4_fp8_sweep_hessian   _fp8_scale_sweep_hessian_kernel  (gemm/nvfp4_fp8_sweep.py:174-226)
//   moq_nvfp4_pack / _unpack      NVFP4QTensor.quantize / .dequantize (qtensor/nvfp4_tensor.py:253-407), the checkpoint form
//
// The sweeps try the 126 positive finite E4M3 values c_k * 448 as block scales.  The reference rounds fl(|w| / s_k)
// onto the E2M1 grid (fp4_round_magnitude, common/nvfp4_quant.py).  fl(a / s) is monotone in a, so each of the seven
// rounding thresholds of one candidate is one exact boundary on |w|: U = the largest a whose quotient still rounds to
// the lower side.  The 126 x 7 boundaries and the 126 x 8 products fl(q * s) are computed (with IEEE divisions) once
// per workgroup into LDS; an element-candidate then costs seven compares / selects, a subtraction and a square --
// no division -- and gives the value of the correctly rounded quotient bit for bit.
#include "moq_chunk.h"

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

// ------------------------------------------------------------------------------------------------ (d) pack / unpack
// The stored byte of a block scale: torch's clamp(2^-9, 448) keeps a NaN, its cast to float8_e4m3fn is RNE.
__device__ __forceinline__ uint32_t scale_byte(float s) {
  if (s != s) return 0x7Fu | ((__float_as_uint(s) >> 24) & 0x80u);
  const float c = __builtin_fminf(__builtin_fmaxf(s, 0x1p-9f), 448.0f);
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c, c, 0, false) & 0xFFu;
}

// NVFP4QTensor._cast_fp4 of one quotient: sign bit = (q < 0) (so -0 and NaN have none), magnitude code = round half to
// even onto {0, .5, 1, 1.5, 2, 3, 4, 6}, saturating; a NaN gives 7.  a = min(|q|, 6) (a NaN becomes 6).  For a >= 1 the code
// is the exponent field and the top mantissa bit of a rounded to nearest even at that bit (+4 folded into the rounding
// constant, so that the low three bits are the code); below 1 the grid step is 0.5 and the fp32 addition of 2^22 -- whose
// ulp is 0.5 -- rounds to it, ties to the even multiple, leaving the code in the low bits of the sum.
__device__ __forceinline__ uint32_t e2m1_nibble(float q) {
  const float a = __builtin_fminf(__builtin_fabsf(q), 6.0f);
  const uint32_t u = __float_as_uint(a);
  const uint32_t big = (u + 0x011FFFFFu + ((u >> 22) & 1u)) >> 22;
  const uint32_t small = __float_as_uint(a + 0x1p22f);
  return ((a < 1.0f ? small : big) & 7u) | (q < 0.0f ? 8u : 0u);
}

// One chunk of 8192 elements (512 blocks) per workgroup, one 16-byte packet per lane and step: a block is LPG = 2 lanes
// (16-bit dtypes) or 4 (f32).  Every lane of a block forms the block's scale byte itself (the same operations on the same
// values); the first one stores it.  The 16 quotients x / d of a block share d = fl(float(scale byte) * scale_2): inside
// [2^-40, 2^20] and with every x of the packet zero or in [2^-100, 2^80] no quotient and no residual leaves the normal range
// (an overflowing quotient would turn into a NaN in the residual steps and lose its sign), and the division is five FMAs on
// a refined reciprocal, bit for bit the IEEE quotient (SharedDiv, moq_common.h); every other packet divides.
// STATIC: block amax given.  GIVEN: the scale bytes are an input (NVFP4QTensor.quantize with weights_scaling_factor).
template <int DT, bool STATIC, bool GIVEN>
__global__ void __launch_bounds__(kBlock) nvfp4_pack_kernel(const void* __restrict__ x, const float* __restrict__ amax,
                                                            const float* __restrict__ gamax,
                                                            const float* __restrict__ scale2,
                                                            uint8_t* __restrict__ packed, uint8_t* __restrict__ scales,
                                                            int64_t n) {
  constexpr int V = Elem<DT>::kVec;
  constexpr int P = Chunk<DT>::kPackets;
  constexpr int LPG = kNvBlock / V;
  const float s2 = scale2[0];
  const float six_s2 = 6.0f * s2;
  float scale_max = 1.0f;
  if constexpr (STATIC && !GIVEN) scale_max = gamax[0] / 6.0f;
  const int64_t n_chunks = (n + MOQ_MT_CHUNK - 1) / MOQ_MT_CHUNK;
  const int lane = threadIdx.x & 63;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t e0 = c * MOQ_MT_CHUNK;
    Pack16 in[P];
    float am[P];
    uint32_t sb[P];
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int64_t e = e0 + packet_off<DT>(u);
      am[u] = 0.0f;
      sb[u] = 0u;
      if (e < n) {
        in[u] = load16_nt(reinterpret_cast<const char*>(x) + e * (16 / V));
        if constexpr (GIVEN) sb[u] = scales[e >> 4];
        else if constexpr (STATIC) am[u] = amax[e >> 4];
      } else {
        in[u].w[0] = in[u].w[1] = in[u].w[2] = in[u].w[3] = 0u;
      }
    }
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int64_t e = e0 + packet_off<DT>(u);
      const uint32_t own_bits = pack_absmax<DT>(in[u]);
      if constexpr (!GIVEN) {
        float s;
        if constexpr (STATIC) {
          s = am[u] / 6.0f;
          s = s == 0.0f ? 1.0f : s;
          s = (s * 448.0f) / scale_max;
        } else {
          s = __uint_as_float(group_max_u32<LPG>(own_bits)) / six_s2;
          s = s == 0.0f ? 1.0f : s;
        }
        sb[u] = scale_byte(s);
      }
      const float d = __builtin_amdgcn_cvt_f32_fp8((int)sb[u], 0) * s2;
      const SharedDiv sd = make_shared_div(d);
      const float ad = __builtin_fabsf(d);
      const bool fast = ad >= 0x1p-40f && ad <= 0x1p20f && own_bits <= 0x67800000u /* 2^80 */ &&
                        !pack_has_tiny_nonzero<DT>(in[u]);
      float v[8];
      unpack<DT>(in[u], v);
      uint32_t word = 0;
      if (fast) {
#pragma unroll
        for (int i = 0; i < V; ++i) word |= e2m1_nibble(shared_div_in_window(v[i], sd)) << (4 * i);
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) word |= e2m1_nibble(v[i] / d) << (4 * i);
      }
      if (e < n) {
        if constexpr (V == 8) __builtin_nontemporal_store(word, reinterpret_cast<uint32_t*>(packed + e / 2));
        else *reinterpret_cast<uint16_t*>(packed + e / 2) = (uint16_t)word;
        if constexpr (!GIVEN) {
          if ((lane & (LPG - 1)) == 0) scales[e >> 4] = (uint8_t)sb[u];
        }
      }
    }
  }
}

// 4 packed bytes -> 8 elements per lane: out = to_dt(e2m1_values[nibble] * fl(float(scale byte) * scale_2)); the table's
// entry for nibble 8 is +0 (qtensor/nvfp4_tensor.py:27)
template <int DT>
__global__ void __launch_bounds__(kBlock) nvfp4_unpack_kernel(const uint8_t* __restrict__ packed,
                                                              const uint8_t* __restrict__ scales,
                                                              const float* __restrict__ scale2, void* __restrict__ out,
                                                              int64_t n_words) {
  constexpr int V = Elem<DT>::kVec;
  const float s2 = scale2[0];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_words; p += stride) {
    const uint32_t w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(packed) + p);
    const float d = __builtin_amdgcn_cvt_f32_fp8((int)scales[p >> 1], 0) * s2;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t nib = (w >> (4 * i)) & 0xFu, m = nib & 7u;
      const float mag = m < 2 ? 0.5f * (float)m : __uint_as_float(((m >> 1) + 126u) << 23 | (m & 1u) << 22);
      v[i] = (m != 0 && (nib & 8u) ? -mag : mag) * d;
    }
#pragma unroll
    for (int h = 0; h < 8 / V; ++h)
      store16_nt(reinterpret_cast<char*>(out) + (p * 8 + h * V) * (16 / V), pack<DT>(v + h * V));
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

extern "C" int moq_nvfp4_pack(const void* x, const float* amax, const float* global_amax, const float* scale_2,
                              uint8_t* packed, uint8_t* scale_e4m3, int scales_given, int64_t n_blocks, int block, int dt,
                              void* stream) {
  const bool is_static = amax != nullptr;
  if (n_blocks < 0 || (n_blocks > 0 && (!x || !scale_2 || !packed || !scale_e4m3 ||
                                        (is_static && !scales_given && !global_amax)))) {
    set_error("moq_nvfp4_pack: bad arguments");
    return MOQ_ERR_INVALID;
  }
  if (block != kNvBlock) {
    set_error("moq_nvfp4_pack: block size %d (only 16)", block);
    return MOQ_ERR_UNSUPPORTED;
  }
  if (((uintptr_t)x & 15u) || ((uintptr_t)packed & 3u) || ((uintptr_t)amax & 3u)) {
    set_error("moq_nvfp4_pack: x must be 16-byte, packed and amax 4-byte aligned");
    return MOQ_ERR_UNSUPPORTED;
  }
  if (n_blocks == 0) return MOQ_OK;
  const int64_t n = n_blocks * kNvBlock;
  const int grid = copy_grid((n + MOQ_MT_CHUNK - 1) / MOQ_MT_CHUNK);
  hipStream_t st = (hipStream_t)stream;
#define MOQ_NVP_LAUNCH(S, G)                                                                                      \
  MOQ_DISPATCH_DTYPE(dt, hipLaunchKernelGGL((nvfp4_pack_kernel<DT, S, G>), dim3(grid), dim3(kBlock), 0, st, x, amax, \
                                            global_amax, scale_2, packed, scale_e4m3, n))
  if (scales_given) {
    MOQ_NVP_LAUNCH(false, true);
  } else if (is_static) {
    MOQ_NVP_LAUNCH(true, false);
  } else {
    MOQ_NVP_LAUNCH(false, false);
  }
#undef MOQ_NVP_LAUNCH
  return check_launch("moq_nvfp4_pack");
}

extern "C" int moq_nvfp4_unpack(const uint8_t* packed, const uint8_t* scale_e4m3, const float* scale_2, void* out,
                                int64_t n_blocks, int block, int dt, void* stream) {
  if (n_blocks < 0 || (n_blocks > 0 && (!packed || !scale_e4m3 || !scale_2 || !out))) {
    set_error("moq_nvfp4_unpack: bad arguments");
    return MOQ_ERR_INVALID;
  }
  if (block != kNvBlock) {
    set_error("moq_nvfp4_unpack: block size %d (only 16)", block);
    return MOQ_ERR_UNSUPPORTED;
  }
  if (((uintptr_t)packed & 3u) || ((uintptr_t)out & 15u)) {
    set_error("moq_nvfp4_unpack: packed must be 4-byte, out 16-byte aligned");
    return MOQ_ERR_UNSUPPORTED;
  }
  if (n_blocks == 0) return MOQ_OK;
  const int64_t words = n_blocks * 2;
  hipStream_t st = (hipStream_t)stream;
  MOQ_DISPATCH_DTYPE(dt, hipLaunchKernelGGL(nvfp4_unpack_kernel<DT>, dim3(launch_grid(kBlock, words)), dim3(kBlock), 0, st,
                                            packed, scale_e4m3, scale_2, out, words));
  return check_launch("moq_nvfp4_unpack");
}
