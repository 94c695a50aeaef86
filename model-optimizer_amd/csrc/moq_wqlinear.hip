// moq_wqlinear.hip -- y[T, N] = x[T, K] . W^[N, K]^T (+ bias) for T <= 32 tokens on PACKED 4-bit weights (RealQuantLinear's
// small-batch forward after mtq.compress).  W^ is never written: a weight-STREAMING kernel, not a tiled GEMM -- at T <= 32 the
// call does at most 128 flop per packed byte, far under the chip's ridge, so the floor of its time is one read of the weight
// bytes.  This first form is far from that floor (profiles/r11_compress.md: 0.05-0.15 of 8 TB/s on the packed bytes): a wave's
// load touches 32 rows x 32 contiguous bytes, every 128-byte line of a row is fetched by four waves, the grid is only N / 32
// workgroups (128 for N = 4096 on 256 CUs) and each wave runs one dependent load-decode-MFMA chain.  It wins over
// unpack + F.linear because that route moves nine times the bytes, not because it streams well.
//
//   * one workgroup per 32 output rows, its 8 waves splitting K in steps of 64; each lane loads ONE 16-byte packet per step
//     (32 k of its row, non-temporal: the weights are read once) and decodes it in registers to four 8-element fragments of
//     the storage dtype -- the A operand of four v_mfma_f32_32x32x16_{bf16,f16};
//   * x is the B operand, its token tile zero-padded to 32: 16-byte loads of 8 k per lane and MFMA, re-read by every
//     workgroup through L2 (at most 32 x K elements);
//   * operand k order: lane (r = lane & 31, h = lane >> 5) of MFMA s (0..3) of a step starting at k0 holds, on BOTH sides,
//     k = k0 + 32 h + 8 s + j in element j -- A: row r of the tile, B: token r.  The instruction sums over its 16 (h, j) pairs,
//     so any assignment of k to them is right as long as A and B use the same one
//     (tests/test_gpu_compress.py checks it with exact data and a token that differs from its neighbour in a single k);
//   * the 8 partial tiles are summed through LDS in wave order 0..7 by a fixed thread per element: no float atomics, the same
//     bits every run.  Bias is added in fp32, one rounding to the storage dtype.
//
// Each decoded weight is bit-identical to what moq_int4_unpack / moq_nvfp4_unpack write (the decode bodies below are theirs),
// products of two 16-bit floats are exact in fp32, accumulation is fp32.
#include "moq_common.h"

namespace moq {
namespace {

constexpr int kWqWaves = 8;                 // waves per workgroup = K split
constexpr int kWqThreads = kWqWaves * kWave;
constexpr int kWqRows = 32;                 // output rows per workgroup (the MFMA's M)
constexpr int kWqStep = 64;                 // k per wave step: 32 per lane half

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int DT>
__device__ __forceinline__ f32x16 mfma_32x32x16(const Pack16& a, const Pack16& b, f32x16 c) {
  if constexpr (DT == MOQ_BF16) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&a), *reinterpret_cast<const bf16x8*>(&b),
                                                   c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(&a), *reinterpret_cast<const f16x8*>(&b), c,
                                                  0, 0, 0);
  }
}

// A decoder turns the 16-byte packet of one lane (32 consecutive k of one row, starting at element index e = row * K + k,
// k % 32 == 0) into four fragments of 8 elements in the storage dtype.  `begin` runs once per lane, `prepare` loads the
// packet's scales.
// A further 4-bit format (MXFP4: low nibble first like NVFP4, one E8M0 byte per 32 k) is one more struct of this shape.
template <int DT>
struct DecodeInt4 {  // moq_int4_pack layout: byte b = (element 2b << 4) | element 2b + 1, value = (nibble - 8) / scale[e / g]
  const void* scales;
  int g;
  float sc;
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void prepare(int64_t e) { sc = load1<DT>(scales, e / g); }  // g % 32 == 0: one group per packet
  __device__ __forceinline__ Pack16 fragment(uint32_t w, int /*s*/) const {
    float v[8];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t byte = (w >> (8 * b)) & 0xFFu;
      v[2 * b] = (float)((int)(byte >> 4) - 8);
      v[2 * b + 1] = (float)((int)(byte & 0xFu) - 8);
    }
    const SharedDiv sd = make_shared_div(sc);  // (int4_unpack_kernel: exact for these numerators inside its window)
    if (sd.fast) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = shared_div_in_window(v[i], sd);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = v[i] / sc;
    }
    return pack<DT>(v);
  }
};

template <int DT>
struct DecodeNvfp4 {  // moq_nvfp4_pack layout: byte b = (element 2b + 1 << 4) | element 2b, one E4M3 byte per 16 k, fp32 scale_2
  const uint8_t* scales;
  const float* scale2;
  float s2;
  float d[2];
  __device__ __forceinline__ void begin() { s2 = scale2[0]; }
  __device__ __forceinline__ void prepare(int64_t e) {
    const uint16_t two = *reinterpret_cast<const uint16_t*>(scales + (e >> 4));  // e % 32 == 0: 2-byte aligned
    d[0] = __builtin_amdgcn_cvt_f32_fp8((int)(two & 0xFFu), 0) * s2;
    d[1] = __builtin_amdgcn_cvt_f32_fp8((int)(two >> 8), 0) * s2;
  }
  __device__ __forceinline__ Pack16 fragment(uint32_t w, int s) const {
    const float dd = d[s >> 1];
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // (nvfp4_unpack_kernel; nibble 8 is +0)
      const uint32_t nib = (w >> (4 * i)) & 0xFu, m = nib & 7u;
      const float mag = m < 2 ? 0.5f * (float)m : __uint_as_float(((m >> 1) + 126u) << 23 | (m & 1u) << 22);
      v[i] = (m != 0 && (nib & 8u) ? -mag : mag) * dd;
    }
    return pack<DT>(v);
  }
};

template <int DT, class Decode>
__global__ __launch_bounds__(kWqThreads) void wq_linear_kernel(const void* __restrict__ x, const uint8_t* __restrict__ packed,
                                                               Decode dec, const void* __restrict__ bias,
                                                               void* __restrict__ y, int T, int64_t N, int64_t K) {
  __shared__ float red[kWqWaves][16][kWave];  // 32 KiB: every wave's partial 32 x 32 tile, [register][lane]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int r = lane & 31, h = lane >> 5;
  const int64_t n = (int64_t)blockIdx.x * kWqRows + r;  // this lane's weight row
  const bool row_ok = n < N, tok_ok = r < T;             // r is also this lane's token (B operand, output column)
  const char* xrow = reinterpret_cast<const char*>(x) + (int64_t)r * K * 2;
  f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const Pack16 zero = {{0, 0, 0, 0}};
  dec.begin();
  for (int64_t k0 = (int64_t)wave * kWqStep; k0 < K; k0 += kWqWaves * kWqStep) {
    const int64_t k = k0 + 32 * h;  // K % 32 == 0: the packet [k, k + 32) is inside the row or wholly past it
    const bool k_ok = k < K;
    Pack16 wp = zero, xb[4] = {zero, zero, zero, zero};
    if (row_ok && k_ok) {
      const int64_t e = n * K + k;
      wp = load16_nt(packed + (e >> 1));
      dec.prepare(e);
    }
    if (tok_ok && k_ok) {
#pragma unroll
      for (int s = 0; s < 4; ++s) xb[s] = load16(xrow + (k + 8 * s) * 2);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const Pack16 a = (row_ok && k_ok) ? dec.fragment(wp.w[s], s) : zero;
      acc = mfma_32x32x16<DT>(a, xb[s], acc);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) red[wave][i][lane] = acc[i];
  __syncthreads();
  // 16 x 64 = 1024 tile elements, two per thread; element (i, l): row (i & 3) + 8 (i >> 2) + 4 (l >> 5), token l & 31
  for (int o = threadIdx.x; o < 16 * kWave; o += kWqThreads) {
    const int i = o / kWave, l = o % kWave;
    float sum = red[0][i][l];
#pragma unroll
    for (int w = 1; w < kWqWaves; ++w) sum += red[w][i][l];
    const int64_t on = (int64_t)blockIdx.x * kWqRows + (i & 3) + 8 * (i >> 2) + 4 * (l >> 5);
    const int t = l & 31;
    if (on < N && t < T) {
      if (bias != nullptr) sum += load1<DT>(bias, on);
      store1<DT>(y, (int64_t)t * N + on, sum);
    }
  }
}

}  // namespace
}  // namespace moq

using namespace moq;

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

extern "C" int moq_wq_linear(const void* x, const uint8_t* packed, const void* scales, const float* scale_2, const void* bias,
                             void* y, int64_t t, int64_t n, int64_t k, int g, int fmt, int dt, void* stream) {
  if (t < 0 || n < 0 || k < 0 || (t * n * k > 0 && (x == nullptr || packed == nullptr || scales == nullptr || y == nullptr)) ||
      (fmt != MOQ_WQ_INT4 && fmt != MOQ_WQ_NVFP4) || (fmt == MOQ_WQ_NVFP4 && scale_2 == nullptr && t * n * k > 0)) {
    set_error("moq_wq_linear: bad arguments");
    return MOQ_ERR_INVALID;
  }
  if (t == 0 || n == 0) return MOQ_OK;
  if (dt != MOQ_BF16 && dt != MOQ_F16) {
    set_error("moq_wq_linear: bf16 or f16 only");
    return MOQ_ERR_UNSUPPORTED;
  }
  if (t > 32 || k <= 0 || k % 32 != 0 || n > 0x7FFFFFFFLL / kWqRows) {
    set_error("moq_wq_linear: needs 1 <= T <= 32 and K a positive multiple of 32 (T %lld, K %lld)", (long long)t, (long long)k);
    return MOQ_ERR_UNSUPPORTED;
  }
  if (fmt == MOQ_WQ_INT4 ? (g <= 0 || g % 32 != 0 || k % g != 0) : g != 16) {
    set_error("moq_wq_linear: INT4 groups must be a multiple of 32 dividing K, NVFP4 blocks 16 (g %d)", g);
    return MOQ_ERR_UNSUPPORTED;
  }
  if ((reinterpret_cast<uintptr_t>(x) & 15u) || (reinterpret_cast<uintptr_t>(packed) & 15u) ||
      (reinterpret_cast<uintptr_t>(scales) & 1u) || (reinterpret_cast<uintptr_t>(y) & 1u) ||
      (reinterpret_cast<uintptr_t>(bias) & 1u)) {
    set_error("moq_wq_linear: x and the packed weight must be 16-byte aligned");
    return MOQ_ERR_UNSUPPORTED;
  }
  const dim3 grid((unsigned)((n + kWqRows - 1) / kWqRows)), block(kWqThreads);
  if (fmt == MOQ_WQ_INT4) {
    if (dt == MOQ_BF16) {
      DecodeInt4<MOQ_BF16> dec{scales, g, 1.0f};
      hipLaunchKernelGGL((wq_linear_kernel<MOQ_BF16, DecodeInt4<MOQ_BF16>>), grid, block, 0, S(stream), x, packed, dec, bias, y,
                         (int)t, n, k);
    } else {
      DecodeInt4<MOQ_F16> dec{scales, g, 1.0f};
      hipLaunchKernelGGL((wq_linear_kernel<MOQ_F16, DecodeInt4<MOQ_F16>>), grid, block, 0, S(stream), x, packed, dec, bias, y,
                         (int)t, n, k);
    }
  } else {
    if (dt == MOQ_BF16) {
      hipLaunchKernelGGL((wq_linear_kernel<MOQ_BF16, DecodeNvfp4<MOQ_BF16>>), grid, block, 0, S(stream), x, packed,
                         (DecodeNvfp4<MOQ_BF16>{reinterpret_cast<const uint8_t*>(scales), scale_2, 0.0f, {0.0f, 0.0f}}), bias, y, (int)t, n,
                         k);
    } else {
      hipLaunchKernelGGL((wq_linear_kernel<MOQ_F16, DecodeNvfp4<MOQ_F16>>), grid, block, 0, S(stream), x, packed,
                         (DecodeNvfp4<MOQ_F16>{reinterpret_cast<const uint8_t*>(scales), scale_2, 0.0f, {0.0f, 0.0f}}), bias, y, (int)t, n,
                         k);
    }
  }
  return check_launch("moq_wq_linear");
}
