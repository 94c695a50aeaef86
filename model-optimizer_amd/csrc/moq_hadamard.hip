// moq_hadamard.hip -- normalized fast Walsh-Hadamard transform over blocks of the last dimension (the "rotate" of
// TensorQuantizer), alone and fused with the dynamic MX / NVFP4 block QDQ that follows it.
//
// The arithmetic, per contiguous block of B = 2^k elements (2 <= B <= 16384, cols % B == 0), is fixed bit for bit:
//   1. the block is converted to fp32;
//   2. for h = 1, 2, 4, ..., B/2 in this order, for every i with (i & h) == 0:
//          (v[i], v[i+h]) <- (v[i] + v[i+h], v[i] - v[i+h])          each one IEEE fp32 add, no contraction, no flushing;
//   3. v[i] <- v[i] * scale, scale = float32(B ** -0.5) computed by the host;
//   4. one RNE rounding to the tensor's dtype.
// This is H_B in Sylvester (natural) order.  a - b is computed as a + (-b), which IEEE defines to be the same value.
//
// Layout: the chunk skeleton of moq_chunk.h.  Packet u of thread t covers elements (u * 256 + t) * kVec ... of the
// chunk, so the index of an element inside its chunk splits, low bits first, into
//     [ in-packet: log2 kVec bits | lane: 6 bits | wave: 2 bits | packet u: 2..4 bits ]
// and the ascending stride order of the definition is the natural order of this layout:
//   * strides inside a packet are register butterflies;
//   * strides across lanes are xor exchanges: distance 1 and 2 by DPP quad_perm, 8 by DPP row_ror:8, 4 and 16 by
//     ds_swizzle (bit-mask mode), 32 by __shfl_xor.  (row_mirror / row_half_mirror, which the abs-max butterflies use, are
//     not xor partners and would be wrong here.)  The lane whose index has the stride bit set holds a - b with a from
//     the partner: it negates its own value and adds the partner's.
// In-wave tier (B <= 512 for 16-bit types, <= 256 for f32): a wave's packet holds whole blocks; nothing else is needed.
// LDS tier (up to 16384): a workgroup owns a tile of max(B, 8192) elements.  After the in-wave stages the two WAVE bits
//   are exchanged through LDS in one round: every thread writes its fp32 values, and after one barrier reads the values
//   the other waves hold at its own (packet, lane, element) position and forms both stages' sums in the order of the
//   definition.  The strides above that are the PACKET bits: butterflies between registers of one thread.
//   LDS index: the tile is stored as 16-byte slots [packet u][wave w][plane q = element / 4][lane], so a wave's
//   ds_write_b128 / ds_read_b128 touches 64 consecutive slots (1 KiB, every bank exactly once per 16-lane group):
//   free of bank conflicts for the writes and for the reads of another wave's data alike.  (Storing a 16-bit packet's
//   eight floats contiguously would put lanes 32 bytes apart: a two-way conflict.)  32 KiB, 64 KiB for B = 16384.
// Generic fallback (pointers that are not 16-byte aligned): one workgroup per block, the block in LDS, one barrier per
//   stride.  Same arithmetic; slow, and only for odd views.
#include "moq_common.h"
#include "moq_chunk.h"
#include "moq_mx.h"

namespace moq {

constexpr int kHadMaxLog = 14;  // B <= 16384: 64 KiB of fp32 in LDS

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  const int b = (int)__float_as_uint(v);
  return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(b, b, CTRL, 0xF, 0xF, false));
}
// the value lane (l ^ D) holds
template <int D>
__device__ __forceinline__ float xor_lane(float v) {
  if constexpr (D == 1) return dpp_f32<0xB1>(v);        // quad_perm [1,0,3,2]
  else if constexpr (D == 2) return dpp_f32<0x4E>(v);   // quad_perm [2,3,0,1]
  else if constexpr (D == 8) return dpp_f32<0x128>(v);  // row_ror:8 (a row is 16 lanes: rotating by 8 is xor 8)
  else if constexpr (D == 4) return __uint_as_float((uint32_t)__builtin_amdgcn_ds_swizzle((int)__float_as_uint(v), 0x101F));
  else if constexpr (D == 16) return __uint_as_float((uint32_t)__builtin_amdgcn_ds_swizzle((int)__float_as_uint(v), 0x401F));
  else return __shfl_xor(v, 32, 64);
}
template <int D, int V>
__device__ __forceinline__ void lane_stage(float (&v)[8], int lane) {
  const uint32_t neg = (lane & D) ? 0x80000000u : 0u;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const float o = xor_lane<D>(v[i]);
    v[i] = o + __uint_as_float(__float_as_uint(v[i]) ^ neg);  // stride bit clear: a + b;  set: a + (-b), a from the partner
  }
}
// strides 1 .. min(B, wave span) / 2 of one packet per lane; logb = log2 B (wave-uniform)
template <int DT>
__device__ __forceinline__ void wave_fwht(float (&v)[8], int logb, int lane) {
  constexpr int V = Elem<DT>::kVec;
  constexpr int LV = V == 8 ? 3 : 2;
#pragma unroll
  for (int s = 0; s < LV; ++s) {
    if (logb > s) {
      const int h = 1 << s;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        if ((i & h) == 0) {
          const float a = v[i], b = v[i + h];
          v[i] = a + b;
          v[i + h] = a - b;
        }
      }
    }
  }
  if (logb > LV) lane_stage<1, V>(v, lane);
  if (logb > LV + 1) lane_stage<2, V>(v, lane);
  if (logb > LV + 2) lane_stage<4, V>(v, lane);
  if (logb > LV + 3) lane_stage<8, V>(v, lane);
  if (logb > LV + 4) lane_stage<16, V>(v, lane);
  if (logb > LV + 5) lane_stage<32, V>(v, lane);
}
template <int DT>
__device__ __forceinline__ Pack16 scale_pack(float (&v)[8], float scale) {
#pragma unroll
  for (int i = 0; i < Elem<DT>::kVec; ++i) v[i] = v[i] * scale;
  return pack<DT>(v);
}
// s_red: kBlock / kWave words of LDS nobody else is using any more
__device__ __forceinline__ void publish_amax(uint32_t acc, float* running_amax, uint32_t* s_red) {
  acc = block_max_u32(acc, s_red);
  // the buffer holds a non-negative float or NaN: patterns order like the values, every NaN above +inf (moq_amax)
  // Same-address atomics retire slowly, and most workgroups bring nothing new: the buffer only ever grows, so a value read
  // from it now (possibly stale, hence possibly too small) that is already >= ours makes the atomic a no-op.
  if (threadIdx.x == 0) {
    uint32_t* out = reinterpret_cast<uint32_t*>(running_amax);
    if (acc > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, acc);
  }
}

// ------------------------------------------------------------------------------------------------ in-wave tier
template <int DT, bool FAST>
__device__ __forceinline__ void had_wave_chunk(const void* x, void* y, int64_t e0, int64_t n, int logb, float scale,
                                               uint32_t& amax) {
  constexpr int P = Chunk<DT>::kPackets;
  const int lane = threadIdx.x & 63;
  Pack16 in[P];
#pragma unroll
  for (int u = 0; u < P; ++u) in[u] = ld_packet<DT, FAST>(x, e0 + packet_off<DT>(u), n);
#pragma unroll
  for (int u = 0; u < P; ++u) {
    float v[8];
    unpack<DT>(in[u], v);
    wave_fwht<DT>(v, logb, lane);
    const Pack16 out = scale_pack<DT>(v, scale);
    const uint32_t m = pack_absmax<DT>(out);
    amax = m > amax ? m : amax;
    st_packet<DT, FAST>(y, e0 + packet_off<DT>(u), n, out);
  }
}
template <int DT>
__global__ __launch_bounds__(kBlock) void had_wave_kernel(const void* x, void* y, int64_t n,
                                                          int logb, float scale, float* __restrict__ running_amax) {
  __shared__ uint32_t s_red[kBlock / kWave];
  const int64_t n_chunks = (n + MOQ_MT_CHUNK - 1) / MOQ_MT_CHUNK;
  uint32_t amax = 0u;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t e0 = c * MOQ_MT_CHUNK;
    // a partial last chunk holds whole blocks but, for B below the packet width, possibly a partial packet: guarded
    // element accesses, zeros past the end (they only meet each other in the butterflies)
    if (e0 + MOQ_MT_CHUNK <= n) had_wave_chunk<DT, true>(x, y, e0, n, logb, scale, amax);
    else had_wave_chunk<DT, false>(x, y, e0, n, logb, scale, amax);
  }
  if (running_amax != nullptr) publish_amax(amax, running_amax, s_red);
}

// ------------------------------------------------------------------------------------------------ LDS tier
template <int DT, int LOGB>
__global__ __launch_bounds__(kBlock) void had_lds_kernel(const void* x, void* y, int64_t n,
                                                         float scale, float* __restrict__ running_amax) {
  constexpr int V = Elem<DT>::kVec;
  constexpr int ES = 16 / V;
  constexpr int Q = V / 4;                        // 16-byte planes of a packet's fp32 values
  constexpr int WL = (V == 8 ? 3 : 2) + 6;        // log2 of the elements a wave's packet spans
  constexpr int NW = LOGB - WL >= 2 ? 2 : 1;      // wave bits below B
  constexpr int NU = LOGB - WL - 2 > 0 ? LOGB - WL - 2 : 0;  // packet bits below B
  constexpr int TILE = (1 << LOGB) > MOQ_MT_CHUNK ? (1 << LOGB) : MOQ_MT_CHUNK;
  constexpr int P = TILE / (kBlock * V);
  static_assert(LOGB > WL && LOGB <= kHadMaxLog && (1 << NU) <= P, "tier bounds");
  extern __shared__ float4 s_x[];  // [P][4 waves][Q][64 lanes]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const char* xb = reinterpret_cast<const char*>(x);
  char* yb = reinterpret_cast<char*>(y);
  const int64_t n_tiles = (n + TILE - 1) / TILE;
  uint32_t amax = 0u;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t e0 = t * TILE;
    Pack16 in[P];
    // n is a multiple of B >= the packet width: a packet is entirely live or entirely past the end
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int64_t e = e0 + packet_off<DT>(u);
      if (e < n) in[u] = load16_nt(xb + e * ES);
      else in[u].w[0] = in[u].w[1] = in[u].w[2] = in[u].w[3] = 0u;
    }
    float v[P][8];
#pragma unroll
    for (int u = 0; u < P; ++u) {
      unpack<DT>(in[u], v[u]);
      wave_fwht<DT>(v[u], WL, lane);
#pragma unroll
      for (int q = 0; q < Q; ++q)
        s_x[((u * 4 + w) * Q + q) * 64 + lane] = make_float4(v[u][4 * q], v[u][4 * q + 1], v[u][4 * q + 2], v[u][4 * q + 3]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < P; ++u) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        float* o = &v[u][4 * q];
        if constexpr (NW == 1) {
          const float4 b = s_x[((u * 4 + (w ^ 1)) * Q + q) * 64 + lane];
          const float other[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = (w & 1) ? other[i] - o[i] : o[i] + other[i];
        } else {
          // stride bit 0 of the wave index first (pairs 0|1 and 2|3), then bit 1, as the definition orders them
          const float4 a0 = s_x[((u * 4 + 0) * Q + q) * 64 + lane], a1 = s_x[((u * 4 + 1) * Q + q) * 64 + lane];
          const float4 a2 = s_x[((u * 4 + 2) * Q + q) * 64 + lane], a3 = s_x[((u * 4 + 3) * Q + q) * 64 + lane];
          const float x0[4] = {a0.x, a0.y, a0.z, a0.w}, x1[4] = {a1.x, a1.y, a1.z, a1.w};
          const float x2[4] = {a2.x, a2.y, a2.z, a2.w}, x3[4] = {a3.x, a3.y, a3.z, a3.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float lo = (w & 1) ? x0[i] - x1[i] : x0[i] + x1[i];
            const float hi = (w & 1) ? x2[i] - x3[i] : x2[i] + x3[i];
            o[i] = (w & 2) ? lo - hi : lo + hi;
          }
        }
      }
    }
    __syncthreads();  // the next tile's writes must not overtake these reads
#pragma unroll
    for (int s = 0; s < NU; ++s) {
#pragma unroll
      for (int u = 0; u < P; ++u) {
        if ((u & (1 << s)) == 0) {
#pragma unroll
          for (int i = 0; i < V; ++i) {
            const float a = v[u][i], b = v[u + (1 << s)][i];
            v[u][i] = a + b;
            v[u + (1 << s)][i] = a - b;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int64_t e = e0 + packet_off<DT>(u);
      const Pack16 out = scale_pack<DT>(v[u], scale);
      const uint32_t m = pack_absmax<DT>(out);
      amax = m > amax ? m : amax;
      if (e < n) store16_nt(yb + e * ES, out);
    }
  }
  // (every read of the tile is behind the loop's last barrier: its first words serve the reduction)
  if (running_amax != nullptr) publish_amax(amax, running_amax, reinterpret_cast<uint32_t*>(s_x));
}

// ------------------------------------------------------------------------------------------------ generic fallback
template <int DT>
__global__ __launch_bounds__(kBlock) void had_generic_kernel(const void* x, void* y,
                                                             int64_t n_blocks, int logb, float scale,
                                                             float* __restrict__ running_amax) {
  extern __shared__ float s_v[];  // max(B, 4) floats
  const int B = 1 << logb;
  uint32_t amax = 0u;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const int64_t base = blk * B;
    for (int i = threadIdx.x; i < B; i += kBlock) s_v[i] = load1<DT>(x, base + i);
    __syncthreads();
    for (int s = 0; s < logb; ++s) {
      const int h = 1 << s;
      for (int p = threadIdx.x; p < B / 2; p += kBlock) {
        const int i = ((p >> s) << (s + 1)) | (p & (h - 1));
        const float a = s_v[i], b = s_v[i + h];
        s_v[i] = a + b;
        s_v[i + h] = a - b;
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < B; i += kBlock) {
      const float r = round_to_dtype<DT>(s_v[i] * scale);
      store1<DT>(y, base + i, r);
      const uint32_t m = absbits(r);
      amax = m > amax ? m : amax;
    }
    __syncthreads();
  }
  if (running_amax != nullptr) publish_amax(amax, running_amax, reinterpret_cast<uint32_t*>(s_v));
}

// ------------------------------------------------------------------------------------------------ fused with the MX block QDQ
// transform -> rounding to the dtype -> dynamic block QDQ of mx_chunk (moq_formats.hip) on the rounded values ->
// optionally the transform again: what the three standalone launches write, without leaving registers.
template <int DT, int LPG, bool HW4, class ScaleFn>
__device__ __forceinline__ void had_mx_chunk(const char* xb, char* yb, int64_t e0, int64_t n, int logb, float scale,
                                             const MxFmt f, const ScaleFn& scale_of, bool rotate_back) {
  constexpr int V = Elem<DT>::kVec;
  constexpr int P = Chunk<DT>::kPackets;
  constexpr int ES = 16 / V;
  const int lane = threadIdx.x & 63;
  Pack16 in[P];
  // n is a multiple of the rotation block, itself a multiple of the QDQ block (= LPG * V elements)
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const int64_t e = e0 + packet_off<DT>(u);
    if (e < n) in[u] = load16_nt(xb + e * ES);
    else in[u].w[0] = in[u].w[1] = in[u].w[2] = in[u].w[3] = 0u;
  }
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const int64_t e = e0 + packet_off<DT>(u);
    float v[8];
    unpack<DT>(in[u], v);
    wave_fwht<DT>(v, logb, lane);
    const Pack16 rot = scale_pack<DT>(v, scale);  // the rotated tensor AS STORED
    unpack<DT>(rot, v);
    if constexpr (HW4) {
      if (!mx_e2m1_hw<V>(v, group_max_u32<LPG>(pack_absmax<DT>(rot)))) mx_packet_general<DT, LPG>(v, f, scale_of);
    } else {
      mx_packet_general<DT, LPG>(v, f, scale_of);
    }
    Pack16 out = pack<DT>(v);
    if (rotate_back) {  // (uniform)
      unpack<DT>(out, v);
      wave_fwht<DT>(v, logb, lane);
      out = scale_pack<DT>(v, scale);
    }
    if (e < n) store16_nt(yb + e * ES, out);
  }
}
// TWO_LEVEL: an element format as the scale format, optional tensor-wide amax (NVFP4-style); else E8M0 scales.
// FMT / SFMT >= 0 fix the element / scale format at compile time so that the rounding constants fold (NVFP4, MXFP4, MXFP8: the
// specialisations mx_kernel / mx_two_level_kernel have); < 0 read them from the arguments.
template <int DT, int LPG, bool TWO_LEVEL, int FMT, int SFMT>
__global__ __launch_bounds__(kBlock) void had_mx_kernel(const void* x, void* y, int64_t n,
                                                        int logb, float scale, int fmt, int scale_fmt,
                                                        const float* __restrict__ global_amax, int rotate_back) {
  __shared__ float2 s_table[8];
  const MxFmt f = mx_fmt(FMT >= 0 ? FMT : fmt);
  const char* xb = reinterpret_cast<const char*>(x);
  char* yb = reinterpret_cast<char*>(y);
  const int64_t n_chunks = (n + MOQ_MT_CHUNK - 1) / MOQ_MT_CHUNK;
  const bool back = rotate_back != 0;
  if constexpr (TWO_LEVEL) {
    const MxFmt sf = mx_fmt(SFMT >= 0 ? SFMT : scale_fmt);
    if (global_amax != nullptr && sf.kind != 2 && sf.m <= 3) {  // (workgroup-uniform) the table of MxScaleTwoLevelTable
      const float g = *global_amax;
      const bool g_bad = mx_bad_amax(g);
      const double two_level = (double)sf.maxv * (double)(f.maxv / g);
      if (threadIdx.x < 8 && !g_bad) {
        const double q = (double)(float)(8 + threadIdx.x) / two_level;
        s_table[threadIdx.x] = make_float2((float)q, (float)(1.0 / q));
      }
      __syncthreads();
      const MxScaleTwoLevelTable scale_of{f.maxv, sf, global_amax, two_level, g_bad, s_table};
      for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x)
        had_mx_chunk<DT, LPG, false>(xb, yb, c * MOQ_MT_CHUNK, n, logb, scale, f, scale_of, back);
      return;
    }
    const MxScaleGeneral scale_of{f.maxv, sf, global_amax};
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x)
      had_mx_chunk<DT, LPG, false>(xb, yb, c * MOQ_MT_CHUNK, n, logb, scale, f, scale_of, back);
  } else {
    const MxScaleE8M0 scale_of{f.maxv};
    // MXFP4 at up to 8 lanes per block runs on the chip's scaled FP4 converters, as in mx_kernel
    if (LPG <= 8 && (FMT >= 0 ? FMT : fmt) == MOQ_E2M1) {
      for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x)
        had_mx_chunk<DT, LPG, true>(xb, yb, c * MOQ_MT_CHUNK, n, logb, scale, f, scale_of, back);
    } else {
      for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x)
        had_mx_chunk<DT, LPG, false>(xb, yb, c * MOQ_MT_CHUNK, n, logb, scale, f, scale_of, back);
    }
  }
}

}  // namespace moq

// ================================================================================================
// C-ABI
// ================================================================================================
using namespace moq;
static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// 0 = fine; else the status to return (message set)
static int had_check(const char* who, const void* x, const void* y, int64_t rows, int64_t cols, int block, int dt) {
  if (rows < 0 || cols < 0 || (rows > 0 && cols > 0 && (x == nullptr || y == nullptr))) {
    set_error("%s: bad arguments", who);
    return MOQ_ERR_INVALID;
  }
  if (dt != MOQ_F32 && dt != MOQ_F16 && dt != MOQ_BF16) {
    set_error("%s: unknown dtype code %d", who, dt);
    return MOQ_ERR_INVALID;
  }
  if (block < 2 || (block & (block - 1)) != 0) {
    set_error("%s: the rotation block must be a power of two >= 2, got %d", who, block);
    return MOQ_ERR_INVALID;
  }
  if (block > (1 << kHadMaxLog)) {
    set_error("%s: rotation blocks above %d are not supported, got %d", who, 1 << kHadMaxLog, block);
    return MOQ_ERR_UNSUPPORTED;
  }
  if (cols % block != 0) {
    set_error("%s: cols = %lld is not divisible by the rotation block %d", who, (long long)cols, block);
    return MOQ_ERR_INVALID;
  }
  return MOQ_OK;
}

extern "C" int moq_hadamard(const void* x, void* y, int64_t rows, int64_t cols, int block, float scale, int dt,
                            float* running_amax, void* stream) {
  if (const int rc = had_check("moq_hadamard", x, y, rows, cols, block, dt)) return rc;
  const int64_t n = rows * cols;
  if (n == 0) return MOQ_OK;
  const int logb = log2_or_neg(block);
  const int wave_log = dt == MOQ_F32 ? 8 : 9;
  const bool aligned = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0;
  // with a running abs-max a workgroup walks several chunks and publishes ONE atomic (same-address atomics are slow)
  const int64_t grid_cap = running_amax != nullptr ? 8192 : 0x7FFFFFFF;
  if (!aligned) {
    const int64_t nb = n / block;
    const int grid = (int)(nb < 8192 ? nb : 8192);
    MOQ_DISPATCH_DTYPE(dt, hipLaunchKernelGGL((had_generic_kernel<DT>), dim3(grid), dim3(kBlock), (size_t)(block < 4 ? 4 : block) * sizeof(float),
                                              S(stream), x, y, nb, logb, scale, running_amax));
  } else if (logb <= wave_log) {
    int64_t grid = copy_grid64((n + MOQ_MT_CHUNK - 1) / MOQ_MT_CHUNK);
    if (grid > grid_cap) grid = grid_cap;
    MOQ_DISPATCH_DTYPE(dt, hipLaunchKernelGGL((had_wave_kernel<DT>), dim3((int)grid), dim3(kBlock), 0, S(stream), x, y, n,
                                              logb, scale, running_amax));
  } else {
    const int64_t tile = block > MOQ_MT_CHUNK ? block : MOQ_MT_CHUNK;
    int64_t grid = copy_grid64((n + tile - 1) / tile);
    if (grid > grid_cap) grid = grid_cap;
#define MOQ_HAD_LDS(L)                                                                                                   \
  case L:                                                                                                                \
    hipLaunchKernelGGL((had_lds_kernel<DT, (L > WLOG ? L : WLOG + 1)>), dim3((int)grid), dim3(kBlock),                   \
                       (size_t)tile * sizeof(float), S(stream), x, y, n, scale, running_amax);                           \
    break;
#define MOQ_HAD_LDS_SWITCH                                                                                               \
  switch (logb) {                                                                                                        \
    MOQ_HAD_LDS(9) MOQ_HAD_LDS(10) MOQ_HAD_LDS(11) MOQ_HAD_LDS(12) MOQ_HAD_LDS(13) MOQ_HAD_LDS(14)                         \
    default: set_error("unreachable"); return MOQ_ERR_INVALID;                                                           \
  }
    switch (dt) {
      case MOQ_F32: { constexpr int DT = MOQ_F32; constexpr int WLOG = 8; MOQ_HAD_LDS_SWITCH } break;
      case MOQ_F16: { constexpr int DT = MOQ_F16; constexpr int WLOG = 9; MOQ_HAD_LDS_SWITCH } break;
      default: { constexpr int DT = MOQ_BF16; constexpr int WLOG = 9; MOQ_HAD_LDS_SWITCH } break;
    }
#undef MOQ_HAD_LDS_SWITCH
#undef MOQ_HAD_LDS
  }
  return check_launch("moq_hadamard");
}

extern "C" int moq_hadamard_mx_qdq(const void* x, void* y, int64_t rows, int64_t cols, int rot_block, float scale,
                                   int block, int dt, int fmt, int scale_fmt, const float* global_amax, int rotate_back,
                                   void* stream) {
  if (const int rc = had_check("moq_hadamard_mx_qdq", x, y, rows, cols, rot_block, dt)) return rc;
  if (block <= 0) {
    set_error("moq_hadamard_mx_qdq: bad arguments");
    return MOQ_ERR_INVALID;
  }
  if (scale_fmt == MOQ_E8M0 ? global_amax != nullptr : mx_fmt(scale_fmt).kind < 0) {
    set_error("moq_hadamard_mx_qdq: block scales are E8M0 (no global amax) or an element format "
              "(E4M3, ...; optional global amax)");
    return MOQ_ERR_UNSUPPORTED;
  }
  if (mx_fmt(fmt).kind < 0) {
    set_error("moq_hadamard_mx_qdq: unknown element format %d", fmt);
    return MOQ_ERR_INVALID;
  }
  const int vec = dt == MOQ_F32 ? 4 : 8;
  const int lpg = block / vec;
  const bool aligned = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0;
  const bool two_level = scale_fmt != MOQ_E8M0;
  if (!aligned || rot_block > 64 * vec || rot_block % block != 0 || block % vec != 0 || (lpg & (lpg - 1)) != 0 ||
      lpg > (two_level ? 8 : 64)) {
    set_error("moq_hadamard_mx_qdq: fused for 16-byte aligned tensors, rotation blocks up to %d and QDQ blocks that divide "
              "them in the fast layouts of moq_mx_fused_amax_convert (rot_block %d, block %d): compose moq_hadamard and "
              "moq_mx_fused_amax_convert", 64 * vec, rot_block, block);
    return MOQ_ERR_UNSUPPORTED;
  }
  const int64_t n = rows * cols;
  if (n == 0) return MOQ_OK;
  const int logb = log2_or_neg(rot_block);
  const int grid = copy_grid((n + MOQ_MT_CHUNK - 1) / MOQ_MT_CHUNK);
#define MOQ_HADMX_LAUNCH(L, TL, F, SF)                                                                                    \
  MOQ_DISPATCH_DTYPE(dt, hipLaunchKernelGGL((had_mx_kernel<DT, L, TL, F, SF>), dim3(grid), dim3(kBlock), 0, S(stream), x, y, n, \
                                            logb, scale, fmt, scale_fmt, global_amax, rotate_back))
#define MOQ_HADMX2_CASE(L)                                                                          \
  case L:                                                                                           \
    if (fmt == MOQ_E2M1 && scale_fmt == MOQ_E4M3) { MOQ_HADMX_LAUNCH(L, true, MOQ_E2M1, MOQ_E4M3); } \
    else { MOQ_HADMX_LAUNCH(L, true, -1, -1); }                                                      \
    break;
#define MOQ_HADMX_CASE(L)                                                                              \
  case L:                                                                                              \
    if (L <= 8 && fmt == MOQ_E2M1) { MOQ_HADMX_LAUNCH(L, false, (L <= 8 ? MOQ_E2M1 : -1), -1); }        \
    else if (L <= 8 && fmt == MOQ_E4M3) { MOQ_HADMX_LAUNCH(L, false, (L <= 8 ? MOQ_E4M3 : -1), -1); }   \
    else { MOQ_HADMX_LAUNCH(L, false, -1, -1); }                                                        \
    break;
  if (two_level) {
    switch (lpg) {
      MOQ_HADMX2_CASE(1) MOQ_HADMX2_CASE(2) MOQ_HADMX2_CASE(4) MOQ_HADMX2_CASE(8)
      default: set_error("unreachable"); return MOQ_ERR_INVALID;
    }
  } else {
    switch (lpg) {
      MOQ_HADMX_CASE(1) MOQ_HADMX_CASE(2) MOQ_HADMX_CASE(4) MOQ_HADMX_CASE(8)
      MOQ_HADMX_CASE(16) MOQ_HADMX_CASE(32) MOQ_HADMX_CASE(64)
      default: set_error("unreachable"); return MOQ_ERR_INVALID;
    }
  }
#undef MOQ_HADMX2_CASE
#undef MOQ_HADMX_LAUNCH
#undef MOQ_HADMX_CASE
  return check_launch("moq_hadamard_mx_qdq");
}
