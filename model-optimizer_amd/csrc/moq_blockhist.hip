// moq_blockhist.hip -- moq_block_amax_log2_hist: the collect pass of the NVFP4 activation headroom calibrator
// (calib/nvfp4_act_headroom.py:116-149) as ONE read of the activation: the abs-max of every block of 16, its bin in the
// log2 histogram, the running per-tensor max and the NaN / Inf check.
//
// No log2 on the device.  The reference bins with floor((log2(v) - lo) / (hi - lo) * bins) in fp32 on the host, an
// expression that is monotone in v, so bin k begins at ONE fp32 value: the host bisects the `bins - 1` edges out of the
// reference's own expression and the kernel only compares bit patterns (positive floats order like their patterns).
// The search is indexed by the exponent first: lo[e] = number of edges below 2^(e - 127), so an amax of exponent e only
// has the edges of its own octave left (6.4 per octave with 512 bins over 80 octaves: three halving steps).
//
// Data path: the chunk skeleton of moq_chunk.h (16-byte packets, all loads of a chunk before the first use).  A block of
// 16 is two adjacent lanes (16-bit) or four (fp32), settled by DPP quad_perm maxima; every lane then bins ONE block of its
// lane group (lane j of the group takes packet j), so no lane idles at the LDS atomic.  Counts live in R interleaved LDS
// copies of u32 counters (as the |x| histogram, moq_hist.h) and are flushed with 64-bit global atomics.
#include "moq_chunk.h"

namespace moq {
namespace {

constexpr int kBhBlock = 1024;                 // 16 waves around one LDS histogram; each 256-thread quarter walks chunks
constexpr int kBhMaxBins = 4096;               // thresholds 16 KiB + counters <= 32 KiB + exponent table 1 KiB of LDS
constexpr int kBhCounterWords = 8192;          // LDS words the counter copies may take
constexpr int kBhMisc = 3;                     // LDS words of BhLds::misc
// a workgroup adds at most 4 quarters x 512 blocks per iteration to its u32 counters: flush every 2^20 iterations (2^31)
constexpr int64_t kBhFlushIters = 1ll << 20;

template <int DT>
struct BhGeom {
  static constexpr int kLanes = 16 / Elem<DT>::kVec;  // lanes that share one block of 16: 2 (16-bit) or 4 (fp32)
  static constexpr int kGroups = Chunk<DT>::kPackets / kLanes;
  static_assert(kGroups * kLanes == Chunk<DT>::kPackets, "packets of a chunk must split into lane groups");
};

struct BhLds {
  uint32_t* thr;   // [bins]      the bins - 1 edges, then a 0xFFFFFFFF sentinel
  uint32_t* lo;    // [257]       lo[e] = #{k : thr[k] < e << 23}
  uint32_t* cnt;   // [(bins + 1) << rshift]  counters; slot `bins` is the trash slot (zero / non-finite / past the end)
  uint32_t* misc;  // [0] the most edges one octave holds, [1] the workgroup's abs-max pattern, [2] its NaN / Inf flag
};

// bin of a finite non-zero abs-max pattern `a`: #{k : thr[k] <= a}
__device__ __forceinline__ int bh_bin(uint32_t a, const BhLds& s, int bins, int top_step) {
  uint32_t pos = s.lo[a >> 23];
  // edges at or past the next octave are > a and the sentinel ends the table, so no upper limit is needed
  for (int step = top_step; step > 0; step >>= 1) {
    const uint32_t j = pos + (uint32_t)step - 1u;
    const uint32_t t = s.thr[j < (uint32_t)bins - 1u ? j : (uint32_t)bins - 1u];
    pos = t <= a ? pos + (uint32_t)step : pos;
  }
  return (int)pos;
}

template <int DT, bool FAST>
__device__ __forceinline__ void bh_chunk(const void* x, int64_t e0, int64_t n, const BhLds& s, int bins, int top_step,
                                         int rshift, int copy, uint32_t& run_max, uint32_t& bad) {
  constexpr int V = Elem<DT>::kVec;
  constexpr int P = Chunk<DT>::kPackets;
  constexpr int L = BhGeom<DT>::kLanes;
  const int tid = threadIdx.x & (kBlock - 1);
  Pack16 in[P];
#pragma unroll
  for (int u = 0; u < P; ++u) in[u] = ld_packet<DT, FAST>(x, e0 + (int64_t)(u * kBlock + tid) * V, n);
  uint32_t gm[P];
#pragma unroll
  for (int u = 0; u < P; ++u) gm[u] = group_max_u32<L>(pack_absmax<DT>(in[u]));
  const int sub = tid & (L - 1);
#pragma unroll
  for (int g = 0; g < P / L; ++g) {
    uint32_t a = gm[g * L];
#pragma unroll
    for (int j = 1; j < L; ++j) a = sub == j ? gm[g * L + j] : a;
    const bool finite = a < 0x7F800000u;
    // bit 0: NaN, bit 1: Inf -- of the block's abs-max: a NaN pattern is the larger, so a block with both reports NaN
    bad |= finite ? 0u : a > 0x7F800000u ? 1u : 2u;
    const uint32_t av = finite ? a : 0u;
    run_max = av > run_max ? av : run_max;
    const int b = bh_bin(av, s, bins, top_step);
    atomicAdd(&s.cnt[((av != 0u ? b : bins) << rshift) + copy], 1u);
  }
}

template <int DT>
__global__ __launch_bounds__(kBhBlock) void block_amax_log2_hist_kernel(
    const void* __restrict__ x, int64_t n, const uint32_t* __restrict__ thresholds, int bins,
    unsigned long long* __restrict__ counts, uint32_t* __restrict__ running_max, uint32_t* __restrict__ bad_flag,
    int rshift) {
  extern __shared__ __attribute__((aligned(16))) uint32_t bh_lds[];
  BhLds s;
  s.thr = bh_lds;
  s.lo = s.thr + bins;
  s.misc = s.lo + 257;
  s.cnt = s.misc + kBhMisc;
  const int slots = (bins + 1) << rshift;
  for (int k = threadIdx.x; k < bins; k += kBhBlock) s.thr[k] = k < bins - 1 ? thresholds[k] : 0xFFFFFFFFu;
  for (int k = threadIdx.x; k < slots; k += kBhBlock) s.cnt[k] = 0;
  if (threadIdx.x < kBhMisc) s.misc[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x <= 256) {  // lower bound of (e << 23) among the edges
    const uint32_t key = (uint32_t)threadIdx.x << 23;
    int a = 0, b = bins - 1;
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (s.thr[mid] < key) a = mid + 1; else b = mid;
    }
    s.lo[threadIdx.x] = (uint32_t)a;
  }
  __syncthreads();
  if (threadIdx.x < 256) atomicMax(&s.misc[0], s.lo[threadIdx.x + 1] - s.lo[threadIdx.x]);
  __syncthreads();
  int top_step = 0;  // the largest power of two <= the fullest octave: steps top, top / 2, .., 1 reach 2 * top - 1 edges
  {
    const int kmax = __builtin_amdgcn_readfirstlane((int)s.misc[0]);
    while ((2 << top_step) <= kmax) ++top_step;
    top_step = kmax > 0 ? 1 << top_step : 0;
  }

  const int copy = (int)(threadIdx.x & ((1u << rshift) - 1u));
  // the host entry refuses an unaligned x, so `al` holds and the guarded path is the tail chunk's alone; the test stays so
  // that the kernel is safe on its own terms
  const bool al = aligned16(x);
  const int64_t n_chunks = (n + MOQ_MT_CHUNK - 1) / MOQ_MT_CHUNK;
  constexpr int Q = kBhBlock / kBlock;
  const int64_t stride = (int64_t)gridDim.x * Q;
  uint32_t run_max = 0, bad = 0;
  const int64_t first = (int64_t)blockIdx.x * Q;
  int64_t c = first + (threadIdx.x / kBlock);
  // rounds of at most kBhFlushIters chunks per quarter, a flush after each; the first quarter has the most chunks, so
  // its count decides for the whole workgroup (the barriers are uniform)
  const int64_t iters = first < n_chunks ? (n_chunks - first + stride - 1) / stride : 0;
  const int64_t rounds = iters > kBhFlushIters ? (iters + kBhFlushIters - 1) / kBhFlushIters : 1;
  for (int64_t round = 0; round < rounds; ++round) {
    for (int64_t it = 0; it < kBhFlushIters && c < n_chunks; ++it, c += stride) {
      const int64_t e0 = c * MOQ_MT_CHUNK;
      if (al && e0 + MOQ_MT_CHUNK <= n)
        bh_chunk<DT, true>(x, e0, n, s, bins, top_step, rshift, copy, run_max, bad);
      else
        bh_chunk<DT, false>(x, e0, n, s, bins, top_step, rshift, copy, run_max, bad);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += kBhBlock) {
      uint32_t cnt = 0;
      for (int r = 0; r < (1 << rshift); ++r) {
        cnt += s.cnt[(b << rshift) + r];
        s.cnt[(b << rshift) + r] = 0;
      }
      if (cnt) atomicAdd(&counts[b], (unsigned long long)cnt);
    }
    __syncthreads();
  }

  // running max and the NaN / Inf flag: one vector atomic each per workgroup, and only when they change something
  run_max = group_max_u32<64>(run_max);
  if ((threadIdx.x & 63) == 0) atomicMax(&s.misc[1], run_max);
  if (bad != 0u) atomicOr(&s.misc[2], bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s.misc[1] != 0u) atomicMax(running_max, s.misc[1]);
    if (s.misc[2] != 0u) atomicOr(bad_flag, s.misc[2]);
  }
}

}  // namespace
}  // namespace moq

using namespace moq;

extern "C" int moq_block_amax_log2_hist(const void* x, int64_t rows, int64_t cols, int dt, int block,
                                        const float* thresholds, int bins, unsigned long long* counts,
                                        float* running_max, int* bad, void* stream) {
  if (rows < 0 || cols < 0 || bins < 1 || !counts || !running_max || !bad || (bins > 1 && !thresholds) ||
      (rows * cols > 0 && !x)) {
    set_error("moq_block_amax_log2_hist: bad arguments");
    return MOQ_ERR_INVALID;
  }
  if (block != 16) {
    set_error("moq_block_amax_log2_hist: block size %d (only 16)", block);
    return MOQ_ERR_UNSUPPORTED;
  }
  if (cols % block != 0) {
    set_error("moq_block_amax_log2_hist: %lld columns are not whole blocks of %d (zero-pad the last dim)", (long long)cols,
              block);
    return MOQ_ERR_UNSUPPORTED;
  }
  if (bins > kBhMaxBins) {
    set_error("moq_block_amax_log2_hist: %d bins (at most %d)", bins, kBhMaxBins);
    return MOQ_ERR_UNSUPPORTED;
  }
  if (((uintptr_t)x & 15u) || ((uintptr_t)thresholds & 3u) || ((uintptr_t)counts & 7u)) {
    set_error("moq_block_amax_log2_hist: x must be 16-byte, thresholds 4-byte, counts 8-byte aligned");
    return MOQ_ERR_UNSUPPORTED;
  }
  const int64_t n = rows * cols;
  if (n == 0) return MOQ_OK;
  const int64_t n_chunks = (n + MOQ_MT_CHUNK - 1) / MOQ_MT_CHUNK;
  // <= 512 workgroups of 1024 threads (two per CU), as the |x| histogram: the flush is one 64-bit atomic per non-empty bin
  int64_t grid = (n_chunks + 3) / 4;
  if (grid > 512) grid = 512;
  int rshift = 0;
  while (rshift < 3 && ((int64_t)(bins + 1) << (rshift + 1)) <= kBhCounterWords) ++rshift;
  const size_t lds = ((size_t)bins + 257 + kBhMisc + ((size_t)(bins + 1) << rshift)) * 4;
  hipStream_t st = (hipStream_t)stream;
  MOQ_DISPATCH_DTYPE(dt, hipLaunchKernelGGL(block_amax_log2_hist_kernel<DT>, dim3((int)grid), dim3(kBhBlock), lds, st, x, n,
                                            reinterpret_cast<const uint32_t*>(thresholds), bins, counts,
                                            reinterpret_cast<uint32_t*>(running_max),
                                            reinterpret_cast<uint32_t*>(bad), rshift));
  return check_launch("moq_block_amax_log2_hist");
}
