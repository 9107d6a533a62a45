// qc.exist_reversed_time / coerce_increasing_time: a time coordinate that steps backwards (a known EK60/EK80 defect: one
// ping earlier than its predecessor, the pinging interval undisturbed afterwards) found and repaired where it lies.
// Everything is integer arithmetic on the int64 ticks of the datetime64 values, wrapping like NumPy's: the result is the
// reference's bit for bit, whatever order the wavefronts run in.
//
//   epa_time_reversals    one thread per difference d[i] = t[i+1] - t[i]: how many are negative, where the first one is,
//                         how many times are NaT (INT64_MIN), and the list of the reversed differences.
//   epa_reversal_medians  one wavefront per listed reversal ni: the median of the ORIGINAL differences d[ni-win_len .. ni)
//                         (recomputed from the times, held in LDS, the two middle values found by exact rank counting)
//                         -> sub[ni].
//   epa_time_rebuild      with f the first reversal: out[: f+1] = t[: f+1], out[i+1] = t[f] + sum(d'[f .. i]), d' = sub at
//                         a reversal and d elsewhere.  Tile sums, one workgroup scanning them, apply: three launches, and no
//                         workgroup ever waits for another one of its own launch.
#include "epa_internal.h"

namespace {

using u64 = unsigned long long;
constexpr int64_t kNaT = INT64_MIN;
constexpr int kWaves = epa::kBlock / 64;
constexpr int kMedianGrid = EPA_QC_MEDIAN_WAVES / kWaves;  // workgroups of epa_reversal_medians, whatever the count
constexpr int kPer = 4;                                    // consecutive differences per thread of a scan tile
constexpr int kTile = EPA_QC_SCAN_TILE;
static_assert(kTile == epa::kBlock * kPer, "a scan tile is one workgroup's differences");
static_assert(EPA_QC_MEDIAN_WAVES % kWaves == 0, "whole workgroups");
static_assert(kWaves * EPA_QC_MAX_WIN * sizeof(int64_t) <= 32 * 1024, "the windows of a workgroup: half of LDS at most");

__device__ __forceinline__ int64_t wrap_sub(int64_t a, int64_t b) { return (int64_t)((u64)a - (u64)b); }

__global__ void __launch_bounds__(epa::kBlock)
time_reversals_kernel(const int64_t* __restrict__ t, long long N, int64_t* __restrict__ facts,
                      long long* __restrict__ list) {
  const long long i = (long long)blockIdx.x * epa::kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool nat = false, rev = false;
  if (i < N) {
    const int64_t a = t[i];
    nat = a == kNaT;
    if (i + 1 < N) {
      const int64_t b = t[i + 1];
      rev = !nat && b != kNaT && wrap_sub(b, a) < 0;
    }
  }
  // one atomic per wavefront and fact; a wavefront's reversals take consecutive slots of the list
  const u64 rev_mask = __ballot(rev), nat_mask = __ballot(nat);
  if (nat_mask && lane == 0) atomicAdd((u64*)&facts[EPA_QC_NAT], (u64)__popcll(nat_mask));
  if (!rev_mask) return;
  long long base = 0;
  if (lane == 0) {
    const u64 n = (u64)__popcll(rev_mask);
    atomicAdd((u64*)&facts[EPA_QC_COUNT], n);
    atomicMin((u64*)&facts[EPA_QC_FIRST], (u64)(i + __ffsll((long long)rev_mask) - 1));  // (lane 0: i is the wave's first)
    if (list) base = (long long)atomicAdd((u64*)&facts[EPA_QC_SLOTS], n);
  }
  if (list) {
    base = __shfl(base, 0, 64);
    if (rev) list[base + __popcll(rev_mask & ((1ull << lane) - 1ull))] = i;  // < N-1 slots: one per reversal
  }
}

// Truncating half of the wrapping sum of the two middle values: np.median of an even number of timedelta64
__device__ __forceinline__ int64_t mid_of(int64_t a, int64_t b) { return (int64_t)((u64)a + (u64)b) / 2; }

__global__ void __launch_bounds__(epa::kBlock)
reversal_medians_kernel(const int64_t* __restrict__ t, int win_len, const int64_t* __restrict__ facts,
                        const long long* __restrict__ list, int64_t* __restrict__ sub) {
  __shared__ int64_t win_all[kWaves][EPA_QC_MAX_WIN];
  __shared__ int64_t mid_all[kWaves][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t* win = win_all[wave];
  const long long count = facts[EPA_QC_COUNT];
  // every wavefront of a workgroup makes the same number of rounds (the barriers below), a wavefront past the count idles
  for (long long r0 = (long long)blockIdx.x * kWaves; r0 < count; r0 += (long long)gridDim.x * kWaves) {
    const long long r = r0 + wave;
    long long ni = 0, lo = 0;
    int n = 0;
    if (r < count) {
      ni = list[r];
      lo = ni > win_len ? ni - win_len : 0;
      n = (int)(ni - lo);  // 0 .. win_len <= EPA_QC_MAX_WIN; 0 (a reversal in the first difference): NaT is written
    }
    for (int j = lane; j < n; j += 64) win[j] = wrap_sub(t[lo + j + 1], t[lo + j]);
    __syncthreads();
    // rank of element j: how many are smaller, or equal and earlier -- a permutation of 0 .. n-1, so exactly one element
    // has the rank of the lower middle and one that of the upper middle (the same one when n is odd)
    const int k_lo = (n - 1) >> 1, k_hi = n >> 1;
    for (int j = lane; j < n; j += 64) {
      const int64_t v = win[j];
      int rank = 0;
      for (int i = 0; i < n; ++i) {
        const int64_t w = win[i];
        rank += (w < v) | ((w == v) & (i < j));
      }
      if (rank == k_lo) mid_all[wave][0] = v;
      if (rank == k_hi) mid_all[wave][1] = v;
    }
    __syncthreads();
    // (an empty window, the reversal in the first difference: NaT, the median of nothing -- every listed entry is written)
    if (lane == 0 && r < count)
      sub[ni] = n == 0 ? kNaT : (n & 1) ? mid_all[wave][0] : mid_of(mid_all[wave][0], mid_all[wave][1]);
  }
}

// d'[i] for i >= f, 0 before: the term of difference i in the sum behind the first reversal
__device__ __forceinline__ u64 term(const int64_t* __restrict__ t, const int64_t* __restrict__ sub, long long i,
                                    long long f) {
  if (i < f) return 0;
  const int64_t d = wrap_sub(t[i + 1], t[i]);
  return (u64)(d < 0 ? sub[i] : d);
}

__device__ __forceinline__ long long first_of(const int64_t* __restrict__ facts, long long N) {
  const long long f = facts[EPA_QC_FIRST];
  return f < 0 ? N : f;  // no reversal: every time is copied
}

// inclusive wrapping sum over the workgroup of one value per thread; *total: the workgroup's sum
__device__ __forceinline__ u64 block_scan(u64 v, u64* wsum, u64* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  __syncthreads();  // (wsum may still be read from the previous call)
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  u64 all = 0;
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) incl += wsum[w];
    all += wsum[w];
  }
  *total = all;
  return incl;
}

__global__ void __launch_bounds__(epa::kBlock)
time_tile_sums_kernel(const int64_t* __restrict__ t, long long N, const int64_t* __restrict__ facts,
                      const int64_t* __restrict__ sub, u64* __restrict__ tile_sum) {
  __shared__ u64 wsum[kWaves];
  const long long f = first_of(facts, N);
  const long long i0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kPer;
  u64 s = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (i0 + j < N - 1) s += term(t, sub, i0 + j, f);
  u64 total;
  block_scan(s, wsum, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// tile_sum -> the sum of all tiles BEFORE each one, in place: one workgroup, kBlock tiles per round
__global__ void __launch_bounds__(epa::kBlock)
time_tile_carry_kernel(u64* __restrict__ tile_sum, long long ntiles) {
  __shared__ u64 wsum[kWaves];
  u64 carry = 0;
  for (long long base = 0; base < ntiles; base += epa::kBlock) {
    const long long k = base + threadIdx.x;
    const u64 v = k < ntiles ? tile_sum[k] : 0;
    u64 total;
    const u64 incl = block_scan(v, wsum, &total);
    if (k < ntiles) tile_sum[k] = carry + incl - v;
    carry += total;
  }
}

__global__ void __launch_bounds__(epa::kBlock)
time_rebuild_kernel(const int64_t* __restrict__ t, long long N, const int64_t* __restrict__ facts,
                    const int64_t* __restrict__ sub, const u64* __restrict__ tile_carry, int64_t* __restrict__ out) {
  __shared__ u64 wsum[kWaves];
  const long long f = first_of(facts, N);
  const long long i0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kPer;
  u64 v[kPer], s = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (i0 + j < N - 1) s += term(t, sub, i0 + j, f);
    v[j] = s;
  }
  u64 total;
  const u64 before = block_scan(s, wsum, &total) - s + tile_carry[blockIdx.x];
  const u64 tf = f < N ? (u64)t[f] : 0;
  if (i0 == 0) out[0] = t[0];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const long long i = i0 + j;
    if (i < N - 1) out[i + 1] = i < f ? t[i + 1] : (int64_t)(tf + before + v[j]);
  }
}

}  // namespace

extern "C" int epa_time_reversals(const int64_t* t, long long N, int64_t* facts, long long* list, epa_stream_t stream) {
  EPA_CHECK_ARG(N >= 1, "epa_time_reversals: N=%lld times, at least 1 is needed", N);
  EPA_CHECK_ARG(t && facts, "epa_time_reversals: NULL array argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  EPA_CHECK_HIP(hipMemsetAsync(facts, 0, EPA_QC_FACTS * sizeof(int64_t), st));
  EPA_CHECK_HIP(hipMemsetAsync(facts + EPA_QC_FIRST, 0xff, sizeof(int64_t), st));  // -1, the largest unsigned value
  const long long grid = (N + epa::kBlock - 1) / epa::kBlock;
  EPA_CHECK_ARG(grid <= 0x7fffffffLL, "epa_time_reversals: N=%lld times are more than one launch takes", N);
  hipLaunchKernelGGL(time_reversals_kernel, dim3((unsigned)grid), dim3(epa::kBlock), 0, st, t, N, facts, list);
  return epa::check_launch("time_reversals_kernel");
}

extern "C" int epa_reversal_medians(const int64_t* t, long long N, int win_len, const int64_t* facts,
                                    const long long* list, int64_t* sub, epa_stream_t stream) {
  EPA_CHECK_ARG(N >= 2, "epa_reversal_medians: N=%lld times, at least 2 are needed", N);
  EPA_CHECK_ARG(win_len >= 1 && win_len <= EPA_QC_MAX_WIN, "epa_reversal_medians: win_len=%d, 1 .. %d are served", win_len,
                EPA_QC_MAX_WIN);
  EPA_CHECK_ARG(t && facts && list && sub, "epa_reversal_medians: NULL array argument");
  hipLaunchKernelGGL(reversal_medians_kernel, dim3(kMedianGrid), dim3(epa::kBlock), 0, static_cast<hipStream_t>(stream), t,
                     win_len, facts, list, sub);
  return epa::check_launch("reversal_medians_kernel");
}

// one running sum per tile of kTile differences
size_t epa::scratch::time_rebuild_tile_workspace(long long N, long long, long long) {
  return sizeof(int64_t) * (size_t)((N - 1 + kTile - 1) / kTile);
}

extern "C" int epa_time_rebuild(const int64_t* t, long long N, const int64_t* facts, const int64_t* sub,
                                int64_t* tile_workspace, int64_t* out, epa_stream_t stream) {
  EPA_CHECK_ARG(N >= 2, "epa_time_rebuild: N=%lld times, at least 2 are needed", N);
  EPA_CHECK_ARG(t && facts && sub && tile_workspace && out, "epa_time_rebuild: NULL array argument");
  EPA_CHECK_ARG(out != t, "epa_time_rebuild: out must not be the input");
  const long long ntiles = (N - 1 + kTile - 1) / kTile;
  EPA_CHECK_ARG(ntiles <= 0x7fffffffLL, "epa_time_rebuild: N=%lld times are more than one launch takes", N);
  hipStream_t st = static_cast<hipStream_t>(stream);
  u64* tiles = reinterpret_cast<u64*>(tile_workspace);
  hipLaunchKernelGGL(time_tile_sums_kernel, dim3((unsigned)ntiles), dim3(epa::kBlock), 0, st, t, N, facts, sub, tiles);
  if (int rc = epa::check_launch("time_tile_sums_kernel")) return rc;
  hipLaunchKernelGGL(time_tile_carry_kernel, dim3(1), dim3(epa::kBlock), 0, st, tiles, ntiles);
  if (int rc = epa::check_launch("time_tile_carry_kernel")) return rc;
  hipLaunchKernelGGL(time_rebuild_kernel, dim3((unsigned)ntiles), dim3(epa::kBlock), 0, st, t, N, facts, sub, tiles, out);
  return epa::check_launch("time_rebuild_kernel");
}
