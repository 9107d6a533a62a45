// utils.align.align_to_ping_time / consolidate.add_location: values recorded on an external clock (a navigation track)
// brought onto ping_time.  One thread takes one ping: a binary search over the external times (800 KB for a track of
// 100 000 fixes: they stay in L2), then every row of values from that one position -- latitude and longitude are one launch.
//
// Linear mode is scipy.interpolate.interp1d(kind="linear", fill_value="extrapolate") operation for operation (what
// xarray's interp runs): times as float64 nanoseconds from the first external time, np.searchsorted(side="left") on
// those floats, the index clipped to 1 .. N-1, slope = (y_hi - y_lo) / (x_hi - x_lo), out = slope * (q - x_lo) + y_lo
// with the product rounded before the sum.  Nearest mode takes the same position and decides between its two
// neighbours in int64 nanoseconds, ties to the earlier sample.
#include "epa_internal.h"

namespace {

constexpr int kLinear = 0, kNearest = 1;

// (double)(t - t0): the integer difference first (wrapping like NumPy's), then one conversion, round to nearest even
__device__ __forceinline__ double ns_from(int64_t t, int64_t t0) {
  return (double)(int64_t)((uint64_t)t - (uint64_t)t0);
}

__global__ void __launch_bounds__(epa::kBlock)
align_to_ping_time_kernel(const int64_t* __restrict__ t_ext, int N, const double* __restrict__ y, int V,
                          const int64_t* __restrict__ ping_time, int P, int mode, double* __restrict__ out) {
  const long long p = (long long)blockIdx.x * epa::kBlock + threadIdx.x;
  if (p >= P) return;
  const int64_t tp = ping_time[p];
  if (tp == INT64_MIN) {  // NaT
    for (int v = 0; v < V; ++v) out[(long long)v * P + p] = epa::M<double>::nan();
    return;
  }
  const int64_t t0 = t_ext[0];
  const double q = ns_from(tp, t0);
  // first i in 0 .. N with x_i >= q, compared as the converted doubles
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (ns_from(t_ext[mid], t0) < q) lo = mid + 1;
    else hi = mid;
  }
  const int k = lo < 1 ? 1 : (lo > N - 1 ? N - 1 : lo);  // 1 <= k <= N-1 since N >= 2: k-1 and k are both inside
  const int64_t ta = t_ext[k - 1], tb = t_ext[k];
  if (mode == kNearest) {
    const int64_t before = (int64_t)((uint64_t)tp - (uint64_t)ta), after = (int64_t)((uint64_t)tb - (uint64_t)tp);
    const int pick = before <= after ? k - 1 : k;
    for (int v = 0; v < V; ++v) out[(long long)v * P + p] = y[(long long)v * N + pick];
    return;
  }
  const double xa = ns_from(ta, t0), xb = ns_from(tb, t0);
  const double dx = xb - xa, dq = q - xa;
  for (int v = 0; v < V; ++v) {
#pragma clang fp contract(off)
    const double ya = y[(long long)v * N + k - 1], yb = y[(long long)v * N + k];
    const double slope = (yb - ya) / dx;
    const double prod = slope * dq;
    out[(long long)v * P + p] = prod + ya;
  }
}

}  // namespace

extern "C" int epa_align_to_ping_time(const int64_t* t_ext, int N, const double* y, int V, const int64_t* ping_time,
                                      int P, int mode, double* out, epa_stream_t stream) {
  EPA_CHECK_ARG(N >= 2, "epa_align_to_ping_time: N=%d external times, at least 2 are needed", N);
  EPA_CHECK_ARG(V >= 1, "epa_align_to_ping_time: V=%d rows of values, at least 1 is needed", V);
  EPA_CHECK_ARG(P >= 1, "epa_align_to_ping_time: P=%d pings, at least 1 is needed", P);
  EPA_CHECK_ARG(t_ext && y && ping_time && out, "epa_align_to_ping_time: NULL array argument");
  EPA_CHECK_ARG(mode == kLinear || mode == kNearest, "epa_align_to_ping_time: bad mode %d (0 linear, 1 nearest)", mode);
  const int grid = (int)(((long long)P + epa::kBlock - 1) / epa::kBlock);
  hipLaunchKernelGGL(align_to_ping_time_kernel, dim3(grid), dim3(epa::kBlock), 0, static_cast<hipStream_t>(stream),
                     t_ext, N, y, V, ping_time, P, mode, out);
  return epa::check_launch("align_to_ping_time_kernel");
}
