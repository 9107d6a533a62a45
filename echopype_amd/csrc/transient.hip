// Transient-noise detectors of clean.detect_transient (reference: echopype clean/transient_noise/
// transient_fielding.py, transient_matecho.py).  Masks are uint8 [C*P*S] (1 = True = VALID, 0 = transient noise) in
// the (channel, ping_time, range_sample) layout of Sv; every channel of a call in one launch sequence.
//
// Both are order statistics of windows of a deep layer, found exactly by the radix selection of select.h on the dB
// values; all arithmetic is float64 whatever the storage type.  The scalars that depend on the range row alone
// (layer limits, step, window rows) are derived on the host with the reference's own expressions and come in as
// small per-channel tables; everything per ping is decided here.
//
// fielding   1. tr_fielding_flag_kernel   one workgroup per (channel, ping): writes the ping's row of the mask all-True;
//                                         median and 75th percentile (linear domain) of the ping's layer [up, lw),
//                                         median of the 2n-ping block [j-n, j+n); a flagged ping is appended to a list
//            2. tr_fielding_walk_kernel   one workgroup per LISTED ping (quiet data: every workgroup reads a zero count
//                                         and leaves): the dependent walk up the water column, then the column fill
// matecho    1. tr_matecho_rows_kernel    one lane per (channel, ping): minimum of the bottom over [j0, j1), the end
//                                         s_hi(j) of the run of window samples above it by binary search (float64)
//            2. tr_matecho_flag_kernel    one workgroup per (channel, ping): linear mean of the ping's samples, then ONE
//                                         counting sweep of the ping x depth window settles mean_db > pctl + delta_db
//                                         unless the threshold falls between the two ranks the percentile
//                                         interpolates; only then the selection runs
//            3. tr_matecho_fill_kernel    dilation along pings and the column fill
#include "fast_math.h"
#include "select.h"

namespace {

using epa::kBlock;
using namespace epa::sel;

constexpr long long kMaxGrid = 262144;

inline unsigned grid_for(long long rows) { return (unsigned)(rows < kMaxGrid ? (rows > 0 ? rows : 1) : kMaxGrid); }

__device__ __forceinline__ double block_sum_f64(double v, double* sh4) {
  v = epa::wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return epa::slots_sum(sh4);
}

// m[from .. n) = v by the workgroup: 4-byte stores over the aligned middle, single bytes at the two ragged ends
__device__ __forceinline__ void fill_bytes(uint8_t* m, int from, int n, uint8_t v) {
  const int len = n - from;
  if (len <= 0) return;
  uint8_t* p = m + from;
  const int head = min((int)((4u - (unsigned)((size_t)p & 3u)) & 3u), len);
  const int words = (len - head) >> 2;
  if ((int)threadIdx.x < head) p[threadIdx.x] = v;
  uint32_t* pw = reinterpret_cast<uint32_t*>(p + head);
  const uint32_t w = 0x01010101u * v;
  for (int i = threadIdx.x; i < words; i += kBlock) pw[i] = w;
  for (int i = head + 4 * words + (int)threadIdx.x; i < len; i += kBlock) p[i] = v;
}

__device__ __forceinline__ double to_db(double lin, const double2* log_tab) {
  return 10.0 * epa::fast_log10(lin, log_tab);
}

// ---- fielding --------------------------------------------------------------------------------------------------------
// chan: [C][4] = up, lw, rmin, sf of the channel (up >= lw: empty layer, nothing is ever flagged)
template <typename T>
__global__ __launch_bounds__(kBlock) void tr_fielding_flag_kernel(const T* __restrict__ sv, int P, int S, long long rows,
                                                                  const int* __restrict__ chan, int n, double thr0,
                                                                  double maxts, uint8_t* __restrict__ mask,
                                                                  long long* __restrict__ list,
                                                                  unsigned* __restrict__ count) {
  __shared__ __attribute__((aligned(16))) unsigned char tabs[epa::kMathTabBytes];
  __shared__ SelectScratch sc;
  const epa::MathTabs mt = epa::build_math_tabs(tabs);
  __syncthreads();
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int p = (int)(row % P);
    const long long c = row / P;
    const int up = chan[4 * c], lw = chan[4 * c + 1];
    fill_bytes(mask + (size_t)row * S, 0, S, 1);
    bool flag = false;
    if (p - n >= 0 && (long long)p + n <= (long long)P - 1 && lw > up) {
      const T* cb = sv + (size_t)c * P * S;
      const Window<T> own{cb, S, p, 1, up, lw - up, P, 0, false};
      unsigned nv;
      const double med = window_median_lin(own, &sc, mt.exp2_tab, nv, lw - up);
      if (nv) {  // (an all-NaN layer: uncomputable, nothing masked)
        const PercentileRank r75{75.0};
        unsigned long long k1, k2;
        window_select(own, &sc, r75, nv, k1, k2, lw - up);
        const double p75 = r75.lerp(epa::lin_from_db(key_value(k1), mt.exp2_tab),
                                    epa::lin_from_db(key_value(k2), mt.exp2_tab), nv);
        const Window<T> block{cb, S, p - n, 2 * n, up, lw - up, P, 0, false};
        unsigned nb;
        const double bmed = window_median_lin(block, &sc, mt.exp2_tab, nb, 2 * n * (lw - up));
        const double block_db = nb ? to_db(bmed, mt.log_tab) : __builtin_nan("");
        flag = (to_db(p75, mt.log_tab) < maxts) && ((to_db(med, mt.log_tab) - block_db) > thr0);
      }
    }
    if (flag && threadIdx.x == 0) list[atomicAdd(count, 1u)] = row;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void tr_fielding_walk_kernel(const T* __restrict__ sv, int P, int S,
                                                                  const int* __restrict__ chan, int n, double thr1,
                                                                  const long long* __restrict__ list,
                                                                  const unsigned* __restrict__ count,
                                                                  uint8_t* __restrict__ mask) {
  const unsigned nflag = *count;
  if (blockIdx.x >= nflag) return;  // quiet data: nothing but this read
  __shared__ __attribute__((aligned(16))) unsigned char tabs[epa::kMathTabBytes];
  __shared__ SelectScratch sc;
  const epa::MathTabs mt = epa::build_math_tabs(tabs);
  __syncthreads();
  for (unsigned i = blockIdx.x; i < nflag; i += gridDim.x) {
    const long long row = list[i];
    const int p = (int)(row % P);
    const long long c = row / P;
    const int up = chan[4 * c], rmin = chan[4 * c + 2], sf = chan[4 * c + 3];
    const T* cb = sv + (size_t)c * P * S;
    // r0_ > rmin >= 0 and r0_ + sf <= up < S inside the loop: every window lies inside the row
    int r0 = up - sf;
    while (r0 > rmin) {
      const Window<T> own{cb, S, p, 1, r0, sf, P, 0, false};
      const Window<T> block{cb, S, p - n, 2 * n, r0, sf, P, 0, false};
      unsigned na, nb;
      const double a = window_median_lin(own, &sc, mt.exp2_tab, na, sf);
      const double b = window_median_lin(block, &sc, mt.exp2_tab, nb, 2 * n * sf);
      const double diff = (na ? to_db(a, mt.log_tab) : __builtin_nan("")) - (nb ? to_db(b, mt.log_tab) : __builtin_nan(""));
      r0 -= sf;               // the window moves up BEFORE the test, as in the reference:
      if (diff < thr1) break;  // the mask starts one step above the last window compared; a NaN does not stop the walk
    }
    // mask[r0_:, j] with Python's slice semantics: a negative start counts from the end
    const int start = r0 < 0 ? max(0, S + r0) : min(r0, S);
    fill_bytes(mask + (size_t)row * S, start, S, 0);
  }
}

// ---- matecho ---------------------------------------------------------------------------------------------------------
// chan_i: [C][2] = s_lo, s_top: the run of samples with start_depth <= r <= start_depth + window_meter
// chan_d: [C][2] = r[1] - r[0], r[-1]
__global__ __launch_bounds__(kBlock) void tr_matecho_rows_kernel(const double* __restrict__ bottom, int bottom_rows,
                                                                 const double* __restrict__ range, int P, int S,
                                                                 long long rows, const int* __restrict__ chan_i,
                                                                 const double* __restrict__ chan_d, int h,
                                                                 int* __restrict__ s_hi) {
  for (long long row = (long long)blockIdx.x * kBlock + threadIdx.x; row < rows; row += (long long)gridDim.x * kBlock) {
    const int j = (int)(row % P);
    const long long c = row / P;
    const int s_lo = chan_i[2 * c], s_top = chan_i[2 * c + 1];
    const double r_last = chan_d[2 * c + 1];
    const int j0 = max(0, j - h), j1 = (int)min((long long)P, (long long)j + h);
    const double* b = bottom ? bottom + (bottom_rows > 1 ? (size_t)c * P : 0) : nullptr;
    double lb = __builtin_inf();
    bool nan = j0 >= j1;
    for (int q = j0; q < j1; ++q) {  // np.min: a NaN (here only r[-1] itself) wins
      double v = b ? b[q] : r_last;
      if (!(v == v)) v = r_last;
      nan |= !(v == v);
      lb = fmin(lb, v);
    }
    int hi = s_lo;
    if (!nan) {  // first sample of the run that is not above the bottom: r < local_bottom compared in float64
      const double* r = range + (size_t)c * S;
      int a = s_lo, e = s_top;
      while (a < e) {
        const int mid = a + (e - a) / 2;
        if (r[mid] < lb) a = mid + 1;
        else e = mid;
      }
      hi = a;
    }
    s_hi[row] = hi;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void tr_matecho_flag_kernel(const T* __restrict__ sv, int P, int S, long long rows,
                                                                 const int* __restrict__ chan_i,
                                                                 const double* __restrict__ chan_d,
                                                                 const int* __restrict__ s_hi, int h, double percentile,
                                                                 double delta_db, double min_window,
                                                                 uint8_t* __restrict__ flag) {
  __shared__ __attribute__((aligned(16))) unsigned char tabs[epa::kMathTabBytes];
  __shared__ SelectScratch sc;
  __shared__ double d4[4];
  const epa::MathTabs mt = epa::build_math_tabs(tabs);
  __syncthreads();
  const PercentileRank rank{percentile};
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int j = (int)(row % P);
    const long long c = row / P;
    const int s_lo = chan_i[2 * c], cnt = s_hi[row] - s_lo;
    bool bad = false;
    if (cnt > 0 && !(chan_d[2 * c] * (double)cnt < min_window)) {
      const T* cb = sv + (size_t)c * P * S;
      const T* own = cb + (size_t)j * S + s_lo;
      double sum = 0.0;
      unsigned nn = 0u;
      for (int s = threadIdx.x; s < cnt; s += kBlock) {
        const double v = (double)own[s];
        if (v == v) {
          sum += epa::lin_from_db(v, mt.exp2_tab);
          ++nn;
        }
      }
      sum = block_sum_f64(sum, d4);
      nn = block_sum(nn, sc.u4);
      if (nn) {  // (an all-NaN ping: NaN mean, never above anything)
        const double mean_db = to_db(sum / (double)nn, mt.log_tab);
        const int j0 = max(0, j - h), j1 = (int)min((long long)P, (long long)j + h);
        const Window<T> w{cb, S, j0, j1 - j0, s_lo, cnt, P, 0, false};
        // values whose  v + delta_db < mean_db  (monotone in v): with k, k + 1 the ranks the percentile interpolates,
        // at most k of them -> a[k] + delta >= mean, and pctl >= a[k]: not flagged; at least k + 2 (k + 1 without
        // interpolation) -> a[k+1] + delta < mean, and pctl <= a[k+1]: flagged -- the same outcome as the reference's
        // comparison of the rounded sum, since rounding is monotone.  Only in between does the percentile matter.
        unsigned nv = 0u, lt = 0u;
        w.for_each([&](double v) {
          if (v == v) {
            ++nv;
            if (v + delta_db < mean_db) ++lt;
          }
        });
        nv = block_sum(nv, sc.u4);
        lt = block_sum(lt, sc.u4);
        if (nv) {
          bool next;
          const unsigned k = rank(nv, next);
          if (lt <= k) bad = false;
          else if (lt >= k + (next ? 2u : 1u)) bad = true;
          else {
            unsigned long long k1, k2;
            unsigned n2;
            window_select(w, &sc, rank, n2, k1, k2, (j1 - j0) * cnt);
            bad = mean_db > rank.lerp(key_value(k1), key_value(k2), n2) + delta_db;
          }
        }
      }
    }
    if (threadIdx.x == 0) flag[row] = bad ? 1 : 0;
  }
}

// scipy.ndimage.binary_dilation of the per-ping flags with ones(2e + 1) (outside the axis: False), whole columns
__global__ __launch_bounds__(kBlock) void tr_matecho_fill_kernel(const uint8_t* __restrict__ flag, int P, int S,
                                                                 long long rows, int e, uint8_t* __restrict__ mask) {
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int j = (int)(row % P);
    const uint8_t* f = flag + (size_t)(row - j);
    const int lo = max(0, j - e), hi = (int)min((long long)P - 1, (long long)j + e);
    int any = 0;
    for (int q = lo + (int)threadIdx.x; q <= hi; q += kBlock) any |= f[q];
    const uint8_t keep = __syncthreads_or(any) ? 0 : 1;
    fill_bytes(mask + (size_t)row * S, 0, S, keep);
  }
}

int check_cube(const char* who, const void* sv, const void* mask, int dtype, int C, int P, int S) {
  EPA_CHECK_ARG(sv && mask, "%s: NULL array argument", who);
  EPA_CHECK_ARG(C > 0 && P > 0 && S > 0, "%s: C=%d P=%d S=%d", who, C, P, S);
  EPA_CHECK_REAL(who, dtype);
  return EPA_OK;
}

}  // namespace

// Fielding: the list of (channel, ping) rows left to the walk and its length; Matecho: s_hi and the flag of every row
size_t epa::scratch::transient_fielding_todo(long long C, long long P, long long) { return sizeof(long long) * (size_t)C * P; }
size_t epa::scratch::transient_fielding_count(long long, long long, long long) { return sizeof(unsigned); }
size_t epa::scratch::transient_matecho_s_hi(long long C, long long P, long long) { return sizeof(int) * (size_t)C * P; }
size_t epa::scratch::transient_matecho_flag(long long C, long long P, long long) { return sizeof(uint8_t) * (size_t)C * P; }

extern "C" int epa_transient_fielding(const void* sv, int dtype, int C, int P, int S, const int* chan, int max_rows,
                                      int n, double thr0, double thr1, double maxts, long long* list,
                                      unsigned* count, uint8_t* mask, epa_stream_t stream) {
  const char* who = "epa_transient_fielding";
  if (int rc = check_cube(who, sv, mask, dtype, C, P, S)) return rc;
  EPA_CHECK_ARG(chan && list && count, "%s: NULL array argument", who);
  EPA_CHECK_ARG(n >= 0 && max_rows >= 0 && 2LL * n * max_rows < 0x7fffffffLL,
                "%s: a block of 2 * n = %lld pings x %d samples does not fit 31 bits", who, 2LL * n, max_rows);
  hipStream_t st = (hipStream_t)stream;
  const long long rows = (long long)C * P;
  EPA_CHECK_HIP(hipMemsetAsync(count, 0, epa::scratch::transient_fielding_count(0, 0, 0), st));
  return epa::dispatch_real(who, dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    tr_fielding_flag_kernel<T><<<grid_for(rows), kBlock, 0, st>>>((const T*)sv, P, S, rows, chan, n, thr0, maxts, mask,
                                                                  list, count);
    if (int rc = epa::check_launch("tr_fielding_flag_kernel")) return rc;
    const unsigned walkers = grid_for(rows < 16384 ? rows : 16384);
    tr_fielding_walk_kernel<T><<<walkers, kBlock, 0, st>>>((const T*)sv, P, S, chan, n, thr1, list, count, mask);
    return epa::check_launch("tr_fielding_walk_kernel");
  });
}

extern "C" int epa_transient_matecho(const void* sv, int dtype, int C, int P, int S, const double* range,
                                     const int* chan_i, const double* chan_d, const double* bottom, int bottom_rows,
                                     int half_window, double percentile, double delta_db, int extend_ping,
                                     double min_window, int* s_hi, uint8_t* flag, uint8_t* mask, epa_stream_t stream) {
  const char* who = "epa_transient_matecho";
  if (int rc = check_cube(who, sv, mask, dtype, C, P, S)) return rc;
  EPA_CHECK_ARG(range && chan_i && chan_d && s_hi && flag, "%s: NULL array argument", who);
  EPA_CHECK_ARG(bottom_rows == 0 ? bottom == nullptr : (bottom != nullptr && (bottom_rows == 1 || bottom_rows == C)),
                "%s: bottom_rows=%d (0 without a bottom, 1 or C=%d with one)", who, bottom_rows, C);
  EPA_CHECK_ARG(half_window >= 0 && 2LL * (half_window < P ? half_window : P) * S < 0x7fffffffLL,
                "%s: a window of 2 * %d pings x %d samples does not fit 31 bits", who, half_window, S);
  EPA_CHECK_ARG(percentile >= 0.0 && percentile <= 100.0, "%s: percentile %g outside [0, 100]", who, percentile);
  hipStream_t st = (hipStream_t)stream;
  const long long rows = (long long)C * P;
  if (half_window > P) half_window = P;
  if (extend_ping < 0) extend_ping = 0;
  if (extend_ping > P) extend_ping = P;
  tr_matecho_rows_kernel<<<grid_for((rows + kBlock - 1) / kBlock), kBlock, 0, st>>>(bottom, bottom_rows, range, P, S, rows,
                                                                                    chan_i, chan_d, half_window, s_hi);
  if (int rc = epa::check_launch("tr_matecho_rows_kernel")) return rc;
  const int rc = epa::dispatch_real(who, dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    tr_matecho_flag_kernel<T><<<grid_for(rows), kBlock, 0, st>>>((const T*)sv, P, S, rows, chan_i, chan_d, s_hi,
                                                                 half_window, percentile, delta_db, min_window, flag);
    return epa::check_launch("tr_matecho_flag_kernel");
  });
  if (rc) return rc;
  tr_matecho_fill_kernel<<<grid_for(rows), kBlock, 0, st>>>(flag, P, S, rows, extend_ping, mask);
  return epa::check_launch("tr_matecho_fill_kernel");
}
