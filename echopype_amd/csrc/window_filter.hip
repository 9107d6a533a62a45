// clean.window_filter: the per-sample 2-D window operators on Sv -- NaN-aware median, linear-domain mean, min and max
// (erosion / dilation) over ping_num x range_sample_num samples, both odd and at most EPA_WINDOW_FILTER_MAX.  THE RULE is
// in echopype_amd.h (epa_window_filter) and restated in NumPy in tests/window_filter_ref.py: the window is clipped to the
// array (it shrinks at the edges), never crosses channels, its valid values are the non-NaN ones (+-inf are values), a
// window with fewer than min_valid of them gives NaN, and with keep_nan a NaN sample stays NaN.
//
// One launch.  A workgroup of 256 lanes owns a tile of TP x TS = 16 pings x 64 samples and loads it with its halo of
// hp / hs on every side into LDS once: (TP + 2 hp) rows of (TS + 2 hs) elements, a wave per row, lanes along range_sample
// (consecutive addresses).  Positions outside the array are loaded as "NaN", so the clipping costs no branch in the inner
// loops.  What lies in LDS depends on the method:
//   mean            : 10^(v / 10) as a double, converted ONCE per loaded element (lin_from_db), NaN where v is;
//   median, min, max: the order-preserving key of v (ordered_key.h; 32 bits for float32, 64 for float64), NaN as the
//                     all-ones word no number maps to -- it is above every candidate of the selection, so it is never
//                     counted, and above every key, so a minimum skips it.
// The largest tile, 30 x 78 doubles, is 18.3 KiB (22.3 with the tables of the mean): seven workgroups fit the 160 KiB of
// a CU.  A lane computes the outputs of ONE column in FOUR consecutive rows: lanes read consecutive LDS words.
//   mean, min, max are separable: a lane reduces each of the 4 + 2 hp rows of its column strip once along range_sample
//     (sum and count, or extremum and count) and folds the row's result into those of its four outputs whose window holds
//     the row: (4 + 2 hp)(2 hs + 1) LDS reads for four outputs instead of 4 (2 hp + 1)(2 hs + 1).
//   median is ONE selection for every window size and every count of valid values: a first sweep of the window gives
//     the count n, the smallest and the largest key; the keys agree in every bit above the highest bit in which those
//     two differ, and each lower bit is decided, from the top, by counting the keys below prefix | bit (at most the
//     rank: the bit is set).  That is the key of rank (n - 1) / 2, exactly.  For an even n one more sweep counts the
//     keys <= it and finds the smallest key above it: the next rank.
// Every output element is stored exactly once (non-temporal: it is not read again here); nothing is pre-filled.
#include "epa_internal.h"
#include "fast_math.h"
#include "ordered_key.h"

#include <climits>
#include <type_traits>

namespace {

using epa::kBlock;

constexpr int TP = EPA_WINDOW_FILTER_TP, TS = EPA_WINDOW_FILTER_TS;
constexpr int kHaloMax = EPA_WINDOW_FILTER_MAX / 2;
constexpr int kTileElems = (TP + 2 * kHaloMax) * (TS + 2 * kHaloMax);
using epa::kWaves;
constexpr int kRows = TP / kWaves;        // consecutive rows of one column that a lane computes
constexpr int kWindowMaxGrid = 1 << 20;  // workgroups of a launch: further tiles are taken in a loop
static_assert(TS == 64 && kRows * kWaves == TP, "a wave spans a tile row, the waves share its rows evenly");
static_assert(kTileElems * sizeof(double) + epa::kMathTabBytes <= 32 * 1024, "several workgroups per CU");

struct WindowArgs {
  const void* in;
  void* out;
  int P, S, hp, hs, min_valid, keep_nan;
  int tiles_p, tiles_s, ntiles, xcd_map;
};

template <typename T>
struct KeyOf {
  using type = unsigned;
};
template <>
struct KeyOf<double> {
  using type = unsigned long long;
};

__device__ __forceinline__ int high_bit(unsigned x) { return 31 - __builtin_clz(x); }
__device__ __forceinline__ int high_bit(unsigned long long x) { return 63 - __builtin_clzll(x); }

// the even median of two different middle values, in the linear domain (rare: only windows that the array's edge or a
// NaN leaves with an even count come here, so the full-precision routines are called out of line)
__device__ __noinline__ double median_pair_db(double a, double b) {
  return 10.0 * epa::M<double>::log10((epa::M<double>::exp10(a / 10.0) + epa::M<double>::exp10(b / 10.0)) * 0.5);
}

// The keys of rank (n - 1) / 2 and n / 2 among the n valid keys of the np x ns window at w (row pitch W); false if
// n < min_valid.  kNone (all ones) marks NaN.
template <typename K>
__device__ __forceinline__ bool window_median_keys(const K* w, int W, int np, int ns, int min_valid, K& lo, K& hi) {
  constexpr K kNone = ~K(0);
  int n = 0;
  K kmin = kNone, kmax = 0;
  for (int dp = 0; dp < np; ++dp) {
    for (int ds = 0; ds < ns; ++ds) {
      const K k = w[dp * W + ds];
      const bool ok = k != kNone;
      n += ok;
      kmin = k < kmin ? k : kmin;
      kmax = (ok && k > kmax) ? k : kmax;
    }
  }
  if (n < min_valid) return false;
  const int rank = (n - 1) >> 1;
  K a = kmin;
  if (kmin != kmax) {
    const int top = high_bit((K)(kmin ^ kmax));
    a = kmin & ~((K(2) << top) - K(1));  // the bits every key shares (K(2) << top is 0 for the top bit: nothing shared)
    for (int bit = top; bit >= 0; --bit) {
      const K cand = a | (K(1) << bit);
      int below = 0;
      for (int dp = 0; dp < np; ++dp)
        for (int ds = 0; ds < ns; ++ds) below += w[dp * W + ds] < cand;
      if (below <= rank) a = cand;
    }
  }
  lo = hi = a;
  if (!(n & 1)) {
    int le = 0;
    K next = kNone;
    for (int dp = 0; dp < np; ++dp) {
      for (int ds = 0; ds < ns; ++ds) {
        const K k = w[dp * W + ds];
        le += k <= a;
        next = (k > a && k < next) ? k : next;
      }
    }
    if (le <= rank + 1) hi = next;  // (a valid key: le < n here)
  }
  return true;
}

template <typename T, int METHOD>
__global__ __launch_bounds__(kBlock) void window_filter_kernel(WindowArgs a) {
  using K = typename KeyOf<T>::type;
  constexpr bool kMean = METHOD == EPA_WINDOW_MEAN;
  using E = std::conditional_t<kMean, double, K>;
  constexpr K kNone = ~K(0);
  __shared__ E s_tile[kTileElems];
  __shared__ __align__(16) unsigned char s_tabs[kMean ? epa::kMathTabBytes : 16];

  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int P = a.P, S = a.S, hp = a.hp, hs = a.hs;
  const int np = 2 * hp + 1, ns = 2 * hs + 1;
  const int W = TS + 2 * hs, H = TP + 2 * hp;
  const T nan = epa::M<T>::nan();
  const T* __restrict__ in = static_cast<const T*>(a.in);
  T* __restrict__ out = static_cast<T*>(a.out);

  epa::MathTabs tabs{nullptr, nullptr};
  if (kMean) {
    tabs = epa::build_math_tabs(s_tabs);
    __syncthreads();
  }

  const int g = a.xcd_map ? epa::xcd_contiguous((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  for (long long t = g; t < a.ntiles; t += gridDim.x) {
    const int ts = (int)(t % a.tiles_s);
    const long long tq = t / a.tiles_s;
    const int tp = (int)(tq % a.tiles_p);
    const long long c = tq / a.tiles_p;
    const int p0 = tp * TP, s0 = ts * TS;
    const size_t plane = (size_t)c * P;

    // ---- the tile and its halo: a wave per row, lanes along range_sample ---------------------------------------------
#pragma unroll 2
    for (int i = wave; i < H; i += kWaves) {
      const int p = p0 - hp + i;
      const bool row_in = p >= 0 && p < P;
      const T* __restrict__ src = in + (plane + (size_t)(row_in ? p : 0)) * S;
      for (int j = lane; j < W; j += 64) {
        const int s = s0 - hs + j;
        T v = nan;
        if (row_in && s >= 0 && s < S) v = src[s];
        if constexpr (kMean) s_tile[i * W + j] = epa::lin_from_db((double)v, tabs.exp2_tab);
        else s_tile[i * W + j] = v == v ? epa::ordered_key(v) : kNone;
      }
    }
    __syncthreads();

    // ---- four consecutive rows of one column per lane -----------------------------------------------------------------
    const int r0 = wave * kRows;
    const int s = s0 + lane;
    if (p0 + r0 < P && s < S) {
      T res[kRows];
      if constexpr (METHOD == EPA_WINDOW_MEDIAN) {
        for (int k = 0; k < kRows; ++k) {
          const E* w = s_tile + (r0 + k) * W + lane;
          K lo, hi;
          T r = nan;
          if (window_median_keys<K>(w, W, np, ns, a.min_valid, lo, hi)) {
            const T va = epa::key_value(lo), vb = epa::key_value(hi);
            r = va == vb ? va : (T)median_pair_db((double)va, (double)vb);
          }
          if (a.keep_nan && w[hp * W + hs] == kNone) r = nan;
          res[k] = r;
        }
      } else {
        E acc[kRows];
        int cnt[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
          acc[k] = kMean ? E(0) : (METHOD == EPA_WINDOW_MIN ? (E)kNone : E(0));
          cnt[k] = 0;
        }
        for (int rr = 0; rr < kRows + 2 * hp; ++rr) {
          const E* row = s_tile + (r0 + rr) * W + lane;
          E racc = kMean ? E(0) : (METHOD == EPA_WINDOW_MIN ? (E)kNone : E(0));
          int rcnt = 0;
          for (int ds = 0; ds < ns; ++ds) {
            const E v = row[ds];
            if constexpr (kMean) {
              const bool ok = v == v;
              racc += ok ? v : 0.0;
              rcnt += ok;
            } else {
              const bool ok = v != kNone;
              rcnt += ok;
              if (METHOD == EPA_WINDOW_MIN) racc = v < racc ? v : racc;
              else racc = (ok && v > racc) ? v : racc;
            }
          }
#pragma unroll
          for (int k = 0; k < kRows; ++k) {
            const bool inside = rr >= k && rr <= k + 2 * hp;
            if constexpr (kMean) acc[k] += inside ? racc : 0.0;
            else if (METHOD == EPA_WINDOW_MIN) acc[k] = (inside && racc < acc[k]) ? racc : acc[k];
            else acc[k] = (inside && racc > acc[k]) ? racc : acc[k];
            cnt[k] += inside ? rcnt : 0;
          }
        }
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
          const E centre = s_tile[(r0 + k + hp) * W + lane + hs];
          T r = nan;
          if (cnt[k] >= a.min_valid) {
            if constexpr (kMean) r = (T)(10.0 * epa::fast_log10(acc[k] / (double)cnt[k], tabs.log_tab));
            else r = epa::key_value((K)acc[k]);
          }
          bool centre_nan;
          if constexpr (kMean) centre_nan = !(centre == centre);
          else centre_nan = centre == kNone;
          if (a.keep_nan && centre_nan) r = nan;
          res[k] = r;
        }
      }
#pragma unroll
      for (int k = 0; k < kRows; ++k) {
        const int p = p0 + r0 + k;
        if (p < P) __builtin_nontemporal_store(res[k], out + (plane + (size_t)p) * S + s);
      }
    }
    __syncthreads();  // (the next tile overwrites s_tile)
  }
}

}  // namespace

extern "C" int epa_window_filter(const void* x, int dtype, int C, int P, int S, int method, int ping_num,
                                 int range_sample_num, int min_valid, int keep_nan, void* out, int max_grid,
                                 epa_stream_t stream) {
  EPA_CHECK_REAL("epa_window_filter", dtype);
  EPA_CHECK_ARG(method >= EPA_WINDOW_MEDIAN && method <= EPA_WINDOW_MAX, "epa_window_filter: bad method %d", method);
  EPA_CHECK_ARG(C >= 0 && P >= 0 && S >= 0, "epa_window_filter: bad shape C=%d P=%d S=%d", C, P, S);
  EPA_CHECK_ARG((ping_num & 1) && ping_num >= 1 && ping_num <= EPA_WINDOW_FILTER_MAX && (range_sample_num & 1) &&
                    range_sample_num >= 1 && range_sample_num <= EPA_WINDOW_FILTER_MAX,
                "epa_window_filter: the window sizes must be odd and within 1 .. %d, got %d x %d", EPA_WINDOW_FILTER_MAX,
                ping_num, range_sample_num);
  EPA_CHECK_ARG(min_valid >= 1 && min_valid <= ping_num * range_sample_num,
                "epa_window_filter: min_valid must be within 1 .. %d, got %d", ping_num * range_sample_num, min_valid);
  EPA_CHECK_ARG(max_grid >= 0, "epa_window_filter: max_grid must not be negative");
  if (C == 0 || P == 0 || S == 0) return EPA_OK;
  EPA_CHECK_ARG(x && out, "epa_window_filter: NULL array argument");
  const long long tiles_p = ((long long)P + TP - 1) / TP, tiles_s = ((long long)S + TS - 1) / TS;
  EPA_CHECK_ARG((long long)C * tiles_p <= INT_MAX / tiles_s,  // (C * tiles_p < 2^58)
                "epa_window_filter: %d x %lld x %lld tiles do not fit one launch", C, tiles_p, tiles_s);
  const long long ntiles = (long long)C * tiles_p * tiles_s;
  // (at most 2^31 tiles of TP * TS samples: the byte count fits 64 bits)
  const unsigned long long bytes = (unsigned long long)C * (unsigned long long)P * (unsigned long long)S * (dtype == EPA_F64 ? 8u : 4u);
  const uintptr_t xb = reinterpret_cast<uintptr_t>(x), ob = reinterpret_cast<uintptr_t>(out);
  EPA_CHECK_ARG(xb + bytes <= ob || ob + bytes <= xb,
                "epa_window_filter: out overlaps x (a neighbour's halo would read results)");

  WindowArgs a;
  a.in = x, a.out = out, a.P = P, a.S = S, a.hp = ping_num / 2, a.hs = range_sample_num / 2;
  a.min_valid = min_valid, a.keep_nan = keep_nan != 0;
  a.tiles_p = (int)tiles_p, a.tiles_s = (int)tiles_s, a.ntiles = (int)ntiles, a.xcd_map = epa::xcd_map_enabled();
  const long long cap = max_grid > 0 ? max_grid : kWindowMaxGrid;
  const unsigned grid = (unsigned)(ntiles < cap ? ntiles : cap);
  hipStream_t st = (hipStream_t)stream;
  return epa::dispatch_real("epa_window_filter", dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    switch (method) {
      case EPA_WINDOW_MEDIAN:
        hipLaunchKernelGGL((window_filter_kernel<T, EPA_WINDOW_MEDIAN>), dim3(grid), dim3(kBlock), 0, st, a);
        return epa::check_launch("window_filter_kernel<median>");
      case EPA_WINDOW_MEAN:
        hipLaunchKernelGGL((window_filter_kernel<T, EPA_WINDOW_MEAN>), dim3(grid), dim3(kBlock), 0, st, a);
        return epa::check_launch("window_filter_kernel<mean>");
      case EPA_WINDOW_MIN:
        hipLaunchKernelGGL((window_filter_kernel<T, EPA_WINDOW_MIN>), dim3(grid), dim3(kBlock), 0, st, a);
        return epa::check_launch("window_filter_kernel<min>");
      default:
        hipLaunchKernelGGL((window_filter_kernel<T, EPA_WINDOW_MAX>), dim3(grid), dim3(kBlock), 0, st, a);
        return epa::check_launch("window_filter_kernel<max>");
    }
  });
}
