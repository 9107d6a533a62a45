// Seafloor detection (mask.detect_seafloor): the "basic" and "blackwell" bottom lines of one channel.
//
// Reference arithmetic replaced (echopype, mask/seafloor_detection/):
//   utils.py:_check_inputs            max over range of |depth - depth[ping 0]| < 1e-16 for every ping (NaN skipped; a
//                                      ping with no finite difference fails)      -> sf_depth_uniform_kernel
//   bottom_basic.py                    first sample s >= bin_skip with tmin < Sv < tmax per ping, else bin_skip
//                                                                                  -> sf_basic_kernel
//   bottom_blackwell.py                convolve2d(angle, ones(w, w) / w^2, "same", boundary="symm") ** 2 > t for both
//                                      angles, OR-ed                               -> sf_box_rows_kernel, sf_box_cols_kernel
//                                      nanmedian of Sv under that mask (selected in dB: 10^(x/10) is monotone; the
//                                      host finishes the one or two middle values with NumPy's own expression)
//                                                                                  -> sf_median_hist_kernel, sf_median_pick_kernel
//                                      scipy.ndimage.label (8-connectivity) of Sv > threshold, the components that
//                                      meet the angle mask kept, first kept sample per ping
//                                                                                  -> sf_cc_init/merge/compress/seed_kernel,
//                                                                                     sf_bottom_kernel
//
// The box filter is two direct passes (window sums along range, then along pings), summed in f64: NaN anywhere in the
// window propagates into the sum exactly as it does through convolve2d, with no NaN counts needed.  "same" centring:
// output i averages inputs i - w/2 .. i + w - 1 - w/2; "symm" reflects with the edge sample repeated, periodically
// (period 2N) when the window is longer than the crop.
//
// Connected components: union-find on the whole crop (a seabed component spans every ping, so label propagation
// would need as many sweeps as there are pings).  Every foreground pixel unions itself with its W, NW, N and NE
// neighbours; links always point to a smaller index (atomic min on the root), so the forest has no cycles and a
// find is bounded by the number of pixels; finds of the merge pass halve their paths with plain stores (a halving
// write only ever replaces a non-root's parent by one of its ancestors).  The compression pass that follows stores
// roots only (a halving store there could overwrite a root another thread has just stored).  No workgroup waits for
// another: nothing relies on all of them being resident.  Each retry loop has a bound (the pixel count: a correct run cannot reach it); a loop that
// reaches it counts into an error word the host turns into an exception.
#include "epa_internal.h"
#include "ordered_key.h"
#include "union_find.h"

namespace {

using epa::uf::ld;
using epa::uf::st;
using epa::uf::uf_root;
using epa::uf::uf_union;

using epa::kWaves;
constexpr int kMaxBlocks = 16384;

// state words (EPA_SEAFLOOR_STATE_WORDS u64, zeroed by the caller)
enum : int {
  kMasked = 0,  // pixels under the angle mask
  kCount = 1,   // non-NaN Sv values under it
  kPrefLo = 2,  // radix-select prefixes (then the full keys) of the lower / upper middle value
  kPrefHi = 3,
  kRankLo = 4,  // ranks still to skip inside the current prefix
  kRankHi = 5,
  kValLo = 6,   // the two middle values as f64 bits
  kValHi = 7,
  kError = 8,   // union-find loops that reached their bound
};

inline int blocks_for(long long n) {
  long long b = (n + epa::kBlock - 1) / epa::kBlock;
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}
inline int blocks_for_rows(long long rows) {
  long long b = (rows + kWaves - 1) / kWaves;
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// index of the "symm" extension of an axis of n samples (n >= 1): ... x1 x0 | x0 x1 ... x(n-1) | x(n-1) x(n-2) ...
__device__ __forceinline__ long long reflect(long long m, long long n) {
  if (m >= 0 && m < n) return m;
  const long long p = 2 * n;
  m %= p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// ---- depth grid uniformity (utils.py:_check_inputs) ------------------------------------------------------------------
template <typename D>
__global__ __launch_bounds__(epa::kBlock) void sf_depth_uniform_kernel(const D* __restrict__ depth, long long P,
                                                                       long long S, int* __restrict__ bad_pings) {
  const int lane = threadIdx.x & 63;
  for (long long p = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); p < P; p += (long long)gridDim.x * kWaves) {
    const D* row = depth + p * S;
    bool has = false, bad = false;
    for (long long s = lane; s < S; s += 64) {
      const D d = row[s] - depth[s];
      const D a = d < (D)0 ? -d : d;
      if (a == a) {
        has = true;
        if (!(a < (D)1e-16)) bad = true;
      }
    }
    const bool any_has = __ballot(has) != 0;
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0 && (!any_has || any_bad)) atomicAdd(bad_pings, 1);
  }
}

// ---- basic: first crossing per ping -------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(epa::kBlock) void sf_basic_kernel(const T* __restrict__ sv, long long P, long long S,
                                                               long long skip, T tmin, T tmax,
                                                               const double* __restrict__ depth0, double offset,
                                                               double* __restrict__ out) {
  constexpr int U = 8;  // 8 loads of 64 samples in flight per wave before the first ballot
  const int lane = threadIdx.x & 63;
  for (long long p = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); p < P; p += (long long)gridDim.x * kWaves) {
    const T* row = sv + p * S;
    long long idx = skip;
    for (long long base = skip; base < S; base += 64 * U) {
      T v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long s = base + u * 64 + lane;
        v[u] = s < S ? row[s] : (T)0;
      }
      long long hit = -1;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long s = base + u * 64 + lane;
        const unsigned long long b = __ballot(s < S && v[u] > tmin && v[u] < tmax);
        if (hit < 0 && b) hit = base + u * 64 + (__ffsll(b) - 1);
      }
      if (hit >= 0) {
        idx = hit;
        break;
      }
    }
    if (lane == 0) {
#pragma clang fp contract(off)
      out[p] = depth0[idx] - offset;
    }
  }
}

// ---- blackwell: box-filtered angle mask ---------------------------------------------------------------------------
// pass 1: window sums along range of both angles over the crop [r0, r0 + R) of every ping -> h (2 * P * R doubles)
template <typename A>
__global__ __launch_bounds__(epa::kBlock) void sf_box_rows_kernel(const A* __restrict__ theta,
                                                                  const A* __restrict__ phi, long long P, long long S,
                                                                  long long r0, long long R, int wt, int wp,
                                                                  double* __restrict__ h) {
  const long long n = P * R;
  const int ht = wt / 2, hp = wp / 2;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    const long long p = q / R, i = q - p * R;
    const A* tr = theta + p * S + r0;
    const A* pr = phi + p * S + r0;
    double st = 0.0, sp = 0.0;
    if (i - ht >= 0 && i - ht + wt <= R) {
      for (int k = 0; k < wt; ++k) st += (double)tr[i - ht + k];
    } else {
      for (int k = 0; k < wt; ++k) st += (double)tr[reflect(i - ht + k, R)];
    }
    if (i - hp >= 0 && i - hp + wp <= R) {
      for (int k = 0; k < wp; ++k) sp += (double)pr[i - hp + k];
    } else {
      for (int k = 0; k < wp; ++k) sp += (double)pr[reflect(i - hp + k, R)];
    }
    h[q] = st;
    h[n + q] = sp;
  }
}

// pass 2: window sums along pings, the squared means against the thresholds -> mask bit 0; masked pixels counted
__global__ __launch_bounds__(epa::kBlock) void sf_box_cols_kernel(const double* __restrict__ h, long long P,
                                                                  long long R, int wt, int wp, double ttheta,
                                                                  double tphi, unsigned char* __restrict__ mask,
                                                                  unsigned long long* __restrict__ state) {
  const long long n = P * R;
  const int ht = wt / 2, hp = wp / 2;
  const double nt = (double)wt * (double)wt, np_ = (double)wp * (double)wp;
  unsigned long long cnt = 0;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    const long long p = q / R, i = q - p * R;
    double st = 0.0, sp = 0.0;
    if (p - ht >= 0 && p - ht + wt <= P) {
      for (int k = 0; k < wt; ++k) st += h[(p - ht + k) * R + i];
    } else {
      for (int k = 0; k < wt; ++k) st += h[reflect(p - ht + k, P) * R + i];
    }
    if (p - hp >= 0 && p - hp + wp <= P) {
      for (int k = 0; k < wp; ++k) sp += h[n + (p - hp + k) * R + i];
    } else {
      for (int k = 0; k < wp; ++k) sp += h[n + reflect(p - hp + k, P) * R + i];
    }
    const double mt = st / nt, mp = sp / np_;
    const bool m = (mt * mt > ttheta) || (mp * mp > tphi);  // NaN compares false
    mask[q] = m ? 1 : 0;
    cnt += m ? 1 : 0;
  }
  // one atomic per wave
  cnt = epa::wave_sum(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&state[kMasked], cnt);
}

// ---- blackwell: median of Sv under the angle mask (radix select on order-preserving keys, 8 bits per pass) -----------
template <typename T>
struct Key;
template <>
struct Key<float> {
  using U = unsigned int;
  static constexpr int kBits = 32;
  static __device__ __forceinline__ U of(float x) { return epa::ordered_key(x); }
  static __device__ __forceinline__ double value(unsigned long long k) { return (double)epa::key_value((U)k); }
};
template <>
struct Key<double> {
  using U = unsigned long long;
  static constexpr int kBits = 64;
  static __device__ __forceinline__ U of(double x) { return epa::ordered_key(x); }
  static __device__ __forceinline__ double value(unsigned long long key) { return epa::key_value(key); }
};

template <typename T>
__global__ __launch_bounds__(epa::kBlock) void sf_median_hist_kernel(const T* __restrict__ sv, long long P,
                                                                     long long S, long long r0, long long R,
                                                                     const unsigned char* __restrict__ mask, int shift,
                                                                     const unsigned long long* __restrict__ state,
                                                                     unsigned long long* __restrict__ hist) {
  using K = Key<T>;
  __shared__ unsigned int lh[2][256];
  for (int j = threadIdx.x; j < 512; j += blockDim.x) lh[j >> 8][j & 255] = 0;
  __syncthreads();
  const bool first = shift + 8 >= K::kBits;
  const int hs = first ? 0 : shift + 8;
  const typename K::U plo = first ? 0 : (typename K::U)(state[kPrefLo] >> hs);
  const typename K::U phi = first ? 0 : (typename K::U)(state[kPrefHi] >> hs);
  const long long n = P * R;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    if (!(mask[q] & 1)) continue;
    const long long p = q / R, i = q - p * R;
    const T v = sv[p * S + r0 + i];
    if (!(v == v)) continue;
    const typename K::U k = K::of(v);
    const unsigned d = (unsigned)(k >> shift) & 255u;
    if (first || (k >> hs) == plo) atomicAdd(&lh[0][d], 1u);
    if (first || (k >> hs) == phi) atomicAdd(&lh[1][d], 1u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 512; j += blockDim.x) {
    const unsigned c = lh[j >> 8][j & 255];
    if (c) atomicAdd(&hist[j], (unsigned long long)c);
  }
}

template <typename T>
__global__ void sf_median_pick_kernel(const unsigned long long* __restrict__ hist, int shift,
                                      unsigned long long* __restrict__ state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (shift + 8 >= Key<T>::kBits) {
    unsigned long long n = 0;
    for (int d = 0; d < 256; ++d) n += hist[d];
    state[kCount] = n;
    state[kPrefLo] = state[kPrefHi] = 0;
    state[kRankLo] = n ? (n - 1) / 2 : 0;
    state[kRankHi] = n / 2;
  }
  if (state[kCount] == 0) return;
  for (int j = 0; j < 2; ++j) {
    unsigned long long k = state[kRankLo + j], cum = 0;
    for (int d = 0; d < 256; ++d) {
      const unsigned long long c = hist[j * 256 + d];
      if (k < cum + c) {
        state[kPrefLo + j] |= (unsigned long long)d << shift;
        state[kRankLo + j] = k - cum;
        break;
      }
      cum += c;
    }
    if (shift == 0) {
      const double v = Key<T>::value(state[kPrefLo + j]);
      state[kValLo + j] = (unsigned long long)__double_as_longlong(v);
    }
  }
}

// ---- blackwell: connected components of Sv > threshold (8-connectivity), kept where they meet the angle mask --------
template <typename T>
__global__ __launch_bounds__(epa::kBlock) void sf_cc_init_kernel(const T* __restrict__ sv, long long P, long long S,
                                                                 long long r0, long long R, T thr,
                                                                 long long* __restrict__ par) {
  const long long n = P * R;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    const long long p = q / R, i = q - p * R;
    par[q] = sv[p * S + r0 + i] > thr ? q : -1;
  }
}

__global__ __launch_bounds__(epa::kBlock) void sf_cc_merge_kernel(long long* par, long long P, long long R,
                                                                  unsigned long long* err) {
  const long long n = P * R;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    if (ld(par + q) < 0) continue;
    const long long p = q / R, i = q - p * R;
    if (i > 0 && ld(par + q - 1) >= 0) uf_union(par, q, q - 1, n, err);
    if (p > 0) {
      const long long u = q - R;
      if (i > 0 && ld(par + u - 1) >= 0) uf_union(par, q, u - 1, n, err);
      if (ld(par + u) >= 0) uf_union(par, q, u, n, err);
      if (i + 1 < R && ld(par + u + 1) >= 0) uf_union(par, q, u + 1, n, err);
    }
  }
}

__global__ __launch_bounds__(epa::kBlock) void sf_cc_compress_kernel(long long* par, long long n,
                                                                     unsigned long long* err) {
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    if (ld(par + q) < 0) continue;
    st(par + q, uf_root(par, q, n, err));  // only roots are stored: every pixel ends on its root
  }
}

// a seed (foreground pixel under the angle mask) marks its root: bit 1 of the root's mask byte (bit 0 is only read)
__global__ __launch_bounds__(epa::kBlock) void sf_cc_seed_kernel(const long long* __restrict__ par, long long n,
                                                                 unsigned char* mask) {
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    const long long r = par[q];
    if (r >= 0 && (mask[q] & 1)) mask[r] |= 2;
  }
}

// per ping: the first crop sample whose component is kept -> depth0[r0 + i] - offset, else depth0[0] - offset
// (par == nullptr: nothing is kept anywhere -- the empty angle mask)
template <typename O>
__global__ __launch_bounds__(epa::kBlock) void sf_bottom_kernel(const long long* __restrict__ par,
                                                                const unsigned char* __restrict__ mask, long long P,
                                                                long long R, long long r0,
                                                                const double* __restrict__ depth0, double offset,
                                                                O* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (long long p = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); p < P; p += (long long)gridDim.x * kWaves) {
    long long idx = 0;
    if (par) {
      const long long* row = par + p * R;
      for (long long base = 0; base < R; base += 64) {
        const long long i = base + lane;
        bool kept = false;
        if (i < R) {
          const long long r = row[i];
          kept = r >= 0 && (mask[r] & 2);
        }
        const unsigned long long b = __ballot(kept);
        if (b) {
          idx = r0 + base + (__ffsll(b) - 1);
          break;
        }
      }
    }
    if (lane == 0) {
#pragma clang fp contract(off)
      out[p] = (O)depth0[idx] - (O)offset;
    }
  }
}

}  // namespace

extern "C" int epa_seafloor_depth_uniform(const void* depth, int dtype, long long P, long long S, int* bad_pings,
                                          epa_stream_t stream) {
  const char* who = "epa_seafloor_depth_uniform";
  EPA_CHECK_ARG(depth && bad_pings, "%s: NULL array argument", who);
  EPA_CHECK_ARG(P > 0 && S > 0, "%s: P=%lld S=%lld", who, P, S);
  EPA_CHECK_REAL(who, dtype);
  hipStream_t st = (hipStream_t)stream;
  return epa::dispatch_real(who, dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sf_depth_uniform_kernel<T><<<blocks_for_rows(P), epa::kBlock, 0, st>>>((const T*)depth, P, S, bad_pings);
    return epa::check_launch("sf_depth_uniform_kernel");
  });
}

extern "C" int epa_seafloor_basic(const void* sv, int dtype, long long P, long long S, long long skip, double tmin,
                                  double tmax, const double* depth0, double offset, double* out, epa_stream_t stream) {
  const char* who = "epa_seafloor_basic";
  EPA_CHECK_ARG(sv && depth0 && out, "%s: NULL array argument", who);
  EPA_CHECK_ARG(P > 0 && S > 0, "%s: P=%lld S=%lld", who, P, S);
  EPA_CHECK_ARG(skip >= 0 && skip < S, "%s: bin_skip %lld outside [0, %lld)", who, skip, S);
  EPA_CHECK_REAL(who, dtype);
  hipStream_t st = (hipStream_t)stream;
  return epa::dispatch_real(who, dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sf_basic_kernel<T><<<blocks_for_rows(P), epa::kBlock, 0, st>>>((const T*)sv, P, S, skip, (T)tmin, (T)tmax, depth0,
                                                                    offset, out);
    return epa::check_launch("sf_basic_kernel");
  });
}

namespace {
constexpr int kMedianHistWords = 512;  // two 256-bin histograms of one radix pass (sf_median_hist_kernel)
}  // namespace
size_t epa::scratch::seafloor_state(long long, long long, long long) {
  return sizeof(unsigned long long) * EPA_SEAFLOOR_STATE_WORDS;
}
// the window sums along range of both angles over the crop (sf_box_rows_kernel)
size_t epa::scratch::seafloor_angle_mask_work(long long P, long long R, long long) {
  return 2 * sizeof(double) * (size_t)P * (size_t)R;
}
size_t epa::scratch::seafloor_median_hist(long long, long long, long long) {
  return sizeof(unsigned long long) * kMedianHistWords;
}

extern "C" int epa_seafloor_angle_mask(const void* theta, const void* phi, int dtype, long long P, long long S,
                                       long long r0, long long R, int wtheta, int wphi, double ttheta, double tphi,
                                       double* work, unsigned char* mask, unsigned long long* state,
                                       epa_stream_t stream) {
  const char* who = "epa_seafloor_angle_mask";
  EPA_CHECK_ARG(theta && phi && work && mask && state, "%s: NULL array argument", who);
  EPA_CHECK_ARG(P > 0 && R > 0 && r0 >= 0 && r0 + R <= S, "%s: P=%lld S=%lld crop [%lld, +%lld)", who, P, S, r0, R);
  EPA_CHECK_ARG(wtheta > 0 && wphi > 0, "%s: windows must be positive (%d, %d)", who, wtheta, wphi);
  EPA_CHECK_REAL(who, dtype);
  hipStream_t st = (hipStream_t)stream;
  const int nb = blocks_for(P * R);
  return epa::dispatch_real(who, dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sf_box_rows_kernel<T><<<nb, epa::kBlock, 0, st>>>((const T*)theta, (const T*)phi, P, S, r0, R, wtheta, wphi, work);
    if (int rc = epa::check_launch("sf_box_rows_kernel")) return rc;
    sf_box_cols_kernel<<<nb, epa::kBlock, 0, st>>>(work, P, R, wtheta, wphi, ttheta, tphi, mask, state);
    return epa::check_launch("sf_box_cols_kernel");
  });
}

extern "C" int epa_seafloor_median(const void* sv, int dtype, long long P, long long S, long long r0, long long R,
                                   const unsigned char* mask, unsigned long long* state, unsigned long long* hist,
                                   epa_stream_t stream) {
  const char* who = "epa_seafloor_median";
  EPA_CHECK_ARG(sv && mask && state && hist, "%s: NULL array argument", who);
  EPA_CHECK_ARG(P > 0 && R > 0 && r0 >= 0 && r0 + R <= S, "%s: P=%lld S=%lld crop [%lld, +%lld)", who, P, S, r0, R);
  EPA_CHECK_REAL(who, dtype);
  hipStream_t st = (hipStream_t)stream;
  const int nb = blocks_for(P * R);
  return epa::dispatch_real(who, dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    for (int shift = (int)sizeof(T) * 8 - 8; shift >= 0; shift -= 8) {
      EPA_CHECK_HIP(hipMemsetAsync(hist, 0, epa::scratch::seafloor_median_hist(0, 0, 0), st));
      sf_median_hist_kernel<T><<<nb, epa::kBlock, 0, st>>>((const T*)sv, P, S, r0, R, mask, shift, state, hist);
      if (int rc = epa::check_launch("sf_median_hist_kernel")) return rc;
      sf_median_pick_kernel<T><<<1, 64, 0, st>>>(hist, shift, state);
      if (int rc = epa::check_launch("sf_median_pick_kernel")) return rc;
    }
    return EPA_OK;
  });
}

extern "C" int epa_seafloor_components(const void* sv, int dtype, long long P, long long S, long long r0, long long R,
                                       double threshold, unsigned char* mask, long long* parent,
                                       unsigned long long* state, epa_stream_t stream) {
  const char* who = "epa_seafloor_components";
  EPA_CHECK_ARG(sv && mask && parent && state, "%s: NULL array argument", who);
  EPA_CHECK_ARG(P > 0 && R > 0 && r0 >= 0 && r0 + R <= S, "%s: P=%lld S=%lld crop [%lld, +%lld)", who, P, S, r0, R);
  EPA_CHECK_REAL(who, dtype);
  hipStream_t st = (hipStream_t)stream;
  const long long n = P * R;
  const int nb = blocks_for(n);
  const int rc = epa::dispatch_real(who, dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sf_cc_init_kernel<T><<<nb, epa::kBlock, 0, st>>>((const T*)sv, P, S, r0, R, (T)threshold, parent);
    return epa::check_launch("sf_cc_init_kernel");
  });
  if (rc) return rc;
  sf_cc_merge_kernel<<<nb, epa::kBlock, 0, st>>>(parent, P, R, state + kError);
  if (int rc = epa::check_launch("sf_cc_merge_kernel")) return rc;
  sf_cc_compress_kernel<<<nb, epa::kBlock, 0, st>>>(parent, n, state + kError);
  if (int rc = epa::check_launch("sf_cc_compress_kernel")) return rc;
  sf_cc_seed_kernel<<<nb, epa::kBlock, 0, st>>>(parent, n, mask);
  return epa::check_launch("sf_cc_seed_kernel");
}

extern "C" int epa_seafloor_bottom(const long long* parent, const unsigned char* mask, long long P, long long R,
                                   long long r0, const double* depth0, double offset, void* out, int out_dtype,
                                   epa_stream_t stream) {
  const char* who = "epa_seafloor_bottom";
  EPA_CHECK_ARG(depth0 && out && (!parent || mask), "%s: NULL array argument", who);
  EPA_CHECK_ARG(P > 0 && (!parent || (R > 0 && r0 >= 0)), "%s: P=%lld R=%lld r0=%lld", who, P, R, r0);
  EPA_CHECK_REAL_OUT(who, out_dtype);
  hipStream_t st = (hipStream_t)stream;
  return epa::dispatch_real(who, out_dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sf_bottom_kernel<T><<<blocks_for_rows(P), epa::kBlock, 0, st>>>(parent, mask, P, R, r0, depth0, offset, (T*)out);
    return epa::check_launch("sf_bottom_kernel");
  });
}
