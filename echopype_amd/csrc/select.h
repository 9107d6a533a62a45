// Exact order statistics of a window of dB values by radix selection, shared by the noise masks (noise_masks.hip:
// NaN-skipping medians of the LINEAR values) and the transient-noise detectors (transient.hip: medians, the 75th
// percentile in the linear domain, a percentile in dB).
//
// 10^(x/10) is monotone, so the order statistics of the linear values are those of x: the selection runs on the dB
// values and returns the values at two neighbouring ranks k and k + 1 of the non-NaN values, from which the caller
// interpolates in whichever domain it needs (a median of an even count averages the two middle linear values, as
// np.nanmedian(_log2lin(.)) does; np.percentile interpolates linearly between floor((N - 1) q) and the next rank).
// Which rank is wanted is a function of the count N, known only after the first sweep: a RANK functor
//     unsigned operator()(unsigned N, bool& next) const      -> k < N; next: the value at rank k + 1 is wanted too
// All functions here are called by every thread of a 256-thread workgroup.
#pragma once
#include "fast_math.h"
#include "ordered_key.h"

namespace epa {
namespace sel {

// scipy.ndimage / dask_image mode="reflect":  d c b a | a b c d | d c b a   (period 2n)
__device__ __forceinline__ int reflect_index(int i, int n) {
  const int period = 2 * n;
  i %= period;
  if (i < 0) i += period;
  return i < n ? i : period - 1 - i;
}

// ------------------------------------------------------------------------------------------------
// workgroup reductions (256 threads = 4 wavefronts); every thread gets the result
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* sh4) {
  v = epa::wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh4[0] + sh4[1] + sh4[2] + sh4[3];
}

__device__ __forceinline__ unsigned long long block_min(unsigned long long v, unsigned long long* sh4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_down(v, o, 64);
    v = w < v ? w : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = sh4[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) r = sh4[i] < r ? sh4[i] : r;
  return r;
}

// the selection runs on the order-preserving keys of the values (ordered_key.h)
using epa::key_value;
using epa::ordered_key;

template <typename T>
struct Window {
  const T* base;  // channel base pointer
  int S;          // row stride
  int p_lo, np;   // pings p_lo .. p_lo+np-1
  int s_lo, ns;   // samples s_lo .. s_lo+ns-1
  int P, s0;      // reflect domain: pings [0,P), samples [s0,S)
  bool reflect;
  // calls f(value) for every element this thread owns
  template <typename F>
  __device__ __forceinline__ void for_each(F f) const {
    const int ne = np * ns;
    for (int i = threadIdx.x; i < ne; i += kBlock) {
      const int ip = i / ns, is = i - ip * ns;
      int p = p_lo + ip, s = s_lo + is;
      if (reflect) {
        p = reflect_index(p, P);
        s = s0 + reflect_index(s - s0, S - s0);
      }
      f((double)base[(size_t)p * S + s]);
    }
  }
};

constexpr int kCandCap = 2048;  // candidates kept in LDS once the selected radix bucket is this small

template <int CAP>
struct SelectScratchT {
  static constexpr int kCap = CAP;
  unsigned hist[256];
  unsigned u4[4];
  unsigned long long q4[4];
  unsigned digit, krem, bucket, ncand;
  unsigned long long cand[CAP];
};
using SelectScratch = SelectScratchT<kCandCap>;

// the lower median rank; the upper one is wanted when the count is even
struct MedianRank {
  __device__ __forceinline__ unsigned operator()(unsigned N, bool& next) const {
    next = (N & 1u) == 0u;
    return (N - 1u) / 2u;
  }
};

// np.percentile / np.nanpercentile, method "linear": virtual index (N - 1) * (q / 100), the value at its floor and,
// when it has a fractional part, the next one
struct PercentileRank {
  double q;  // percent, 0 .. 100
  __device__ __forceinline__ double virtual_index(unsigned N) const { return (double)(N - 1u) * (q / 100.0); }
  __device__ __forceinline__ unsigned operator()(unsigned N, bool& next) const {
    const double v = virtual_index(N);
    const double f = floor(v);
    unsigned k = (unsigned)fmin(fmax(f, 0.0), (double)(N - 1u));
    next = v > f && k + 1u < N;
    return k;
  }
  // numpy's _lerp(a, b, t) between the two selected values
  __device__ __forceinline__ double lerp(double a, double b, unsigned N) const {
    const double v = virtual_index(N);
    const double t = v - floor(v);
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
  }
};

// One 8-bit radix step of the selection: histogram of digit (key >> shift) & 255 over the keys that
// `each` enumerates and that match `prefix` on the bits above the digit; picks the bucket holding
// rank k.  Returns the total number of keys counted; updates prefix / k; *bucket = size of the bucket.
template <typename Each, typename SC, typename Rank>
__device__ __forceinline__ unsigned radix_step(Each each, SC* sc, int shift,
                                               unsigned long long& prefix, unsigned& k, unsigned& bucket,
                                               bool k_known, unsigned* total_out, Rank rank, bool* next_out) {
  __syncthreads();
  sc->hist[threadIdx.x] = 0u;  // kBlock == 256
  __syncthreads();
  const unsigned long long hi_mask = shift == 56 ? 0ull : (~0ull << (shift + 8));
  unsigned* hist = sc->hist;
  const unsigned long long pre = prefix;
  each([&](unsigned long long key) {
    if ((key & hi_mask) == pre) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
  });
  __syncthreads();
  if (!k_known) {  // first step: the histogram total is the number of valid values, which decides the rank
    const unsigned total = block_sum(sc->hist[threadIdx.x], sc->u4);
    *total_out = total;
    if (total == 0u) return 0u;
    k = rank(total, *next_out);
  }
  if (threadIdx.x < 64) {
    const unsigned l = threadIdx.x;
    const unsigned h0 = sc->hist[4 * l], h1 = sc->hist[4 * l + 1], h2 = sc->hist[4 * l + 2],
                   h3 = sc->hist[4 * l + 3];
    const unsigned tot = h0 + h1 + h2 + h3;
    unsigned incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(incl, o, 64);
      if ((int)l >= o) incl += t;
    }
    const unsigned excl = incl - tot;
    if (excl <= k && k < incl) {
      unsigned r = k - excl, d;
      if (r < h0) d = 0;
      else if ((r -= h0) < h1) d = 1;
      else if ((r -= h1) < h2) d = 2;
      else { r -= h2; d = 3; }
      sc->digit = 4 * l + d;
      sc->krem = r;
      sc->bucket = d == 0 ? h0 : (d == 1 ? h1 : (d == 2 ? h2 : h3));
    }
  }
  __syncthreads();
  prefix |= (unsigned long long)sc->digit << shift;
  k = sc->krem;
  bucket = sc->bucket;
  return 1u;
}

// Selects, among the non-NaN x of the window, the value at the rank k = rank(N) and, if the functor asks for it, the
// one at k + 1 (key2 == key1 otherwise), as sort keys.  n_valid = N; returns false when it is 0.
// The window is swept from memory only until the bucket that holds the rank has at most kCandCap
// members (typically 2 sweeps for a 16 k-element block of dB values, 0 for a small window); those
// candidates are then gathered into LDS in one more sweep and the remaining digits are resolved there.
template <typename W, typename SC, typename Rank>
__device__ bool window_select(const W& w, SC* sc, Rank rank, unsigned& n_valid, unsigned long long& key1,
                              unsigned long long& key2, int size_hint = 0x7fffffff) {
  constexpr int kCandCap = SC::kCap;  // (shadows the default capacity)
  auto each_global = [&](auto f) {
    w.for_each([&](double v) {
      if (v == v) f(ordered_key(v));
    });
  };
  unsigned long long prefix = 0ull;
  unsigned k = 0u, bucket = 0xffffffffu, N = 0u, k_all = 0u;
  bool k_known = false, next = false;
  int shift = 64;  // bits [shift, 64) of the selected key are decided
  if (size_hint > kCandCap) {
    while (shift > 0 && bucket > (unsigned)kCandCap) {
      shift -= 8;
      if (!radix_step(each_global, sc, shift, prefix, k, bucket, k_known, &N, rank, &next)) {
        n_valid = 0u;
        return false;
      }
      if (!k_known) {
        bool unused;
        k_all = rank(N, unused);
      }
      k_known = true;
    }
  }
  if (shift == 0) {
    // resolved entirely from memory (a bucket of > kCandCap equal values): one more sweep for the next rank
    key1 = key2 = prefix;
    if (next) {
      unsigned le = 0;
      unsigned long long gt = ~0ull;
      each_global([&](unsigned long long key) {
        if (key <= prefix) ++le;
        else gt = key < gt ? key : gt;
      });
      const unsigned n_le = block_sum(le, sc->u4);
      const unsigned long long min_gt = block_min(gt, sc->q4);
      if (n_le < k_all + 2u) key2 = min_gt;
    }
  } else {
    // gather the candidates (keys matching the decided bits) into LDS; remember the smallest key above them
    const unsigned long long dmask = shift == 64 ? 0ull : (~0ull << shift);
    __syncthreads();
    if (threadIdx.x == 0) sc->ncand = 0u;
    __syncthreads();
    unsigned long long above = ~0ull;
    unsigned* ncand = &sc->ncand;
    unsigned long long* cand = sc->cand;
    const unsigned long long pre = prefix;
    each_global([&](unsigned long long key) {
      const unsigned long long hi = key & dmask;
      if (hi == pre) {
        const unsigned at = atomicAdd(ncand, 1u);
        if (at < (unsigned)kCandCap) cand[at] = key;
      } else if (hi > pre) {
        above = key < above ? key : above;
      }
    });
    const unsigned long long min_above = block_min(above, sc->q4);  // (barriers inside publish cand / ncand)
    const unsigned M = sc->ncand;
    if (!k_known) {  // small window gathered whole: M is the number of valid values
      N = M;
      if (N == 0u) {
        n_valid = 0u;
        return false;
      }
      k = rank(N, next);
    }
    const unsigned r0 = k;  // the wanted rank inside the candidate set
    auto each_cand = [&](auto f) {
      for (unsigned i = threadIdx.x; i < M; i += kBlock) f(cand[i]);
    };
    unsigned dummy;
    bool dummy_next;
    while (shift > 0) {
      shift -= 8;
      radix_step(each_cand, sc, shift, prefix, k, bucket, true, &dummy, rank, &dummy_next);
    }
    key1 = key2 = prefix;
    if (next) {
      unsigned le = 0;
      unsigned long long gt = ~0ull;
      each_cand([&](unsigned long long key) {
        if (key <= prefix) ++le;
        else gt = key < gt ? key : gt;
      });
      const unsigned n_le = block_sum(le, sc->u4);
      const unsigned long long min_gt = block_min(gt, sc->q4);
      if (n_le < r0 + 2u) key2 = (min_gt != ~0ull) ? min_gt : min_above;
    }
  }
  n_valid = N;
  return true;
}

// Returns the median of 10^(x/10) over the non-NaN x of the window; n_valid = their count (the
// result is NaN when it is 0).  Must be called by all threads of the workgroup.
template <typename W, typename SC>
__device__ double window_median_lin(const W& w, SC* sc, const double* exp2_tab,
                                    unsigned& n_valid, int size_hint = 0x7fffffff) {
  unsigned long long key1, key2;
  if (!window_select(w, sc, MedianRank{}, n_valid, key1, key2, size_hint)) return __builtin_nan("");
  const double a = lin_from_db(key_value(key1), exp2_tab);
  return key1 == key2 ? a : (a + lin_from_db(key_value(key2), exp2_tab)) * 0.5;
}

}  // namespace sel
}  // namespace epa
