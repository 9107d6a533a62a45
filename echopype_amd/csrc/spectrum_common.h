// What the two broadband spectrum products share (target_spectrum.hip: TS(f) of single targets; sv_spectrum.hip: Sv(f)
// of range cells): the replica in LDS with its energy, the replica-table kernel and the staging of a span of one ping.
// One definition each, so that both products read the same replica and the same zero fill.
//
// The functions are templates over the `Args` of the translation unit, which holds
//   replica, replica_off, replica_len, max_taps, R   the replicas (interleaved f32, offsets in complex elements)
//   rep_dt [R], fparams [R][Args::kFParams][F], F    per replica: sample interval; row 0 of fparams is f in Hz
//   h                                                the largest lag of A(f)
//   table [R][Args::kTableRows][F], xs_off           the output of replica_table_kernel; where its lags go in LDS
#pragma once

#include "wg_reduce.h"

namespace epa {
namespace spectrum {

struct Cd {
  double re, im;
};

// the taps of replica r, or 0 when its offsets do not describe 1 .. max_taps taps inside the array
template <class Args>
__device__ __forceinline__ int replica_taps(const Args& a, int r, int& r0) {
  r0 = a.replica_off[r];
  const long long r1 = a.replica_off[r + 1];
  const long long L = r1 - r0;
  return (r0 >= 0 && r1 <= a.replica_len && L >= 1 && L <= a.max_taps) ? (int)L : 0;
}

// replica -> LDS as float64 (conj is applied in the MAC); E = sum |tx|^2, the same bits in every lane and in every kernel
template <class Args>
__device__ __forceinline__ double stage_replica(const Args& a, int r0, int L, Cd* rep, double* red) {
  double part = 0.0;
  for (int k = threadIdx.x; k < L; k += kBlock) {
    const Cd t{(double)a.replica[2 * (size_t)(r0 + k)], (double)a.replica[2 * (size_t)(r0 + k) + 1]};
    rep[k] = t;
    part += t.re * t.re + t.im * t.im;
  }
  part = wave_sum(part);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = part;
  __syncthreads();
  return slots_sum(red);
}

// per replica: E = sum |tx|^2, the autocorrelation a(m), m <= min(h, L - 1), and per frequency the step
// w = exp(-2 pi i f dt) and 1 / |A(f)|^2 -> table.  Dynamic LDS: the replica, then a(0 .. h) at xs_off.
template <class Args>
__global__ __launch_bounds__(kBlock) void replica_table_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Cd* rep = reinterpret_cast<Cd*>(smem);
  Cd* ac = reinterpret_cast<Cd*>(smem + a.xs_off);  // a(0 .. hh)
  __shared__ double red[kWaves];
  constexpr int kTab = Args::kTableRows, kFP = Args::kFParams;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  double* tab = a.table + (size_t)r * kTab * a.F;
  int r0;
  const int L = replica_taps(a, r, r0);
  if (L == 0) {  // (uniform) nothing is served by this replica
    for (int j = tid; j < a.F; j += kBlock) tab[j] = tab[a.F + j] = tab[2 * a.F + j] = __builtin_nan("");
    return;
  }
  const double E = stage_replica(a, r0, L, rep, red);
  const int hh = a.h < L - 1 ? a.h : L - 1;
  // a(m) = (1/E) sum_k tx(k+m) conj(tx(k)): a wavefront per lag, the lanes stride over k
  for (int m = wave; m <= hh; m += kWaves) {
    double sr = 0.0, si = 0.0;
    for (int k = lane; k + m < L; k += kWave) {
      const Cd x = rep[k + m], t = rep[k];
      sr += x.re * t.re + x.im * t.im;
      si += x.im * t.re - x.re * t.im;
    }
    sr = wave_sum(sr), si = wave_sum(si);
    if (lane == 0) ac[m] = Cd{sr / E, si / E};
  }
  __syncthreads();
  const double dt = a.rep_dt[r];
  const double* fp = a.fparams + (size_t)r * kFP * a.F;
  for (int j = tid; j < a.F; j += kBlock) {
    double ws, wc;
    ::sincospi(-2.0 * (fp[j] * dt), &ws, &wc);  // w = exp(-2 pi i f dt)
    // A = a(0) + sum_{m >= 1} a(m) w^m + conj(a(m)) conj(w^m)      (a(-m) = conj(a(m)), |w| = 1)
    double Ar = ac[0].re, Ai = ac[0].im, pr = 1.0, pi = 0.0;
    for (int m = 1; m <= hh; ++m) {
      const double qr = pr * wc - pi * ws, qi = pr * ws + pi * wc;
      pr = qr, pi = qi;
      const Cd v = ac[m];
      Ar += 2.0 * (v.re * pr - v.im * pi);  // a w^m + conj(a w^m) ... conj(a) conj(p) = conj(a p)
    }
    tab[j] = wc;
    tab[a.F + j] = ws;
    tab[2 * a.F + j] = 1.0 / (Ar * Ar + Ai * Ai);
  }
}

// samples [first, first + len) of one ping -> xs: the sum of the valid sectors (only < 0) or sector `only` alone; the
// validity bits of every sample -> vmask (only < 0).  Samples outside [0, S) are zero with no valid sector.
template <typename InT>
__device__ __forceinline__ unsigned stage_window(const InT* __restrict__ re, const InT* __restrict__ im, size_t ping_base,
                                                 long long S, int B, long long first, int len, int only, Cd* xs,
                                                 uint8_t* vmask) {
  unsigned mixed = 0;
  const unsigned full = (1u << B) - 1u;
  for (int i = threadIdx.x; i < len; i += kBlock) {
    const long long n = first + i;
    double sr = 0.0, si = 0.0;
    unsigned m = 0;
    if (n >= 0 && n < S) {
      const InT* pr = re + ping_base + (size_t)n * B;
      const InT* pi = im + ping_base + (size_t)n * B;
      for (int b = 0; b < B; ++b) {
        const InT vr = pr[b], vi = pi[b];
        if (vr == vr && vi == vi) {
          m |= 1u << b;
          if (only < 0 || only == b) sr += (double)vr, si += (double)vi;
        }
      }
    }
    xs[i] = Cd{sr, si};
    if (only < 0) {
      vmask[i] = (uint8_t)m;
      if (m != 0u && m != full) mixed = 1u;
    }
  }
  return mixed;
}

}  // namespace spectrum
}  // namespace epa
