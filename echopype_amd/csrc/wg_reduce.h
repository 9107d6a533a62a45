// Wavefront and workgroup folds of the by-product statistics: {nanmin, nanmax, NaN count} of an echo_range or depth,
// {min, max} pairs of an actual_range, (sum, count) pairs -- one definition of what most kernels end with.
//
// THE CONTRACT, stated here once:
//   * a workgroup is kBlock lanes = kWaves wavefronts of kWave lanes, and every lane of it calls a fold;
//   * wave_min / wave_max / wave_sum walk __shfl_down over the offsets 32, 16, ... 1: LANE 0 of the wavefront holds
//     the result, the other lanes hold partial folds nobody may read;
//   * wave_sum_all walks __shfl_xor over the same offsets: every lane holds the result, with the same bits (each step
//     adds the same two numbers on both sides);
//   * block_fold: lane 0 of every wavefront stores to the caller's LDS array, ONE __syncthreads(), thread 0 combines
//     the four slots pairwise -- (w0 + w1) + (w2 + w3) for sums -- and only thread 0's value is the workgroup's.  A
//     call site inside a loop puts its own barrier in front, so that the previous trip is done with the slots.
// Where the result goes (a partial row, float atomics on a slot, NaN when lo > hi) stays with the call site.
#pragma once

#include "epa_internal.h"

namespace epa {

constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
static_assert(kWaves == 4, "the combines below are written out for four wavefront slots");

template <typename T>
__device__ __forceinline__ T wave_min(T x) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) x = fmin(x, __shfl_down(x, o, kWave));  // fmin / fmax ignore a NaN operand
  return x;
}
template <typename T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) x = fmax(x, __shfl_down(x, o, kWave));
  return x;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) x += __shfl_down(x, o, kWave);
  return x;
}
template <typename T>
__device__ __forceinline__ T wave_sum_all(T x) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
  return x;
}

// the four wavefront slots of one quantity, combined pairwise
__device__ __forceinline__ double slots_min(const double* s) { return fmin(fmin(s[0], s[1]), fmin(s[2], s[3])); }
__device__ __forceinline__ double slots_max(const double* s) { return fmax(fmax(s[0], s[1]), fmax(s[2], s[3])); }
__device__ __forceinline__ double slots_sum(const double* s) { return (s[0] + s[1]) + (s[2] + s[3]); }

// {min, max} of the numbers a lane has seen; an empty pair has lo > hi
struct MinMax {
  double lo = __builtin_inf(), hi = -__builtin_inf();
  __device__ __forceinline__ void take(double v) {
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
  __device__ __forceinline__ void wave_fold() {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      lo = fmin(lo, __shfl_down(lo, o, kWave));
      hi = fmax(hi, __shfl_down(hi, o, kWave));
    }
  }
  __device__ __forceinline__ void block_fold(double* lds /* 2 * kWaves doubles of LDS */) {
    wave_fold();
    if ((threadIdx.x & (kWave - 1)) == 0) {
      lds[threadIdx.x / kWave] = lo;
      lds[kWaves + threadIdx.x / kWave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      lo = slots_min(lds);
      hi = slots_max(lds + kWaves);
    }
  }
};

// {nanmin, nanmax, NaN count}: what compute_MVBS and add_depth ask of a range variable
struct RangeStats {
  double lo = __builtin_inf(), hi = -__builtin_inf(), nn = 0.0;
  __device__ __forceinline__ void take(double v) {
    lo = fmin(lo, v);
    hi = fmax(hi, v);
    nn += v == v ? 0.0 : 1.0;
  }
  __device__ __forceinline__ void wave_fold() {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      lo = fmin(lo, __shfl_down(lo, o, kWave));
      hi = fmax(hi, __shfl_down(hi, o, kWave));
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) nn += __shfl_down(nn, o, kWave);
  }
  __device__ __forceinline__ void block_fold(double* lds /* 3 * kWaves doubles of LDS */) {
    wave_fold();
    if ((threadIdx.x & (kWave - 1)) == 0) {
      lds[threadIdx.x / kWave] = lo;
      lds[kWaves + threadIdx.x / kWave] = hi;
      lds[2 * kWaves + threadIdx.x / kWave] = nn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      lo = slots_min(lds);
      hi = slots_max(lds + kWaves);
      nn = slots_sum(lds + 2 * kWaves);
    }
  }
};

struct SumCount {
  double sum = 0.0, cnt = 0.0;
  __device__ __forceinline__ void wave_fold() {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      sum += __shfl_down(sum, o, kWave);
      cnt += __shfl_down(cnt, o, kWave);
    }
  }
  __device__ __forceinline__ void block_fold(double* lds /* 2 * kWaves doubles of LDS */) {
    wave_fold();
    if ((threadIdx.x & (kWave - 1)) == 0) {
      lds[threadIdx.x / kWave] = sum;
      lds[kWaves + threadIdx.x / kWave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      sum = slots_sum(lds);
      cnt = slots_sum(lds + kWaves);
    }
  }
};

// the wavefront half of a NaN-skipping minimum: lane 0 holds the smallest m and whether any lane had a value
template <typename T>
__device__ __forceinline__ void wave_nanmin(T& m, int& any) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    m = fmin(m, __shfl_down(m, o, kWave));
    any |= __shfl_down(any, o, kWave);
  }
}

// NaN-skipping min over the workgroup, known to every lane; NaN when no lane contributed.  (Two barriers: the first
// lets a caller in a loop reuse scratch.)
template <typename T>
__device__ T block_nanmin(T v, bool valid, T* scratch /* >= 2 * kWaves elements of LDS */) {
  const T inf = (T)__builtin_inf();
  T m = valid ? v : inf;
  int any = valid ? 1 : 0;
  wave_nanmin(m, any);
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  __syncthreads();
  if (lane == 0) {
    scratch[wave] = m;
    scratch[kWaves + wave] = (T)any;
  }
  __syncthreads();
  T r = inf;
  int a = 0;
  for (int w = 0; w < kWaves; ++w) {
    r = fmin(r, scratch[w]);
    a |= (scratch[kWaves + w] != (T)0);
  }
  return a ? r : M<T>::nan();
}

}  // namespace epa
