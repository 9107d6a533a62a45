// Order-preserving integer keys of floating-point values, and the small device helpers of the kernels that publish them.
//
// Every by-product a pass leaves in HBM as a minimum or a maximum -- nanmax(echo_range) and the {nanmin, nanmax, NaN
// count} statistics, the actual_range of Sv_noise / Sv_corrected, the region extrema, the rb and d spans, the radix
// keys of the medians -- travels as such a key: kernels lower or raise it with atomicMin / atomicMax on the integer and
// a single-lane kernel (or the host: ops._unkey) decodes it afterwards.  THE CONTRACT, stated here once:
//   * ordered_key is strictly increasing over all non-NaN values, -inf and +inf included: x < y => key(x) < key(y);
//   * -0.0 < +0.0 as keys (the one place where the keys order what the values call equal);
//   * key_value(ordered_key(x)) has the bits of x;
//   * no non-NaN value maps to kKeyNoMax (0) or kKeyNoMin (all ones): a slot that starts at its sentinel and still
//     holds it was never touched.  (The two NaNs with every payload bit set are the only bit patterns there.)
//   * key_value does not know the sentinels: a kernel that wants "untouched decodes to NaN" tests the slot against its
//     sentinel BEFORE it calls key_value.
// The first part is plain C++ (tools/ordered_key_check.cpp builds it with a host compiler); the device helpers follow
// under __HIPCC__.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EPA_KEY_FN __host__ __device__ __forceinline__
#else
#define EPA_KEY_FN inline
#endif

namespace epa {

constexpr unsigned long long kKeyNoMax = 0ull;   // start of a maximum: below the key of every number
constexpr unsigned long long kKeyNoMin = ~0ull;  // start of a minimum: above the key of every number

// the bits of a value and back.  (Device code keeps HIP's intrinsics: the kernels were tuned on the instructions the
// compiler makes of those, and it makes a v_xor of the same expression on a __builtin_bit_cast where it made a v_or.)
#if defined(__HIP_DEVICE_COMPILE__)
EPA_KEY_FN unsigned long long key_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
EPA_KEY_FN unsigned key_bits(float v) { return __float_as_uint(v); }
EPA_KEY_FN double key_from_bits(unsigned long long b) { return __longlong_as_double((long long)b); }
EPA_KEY_FN float key_from_bits(unsigned b) { return __uint_as_float(b); }
#else
EPA_KEY_FN unsigned long long key_bits(double v) { return __builtin_bit_cast(unsigned long long, v); }
EPA_KEY_FN unsigned key_bits(float v) { return __builtin_bit_cast(unsigned, v); }
EPA_KEY_FN double key_from_bits(unsigned long long b) { return __builtin_bit_cast(double, b); }
EPA_KEY_FN float key_from_bits(unsigned b) { return __builtin_bit_cast(float, b); }
#endif

EPA_KEY_FN unsigned long long ordered_key(double v) {
  const unsigned long long b = key_bits(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
EPA_KEY_FN double key_value(unsigned long long k) {
  return key_from_bits((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}
EPA_KEY_FN unsigned ordered_key(float v) {
  const unsigned b = key_bits(v);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
EPA_KEY_FN float key_value(unsigned k) { return key_from_bits((k >> 31) ? (k & 0x7fffffffu) : ~k); }

}  // namespace epa

#undef EPA_KEY_FN

#if defined(__HIPCC__)
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "wg_reduce.h"

namespace epa {

// {min, max, min, max} running values of one lane's samples (fmin / fmax: a NaN operand is ignored; an empty pair has
// min > max) -> the four keys.  publish_minmax_keys is for the one lane that holds the reduced values.
__device__ __forceinline__ void publish_minmax_keys(const double (&mm)[4], unsigned long long* keys) {
  if (mm[0] <= mm[1]) {
    atomicMin(keys + 0, ordered_key(mm[0]));
    atomicMax(keys + 1, ordered_key(mm[1]));
  }
  if (mm[2] <= mm[3]) {
    atomicMin(keys + 2, ordered_key(mm[2]));
    atomicMax(keys + 3, ordered_key(mm[3]));
  }
}
// the two pairs folded over the wavefront (every lane calls it; lane 0 holds the result)
template <typename U>
__device__ __forceinline__ void wave_fold_minmax4(U (&mm)[4]) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    mm[0] = fmin(mm[0], __shfl_down(mm[0], o, kWave));
    mm[1] = fmax(mm[1], __shfl_down(mm[1], o, kWave));
    mm[2] = fmin(mm[2], __shfl_down(mm[2], o, kWave));
    mm[3] = fmax(mm[3], __shfl_down(mm[3], o, kWave));
  }
}
// every lane of the wavefront calls it; lane 0 publishes
__device__ __forceinline__ void wave_publish_minmax_keys(double (&mm)[4], unsigned long long* keys) {
  if (!keys) return;
  wave_fold_minmax4(mm);
  if ((threadIdx.x & 63) == 0) publish_minmax_keys(mm, keys);
}

// {max, min, NaN count} of the binned coordinate seen by a workgroup -> rmax_key and, when given, rstat[0] (the
// minimum's key) and rstat[1] (the count): wavefront reduction, then the workgroup's four wavefronts meet in LDS, then
// ONE lane sends at most three atomics WITHOUT a return value -- nobody waits for them.  Measured round 6 (4 x 100 000
// x 2000 fp64, ms per launch): one atomic per wavefront and key 1.96-2.12 (2.5 with the three words in one 128-byte
// line: the L2 serialises a line's atomics); per workgroup, filtered by a read of the current keys 2.05 (the read is
// what a workgroup then waits for); per workgroup, unconditional 1.82 = the kernel without the statistics.  The words
// live in different 128-byte lines where the caller's layout allows.
// Every lane of the workgroup calls it (one barrier), with nnan the WAVEFRONT's count already; lds_keys = {kKeyNoMax,
// kKeyNoMin} and *lds_nnan = 0 were set before a barrier of the caller's.
__device__ __forceinline__ void wg_publish_range_keys(double xmax, double xmin, unsigned nnan,
                                                      unsigned long long* lds_keys, unsigned* lds_nnan,
                                                      unsigned long long* rmax_key, unsigned long long* rstat) {
  xmax = wave_max(xmax);
  xmin = wave_min(xmin);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (xmax > -__builtin_inf()) atomicMax(&lds_keys[0], ordered_key(xmax));
    if (xmin < __builtin_inf()) atomicMin(&lds_keys[1], ordered_key(xmin));
    if (nnan > 0u) atomicAdd(lds_nnan, nnan);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long kmax = lds_keys[0], kmin = lds_keys[1];
    if (kmax != kKeyNoMax) atomicMax(rmax_key, kmax);
    if (rstat) {  // the rest of {nanmin, nanmax, NaN count}: what compute_MVBS asks of its range variable
      if (kmin != kKeyNoMin) atomicMin(rstat, kmin);
      if (*lds_nnan > 0u) atomicAdd(rstat + 1, (unsigned long long)*lds_nnan);
    }
  }
}

// v_max / v_min as the hardware has them: the operand that is a number (IEEE maxNum / minNum), without the
// canonicalising copies clang's fmax() / fmin() add
__device__ __forceinline__ double vmax_num(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float vmax_num(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double vmin_num(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float vmin_num(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// the floating-point add without a return value (ds_add_f64 / ds_add_f32 on LDS, global_atomic_add_* on HBM)
template <typename T>
__device__ __forceinline__ void lds_add(T* p, T v) {
  unsafeAtomicAdd(p, v);
}

// "This time bin is left to the next kernel": a specialised kernel that declines a bin writes the mark into the bin's
// first MVBS cell, and the kernel launched after it takes the marked bins only (and overwrites the cell).  The mark is
// a NaN payload no computation produces; each hand-over has its own pair (a cell is eight bytes, or four on float
// grids).
template <unsigned long long kBits64, unsigned kBits32>
struct LeftMark {
  static __device__ __forceinline__ bool is_marked(const double* cell) {
    return *reinterpret_cast<const unsigned long long*>(cell) == kBits64;
  }
  static __device__ __forceinline__ bool is_marked(const float* cell) {
    return *reinterpret_cast<const unsigned*>(cell) == kBits32;
  }
  static __device__ __forceinline__ void mark(double* cell) { *reinterpret_cast<unsigned long long*>(cell) = kBits64; }
  static __device__ __forceinline__ void mark(float* cell) { *reinterpret_cast<unsigned*>(cell) = kBits32; }
};

}  // namespace epa
#endif  // __HIPCC__
