// The scaffolding of the kernels that reduce the pings of a time bin into range-bin accumulators held in LDS
// (fused_sv_mvbs.hip, chain_fast.hip): the accumulators themselves and a range column's cursor over the range bins.
// The lane map they share is epa::PairLanes (sample_math.h).  Written once, here: a change to how these kernels walk
// their pings is made in this file.
//
// Every piece is used only where the compiler's resource report of the kernel stayed what it was with the text written
// out (profiles/time_bin_resources.txt).  Two places keep their own text for that reason: the cursor of
// sv_denoise_mvbs_fast_kernel (BinCol, chain_fast.hip), and the loop over the columns near a range-bin edge in
// mvbs_of_sv_fixed_kernel and sv_denoise_mvbs_drift_kernel, which as a function taking a callable cost either kernel
// registers.
#pragma once
#include "ordered_key.h"
#include "sample_math.h"

namespace epa {

// The (sum, count) accumulators of a workgroup in dynamic LDS: sums at `smem`, counts at `smem + cnt_off`.  A kernel that
// holds several rows of them (one per time bin or ping block of its group) adds to row(first cell of the row): the row's
// two addresses are then formed once, not per column.
template <typename T>
struct BinAcc {
  T* sum;
  uint32_t* cnt;
  __device__ __forceinline__ BinAcc(T* sum_, uint32_t* cnt_) : sum(sum_), cnt(cnt_) {}
  __device__ __forceinline__ BinAcc(unsigned char* smem, unsigned cnt_off)
      : sum(reinterpret_cast<T*>(smem)), cnt(reinterpret_cast<uint32_t*>(smem + cnt_off)) {}
  __device__ __forceinline__ BinAcc row(int cell0) const { return BinAcc(sum + cell0, cnt + cell0); }
  // every lane of the workgroup; no barrier inside: the caller initialises its own shared variables, then synchronises
  __device__ __forceinline__ void clear(int n) const {
    for (int i = threadIdx.x; i < n; i += kBlock) {
      sum[i] = (T)0;
      cnt[i] = 0u;
    }
  }
  __device__ __forceinline__ void add(int cell, T s, uint32_t n) const {
    lds_add(sum + cell, s);
    atomicAdd(cnt + cell, n);
  }
  // every lane of the workgroup, after a barrier: the MVBS cells 10 log10(sum / count) (`fill` where nothing was
  // counted) and the optional raw partials, n cells from cell0 of the three arrays (gsum, gcnt: NULL or whole arrays)
  __device__ __forceinline__ void store(T* out, T* gsum, uint32_t* gcnt, size_t cell0, int n, T fill) const {
    out += cell0;
    gsum = gsum ? gsum + cell0 : nullptr;
    gcnt = gcnt ? gcnt + cell0 : nullptr;
    for (int i = threadIdx.x; i < n; i += kBlock) {
      const uint32_t k = cnt[i];
      const T s = sum[i];
      out[i] = k > 0u ? (T)10 * M<T>::log10(s / (T)k) : fill;
      if (gsum) gsum[i] = s;
      if (gcnt) gcnt[i] = k;
    }
  }
};

// Lane-private cursor of one range column over the range bins (kept across the pings of a time bin): the bin the column
// sits in, by index and by its edges, and what the column has summed since it entered it.
// ``n_clean`` (the fused kernel; 0u elsewhere): the pings of this chunk the whole wavefront took on the lean path so far
// (a scalar: every column of every lane got one valid value from each of them).  A column counts only what the general
// path added, relative to the scalar's value when the column last changed its bin: values in the bin = acc_cnt +
// n_clean (mod 2^32).
template <typename T>
struct BinCursor {
  double blo, bhi;  // edges of the range bin the column currently sits in (empty: blo > bhi)
  T acc_sum;
  int acc_rb;
  uint32_t acc_cnt;
  __device__ __forceinline__ void init() { blo = 1.0; bhi = 0.0; acc_sum = (T)0; acc_rb = -1; acc_cnt = 0u; }
  __device__ __forceinline__ bool inside(double x) const { return (x >= blo) & (x < bhi); }
  __device__ __forceinline__ void flush(const BinAcc<T>& acc, uint32_t n_clean) const {
    const uint32_t n = acc_cnt + n_clean;
    if (acc_rb >= 0 && n > 0u) acc.add(acc_rb, acc_sum, n);
  }
  // the column has left the range bin it sat in: find the new one (``valid`` false: a NaN coordinate, parked outside)
  __device__ __forceinline__ void rebin(double x, bool valid, double bin, double inv_bin, int n_rbins,
                                        const BinAcc<T>& acc, uint32_t n_clean) {
    const int rb = valid ? range_bin_index(x, bin, inv_bin, n_rbins, false) : -1;
    if (rb != acc_rb) {
      flush(acc, n_clean);
      acc_rb = rb;
      acc_sum = (T)0;
      acc_cnt = 0u - n_clean;
    }
    blo = rb >= 0 ? (double)rb * bin : 1.0;
    bhi = rb >= 0 ? (double)(rb + 1) * bin : 0.0;
  }
};

}  // namespace epa
