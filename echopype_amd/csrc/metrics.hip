// metrics: the echo summary statistics of Urmy et al. 2012 per row (reference: echopype metrics/summary_statistics.py:
// abundance, center_of_mass, dispersion, evenness, aggregation).  A row is every sample of one ping; with r the range,
// for j = 1 .. S-1:  dz_j = r_j - r_{j-1} in the type of r (0 -> NaN),  sv_j = 10^(Sv_j / 10),  w_j = sv_j dz_j,
//   A = sum w_j,  B = sum r_j w_j,  Q = sum sv_j^2 dz_j,  I = sum (r_j - cm)^2 w_j,
// every sum skipping its NaN terms (xarray's sum: an all-NaN row sums to 0), and
//   abundance = 10 log10 A,  center_of_mass = B / A,  dispersion = I / A,  evenness = A^2 / Q,  aggregation = Q / A^2.
// One sweep: a row belongs to one wave or one workgroup, which holds it in registers, reduces A, B and Q, forms
// cm = B / A and then takes I about THAT cm from the registers -- never the expanded form sum r^2 w - 2 cm sum r w +
// cm^2 sum w, which for a thin layer far away cancels most digits (0.1 m at 10 km: eleven).  Rows too long for
// registers are read twice, the second time from L2.  No atomics: the result does not depend on scheduling.
#include "wg_reduce.h"

namespace {

using epa::kBlock;

using epa::kWave;
using epa::kWaves;
constexpr int kGroups = 8;  // groups of 4 samples of each array a lane keeps in registers
constexpr long long kWaveRow = (long long)kWave * 4 * kGroups;    // 2048: longest row one wave holds
constexpr long long kBlockRow = (long long)kBlock * 4 * kGroups;  // 8192: longest row one workgroup holds
constexpr int kMaxGrid = 65536;  // workgroups of a launch unless the caller sets fewer; owners take further rows in a loop

constexpr unsigned kNeedB = 1u, kNeedQ = 2u, kNeedI = 4u;

struct MetricsArgs {
  const void* sv;
  const void* range;
  long long range_stride;  // S: a range row per row of sv; 0: one row shared by all
  long long R, S;
  const double* cm_in;  // NULL: I about the row's own B / A
  void* abundance;
  void* center_of_mass;
  void* dispersion;
  void* evenness;
  void* aggregation;
  unsigned need;
  int max_grid;
};

template <typename T>
__device__ __forceinline__ T mt_nan();
template <>
__device__ __forceinline__ float mt_nan<float>() { return __builtin_nanf(""); }
template <>
__device__ __forceinline__ double mt_nan<double>() { return __builtin_nan(""); }

// 10^(v / 10) in the type of the samples: float32 as the other float32 kernels take it (fast_math.h lin_from_db)
__device__ __forceinline__ float mt_linear(float v) { return ::exp10f(v * 0.1f); }
__device__ __forceinline__ double mt_linear(double v) { return ::exp10(v * 0.1); }

// samples j0 .. j0+3 of a row of S: a whole group is one 16-byte load of float32, two of float64.  AL: every row starts
// on a multiple of 16 bytes and holds whole groups' worth of bytes; otherwise the load is issued with the alignment of
// an element (global memory is accessed in unaligned mode under the HSA ABI).  The group that crosses the end of the
// row is read element by element, NaN past the end: a NaN sample makes NaN terms, which every sum skips.
template <typename T, bool AL>
__device__ __forceinline__ void mt_load4(const T* row, long long j0, long long S, T (&v)[4]) {
  if (j0 + 4 <= S) {
    if (AL) {
      __builtin_memcpy(v, __builtin_assume_aligned(row + j0, 16), 4 * sizeof(T));
    } else {
      __builtin_memcpy(v, __builtin_assume_aligned(row + j0, sizeof(T)), 4 * sizeof(T));
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (j0 + e < S) ? row[j0 + e] : mt_nan<T>();
  }
}

// r_{j0-1}: the last range of the lane before this one, which holds the group before; the first lane of a wave reads
// it (a line its neighbour wave has just fetched).  NaN for j0 = 0 (sample 0 has no dz) and past the row.
// Called by all lanes of the wave.
template <typename T>
__device__ __forceinline__ T mt_prev(const T* rg, long long j0, long long S, const T (&r)[4]) {
  T p = __shfl_up(r[3], 1, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) p = (j0 > 0 && j0 <= S) ? rg[j0 - 1] : mt_nan<T>();
  return p;
}

__device__ __forceinline__ double mt_skipna(double x) { return x == x ? x : 0.0; }

struct Sums {
  double A, B, Q, I;
};

// dz of element e of a group, in the type of the range
template <typename T>
__device__ __forceinline__ T mt_dz(const T (&r)[4], T prev, int e) {
  const T dz = r[e] - (e ? r[e - 1] : prev);
  return dz == (T)0 ? mt_nan<T>() : dz;
}

// One group of the first pass: v is replaced by its linear values (the second pass reads them).  The per-sample values
// sv and dz are of type T, every product and sum is double.  centred: I is taken here, about the cm handed in.
template <typename T>
__device__ __forceinline__ void mt_group(T (&v)[4], const T (&r)[4], T prev, unsigned need, bool centred, double cm,
                                         Sums& s) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const T lin = mt_linear(v[e]);
    v[e] = lin;
    const double sd = (double)lin, dz = (double)mt_dz(r, prev, e), rd = (double)r[e];
    const double w = sd * dz;
    s.A += mt_skipna(w);
    if (need & kNeedB) s.B += mt_skipna(rd * w);
    if (need & kNeedQ) s.Q += mt_skipna(sd * sd * dz);
    if (centred) {
      const double d = rd - cm;
      s.I += mt_skipna(d * d * w);
    }
  }
}

// One group of the second pass: lin holds the linear values
template <typename T>
__device__ __forceinline__ double mt_group_centred(const T (&lin)[4], const T (&r)[4], T prev, double cm) {
  double I = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double d = (double)r[e] - cm;
    I += mt_skipna(d * d * ((double)lin[e] * (double)mt_dz(r, prev, e)));
  }
  return I;
}

// the sum over the owners of a row, known to all of them.  LANES = kBlock: through slot (a row of red, one per
// quantity, so that consecutive sums need no barrier between them beyond their own)
template <int LANES>
__device__ __forceinline__ double mt_owner_sum(double x, double (*red)[kWaves], int slot) {
  x = epa::wave_sum_all(x);
  if (LANES == kWave) return x;
  if ((threadIdx.x & (kWave - 1)) == 0) red[slot][threadIdx.x / kWave] = x;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t += red[slot][w];
  return t;
}

template <typename T>
__device__ __forceinline__ void mt_store(const MetricsArgs& a, long long row, const Sums& s) {
  if (a.abundance) static_cast<T*>(a.abundance)[row] = (T)(10.0 * ::log10(s.A));
  if (a.center_of_mass) static_cast<T*>(a.center_of_mass)[row] = (T)(s.B / s.A);
  if (a.dispersion) static_cast<T*>(a.dispersion)[row] = (T)(s.I / s.A);
  const double even = s.A * s.A / s.Q;
  if (a.evenness) static_cast<T*>(a.evenness)[row] = (T)even;
  if (a.aggregation) static_cast<T*>(a.aggregation)[row] = (T)(1.0 / even);
}

// Rows of at most LANES * 4 * kGroups samples, held in registers by LANES lanes: a wave (four rows per workgroup) or
// the workgroup.  Owners beyond the grid's take further rows.
template <typename T, bool AL, int LANES>
__global__ __launch_bounds__(kBlock) void metrics_rows_kernel(MetricsArgs a) {
  __shared__ double red[8][kWaves];
  const long long S = a.S;
  const int t = LANES == kWave ? (int)(threadIdx.x & (kWave - 1)) : (int)threadIdx.x;  // the lane among the owners
  const int wave0 = t & ~(kWave - 1);                                                    // first lane of this wave
  const long long owners = LANES == kWave ? (long long)gridDim.x * kWaves : (long long)gridDim.x;
  long long row = LANES == kWave ? (long long)blockIdx.x * kWaves + threadIdx.x / kWave : (long long)blockIdx.x;
  int parity = 0;  // the rows of red alternate from row to row: a fast wave may not overwrite what a slow one still reads
  for (; row < a.R; row += owners, parity ^= 4) {
    const T* sv = static_cast<const T*>(a.sv) + row * S;
    const T* rg = static_cast<const T*>(a.range) + row * a.range_stride;
    const bool centred = a.cm_in && (a.need & kNeedI);
    const double cm_in = centred ? a.cm_in[row] : 0.0;
    T v[kGroups][4], r[kGroups][4], prev[kGroups];
    // (the guards are uniform over a wave: its lanes past the end of the row hold NaN groups)
#pragma unroll
    for (int k = 0; k < kGroups; ++k) {
      if (((long long)k * LANES + wave0) * 4 < S) {
        const long long j0 = ((long long)k * LANES + t) * 4;
        mt_load4<T, AL>(sv, j0, S, v[k]);
        mt_load4<T, AL>(rg, j0, S, r[k]);
      }
    }
    Sums s = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kGroups; ++k) {
      if (((long long)k * LANES + wave0) * 4 < S) {
        prev[k] = mt_prev(rg, ((long long)k * LANES + t) * 4, S, r[k]);
        mt_group(v[k], r[k], prev[k], a.need, centred, cm_in, s);
      }
    }
    s.A = mt_owner_sum<LANES>(s.A, red, parity + 0);
    if (a.need & kNeedB) s.B = mt_owner_sum<LANES>(s.B, red, parity + 1);
    if (a.need & kNeedQ) s.Q = mt_owner_sum<LANES>(s.Q, red, parity + 2);
    const double cm = s.B / s.A;
    if ((a.need & kNeedI) && !centred) {
#pragma unroll
      for (int k = 0; k < kGroups; ++k)
        if (((long long)k * LANES + wave0) * 4 < S) s.I += mt_group_centred(v[k], r[k], prev[k], cm);
    }
    if (a.need & kNeedI) s.I = mt_owner_sum<LANES>(s.I, red, parity + 3);
    if (t == 0) mt_store<T>(a, row, s);
  }
}

// Rows of any length, one workgroup per row: the second pass reads the row again (it has just come through L2) and
// takes the linear values anew.
template <typename T, bool AL>
__global__ __launch_bounds__(kBlock) void metrics_loop_kernel(MetricsArgs a) {
  __shared__ double red[8][kWaves];
  const long long S = a.S;
  int parity = 0;
  for (long long row = blockIdx.x; row < a.R; row += gridDim.x, parity ^= 4) {
    const T* sv = static_cast<const T*>(a.sv) + row * S;
    const T* rg = static_cast<const T*>(a.range) + row * a.range_stride;
    const bool centred = a.cm_in && (a.need & kNeedI);
    const double cm_in = centred ? a.cm_in[row] : 0.0;
    Sums s = {0.0, 0.0, 0.0, 0.0};
    // (whole workgroups of groups: the trip count is the same for every lane, as mt_prev needs)
    for (long long g0 = 0; g0 * 4 < S; g0 += kBlock) {
      const long long j0 = (g0 + threadIdx.x) * 4;
      T v[4], r[4];
      mt_load4<T, AL>(sv, j0, S, v);
      mt_load4<T, AL>(rg, j0, S, r);
      mt_group(v, r, mt_prev(rg, j0, S, r), a.need, centred, cm_in, s);
    }
    s.A = mt_owner_sum<kBlock>(s.A, red, parity + 0);
    if (a.need & kNeedB) s.B = mt_owner_sum<kBlock>(s.B, red, parity + 1);
    if (a.need & kNeedQ) s.Q = mt_owner_sum<kBlock>(s.Q, red, parity + 2);
    const double cm = s.B / s.A;
    if ((a.need & kNeedI) && !centred) {
      for (long long g0 = 0; g0 * 4 < S; g0 += kBlock) {
        const long long j0 = (g0 + threadIdx.x) * 4;
        T v[4], r[4];
        mt_load4<T, AL>(sv, j0, S, v);
        mt_load4<T, AL>(rg, j0, S, r);
        const T prev = mt_prev(rg, j0, S, r);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = mt_linear(v[e]);
        s.I += mt_group_centred(v, r, prev, cm);
      }
    }
    if (a.need & kNeedI) s.I = mt_owner_sum<kBlock>(s.I, red, parity + 3);
    if (threadIdx.x == 0) mt_store<T>(a, row, s);
  }
}

template <typename T>
int launch_metrics(const MetricsArgs& a, hipStream_t st) {
  // aligned: every row of both arrays starts on a multiple of 16 bytes
  const bool rows_al = a.R == 1 || (a.S * sizeof(T)) % 16 == 0;
  const bool al = reinterpret_cast<uintptr_t>(a.sv) % 16 == 0 && reinterpret_cast<uintptr_t>(a.range) % 16 == 0 && rows_al;
  if (a.S <= kWaveRow) {
    const long long need = (a.R + kWaves - 1) / kWaves;
    const int grid = (int)(need < a.max_grid ? need : a.max_grid);
    if (al) {
      hipLaunchKernelGGL((metrics_rows_kernel<T, true, kWave>), dim3(grid), dim3(kBlock), 0, st, a);
      return epa::check_launch("metrics_wave_kernel");
    }
    hipLaunchKernelGGL((metrics_rows_kernel<T, false, kWave>), dim3(grid), dim3(kBlock), 0, st, a);
    return epa::check_launch("metrics_wave_kernel_unaligned");
  }
  const int grid = (int)(a.R < a.max_grid ? a.R : a.max_grid);
  if (a.S <= kBlockRow) {
    if (al) {
      hipLaunchKernelGGL((metrics_rows_kernel<T, true, kBlock>), dim3(grid), dim3(kBlock), 0, st, a);
      return epa::check_launch("metrics_block_kernel");
    }
    hipLaunchKernelGGL((metrics_rows_kernel<T, false, kBlock>), dim3(grid), dim3(kBlock), 0, st, a);
    return epa::check_launch("metrics_block_kernel_unaligned");
  }
  if (al) {
    hipLaunchKernelGGL((metrics_loop_kernel<T, true>), dim3(grid), dim3(kBlock), 0, st, a);
    return epa::check_launch("metrics_loop_kernel");
  }
  hipLaunchKernelGGL((metrics_loop_kernel<T, false>), dim3(grid), dim3(kBlock), 0, st, a);
  return epa::check_launch("metrics_loop_kernel_unaligned");
}

}  // namespace

extern "C" int epa_echo_metrics(const void* sv, const void* range, int range_per_row, long long R, long long S,
                                const double* cm_in, void* abundance, void* center_of_mass, void* dispersion,
                                void* evenness, void* aggregation, int dtype, int max_grid, epa_stream_t stream) {
  EPA_CHECK_REAL("epa_echo_metrics", dtype);
  EPA_CHECK_ARG(R >= 0 && S >= 0, "epa_echo_metrics: bad shape R=%lld S=%lld", R, S);
  EPA_CHECK_ARG(S <= (1LL << 40) && R <= (1LL << 40), "epa_echo_metrics: R=%lld S=%lld is too large", R, S);
  EPA_CHECK_ARG((sv && range) || R * S == 0, "epa_echo_metrics: NULL array argument");
  EPA_CHECK_ARG(abundance || center_of_mass || dispersion || evenness || aggregation,
                "epa_echo_metrics: no statistic asked for");
  EPA_CHECK_ARG(max_grid >= 0 && max_grid <= kMaxGrid, "epa_echo_metrics: max_grid %d is not in 0 .. %d", max_grid,
                kMaxGrid);
  if (R == 0) return EPA_OK;
  MetricsArgs a;
  a.max_grid = max_grid ? max_grid : kMaxGrid;
  a.sv = sv, a.range = range, a.range_stride = range_per_row ? S : 0, a.R = R, a.S = S, a.cm_in = cm_in;
  a.abundance = abundance, a.center_of_mass = center_of_mass, a.dispersion = dispersion, a.evenness = evenness;
  a.aggregation = aggregation;
  a.need = ((center_of_mass || (dispersion && !cm_in)) ? kNeedB : 0u) | ((evenness || aggregation) ? kNeedQ : 0u) |
           (dispersion ? kNeedI : 0u);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return epa::dispatch_real("epa_echo_metrics", dtype, [&](auto tag) {
    return launch_metrics<typename decltype(tag)::type>(a, st);
  });
}
