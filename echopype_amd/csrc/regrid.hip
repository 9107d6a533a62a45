// commongrid.regrid_Sv: every (channel, ping) row of Sv onto one range grid, the echo integral kept.  A source sample i of
// a row stands for the cell [m[i], m[i+1]) between the midpoints of its range and its neighbours' (the two outer cells
// are mirrored); output cell j = [j*bin, (j+1)*bin) receives W_j = sum_i o_ij and N_j = sum_i o_ij * 10^(v_i / 10), o_ij
// the length the two cells share, over the samples whose Sv is not NaN, and Sv_j = 10 log10(N_j / W_j), coverage_j =
// W_j / bin.  Everything is float64; the two outputs are rounded once to the type of Sv.  The rule is restated in NumPy
// in tests/regrid_ref.py.
//
// One workgroup per row.  (1) The lanes sweep the row's range once for n, the length of its leading run of finite
// values, and for the first decrease: a row with n < 2 or a decrease in front of n is written as NaN / 0 and counted.
// (2) The row goes through LDS in tiles of EPA_REGRID_TILE samples: the tile's cell bounds m (one more than samples, so
// the halo of a tile is one range value on either side, read from the array again) and each sample's linear value,
// converted ONCE.  (3) Lanes own output cells: a lane finds the first sample that reaches into its cell by a binary search
// on m and walks the samples up to the cell's far edge, in ascending order.  The cells a tile completes are stored (non-
// temporal: they are not read again here); the one cell its last bound cuts is handed to the next tile through LDS as
// (W, N) and continued there, so the order of the sum is that of the samples whatever the tile length.  Every output
// element is stored exactly once and nothing is pre-filled, the counter of refused rows excepted (a 4-byte memset).
#include "epa_internal.h"

#include <cfloat>

namespace {

using epa::kBlock;

constexpr int kTile = EPA_REGRID_TILE;
constexpr int kRegridMaxGrid = 8192;  // workgroups of a launch: further rows are taken in a loop

struct RegridArgs {
  const void* sv;     // [rows * S], contiguous
  const void* range;  // element (c, p, s) at c*rs_c + p*rs_p + s*rs_s
  long long rs_c, rs_p, rs_s;
  int P, S, J;
  long long rows;
  double bin, inv_bin;
  void* sv_out;   // [rows * J]
  void* cov_out;  // [rows * J] or NULL
  int32_t* n_unordered;
};

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= DBL_MAX; }

// the number of cells that end at or below b: the j with (j + 1) * bin <= b, decided against the edges themselves
__device__ __forceinline__ int cells_below(double b, double bin, double inv_bin, int J) {
  if (!(b > 0.0)) return 0;
  const double t = b * inv_bin;
  if (t >= (double)J + 1.0) return J;
  int k = (int)t;
  if ((double)k * bin > b) --k;
  else if ((double)(k + 1) * bin <= b) ++k;
  return k < 0 ? 0 : (k > J ? J : k);
}

template <typename T>
__device__ __forceinline__ void regrid_store(const RegridArgs& a, size_t at, double sv, double cov) {
  __builtin_nontemporal_store((T)sv, static_cast<T*>(a.sv_out) + at);
  if (a.cov_out) __builtin_nontemporal_store((T)cov, static_cast<T*>(a.cov_out) + at);
}

template <typename T, typename R>
__global__ __launch_bounds__(kBlock) void regrid_rows_kernel(RegridArgs a) {
  __shared__ double s_m[kTile + 1];  // the bounds of the tile's source cells
  __shared__ double s_lin[kTile];    // 10^(Sv / 10) of its samples, NaN where Sv is
  __shared__ double s_carry[2][2];   // (W, N) of the cell a tile's last bound cuts: written by tile k for tile k + 1
  __shared__ int s_first[2];         // the first sample that is not finite, the first that is below its predecessor
  const int tid = (int)threadIdx.x;
  const int S = a.S, J = a.J;
  const double nan = __builtin_nan("");

  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const long long c = row / a.P, p = row - c * a.P;
    const R* rg = static_cast<const R*>(a.range) + c * a.rs_c + p * a.rs_p;
    const T* sv = static_cast<const T*>(a.sv) + (size_t)row * S;
    const size_t out0 = (size_t)row * J;
    const long long ss = a.rs_s;

    // ---- n and the ordering verdict -------------------------------------------------------------------------------------
    if (tid == 0) s_first[0] = s_first[1] = S;
    __syncthreads();
    // (no early exit: the loads of a lane's samples do not wait for one another)
    int bad_at = S, down_at = S;
#pragma unroll 4
    for (int i = tid; i < S; i += kBlock) {
      const double x = (double)rg[i * ss];
      const double y = i > 0 ? (double)rg[(i - 1) * ss] : x;
      const bool fx = finite_d(x);
      if (!fx && i < bad_at) bad_at = i;
      if (fx && finite_d(y) && x < y && i < down_at) down_at = i;
    }
    if (bad_at < S) atomicMin(&s_first[0], bad_at);
    if (down_at < S) atomicMin(&s_first[1], down_at);
    __syncthreads();
    const int n = s_first[0];
    const bool refused = n < 2 || s_first[1] < n;
    if (refused) {
      for (int j = tid; j < J; j += kBlock) regrid_store<T>(a, out0 + j, nan, 0.0);
      if (tid == 0) atomicAdd(a.n_unordered, 1);
      __syncthreads();  // (s_first is set again for the next row)
      continue;
    }

    // ---- the row, a tile of source samples at a time ----------------------------------------------------------------------
    int k = 0;
    for (int t0 = 0; t0 < n; t0 += kTile, ++k) {
      const int t1 = t0 + kTile < n ? t0 + kTile : n, len = t1 - t0;
      for (int i = tid; i <= len; i += kBlock) {
        const int g = t0 + i;
        double m;
        if (g == 0) {
          const double r0 = (double)rg[0], r1 = (double)rg[ss];
          m = r0 - (r1 - r0) / 2;
        } else if (g == n) {
          const double r1 = (double)rg[(long long)(n - 1) * ss], r2 = (double)rg[(long long)(n - 2) * ss];
          m = r1 + (r1 - r2) / 2;
        } else {
          m = ((double)rg[(long long)(g - 1) * ss] + (double)rg[(long long)g * ss]) / 2;
        }
        s_m[i] = m;
        if (i < len) {
          const double v = (double)sv[g];
          s_lin[i] = v == v ? epa::M<double>::exp10(v / 10.0) : nan;
        }
      }
      __syncthreads();
      const bool first = t0 == 0, last = t1 == n;
      // cells [cs, cb) are completed by this tile; cell cb is cut by its last bound and goes on in the next tile
      const int cs = first ? 0 : cells_below(s_m[0], a.bin, a.inv_bin, J);
      const int cb = last ? J : cells_below(s_m[len], a.bin, a.inv_bin, J);
      for (int j = cs + tid; j <= cb && j < J; j += kBlock) {
        const double lo = (double)j * a.bin, hi = (double)(j + 1) * a.bin;
        double W = 0.0, N = 0.0;
        if (!first && j == cs) W = s_carry[k & 1][0], N = s_carry[k & 1][1];
        int i0 = 0, i1 = len;  // the first sample whose cell ends above lo
        while (i0 < i1) {
          const int mid = (i0 + i1) >> 1;
          if (s_m[mid + 1] > lo) i1 = mid;
          else i0 = mid + 1;
        }
        for (int i = i0; i < len && s_m[i] < hi; ++i) {
          const double o = fmin(s_m[i + 1], hi) - fmax(s_m[i], lo);
          const double l = s_lin[i];
          if (o > 0.0 && l == l) {
            W += o;
            N += o * l;
          }
        }
        if (j < cb) {
          regrid_store<T>(a, out0 + j, W > 0.0 ? 10.0 * epa::M<double>::log10(N / W) : nan, W / (hi - lo));
        } else {
          s_carry[(k + 1) & 1][0] = W, s_carry[(k + 1) & 1][1] = N;
        }
      }
      __syncthreads();  // (the next tile, or the next row, overwrites s_m / s_lin / s_first)
    }
  }
}

}  // namespace

extern "C" int epa_regrid_rows(const void* sv, int dtype, const void* range, int range_dtype, long long range_stride_c,
                               long long range_stride_p, long long range_stride_s, int C, int P, int S, double range_bin,
                               int n_rbins, void* sv_out, void* coverage_out, int32_t* n_unordered_out, int max_grid,
                               epa_stream_t stream) {
  EPA_CHECK_REAL("epa_regrid_rows", dtype);
  EPA_CHECK_ARG(epa::is_real(range_dtype), "epa_regrid_rows: bad range dtype %d", range_dtype);
  EPA_CHECK_ARG(C >= 0 && P >= 0 && S >= 0 && S <= (1 << 30), "epa_regrid_rows: bad shape C=%d P=%d S=%d", C, P, S);
  EPA_CHECK_ARG(n_rbins >= 0 && n_rbins <= (1 << 30), "epa_regrid_rows: bad grid n_rbins=%d", n_rbins);
  EPA_CHECK_ARG(range_bin > 0.0 && range_bin < INFINITY, "epa_regrid_rows: range_bin must be positive and finite");
  EPA_CHECK_ARG(range_stride_c >= 0 && range_stride_p >= 0 && range_stride_s >= 0,
                "epa_regrid_rows: strides must not be negative");
  EPA_CHECK_ARG(max_grid >= 0, "epa_regrid_rows: max_grid must not be negative");
  EPA_CHECK_ARG(n_unordered_out != nullptr, "epa_regrid_rows: n_unordered_out is NULL");
  const long long rows = (long long)C * P;
  EPA_CHECK_ARG((sv && range) || rows * S == 0, "epa_regrid_rows: NULL array argument");
  EPA_CHECK_ARG(sv_out || rows * n_rbins == 0, "epa_regrid_rows: sv_out is NULL");
  hipStream_t st = (hipStream_t)stream;
  EPA_CHECK_HIP(hipMemsetAsync(n_unordered_out, 0, sizeof(int32_t), st));
  if (rows == 0) return EPA_OK;

  RegridArgs a;
  a.sv = sv, a.range = range, a.rs_c = range_stride_c, a.rs_p = range_stride_p, a.rs_s = range_stride_s;
  a.P = P, a.S = S, a.J = n_rbins, a.rows = rows, a.bin = range_bin, a.inv_bin = 1.0 / range_bin;
  a.sv_out = sv_out, a.cov_out = coverage_out, a.n_unordered = n_unordered_out;
  const long long cap = max_grid > 0 ? max_grid : kRegridMaxGrid;
  const unsigned grid = (unsigned)(rows < cap ? rows : cap);
  return epa::dispatch_real("epa_regrid_rows", dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return epa::dispatch_real("epa_regrid_rows", range_dtype, [&](auto rtag) {
      using R = typename decltype(rtag)::type;
      hipLaunchKernelGGL((regrid_rows_kernel<T, R>), dim3(grid), dim3(kBlock), 0, st, a);
      return epa::check_launch("regrid_rows_kernel");
    });
  });
}
