// mask.line_mask: the samples between two depth lines.  out[c, p, s] = ub[c, p] <= r[c, p, s] < lb[c, p] (or
// ub < r <= lb), r the range of the sample read from an array or evaluated from the coefficient rows a lazy echo_range /
// depth is a function of.  One pass, 1 byte written per sample; every comparison is made in float64 on the value the
// range array holds (or would hold) in its own type, so the result is exact.
#include "epa_internal.h"

namespace {

using epa::kBlock;

constexpr int kGroup = 16;  // mask bytes per lane: one 16-byte store

struct LineMaskArgs {
  const void* range;  // SRC 0 / 1: the range array, element strides rs_*
  long long rs_c, rs_p, rs_s;
  const epa::CoefRow* coef;  // SRC 2: coefficient rows [C*P], NaN where nan_raw [C*P*S] is (if given), depth = offset +
  const float* nan_raw;      //        scale * range when scale / offset [C*P] are given
  const double* scale;
  const double* offset;
  const double* upper;  // NULL: not tested
  long long us_c, us_p;
  double upper_offset;
  const double* lower;
  long long ls_c, ls_p;
  double lower_offset;
  int closed_right, nan_ignore;
  int P, S;
  long long rows;
  uint8_t* out;
  int lpr_log2;  // lanes per row = 1 << lpr_log2: the lanes of a workgroup form (kBlock >> lpr_log2) rows of lanes
  int chunks;    // runs of (lanes per row) groups that cover a row
  long long pieces;
};

// the bounds of one (channel, ping), made once per row
struct RowBounds {
  double ub, lb;
  bool test_u, test_l, dead;  // dead: a NaN bound under nan_line = exclude, every sample of the row is 0
};

__device__ __forceinline__ RowBounds line_bounds(const LineMaskArgs& a, long long c, long long p) {
  RowBounds b;
  b.ub = b.lb = 0.0;
  b.test_u = a.upper != nullptr, b.test_l = a.lower != nullptr, b.dead = false;
  if (b.test_u) {
    b.ub = a.upper[c * a.us_c + p * a.us_p] + a.upper_offset;
    if (!(b.ub == b.ub)) {
      if (a.nan_ignore) b.test_u = false; else b.dead = true;
    }
  }
  if (b.test_l) {
    b.lb = a.lower[c * a.ls_c + p * a.ls_p] + a.lower_offset;
    if (!(b.lb == b.lb)) {
      if (a.nan_ignore) b.test_l = false; else b.dead = true;
    }
  }
  return b;
}

__device__ __forceinline__ uint32_t line_test(double r, const RowBounds& b, bool right) {
  bool ok = (r == r) && !b.dead;
  if (b.test_u) ok = ok && (right ? b.ub < r : b.ub <= r);
  if (b.test_l) ok = ok && (right ? r <= b.lb : r < b.lb);
  return ok ? 1u : 0u;
}

// four consecutive elements from an address that is a multiple of the element size only: one 16-byte load of float32,
// two of float64 (global memory is accessed in unaligned mode; mask_grid.hip's fd_load4)
template <typename T>
__device__ __forceinline__ void lm_load4(const T* p, T* v) {
  __builtin_memcpy(v, __builtin_assume_aligned(p, sizeof(T)), 4 * sizeof(T));
}

// The range of samples s0 + j, j in [lo, hi), of row (c, p) as float64 (other j: NaN, never stored).
//   SRC 0: the array, sample stride 1;  SRC 1: the array, any sample stride;
//   SRC 2: evaluated in T from the coefficient rows exactly as epa_range_power / epa_depth_rows write it.
template <typename T, int SRC>
__device__ __forceinline__ void lm_values(const LineMaskArgs& a, long long row, long long c, long long p, int s0, int lo,
                                          int hi, double (&r)[kGroup]) {
  const bool whole = lo == 0 && hi == kGroup;
  if (SRC == 2) {
    const epa::CoefRow cr = a.coef[row];
    float raw[kGroup];
    if (a.nan_raw) {
      const float* rp = a.nan_raw + (size_t)row * a.S + s0;
      if (whole) {
#pragma unroll
        for (int k = 0; k < kGroup; k += 4) lm_load4<float>(rp + k, raw + k);
      } else {
#pragma unroll
        for (int j = 0; j < kGroup; ++j) raw[j] = (j >= lo && j < hi) ? rp[j] : 0.0f;
      }
    }
    T sc = (T)1, of = (T)0;
    if (a.scale) {
      sc = (T)a.scale[row];
      of = (T)a.offset[row];
    }
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
      T v = (T)epa::row_range(cr, s0 + j);
      if (a.nan_raw && !(raw[j] == raw[j])) v = epa::M<T>::nan();
      if (a.scale) v = epa::depth_of(sc, of, v);
      r[j] = (j >= lo && j < hi) ? (double)v : __builtin_nan("");
    }
  } else {
    const T* base = static_cast<const T*>(a.range) + c * a.rs_c + p * a.rs_p;
    T v[kGroup];
    if (SRC == 0 && whole) {
#pragma unroll
      for (int k = 0; k < kGroup; k += 4) lm_load4<T>(base + s0 + k, v + k);
    } else {
      const long long ss = SRC == 0 ? 1 : a.rs_s;
#pragma unroll
      for (int j = 0; j < kGroup; ++j) v[j] = (j >= lo && j < hi) ? base[(long long)(s0 + j) * ss] : (T)0;
    }
#pragma unroll
    for (int j = 0; j < kGroup; ++j) r[j] = (j >= lo && j < hi) ? (double)v[j] : __builtin_nan("");
  }
}

// bytes [lo, hi) of the 16-byte aligned group at g16 as the widest naturally aligned stores that stay inside them
__device__ __forceinline__ void lm_store_part(uint8_t* g16, uint64_t q0, uint64_t q1, int lo, int hi) {
  int pos = lo;
  while (pos < hi) {
    int w = 8;
    while ((pos & (w - 1)) != 0 || pos + w > hi) w >>= 1;
    const uint64_t q = (pos < 8 ? q0 : q1) >> (8 * (pos & 7));
    if (w == 8) *reinterpret_cast<uint64_t*>(g16 + pos) = q;
    else if (w == 4) *reinterpret_cast<uint32_t*>(g16 + pos) = (uint32_t)q;
    else if (w == 2) *reinterpret_cast<uint16_t*>(g16 + pos) = (uint16_t)q;
    else g16[pos] = (uint8_t)q;
    pos += w;
  }
}

// A lane decides the 16 bytes of one 16-byte aligned group of the OUTPUT and stores them at once; the groups are laid
// over each row from the aligned address at or below its first byte, so the group that holds a row's first byte and the
// one that holds its last are written in part (narrower stores, nothing outside the row).  A piece = (kBlock >> lpr_log2)
// consecutive rows x (1 << lpr_log2) consecutive groups; a workgroup normally takes one piece and ends.
template <typename T, int SRC>
__global__ __launch_bounds__(kBlock) void line_mask_kernel(LineMaskArgs a) {
  const int lpr = 1 << a.lpr_log2, rpb = kBlock >> a.lpr_log2;
  const int lane = (int)threadIdx.x & (lpr - 1), ro = (int)threadIdx.x >> a.lpr_log2;
  const bool right = a.closed_right != 0;
  for (long long piece = blockIdx.x; piece < a.pieces; piece += gridDim.x) {
    const long long rblock = piece / a.chunks;
    const int chunk = (int)(piece - rblock * a.chunks);
    const long long row = rblock * rpb + ro;
    if (row >= a.rows) continue;
    uint8_t* orow = a.out + (size_t)row * a.S;
    const int mis = (int)(reinterpret_cast<uintptr_t>(orow) & (kGroup - 1));
    const long long first = ((long long)chunk * lpr + lane) * kGroup - mis;  // the sample of the group's byte 0
    if (first >= a.S) continue;
    const int s0 = (int)first;
    const int lo = s0 < 0 ? -s0 : 0;
    const int hi = a.S - s0 < kGroup ? a.S - s0 : kGroup;
    const long long c = row / a.P, p = row - c * a.P;
    const RowBounds b = line_bounds(a, c, p);
    double r[kGroup];
    lm_values<T, SRC>(a, row, c, p, s0, lo, hi, r);
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      w[k] = line_test(r[4 * k], b, right) | (line_test(r[4 * k + 1], b, right) << 8) |
             (line_test(r[4 * k + 2], b, right) << 16) | (line_test(r[4 * k + 3], b, right) << 24);
    uint8_t* g16 = orow + s0;  // (a multiple of 16 by construction; below the row when lo > 0, nothing is stored there)
    if (lo == 0 && hi == kGroup) {
      *reinterpret_cast<uint4*>(g16) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      lm_store_part(g16, (uint64_t)w[0] | ((uint64_t)w[1] << 32), (uint64_t)w[2] | ((uint64_t)w[3] << 32), lo, hi);
    }
  }
}

constexpr long long kLineMaskMaxGrid = 1ll << 22;  // workgroups of a launch: further pieces are taken in a loop

}  // namespace

extern "C" int epa_line_mask(const void* range, long long range_stride_c, long long range_stride_p,
                             long long range_stride_s, const double* coef, const float* nan_raw, const double* scale,
                             const double* offset, int dtype, const double* upper, long long upper_stride_c,
                             long long upper_stride_p, double upper_offset, const double* lower, long long lower_stride_c,
                             long long lower_stride_p, double lower_offset, unsigned flags, int C, int P, int S,
                             uint8_t* out, epa_stream_t stream) {
  EPA_CHECK_ARG(out != nullptr, "epa_line_mask: out is NULL");
  EPA_CHECK_ARG(upper || lower, "epa_line_mask: both lines are NULL");
  EPA_CHECK_REAL("epa_line_mask", dtype);
  EPA_CHECK_ARG((range != nullptr) != (coef != nullptr),
                "epa_line_mask: the range comes as an array or as coefficient rows, one of the two");
  EPA_CHECK_ARG(coef || !(nan_raw || scale || offset),
                "epa_line_mask: nan_raw, scale and offset go with the coefficient rows");
  EPA_CHECK_ARG((scale != nullptr) == (offset != nullptr), "epa_line_mask: scale and offset come together");
  EPA_CHECK_ARG((flags & ~(EPA_LINE_CLOSED_RIGHT | EPA_LINE_NAN_IGNORE)) == 0,
                "epa_line_mask: flags takes EPA_LINE_CLOSED_RIGHT and EPA_LINE_NAN_IGNORE only");
  EPA_CHECK_ARG(C >= 0 && P >= 0 && S >= 0 && S <= (1 << 30), "epa_line_mask: bad shape C=%d P=%d S=%d", C, P, S);
  EPA_CHECK_ARG(range_stride_c >= 0 && range_stride_p >= 0 && range_stride_s >= 0 && upper_stride_c >= 0 &&
                    upper_stride_p >= 0 && lower_stride_c >= 0 && lower_stride_p >= 0,
                "epa_line_mask: strides must not be negative");
  EPA_CHECK_ARG(upper_offset == upper_offset && lower_offset == lower_offset, "epa_line_mask: an offset is NaN");
  if ((size_t)C * P * S == 0) return EPA_OK;

  LineMaskArgs a;
  a.range = range, a.rs_c = range_stride_c, a.rs_p = range_stride_p, a.rs_s = range_stride_s;
  a.coef = reinterpret_cast<const epa::CoefRow*>(coef), a.nan_raw = nan_raw, a.scale = scale, a.offset = offset;
  a.upper = upper, a.us_c = upper_stride_c, a.us_p = upper_stride_p, a.upper_offset = upper_offset;
  a.lower = lower, a.ls_c = lower_stride_c, a.ls_p = lower_stride_p, a.lower_offset = lower_offset;
  a.closed_right = (flags & EPA_LINE_CLOSED_RIGHT) ? 1 : 0, a.nan_ignore = (flags & EPA_LINE_NAN_IGNORE) ? 1 : 0;
  a.P = P, a.S = S, a.rows = (long long)C * P, a.out = out;
  // a row whose first byte is the last of its group spreads over this many groups
  const long long groups = ((long long)S + 2 * kGroup - 2) / kGroup;
  a.lpr_log2 = 0;
  while ((1ll << a.lpr_log2) < groups && a.lpr_log2 < 8) ++a.lpr_log2;
  const int rpb = kBlock >> a.lpr_log2;
  a.chunks = (int)((groups + (1 << a.lpr_log2) - 1) >> a.lpr_log2);
  a.pieces = ((a.rows + rpb - 1) / rpb) * a.chunks;
  const unsigned grid = (unsigned)(a.pieces < kLineMaskMaxGrid ? a.pieces : kLineMaskMaxGrid);
  hipStream_t st = (hipStream_t)stream;
  return epa::dispatch_real("epa_line_mask", dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (coef) {
      hipLaunchKernelGGL((line_mask_kernel<T, 2>), dim3(grid), dim3(kBlock), 0, st, a);
      return epa::check_launch("line_mask_kernel_rows");
    }
    if (range_stride_s == 1) {
      hipLaunchKernelGGL((line_mask_kernel<T, 0>), dim3(grid), dim3(kBlock), 0, st, a);
      return epa::check_launch("line_mask_kernel");
    }
    hipLaunchKernelGGL((line_mask_kernel<T, 1>), dim3(grid), dim3(kBlock), 0, st, a);
    return epa::check_launch("line_mask_kernel_strided");
  });
}
