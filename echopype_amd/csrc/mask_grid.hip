// mask.frequency_differencing and mask.regrid_mask (reference: echopype mask/api.py:467-675, :678-863): a mask from the
// difference of two Sv planes, and a mask brought onto the (ping-time bin, range bin) grid of compute_MVBS.  Both make
// one pass over a large array; their results are bytes, so they are exact.
#include "epa_internal.h"

namespace {

using epa::kBlock;

// ---- epa_freq_diff_mask ------------------------------------------------------------------------------------------------
// cmp as three wanted outcomes of comparing d = a - b with the threshold: d > thr, d < thr, d == thr.  A NaN d (NaN on
// either side, inf - inf) has none of the three, so every operator gives 0 for it.
constexpr unsigned kWantGT = 1u, kWantLT = 2u, kWantEQ = 4u;

template <typename T>
__device__ __forceinline__ unsigned fd_test(T a, T b, T thr, unsigned want) {
  const T d = a - b;  // rounded in T: NumPy's subtraction of two arrays of that type
  return ((d > thr) ? (want & 1u) : 0u) | ((d < thr) ? ((want >> 1) & 1u) : 0u) | ((d == thr) ? ((want >> 2) & 1u) : 0u);
}

// four consecutive elements: one 16-byte load of float32, two of float64.  AL: the address is a multiple of 16;
// otherwise it is a multiple of the element size only (plane b starts n elements after plane a) and the load is
// issued with that alignment.
template <typename T, bool AL>
__device__ __forceinline__ void fd_load4(const T* p, T (&v)[4]) {
  if (AL) {
    __builtin_memcpy(v, __builtin_assume_aligned(p, 16), 4 * sizeof(T));
  } else {
    __builtin_memcpy(v, __builtin_assume_aligned(p, sizeof(T)), 4 * sizeof(T));
  }
}

constexpr int kFdUnroll = 4;  // groups of 4 elements per lane and tile: the loads of a tile are issued before its compares

// groups: number of whole 4-element groups served by vector loads and one packed 32-bit mask store each (0 when the
// mask is not 4-byte aligned); the elements from 4*groups on are done one by one.
template <typename T, bool AL>
__global__ __launch_bounds__(kBlock) void freq_diff_kernel(const T* __restrict__ a, const T* __restrict__ b, size_t groups,
                                                          size_t n, T thr, unsigned want, uint8_t* __restrict__ out) {
  constexpr size_t kTile = (size_t)kBlock * kFdUnroll;
  for (size_t tile = blockIdx.x; tile * kTile < groups; tile += gridDim.x) {
    T va[kFdUnroll][4], vb[kFdUnroll][4];
#pragma unroll
    for (int k = 0; k < kFdUnroll; ++k) {
      const size_t g = tile * kTile + (size_t)k * kBlock + threadIdx.x;
      if (g < groups) {
        fd_load4<T, AL>(a + 4 * g, va[k]);
        fd_load4<T, AL>(b + 4 * g, vb[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < kFdUnroll; ++k) {
      const size_t g = tile * kTile + (size_t)k * kBlock + threadIdx.x;
      if (g < groups) {
        const uint32_t m = fd_test(va[k][0], vb[k][0], thr, want) | (fd_test(va[k][1], vb[k][1], thr, want) << 8) |
                           (fd_test(va[k][2], vb[k][2], thr, want) << 16) | (fd_test(va[k][3], vb[k][3], thr, want) << 24);
        *reinterpret_cast<uint32_t*>(out + 4 * g) = m;
      }
    }
  }
  for (size_t i = 4 * groups + (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
    out[i] = (uint8_t)fd_test(a[i], b[i], thr, want);
}

template <typename T>
int launch_freq_diff(const void* sv, size_t n, int chan_a, int chan_b, unsigned want, double diff, uint8_t* out,
                     hipStream_t st) {
  const T* a = static_cast<const T*>(sv) + (size_t)chan_a * n;
  const T* b = static_cast<const T*>(sv) + (size_t)chan_b * n;
  const size_t groups = (reinterpret_cast<uintptr_t>(out) % 4 == 0) ? n / 4 : 0;
  const size_t rest = n - 4 * groups;
  const size_t tiles = (groups + (size_t)kBlock * kFdUnroll - 1) / ((size_t)kBlock * kFdUnroll);
  size_t blocks = tiles > (rest + kBlock - 1) / kBlock ? tiles : (rest + kBlock - 1) / kBlock;
  if (blocks < 1) blocks = 1;
  const int grid = (int)(blocks < 65536 ? blocks : 65536);
  const bool al = reinterpret_cast<uintptr_t>(a) % 16 == 0 && reinterpret_cast<uintptr_t>(b) % 16 == 0;
  const T thr = (T)diff;  // the Python scalar in the array's type
  if (al) {
    hipLaunchKernelGGL((freq_diff_kernel<T, true>), dim3(grid), dim3(kBlock), 0, st, a, b, groups, n, thr, want, out);
    return epa::check_launch("freq_diff_kernel");
  }
  hipLaunchKernelGGL((freq_diff_kernel<T, false>), dim3(grid), dim3(kBlock), 0, st, a, b, groups, n, thr, want, out);
  return epa::check_launch("freq_diff_kernel_unaligned");
}

// ---- epa_regrid_mask ---------------------------------------------------------------------------------------------------
// The byte of an output cell while the sweep runs: kSeen = a sample fell into the cell, kDec = one of them decides the
// cell (a zero for AND, a one for OR).  Bits are only ever set, by atomic OR, so the cell does not depend on who comes
// first; regrid_final_kernel turns the flags into the 0 / 1 of the result.
constexpr uint32_t kSeen = 2u, kDec = 4u;
constexpr int kCols = 16;  // mask bytes of a row per lane: one 16-byte load

struct RegridArgs {
  const uint8_t* mask;
  const int32_t* group;
  int T, P, D;
  const double* range;
  const int32_t* bin_start;
  int n_tbins;
  double range_bin, inv_bin;
  int n_rbins;
  int closed_right;
  int func;
  uint8_t* out;
  int32_t* nonbinary;
  int lpr_log2;  // lanes per row = 1 << lpr_log2: the lanes of a workgroup form (kBlock >> lpr_log2) rows of lanes
  int chunk;     // pings per workgroup
};

// the output slice of input slice t; -1: a value outside 0 .. T-1, which no well-formed group table holds
__device__ __forceinline__ int regrid_slice(const RegridArgs& a, int t) {
  if (!a.group) return t;
  const int g = a.group[t];
  return (g >= 0 && g < a.T) ? g : -1;
}

// the output slice of input slice t if t is the first input slice that maps to it (the one that clears and finalises
// it), else -1
__device__ __forceinline__ int regrid_owned_slice(const RegridArgs& a, int t) {
  const int g = regrid_slice(a, t);
  if (a.group)
    for (int u = 0; u < t; ++u)
      if (a.group[u] == g) return -1;
  return g;
}

__global__ __launch_bounds__(kBlock) void regrid_clear_kernel(RegridArgs a) {
  const int g = regrid_owned_slice(a, blockIdx.y);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.nonbinary = 0;
  if (g < 0) return;
  const size_t cells = (size_t)a.n_tbins * a.n_rbins;
  uint8_t* o = a.out + (size_t)g * cells;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < cells; i += (size_t)gridDim.x * kBlock) o[i] = 0;
}

__global__ __launch_bounds__(kBlock) void regrid_final_kernel(RegridArgs a) {
  const int g = regrid_owned_slice(a, blockIdx.y);
  if (g < 0) return;
  const size_t cells = (size_t)a.n_tbins * a.n_rbins;
  uint8_t* o = a.out + (size_t)g * cells;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < cells; i += (size_t)gridDim.x * kBlock) {
    const uint32_t f = o[i];
    // AND: the mean of the cell's samples is 1.0; OR: it is not 0.0; an empty cell fails both (fill_value = 0.0)
    o[i] = a.func == 0 ? (uint8_t)((f & kSeen) && !(f & kDec)) : (uint8_t)((f & kDec) != 0);
  }
}

// flags into the byte of a cell, through the 32-bit word that holds it
__device__ __forceinline__ void regrid_or_global(uint8_t* out, size_t cell, uint32_t f) {
  uint32_t* w = reinterpret_cast<uint32_t*>(out) + (cell >> 2);
  atomicOr(w, f << (8u * (unsigned)(cell & 3)));
}

// the lane's 16 mask bytes of one row as four words.  AL: rows start on multiples of 16 bytes and D % 16 == 0, so the
// group is whole and aligned.  Otherwise a whole group is still one 16-byte load, issued with byte alignment (global
// memory is accessed in unaligned mode under the HSA ABI), and the group that crosses the end of the row is read byte by
// byte, with zeros past the end
template <bool AL>
__device__ __forceinline__ void regrid_load16(const uint8_t* row, int col0, int D, uint32_t (&v)[4]) {
  if (AL) {
    const uint4 q = *reinterpret_cast<const uint4*>(row + col0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else if (col0 + kCols <= D) {
    __builtin_memcpy(v, row + col0, kCols);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t w = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = col0 + 4 * k + j;
        if (col < D) w |= (uint32_t)row[col] << (8 * j);
      }
      v[k] = w;
    }
  }
}

// One workgroup per (chunk of pings, tile of 4096 columns, input slice).  The pings of a chunk are consecutive, so the
// time bins they fall into are consecutive too (bin_start is a CSR over the sorted pings): the workgroup walks those
// bins, and a time bin with many pings is shared by all the chunks that cut it.
//   PER_PING = false: a lane's columns keep their range bins from row to row; it ORs and ANDs the rows of a time bin in
//     registers and hands over its flags once per time bin.
//   PER_PING = true: every sample has a range of its own, its bin is taken per sample.
//   USE_LDS: the flags of the current time bin are gathered in LDS and merged into the output once per time bin;
//     otherwise (a range grid that does not fit) they go to the output directly.
template <bool AL, bool PER_PING, bool USE_LDS>
__global__ __launch_bounds__(kBlock) void regrid_sweep_kernel(RegridArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lflags[];
  const int t = blockIdx.z;
  const int g = regrid_slice(a, t);
  if (g < 0) return;
  const int D = a.D;
  const int lpr = 1 << a.lpr_log2, rpi = kBlock >> a.lpr_log2;
  const int col0 = ((int)blockIdx.y * kBlock + (int)(threadIdx.x & (lpr - 1))) * kCols;
  const int ro = threadIdx.x >> a.lpr_log2;
  const bool lane_on = col0 < D;
  const int p0 = blockIdx.x * a.chunk;
  const int p1 = a.P - p0 > a.chunk ? p0 + a.chunk : a.P;
  const bool closed_right = a.closed_right != 0;

  int cb[kCols];  // (1-D range) the range bin of each of the lane's columns, -1: none
  if (!PER_PING) {
#pragma unroll
    for (int j = 0; j < kCols; ++j) {
      const int col = col0 + j;
      cb[j] = col < D ? epa::range_bin_index(a.range[col], a.range_bin, a.inv_bin, a.n_rbins, closed_right) : -1;
    }
  }
  if (USE_LDS) {
    for (int i = threadIdx.x; i < a.n_rbins; i += kBlock) lflags[i] = 0;
    __syncthreads();
  }

  // the first time bin that ends after p0
  int lo = 0, hi = a.n_tbins;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.bin_start[mid + 1] > p0) hi = mid; else lo = mid + 1;
  }
  uint32_t nonbin = 0;
  const uint8_t* slice = a.mask + (size_t)t * a.P * D;
  for (int tb = lo; tb < a.n_tbins; ++tb) {
    const int b0 = a.bin_start[tb], b1 = a.bin_start[tb + 1];
    const int s0 = b0 > p0 ? b0 : p0, s1 = b1 < p1 ? b1 : p1;
    if (s0 >= p1) break;
    if (s1 <= s0) continue;  // an empty time bin
    const size_t cell0 = ((size_t)g * a.n_tbins + tb) * a.n_rbins;
    auto emit = [&](int bin, uint32_t f) {
      if (USE_LDS) atomicOr(&lflags[bin], f); else regrid_or_global(a.out, cell0 + bin, f);
    };
    if (lane_on) {
      if (!PER_PING) {
        uint32_t o[4] = {0u, 0u, 0u, 0u}, n[4] = {~0u, ~0u, ~0u, ~0u};
        bool any = false;
#pragma unroll 4
        for (int p = s0 + ro; p < s1; p += rpi) {
          uint32_t v[4];
          regrid_load16<AL>(slice + (size_t)p * D, col0, D, v);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            o[k] |= v[k];
            n[k] &= v[k];
            nonbin |= v[k] & 0xFEFEFEFEu;
          }
          any = true;
        }
        if (any) {
          int cur = -1;
          uint32_t f = 0;
#pragma unroll
          for (int j = 0; j < kCols; ++j) {
            const int bin = cb[j];
            if (bin != cur) {
              if (cur >= 0) emit(cur, f);
              cur = bin, f = 0;
            }
            const uint32_t one = (o[j >> 2] >> (8 * (j & 3))) & 1u, all = (n[j >> 2] >> (8 * (j & 3))) & 1u;
            f |= kSeen | ((a.func == 0 ? !all : one) ? kDec : 0u);
          }
          if (cur >= 0) emit(cur, f);
        }
      } else {
        for (int p = s0 + ro; p < s1; p += rpi) {
          uint32_t v[4];
          regrid_load16<AL>(slice + (size_t)p * D, col0, D, v);
          const double* rr = a.range + (size_t)p * D;
          int cur = -1;
          uint32_t f = 0;
#pragma unroll
          for (int j = 0; j < kCols; ++j) {
            const int col = col0 + j;
            const int bin = col < D ? epa::range_bin_index(rr[col], a.range_bin, a.inv_bin, a.n_rbins, closed_right) : -1;
            if (bin != cur) {
              if (cur >= 0) emit(cur, f);
              cur = bin, f = 0;
            }
            const uint32_t one = (v[j >> 2] >> (8 * (j & 3))) & 1u;
            f |= kSeen | ((a.func == 0 ? !one : one) ? kDec : 0u);
          }
          if (cur >= 0) emit(cur, f);
#pragma unroll
          for (int k = 0; k < 4; ++k) nonbin |= v[k] & 0xFEFEFEFEu;
        }
      }
    }
    if (USE_LDS) {
      __syncthreads();
      for (int i = threadIdx.x; i < a.n_rbins; i += kBlock) {
        const uint32_t f = lflags[i];
        if (f) {
          regrid_or_global(a.out, cell0 + i, f);
          lflags[i] = 0;
        }
      }
      __syncthreads();
    }
  }
  if (nonbin) atomicOr(reinterpret_cast<unsigned int*>(a.nonbinary), 1u);
}

constexpr size_t kRegridLdsMax = 128 * 1024;  // the flags of one time bin, 4 bytes per range bin (block_reduce.hip::make_plan)
inline bool regrid_flags_in_lds(int n_rbins) { return (size_t)n_rbins * 4 <= kRegridLdsMax; }

template <bool AL, bool PER_PING, bool USE_LDS>
int launch_regrid_sweep(const RegridArgs& a, dim3 grid, hipStream_t st) {
  auto kern = regrid_sweep_kernel<AL, PER_PING, USE_LDS>;
  const size_t lds = USE_LDS ? (((size_t)a.n_rbins * 4 + 15) & ~(size_t)15) : 0;
  if (int rc = epa::allow_lds(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, st, a);
  return EPA_OK;
}

// al: 16-byte aligned rows of whole 16-byte groups
template <bool PER_PING, bool USE_LDS>
int launch_regrid_sweep(const RegridArgs& a, bool al, dim3 grid, hipStream_t st) {
  return al ? launch_regrid_sweep<true, PER_PING, USE_LDS>(a, grid, st)
            : launch_regrid_sweep<false, PER_PING, USE_LDS>(a, grid, st);
}

}  // namespace

extern "C" int epa_freq_diff_mask(const void* sv, int C, size_t n, int chan_a, int chan_b, int cmp, double diff,
                                  uint8_t* mask_out, int dtype, epa_stream_t stream) {
  EPA_CHECK_ARG(sv && mask_out, "epa_freq_diff_mask: NULL array argument");
  EPA_CHECK_ARG(C > 0 && chan_a >= 0 && chan_a < C && chan_b >= 0 && chan_b < C,
                "epa_freq_diff_mask: channels %d and %d are not both in 0 .. %d", chan_a, chan_b, C - 1);
  EPA_CHECK_ARG(cmp >= EPA_CMP_GT && cmp <= EPA_CMP_EQ, "epa_freq_diff_mask: bad comparison %d", cmp);
  EPA_CHECK_REAL("epa_freq_diff_mask", dtype);
  if (n == 0) return EPA_OK;
  static const unsigned kWant[5] = {kWantGT, kWantLT, kWantLT | kWantEQ, kWantGT | kWantEQ, kWantEQ};
  hipStream_t st = (hipStream_t)stream;
  return epa::dispatch_real("epa_freq_diff_mask", dtype, [&](auto tag) {
    return launch_freq_diff<typename decltype(tag)::type>(sv, n, chan_a, chan_b, kWant[cmp], diff, mask_out, st);
  });
}

// the output cells as whole 32-bit words: regrid_or_global sets a cell's flags through the word that holds it
size_t epa::scratch::regrid_mask_out(long long G, long long n_tbins, long long n_rbins) {
  return ((size_t)G * (size_t)n_tbins * (size_t)n_rbins + 3) / 4 * 4;
}
// the flags of one time bin (4 bytes per range bin) do not fit in LDS: the sweep sets them in the output itself
extern "C" int epa_regrid_needs_global_flags(int n_rbins, int* yes) {
  EPA_CHECK_ARG(yes != nullptr, "epa_regrid_needs_global_flags: yes is NULL");
  *yes = regrid_flags_in_lds(n_rbins) ? 0 : 1;
  return EPA_OK;
}

extern "C" int epa_regrid_mask(const uint8_t* mask, const int32_t* group, int T, int P, int D, const double* range,
                               int range_per_ping, const int32_t* bin_start, int n_tbins, double range_bin, int n_rbins,
                               unsigned bin_flags, int func, uint8_t* out, int32_t* nonbinary_out, epa_stream_t stream) {
  EPA_CHECK_ARG(out && nonbinary_out && bin_start, "epa_regrid_mask: NULL array argument");
  EPA_CHECK_ARG(T >= 1 && T <= 65535 && P >= 0 && D >= 0, "epa_regrid_mask: bad shape T=%d P=%d D=%d", T, P, D);
  EPA_CHECK_ARG((mask && range) || (size_t)P * D == 0, "epa_regrid_mask: NULL array argument");
  EPA_CHECK_ARG(n_tbins >= 0 && n_rbins >= 0, "epa_regrid_mask: bad grid %d x %d", n_tbins, n_rbins);
  EPA_CHECK_ARG(range_bin > 0.0 && range_bin < INFINITY, "epa_regrid_mask: range_bin must be positive and finite");
  EPA_CHECK_ARG(func == 0 || func == 1, "epa_regrid_mask: func must be 0 (AND) or 1 (OR), got %d", func);
  EPA_CHECK_ARG((bin_flags & ~EPA_BIN_CLOSED_RIGHT) == 0, "epa_regrid_mask: bin_flags takes EPA_BIN_CLOSED_RIGHT only");
  EPA_CHECK_ARG(reinterpret_cast<uintptr_t>(out) % 4 == 0, "epa_regrid_mask: out must be 4-byte aligned");
  const int groups16 = (D + kCols - 1) / kCols;
  EPA_CHECK_ARG((groups16 + kBlock - 1) / kBlock <= 65535, "epa_regrid_mask: D=%d is too large", D);
  hipStream_t st = (hipStream_t)stream;

  RegridArgs a;
  a.mask = mask, a.group = group, a.T = T, a.P = P, a.D = D, a.range = range, a.bin_start = bin_start;
  a.n_tbins = n_tbins, a.range_bin = range_bin, a.inv_bin = 1.0 / range_bin, a.n_rbins = n_rbins;
  a.closed_right = (bin_flags & EPA_BIN_CLOSED_RIGHT) ? 1 : 0, a.func = func, a.out = out, a.nonbinary = nonbinary_out;
  a.lpr_log2 = 0;
  while ((1 << a.lpr_log2) < groups16 && a.lpr_log2 < 8) ++a.lpr_log2;
  const int rpi = kBlock >> a.lpr_log2;
  const int ctiles = groups16 > kBlock ? (groups16 + kBlock - 1) / kBlock : 1;
  // enough workgroups to fill the card, none with fewer than 16 rows per row of lanes
  const long long want = ((long long)P * T * ctiles + 2047) / 2048;
  long long chunk = want > 16LL * rpi ? want : 16LL * rpi;
  chunk = (chunk + rpi - 1) / rpi * rpi;
  a.chunk = (int)(chunk < (1 << 30) ? chunk : (1 << 30));

  const size_t cells = (size_t)n_tbins * n_rbins;
  size_t cblocks = (cells + kBlock - 1) / kBlock;
  cblocks = cblocks < 1 ? 1 : (cblocks > 4096 ? 4096 : cblocks);
  hipLaunchKernelGGL(regrid_clear_kernel, dim3((unsigned)cblocks, (unsigned)T), dim3(kBlock), 0, st, a);
  if (int rc = epa::check_launch("regrid_clear_kernel")) return rc;
  if (cells == 0 || (size_t)P * D == 0) return EPA_OK;

  const dim3 grid((unsigned)((P + a.chunk - 1) / a.chunk), (unsigned)ctiles, (unsigned)T);
  const bool al = D % 16 == 0 && reinterpret_cast<uintptr_t>(mask) % 16 == 0;
  const bool lds = regrid_flags_in_lds(n_rbins);
  int rc;
  if (range_per_ping && lds) {
    if ((rc = launch_regrid_sweep<true, true>(a, al, grid, st))) return rc;
    rc = epa::check_launch("regrid_sweep_kernel_ping_lds");
  } else if (range_per_ping) {
    if ((rc = launch_regrid_sweep<true, false>(a, al, grid, st))) return rc;
    rc = epa::check_launch("regrid_sweep_kernel_ping_global");
  } else if (lds) {
    if ((rc = launch_regrid_sweep<false, true>(a, al, grid, st))) return rc;
    rc = epa::check_launch("regrid_sweep_kernel_lds");
  } else {
    if ((rc = launch_regrid_sweep<false, false>(a, al, grid, st))) return rc;
    rc = epa::check_launch("regrid_sweep_kernel_global");
  }
  if (rc) return rc;
  hipLaunchKernelGGL(regrid_final_kernel, dim3((unsigned)cblocks, (unsigned)T), dim3(kBlock), 0, st, a);
  return epa::check_launch("regrid_final_kernel");
}
