// Region tables (mask.label_regions, mask.region_statistics): what a labelled (ping, range) plane holds per region.
//
// The labelling is epa_shoal_label (shoal.hip) as it stands: a code per pixel, -(id + 2) on component id and -1 on
// background, ids from an atomic counter and so in no particular order.  Two entries follow it:
//   epa_region_stats    one sweep over the code plane and the C planes of Sv and of the range ->
//                       per (channel, id) the raw sums, counts and extrema the statistics are made of,
//                       per id the pixel count and the smallest linear pixel index (the host orders the ids by it:
//                       the raster-order numbering of scipy.ndimage.label)                 -> region_stats_kernel
//   epa_region_labels   code plane + rank table (id -> number) -> int32 label plane            -> region_labels_kernel
//
// The sweep: a wave owns 64 adjacent samples (coalesced loads) of one channel and walks kPings pings.  A lane sums in
// registers while the code at its sample stays the same from ping to ping; when the code of any lane changes the wave
// flushes: runs of adjacent lanes with one code are folded into the run's first lane by a segmented shuffle
// reduction, and that lane updates the table, once per run -- never once per pixel.  Inside one large school a wave
// flushes once per kPings pings (64 * kPings pixels per update of the school's entry); a plane of single-pixel regions
// flushes a run per pixel, on as many different entries.  Extrema are updated only where they improve the entry.
// Background costs the code load alone: Sv is not read there, the range only in waves that hold foreground.
// Sums depend on the order in which the updates arrive: their last bits can differ from run to run; counts and extrema
// cannot.  No workgroup waits for another.
#include "epa_internal.h"
#include "fast_math.h"
#include "ordered_key.h"
#include "union_find.h"

namespace {

using epa::uf::ld;

using epa::kWaves;
constexpr int kPings = 32;       // pings walked by one wave
constexpr int kMaxBlocks = 4096;  // workgroups of the sweep (each builds the 10^x table once, then strides over the tiles)

// the extrema are maxima of ordered keys in tables the caller zeroed: no number has the key 0 (epa::kKeyNoMax)
using epa::ordered_key;
static_assert(epa::kKeyNoMax == 0ull, "a zeroed table holds 'nothing seen'");

// what a lane has gathered for the code it sits on
struct Acc {
  unsigned n_pix, n_valid, n_range;
  long long first;               // smallest linear pixel index
  double sv_max, r_min, r_max;   // -inf, +inf, -inf: nothing seen
  double s_sv, s_r, s_sv_r, s_sv_at_r, s_dz, s_sv_dz;
  __device__ __forceinline__ void reset() {
    n_pix = n_valid = n_range = 0;
    first = 0x7fffffffffffffffLL;
    sv_max = r_max = -__builtin_inf();
    r_min = __builtin_inf();
    s_sv = s_r = s_sv_r = s_sv_at_r = s_dz = s_sv_dz = 0.0;
  }
};

// v of the lanes [lane, end] folded into lane (end: the last lane of the run `lane` belongs to)
template <typename V, typename Op>
__device__ __forceinline__ V run_reduce(V v, int lane, int end, Op op) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const V o = __shfl_down(v, d, 64);
    if (lane + d <= end) v = op(v, o);
  }
  return v;
}

struct Tables {
  unsigned long long* stats;  // [C][n][EPA_REGION_WORDS]
  unsigned long long* ids;    // [n][EPA_REGION_ID_WORDS]
  long long n, n_pix;
  int C;
};

__device__ __forceinline__ void add_f64(unsigned long long* word, double v) {
  if (v != 0.0) unsafeAtomicAdd(reinterpret_cast<double*>(word), v);
}
__device__ __forceinline__ void max_key(unsigned long long* word, unsigned long long key) {
  if (key > ld(word)) atomicMax(word, key);
}

// every lane of the wave calls it; `code` is -1 or a checked code
__device__ void flush(const Tables& t, int c, long long code, Acc& a) {
  const int lane = threadIdx.x & 63;
  const bool fg = code != -1;
  if (!__any(fg)) return;
  const long long left = __shfl_up(code, 1, 64), right = __shfl_down(code, 1, 64);
  const bool head = fg && (lane == 0 || left != code);
  const bool last = !fg || lane == 63 || right != code;  // a background lane is a run of its own: it takes nothing in
  const unsigned long long lasts = __ballot(last);
  const int end = lane + __ffsll((long long)(lasts >> lane)) - 1;
  const auto sum = [](auto x, auto y) { return x + y; };
  const auto mx = [](double x, double y) { return x > y ? x : y; };
  const auto mn = [](double x, double y) { return x < y ? x : y; };
  if (c == 0) {
    a.n_pix = run_reduce(a.n_pix, lane, end, sum);
    a.first = run_reduce(a.first, lane, end, [](long long x, long long y) { return x < y ? x : y; });
  }
  if (t.C > 0) {
    a.n_valid = run_reduce(a.n_valid, lane, end, sum);
    a.n_range = run_reduce(a.n_range, lane, end, sum);
    a.sv_max = run_reduce(a.sv_max, lane, end, mx);
    a.r_min = run_reduce(a.r_min, lane, end, mn);
    a.r_max = run_reduce(a.r_max, lane, end, mx);
    a.s_sv = run_reduce(a.s_sv, lane, end, sum);
    a.s_r = run_reduce(a.s_r, lane, end, sum);
    a.s_sv_r = run_reduce(a.s_sv_r, lane, end, sum);
    a.s_sv_at_r = run_reduce(a.s_sv_at_r, lane, end, sum);
    a.s_dz = run_reduce(a.s_dz, lane, end, sum);
    a.s_sv_dz = run_reduce(a.s_sv_dz, lane, end, sum);
  }
  if (!head) return;
  const long long id = -code - 2;  // in [0, n): checked where the code was read
  if (c == 0) {
    unsigned long long* e = t.ids + (size_t)id * EPA_REGION_ID_WORDS;
    atomicAdd(e + EPA_REGION_ID_SAMPLES, (unsigned long long)a.n_pix);
    max_key(e + EPA_REGION_ID_FIRST, (unsigned long long)(t.n_pix - a.first));
  }
  if (t.C > 0) {
    unsigned long long* e = t.stats + ((size_t)c * (size_t)t.n + (size_t)id) * EPA_REGION_WORDS;
    if (a.n_valid) {
      atomicAdd(e + EPA_REGION_N_VALID, (unsigned long long)a.n_valid);
      max_key(e + EPA_REGION_SV_MAX, ordered_key(a.sv_max));
      add_f64(e + EPA_REGION_SUM_SV, a.s_sv);
      add_f64(e + EPA_REGION_SUM_SV_DZ, a.s_sv_dz);
    }
    if (a.n_range) {
      atomicAdd(e + EPA_REGION_N_RANGE, (unsigned long long)a.n_range);
      max_key(e + EPA_REGION_RANGE_MIN, ordered_key(-a.r_min));
      max_key(e + EPA_REGION_RANGE_MAX, ordered_key(a.r_max));
      add_f64(e + EPA_REGION_SUM_RANGE, a.s_r);
      add_f64(e + EPA_REGION_SUM_SV_RANGE, a.s_sv_r);
      add_f64(e + EPA_REGION_SUM_SV_AT_RANGE, a.s_sv_at_r);
      add_f64(e + EPA_REGION_SUM_DZ, a.s_dz);
    }
  }
}

// Tiles: (channel, 64 samples, kPings pings), the channel fastest: the waves of a workgroup read the same codes.
// rs_c / rs_p: element strides of the range along channel and ping (0: shared), samples adjacent.
template <typename T>
__global__ __launch_bounds__(epa::kBlock) void region_stats_kernel(const long long* __restrict__ codes,
                                                                   const T* __restrict__ sv, const T* __restrict__ rng,
                                                                   long long rs_c, long long rs_p, long long P,
                                                                   long long S, Tables t, unsigned long long* err) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[epa::kMathTabBytes];
  const epa::MathTabs mt = epa::build_math_tabs(smem);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long nc = t.C > 0 ? t.C : 1;
  const long long segs = (S + 63) / 64, chunks = (P + kPings - 1) / kPings, tiles = nc * segs * chunks;
  const double nan = __builtin_nan("");
  for (long long w = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); w < tiles; w += (long long)gridDim.x * kWaves) {
    const int c = (int)(w % nc);
    const long long tile = w / nc, seg = tile % segs, p0 = (tile / segs) * kPings;
    const long long p1 = p0 + kPings < P ? p0 + kPings : P;
    const long long s = seg * 64 + lane;
    long long cur = -1;
    Acc a;
    a.reset();
    for (long long p = p0; p < p1; ++p) {
      const long long q = p * S + s;
      long long code = s < S ? codes[q] : -1;
      if (code != -1 && (code > -2 || -code - 2 >= t.n)) {  // no id of this table: counted, never written
        atomicAdd(err, 1ull);
        code = -1;
      }
      if (__any(code != cur)) {
        flush(t, c, cur, a);
        a.reset();
        cur = code;
      }
      if (!__any(code != -1)) continue;
      const bool fg = code != -1;
      if (fg) {
        ++a.n_pix;
        if (q < a.first) a.first = q;
      }
      if (t.C == 0) continue;
      const T* rrow = rng + c * rs_c + p * rs_p;
      const double r = s < S ? (double)rrow[s] : nan;
      double before = __shfl_up(r, 1, 64);
      if (lane == 0) before = s > 0 && s < S ? (double)rrow[s - 1] : nan;
      if (!fg) continue;
      const double dz = s > 0 ? r - before : (S > 1 ? (double)rrow[1] - r : nan);
      const double x = (double)sv[((long long)c * P + p) * S + s];
      const double lin = epa::lin_from_db(x, mt.exp2_tab);
      const bool xv = x == x, rv = r == r, dv = dz == dz;
      if (xv) {
        ++a.n_valid;
        a.s_sv += lin;
        a.sv_max = x > a.sv_max ? x : a.sv_max;
        if (rv) {
          a.s_sv_r += lin * r;
          a.s_sv_at_r += lin;
        }
        if (dv) a.s_sv_dz += lin * dz;
      }
      if (rv) {
        ++a.n_range;
        a.s_r += r;
        a.r_min = r < a.r_min ? r : a.r_min;
        a.r_max = r > a.r_max ? r : a.r_max;
      }
      if (dv) a.s_dz += dz;
    }
    flush(t, c, cur, a);
  }
}

__global__ __launch_bounds__(epa::kBlock) void region_labels_kernel(const long long* __restrict__ codes, long long n_pix,
                                                                    const int* __restrict__ rank, long long n,
                                                                    int* __restrict__ labels) {
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n_pix; q += (long long)gridDim.x * blockDim.x) {
    const long long code = codes[q];
    const long long id = -code - 2;
    labels[q] = (code <= -2 && id < n) ? rank[id] : 0;
  }
}

int check_plane(const char* who, const long long* code, long long P, long long S, long long n) {
  EPA_CHECK_ARG(code, "%s: NULL code plane", who);
  EPA_CHECK_ARG(P > 0 && S > 0 && P < 0x7fffffffLL && S < 0x7fffffffLL, "%s: P=%lld S=%lld", who, P, S);
  EPA_CHECK_ARG(n > 0 && n <= 0x70000000LL && n <= P * S, "%s: n=%lld regions (1 .. min(P*S, 0x70000000))", who, n);
  return EPA_OK;
}

}  // namespace

extern "C" int epa_region_stats(const long long* code, long long P, long long S, const void* sv, const void* range,
                                int dtype, long long C, long long range_stride_c, long long range_stride_p,
                                long long n, unsigned long long* stats, unsigned long long* ids,
                                unsigned long long* state, epa_stream_t stream) {
  const char* who = "epa_region_stats";
  if (int rc = check_plane(who, code, P, S, n)) return rc;
  EPA_CHECK_ARG(ids && state, "%s: NULL table argument", who);
  EPA_CHECK_ARG(C >= 0 && C <= 65535, "%s: C=%lld channels", who, C);
  if (C > 0) {
    EPA_CHECK_ARG(sv && range && stats, "%s: NULL array argument", who);
    EPA_CHECK_REAL(who, dtype);
    EPA_CHECK_ARG(range_stride_c >= 0 && range_stride_p >= 0, "%s: range strides %lld, %lld", who, range_stride_c,
                  range_stride_p);
  }
  hipStream_t st = (hipStream_t)stream;
  const Tables t{stats, ids, n, P * S, (int)C};
  const long long tiles = (C > 0 ? C : 1) * ((S + 63) / 64) * ((P + kPings - 1) / kPings);
  const long long want = (tiles + kWaves - 1) / kWaves;
  const int nb = (int)(want > kMaxBlocks ? kMaxBlocks : want);
  unsigned long long* err = state + EPA_SHOAL_STATE_ERROR;
  return epa::dispatch_real(who, C > 0 ? dtype : EPA_F64, [&](auto tag) {
    using T = typename decltype(tag)::type;
    region_stats_kernel<T><<<nb, epa::kBlock, 0, st>>>(code, (const T*)sv, (const T*)range, range_stride_c,
                                                       range_stride_p, P, S, t, err);
    return epa::check_launch("region_stats_kernel");
  });
}

extern "C" int epa_region_labels(const long long* code, long long P, long long S, const int* rank, long long n,
                                 int* labels, epa_stream_t stream) {
  const char* who = "epa_region_labels";
  if (int rc = check_plane(who, code, P, S, n)) return rc;
  EPA_CHECK_ARG(rank && labels, "%s: NULL array argument", who);
  const long long n_pix = P * S;
  const long long want = (n_pix + epa::kBlock - 1) / epa::kBlock;
  region_labels_kernel<<<(int)(want > 16384 ? 16384 : want), epa::kBlock, 0, (hipStream_t)stream>>>(code, n_pix, rank, n,
                                                                                                    labels);
  return epa::check_launch("region_labels_kernel");
}
