// Volume backscattering spectra Sv(f) of range cells from EK80 FM pings (calibrate.compute_Sv_spectrum): a short-time
// Fourier analysis of the whole pulse-compressed volume.  The rules are this project's restatement of Andersen et al.
// (2021), "Quantitative processing of broadband data as implemented in a scientific split-beam echosounder";
// echopype_amd/calibrate/sv_spectrum.py states them word for word and tests/sv_spectrum_ref.py is the NumPy judge.
// One entry, two kernels:
//   sv_spectrum_replica_kernel   spectrum_common.h: per replica and frequency the step w = exp(-2 pi i f dt) and
//                                1 / |A(f)|^2 with lags up to min(floor((N_w - 1) / 2), L - 1) -> `table`
//   sv_spectrum_kernel           per (ping, tile of consecutive cells): span staged, compressed, Fourier sums, rules 7, 8
//
// A workgroup (256 lanes) serves one tile: the cells m0 .. m0 + nc - 1 of one ping, which cover the samples
// n0 .. n0 + span - 1 (span = (nc - 1) hop + N_w).  The samples n0 .. n0 + span + L - 2 are staged ONCE in LDS as the
// sector SUM (NaN zero-filled) with a validity byte per sample, the replica beside them; a span with a mixed NaN
// pattern takes one compression per sector behind a workgroup-uniform branch (the device of target_spectrum.hip).
// Lane t compresses J = ceil(span / 256) consecutive samples of the span side by side, every tap sum in tap order (a tap
// and a staged sample read from LDS serve J sums: compress_span), into ps(n) = r(n) pc(n) in LDS: overlapping cells of
// a tile share it, and no compressed cube goes to HBM.  The Fourier sums run over the
// (cell, frequency) pairs of the tile, consecutive lanes on consecutive frequencies (so are the stores):
// Y = sum_k w~(k) ps(n_m + k) w^k by Horner's rule, w~ and ps read from LDS as broadcasts.  All arithmetic is float64
// and no sum depends on scheduling.  Not a GEMM here: MFMA forms are left out.
#include "spectrum_common.h"

namespace {

using epa::kBlock;
using epa::kWave;
using epa::kWaves;
using epa::spectrum::Cd;
using epa::spectrum::replica_taps;
using epa::spectrum::stage_replica;
using epa::spectrum::stage_window;

constexpr int kMaxWin = EPA_SV_SPECTRUM_MAX_WINDOW;
constexpr int kMaxF = EPA_SV_SPECTRUM_MAX_FREQ;
constexpr int kMaxTaps = EPA_SV_SPECTRUM_MAX_TAPS;
constexpr int kFP = EPA_SV_SPECTRUM_FPARAMS;
constexpr int kPP = EPA_SV_SPECTRUM_PPARAMS;
constexpr int kTab = EPA_SV_SPECTRUM_TABLE_ROWS;
constexpr int kMaxCells = EPA_SV_SPECTRUM_MAX_TILE_CELLS;
constexpr int kMaxBeams = 8;
constexpr int kMaxGrid = 1 << 20;  // workgroups of a launch; each takes further tiles in a loop
static_assert(kFP == 5 && kPP == 4, "the rows of fparams and pparams the kernel reads by number");
// The tile: as many cells as keep a workgroup's LDS within a third of a CU's 160 KiB (three workgroups = 12 wavefronts
// per CU), at most kMaxCells, at least one -- whatever that one takes, up to the whole 160 KiB.
constexpr int kMaxJ = 5;  // samples of the span a lane compresses side by side (compress_span)
constexpr size_t kLdsCu = 160 * 1024;
constexpr size_t kLdsTarget = kLdsCu / 3;

struct Args {
  static constexpr int kFParams = kFP, kTableRows = kTab;  // (what spectrum_common.h reads)
  const void* re;
  const void* im;
  long long C, P, S;
  int B;
  const float* replica;        // interleaved (re, im) f32
  const int32_t* replica_off;  // [R + 1] in complex elements
  const int32_t* replica_id;   // optional [C*P]; NULL: replica c for every ping of channel c
  int R;
  long long replica_len;
  int max_taps;
  const double* rep_dt;   // [R]
  const double* fparams;  // [R][kFP][F]: f, absorption, gain, z_et, psi
  int F, h;               // h: the largest lag of A(f), floor((Nw - 1) / 2)
  const double* pparams;  // [kPP][C*P]: transmit power, sound speed, z_er, sample interval
  const double* window;   // [Nw]: w~
  int Nw;
  long long hop, M;
  int T, tiles;  // cells of a tile; tiles of a ping
  long long total;
  double* table;  // [R][kTab][F]: w.re, w.im, 1 / |A|^2
  void* sv;       // [C*P][M][F]
  double* range;  // [C*P][M]
  unsigned xs_off, ps_off, win_off, ok_off, mask_off;  // byte offsets in dynamic LDS (the replica is first)
};

// r(n) = (n dt) (c_w / 2), the expression of echo_range for complex samples (power_coef.hip, ek80_complex.hip)
__device__ __forceinline__ double sample_range(long long n, double dt, double half_c) { return ((double)n * dt) * half_c; }

// r_m = (r(n_m) + r(n_m + Nw - 1)) / 2, every operation rounded on its own: echo_range is held to bit equality
__device__ __forceinline__ double cell_range(long long n_first, int Nw, double dt, double half_c) {
#pragma clang fp contract(off)
  const double r0 = ((double)n_first * dt) * half_c;
  const double r1 = ((double)(n_first + Nw - 1) * dt) * half_c;
  return (r0 + r1) / 2.0;
}

__device__ __forceinline__ void mac(double& ar, double& ai, const Cd& x, const Cd& t) {
  ar = fma(x.re, t.re, ar);
  ar = fma(x.im, t.im, ar);
  ai = fma(x.im, t.re, ai);
  ai = fma(-x.re, t.im, ai);
}

// acc(i) = sum_k xs(i + k) conj(rep(k)), every sum in tap order.  Lane t owns the J consecutive samples J t .. J t + J - 1
// (and those kBlock J further on): a tap read from LDS serves J sums, and of the J samples a sum step needs, J - 1 are
// kept in registers from the step before (a sliding window; the index arithmetic below is all compile-time).  Reads up
// to J - 1 staged samples past the last one a kept sum needs.  bit < 0: ps(i) = acc(i); else ps(i) += acc(i) where
// sector `bit` is valid at i.  (No barrier inside: a lane owns its samples.)
template <int J>
__device__ __forceinline__ void compress_span_j(const Cd* xs, const Cd* rep, int L, int span, const uint8_t* vmask, int bit,
                                                Cd* ps) {
  for (int base = threadIdx.x * J; base < span; base += kBlock * J) {
    double ar[J], ai[J];
    Cd x[J];
#pragma unroll
    for (int j = 0; j < J; ++j) ar[j] = ai[j] = 0.0;
#pragma unroll
    for (int j = 0; j < J - 1; ++j) x[j] = xs[base + j];
    int k = 0;
    for (; k + J <= L; k += J) {
#pragma unroll
      for (int u = 0; u < J; ++u) {
        x[(u + J - 1) % J] = xs[base + k + u + J - 1];
        const Cd t = rep[k + u];
#pragma unroll
        for (int j = 0; j < J; ++j) mac(ar[j], ai[j], x[(u + j) % J], t);
      }
    }
    for (; k < L; ++k) {  // (the window is back at x[0 .. J - 2] after every whole turn)
      x[J - 1] = xs[base + k + J - 1];
      const Cd t = rep[k];
#pragma unroll
      for (int j = 0; j < J; ++j) mac(ar[j], ai[j], x[j], t);
#pragma unroll
      for (int j = 0; j < J - 1; ++j) x[j] = x[j + 1];
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int i = base + j;
      if (i >= span) break;
      if (bit < 0)
        ps[i] = Cd{ar[j], ai[j]};
      else if (vmask[i] & (1u << bit))
        ps[i].re += ar[j], ps[i].im += ai[j];
    }
  }
}

// J = ceil(span / 256) up to kMaxJ: one pass with every lane busy for spans up to 256 kMaxJ samples (workgroup-uniform)
__device__ __forceinline__ void compress_span(const Cd* xs, const Cd* rep, int L, int span, const uint8_t* vmask, int bit,
                                              Cd* ps) {
  switch ((span + kBlock - 1) / kBlock) {
    case 1: return compress_span_j<1>(xs, rep, L, span, vmask, bit, ps);
    case 2: return compress_span_j<2>(xs, rep, L, span, vmask, bit, ps);
    case 3: return compress_span_j<3>(xs, rep, L, span, vmask, bit, ps);
    case 4: return compress_span_j<4>(xs, rep, L, span, vmask, bit, ps);
    default: return compress_span_j<kMaxJ>(xs, rep, L, span, vmask, bit, ps);
  }
}

template <typename InT, typename OutT>
__global__ __launch_bounds__(kBlock) void sv_spectrum_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Cd* rep = reinterpret_cast<Cd*>(smem);
  Cd* xs = reinterpret_cast<Cd*>(smem + a.xs_off);
  Cd* ps = reinterpret_cast<Cd*>(smem + a.ps_off);
  double* win = reinterpret_cast<double*>(smem + a.win_off);
  int* ok = reinterpret_cast<int*>(smem + a.ok_off);
  uint8_t* vmask = smem + a.mask_off;
  __shared__ double red[kWaves];
  const int tid = threadIdx.x;
  const int Nw = a.Nw, F = a.F;
  const long long hop = a.hop;
  const size_t CP = (size_t)a.C * a.P;
  const InT* re = static_cast<const InT*>(a.re);
  const InT* im = static_cast<const InT*>(a.im);
  const unsigned full = (1u << a.B) - 1u;
  for (int k = tid; k < Nw; k += kBlock) win[k] = a.window[k];  // (published by the first barrier of the loop)
  for (long long w = blockIdx.x; w < a.total; w += gridDim.x) {
    __syncthreads();  // the tile before is done with LDS
    const size_t row = (size_t)(w / a.tiles);
    const int tile = (int)(w - (long long)row * a.tiles);
    const long long m0 = (long long)tile * a.T;
    const int nc = (int)(a.M - m0 < a.T ? a.M - m0 : a.T);
    const long long n0 = m0 * hop;
    const int span = (int)((nc - 1) * hop) + Nw;
    const int c = (int)(row / (size_t)a.P);
    const double p_t = a.pparams[row], c_w = a.pparams[CP + row], z_er = a.pparams[2 * CP + row];
    const double dt = a.pparams[3 * CP + row], half_c = c_w / 2;
    OutT* out = static_cast<OutT*>(a.sv) + ((size_t)row * a.M + m0) * F;
    double* rng = a.range + (size_t)row * a.M + m0;
    for (int m = tid; m < nc; m += kBlock) rng[m] = cell_range(n0 + m * hop, Nw, dt, half_c);
    // ---- the replica of the ping, checked: nothing is read through an index the arrays do not hold (all uniform)
    int r0 = 0, L = 0;
    const int rid = a.replica_id ? a.replica_id[row] : c;
    if (rid >= 0 && rid < a.R) L = replica_taps(a, rid, r0);
    if (L == 0) {  // covered by no filter interval: NaN cells, their echo_range written
      for (int q = tid; q < nc * F; q += kBlock) out[q] = epa::M<OutT>::nan();
      continue;
    }
    const size_t ping_base = row * (size_t)a.S * a.B;
    const int len = span + L - 1 + (kMaxJ - 1);  // (compress_span reads up to kMaxJ - 1 samples past the last tap)
    const double E = stage_replica(a, r0, L, rep, red);
    const unsigned mixed_l = stage_window<InT>(re, im, ping_base, a.S, a.B, n0, len, -1, xs, vmask);
    const int mixed = __syncthreads_or((int)mixed_l);
    // ---- pulse compression of the span
    if (!mixed) {
      compress_span(xs, rep, L, span, vmask, -1, ps);
    } else {
      // one compression per sector; a sector counts at sample n only where it is valid at n
      for (int i = tid; i < span; i += kBlock) ps[i] = Cd{0.0, 0.0};
      for (int b = 0; b < a.B; ++b) {
        __syncthreads();
        stage_window<InT>(re, im, ping_base, a.S, a.B, n0, len, b, xs, vmask);
        __syncthreads();
        compress_span(xs, rep, L, span, vmask, b, ps);
      }
    }
    __syncthreads();  // (compress_span and the loops around it assign the samples to lanes differently)
    // ---- ps(n) = r(n) pc(n)
    for (int i = tid; i < span; i += kBlock) {
      const unsigned nv = __popc(vmask[i] & full);
      Cd v{0.0, 0.0};
      if (nv) {
        const double d = E * (double)nv, r = sample_range(n0 + i, dt, half_c);
        v = Cd{r * (ps[i].re / d), r * (ps[i].im / d)};
      }
      ps[i] = v;
    }
    // ---- a cell counts when all its samples are valid and its centre lies at a positive range
    for (int m = tid; m < nc; m += kBlock) {
      const uint8_t* vm = vmask + (size_t)m * hop;
      int good = cell_range(n0 + m * hop, Nw, dt, half_c) > 0.0;
      for (int k = 0; k < Nw; ++k) good &= (vm[k] & full) != 0u;
      ok[m] = good;
    }
    __syncthreads();
    // ---- Fourier sums and rules 7 and 8 over the (cell, frequency) pairs
    const double* tab = a.table + (size_t)rid * kTab * F;
    const double* fp = a.fparams + (size_t)rid * kFP * F;
    const double len_db = 10.0 * ::log10((double)Nw * dt);
    for (int q = tid; q < nc * F; q += kBlock) {
      const int m = q / F, j = q - m * F;
      if (!ok[m]) {
        out[q] = epa::M<OutT>::nan();
        continue;
      }
      const Cd* x = ps + (size_t)m * hop;
      const double wr = tab[j], wi = tab[F + j], inv_a2 = tab[2 * F + j];
      double yr = win[Nw - 1] * x[Nw - 1].re, yi = win[Nw - 1] * x[Nw - 1].im;
      for (int k = Nw - 2; k >= 0; --k) {
        const double g = win[k];
        const Cd v = x[k];
        const double nr = fma(yr, wr, fma(-yi, wi, g * v.re));
        const double ni = fma(yr, wi, fma(yi, wr, g * v.im));
        yr = nr, yi = ni;
      }
      const double f = fp[j], alpha = fp[F + j], gain = fp[2 * F + j], z_et = fp[3 * F + j], psi = fp[4 * F + j];
      const double zr = ::fabs(z_er + z_et) / z_er;
      double prx = (double)a.B * ((yr * yr + yi * yi) * inv_a2) / 8.0 * (zr * zr) / z_et;
      if (!(prx > 0.0) || !(prx < __builtin_inf())) prx = __builtin_nan("");
      const double lam = c_w / f, r_m = cell_range(n0 + m * hop, Nw, dt, half_c);
      const double sv = 10.0 * ::log10(prx) + 2.0 * alpha * r_m -
                        10.0 * ::log10(p_t * lam * lam * c_w / (32.0 * M_PI * M_PI)) - 2.0 * gain - len_db - psi;
      out[q] = (OutT)sv;
    }
  }
}

struct Plan {
  int T, tiles;
  unsigned xs_off, ps_off, win_off, ok_off, mask_off;
  size_t total;
};

size_t lds_bytes(int max_taps, int Nw, long long span, long long cells, Plan* p) {
  const size_t staged = (size_t)span + (size_t)max_taps - 1 + (kMaxJ - 1);
  size_t o = (size_t)max_taps * sizeof(Cd);
  const size_t xs = o;
  o += staged * sizeof(Cd);
  const size_t ps = o;
  o += (size_t)span * sizeof(Cd);
  const size_t win = o;
  o += (size_t)Nw * sizeof(double);
  const size_t ok = o;
  o += (size_t)cells * sizeof(int);
  const size_t mask = o;
  o = (o + staged + 15) & ~(size_t)15;
  if (p) p->xs_off = (unsigned)xs, p->ps_off = (unsigned)ps, p->win_off = (unsigned)win, p->ok_off = (unsigned)ok,
         p->mask_off = (unsigned)mask, p->total = o;
  return o;
}

// the tile of (max_taps, Nw, hop, M): see kLdsTarget.  false: one cell does not fit a CU's LDS.
bool make_plan(int max_taps, int Nw, long long hop, long long M, Plan* p) {
  long long T = 1;
  const long long cap = M < kMaxCells ? M : kMaxCells;
  while (T < cap && lds_bytes(max_taps, Nw, T * hop + Nw, T + 1, nullptr) <= kLdsTarget) ++T;  // (T + 1 cells fit)
  const long long tiles = (M + T - 1) / T;
  T = (M + tiles - 1) / tiles;  // the same number of tiles, evenly filled
  p->T = (int)T, p->tiles = (int)tiles;
  return lds_bytes(max_taps, Nw, (T - 1) * hop + Nw, T, p) <= kLdsCu;
}

bool aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace

// f64 [R][EPA_SV_SPECTRUM_TABLE_ROWS][F]: per replica and frequency the step w (re, im) and 1 / |A|^2
size_t epa::scratch::sv_spectrum_table(long long R, long long F, long long) {
  return (size_t)R * kTab * (size_t)F * sizeof(double);
}

extern "C" int epa_sv_spectrum_plan(int max_taps, int window_samples, long long step_samples, long long M, int* tile_cells,
                                    int* tiles, size_t* lds_bytes_out) {
  const char* who = "epa_sv_spectrum_plan";
  EPA_CHECK_ARG(max_taps >= 1 && max_taps <= kMaxTaps && window_samples >= 2 && window_samples <= kMaxWin &&
                    step_samples >= 1 && step_samples < 0x7fffffffLL && M >= 1 && M < 0x7fffffffLL,
                "%s: max_taps=%d window_samples=%d step_samples=%lld M=%lld", who, max_taps, window_samples, step_samples, M);
  EPA_CHECK_ARG(tile_cells && tiles && lds_bytes_out, "%s: NULL argument", who);
  Plan p;
  EPA_CHECK_ARG(make_plan(max_taps, window_samples, step_samples, M, &p),
                "%s: a window of %d samples with replicas of %d taps does not fit the %zu bytes of LDS of a CU", who,
                window_samples, max_taps, kLdsCu);
  *tile_cells = p.T, *tiles = p.tiles, *lds_bytes_out = p.total;
  return EPA_OK;
}

extern "C" int epa_sv_spectrum(const void* re, const void* im, int in_dtype, long long C, long long P, long long S, int B,
                               const float* replica, const int32_t* replica_off, const int32_t* replica_id,
                               int n_replicas, long long replica_len, int max_taps, const double* rep_dt,
                               const double* fparams, int F, const double* pparams, const double* window,
                               int window_samples, long long step_samples, long long M, double* table, void* sv_out,
                               int out_dtype, double* range_out, epa_stream_t stream) {
  const char* who = "epa_sv_spectrum";
  EPA_CHECK_REAL(who, in_dtype);
  EPA_CHECK_REAL_OUT(who, out_dtype);
  EPA_CHECK_ARG(C > 0 && P > 0 && S > 0 && C <= 65535 && P < 0x7fffffffLL && S < 0x7fffffffLL - kMaxWin - kMaxTaps &&
                    C * P < 0x7fffffffLL,
                "%s: bad shape C=%lld P=%lld S=%lld", who, C, P, S);
  EPA_CHECK_ARG(B > 0 && B <= kMaxBeams, "%s: 1 .. %d sectors supported (got %d)", who, kMaxBeams, B);
  EPA_CHECK_ARG(window_samples >= 2 && window_samples <= kMaxWin, "%s: window_samples %d outside 2 .. %d", who,
                window_samples, kMaxWin);
  EPA_CHECK_ARG(step_samples >= 1 && step_samples < 0x7fffffffLL, "%s: step_samples %lld outside 1 .. 2^31 - 2", who,
                step_samples);
  EPA_CHECK_ARG(F >= 1 && F <= kMaxF, "%s: %d frequencies outside 1 .. %d", who, F, kMaxF);
  EPA_CHECK_ARG(max_taps >= 1 && max_taps <= kMaxTaps, "%s: replicas of up to %d taps are served (max_taps %d)", who,
                kMaxTaps, max_taps);
  EPA_CHECK_ARG(S >= window_samples, "%s: a window of %d samples on pings of %lld", who, window_samples, S);
  EPA_CHECK_ARG(M == (S - window_samples) / step_samples + 1, "%s: M=%lld is not floor((S - window_samples) / step_samples) + 1", who, M);
  EPA_CHECK_ARG(n_replicas >= 1 && n_replicas <= 65535 && replica_len >= 1 && replica_len < 0x7fffffffLL,
                "%s: n_replicas=%d replica_len=%lld", who, n_replicas, replica_len);
  EPA_CHECK_ARG(replica_id || n_replicas >= C, "%s: without replica_id every channel needs its replica (%d of %lld)", who,
                n_replicas, C);
  Plan p;
  EPA_CHECK_ARG(make_plan(max_taps, window_samples, step_samples, M, &p),
                "%s: a window of %d samples with replicas of %d taps does not fit the %zu bytes of LDS of a CU", who,
                window_samples, max_taps, kLdsCu);
  EPA_CHECK_ARG(re && im && replica && replica_off && rep_dt && fparams && pparams && window, "%s: NULL array argument", who);
  EPA_CHECK_ARG(table && sv_out && range_out, "%s: NULL output argument", who);
  const size_t in_size = in_dtype == EPA_F64 ? 8 : 4, out_size = out_dtype == EPA_F64 ? 8 : 4;
  EPA_CHECK_ARG(aligned(re, in_size) && aligned(im, in_size) && aligned(replica, 4) && aligned(replica_off, 4) &&
                    aligned(replica_id, 4) && aligned(rep_dt, 8) && aligned(fparams, 8) && aligned(pparams, 8) &&
                    aligned(window, 8) && aligned(table, 8) && aligned(sv_out, out_size) && aligned(range_out, 8),
                "%s: an array is not aligned to its element size", who);
  Args a = {};
  a.re = re, a.im = im, a.C = C, a.P = P, a.S = S, a.B = B;
  a.replica = replica, a.replica_off = replica_off, a.replica_id = replica_id, a.R = n_replicas;
  a.replica_len = replica_len, a.max_taps = max_taps, a.rep_dt = rep_dt, a.fparams = fparams, a.F = F;
  a.h = (window_samples - 1) / 2;
  a.pparams = pparams, a.window = window, a.Nw = window_samples, a.hop = step_samples, a.M = M;
  a.T = p.T, a.tiles = p.tiles, a.total = C * P * (long long)p.tiles;
  a.table = table, a.sv = sv_out, a.range = range_out;
  a.xs_off = p.xs_off, a.ps_off = p.ps_off, a.win_off = p.win_off, a.ok_off = p.ok_off, a.mask_off = p.mask_off;
  hipStream_t st = (hipStream_t)stream;
  {
    // (the replica, then the lags a(0 .. h) where the main kernel keeps its span)
    const int hh = a.h < max_taps - 1 ? a.h : max_taps - 1;
    const size_t lds = (size_t)p.xs_off + (size_t)(hh + 1) * sizeof(Cd);
    auto kern = epa::spectrum::replica_table_kernel<Args>;
    if (int rc = epa::allow_lds(kern, lds)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_replicas), dim3(kBlock), lds, st, a);
    if (int rc = epa::check_launch("sv_spectrum_replica_kernel")) return rc;
  }
  const unsigned grid = (unsigned)(a.total < kMaxGrid ? a.total : kMaxGrid);
  return epa::dispatch_real(who, in_dtype, [&](auto in) {
    return epa::dispatch_real(who, out_dtype, [&](auto out) {
      using InT = typename decltype(in)::type;
      using OutT = typename decltype(out)::type;
      auto kern = sv_spectrum_kernel<InT, OutT>;
      if (int rc = epa::allow_lds(kern, p.total)) return rc;
      hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), p.total, st, a);
      return epa::check_launch("sv_spectrum_kernel");
    });
  });
}
