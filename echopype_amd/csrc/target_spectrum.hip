// Target strength spectra TS(f) of single targets from EK80 FM pings (targets.target_spectra): the broadband product
// behind the target table.  The rules are this project's restatement of Andersen et al. (2021), "Quantitative
// processing of broadband data as implemented in a scientific split-beam echosounder"; echopype_amd/targets/spectra.py
// states them word for word and tests/target_spectra_ref.py is the NumPy judge.  One entry, two kernels:
//   target_spectrum_replica_kernel   per replica: E = sum |tx|^2, the autocorrelation a(m), |m| <= min(h, L - 1), and
//                                    per frequency the step w = exp(-2 pi i f dt) and 1 / |A(f)|^2 -> `table`
//                                    (spectrum_common.h: shared with sv_spectrum.hip, as is the staging of a span)
//   target_spectrum_kernel           per target: window staged, pulse compression, F Fourier sums, rules 5 to 7
//
// A target belongs to one workgroup (256 lanes), which takes further targets in a loop.  The samples s-h .. s+h+L-1 of
// the target's ping are staged ONCE in LDS as the sector SUM (NaN zero-filled) with a validity mask per sample, the
// replica beside them: exact when all sectors share one NaN pattern over the staged span (the usual end-of-ping padding),
// as in ek80_complex.hip; a span with a mixed pattern takes one compression per sector (a workgroup-uniform branch).
// The 2h+1 compressed samples are few, the taps many: the tap sum of every output is split over G = 256 / (2h+1)
// lanes, whose partial sums go through LDS and are added in lane order (no sum depends on scheduling).  The F Fourier
// sums are one lane per frequency: Y(f) = sum_n pc(s+n) w^n is evaluated by Horner's rule on the window in LDS (every
// lane reads the same sample: a broadcast), and since only |Y / A| enters rule 5 the unit factor w^-h is left out.
// All arithmetic is float64.  Not a GEMM: 2h+1 outputs per target are too few rows for MFMA tiles.
#include "spectrum_common.h"

namespace {

using epa::kBlock;
using epa::kWave;
using epa::kWaves;
using epa::spectrum::Cd;
using epa::spectrum::replica_taps;
using epa::spectrum::stage_replica;
using epa::spectrum::stage_window;

constexpr int kMaxH = EPA_TARGET_SPECTRA_MAX_HALF_WINDOW;
constexpr int kMaxF = EPA_TARGET_SPECTRA_MAX_FREQ;
constexpr int kMaxTaps = EPA_TARGET_SPECTRA_MAX_TAPS;
constexpr int kFP = EPA_TARGET_SPECTRA_FPARAMS;
constexpr int kTab = EPA_TARGET_SPECTRA_TABLE_ROWS;
constexpr int kMaxBeams = 8;
constexpr int kMaxGrid = 1 << 20;  // workgroups of a launch; each takes further targets in a loop
static_assert(2 * kMaxH + 1 <= kBlock, "one lane per compressed sample");

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
  const double* fparams;  // [R][kFP][F]
  int F, h;
  const double* pparams;  // [EPA_TARGET_SPECTRA_PPARAMS][C*P]
  const int32_t* chan_map;
  int n_map;
  const int32_t* t_channel;
  const int32_t* t_ping;
  const int32_t* t_sample;
  const double* t_range;
  const double* t_along;
  const double* t_athw;
  long long N;
  double* table;  // [R][kTab][F]: w.re, w.im, 1 / |A|^2
  void* ts;
  void* ts_uncomp;
  int32_t* n_window;
  unsigned xs_off, part_off, pc_off, mask_off;  // byte offsets in dynamic LDS (the replica is first)
};

// y(i) = sum_k xs(i + k) conj(rep(k)), i < W: the tap sum of output i split over G lanes, added in lane order by lane i.
// (barriers inside: every lane of the workgroup calls it)
__device__ __forceinline__ Cd compress(const Cd* xs, const Cd* rep, int L, int W, int G, Cd* part) {
  const int tid = threadIdx.x;
  if (tid < W * G) {
    const int i = tid / G, j = tid - i * G;
    double ar = 0.0, ai = 0.0;
    for (int k = j; k < L; k += G) {
      const Cd x = xs[i + k], t = rep[k];
      ar = fma(x.re, t.re, ar);
      ar = fma(x.im, t.im, ar);
      ai = fma(x.im, t.re, ai);
      ai = fma(-x.re, t.im, ai);
    }
    part[tid] = Cd{ar, ai};
  }
  __syncthreads();
  Cd y{0.0, 0.0};
  if (tid < W)
    for (int j = 0; j < G; ++j) y.re += part[tid * G + j].re, y.im += part[tid * G + j].im;
  return y;
}

template <typename OutT>
__device__ __forceinline__ void nan_row(const Args& a, long long t) {
  OutT* ts = static_cast<OutT*>(a.ts) + (size_t)t * a.F;
  OutT* tu = static_cast<OutT*>(a.ts_uncomp) + (size_t)t * a.F;
  for (int j = threadIdx.x; j < a.F; j += kBlock) ts[j] = tu[j] = epa::M<OutT>::nan();
  if (threadIdx.x == 0) a.n_window[t] = 0;
}

template <typename InT, typename OutT>
__global__ __launch_bounds__(kBlock) void target_spectrum_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Cd* rep = reinterpret_cast<Cd*>(smem);
  Cd* xs = reinterpret_cast<Cd*>(smem + a.xs_off);
  Cd* part = reinterpret_cast<Cd*>(smem + a.part_off);
  Cd* pc = reinterpret_cast<Cd*>(smem + a.pc_off);
  uint8_t* vmask = smem + a.mask_off;
  __shared__ double red[kWaves];
  const int tid = threadIdx.x;
  const int h = a.h, W = 2 * h + 1, G = kBlock / W, F = a.F;
  const InT* re = static_cast<const InT*>(a.re);
  const InT* im = static_cast<const InT*>(a.im);
  const unsigned full = (1u << a.B) - 1u;
  for (long long t = blockIdx.x; t < a.N; t += gridDim.x) {
    __syncthreads();  // the target before is done with LDS
    // ---- the row of the table, checked: nothing is read through an index the cubes do not hold (all uniform)
    const int ct = a.t_channel[t];
    const long long p = a.t_ping[t], s = a.t_sample[t];
    int c = -1, rid = -1, r0 = 0, L = 0;
    if (ct >= 0 && ct < a.n_map) c = a.chan_map[ct];
    if (c >= 0 && c < a.C && p >= 0 && p < a.P && s >= 0 && s < a.S) {
      rid = a.replica_id ? a.replica_id[(size_t)c * a.P + p] : c;
      if (rid >= 0 && rid < a.R) L = replica_taps(a, rid, r0);
    }
    if (L == 0) {
      nan_row<OutT>(a, t);
      continue;
    }
    const size_t row = (size_t)c * a.P + p;
    const size_t ping_base = row * (size_t)a.S * a.B;
    const int len = W + L - 1;
    const long long first = s - h;
    const double E = stage_replica(a, r0, L, rep, red);
    const unsigned mixed_l = stage_window<InT>(re, im, ping_base, a.S, a.B, first, len, -1, xs, vmask);
    const int mixed = __syncthreads_or((int)mixed_l);
    // ---- pulse compression of the window
    Cd y{0.0, 0.0};
    if (!mixed) {
      y = compress(xs, rep, L, W, G, part);
    } else {
      // one compression per sector; a sector counts at output n only where it is valid at n
      for (int b = 0; b < a.B; ++b) {
        __syncthreads();
        stage_window<InT>(re, im, ping_base, a.S, a.B, first, len, b, xs, vmask);
        __syncthreads();
        const Cd yb = compress(xs, rep, L, W, G, part);
        if (tid < W && (vmask[tid] & (1u << b))) y.re += yb.re, y.im += yb.im;
      }
    }
    int counted = 0;
    if (tid < W) {
      const unsigned nv = __popc(vmask[tid] & full);  // (0 outside [0, S))
      Cd v{0.0, 0.0};
      if (nv) {
        const double d = E * (double)nv;
        v = Cd{y.re / d, y.im / d};
        counted = 1;
      }
      pc[tid] = v;
    }
    const int n_win = __syncthreads_count(counted);
    if (tid == 0) a.n_window[t] = n_win;
    // ---- Fourier sums and rules 5 to 7, a lane per frequency
    const double r = a.t_range[t], th = a.t_along[t], ph = a.t_athw[t];
    const double p_t = a.pparams[row], c_w = a.pparams[(size_t)a.C * a.P + row], z_er = a.pparams[2 * (size_t)a.C * a.P + row];
    const double* tab = a.table + (size_t)rid * kTab * F;
    const double* fp = a.fparams + (size_t)rid * kFP * F;
    OutT* ts = static_cast<OutT*>(a.ts) + (size_t)t * F;
    OutT* tu = static_cast<OutT*>(a.ts_uncomp) + (size_t)t * F;
    const bool r_ok = r > 0.0;
    const double spread = r_ok ? 40.0 * ::log10(r) : __builtin_nan("");
    for (int j = tid; j < F; j += kBlock) {
      const double wr = tab[j], wi = tab[F + j], inv_a2 = tab[2 * F + j];
      double yr = pc[W - 1].re, yi = pc[W - 1].im;
      for (int k = W - 2; k >= 0; --k) {
        const Cd v = pc[k];
        const double nr = fma(yr, wr, fma(-yi, wi, v.re));
        const double ni = fma(yr, wi, fma(yi, wr, v.im));
        yr = nr, yi = ni;
      }
      const double f = fp[j], alpha = fp[F + j], gain = fp[2 * F + j], z_et = fp[3 * F + j];
      const double bw_al = fp[4 * F + j], bw_at = fp[5 * F + j], off_al = fp[6 * F + j], off_at = fp[7 * F + j];
      const double zr = ::fabs(z_er + z_et) / z_er;
      double prx = (double)a.B * ((yr * yr + yi * yi) * inv_a2) / 8.0 * (zr * zr) / z_et;
      if (!(prx > 0.0) || !(prx < __builtin_inf())) prx = __builtin_nan("");
      const double lam = c_w / f;
      const double unc = 10.0 * ::log10(prx) + spread + 2.0 * alpha * r -
                         10.0 * ::log10(p_t * lam * lam / (16.0 * M_PI * M_PI)) - 2.0 * gain;
      const double x = 2.0 * (th - off_al) / bw_al, yy = 2.0 * (ph - off_at) / bw_at;
      const double x2 = x * x, y2 = yy * yy;
      const double comp = 6.0206 * (x2 + y2 - 0.18 * x2 * y2);
      tu[j] = (OutT)unc;
      ts[j] = (OutT)(unc + comp);
    }
  }
}

struct Lds {
  unsigned xs_off, part_off, pc_off, mask_off;
  size_t total;
};
Lds lds_layout(int max_taps, int h) {
  const int W = 2 * h + 1;
  Lds l;
  l.xs_off = (unsigned)((size_t)max_taps * sizeof(Cd));
  l.part_off = l.xs_off + (unsigned)((size_t)(W + max_taps - 1) * sizeof(Cd));
  l.pc_off = l.part_off + (unsigned)(kBlock * sizeof(Cd));
  l.mask_off = l.pc_off + (unsigned)(kBlock * sizeof(Cd));
  l.total = ((size_t)l.mask_off + (size_t)(W + max_taps - 1) + 15) & ~(size_t)15;
  return l;
}

}  // namespace

// f64 [R][EPA_TARGET_SPECTRA_TABLE_ROWS][F]: per replica and frequency the step w (re, im) and 1 / |A|^2
size_t epa::scratch::target_spectra_table(long long R, long long F, long long) {
  return (size_t)R * kTab * (size_t)F * sizeof(double);
}

extern "C" int epa_target_spectra(const void* re, const void* im, int in_dtype, long long C, long long P, long long S,
                                  int B, const float* replica, const int32_t* replica_off, const int32_t* replica_id,
                                  int n_replicas, long long replica_len, int max_taps, const double* rep_dt,
                                  const double* fparams, int F, int half_window, const double* pparams,
                                  const int32_t* chan_map, int n_map, const int32_t* t_channel, const int32_t* t_ping,
                                  const int32_t* t_sample, const double* t_range, const double* t_along,
                                  const double* t_athw, long long N, double* table, void* ts_out, void* ts_uncomp_out,
                                  int out_dtype, int32_t* n_window, epa_stream_t stream) {
  const char* who = "epa_target_spectra";
  EPA_CHECK_REAL(who, in_dtype);
  EPA_CHECK_REAL_OUT(who, out_dtype);
  EPA_CHECK_ARG(C > 0 && P > 0 && S > 0 && C <= 65535 && P < 0x7fffffffLL && S < 0x7fffffffLL - 2 * kMaxH - kMaxTaps &&
                    C * P < 0x7fffffffLL,
                "%s: bad shape C=%lld P=%lld S=%lld", who, C, P, S);
  EPA_CHECK_ARG(B > 0 && B <= kMaxBeams, "%s: 1 .. %d sectors supported (got %d)", who, kMaxBeams, B);
  EPA_CHECK_ARG(half_window >= 0 && half_window <= kMaxH, "%s: half_window %d outside 0 .. %d", who, half_window, kMaxH);
  EPA_CHECK_ARG(F >= 1 && F <= kMaxF, "%s: %d frequencies outside 1 .. %d", who, F, kMaxF);
  EPA_CHECK_ARG(max_taps >= 1 && max_taps <= kMaxTaps, "%s: replicas of up to %d taps are served (max_taps %d)", who,
                kMaxTaps, max_taps);
  EPA_CHECK_ARG(n_replicas >= 1 && n_replicas <= 65535 && replica_len >= 1 && replica_len < 0x7fffffffLL,
                "%s: n_replicas=%d replica_len=%lld", who, n_replicas, replica_len);
  EPA_CHECK_ARG(replica_id || n_replicas >= C, "%s: without replica_id every channel needs its replica (%d of %lld)", who,
                n_replicas, C);
  EPA_CHECK_ARG(n_map >= 1 && N >= 0 && N < 0x7fffffffLL, "%s: n_map=%d N=%lld", who, n_map, N);
  if (N == 0) return EPA_OK;
  EPA_CHECK_ARG(re && im && replica && replica_off && rep_dt && fparams && pparams && chan_map, "%s: NULL array argument",
                who);
  EPA_CHECK_ARG(t_channel && t_ping && t_sample && t_range && t_along && t_athw, "%s: NULL table column", who);
  EPA_CHECK_ARG(table && ts_out && ts_uncomp_out && n_window, "%s: NULL output argument", who);
  Args a = {};
  a.re = re, a.im = im, a.C = C, a.P = P, a.S = S, a.B = B;
  a.replica = replica, a.replica_off = replica_off, a.replica_id = replica_id, a.R = n_replicas;
  a.replica_len = replica_len, a.max_taps = max_taps, a.rep_dt = rep_dt, a.fparams = fparams, a.F = F, a.h = half_window;
  a.pparams = pparams, a.chan_map = chan_map, a.n_map = n_map;
  a.t_channel = t_channel, a.t_ping = t_ping, a.t_sample = t_sample, a.t_range = t_range, a.t_along = t_along;
  a.t_athw = t_athw, a.N = N, a.table = table, a.ts = ts_out, a.ts_uncomp = ts_uncomp_out, a.n_window = n_window;
  const Lds l = lds_layout(max_taps, half_window);
  a.xs_off = l.xs_off, a.part_off = l.part_off, a.pc_off = l.pc_off, a.mask_off = l.mask_off;
  hipStream_t st = (hipStream_t)stream;
  {
    // (the replica, then the lags a(0 .. h) where the main kernel keeps its window)
    const size_t lds = (size_t)l.xs_off + (size_t)(half_window + 1) * sizeof(Cd);
    auto kern = epa::spectrum::replica_table_kernel<Args>;
    if (int rc = epa::allow_lds(kern, lds)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_replicas), dim3(kBlock), lds, st, a);
    if (int rc = epa::check_launch("target_spectrum_replica_kernel")) return rc;
  }
  const unsigned grid = (unsigned)(N < kMaxGrid ? N : kMaxGrid);
  return epa::dispatch_real(who, in_dtype, [&](auto in) {
    return epa::dispatch_real(who, out_dtype, [&](auto out) {
      using InT = typename decltype(in)::type;
      using OutT = typename decltype(out)::type;
      auto kern = target_spectrum_kernel<InT, OutT>;
      if (int rc = epa::allow_lds(kern, l.total)) return rc;
      hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), l.total, st, a);
      return epa::check_launch("target_spectrum_kernel");
    });
  });
}
