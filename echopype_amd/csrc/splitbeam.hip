// Split-beam angles (consolidate.add_splitbeam_angle): the alongship / athwartship angle of every sample of a Simrad
// split-beam file, from power/angle samples or from complex samples (with or without pulse compression).
//
// Reference arithmetic replaced (paths under /root/reference/echopype):
//   consolidate/split_beam_angle.py:121-171  power/angle: theta = (180/128) * angle / sensitivity - offset
//   consolidate/split_beam_angle.py:34-118   complex: the sector combinations of the channel's beam_type, two
//                                            angle(a * conj(b)) per sample, / sensitivity - offset
//   consolidate/split_beam_angle.py:208-219  BB with pulse compression: compress_pulse (ek80_complex.py:316-369) of
//                                            every sector, NaN zero-filled before and restored after, sector by sector
//
// Beam types (a per-channel table; a channel the caller marks -1 is skipped: its rows are NaN):
//   1          fore = b2 + b3, aft = b0 + b1, star = b0 + b3, port = b1 + b2;  theta = angle(fore conj(aft)),
//              phi = angle(star conj(port))
//   17         star = b0, port = b1, fore = b2                                  fac1 = angle(fore conj(star)),
//   49/65/81   star = b0 + b3, port = b1 + b3, fore = b2 + b3                   fac2 = angle(fore conj(port)),
//                                                                                theta = (fac1 + fac2) / sqrt 3,
//                                                                                phi = fac2 - fac1
// The reference halves every two-sector sum: a positive factor moves no phase, so it is left out.
//
// Pulse compression.  The matched filter is linear, so filtering a combination of the zero-filled sectors equals
// combining the filtered zero-filled sectors: the kernels filter the 3 (types 17/49/65/81) or 4 (type 1)
// combinations.  The reference restores a NaN wherever a sector was NaN at its input; every output angle involves
// every sector its beam type uses (b0..b2, and b3 unless the type is 17), so an angle is NaN exactly where one of those
// sectors is NaN at the sample itself -- a per-sample bit, known before any filtering: unlike the Sv kernels (whose
// NaN-skipping sector MEAN needs the sectors apart where only some are NaN) nothing here is redone a second time.
//   direct form  (sba_pc_direct_kernel): the tile of sv_complex_kernel (ek80_complex.hip) -- 2048 outputs per
//                workgroup, eight consecutive per lane, replica in LDS -- staged and filtered once per combination.
//   FFT form     (sba_pc_fft_kernel): the 2048-point overlap-save tile of ek80_fft.hip (lds_fft.h::correlate), one
//                forward and one inverse transform per combination: 6 transforms per tile for types 17/49/65/81 and 8
//                for type 1.  (One forward transform per sector with the combinations formed in the frequency domain
//                needs B + K: 7 for 49/65/81, 6 for 17, 8 for 1 -- never fewer, and it holds B spectra at once.)
//
// atan2: gfx950 has no instruction for it; ocml's atan2 / atan2f (range reduction by one division, a minimax
// polynomial, quadrant fix-up) is what the kernels call.  Its cost per output, counted in the ISA, is in DESIGN.md.
#include "fast_math.h"
#include "lds_fft.h"

namespace {

constexpr int kMaxChan = 64;
constexpr int kMaxSectors = 4;
enum Kind : int { kSkip = 0, kFour = 1, kThree = 2, kThreeC = 3 };

struct AngleParams {
  const double* v[4];  // sensitivity alongship, sensitivity athwartship, offset alongship, offset athwartship
  int mode[4];         // epa_param_mode: scalar, [C] or [C*P]
};

struct SbaArgs {
  const void* re;  // power form: angle_alongship; complex forms: backscatter_r (C, P, S, B)
  const void* im;  // power form: angle_athwartship; complex forms: backscatter_i
  AngleParams q;
  int C, P, S, B;
  int tiles, out_per_tile;
  const float* replica;        // interleaved (re, im) f32, direct form
  const int32_t* replica_off;  // [n_replicas + 1]
  const int32_t* replica_id;   // optional [C*P]; NULL: replica c for every ping of channel c
  const double* ws;            // FFT form: twiddles + replica spectra (ws_* below)
  void* theta;
  void* phi;
  unsigned rep_lds_off;
  int8_t kind[kMaxChan];
};

struct RowParams {
  double sa, st, oa, ot;
};

__device__ __forceinline__ double pval(const AngleParams& q, int k, int c, int p, int P) {
  const int m = q.mode[k];
  const size_t i = m == EPA_PM_SCALAR ? 0 : (m == EPA_PM_CHANNEL ? (size_t)c : (size_t)c * P + p);
  return q.v[k][i];
}
__device__ __forceinline__ RowParams row_params(const AngleParams& q, int c, int p, int P) {
  return RowParams{pval(q, 0, c, p, P), pval(q, 1, c, p, P), pval(q, 2, c, p, P), pval(q, 3, c, p, P)};
}

template <typename A>
struct AM;
template <>
struct AM<double> {
  static __device__ __forceinline__ double atan2(double y, double x) { return ::atan2(y, x); }
  static __device__ __forceinline__ double nan() { return __builtin_nan(""); }
};
template <>
struct AM<float> {
  static __device__ __forceinline__ float atan2(float y, float x) { return ::atan2f(y, x); }
  static __device__ __forceinline__ float nan() { return __builtin_nanf(""); }
};

// angle of a * conj(b) in degrees (np.arctan2(imag, real) / pi * 180)
template <typename A>
__device__ __forceinline__ A angle_deg(A ar, A ai, A br, A bi) {
  const A re = ar * br + ai * bi;
  const A im = ai * br - ar * bi;
  return AM<A>::atan2(im, re) * (A)57.295779513082320877;
}

// theta / phi from the two angles of the combinations (kind-uniform), then / sensitivity - offset
template <typename A>
__device__ __forceinline__ void finish(int kind, A a0, A a1, const RowParams& rp, A& th, A& ph) {
  A t = a0, f = a1;
  if (kind != kFour) {
    t = (a0 + a1) / (A)1.7320508075688772935;
    f = a1 - a0;
  }
  th = t / (A)rp.sa - (A)rp.oa;
  ph = f / (A)rp.st - (A)rp.ot;
}

// sectors of combination k of a kind (second = -1: a single sector); order fore, aft, star, port (type 1) or
// fore, star, port (the three-sector types)
__device__ __forceinline__ void combo_sectors(int kind, int k, int& u, int& v) {
  if (kind == kFour) {  // (2, 3) (0, 1) (0, 3) (1, 2)
    u = k == 0 ? 2 : (k == 3 ? 1 : 0);
    v = k == 0 ? 3 : (k == 1 ? 1 : (k == 2 ? 3 : 2));
  } else {  // 2, 0, 1 [+ 3]
    u = k == 0 ? 2 : k - 1;
    v = kind == kThreeC ? 3 : -1;
  }
}
__device__ __forceinline__ int n_combos(int kind) { return kind == kFour ? 4 : 3; }
__device__ __forceinline__ unsigned used_sectors(int kind) { return kind == kThree ? 0x7u : 0xfu; }

// ------------------------------------------------------------------------------------------------
// Power/angle samples: a streaming pass.  One workgroup takes 4096 samples of one (channel, ping); lane l the samples
// 4 l + 1024 i + e (e < 4, i < 4): every wavefront load is 256 B (int8) / 1 KiB (f32) contiguous per plane, every
// store 2 KiB (f64).  VEC: S % 4 == 0 and the planes aligned, so that the four samples of a lane are one vector.
// ------------------------------------------------------------------------------------------------
constexpr int kPowPiece = 4 * 4 * epa::kBlock;

template <typename InT, int N>
struct Vec {
  typedef InT type __attribute__((ext_vector_type(N)));
};

// (180 / 128) * angle in the angle's own type, as NumPy evaluates a Python float times an array: exact for the int8
// steps of a file, rounded like the reference for float32 planes
constexpr double kConv = 180.0 / 128.0;
__device__ __forceinline__ double scaled(int8_t x) { return kConv * (double)x; }
__device__ __forceinline__ double scaled(float x) { return (double)((float)kConv * x); }
__device__ __forceinline__ double scaled(double x) { return kConv * x; }

template <typename InT, typename T, bool VEC>
__global__ __launch_bounds__(epa::kBlock) void sba_power_kernel(SbaArgs a) {
  const int c = blockIdx.y;
  const int p = blockIdx.x / a.tiles, piece = blockIdx.x - p * a.tiles;
  const int S = a.S;
  const size_t row = (size_t)c * a.P + p;
  const RowParams rp = row_params(a.q, c, p, a.P);
  const InT* al = reinterpret_cast<const InT*>(a.re) + row * S;
  const InT* at = reinterpret_cast<const InT*>(a.im) + row * S;
  T* th = reinterpret_cast<T*>(a.theta) + row * S;
  T* ph = reinterpret_cast<T*>(a.phi) + row * S;
  InT va[4][4] = {}, vt[4][4] = {};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s0 = piece * kPowPiece + 1024 * i + 4 * (int)threadIdx.x;
    if (VEC) {
      if (s0 < S) {  // (S % 4 == 0: the four samples are inside together)
        const typename Vec<InT, 4>::type x = *reinterpret_cast<const typename Vec<InT, 4>::type*>(al + s0);
        const typename Vec<InT, 4>::type y = *reinterpret_cast<const typename Vec<InT, 4>::type*>(at + s0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          va[i][e] = x[e];
          vt[i][e] = y[e];
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int s = s0 + e;
        va[i][e] = s < S ? al[s] : (InT)0;
        vt[i][e] = s < S ? at[s] : (InT)0;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s0 = piece * kPowPiece + 1024 * i + 4 * (int)threadIdx.x;
    T ot[4], op[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // split_beam_angle.py:142-148, in its operation order
      ot[e] = (T)(scaled(va[i][e]) / rp.sa - rp.oa);
      op[e] = (T)(scaled(vt[i][e]) / rp.st - rp.ot);
    }
    if (VEC) {
      if (s0 < S) {
        typename Vec<T, 4>::type x, y;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x[e] = ot[e];
          y[e] = op[e];
        }
        *reinterpret_cast<typename Vec<T, 4>::type*>(th + s0) = x;
        *reinterpret_cast<typename Vec<T, 4>::type*>(ph + s0) = y;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (s0 + e < S) {
          th[s0 + e] = ot[e];
          ph[s0 + e] = op[e];
        }
      }
    }
  }
}

// NaN over samples [s_begin, s_end) of one (channel, ping) row: a skipped channel, a ping without a replica
template <typename T>
__device__ __forceinline__ void nan_fill(const SbaArgs& a, size_t row, int s_begin, int s_end) {
  T* th = reinterpret_cast<T*>(a.theta) + row * a.S;
  T* ph = reinterpret_cast<T*>(a.phi) + row * a.S;
  s_end = min(s_end, a.S);
  for (int s = s_begin + (int)threadIdx.x; s < s_end; s += epa::kBlock) {
    th[s] = AM<T>::nan();
    ph[s] = AM<T>::nan();
  }
}

// the B (<= 4) sectors of one sample; NB = 4: two 16-byte (f32) or four (f64) vector loads per plane
template <typename InT, typename A, int NB>
__device__ __forceinline__ void load_sectors(const InT* __restrict__ pr, const InT* __restrict__ pi, int B,
                                             A (&r)[kMaxSectors], A (&i)[kMaxSectors]) {
  if (NB == 4) {
    constexpr int kPer = 16 / sizeof(InT);
    typedef InT vec_t __attribute__((ext_vector_type(kPer)));
#pragma unroll
    for (int q = 0; q < 4 / kPer; ++q) {
      const vec_t tr = reinterpret_cast<const vec_t*>(pr)[q], ti = reinterpret_cast<const vec_t*>(pi)[q];
#pragma unroll
      for (int e = 0; e < kPer; ++e) {
        r[q * kPer + e] = (A)tr[e];
        i[q * kPer + e] = (A)ti[e];
      }
    }
  } else {
#pragma unroll
    for (int b = 0; b < kMaxSectors; ++b) {
      r[b] = b < B ? (A)pr[b] : (A)0;
      i[b] = b < B ? (A)pi[b] : (A)0;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Complex samples without a replica (CW; BB without pulse compression): a sample depends on its own sectors only.
// The lane layout of sv_complex_cw_kernel: lane j takes the samples j + 256 i of a 2048- (f64 planes: 1024-) sample
// piece of one ping, every wavefront load 1 KiB contiguous per plane (B = 4, f32).  A NaN sector makes its
// combinations NaN, and with them both angles: no test is needed.
// ------------------------------------------------------------------------------------------------
template <typename InT>
constexpr int cw_piece() { return sizeof(InT) == 8 ? 1024 : 2048; }

template <typename InT, typename T, int NB>
__global__ __launch_bounds__(epa::kBlock) void sba_complex_cw_kernel(SbaArgs a) {
  const int c = blockIdx.y;
  const int p = blockIdx.x / a.tiles, piece = blockIdx.x - p * a.tiles;
  const int S = a.S, B = NB > 0 ? NB : a.B;
  const size_t row = (size_t)c * a.P + p;
  constexpr int kPiece = cw_piece<InT>();
  constexpr int kPer = kPiece / epa::kBlock;
  const int kind = a.kind[c];
  if (kind == kSkip) {
    nan_fill<T>(a, row, piece * kPiece, piece * kPiece + kPiece);
    return;
  }
  const RowParams rp = row_params(a.q, c, p, a.P);
  const InT* re = reinterpret_cast<const InT*>(a.re) + row * (size_t)S * B;
  const InT* im = reinterpret_cast<const InT*>(a.im) + row * (size_t)S * B;
  T* th = reinterpret_cast<T*>(a.theta) + row * S;
  T* ph = reinterpret_cast<T*>(a.phi) + row * S;
  // all loads of the lane first (independent), then the arithmetic
  T r[kPer][kMaxSectors], i[kPer][kMaxSectors];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int s = min(piece * kPiece + (int)threadIdx.x + epa::kBlock * k, S - 1);  // (clamped: no partial arrays)
    load_sectors<InT, T, NB>(re + (size_t)s * B, im + (size_t)s * B, B, r[k], i[k]);
  }
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int s = piece * kPiece + (int)threadIdx.x + epa::kBlock * k;
    if (s >= S) break;
    const T* x = r[k];
    const T* y = i[k];
    T a0, a1;
    if (kind == kFour) {
      a0 = angle_deg<T>(x[2] + x[3], y[2] + y[3], x[0] + x[1], y[0] + y[1]);
      a1 = angle_deg<T>(x[0] + x[3], y[0] + y[3], x[1] + x[2], y[1] + y[2]);
    } else {
      const T cr = kind == kThreeC ? x[3] : (T)0, ci = kind == kThreeC ? y[3] : (T)0;
      const T fr = x[2] + cr, fi = y[2] + ci;
      a0 = angle_deg<T>(fr, fi, x[0] + cr, y[0] + ci);
      a1 = angle_deg<T>(fr, fi, x[1] + cr, y[1] + ci);
    }
    T ot, op;
    finish<T>(kind, a0, a1, rp, ot, op);
    th[s] = ot;
    ph[s] = op;
  }
}

// sector validity of sample s: all sectors the kind uses are numbers (re and im)
template <typename InT>
__device__ __forceinline__ bool sample_valid(const InT* __restrict__ pr, const InT* __restrict__ pi, unsigned used) {
  bool ok = true;
#pragma unroll
  for (int b = 0; b < kMaxSectors; ++b)
    if (used & (1u << b)) ok = ok && (pr[b] == pr[b]) && (pi[b] == pi[b]);
  return ok;
}

// combination (u [+ v]) of the zero-filled sectors of one sample
template <typename InT, typename A>
__device__ __forceinline__ void combo_value(const InT* __restrict__ pr, const InT* __restrict__ pi, int u, int v, A& cr,
                                            A& ci) {
  const InT ur = pr[u], ui = pi[u];
  const bool uok = (ur == ur) && (ui == ui);
  cr = uok ? (A)ur : (A)0;
  ci = uok ? (A)ui : (A)0;
  if (v >= 0) {
    const InT vr = pr[v], vi = pi[v];
    const bool vok = (vr == vr) && (vi == vi);
    cr += vok ? (A)vr : (A)0;
    ci += vok ? (A)vi : (A)0;
  }
}

// ------------------------------------------------------------------------------------------------
// Pulse compression, direct form: the tile of sv_complex_kernel (2048 outputs per workgroup, lane j the outputs 8 j ..
// 8 j + 7, a 16-element register window sliding over the staged tile, replica conj in the MAC) -- the tile is staged
// and filtered once per combination; the lane keeps the first combination of a pair and the angles.
// ------------------------------------------------------------------------------------------------
constexpr int kR = 8;
constexpr int kTile = epa::kBlock * kR;

template <typename A>
struct Cx {
  A re, im;
};
__device__ __forceinline__ int pad_idx(int a) { return a + (a >> 3); }

// y[i] = sum_j x[k0+i+j] * conj(rep[j]), i = 0..7 (ek80_complex.hip conv8)
template <typename A>
__device__ __forceinline__ void conv8(const Cx<A>* __restrict__ xs, const Cx<A>* __restrict__ rep, int taps, int k0,
                                      Cx<A> (&acc)[kR]) {
  Cx<A> w[2 * kR];
#pragma unroll
  for (int e = 0; e < kR; ++e) w[e] = xs[pad_idx(k0 + e)];
  for (int q = 0; q < taps; q += kR) {
#pragma unroll
    for (int e = 0; e < kR; ++e) w[kR + e] = xs[pad_idx(k0 + q + kR + e)];
#pragma unroll
    for (int jj = 0; jj < kR; ++jj) {
      const Cx<A> t = rep[q + jj];
#pragma unroll
      for (int i = 0; i < kR; ++i) {
        const Cx<A> x = w[i + jj];
        acc[i].re = fma(x.re, t.re, acc[i].re);
        acc[i].re = fma(x.im, t.im, acc[i].re);
        acc[i].im = fma(x.im, t.re, acc[i].im);
        acc[i].im = fma(-x.re, t.im, acc[i].im);
      }
    }
#pragma unroll
    for (int e = 0; e < kR; ++e) w[e] = w[kR + e];
  }
}

template <typename InT, typename T>
__global__ __launch_bounds__(epa::kBlock) void sba_pc_direct_kernel(SbaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Cx<T>* xs = reinterpret_cast<Cx<T>*>(smem);
  Cx<T>* rep = reinterpret_cast<Cx<T>*>(smem + a.rep_lds_off);
  const int c = blockIdx.y;
  const int p = blockIdx.x / a.tiles;
  const int tile = blockIdx.x - p * a.tiles;
  const int S = a.S, B = a.B;
  const int k_begin = tile * kTile;
  const size_t row = (size_t)c * a.P + p;
  const int kind = a.kind[c];
  const int rid = a.replica_id ? a.replica_id[row] : c;
  if (kind == kSkip || rid < 0) {  // (block-uniform, before any barrier)
    nan_fill<T>(a, row, k_begin, k_begin + kTile);
    return;
  }
  const InT* re = reinterpret_cast<const InT*>(a.re) + row * (size_t)S * B;
  const InT* im = reinterpret_cast<const InT*>(a.im) + row * (size_t)S * B;

  // ---- replica -> LDS, zero-padded to a multiple of 8 taps
  const int r0 = a.replica_off[rid], taps = a.replica_off[rid + 1] - r0;
  const int taps8 = (taps + kR - 1) / kR * kR;
  for (int j = threadIdx.x; j < taps8; j += epa::kBlock) {
    Cx<T> t{(T)0, (T)0};
    if (j < taps) {
      t.re = (T)a.replica[2 * (size_t)(r0 + j)];
      t.im = (T)a.replica[2 * (size_t)(r0 + j) + 1];
    }
    rep[j] = t;
  }
  const int len = kTile + taps8 + kR;  // outputs [k_begin, k_begin + kTile) read up to k_begin + kTile + taps8 - 1 (+8)
  const int k0 = threadIdx.x * kR;
  const unsigned used = used_sectors(kind);
  bool valid[kR];
#pragma unroll
  for (int i = 0; i < kR; ++i) {
    const int s = k_begin + k0 + i;
    valid[i] = s < S && sample_valid<InT>(re + (size_t)s * B, im + (size_t)s * B, used);
  }
  const int K = n_combos(kind);
  Cx<T> h[kR];
  T ang0[kR], ang1[kR];
  for (int k = 0; k < K; ++k) {
    int u, v;
    combo_sectors(kind, k, u, v);
    __syncthreads();  // (the previous combination's window reads are done; the replica is published)
    for (int t = threadIdx.x; t < len; t += epa::kBlock) {
      const int s = k_begin + t;
      Cx<T> x{(T)0, (T)0};
      if (s < S) combo_value<InT, T>(re + (size_t)s * B, im + (size_t)s * B, u, v, x.re, x.im);
      xs[pad_idx(t)] = x;
    }
    __syncthreads();
    Cx<T> y[kR];
#pragma unroll
    for (int i = 0; i < kR; ++i) y[i] = Cx<T>{(T)0, (T)0};
    conv8<T>(xs, rep, taps8, k0, y);
#pragma unroll
    for (int i = 0; i < kR; ++i) {
      if (k == 0 || (k == 2 && K == 4)) {
        h[i] = y[i];
      } else {
        const T g = angle_deg<T>(h[i].re, h[i].im, y[i].re, y[i].im);
        if (k == 1) ang0[i] = g;
        else ang1[i] = g;
      }
    }
  }
  const RowParams rp = row_params(a.q, c, p, a.P);
  T* th = reinterpret_cast<T*>(a.theta) + row * S;
  T* ph = reinterpret_cast<T*>(a.phi) + row * S;
#pragma unroll
  for (int i = 0; i < kR; ++i) {
    const int s = k_begin + k0 + i;
    if (s >= S) break;
    T ot, op;
    finish<T>(kind, ang0[i], ang1[i], rp, ot, op);
    th[s] = valid[i] ? ot : AM<T>::nan();
    ph[s] = valid[i] ? op : AM<T>::nan();
  }
}

// ------------------------------------------------------------------------------------------------
// Pulse compression, FFT form: overlap-save tiles of kN = 2048 samples, kN - max_taps + 1 outputs each; lane j owns the
// samples j + 256 i from the load to the store (lds_fft.h).  Per combination: the lane's eight combined samples
// (zero-filled), correlate() with the replica spectrum, the pair's angle.
//
// workspace (doubles): [0, 512) 256 twiddles w_2048^m as double2, [512, 768) the same as float2, then per replica
// conj(FFT(tx)) / N in the transform's digit-reversed order: 2048 double2, then 2048 float2
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline size_t sws_tw64() { return 0; }
__host__ __device__ inline size_t sws_tw32() { return 512; }
__host__ __device__ constexpr size_t sws_spec64(int r) { return 768 + (size_t)r * 3 * kN; }
__host__ __device__ inline size_t sws_spec32(int r) { return sws_spec64(r) + 2 * kN; }

__global__ __launch_bounds__(epa::kBlock) void sba_replica_spectrum_kernel(const float* __restrict__ replica,
                                                                           const int32_t* __restrict__ off,
                                                                           double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned char xs[Xs<double>::kBytes];
  __shared__ C2<double> tw[256];
  const int r = blockIdx.x, j = threadIdx.x;
  {
    double sn, cs;
    sincospi(-2.0 * (double)j / (double)kN, &sn, &cs);
    tw[j] = C2<double>{cs, sn};
    if (r == 0) {
      reinterpret_cast<C2<double>*>(ws + sws_tw64())[j] = tw[j];
      reinterpret_cast<C2<float>*>(ws + sws_tw32())[j] = C2<float>{(float)cs, (float)sn};
    }
  }
  __syncthreads();
  const int r0 = off[r], taps = min(off[r + 1] - r0, kN);
  C2<double> v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = j + 256 * i;
    C2<double> t{0.0, 0.0};
    if (n < taps) {
      t.re = (double)replica[2 * (size_t)(r0 + n)];
      t.im = (double)replica[2 * (size_t)(r0 + n) + 1];
    }
    v[i] = t;
  }
  const LaneMap lm = lane_map();
  fwd_pass0<double>(v, tw[j]);
#pragma unroll
  for (int i = 0; i < 8; ++i) Xs<double>::st(xs, j + 256 * i, v[i]);
  __syncthreads();
  ld8<double, 64>(xs, lm.a1, v);
  dft8(v);
  twiddle8<double, false>(v, tw[lm.t1]);
  st8<double, 64>(xs, lm.a1, v);
  __builtin_amdgcn_wave_barrier();
  ld8<double, 8>(xs, lm.a2, v);
  dft8(v);
  twiddle8<double, false>(v, tw[lm.t2]);
  st8<double, 8>(xs, lm.a2, v);
  __builtin_amdgcn_wave_barrier();
  ld8<double, 1>(xs, lm.a3, v);
  dft8(v);
  C2<double>* s64 = reinterpret_cast<C2<double>*>(ws + sws_spec64(r));
  C2<float>* s32 = reinterpret_cast<C2<float>*>(ws + sws_spec32(r));
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const C2<double> z{v[q].re * (1.0 / kN), -v[q].im * (1.0 / kN)};
    s64[lm.a3 + q] = z;
    s32[lm.a3 + q] = C2<float>{(float)z.re, (float)z.im};
  }
}

template <typename InT, typename T, typename F>
__global__ __launch_bounds__(epa::kBlock) void sba_pc_fft_kernel(SbaArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char xs[Xs<F>::kBytes];
  __shared__ C2<F> tw[kTwEntries<F>];
  const int j = threadIdx.x;
  const int c = blockIdx.y;
  const int p = blockIdx.x / a.tiles;
  const int tile = blockIdx.x - p * a.tiles;
  const int S = a.S, B = a.B;
  const int k_begin = tile * a.out_per_tile;
  const size_t row = (size_t)c * a.P + p;
  const int kind = a.kind[c];
  const int rid = a.replica_id ? a.replica_id[row] : c;
  if (kind == kSkip || rid < 0) {  // (block-uniform, before any barrier)
    nan_fill<T>(a, row, k_begin, k_begin + a.out_per_tile);
    return;
  }
  // twiddles L2 -> LDS (published by correlate()'s first barrier)
  const C2<F>* wtab = reinterpret_cast<const C2<F>*>(a.ws + (sizeof(F) == 4 ? sws_tw32() : sws_tw64()));
  if (!kSmallTw<F>) tw[j] = wtab[j];
  else if (j < 68) tw[j] = j < 64 ? wtab[4 * j] : wtab[j - 64];
  const C2<F> w_lane = wtab[j];
  const C2<F>* spec = reinterpret_cast<const C2<F>*>(a.ws + (sizeof(F) == 4 ? sws_spec32(rid) : sws_spec64(rid)));
  const LaneMap lm = lane_map();
  const InT* re = reinterpret_cast<const InT*>(a.re) + row * (size_t)S * B;
  const InT* im = reinterpret_cast<const InT*>(a.im) + row * (size_t)S * B;
  const unsigned used = used_sectors(kind);
  bool valid[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int s = k_begin + j + 256 * i;
    valid[i] = s < S && sample_valid<InT>(re + (size_t)s * B, im + (size_t)s * B, used);
  }
  const int K = n_combos(kind);
  C2<F> h[8];
  T ang0[8], ang1[8];
  for (int k = 0; k < K; ++k) {
    int u, v;
    combo_sectors(kind, k, u, v);
    C2<F> y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int s = k_begin + j + 256 * i;
      y[i] = C2<F>{(F)0, (F)0};
      if (s < S) combo_value<InT, F>(re + (size_t)s * B, im + (size_t)s * B, u, v, y[i].re, y[i].im);
    }
    correlate<F>(y, xs, tw, spec, lm, w_lane);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (k == 0 || (k == 2 && K == 4)) {
        h[i] = y[i];
      } else {
        const T g = angle_deg<T>((T)h[i].re, (T)h[i].im, (T)y[i].re, (T)y[i].im);
        if (k == 1) ang0[i] = g;
        else ang1[i] = g;
      }
    }
  }
  const RowParams rp = row_params(a.q, c, p, a.P);
  T* th = reinterpret_cast<T*>(a.theta) + row * S;
  T* ph = reinterpret_cast<T*>(a.phi) + row * S;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int t = j + 256 * i;
    const int s = k_begin + t;
    if (t < a.out_per_tile && s < S) {
      T ot, op;
      finish<T>(kind, ang0[i], ang1[i], rp, ot, op);
      th[s] = valid[i] ? ot : AM<T>::nan();
      ph[s] = valid[i] ? op : AM<T>::nan();
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------

int set_params(SbaArgs& a, const double* const* params, const int* modes, const char* who) {
  EPA_CHECK_ARG(params && modes, "%s: NULL params / modes", who);
  for (int k = 0; k < 4; ++k) {
    EPA_CHECK_ARG(params[k], "%s: NULL angle parameter %d", who, k);
    EPA_CHECK_ARG(modes[k] == EPA_PM_SCALAR || modes[k] == EPA_PM_CHANNEL || modes[k] == EPA_PM_CHANNEL_PING,
                  "%s: bad mode %d of angle parameter %d", who, modes[k], k);
    a.q.v[k] = params[k];
    a.q.mode[k] = modes[k];
  }
  return EPA_OK;
}

int set_kinds(SbaArgs& a, const int32_t* beam_type_host, int C, int B, const char* who) {
  EPA_CHECK_ARG(beam_type_host, "%s: NULL beam_type_host", who);
  EPA_CHECK_ARG(C <= kMaxChan, "%s: at most %d channels per call (got %d)", who, kMaxChan, C);
  EPA_CHECK_ARG(B == 3 || B == 4, "%s: split-beam samples have 3 or 4 sectors (got B=%d)", who, B);
  for (int c = 0; c < C; ++c) {
    const int bt = beam_type_host[c];
    int k;
    switch (bt) {
      case -1: k = kSkip; break;
      case 1: k = kFour; break;
      case 17: k = kThree; break;
      case 49: case 65: case 81: k = kThreeC; break;
      default:
        epa::set_error("%s: beam_type %d of channel %d is not 1, 17, 49, 65, 81 (or -1: skip)", who, bt, c);
        return EPA_EINVAL;
    }
    EPA_CHECK_ARG(k == kSkip || k == kThree || B == 4, "%s: beam_type %d needs 4 sectors (got B=%d)", who, bt, B);
    a.kind[c] = (int8_t)k;
  }
  for (int c = C; c < kMaxChan; ++c) a.kind[c] = (int8_t)kSkip;
  return EPA_OK;
}

template <typename InT, typename T>
int launch_power(SbaArgs& a, hipStream_t st) {
  a.tiles = (a.S + kPowPiece - 1) / kPowPiece;
  const dim3 grid((unsigned)((long long)a.P * a.tiles), (unsigned)a.C);
  const bool vec = a.S % 4 == 0 && (reinterpret_cast<uintptr_t>(a.re) % (4 * sizeof(InT))) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.im) % (4 * sizeof(InT))) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.theta) % (4 * sizeof(T))) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.phi) % (4 * sizeof(T))) == 0;
  if (vec) hipLaunchKernelGGL((sba_power_kernel<InT, T, true>), grid, dim3(epa::kBlock), 0, st, a);
  else hipLaunchKernelGGL((sba_power_kernel<InT, T, false>), grid, dim3(epa::kBlock), 0, st, a);
  return epa::check_launch("sba_power_kernel");
}

template <typename InT, typename T>
int launch_cw(SbaArgs& a, hipStream_t st) {
  a.tiles = (a.S + cw_piece<InT>() - 1) / cw_piece<InT>();
  const dim3 grid((unsigned)((long long)a.P * a.tiles), (unsigned)a.C);
  const bool b4 = a.B == 4 && (reinterpret_cast<uintptr_t>(a.re) & 15u) == 0 &&
                  (reinterpret_cast<uintptr_t>(a.im) & 15u) == 0;
  if (b4) hipLaunchKernelGGL((sba_complex_cw_kernel<InT, T, 4>), grid, dim3(epa::kBlock), 0, st, a);
  else hipLaunchKernelGGL((sba_complex_cw_kernel<InT, T, 0>), grid, dim3(epa::kBlock), 0, st, a);
  return epa::check_launch("sba_complex_cw_kernel");
}

template <typename InT, typename T>
int launch_direct(SbaArgs& a, int max_taps, hipStream_t st) {
  const int taps8 = (max_taps + kR - 1) / kR * kR;
  const int len = kTile + taps8 + kR;
  const size_t xs_bytes = ((size_t)(len + (len >> 3) + 1) * sizeof(Cx<T>) + 15) & ~(size_t)15;
  const size_t rep_bytes = (size_t)taps8 * sizeof(Cx<T>);
  const size_t lds = xs_bytes + rep_bytes;
  EPA_CHECK_ARG(lds <= 150 * 1024, "epa_splitbeam_complex: replica of %d taps does not fit the LDS tile", max_taps);
  a.rep_lds_off = (unsigned)xs_bytes;
  a.tiles = (a.S + kTile - 1) / kTile;
  const dim3 grid((unsigned)((long long)a.P * a.tiles), (unsigned)a.C);
  auto kern = sba_pc_direct_kernel<InT, T>;
  if (int rc = epa::allow_lds(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, grid, dim3(epa::kBlock), lds, st, a);
  return epa::check_launch("sba_pc_direct_kernel");
}

template <typename InT, typename T, typename F>
int launch_fft(SbaArgs& a, const float* replica, const int32_t* replica_off, int n_rep, int max_taps, double* ws,
               hipStream_t st) {
  hipLaunchKernelGGL(sba_replica_spectrum_kernel, dim3((unsigned)n_rep), dim3(epa::kBlock), 0, st, replica, replica_off,
                     ws);
  if (int rc = epa::check_launch("sba_replica_spectrum_kernel")) return rc;
  a.ws = ws;
  a.out_per_tile = kN - max_taps + 1;
  a.tiles = (a.S + a.out_per_tile - 1) / a.out_per_tile;
  const dim3 grid((unsigned)((long long)a.P * a.tiles), (unsigned)a.C);
  hipLaunchKernelGGL((sba_pc_fft_kernel<InT, T, F>), grid, dim3(epa::kBlock), 0, st, a);
  return epa::check_launch("sba_pc_fft_kernel");
}

int complex_common(SbaArgs& a, const void* re, const void* im, int in_dtype, const int32_t* beam_type_host,
                   const double* const* params, const int* modes, const float* replica, const int32_t* replica_off,
                   const int32_t* replica_id, int n_replicas, int max_taps, int C, int P, int S, int B, void* theta,
                   void* phi, int out_dtype, const char* who) {
  EPA_CHECK_ARG(re && im && theta && phi, "%s: NULL array argument", who);
  EPA_CHECK_ARG(C > 0 && P > 0 && S > 0, "%s: C=%d P=%d S=%d", who, C, P, S);
  EPA_CHECK_ARG(epa::is_real(in_dtype), "%s: bad input dtype %d", who, in_dtype);
  EPA_CHECK_REAL_OUT(who, out_dtype);
  EPA_CHECK_ARG((replica == nullptr) == (replica_off == nullptr),
                "%s: replica and replica_off must both be given (pulse compression) or both NULL", who);
  EPA_CHECK_ARG(!replica || max_taps > 0, "%s: max_taps must be positive with a replica", who);
  EPA_CHECK_ARG(!replica_id || (replica && n_replicas > 0), "%s: replica_id needs a replica and n_replicas > 0", who);
  if (int rc = set_kinds(a, beam_type_host, C, B, who)) return rc;
  if (int rc = set_params(a, params, modes, who)) return rc;
  a.re = re; a.im = im; a.C = C; a.P = P; a.S = S; a.B = B;
  a.replica = replica; a.replica_off = replica_off; a.replica_id = replica_id;
  a.theta = theta; a.phi = phi;
  return EPA_OK;
}

}  // namespace

extern "C" int epa_splitbeam_power(const void* along, const void* athw, int in_dtype, const double* const* params_host,
                                   const int* modes_host, int C, int P, int S, void* theta, void* phi, int out_dtype,
                                   epa_stream_t stream) {
  const char* who = "epa_splitbeam_power";
  EPA_CHECK_ARG(along && athw && theta && phi, "%s: NULL array argument", who);
  EPA_CHECK_ARG(C > 0 && P > 0 && S > 0, "%s: C=%d P=%d S=%d", who, C, P, S);
  SbaArgs a{};
  if (int rc = set_params(a, params_host, modes_host, who)) return rc;
  a.re = along; a.im = athw; a.C = C; a.P = P; a.S = S; a.B = 1;
  a.theta = theta; a.phi = phi;
  hipStream_t st = (hipStream_t)stream;
  EPA_CHECK_REAL_OUT(who, out_dtype);
  return epa::dispatch_real(who, out_dtype, [&](auto out) -> int {
    using T = typename decltype(out)::type;
    if (in_dtype == EPA_I8) return launch_power<int8_t, T>(a, st);
    if (in_dtype == EPA_F32) return launch_power<float, T>(a, st);
    if (in_dtype == EPA_F64) return launch_power<double, T>(a, st);
    epa::set_error("%s: bad input dtype %d", who, in_dtype);
    return EPA_EINVAL;
  });
}

extern "C" int epa_splitbeam_complex(const void* re, const void* im, int in_dtype, const int32_t* beam_type_host,
                                     const double* const* params_host, const int* modes_host, const float* replica,
                                     const int32_t* replica_off, const int32_t* replica_id, int n_replicas, int max_taps,
                                     int C, int P, int S, int B, void* theta, void* phi, int out_dtype,
                                     epa_stream_t stream) {
  const char* who = "epa_splitbeam_complex";
  SbaArgs a{};
  if (int rc = complex_common(a, re, im, in_dtype, beam_type_host, params_host, modes_host, replica, replica_off,
                              replica_id, n_replicas, max_taps, C, P, S, B, theta, phi, out_dtype, who))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  return epa::dispatch_real(who, in_dtype, [&](auto in) {
    return epa::dispatch_real(who, out_dtype, [&](auto out) {
      using InT = typename decltype(in)::type;
      using T = typename decltype(out)::type;
      if (!replica) return launch_cw<InT, T>(a, st);
      return launch_direct<InT, T>(a, max_taps, st);
    });
  });
}

// twiddles, then the spectra of n replicas: where the spectrum of replica n would begin
size_t epa::scratch::splitbeam_complex_fft_workspace(long long n, long long, long long) {
  static_assert(sws_spec64(3) == EPA_SPLITBEAM_FFT_WS_DOUBLES(3), "header macro and workspace layout");
  return sizeof(double) * sws_spec64((int)n);
}

extern "C" int epa_splitbeam_complex_fft(const void* re, const void* im, int in_dtype, const int32_t* beam_type_host,
                                         const double* const* params_host, const int* modes_host, const float* replica,
                                         const int32_t* replica_off, const int32_t* replica_id, int n_replicas,
                                         int max_taps, int C, int P, int S, int B, void* theta, void* phi, int out_dtype,
                                         int fft_dtype, double* workspace, epa_stream_t stream) {
  const char* who = "epa_splitbeam_complex_fft";
  EPA_CHECK_ARG(replica && replica_off && workspace, "%s: replica, replica_off and workspace are needed", who);
  EPA_CHECK_ARG(max_taps >= 1 && max_taps <= kN / 2, "%s: the FFT form takes replicas of 1 .. %d taps (got %d)", who,
                kN / 2, max_taps);
  EPA_CHECK_ARG(epa::is_real(fft_dtype), "%s: bad fft_dtype %d", who, fft_dtype);
  SbaArgs a{};
  if (int rc = complex_common(a, re, im, in_dtype, beam_type_host, params_host, modes_host, replica, replica_off,
                              replica_id, n_replicas, max_taps, C, P, S, B, theta, phi, out_dtype, who))
    return rc;
  const int n_rep = replica_id ? n_replicas : C;
  hipStream_t st = (hipStream_t)stream;
  return epa::dispatch_real(who, in_dtype, [&](auto in) {
    return epa::dispatch_real(who, out_dtype, [&](auto out) {
      return epa::dispatch_real(who, fft_dtype, [&](auto fft) {
        return launch_fft<typename decltype(in)::type, typename decltype(out)::type, typename decltype(fft)::type>(
            a, replica, replica_off, n_rep, max_taps, workspace, st);
      });
    });
  });
}
