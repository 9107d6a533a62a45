// The LDS-resident 2048-point transform of the EK80 pulse-compression kernels, shared by ek80_fft.hip (Sv / TS) and
// splitbeam.hip (split-beam angles): radix-4.8.8.8 decimation in frequency in place, its transposed inverse, and
// correlate() -- the circular correlation of one tile held as v[i] = x[j + 256 i] with a replica spectrum.  The design
// notes are in the header comment of ek80_fft.hip.
#pragma once
#include "fast_math.h"

namespace {

constexpr int kN = EPA_EK80_NFFT;
constexpr int kPlane = kN + kN / 8;  // padded element count
static_assert(kN == 2048 && epa::kBlock == 256, "written for N = 2048, 256 lanes");

template <typename F>
struct C2 {
  F re, im;
};

// One pad element per 8: with the lane <-> butterfly maps below the stride-8 and stride-1 passes of a wavefront are
// free of bank conflicts (slot = element + element / 8 mod 32: 8 g + 9 r + o resp. 9 lane + r over the 32 lanes of a
// read group), the stride-64 pass and the lane's own samples collide two-fold on 3 of 32 slots.
__device__ __forceinline__ int pad(int a) { return a + (a >> 3); }

// ---- LDS element access: float2 elements / separate double planes (8-byte accesses either way)
template <typename F>
struct Xs;
template <>
struct Xs<float> {
  static constexpr size_t kBytes = (size_t)kPlane * 8;
  static __device__ __forceinline__ C2<float> ld(const unsigned char* xs, int a) {
    const float2 v = reinterpret_cast<const float2*>(xs)[pad(a)];
    return C2<float>{v.x, v.y};
  }
  static __device__ __forceinline__ void st(unsigned char* xs, int a, C2<float> v) {
    reinterpret_cast<float2*>(xs)[pad(a)] = make_float2(v.re, v.im);
  }
};
template <>
struct Xs<double> {
  static constexpr size_t kBytes = (size_t)kPlane * 16;
  static __device__ __forceinline__ C2<double> ld(const unsigned char* xs, int a) {
    const double* p = reinterpret_cast<const double*>(xs);
    return C2<double>{p[pad(a)], p[kPlane + pad(a)]};
  }
  static __device__ __forceinline__ void st(unsigned char* xs, int a, C2<double> v) {
    double* p = reinterpret_cast<double*>(xs);
    p[pad(a)] = v.re;
    p[kPlane + pad(a)] = v.im;
  }
};

template <typename F>
__device__ __forceinline__ C2<F> cmul(C2<F> a, C2<F> b) {
  return C2<F>{fma(a.re, b.re, -a.im * b.im), fma(a.re, b.im, a.im * b.re)};
}
template <typename F>
__device__ __forceinline__ C2<F> cmulc(C2<F> a, C2<F> b) {  // a * conj(b)
  return C2<F>{fma(a.re, b.re, a.im * b.im), fma(a.im, b.re, -a.re * b.im)};
}
template <typename F>
__device__ __forceinline__ C2<F> cadd(C2<F> a, C2<F> b) { return C2<F>{a.re + b.re, a.im + b.im}; }
template <typename F>
__device__ __forceinline__ C2<F> csub(C2<F> a, C2<F> b) { return C2<F>{a.re - b.re, a.im - b.im}; }
template <typename F>
__device__ __forceinline__ C2<F> mul_mi(C2<F> a) { return C2<F>{a.im, -a.re}; }  // * (-i)
template <typename F>
__device__ __forceinline__ C2<F> cswap(C2<F> a) { return C2<F>{a.im, a.re}; }

// forward 4-point DFT (e^{-2 pi i rq/4}), in place
template <typename F>
__device__ __forceinline__ void dft4(C2<F>& u0, C2<F>& u1, C2<F>& u2, C2<F>& u3) {
  const C2<F> s02 = cadd(u0, u2), d02 = csub(u0, u2), s13 = cadd(u1, u3), d13 = mul_mi(csub(u1, u3));
  u0 = cadd(s02, s13);
  u2 = csub(s02, s13);
  u1 = cadd(d02, d13);
  u3 = csub(d02, d13);
}
template <typename F>
__device__ __forceinline__ void dft8(C2<F> (&v)[8]) {
  const F kH = (F)0.70710678118654752440;
  C2<F> e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6], o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
  dft4(e0, e1, e2, e3);
  dft4(o0, o1, o2, o3);
  const C2<F> t1 = C2<F>{(o1.re + o1.im) * kH, (o1.im - o1.re) * kH};   // * e^{-i pi/4}
  const C2<F> t2 = mul_mi(o2);                                           // * e^{-i pi/2}
  const C2<F> t3 = C2<F>{(o3.im - o3.re) * kH, -(o3.re + o3.im) * kH};  // * e^{-3i pi/4}
  v[0] = cadd(e0, o0); v[4] = csub(e0, o0);
  v[1] = cadd(e1, t1); v[5] = csub(e1, t1);
  v[2] = cadd(e2, t2); v[6] = csub(e2, t2);
  v[3] = cadd(e3, t3); v[7] = csub(e3, t3);
}
// the conjugate transforms through swap(DFT(swap(.))): the swaps are register renames
template <typename F>
__device__ __forceinline__ void idft4(C2<F>& u0, C2<F>& u1, C2<F>& u2, C2<F>& u3) {
  u0 = cswap(u0); u1 = cswap(u1); u2 = cswap(u2); u3 = cswap(u3);
  dft4(u0, u1, u2, u3);
  u0 = cswap(u0); u1 = cswap(u1); u2 = cswap(u2); u3 = cswap(u3);
}
template <typename F>
__device__ __forceinline__ void idft8(C2<F> (&v)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = cswap(v[r]);
  dft8(v);
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = cswap(v[r]);
}

// v[q] *= w^q (CONJ: conj(w)^q), q = 1..7, powers by a depth-3 product tree
template <typename F, bool CONJ>
__device__ __forceinline__ void twiddle8(C2<F> (&v)[8], C2<F> w1) {
  if (CONJ) w1.im = -w1.im;
  const C2<F> w2 = cmul(w1, w1), w3 = cmul(w2, w1), w4 = cmul(w2, w2);
  v[1] = cmul(v[1], w1);
  v[2] = cmul(v[2], w2);
  v[3] = cmul(v[3], w3);
  v[4] = cmul(v[4], w4);
  v[5] = cmul(v[5], cmul(w4, w1));
  v[6] = cmul(v[6], cmul(w3, w3));
  v[7] = cmul(v[7], cmul(w4, w3));
}
template <typename F, bool CONJ>
__device__ __forceinline__ void twiddle4(C2<F>& u1, C2<F>& u2, C2<F>& u3, C2<F> w1) {
  if (CONJ) w1.im = -w1.im;
  const C2<F> w2 = cmul(w1, w1);
  u1 = cmul(u1, w1);
  u2 = cmul(u2, w2);
  u3 = cmul(u3, cmul(w2, w1));
}

// lane <-> butterfly maps (element index of r = 0 and the element stride); see the header comment
struct LaneMap {
  int a1, a2, a3;  // first element of the lane's butterfly in the stride-64, stride-8 and stride-1 passes
  int t1, t2;      // twiddle table index (w_2048^t) of those butterflies' offset
};
__device__ __forceinline__ LaneMap lane_map() {
  const int j = threadIdx.x;
  LaneMap m;
  // After the first pass the transform is four independent 512-point transforms, elements [512 w, 512 w + 512): a
  // wavefront holds exactly one of them (64 lanes x 8 elements), so its three inner passes -- and their inverses --
  // exchange data among its OWN lanes only: no workgroup barrier between them (LDS serves a wavefront's requests in
  // order), two barriers per tile instead of seven.
  const int w = j >> 6, l = j & 63;
  m.a1 = 512 * w + l;
  m.t1 = 4 * l;
  m.a2 = 512 * w + 64 * (l >> 3) + (l & 7);
  m.t2 = 32 * (l & 7);
  m.a3 = 512 * w + 8 * l;
  return m;
}

// The twiddle table w_2048^m, m < 256.  The double-precision tile leaves no room for all 256 entries next to its
// padded planes (4 workgroups per CU = 40 960 B each): SMALL keeps w^(4k), k < 64, and w^0..w^3 -- every index of
// the inner passes is a multiple of 4, the first pass pays one complex product.
template <typename F, bool SMALL>
__device__ __forceinline__ C2<F> tw_any(const C2<F>* tw, int m) {
  if (!SMALL) return tw[m];
  return cmul(tw[m >> 2], tw[64 + (m & 3)]);
}
template <typename F, bool SMALL>
__device__ __forceinline__ C2<F> tw_mul4(const C2<F>* tw, int t) {  // t % 4 == 0
  return SMALL ? tw[t >> 2] : tw[t];
}
template <typename F>
constexpr bool kSmallTw = sizeof(F) == 8;
template <typename F>
constexpr int kTwEntries = kSmallTw<F> ? 68 : 256;

// first forward pass (sub-size 2048, radix 4, two butterflies per lane), on the lane's registers:
// v[i] = sample j + 256 i.  tw = 256-entry table of w_2048^m.
// wa = w_2048^j comes from the caller (read from the full table in global memory next to the lane's samples): the
// LDS copy of the table is only published by correlate()'s first barrier, which lies behind this pass.
template <typename F>
__device__ __forceinline__ void fwd_pass0(C2<F> (&v)[8], C2<F> wa) {
  const F kH = (F)0.70710678118654752440;
  const C2<F> wb = C2<F>{(wa.re + wa.im) * kH, (wa.im - wa.re) * kH};  // w^(j+256) = w^j e^{-i pi/4}
  dft4(v[0], v[2], v[4], v[6]);
  twiddle4<F, false>(v[2], v[4], v[6], wa);
  dft4(v[1], v[3], v[5], v[7]);
  twiddle4<F, false>(v[3], v[5], v[7], wb);
}
template <typename F, bool SMALL>
__device__ __forceinline__ void inv_pass0(C2<F> (&v)[8], const C2<F>* tw) {
  const C2<F> wa = tw_any<F, SMALL>(tw, threadIdx.x);
  const F kH = (F)0.70710678118654752440;
  const C2<F> wb = C2<F>{(wa.re + wa.im) * kH, (wa.im - wa.re) * kH};
  twiddle4<F, true>(v[2], v[4], v[6], wa);
  idft4(v[0], v[2], v[4], v[6]);
  twiddle4<F, true>(v[3], v[5], v[7], wb);
  idft4(v[1], v[3], v[5], v[7]);
}

template <typename F, int STRIDE>
__device__ __forceinline__ void ld8(const unsigned char* xs, int a0, C2<F> (&v)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = Xs<F>::ld(xs, a0 + STRIDE * r);
}
template <typename F, int STRIDE>
__device__ __forceinline__ void st8(unsigned char* xs, int a0, const C2<F> (&v)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) Xs<F>::st(xs, a0 + STRIDE * r, v[r]);
}

// ---- experiment (25), compile-time EPA_FFT_XPOSE (bit 0: stride-64 <-> stride-8, bit 1: stride-8 <-> stride-1): the
// wave-local exchanges between two passes as register transposes across lanes instead of an LDS round trip.  With lane
// l = 8 a + b the stride-64 pass holds element l + 64 r in register r, the stride-8 pass element 64 a + b + 8 r, the
// stride-1 pass element 8 l + r: going from one to the next transposes the register index with the lane's bits 3..5
// (a) resp. 0..2 (b) -- three exchange stages each, a 32-bit word at a time: v_permlane32_swap / v_permlane16_swap
// (gfx950) for lane distances 32 and 16, DPP moves for 8, 4 (row_half_mirror then quad_perm), 2 and 1.
#ifndef EPA_FFT_XPOSE
#define EPA_FFT_XPOSE 0
#endif
namespace xp {
template <int CTRL>
__device__ __forceinline__ unsigned dpp(unsigned x) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}
// exchange word a of the lanes with `hi` set against word b of their partner (lane ^ distance) without it
template <int DIST>
__device__ __forceinline__ void exch(unsigned& a, unsigned& b, bool hi) {
  if (DIST == 32) {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);  // a of lanes 32..63 <-> b of lanes 0..31
    a = r[0];
    b = r[1];
  } else if (DIST == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);  // a of the odd rows <-> b of the even rows
    a = r[0];
    b = r[1];
  } else {
    const unsigned y = hi ? a : b;
    unsigned t;
    if (DIST == 8) t = dpp<0x128>(y);                 // row_ror:8
    else if (DIST == 4) t = dpp<0x1B>(dpp<0x141>(y));  // row_half_mirror (l ^ 7), then quad_perm [3,2,1,0] (l ^ 3)
    else if (DIST == 2) t = dpp<0x4E>(y);             // quad_perm [2,3,0,1]
    else t = dpp<0xB1>(y);                            // quad_perm [1,0,3,2]
    a = hi ? t : a;
    b = hi ? b : t;
  }
}
// transpose the register index of an 8-element lane set with three lane bits (LB = the lowest of them: 3 or 0)
template <int LB, int WORDS>
__device__ __forceinline__ void transpose(unsigned (&w)[8][WORDS]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int bit = 2; bit >= 0; --bit) {
    const bool hi = ((lane >> (LB + bit)) & 1) != 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (r & (1 << bit)) continue;
#pragma unroll
      for (int k = 0; k < WORDS; ++k) {
        if (LB + bit == 5) exch<32>(w[r][k], w[r | (1 << bit)][k], hi);
        else if (LB + bit == 4) exch<16>(w[r][k], w[r | (1 << bit)][k], hi);
        else if (LB + bit == 3) exch<8>(w[r][k], w[r | (1 << bit)][k], hi);
        else if (LB + bit == 2) exch<4>(w[r][k], w[r | (1 << bit)][k], hi);
        else if (LB + bit == 1) exch<2>(w[r][k], w[r | (1 << bit)][k], hi);
        else exch<1>(w[r][k], w[r | (1 << bit)][k], hi);
      }
    }
  }
}
template <int LB, typename V>
__device__ __forceinline__ void transpose_vals(V (&v)[8]) {
  constexpr int WORDS = sizeof(V) / 4;
  unsigned w[8][WORDS];
#pragma unroll
  for (int r = 0; r < 8; ++r) __builtin_memcpy(w[r], &v[r], sizeof(V));
  transpose<LB, WORDS>(w);
#pragma unroll
  for (int r = 0; r < 8; ++r) __builtin_memcpy(&v[r], w[r], sizeof(V));
}
}  // namespace xp

// Circular correlation of the tile held as v[i] = x[j + 256 i] with the channel's replica (spectrum `spec` in
// the digit-reversed order of the forward transform, conj and 1/N applied).  Result in v, same ownership.
// Barriers: the caller guarantees nobody still reads xs on entry; on exit xs holds nothing of value.
template <typename F>
__device__ __forceinline__ void correlate(C2<F> (&v)[8], unsigned char* xs, const C2<F>* tw,
                                          const C2<F>* __restrict__ spec, const LaneMap& lm, C2<F> w_lane) {
  const int j = threadIdx.x;
  constexpr bool SMALL = kSmallTw<F>;
  fwd_pass0<F>(v, w_lane);
#pragma unroll
  for (int i = 0; i < 8; ++i) Xs<F>::st(xs, j + 256 * i, v[i]);
  __syncthreads();
  ld8<F, 64>(xs, lm.a1, v);
  dft8(v);
  twiddle8<F, false>(v, tw_mul4<F, SMALL>(tw, lm.t1));
  if (EPA_FFT_XPOSE & 1) {
    xp::transpose_vals<3>(v);
  } else {
    st8<F, 64>(xs, lm.a1, v);
    __builtin_amdgcn_wave_barrier();  // (own wavefront's data: ordering for the compiler only)
    ld8<F, 8>(xs, lm.a2, v);
  }
  // the replica spectrum of the fused pass: 8 consecutive elements per lane, requested before the barrier
  C2<F> sp[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) sp[r] = spec[lm.a3 + r];
  dft8(v);
  twiddle8<F, false>(v, tw_mul4<F, SMALL>(tw, lm.t2));
  if (EPA_FFT_XPOSE & 2) {
    xp::transpose_vals<0>(v);
  } else {
    st8<F, 8>(xs, lm.a2, v);
    __builtin_amdgcn_wave_barrier();  // (own wavefront's data: ordering for the compiler only)
    ld8<F, 1>(xs, lm.a3, v);
  }
  dft8(v);
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = cmul(v[r], sp[r]);
  idft8(v);
  if (EPA_FFT_XPOSE & 2) {
    xp::transpose_vals<0>(v);
  } else {
    st8<F, 1>(xs, lm.a3, v);
    __builtin_amdgcn_wave_barrier();  // (own wavefront's data: ordering for the compiler only)
    ld8<F, 8>(xs, lm.a2, v);
  }
  twiddle8<F, true>(v, tw_mul4<F, SMALL>(tw, lm.t2));
  idft8(v);
  if (EPA_FFT_XPOSE & 1) {
    xp::transpose_vals<3>(v);
  } else {
    st8<F, 8>(xs, lm.a2, v);
    __builtin_amdgcn_wave_barrier();  // (own wavefront's data: ordering for the compiler only)
    ld8<F, 64>(xs, lm.a1, v);
  }
  twiddle8<F, true>(v, tw_mul4<F, SMALL>(tw, lm.t1));
  idft8(v);
  st8<F, 64>(xs, lm.a1, v);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = Xs<F>::ld(xs, j + 256 * i);
  inv_pass0<F, SMALL>(v, tw);
}

// ---- complex64: the same transform on (re, im) register pairs with the packed-f32 instructions of gfx950.
// Left to the vectoriser, the scalar C2<float> code above becomes v_pk_* instructions glued together with moves and
// sign flips (189 v_mov / v_pk_mov and 35 v_xor in a 703-instruction transform): the operand modifiers of VOP3P --
// op_sel / op_sel_hi pick which half of a source feeds the low / high lane, neg_lo / neg_hi negate it -- do the
// swaps and negations of complex arithmetic for free, but the compiler does not use them for f32 pairs.  Written out:
// one instruction per complex add (also with a factor of -i or +i on the second operand), two per complex product,
// 26 per radix-8 butterfly.  Same operations in the same order as the scalar templates (products then fused
// multiply-adds, the 1/sqrt2 rotations fused into the following sum).
namespace pk {
typedef float f2 __attribute__((ext_vector_type(2)));
#define EPA_PK2(name, text)                                              \
  __device__ __forceinline__ f2 name(f2 a, f2 b) {                       \
    f2 r;                                                                \
    asm(text : "=v"(r) : "v"(a), "v"(b));                                \
    return r;                                                            \
  }
#define EPA_PK3(name, text)                                              \
  __device__ __forceinline__ f2 name(f2 a, f2 b, f2 c) {                 \
    f2 r;                                                                \
    asm(text : "=v"(r) : "v"(a), "v"(b), "v"(c));                        \
    return r;                                                            \
  }
EPA_PK2(add, "v_pk_add_f32 %0, %1, %2")
EPA_PK2(sub, "v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]")
// a + (-i) b = (a.re + b.im, a.im - b.re);  a + i b = (a.re - b.im, a.im + b.re)
EPA_PK2(add_mi, "v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]")
EPA_PK2(add_pi, "v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]")
EPA_PK2(mul, "v_pk_mul_f32 %0, %1, %2")
// (a.im b.im, a.im b.re) and (a.im b.im, a.re b.im): the first halves of a b and of a conj(b)
EPA_PK2(mul_ii_ir, "v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]")
EPA_PK2(mul_ii_ri, "v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]")
// (a.re b.re - t.lo, a.re b.im + t.hi);  (a.re b.re + t.lo, a.im b.re - t.hi)
EPA_PK3(fma_rr_ri, "v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_lo:[0,0,1]")
EPA_PK3(fma_rr_ir, "v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1] neg_hi:[0,0,1]")
EPA_PK3(fma, "v_pk_fma_f32 %0, %1, %2, %3")
EPA_PK3(fnma, "v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[1,0,0] neg_hi:[1,0,0]")  // c - a b
#undef EPA_PK2
#undef EPA_PK3
__device__ __forceinline__ f2 cmul(f2 a, f2 b) { return fma_rr_ri(a, b, mul_ii_ir(a, b)); }
__device__ __forceinline__ f2 conj(f2 a) { return f2{a.x, -a.y}; }

__device__ __forceinline__ void dft4(f2& u0, f2& u1, f2& u2, f2& u3) {
  const f2 s02 = add(u0, u2), d02 = sub(u0, u2), s13 = add(u1, u3), d13 = sub(u1, u3);
  u0 = add(s02, s13);
  u2 = sub(s02, s13);
  u1 = add_mi(d02, d13);
  u3 = add_pi(d02, d13);
}
__device__ __forceinline__ void idft4(f2& u0, f2& u1, f2& u2, f2& u3) {
  const f2 s02 = add(u0, u2), d02 = sub(u0, u2), s13 = add(u1, u3), d13 = sub(u1, u3);
  u0 = add(s02, s13);
  u2 = sub(s02, s13);
  u1 = add_pi(d02, d13);
  u3 = add_mi(d02, d13);
}
template <bool INV>
__device__ __forceinline__ void dft8(f2 (&v)[8], f2 kh) {
  f2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6], o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
  if (INV) {
    idft4(e0, e1, e2, e3);
    idft4(o0, o1, o2, o3);
  } else {
    dft4(e0, e1, e2, e3);
    dft4(o0, o1, o2, o3);
  }
  // forward: o1 e^{-i pi/4} = kh (o1 - i o1), o3 e^{-3i pi/4} = -kh (o3 + i o3); inverse: the conjugate factors
  const f2 q1 = INV ? add_pi(o1, o1) : add_mi(o1, o1);
  const f2 q3 = INV ? add_mi(o3, o3) : add_pi(o3, o3);
  v[0] = add(e0, o0);
  v[4] = sub(e0, o0);
  v[1] = fma(q1, kh, e1);
  v[5] = fnma(q1, kh, e1);
  v[2] = INV ? add_pi(e2, o2) : add_mi(e2, o2);
  v[6] = INV ? add_mi(e2, o2) : add_pi(e2, o2);
  v[3] = fnma(q3, kh, e3);
  v[7] = fma(q3, kh, e3);
}
__device__ __forceinline__ void twiddle8(f2 (&v)[8], f2 w1) {
  const f2 w2 = cmul(w1, w1), w3 = cmul(w2, w1), w4 = cmul(w2, w2);
  v[1] = cmul(v[1], w1);
  v[2] = cmul(v[2], w2);
  v[3] = cmul(v[3], w3);
  v[4] = cmul(v[4], w4);
  v[5] = cmul(v[5], cmul(w4, w1));
  v[6] = cmul(v[6], cmul(w3, w3));
  v[7] = cmul(v[7], cmul(w4, w3));
}
__device__ __forceinline__ void twiddle4(f2& u1, f2& u2, f2& u3, f2 w1) {
  const f2 w2 = cmul(w1, w1);
  u1 = cmul(u1, w1);
  u2 = cmul(u2, w2);
  u3 = cmul(u3, cmul(w2, w1));
}
__device__ __forceinline__ f2 ld(const unsigned char* xs, int a) { return reinterpret_cast<const f2*>(xs)[pad(a)]; }
__device__ __forceinline__ void st(unsigned char* xs, int a, f2 v) { reinterpret_cast<f2*>(xs)[pad(a)] = v; }
template <int STRIDE>
__device__ __forceinline__ void ld8(const unsigned char* xs, int a0, f2 (&v)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = ld(xs, a0 + STRIDE * r);
}
template <int STRIDE>
__device__ __forceinline__ void st8(unsigned char* xs, int a0, const f2 (&v)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) st(xs, a0 + STRIDE * r, v[r]);
}
}  // namespace pk

template <>
__device__ __forceinline__ void correlate<float>(C2<float> (&vc)[8], unsigned char* xs, const C2<float>* tw,
                                                 const C2<float>* __restrict__ spec, const LaneMap& lm,
                                                 C2<float> w_lane) {
  using pk::f2;
  const int j = threadIdx.x;
  const f2* twp = reinterpret_cast<const f2*>(tw);
  const f2* specp = reinterpret_cast<const f2*>(spec);
  const f2 kh = f2{0.70710678118654752440f, 0.70710678118654752440f};
  f2 v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = f2{vc[i].re, vc[i].im};
  // first pass (sub-size 2048, radix 4, two butterflies per lane): w^(j + 256) = w^j e^{-i pi/4} = kh (w - i w)
  const f2 wa = f2{w_lane.re, w_lane.im};
  const f2 wb = pk::mul(pk::add_mi(wa, wa), kh);
  pk::dft4(v[0], v[2], v[4], v[6]);
  pk::twiddle4(v[2], v[4], v[6], wa);
  pk::dft4(v[1], v[3], v[5], v[7]);
  pk::twiddle4(v[3], v[5], v[7], wb);
#pragma unroll
  for (int i = 0; i < 8; ++i) pk::st(xs, j + 256 * i, v[i]);
  __syncthreads();
  pk::ld8<64>(xs, lm.a1, v);
  pk::dft8<false>(v, kh);
  pk::twiddle8(v, twp[lm.t1]);
  if (EPA_FFT_XPOSE & 1) {
    xp::transpose_vals<3>(v);
  } else {
    pk::st8<64>(xs, lm.a1, v);
    __builtin_amdgcn_wave_barrier();  // (own wavefront's data: ordering for the compiler only)
    pk::ld8<8>(xs, lm.a2, v);
  }
  f2 sp[8];  // the replica spectrum of the fused pass, requested early
#pragma unroll
  for (int r = 0; r < 8; ++r) sp[r] = specp[lm.a3 + r];
  pk::dft8<false>(v, kh);
  pk::twiddle8(v, twp[lm.t2]);
  if (EPA_FFT_XPOSE & 2) {
    xp::transpose_vals<0>(v);
  } else {
    pk::st8<8>(xs, lm.a2, v);
    __builtin_amdgcn_wave_barrier();
    pk::ld8<1>(xs, lm.a3, v);
  }
  pk::dft8<false>(v, kh);
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = pk::cmul(v[r], sp[r]);
  pk::dft8<true>(v, kh);
  if (EPA_FFT_XPOSE & 2) {
    xp::transpose_vals<0>(v);
  } else {
    pk::st8<1>(xs, lm.a3, v);
    __builtin_amdgcn_wave_barrier();
    pk::ld8<8>(xs, lm.a2, v);
  }
  pk::twiddle8(v, pk::conj(twp[lm.t2]));
  pk::dft8<true>(v, kh);
  if (EPA_FFT_XPOSE & 1) {
    xp::transpose_vals<3>(v);
  } else {
    pk::st8<8>(xs, lm.a2, v);
    __builtin_amdgcn_wave_barrier();
    pk::ld8<64>(xs, lm.a1, v);
  }
  pk::twiddle8(v, pk::conj(twp[lm.t1]));
  pk::dft8<true>(v, kh);
  pk::st8<64>(xs, lm.a1, v);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = pk::ld(xs, j + 256 * i);
  // last pass: conjugate twiddles, then the inverse radix-4 butterflies
  const f2 wl = twp[j];
  const f2 wlb = pk::mul(pk::add_mi(wl, wl), kh);
  pk::twiddle4(v[2], v[4], v[6], pk::conj(wl));
  pk::idft4(v[0], v[2], v[4], v[6]);
  pk::twiddle4(v[3], v[5], v[7], pk::conj(wlb));
  pk::idft4(v[1], v[3], v[5], v[7]);
#pragma unroll
  for (int i = 0; i < 8; ++i) vc[i] = C2<float>{v[i].x, v[i].y};
}

}  // namespace
