// combine_echodata: the (channel, ping_time, range_sample[, beam]) cubes of many files joined along ping_time into one
// volume, the shorter rows NaN-padded to the longest (xarray's outer join on range_sample) -- a ragged concatenation in
// ONE launch per variable, every source byte read once and every output byte written once.
//
//   epa_concat_rows   out[c][p][:] for p in file i's pings = src_i[chan[i][c]][p - first_i][:W_i], NaN behind W_i.
//
// A wavefront owns whole output rows (a workgroup: kRowsPerGroup consecutive ones).  It finds the file of its row by a
// wave-uniform binary search of the first-ping column of the segment table, then streams the row in 16-byte chunks that
// are aligned in the OUTPUT: the elements in front of the first aligned chunk and behind the last one are stored one by
// one (at most 15 bytes each).  A source row starts at (c * P_i + p) * W_i elements, so for odd W_i it is only
// element-aligned and shifted against the output row: the 16 source bytes of a chunk are loaded with no more than the
// element's own alignment promised to the compiler (gfx950's vector memory unit serves such loads; the compiler keeps them
// as wide as the target allows).  The chunk that straddles W_i is put together element by element, the chunks behind it
// are the NaN pattern (NumPy's: 0x7FC00000 / 0x7FF8000000000000).  Stores are non-temporal: nothing re-reads the volume soon.
#include "epa_internal.h"

namespace {

constexpr int kWaves = epa::kBlock / 64;
constexpr int kRowsPerWave = 4;
constexpr int kRowsPerGroup = kWaves * kRowsPerWave;

template <typename D>
struct NaNBits;
template <>
struct NaNBits<float> {
  static __device__ __forceinline__ float get() { return __uint_as_float(0x7FC00000u); }
};
template <>
struct NaNBits<double> {
  static __device__ __forceinline__ double get() { return __longlong_as_double(0x7FF8000000000000LL); }
};
// same-type copies move unsigned words: the pad of a 4- / 8-byte one is the float pattern of that width (the entry point
// lets a pad through for float types only); 1- and 2-byte elements are never padded
template <>
struct NaNBits<uint32_t> {
  static __device__ __forceinline__ uint32_t get() { return 0x7FC00000u; }
};
template <>
struct NaNBits<uint64_t> {
  static __device__ __forceinline__ uint64_t get() { return 0x7FF8000000000000ULL; }
};
template <>
struct NaNBits<uint8_t> {
  static __device__ __forceinline__ uint8_t get() { return 0; }
};
template <>
struct NaNBits<uint16_t> {
  static __device__ __forceinline__ uint16_t get() { return 0; }
};

template <typename S, typename D>
__device__ __forceinline__ D conv(S v) {
  return static_cast<D>(v);  // int -> float: round to nearest even, as ndarray.astype does; same type: the bits
}

template <typename D>
struct Chunk {
  static constexpr int N = 16 / sizeof(D);
  typedef D vec __attribute__((ext_vector_type(N)));
};

// N consecutive source elements behind an address that is aligned like ONE element
template <typename S, int N>
struct Elems {
  typedef S full __attribute__((ext_vector_type(N)));
  typedef full vec __attribute__((aligned(sizeof(S))));
};

template <typename S, typename D>
__global__ void __launch_bounds__(epa::kBlock)
concat_rows_kernel(const epa_concat_seg* __restrict__ segs, const int* __restrict__ chan, int nseg, int C,
                   long long P_tot, long long W_out, long long rows, D* __restrict__ out, int xcd_map) {
  constexpr int N = Chunk<D>::N;
  using vec = typename Chunk<D>::vec;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long g = xcd_map ? epa::xcd_contiguous((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  const D nan = NaNBits<D>::get();
#pragma unroll 1
  for (int k = 0; k < kRowsPerWave; ++k) {
    const long long row = g * kRowsPerGroup + (long long)k * kWaves + wave;  // wave-uniform
    if (row >= rows) return;
    const long long c = row / P_tot, p = row - c * P_tot;
    // the last segment whose first ping is <= p (segs[0].first == 0, the firsts ascend strictly)
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[mid].first <= p) lo = mid;
      else hi = mid - 1;
    }
    const epa_concat_seg sg = segs[lo];
    const long long W = sg.W;
    const long long cs = chan[(long long)lo * C + c];
    // (the base comes out of a table: told to be global memory, the loads are global_load, not flat_load)
    typedef const S __attribute__((address_space(1))) * src_ptr;
    const src_ptr src = (src_ptr)(uintptr_t)sg.base + (cs * sg.P + (p - sg.first)) * W;
    D* __restrict__ dst = out + row * W_out;
    // elements in front of the first 16-byte boundary of the output row (dst is element-aligned: a whole number)
    long long head = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / sizeof(D));
    if (head > W_out) head = W_out;
    const long long nchunk = (W_out - head) / N;
    const long long tail0 = head + nchunk * N;
    if (lane < head) {
      const long long j = lane;
      __builtin_nontemporal_store(j < W ? conv<S, D>(src[j]) : nan, dst + j);
    }
    if (tail0 + lane < W_out) {  // (fewer than N <= 16 elements)
      const long long j = tail0 + lane;
      __builtin_nontemporal_store(j < W ? conv<S, D>(src[j]) : nan, dst + j);
    }
    for (long long ch = lane; ch < nchunk; ch += 64) {
      const long long j = head + ch * N;
      vec v;
      if (j + N <= W) {
        typedef const typename Elems<S, N>::vec __attribute__((address_space(1))) * elems_ptr;
        const typename Elems<S, N>::full s = *(elems_ptr)(src + j);
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = conv<S, D>(s[e]);
      } else {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = j + e < W ? conv<S, D>(src[j + e]) : nan;
      }
      __builtin_nontemporal_store(v, reinterpret_cast<vec*>(dst + j));
    }
  }
}

constexpr int kSize[EPA_CT_COUNT] = {1, 2, 4, 8, 4, 8};

inline bool is_float(int t) { return t == EPA_CT_F32 || t == EPA_CT_F64; }

template <typename S, typename D>
int launch(const epa_concat_seg* segs, const int* chan, int nseg, int C, long long P_tot, long long W_out, void* out,
           hipStream_t st) {
  const long long rows = (long long)C * P_tot;
  const long long grid = (rows + kRowsPerGroup - 1) / kRowsPerGroup;
  hipLaunchKernelGGL((concat_rows_kernel<S, D>), dim3((unsigned)grid), dim3(epa::kBlock), 0, st, segs, chan, nseg, C, P_tot,
                     W_out, rows, static_cast<D*>(out), epa::xcd_map_enabled() ? 1 : 0);
  return epa::check_launch("concat_rows_kernel");
}

}  // namespace

extern "C" int epa_concat_rows(const epa_concat_seg* segs_host, const epa_concat_seg* segs, const int* chan_host,
                               const int* chan, int nseg, int C, long long W_out, int src_type, int out_type, void* out,
                               epa_stream_t stream) {
  EPA_CHECK_ARG(segs_host && segs && chan_host && chan, "epa_concat_rows: NULL table argument");
  EPA_CHECK_ARG(nseg >= 1 && C >= 1 && W_out >= 1, "epa_concat_rows: nseg=%d, C=%d, W_out=%lld must all be at least 1", nseg, C,
                W_out);
  EPA_CHECK_ARG(src_type >= 0 && src_type < EPA_CT_COUNT && out_type >= 0 && out_type < EPA_CT_COUNT,
                "epa_concat_rows: element types %d -> %d are not of enum epa_concat_type", src_type, out_type);
  const bool same = src_type == out_type;
  const bool widen = (src_type == EPA_CT_I8 && out_type == EPA_CT_F32) || (src_type == EPA_CT_I16 && out_type == EPA_CT_F32) ||
                     (src_type == EPA_CT_I32 && out_type == EPA_CT_F64) || (src_type == EPA_CT_I64 && out_type == EPA_CT_F64);
  EPA_CHECK_ARG(same || widen,
                "epa_concat_rows: element types %d -> %d: same-type copies and int8/int16 -> f32, int32/int64 -> f64 are served",
                src_type, out_type);
  long long P_tot = 0;
  bool padded = false;
  // (the shapes before the pointers: an empty segment has no memory, and is refused for what it is)
  for (int i = 0; i < nseg; ++i) {
    const epa_concat_seg& s = segs_host[i];
    EPA_CHECK_ARG(s.P >= 1, "epa_concat_rows: segment %d has P=%lld pings, at least 1 is needed", i, s.P);
    EPA_CHECK_ARG(s.W >= 1 && s.W <= W_out, "epa_concat_rows: segment %d has rows of W=%lld elements, 1 .. W_out=%lld are served",
                  i, s.W, W_out);
    EPA_CHECK_ARG(s.base, "epa_concat_rows: segment %d has no base pointer", i);
    EPA_CHECK_ARG(s.first == P_tot, "epa_concat_rows: segment %d starts at output ping %lld, %lld pings lie before it", i,
                  s.first, P_tot);
    EPA_CHECK_ARG(s.C >= 1 && s.C <= (1LL << 20), "epa_concat_rows: segment %d has C=%lld source channels", i, s.C);
    EPA_CHECK_ARG(s.P <= (1LL << 40) && s.W <= (1LL << 40) && P_tot <= (1LL << 40), "epa_concat_rows: segment %d is too large", i);
    P_tot += s.P;
    padded |= s.W < W_out;
    for (int c = 0; c < C; ++c) {
      const int cs = chan_host[(long long)i * C + c];
      EPA_CHECK_ARG(cs >= 0 && cs < s.C, "epa_concat_rows: segment %d maps output channel %d to source channel %d of %lld", i,
                    c, cs, s.C);
    }
  }
  EPA_CHECK_ARG(!padded || is_float(out_type),
                "epa_concat_rows: rows shorter than W_out=%lld need a NaN pad, the output type %d is an integer", W_out, out_type);
  EPA_CHECK_ARG(out, "epa_concat_rows: out is NULL");
  const long long rows = (long long)C * P_tot;
  EPA_CHECK_ARG((rows + kRowsPerGroup - 1) / kRowsPerGroup <= 0x7fffffffLL && W_out <= (1LL << 40) &&
                    (double)rows * (double)W_out * kSize[out_type] < 9.0e18,
                "epa_concat_rows: %lld rows of %lld elements are more than one launch takes", rows, W_out);
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)(rows * W_out * kSize[out_type]);
  for (int i = 0; i < nseg; ++i) {
    const epa_concat_seg& s = segs_host[i];
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(s.base), b1 = b0 + (uintptr_t)(s.C * s.P * s.W * kSize[src_type]);
    EPA_CHECK_ARG(b1 <= o0 || o1 <= b0, "epa_concat_rows: out overlaps the source of segment %d", i);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (same) {
    switch (kSize[src_type]) {
      case 1: return launch<uint8_t, uint8_t>(segs, chan, nseg, C, P_tot, W_out, out, st);
      case 2: return launch<uint16_t, uint16_t>(segs, chan, nseg, C, P_tot, W_out, out, st);
      case 4: return launch<uint32_t, uint32_t>(segs, chan, nseg, C, P_tot, W_out, out, st);
      default: return launch<uint64_t, uint64_t>(segs, chan, nseg, C, P_tot, W_out, out, st);
    }
  }
  switch (src_type) {
    case EPA_CT_I8: return launch<int8_t, float>(segs, chan, nseg, C, P_tot, W_out, out, st);
    case EPA_CT_I16: return launch<int16_t, float>(segs, chan, nseg, C, P_tot, W_out, out, st);
    case EPA_CT_I32: return launch<int32_t, double>(segs, chan, nseg, C, P_tot, W_out, out, st);
    default: return launch<int64_t, double>(segs, chan, nseg, C, P_tot, W_out, out, st);
  }
}
