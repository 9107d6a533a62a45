// convert.open_raw (EK60): the sample blocks of a Simrad .raw file, lying in HBM as they lie on disk, unpacked into the
// (channel, ping_time, range_sample) volumes in ONE launch -- every file sample byte read once, every output byte
// written once, nothing pre-filled.
//
//   epa_raw_index     the framing walk on the host (raw_index.h), no GPU call
//   epa_raw0_unpack   power[c][p][s] = float32(int16 at off_p + 2s) * float32(10 log10(2) / 256)   (parse_base.py:24,302)
//                     athwartship / alongship[c][p][s] = int8 at off_a + 2s / off_a + 2s + 1       (set_groups_ek60.py:681-694)
//                     NaN behind a row's count and in a row without a datagram (offset -1)
//   epa_raw3_unpack   convert.open_raw_ek80: backscatter_r / _i[c][p][s][b] = the float32 pair at off + 8 (s B_row + b), bit
//                     copies, an imaginary part equal to 0.0 made NaN (parse_base.py:312-314); NaN behind the count, in
//                     sectors the row lacks and in a row without a datagram
//
// A wavefront owns one output row.  NME0 datagrams between the pings have any length, so a sample block starts at ANY
// byte offset: the int16 samples are not 2-byte aligned in general.  The file is therefore read as the aligned dwords
// it is made of -- the block of a ping is contiguous -- and the samples are shifted out of two neighbouring dwords
// (the shift is the same for a whole row).  The allocation is padded to a multiple of 16 bytes, and a dword is only
// fetched when at least one byte of it belongs to the samples asked for, so no load leaves the allocation.  Stores are
// 16-byte chunks aligned in the OUTPUT (rows of odd S start at any element); the elements in front of the first chunk
// and behind the last are stored one by one.  Stores are non-temporal: nothing re-reads the volumes soon.
#include "epa_internal.h"
#include "raw_index.h"

namespace {

constexpr int kWaves = epa::kBlock / 64;
constexpr float kIndex2Power = 0.011758984205624266f;  // float32(10*log10(2)/256), as fused_sv_mvbs.hip
enum { kAngNone = 0, kAngI8 = 1, kAngF32 = 2 };

typedef const uint32_t __attribute__((address_space(1))) * words_ptr;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, unsigned sh) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);  // sh in {0, 8, 16, 24}
}

// the 2 bytes at byte offset b (both inside the file): the second dword only when the pair straddles it
__device__ __forceinline__ uint32_t load2(words_ptr words, long long b) {
  const long long w = b >> 2;
  const unsigned sh = (unsigned)(b & 3) * 8u;
  const uint32_t a = words[w];
  const uint32_t hi = sh == 24u ? words[w + 1] : 0u;
  return funnel(a, hi, sh) & 0xffffu;
}

// N dwords (4 N bytes) of a chunk that lies wholly inside a row's block, from dword w on: N aligned dwords, one more when
// the block is not dword-aligned.  The shift is the ROW's (every chunk starts a whole number of dwords behind the
// first), so SHIFTED is decided once per row and the loop body has no branch: the loads of several chunks are in
// flight together.  The extra dword holds at least one byte of the chunk (SHIFTED), so it lies inside the allocation.
template <int N, bool SHIFTED>
__device__ __forceinline__ void load_row_dwords(words_ptr words, long long w, unsigned sh, uint32_t (&out)[N]) {
  uint32_t d[N + 1];
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = words[w + i];
  d[N] = SHIFTED ? words[w + N] : 0u;
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = SHIFTED ? funnel(d[i], d[i + 1], sh) : d[i];
}

__device__ __forceinline__ float power_of(uint32_t h) { return (float)(short)(h & 0xffffu) * kIndex2Power; }
__device__ __forceinline__ float s8(uint32_t b) { return (float)(signed char)(b & 0xffu); }

// chunks [0, nfull) of a row, all samples present: dst and the file offset b0 are those of chunk 0
template <bool SHIFTED>
__device__ __forceinline__ void power_chunks(words_ptr words, long long b0, float* __restrict__ dst, long long nfull, int lane) {
  const long long w0 = b0 >> 2;
  const unsigned sh = (unsigned)(b0 & 3) * 8u;
#pragma unroll 4
  for (long long ch = lane; ch < nfull; ch += 64) {
    uint32_t r[2];
    load_row_dwords<2, SHIFTED>(words, w0 + 2 * ch, sh, r);
    const f4 v = f4{power_of(r[0]), power_of(r[0] >> 16), power_of(r[1]), power_of(r[1] >> 16)};
    __builtin_nontemporal_store(v, reinterpret_cast<f4*>(dst + 4 * ch));
  }
}

template <bool SHIFTED>
__device__ __forceinline__ void angle_chunks_f32(words_ptr words, long long b0, float* __restrict__ da, float* __restrict__ dl,
                                                 long long nfull, int lane) {
  const long long w0 = b0 >> 2;
  const unsigned sh = (unsigned)(b0 & 3) * 8u;
#pragma unroll 4
  for (long long ch = lane; ch < nfull; ch += 64) {
    uint32_t r[2];
    load_row_dwords<2, SHIFTED>(words, w0 + 2 * ch, sh, r);
    const f4 a = f4{s8(r[0]), s8(r[0] >> 16), s8(r[1]), s8(r[1] >> 16)};
    const f4 l = f4{s8(r[0] >> 8), s8(r[0] >> 24), s8(r[1] >> 8), s8(r[1] >> 24)};
    __builtin_nontemporal_store(a, reinterpret_cast<f4*>(da + 4 * ch));
    __builtin_nontemporal_store(l, reinterpret_cast<f4*>(dl + 4 * ch));
  }
}

template <bool SHIFTED>
__device__ __forceinline__ void angle_chunks_i8(words_ptr words, long long b0, int8_t* __restrict__ da, int8_t* __restrict__ dl,
                                                long long nfull, int lane) {
  const long long w0 = b0 >> 2;
  const unsigned sh = (unsigned)(b0 & 3) * 8u;
#pragma unroll 2
  for (long long ch = lane; ch < nfull; ch += 64) {
    uint32_t r[8];
    load_row_dwords<8, SHIFTED>(words, w0 + 8 * ch, sh, r);
    u4 a, l;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t x = r[2 * q], y = r[2 * q + 1];
      a[q] = (x & 0xffu) | (((x >> 16) & 0xffu) << 8) | ((y & 0xffu) << 16) | (((y >> 16) & 0xffu) << 24);
      l[q] = ((x >> 8) & 0xffu) | ((x >> 24) << 8) | (((y >> 8) & 0xffu) << 16) | ((y >> 24) << 24);
    }
    __builtin_nontemporal_store(a, reinterpret_cast<u4*>(da + 16 * ch));
    __builtin_nontemporal_store(l, reinterpret_cast<u4*>(dl + 16 * ch));
  }
}

template <int ANG>
__global__ void __launch_bounds__(epa::kBlock)
raw0_unpack_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ table, long long rows, long long S,
                   float* __restrict__ power, void* __restrict__ athw_out, void* __restrict__ along_out, int xcd_map) {
  const words_ptr words = (words_ptr)(uintptr_t)bytes;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long g = xcd_map ? epa::xcd_contiguous((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  const long long row = g * kWaves + wave;  // wave-uniform
  if (row >= rows) return;
  const long long off_p = table[3 * row], off_a = table[3 * row + 1], count = table[3 * row + 2];
  const long long np = off_p >= 0 ? count : 0;                      // samples with a power value
  const long long na = (ANG != kAngNone && off_a >= 0) ? count : 0; // ... with an angle pair
  const float nan = __uint_as_float(0x7FC00000u);                   // NumPy's np.nan in float32

  // ---- float32 planes: power, and the angle pair in its padded form (the three rows have ONE geometry: the bases are
  // 16-byte aligned, the entry point sees to it) ----
  {
    float* __restrict__ dp = power + row * S;
    float* __restrict__ da = ANG == kAngF32 ? static_cast<float*>(athw_out) + row * S : nullptr;
    float* __restrict__ dl = ANG == kAngF32 ? static_cast<float*>(along_out) + row * S : nullptr;
    long long head = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dp) & 15u)) & 15u) / 4u);
    if (head > S) head = S;
    const long long nchunk = (S - head) / 4;
    const long long tail0 = head + nchunk * 4;
    auto one = [&](long long j) {
      __builtin_nontemporal_store(j < np ? power_of(load2(words, off_p + 2 * j)) : nan, dp + j);
      if (ANG == kAngF32) {
        const uint32_t pr = j < na ? load2(words, off_a + 2 * j) : 0u;
        __builtin_nontemporal_store(j < na ? s8(pr) : nan, da + j);
        __builtin_nontemporal_store(j < na ? s8(pr >> 8) : nan, dl + j);
      }
    };
    if (lane < head) one(lane);
    if (tail0 + lane < S) one(tail0 + lane);  // (fewer than 4 elements)
    // chunks that lie wholly inside the row's samples: no branch in the loop (the shift is the row's, wave-uniform)
    const long long full_p = np > head ? ((np - head) / 4 < nchunk ? (np - head) / 4 : nchunk) : 0;
    if (full_p > 0) {
      const long long b0 = off_p + 2 * head;
      if (__builtin_amdgcn_readfirstlane((int)(b0 & 3))) power_chunks<true>(words, b0, dp + head, full_p, lane);
      else power_chunks<false>(words, b0, dp + head, full_p, lane);
    }
    long long full_a = 0;
    if (ANG == kAngF32) {
      full_a = na > head ? ((na - head) / 4 < nchunk ? (na - head) / 4 : nchunk) : 0;
      if (full_a > 0) {
        const long long b0 = off_a + 2 * head;
        if (__builtin_amdgcn_readfirstlane((int)(b0 & 3))) angle_chunks_f32<true>(words, b0, da + head, dl + head, full_a, lane);
        else angle_chunks_f32<false>(words, b0, da + head, dl + head, full_a, lane);
      }
    }
    // the chunk that straddles the count, and the NaN chunks behind it
    for (long long ch = full_p + lane; ch < nchunk; ch += 64) {
      const long long j = head + ch * 4;
      f4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = j + e < np ? power_of(load2(words, off_p + 2 * (j + e))) : nan;
      __builtin_nontemporal_store(v, reinterpret_cast<f4*>(dp + j));
    }
    if (ANG == kAngF32) {
      for (long long ch = full_a + lane; ch < nchunk; ch += 64) {
        const long long j = head + ch * 4;
        f4 a, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t pr = j + e < na ? load2(words, off_a + 2 * (j + e)) : 0u;
          a[e] = j + e < na ? s8(pr) : nan;
          l[e] = j + e < na ? s8(pr >> 8) : nan;
        }
        __builtin_nontemporal_store(a, reinterpret_cast<f4*>(da + j));
        __builtin_nontemporal_store(l, reinterpret_cast<f4*>(dl + j));
      }
    }
  }

  // ---- int8 planes: every row is full and has angles (checked on the host), 16 samples = 32 file bytes per chunk ----
  if (ANG == kAngI8) {
    int8_t* __restrict__ da = static_cast<int8_t*>(athw_out) + row * S;
    int8_t* __restrict__ dl = static_cast<int8_t*>(along_out) + row * S;
    long long head = (long long)((16u - (unsigned)(reinterpret_cast<uintptr_t>(da) & 15u)) & 15u);
    if (head > S) head = S;
    const long long nchunk = (S - head) / 16;
    const long long tail0 = head + nchunk * 16;
    auto one = [&](long long j) {
      const uint32_t pr = load2(words, off_a + 2 * j);
      da[j] = (int8_t)(pr & 0xffu);
      dl[j] = (int8_t)((pr >> 8) & 0xffu);
    };
    if (lane < head) one(lane);
    if (tail0 + lane < S) one(tail0 + lane);  // (fewer than 16 elements)
    if (nchunk > 0) {
      const long long b0 = off_a + 2 * head;
      if (__builtin_amdgcn_readfirstlane((int)(b0 & 3))) angle_chunks_i8<true>(words, b0, da + head, dl + head, nchunk, lane);
      else angle_chunks_i8<false>(words, b0, da + head, dl + head, nchunk, lane);
    }
  }
}

// ---- convert.open_raw_ek80: the RAW3 complex sample blocks ---------------------------------------------------------------
// A block holds count * B_row pairs (real, imaginary) of float32, sample by sample, sector by sector.  Values are bit
// copies; the one rule is the reference's (parse_base.py:312-314): an imaginary part that equals 0.0 becomes NaN.
constexpr uint32_t kNanBits = 0x7FC00000u;
constexpr int kMaxBeams = 8;  // as ek80_complex.hip

__device__ __forceinline__ uint32_t imag_of(uint32_t v) { return (v & 0x7fffffffu) ? v : kNanBits; }

// the 4 bytes at byte offset b (all inside the file): the second dword only when the value straddles it
__device__ __forceinline__ uint32_t load4(words_ptr words, long long b) {
  const long long w = b >> 2;
  const unsigned sh = (unsigned)(b & 3) * 8u;
  const uint32_t a = words[w];
  const uint32_t hi = sh ? words[w + 1] : 0u;
  return funnel(a, hi, sh);
}

// chunks [0, nfull) of a row whose B_row is B, all elements present: a flat de-interleave, 8 file dwords -> 4 real + 4
// imaginary words.  dre / dim and the file offset b0 are those of chunk 0.
template <bool SHIFTED>
__device__ __forceinline__ void complex_chunks(words_ptr words, long long b0, uint32_t* __restrict__ dre,
                                               uint32_t* __restrict__ dim, long long nfull, int lane) {
  const long long w0 = b0 >> 2;
  const unsigned sh = (unsigned)(b0 & 3) * 8u;
#pragma unroll 2
  for (long long ch = lane; ch < nfull; ch += 64) {
    uint32_t r[8];
    load_row_dwords<8, SHIFTED>(words, w0 + 8 * ch, sh, r);
    const u4 re = u4{r[0], r[2], r[4], r[6]};
    const u4 im = u4{imag_of(r[1]), imag_of(r[3]), imag_of(r[5]), imag_of(r[7])};
    __builtin_nontemporal_store(re, reinterpret_cast<u4*>(dre + 4 * ch));
    __builtin_nontemporal_store(im, reinterpret_cast<u4*>(dim + 4 * ch));
  }
}

__global__ void __launch_bounds__(epa::kBlock)
raw3_unpack_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ table, long long rows, long long S, int B,
                   uint32_t* __restrict__ re_out, uint32_t* __restrict__ im_out, int xcd_map) {
  const words_ptr words = (words_ptr)(uintptr_t)bytes;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long g = xcd_map ? epa::xcd_contiguous((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  const long long row = g * kWaves + wave;  // wave-uniform
  if (row >= rows) return;
  const long long off = table[3 * row], count = table[3 * row + 1];
  const int brow = (int)table[3 * row + 2];
  const long long N = S * B;                                       // elements of an output row
  const long long nel = (off >= 0 && brow > 0) ? count * B : 0;    // elements in front of the first padded SAMPLE
  const bool flat = brow == B;                                     // wave-uniform: the block is the row's front, interleaved
  uint32_t* __restrict__ dre = re_out + row * N;
  uint32_t* __restrict__ dim = im_out + row * N;                   // (the two planes have ONE geometry: see the entry point)
  long long head = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dre) & 15u)) & 15u) / 4u);
  if (head > N) head = N;
  const long long nchunk = (N - head) / 4;
  const long long tail0 = head + nchunk * 4;
  // element j of the output row: present when its sample lies in front of the count and its sector exists
  auto fetch = [&](long long j, uint32_t& vr, uint32_t& vi) {
    vr = kNanBits;
    vi = kNanBits;
    if (j < nel) {
      long long e = j;
      if (!flat) {
        const long long s = j / B;
        const int b = (int)(j - s * B);
        e = b < brow ? s * brow + b : -1;
      }
      if (e >= 0) {
        vr = load4(words, off + 8 * e);
        vi = imag_of(load4(words, off + 8 * e + 4));
      }
    }
  };
  auto one = [&](long long j) {
    uint32_t vr, vi;
    fetch(j, vr, vi);
    __builtin_nontemporal_store(vr, dre + j);
    __builtin_nontemporal_store(vi, dim + j);
  };
  if (lane < head) one(lane);
  if (tail0 + lane < N) one(tail0 + lane);  // (fewer than 4 elements)
  // chunks that lie wholly inside a flat row's elements: no branch in the loop (the shift is the row's, wave-uniform)
  const long long full = (flat && nel > head) ? ((nel - head) / 4 < nchunk ? (nel - head) / 4 : nchunk) : 0;
  if (full > 0) {
    const long long b0 = off + 8 * head;
    if (__builtin_amdgcn_readfirstlane((int)(b0 & 3))) complex_chunks<true>(words, b0, dre + head, dim + head, full, lane);
    else complex_chunks<false>(words, b0, dre + head, dim + head, full, lane);
  }
  // the chunk that straddles the count and the NaN chunks behind it; every chunk of a row with fewer sectors than B
  for (long long ch = full + lane; ch < nchunk; ch += 64) {
    const long long j = head + ch * 4;
    u4 vr, vi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      uint32_t a, b;
      fetch(j + e, a, b);
      vr[e] = a;
      vi[e] = b;
    }
    __builtin_nontemporal_store(vr, reinterpret_cast<u4*>(dre + j));
    __builtin_nontemporal_store(vi, reinterpret_cast<u4*>(dim + j));
  }
}

}  // namespace

extern "C" int epa_raw3_unpack(const uint8_t* bytes, long long n_bytes, long long n_alloc, const int64_t* table_host,
                               const int64_t* table, int C, long long P, long long S, int B, float* backscatter_r,
                               float* backscatter_i, epa_stream_t stream) {
  EPA_CHECK_ARG(bytes && table_host && table && backscatter_r && backscatter_i, "epa_raw3_unpack: NULL array argument");
  EPA_CHECK_ARG(C >= 1 && P >= 1 && S >= 1 && P <= (1LL << 40) && S <= (1LL << 40),
                "epa_raw3_unpack: C=%d, P=%lld, S=%lld must all be at least 1", C, P, S);
  EPA_CHECK_ARG(B >= 1 && B <= kMaxBeams, "epa_raw3_unpack: 1 .. %d sectors are served (got B=%d)", kMaxBeams, B);
  EPA_CHECK_ARG(n_bytes >= 0 && n_alloc >= n_bytes && n_alloc % 16 == 0 && (reinterpret_cast<uintptr_t>(bytes) & 15u) == 0,
                "epa_raw3_unpack: the file buffer must be 16-byte aligned and padded to a multiple of 16 bytes "
                "(n_bytes=%lld, n_alloc=%lld)", n_bytes, n_alloc);
  // one geometry for both planes: heads and chunks are computed from the real plane's addresses
  EPA_CHECK_ARG((reinterpret_cast<uintptr_t>(backscatter_r) & 15u) == 0 && (reinterpret_cast<uintptr_t>(backscatter_i) & 15u) == 0,
                "epa_raw3_unpack: the output planes must be 16-byte aligned");
  const long long rows = (long long)C * P;
  EPA_CHECK_ARG((rows + kWaves - 1) / kWaves <= 0x7fffffffLL && (double)rows * (double)S * (double)B * 4.0 < 9.0e18,
                "epa_raw3_unpack: %lld rows of %lld samples are more than one launch takes", rows, S);
  for (long long r = 0; r < rows; ++r) {
    const long long off = table_host[3 * r], count = table_host[3 * r + 1], brow = table_host[3 * r + 2];
    EPA_CHECK_ARG(count >= 0 && count <= S, "epa_raw3_unpack: row %lld has count=%lld, 0 .. S=%lld are served", r, count, S);
    EPA_CHECK_ARG(brow >= 0 && brow <= B, "epa_raw3_unpack: row %lld has %lld sectors, 0 .. B=%d are served", r, brow, B);
    EPA_CHECK_ARG(off >= -1 && (off < 0 || (off <= n_bytes && 8 * count * brow <= n_bytes - off)),
                  "epa_raw3_unpack: the complex block of row %lld (offset %lld, %lld samples of %lld sectors) leaves the "
                  "%lld file bytes", r, off, count, brow, n_bytes);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((rows + kWaves - 1) / kWaves)), block(epa::kBlock);
  const int xm = epa::xcd_map_enabled() ? 1 : 0;
  hipLaunchKernelGGL(raw3_unpack_kernel, grid, block, 0, st, bytes, table, rows, S, B, reinterpret_cast<uint32_t*>(backscatter_r),
                     reinterpret_cast<uint32_t*>(backscatter_i), xm);
  return epa::check_launch("raw3_unpack_kernel");
}

extern "C" int epa_raw_index(const uint8_t* bytes_host, long long n_bytes, epa_raw_record* records_out, long long capacity,
                             long long* n_records, long long* n_bytes_consumed) {
  EPA_CHECK_ARG(n_records && n_bytes_consumed, "epa_raw_index: n_records / n_bytes_consumed is NULL");
  *n_records = 0;
  *n_bytes_consumed = 0;
  EPA_CHECK_ARG(n_bytes >= 0 && (bytes_host || n_bytes == 0), "epa_raw_index: bytes_host is NULL or n_bytes=%lld is negative",
                n_bytes);
  EPA_CHECK_ARG(capacity >= 0 && (records_out || capacity == 0), "epa_raw_index: records_out is NULL with capacity=%lld",
                capacity);
  int64_t n = 0, used = 0;
  epa_raw::ScanError err{};
  const int code = epa_raw::scan(bytes_host, n_bytes, records_out, capacity, &n, &used, &err);
  *n_records = n;
  *n_bytes_consumed = used;
  EPA_CHECK_ARG(code != epa_raw::kScanSizeTooSmall,
                "epa_raw_index: datagram %lld at byte offset %lld has size %d, less than the 16 bytes of its own header",
                (long long)n, (long long)err.offset, err.size);
  EPA_CHECK_ARG(code != epa_raw::kScanTrailerDiffers,
                "epa_raw_index: datagram %lld at byte offset %lld: the size behind it (%d) differs from the size in front "
                "(%d); this reader does not search for the next datagram",
                (long long)n, (long long)err.offset, err.trailer, err.size);
  return EPA_OK;
}

extern "C" int epa_raw0_unpack(const uint8_t* bytes, long long n_bytes, long long n_alloc, const int64_t* table_host,
                               const int64_t* table, int C, long long P, long long S, int angle_type, float* power,
                               void* athwartship, void* alongship, epa_stream_t stream) {
  EPA_CHECK_ARG(bytes && table_host && table && power, "epa_raw0_unpack: NULL array argument");
  EPA_CHECK_ARG(C >= 1 && P >= 1 && S >= 1 && P <= (1LL << 40) && S <= (1LL << 40),
                "epa_raw0_unpack: C=%d, P=%lld, S=%lld must all be at least 1", C, P, S);
  EPA_CHECK_ARG(angle_type == EPA_RAW_ANGLE_NONE || angle_type == EPA_RAW_ANGLE_I8 || angle_type == EPA_RAW_ANGLE_F32,
                "epa_raw0_unpack: angle_type %d is not of enum epa_raw_angle", angle_type);
  EPA_CHECK_ARG(angle_type == EPA_RAW_ANGLE_NONE || (athwartship && alongship), "epa_raw0_unpack: an angle plane is NULL");
  EPA_CHECK_ARG(n_bytes >= 0 && n_alloc >= n_bytes && n_alloc % 16 == 0 && (reinterpret_cast<uintptr_t>(bytes) & 15u) == 0,
                "epa_raw0_unpack: the file buffer must be 16-byte aligned and padded to a multiple of 16 bytes "
                "(n_bytes=%lld, n_alloc=%lld)", n_bytes, n_alloc);
  EPA_CHECK_ARG((reinterpret_cast<uintptr_t>(power) & 15u) == 0 &&
                    (angle_type == EPA_RAW_ANGLE_NONE || ((reinterpret_cast<uintptr_t>(athwartship) & 15u) == 0 &&
                                                          (reinterpret_cast<uintptr_t>(alongship) & 15u) == 0)),
                "epa_raw0_unpack: the output planes must be 16-byte aligned");
  const long long rows = (long long)C * P;
  EPA_CHECK_ARG((rows + kWaves - 1) / kWaves <= 0x7fffffffLL && (double)rows * (double)S * 4.0 < 9.0e18,
                "epa_raw0_unpack: %lld rows of %lld samples are more than one launch takes", rows, S);
  for (long long r = 0; r < rows; ++r) {
    const long long off_p = table_host[3 * r], off_a = table_host[3 * r + 1], count = table_host[3 * r + 2];
    EPA_CHECK_ARG(count >= 0 && count <= S, "epa_raw0_unpack: row %lld has count=%lld, 0 .. S=%lld are served", r, count, S);
    EPA_CHECK_ARG(off_p >= -1 && (off_p < 0 || (off_p <= n_bytes && 2 * count <= n_bytes - off_p)),
                  "epa_raw0_unpack: the power block of row %lld (offset %lld, %lld samples) leaves the %lld file bytes", r,
                  off_p, count, n_bytes);
    EPA_CHECK_ARG(off_a >= -1 && (off_a < 0 || (off_a <= n_bytes && 2 * count <= n_bytes - off_a)),
                  "epa_raw0_unpack: the angle block of row %lld (offset %lld, %lld samples) leaves the %lld file bytes", r,
                  off_a, count, n_bytes);
    EPA_CHECK_ARG(angle_type != EPA_RAW_ANGLE_I8 || (off_a >= 0 && count == S),
                  "epa_raw0_unpack: int8 angle planes need an angle block of S=%lld samples in every row, row %lld has "
                  "offset %lld and count %lld (a pad needs NaN: ask for float32 planes)", S, r, off_a, count);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((rows + kWaves - 1) / kWaves)), block(epa::kBlock);
  const int xm = epa::xcd_map_enabled() ? 1 : 0;
  switch (angle_type) {
    case EPA_RAW_ANGLE_NONE:
      hipLaunchKernelGGL((raw0_unpack_kernel<kAngNone>), grid, block, 0, st, bytes, table, rows, S, power, nullptr, nullptr, xm);
      return epa::check_launch("raw0_unpack_kernel<power>");
    case EPA_RAW_ANGLE_I8:
      hipLaunchKernelGGL((raw0_unpack_kernel<kAngI8>), grid, block, 0, st, bytes, table, rows, S, power, athwartship, alongship,
                         xm);
      return epa::check_launch("raw0_unpack_kernel<power, int8 angles>");
    default:
      hipLaunchKernelGGL((raw0_unpack_kernel<kAngF32>), grid, block, 0, st, bytes, table, rows, S, power, athwartship,
                         alongship, xm);
      return epa::check_launch("raw0_unpack_kernel<power, float32 angles>");
  }
}
