// convert.open_raw (EK60): latitude / longitude from the NMEA sentences of the NME0 datagrams, read where they lie -- in
// the file's bytes in HBM, between the sample blocks -- instead of one pynmea2.parse per sentence on the host
// (set_groups_base.py:180-239).  17 bytes go back per fix.  The rules are those of convert/parse_nmea.py (R2 - R6).
//
//   epa_nmea_positions   per selected sentence: lat, lon (float64) and a status byte (EPA_NMEA_*)
//
// A wavefront owns one sentence.  Lane i holds byte i of a 64-byte step; __ballot gives the comma / star / white-space /
// non-printable masks as 64-bit words, which are wave-uniform: everything that follows them -- the k-th comma (a bit scan),
// the field bounds, the digits (read out of the lanes one by one) -- is scalar work.  The checksum is an XOR reduction
// across the lanes.  Longer sentences take further steps.  The text is read as bytes, each inside [offset, offset + length)
// of its table row, which the entry point holds inside the file: no load leaves the allocation.
//
// The kernel decides ONLY the plain form (parse_nmea.plain_form states it; the header repeats it) and answers
// EPA_NMEA_UNDECIDED for everything else: the host applies parse_sentence there.  In the plain form d and the digits of m are
// integers below 10^15, exact in float64, and so is the power of ten (at most 10^15): the IEEE division M / 10^k is
// float(m) bit for bit, and float(d) + that / 60 has no multiply to contract.  (-O3, no fast-math flag: keep it so.)
#include "epa_internal.h"

namespace {

constexpr int kWaves = epa::kBlock / 64;
constexpr int kCommas = 7;                           // RMC's fields 2 .. 5 lie between commas 2 .. 6 (comma 0 is byte 6)
constexpr unsigned long long kDigitBound = 1000000000000000ULL;  // 10^15
constexpr int kMaxDecimals = 15;
constexpr int kMaxField = 64;

__device__ const double kPow10[kMaxDecimals + 1] = {1e0, 1e1, 1e2,  1e3,  1e4,  1e5,  1e6,  1e7,
                                                    1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uniform(long long v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffLL));
  const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
  return ((long long)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ unsigned lane_byte(unsigned v, int j) { return (unsigned)__builtin_amdgcn_readlane((int)v, j); }

__device__ __forceinline__ int wave_xor(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v ^= __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ bool is_alnum(unsigned c) {
  return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
}
__device__ __forceinline__ int hex_value(unsigned c) {
  if (c >= '0' && c <= '9') return (int)(c - '0');
  if (c >= 'A' && c <= 'F') return (int)(c - 'A') + 10;
  if (c >= 'a' && c <= 'f') return (int)(c - 'a') + 10;
  return -1;
}

enum { kValueOk = 0, kValueFails = 1, kValueUndecided = 2 };

// R5 without the sign on the field s[0, L): wave-uniform.  The field's bytes sit in the lanes (lane j: byte j).
__device__ __forceinline__ int parse_value(const uint8_t* __restrict__ s, long long L64, int lane, double* out) {
  *out = 0.0;
  if (L64 == 0) return kValueOk;
  if (L64 > kMaxField) return kValueUndecided;
  const int L = (int)L64;
  const unsigned fb = lane < L ? s[lane] : 0u;
  const unsigned long long all = L == 64 ? ~0ULL : ((1ULL << L) - 1ULL);
  const unsigned long long dig = __ballot(fb >= '0' && fb <= '9');  // (lanes behind the field hold 0: no digit)
  const unsigned long long dot = __ballot(fb == '.');
  if (L == 1 && lane_byte(fb, 0) == '0') return kValueOk;
  if (__popcll(dot) != 1) return kValueFails;
  const int p = __ffsll((long long)dot) - 1;
  if (p < 3 || p > L - 2 || (dig | dot) != all) return kValueFails;  // \d+ \d\d . \d+
  const int k = L - 1 - p;
  unsigned long long D = 0, M = 0;
  for (int j = 0; j < p - 2; ++j) {
    D = D * 10ULL + (lane_byte(fb, j) - '0');
    if (D >= kDigitBound) return kValueUndecided;
  }
  for (int j = p - 2; j < L; ++j) {
    if (j == p) continue;
    M = M * 10ULL + (lane_byte(fb, j) - '0');
    if (M >= kDigitBound) return kValueUndecided;
  }
  if (k > kMaxDecimals) return kValueUndecided;
  *out = (double)D + ((double)M / kPow10[k]) / 60.0;
  return kValueOk;
}

__global__ void __launch_bounds__(epa::kBlock)
nmea_positions_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ table, long long n,
                      double* __restrict__ lat_out, double* __restrict__ lon_out, uint8_t* __restrict__ code_out) {
  const int lane = threadIdx.x & 63;
  const int wave = uniform((int)(threadIdx.x >> 6));
  const long long i = (long long)blockIdx.x * kWaves + wave;  // wave-uniform
  if (i >= n) return;
  const long long len = uniform((long long)table[2 * i + 1]);
  const uint8_t* __restrict__ s = bytes + uniform((long long)table[2 * i]);

  // ---- one pass over the text: the masks of every 64-byte step ----
  long long comma[kCommas];
#pragma unroll
  for (int j = 0; j < kCommas; ++j) comma[j] = -1;
  int ncomma = 0, nstar = 0, x = 0;
  long long star = -1, last_nonws = -1, first_bad = -1;
  for (long long base = 0; base < len; base += 64) {
    const bool in = base + lane < len;
    const unsigned c = in ? s[base + lane] : 0u;
    const bool ws = c == ' ' || c == '\t' || c == '\r' || c == '\n';
    const unsigned long long m_comma = __ballot(in && c == ',');
    const unsigned long long m_star = __ballot(in && c == '*');
    const unsigned long long m_nonws = __ballot(in && !ws);
    const unsigned long long m_bad = __ballot(in && (c < 0x20u || c > 0x7Eu));
    // the checksum covers byte 1 up to the byte in front of the first star
    unsigned long long m_x = star >= 0 ? 0ULL : (m_star ? ((m_star & (~m_star + 1ULL)) - 1ULL) : ~0ULL);
    if (base == 0) m_x &= ~1ULL;
    x ^= wave_xor(((m_x >> lane) & 1ULL) ? (int)c : 0);
    if (star < 0 && m_star) star = base + (__ffsll((long long)m_star) - 1);
    nstar += __popcll(m_star);
    unsigned long long mc = m_comma;
#pragma unroll
    for (int j = 0; j < kCommas; ++j) {
      if (ncomma == j && mc) {
        comma[j] = base + (__ffsll((long long)mc) - 1);
        mc &= mc - 1ULL;
        ++ncomma;
      }
    }
    if (m_nonws) last_nonws = base + 63 - __clzll((long long)m_nonws);
    if (first_bad < 0 && m_bad) first_bad = base + (__ffsll((long long)m_bad) - 1);
  }

  // ---- the plain form ----
  const unsigned hb = (lane < 7 && lane < len) ? s[lane] : 0u;
  unsigned h[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) h[j] = lane_byte(hb, j);
  int type = -1;
  if (h[3] == 'G' && h[4] == 'G' && h[5] == 'A') type = EPA_NMEA_GGA;
  if (h[3] == 'G' && h[4] == 'L' && h[5] == 'L') type = EPA_NMEA_GLL;
  if (h[3] == 'R' && h[4] == 'M' && h[5] == 'C') type = EPA_NMEA_RMC;
  bool plain = len >= 7 && h[0] == '$' && h[6] == ',' && is_alnum(h[1]) && is_alnum(h[2]) && h[1] != 'P' && h[1] != 'p' &&
               type >= 0;
  // non-printable bytes only in the trailing run: the FIRST of them stands behind the last byte that is no white space
  plain = plain && (first_bad < 0 || first_bad > last_nonws) && nstar <= 1;
  const long long content_end = last_nonws + 1;
  long long data_end = len;
  bool checksum_ok = true;
  if (plain && nstar == 1) {
    plain = content_end == star + 3;
    if (plain) {
      const int hi = hex_value(s[star + 1]), lo = hex_value(s[star + 2]);  // (both in front of content_end <= len)
      plain = hi >= 0 && lo >= 0;
      checksum_ok = ((hi << 4) | lo) == x;
    }
    data_end = star;
  }

  double lat = 0.0, lon = 0.0;
  int lat_state = kValueOk, lon_state = kValueOk;
  if (plain) {
    const int k0 = type == EPA_NMEA_GGA ? 1 : type == EPA_NMEA_GLL ? 0 : 2;  // the latitude's field; then lat_dir, lon, lon_dir
    long long cpos[5];  // the commas in front of the four fields and behind the last
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      long long v = -1;
#pragma unroll
      for (int j = 0; j < kCommas; ++j) v = (j == k0 + f) ? comma[j] : v;
      cpos[f] = (v >= 0 && v < data_end) ? v : -1;
    }
    // without a star the data run to the end of the text, the trailing run included: decided only when that run cannot
    // belong to one of the four fields
    if (nstar == 0 && content_end != len && cpos[4] < 0) plain = false;
    long long fs[4], fl[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      fs[f] = cpos[f] < 0 ? 0 : cpos[f] + 1;
      fl[f] = cpos[f] < 0 ? 0 : (cpos[f + 1] >= 0 ? cpos[f + 1] : data_end) - fs[f];
    }
    if (plain) {
      lat_state = parse_value(s + fs[0], fl[0], lane, &lat);
      lon_state = parse_value(s + fs[2], fl[2], lane, &lon);
      const unsigned lat_dir = fl[1] == 1 ? (unsigned)s[fs[1]] : 0u;
      const unsigned lon_dir = fl[3] == 1 ? (unsigned)s[fs[3]] : 0u;
      lat = lat_dir == 'N' ? lat : lat_dir == 'S' ? -lat : 0.0;
      lon = lon_dir == 'E' ? lon : lon_dir == 'W' ? -lon : 0.0;
    }
  }
  const double nan = __longlong_as_double(0x7FF8000000000000LL);  // Python's math.nan
  unsigned code;
  if (!plain || lat_state == kValueUndecided || lon_state == kValueUndecided) {
    code = EPA_NMEA_UNDECIDED;
    lat = lon = nan;
  } else if (!checksum_ok) {
    code = EPA_NMEA_INVALID;
    lat = lon = nan;
  } else {
    code = (unsigned)type << EPA_NMEA_TYPE_SHIFT;
    if (lat_state == kValueFails) { code |= EPA_NMEA_LAT_FAILED; lat = nan; }
    if (lon_state == kValueFails) { code |= EPA_NMEA_LON_FAILED; lon = nan; }
  }
  if (lane == 0) {
    lat_out[i] = lat;
    lon_out[i] = lon;
    code_out[i] = (uint8_t)code;
  }
}

}  // namespace

extern "C" int epa_nmea_positions(const uint8_t* bytes, long long n_bytes, long long n_alloc, const int64_t* table_host,
                                  const int64_t* table, long long n, double* lat, double* lon, uint8_t* code,
                                  epa_stream_t stream) {
  EPA_CHECK_ARG(n >= 0 && n <= 0x7fffffffLL * kWaves, "epa_nmea_positions: n=%lld sentences are not served", n);
  EPA_CHECK_ARG(n_bytes >= 0 && n_alloc >= n_bytes && n_alloc % 16 == 0,
                "epa_nmea_positions: the file buffer must be padded to a multiple of 16 bytes (n_bytes=%lld, n_alloc=%lld)",
                n_bytes, n_alloc);
  if (n == 0) return EPA_OK;
  EPA_CHECK_ARG(bytes && table_host && table && lat && lon && code, "epa_nmea_positions: NULL array argument");
  for (long long r = 0; r < n; ++r) {
    const long long off = table_host[2 * r], len = table_host[2 * r + 1];
    EPA_CHECK_ARG(off >= 0 && len >= 0 && off <= n_bytes && len <= n_bytes - off,
                  "epa_nmea_positions: sentence %lld (offset %lld, %lld bytes) leaves the %lld file bytes", r, off, len,
                  n_bytes);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((n + kWaves - 1) / kWaves)), block(epa::kBlock);
  hipLaunchKernelGGL(nmea_positions_kernel, grid, block, 0, st, bytes, table, n, lat, lon, code);
  return epa::check_launch("nmea_positions_kernel");
}
