// The framing walk of a Simrad .raw file: a sequence of [int32 size][body of size bytes][int32 size], little endian,
// every body starting with char type[4]; uint32 low_date; uint32 high_date.  Plain C++ with no HIP include: the library
// exports it as epa_raw_index, tools/raw_index_check.cpp compiles it into a stand-alone program.
//
// Rules (echopype_amd.h, epa_raw_index): a size below 16 and a trailer that differs from the header are errors; a body
// or trailer that runs past the end -- a file cut while recording -- ends the walk, the complete datagrams before it
// stand.  No read goes outside [0, n_bytes), whatever the bytes are: every access is preceded by a comparison of the
// bytes left, in 64-bit arithmetic (a size is at most 2^31 - 1, so pos + 8 + size cannot wrap).
#pragma once
#include <cstdint>

#include "echopype_amd.h"

namespace epa_raw {

enum ScanCode { kScanOk = 0, kScanSizeTooSmall = 1, kScanTrailerDiffers = 2 };

struct ScanError {
  int code;
  int64_t offset;   // byte offset of the datagram's leading size field
  int32_t size;     // that field
  int32_t trailer;  // the trailing one (kScanTrailerDiffers)
};

inline uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// -> kScanOk or the error's code (err filled in).  records (may be NULL when capacity is 0) receives the first
// min(capacity, *n_records) records; *n_records is the number of complete datagrams found in any case, *n_consumed
// the offset behind the last of them.
inline int scan(const uint8_t* bytes, int64_t n_bytes, epa_raw_record* records, int64_t capacity, int64_t* n_records,
                int64_t* n_consumed, ScanError* err) {
  int64_t pos = 0, count = 0;
  int code = kScanOk;
  while (n_bytes - pos >= 4) {
    const int32_t size = (int32_t)le32(bytes + pos);
    if (size < 16) {
      *err = ScanError{kScanSizeTooSmall, pos, size, 0};
      code = kScanSizeTooSmall;
      break;
    }
    if (n_bytes - pos - 4 < (int64_t)size + 4) break;  // cut inside the body or the trailer
    const uint8_t* body = bytes + pos + 4;
    const int32_t trailer = (int32_t)le32(body + size);
    if (trailer != size) {
      *err = ScanError{kScanTrailerDiffers, pos, size, trailer};
      code = kScanTrailerDiffers;
      break;
    }
    if (count < capacity) {
      epa_raw_record& r = records[count];
      r.offset = pos + 4;
      r.size = size;
      r.type = le32(body);
      r.low_date = le32(body + 4);
      r.high_date = le32(body + 8);
      r.flags = (r.low_date == 0 && r.high_date == 0) ? EPA_RAW_ZERO_TIME : 0u;
      r.reserved = 0;
    }
    ++count;
    pos += (int64_t)size + 8;
  }
  *n_records = count;
  *n_consumed = pos;
  return code;
}

}  // namespace epa_raw
