// Stand-alone check of the .raw framing walk (echopype_amd/csrc/raw_index.h), meant to be built with
// -fsanitize=address,undefined:
//
//   raw_index_check FILE
//
// runs the scanner over FILE, over every prefix of it and over a deterministic set of single-byte corruptions of its
// size fields.  Every input is a heap copy of exactly its length, so a read outside [0, n_bytes) is a sanitizer report.
// Exit status 0: no report, and every record lies inside its input with the framing it claims; 1 otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "raw_index.h"

namespace {

int g_failures = 0;

void fail(const char* what, long long a, long long b) {
  if (g_failures++ < 20) std::fprintf(stderr, "FAIL %s (%lld, %lld)\n", what, a, b);
}

// scan an exact-size heap copy with the count-then-fill protocol; -> the number of datagrams
long long check(const uint8_t* src, int64_t n) {
  uint8_t* buf = static_cast<uint8_t*>(std::malloc(n ? (size_t)n : 1));  // (exactly n bytes: the redzone starts behind them)
  if (n) std::memcpy(buf, src, (size_t)n);
  int64_t count = -1, used = -1, count2 = -1, used2 = -1;
  epa_raw::ScanError err{}, err2{};
  const int code = epa_raw::scan(buf, n, nullptr, 0, &count, &used, &err);
  std::vector<epa_raw_record> rec((size_t)count + 1);
  const int code2 = epa_raw::scan(buf, n, rec.data(), count, &count2, &used2, &err2);
  if (code != code2 || count != count2 || used != used2) fail("the two calls disagree", count, count2);
  if (used < 0 || used > n) fail("n_consumed outside the input", used, n);
  int64_t pos = 0;
  for (int64_t i = 0; i < count; ++i) {
    const epa_raw_record& r = rec[(size_t)i];
    if (r.size < 16 || r.offset != pos + 4 || r.offset + r.size + 4 > n) fail("record outside the input or out of sequence", i, r.offset);
    else if (epa_raw::le32(buf + r.offset - 4) != (uint32_t)r.size || epa_raw::le32(buf + r.offset + r.size) != (uint32_t)r.size)
      fail("record does not match its size fields", i, r.offset);
    pos = r.offset + r.size + 4;
  }
  if (pos != used) fail("n_consumed is not the end of the last record", pos, used);
  if (code != epa_raw::kScanOk && (err.offset != used || err.offset + 4 > n)) fail("error offset", err.offset, used);
  std::free(buf);
  return count;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s FILE\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> data;
  uint8_t chunk[65536];
  for (size_t got; (got = std::fread(chunk, 1, sizeof chunk, f)) > 0;) data.insert(data.end(), chunk, chunk + got);
  std::fclose(f);
  const int64_t n = (int64_t)data.size();

  const long long whole = check(data.data(), n);
  std::printf("whole file: %lld datagrams in %lld bytes\n", whole, (long long)n);

  long long prefixes = 0;
  for (int64_t m = 0; m < n; ++m, ++prefixes)
    if (check(data.data(), m) > whole) fail("a prefix holds more datagrams than the file", m, whole);
  std::printf("%lld prefixes\n", prefixes);

  // the size fields of the whole file, each byte of each replaced by a few fixed values
  std::vector<epa_raw_record> rec((size_t)whole + 1);
  int64_t count = 0, used = 0;
  epa_raw::ScanError err{};
  epa_raw::scan(data.data(), n, rec.data(), whole, &count, &used, &err);
  static const uint8_t kValues[] = {0x00, 0x01, 0x0f, 0x10, 0x7f, 0x80, 0xff};
  long long corruptions = 0;
  std::vector<uint8_t> bad(data);
  for (int64_t i = 0; i < count; ++i) {
    const int64_t fields[2] = {rec[(size_t)i].offset - 4, rec[(size_t)i].offset + rec[(size_t)i].size};
    for (int64_t at : fields)
      for (int b = 0; b < 4; ++b)
        for (uint8_t v : kValues) {
          const uint8_t keep = bad[(size_t)(at + b)];
          if (keep == v) continue;
          bad[(size_t)(at + b)] = v;
          check(bad.data(), n);
          bad[(size_t)(at + b)] = keep;
          ++corruptions;
        }
  }
  std::printf("%lld corruptions of size fields\n", corruptions);
  if (g_failures) {
    std::fprintf(stderr, "%d failure(s)\n", g_failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
