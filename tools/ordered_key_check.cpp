// Stand-alone check of echopype_amd/csrc/ordered_key.h (the plain C++ part: nothing of HIP), built by
// tests/test_ordered_key_host.py with -fsanitize=address,undefined.  For double and float: the round trip is exact in
// the bits, the map is strictly increasing over the non-NaN values (-0.0 below +0.0), no number maps to a sentinel and
// +-inf lie strictly inside them.  Exit status 0 and "ok" when every statement of the header's contract holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <type_traits>
#include <vector>

#include "ordered_key.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (++failures <= 20) {                     \
        std::printf("FAILED %s: ", #cond);        \
        std::printf(__VA_ARGS__);                 \
        std::printf("\n");                        \
      }                                           \
    }                                             \
  } while (0)

template <typename T>
struct Traits;
template <>
struct Traits<double> {
  using U = unsigned long long;
  static constexpr const char* name = "double";
  static constexpr U no_max = epa::kKeyNoMax, no_min = epa::kKeyNoMin;
};
template <>
struct Traits<float> {
  using U = unsigned;
  static constexpr const char* name = "float";
  // the 32-bit keys are radix digits only (no slot starts at a sentinel): the same two patterns, by the same argument
  static constexpr U no_max = 0u, no_min = ~0u;
};

template <typename T, typename U>
U bits_of(T x) {
  U u;
  static_assert(sizeof(u) == sizeof(x), "same width");
  std::memcpy(&u, &x, sizeof(u));
  return u;
}
template <typename T, typename U>
T from_bits(U u) {
  T x;
  std::memcpy(&x, &u, sizeof(x));
  return x;
}

template <typename T>
void check_type(unsigned seed) {
  using U = typename Traits<T>::U;
  using L = std::numeric_limits<T>;
  const char* nm = Traits<T>::name;
  static_assert(std::is_same<decltype(epa::ordered_key(T())), U>::value, "key type");
  static_assert(std::is_same<decltype(epa::key_value(U())), T>::value, "value type");

  // the edge values, in increasing order
  const std::vector<T> edges = {-L::infinity(), -L::max(), T(-1), -L::min(), -L::denorm_min(), T(-0.0), T(0.0),
                                L::denorm_min(), L::min(), T(1), L::max(), L::infinity()};
  auto check_value = [&](T x) {
    const U k = epa::ordered_key(x);
    const T back = epa::key_value(k);
    CHECK((bits_of<T, U>(back) == bits_of<T, U>(x)), "%s round trip of bits %llx", nm, (unsigned long long)bits_of<T, U>(x));
    CHECK(k != Traits<T>::no_max && k != Traits<T>::no_min, "%s bits %llx map to a sentinel", nm,
          (unsigned long long)bits_of<T, U>(x));
  };
  for (T x : edges) check_value(x);
  for (size_t i = 0; i + 1 < edges.size(); ++i) {
    // (-0.0 < +0.0 is false as values; the keys order the pair all the same)
    CHECK(epa::ordered_key(edges[i]) < epa::ordered_key(edges[i + 1]), "%s edge %zu !< edge %zu", nm, i, i + 1);
  }
  CHECK(epa::ordered_key(T(-0.0)) < epa::ordered_key(T(0.0)), "%s -0.0 !< +0.0", nm);
  CHECK(Traits<T>::no_max < epa::ordered_key(-L::infinity()), "%s -inf at the 'no maximum' sentinel", nm);
  CHECK(epa::ordered_key(L::infinity()) < Traits<T>::no_min, "%s +inf at the 'no minimum' sentinel", nm);

  // 100 000 random bit patterns without the NaNs, and 100 000 random pairs of them
  std::mt19937_64 rng(seed);
  std::vector<T> batch;
  while (batch.size() < 100000) {
    const T x = from_bits<T, U>((U)rng());
    if (x == x) batch.push_back(x);
  }
  for (T x : batch) check_value(x);
  std::uniform_int_distribution<size_t> pick(0, batch.size() - 1);
  size_t ordered = 0;
  for (int i = 0; i < 100000; ++i) {
    const T x = batch[pick(rng)], y = batch[pick(rng)];
    if (x < y) {
      ++ordered;
      CHECK(epa::ordered_key(x) < epa::ordered_key(y), "%s pair %d: x < y but not the keys", nm, i);
    } else if (y < x) {
      ++ordered;
      CHECK(epa::ordered_key(y) < epa::ordered_key(x), "%s pair %d: y < x but not the keys", nm, i);
    }
  }
  CHECK(ordered > 90000, "%s: only %zu of the random pairs were ordered", nm, ordered);
  // and over the whole batch at once: sorted by value == sorted by key
  std::vector<T> by_value = batch;
  std::sort(by_value.begin(), by_value.end());
  for (size_t i = 0; i + 1 < by_value.size(); ++i)
    if (by_value[i] < by_value[i + 1])
      CHECK(epa::ordered_key(by_value[i]) < epa::ordered_key(by_value[i + 1]), "%s sorted batch at %zu", nm, i);
  std::printf("%s: %zu edge values, %zu random values, %zu ordered pairs\n", nm, edges.size(), batch.size(), ordered);
}

}  // namespace

int main() {
  static_assert(epa::kKeyNoMax == 0ull && epa::kKeyNoMin == ~0ull, "the sentinels");
  check_type<double>(20240611u);
  check_type<float>(20240612u);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
