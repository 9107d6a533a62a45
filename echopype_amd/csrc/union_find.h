// Lock-free union-find on a parent array in global memory, shared by the connected-component labellings
// (seafloor.hip: pixels of a crop; shoal.hip: pixels of a plane, and components of a plane).
//
// Links always point to a smaller index (atomic min on the root), so the forest has no cycles and a find is bounded
// by the number of elements; finds of a merge pass halve their paths with plain stores (a halving write only ever
// replaces a non-root's parent by one of its ancestors).  A compression pass that follows must store roots only
// (uf_root: a halving store there could overwrite a root another thread has just stored).  No workgroup waits for
// another: nothing relies on all of them being resident.  Each retry loop has a bound (the element count: a correct
// run cannot reach it); a loop that reaches it counts into an error word the host turns into an exception.
// I: long long or int (a negative parent marks an element outside every set; such elements are never passed in).
#pragma once
#include <hip/hip_runtime.h>

namespace epa {
namespace uf {

template <typename I>
__device__ __forceinline__ I ld(const I* a) {
  return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename I>
__device__ __forceinline__ void st(I* a, I v) {
  __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename I>
__device__ I uf_find(I* par, I x, I bound, unsigned long long* err) {
  for (I steps = 0; steps <= bound; ++steps) {
    const I p = ld(par + x);
    if (p == x) return x;
    const I g = ld(par + p);
    if (g != p) st(par + x, g);  // path halving
    x = g;
  }
  atomicAdd(err, 1ull);
  return x;
}

// the root of x without writing anything (the compression pass: a halving store that lands after another thread has
// stored its element's root would leave that element pointing at a non-root)
template <typename I>
__device__ I uf_root(const I* par, I x, I bound, unsigned long long* err) {
  for (I steps = 0; steps <= bound; ++steps) {
    const I p = ld(par + x);
    if (p == x) return x;
    x = p;
  }
  atomicAdd(err, 1ull);
  return x;
}

template <typename I>
__device__ void uf_union(I* par, I a, I b, I bound, unsigned long long* err) {
  for (I it = 0; it <= bound; ++it) {
    a = uf_find(par, a, bound, err);
    b = uf_find(par, b, bound, err);
    if (a == b) return;
    if (a < b) {
      const I t = a;
      a = b;
      b = t;
    }
    // link the larger root under the smaller one; a changed root means somebody linked it meanwhile: go on from there
    const I old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
  atomicAdd(err, 1ull);
}

}  // namespace uf
}  // namespace epa
