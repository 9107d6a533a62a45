// Shoal detection (mask.detect_shoal): the "weill" and "echoview" school masks of one (ping, range) plane.
//
// Reference arithmetic replaced (echopype, mask/shoal_detection/):
//   both                 Sv > thr in f64 (NaN background)                           -> sh_threshold_vfill_kernel
//   shoal_weill.py       background runs along range of length <= maxvgap that have foreground on both sides become
//                        foreground                                              -> sh_threshold_vfill_kernel
//                        the same along pings with maxhgap, on that result       -> sh_hfill_kernel
//                        scipy.ndimage.label (4-connectivity); components whose extent in samples < minvlen or in
//                        pings < minhlen removed                                 -> sh_cc_*, sh_box_kernel,
//                                                                                   sh_weill_keep_kernel, sh_final_kernel
//   shoal_echoview.py    label (8-connectivity); height / width of a component from idim / jdim at its bounding box;
//                        candidates below mincan removed                         -> sh_cc_*, sh_box_kernel,
//                                                                                   sh_candidate_kernel
//                        linking: every component's box grown by maxlink + 1 (nearest idim / jdim entries); the
//                        surviving components with a pixel inside it get one label, transitively
//                                                                                -> sh_link_kernel, sh_link_big_kernel
//                        linked groups below minsho removed; a component no box ever met is kept as it is
//                                                                                -> sh_group_box_kernel,
//                                                                                   sh_group_keep_kernel, sh_final_kernel
//
// Planes are (ping, range) as stored, range contiguous: "vertical" is along range_sample, "horizontal" along pings.
// Neither result depends on label numbers, only on the partition into components.
//
// Labelling is the union-find of union_find.h over pixels.  After path compression the roots are numbered by an atomic
// counter, and every foreground pixel's parent word is rewritten to the code -(id + 2) of its component (-1 stays
// background): later passes read one word per pixel.  The per-component table (bounding box, group parent, flag) is
// indexed by that id; its capacity is the largest number of components the plane can hold (every second pixel with
// 4-connectivity, every second pixel of every second ping with 8-connectivity), so no count has to reach the host
// before the table exists.  Echoview's linking is a second union-find, over component ids.
#include "epa_internal.h"
#include "union_find.h"

namespace {

using epa::uf::ld;
using epa::uf::st;
using epa::uf::uf_root;
using epa::uf::uf_union;

constexpr int kWaves = epa::kBlock / 64;
constexpr int kMaxBlocks = 16384;
constexpr int kHChunk = 128;               // pings walked by one thread of the horizontal fill
constexpr long long kBigArea = 1 << 16;    // link boxes above this many pixels are scanned by the whole grid
constexpr int kBigBlocks = 2048;

// state words (EPA_SHOAL_STATE_WORDS u64, zeroed by the caller)
enum : int {
  kError = EPA_SHOAL_STATE_ERROR,  // union-find loops that reached their bound, component ids beyond the table
  kCount = EPA_SHOAL_STATE_COUNT,  // components numbered
  kBig = 2,    // link boxes queued for the whole-grid scan
};

inline int blocks_for(long long n) {
  long long b = (n + epa::kBlock - 1) / epa::kBlock;
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}
inline int blocks_for_waves(long long waves) {
  long long b = (waves + kWaves - 1) / kWaves;
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// the component table: box[0..3][cap] = min sample, max sample, min ping, max ping
struct Table {
  int* box;
  int* gpar;  // echoview: parent of the component-level union-find, -1 for a removed candidate (NULL for weill)
  int* flag;  // echoview: met by a link box, then "kept"; weill: "kept"
  int cap;
};

__device__ __forceinline__ int comp_count(const unsigned long long* state, int cap) {
  const unsigned long long n = state[kCount];
  return n < (unsigned long long)cap ? (int)n : cap;
}

// ---- threshold and vertical fill: one wave per ping, 64 samples per step -----------------------------------------------
// A background sample becomes foreground when the nearest foreground samples on both sides exist and are at most
// maxvgap + 1 apart.  Inside a step both neighbours come from the ballot; a run that closes in a later step is filled
// by that step (last = the ping's last foreground sample so far), over the samples of the earlier steps.
template <typename T>
__global__ __launch_bounds__(epa::kBlock) void sh_threshold_vfill_kernel(const T* __restrict__ sv, long long P,
                                                                          long long S, double thr, long long maxvgap,
                                                                          unsigned char* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long above = lane == 63 ? 0ull : ~((2ull << lane) - 1ull);
  for (long long p = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); p < P; p += (long long)gridDim.x * kWaves) {
    const T* row = sv + p * S;
    unsigned char* orow = out + p * S;
    long long last = -1;
    for (long long base = 0; base < S; base += 64) {
      const long long s = base + lane;
      const bool fg = s < S && (double)row[s] > thr;  // in f64, as np.ma compares; NaN compares false
      const unsigned long long b = __ballot(fg);
      const unsigned long long lo = b & below, hi = b & above;
      const long long prev = lo ? base + 63 - __clzll((long long)lo) : last;
      const long long next = hi ? base + (__ffsll((long long)hi) - 1) : -1;
      const bool fill = prev >= 0 && next >= 0 && next - prev - 1 <= maxvgap;
      if (s < S) orow[s] = (fg || fill) ? 1 : 0;
      if (b) {
        const long long first = base + (__ffsll((long long)b) - 1);
        if (last >= 0 && first - last - 1 <= maxvgap) {
          for (long long t = last + 1 + lane; t < base; t += 64) orow[t] = 1;  // (empty when last is in this step's reach)
        }
        last = base + 63 - __clzll((long long)b);
      }
    }
  }
}

// ---- horizontal fill, in place: lanes own adjacent samples, a thread walks kHChunk pings ----------------------------
// A thread fills the runs that CLOSE in its chunk, backwards, also over the pings of earlier chunks; it finds the last
// foreground ping before its chunk by looking back at most maxhgap + 1 pings.  Bytes that another thread fills meanwhile
// can only make a reader fill a part of the same run early: every byte written belongs to a run that is filled whole.
__global__ __launch_bounds__(epa::kBlock) void sh_hfill_kernel(unsigned char* plane, long long P, long long S,
                                                               long long maxhgap) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  for (long long c0 = (long long)blockIdx.y * kHChunk; c0 < P; c0 += (long long)gridDim.y * kHChunk) {
    const long long c1 = c0 + kHChunk < P ? c0 + kHChunk : P;
    long long last = -1;
    const long long back = c0 - maxhgap - 1 > 0 ? c0 - maxhgap - 1 : 0;
    for (long long p = c0 - 1; p >= back; --p) {
      if (plane[p * S + s]) {
        last = p;
        break;
      }
    }
    for (long long p = c0; p < c1; ++p) {
      if (!plane[p * S + s]) continue;
      if (last >= 0 && p - last - 1 <= maxhgap) {
        for (long long t = last + 1; t < p; ++t) plane[t * S + s] = 1;
      }
      last = p;
    }
  }
}

// ---- connected components of the u8 plane (4- or 8-connectivity) ------------------------------------------------------
__global__ __launch_bounds__(epa::kBlock) void sh_cc_init_kernel(const unsigned char* __restrict__ plane, long long n,
                                                                 long long* __restrict__ par) {
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x)
    par[q] = plane[q] ? q : -1;
}

template <bool kDiagonal>
__global__ __launch_bounds__(epa::kBlock) void sh_cc_merge_kernel(long long* par, long long P, long long S,
                                                                  unsigned long long* err) {
  const long long n = P * S;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    if (ld(par + q) < 0) continue;
    const long long p = q / S, i = q - p * S;
    if (i > 0 && ld(par + q - 1) >= 0) uf_union(par, q, q - 1, n, err);
    if (p > 0) {
      const long long u = q - S;
      if (kDiagonal && i > 0 && ld(par + u - 1) >= 0) uf_union(par, q, u - 1, n, err);
      if (ld(par + u) >= 0) uf_union(par, q, u, n, err);
      if (kDiagonal && i + 1 < S && ld(par + u + 1) >= 0) uf_union(par, q, u + 1, n, err);
    }
  }
}

__global__ __launch_bounds__(epa::kBlock) void sh_cc_compress_kernel(long long* par, long long n,
                                                                     unsigned long long* err) {
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    if (ld(par + q) < 0) continue;
    st(par + q, uf_root(par, q, n, err));  // only roots are stored: every pixel ends on its root
  }
}

// every root takes the next id, writes its code -(id + 2) over its own parent word and resets its table entry
__global__ __launch_bounds__(epa::kBlock) void sh_cc_number_kernel(long long* par, long long n, Table t,
                                                                   unsigned long long* state) {
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    if (par[q] != q) continue;
    const unsigned long long id = atomicAdd(&state[kCount], 1ull);
    if (id >= (unsigned long long)t.cap) {  // cannot happen (the capacity is the combinatorial bound): never write past it
      atomicAdd(&state[kError], 1ull);
      par[q] = -1;
      continue;
    }
    par[q] = -((long long)id + 2);
    t.box[id] = 0x7fffffff;
    t.box[(size_t)t.cap + id] = -1;
    t.box[2 * (size_t)t.cap + id] = 0x7fffffff;
    t.box[3 * (size_t)t.cap + id] = -1;
    t.flag[id] = 0;
  }
}

// Bounding boxes, and the parent word of every pixel rewritten to its component's code.  One wave per 64 samples of a
// ping: lanes of one run of equal ids reduce to the run's head, which updates the box only where it grows it (one
// large school would otherwise put every pixel's four atomics on one address).
__global__ __launch_bounds__(epa::kBlock) void sh_box_kernel(long long* par, long long P, long long S, Table t) {
  const int lane = threadIdx.x & 63;
  const long long segs = (S + 63) / 64, items = P * segs;
  for (long long w = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); w < items; w += (long long)gridDim.x * kWaves) {
    const long long p = w / segs, i = (w - p * segs) * 64 + lane;
    long long code = -1;
    if (i < S) {
      const long long q = p * S + i;
      code = par[q];
      if (code >= 0) {  // a pixel under a root: the root already carries its code (it was background if the table overflowed)
        code = par[code];
        par[q] = code;
      }
    }
    const long long left = __shfl_up(code, 1, 64);
    const bool head = code <= -2 && (lane == 0 || left != code);
    const unsigned long long heads = __ballot(head || code > -2);  // run ends: the next head or the next background lane
    if (head) {
      const unsigned long long after = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
      const int end = after ? __ffsll((long long)after) - 2 : 63;  // last lane of this run
      const int id = (int)(-code - 2);
      const int i0 = (int)i, i1 = (int)(i + (end - lane)), pp = (int)p;
      int* b = t.box;
      const size_t cap = (size_t)t.cap;
      if (i0 < ld(b + id)) atomicMin(b + id, i0);
      if (i1 > ld(b + cap + id)) atomicMax(b + cap + id, i1);
      if (pp < ld(b + 2 * cap + id)) atomicMin(b + 2 * cap + id, pp);
      if (pp > ld(b + 3 * cap + id)) atomicMax(b + 3 * cap + id, pp);
    }
  }
}

// ---- weill: extents in indices -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(epa::kBlock) void sh_weill_keep_kernel(Table t, const unsigned long long* __restrict__ state,
                                                                    double minvlen, double minhlen) {
  const int n = comp_count(state, t.cap);
  const size_t cap = (size_t)t.cap;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
    const double vlen = (double)(t.box[cap + c] - t.box[c] + 1);
    const double hlen = (double)(t.box[3 * cap + c] - t.box[2 * cap + c] + 1);
    t.flag[c] = ((vlen < minvlen) || (hlen < minhlen)) ? 0 : 1;
  }
}

// ---- echoview ------------------------------------------------------------------------------------------------------------
struct Axes {
  const double* idim;  // ni >= S + 1 entries, nondecreasing
  const double* jdim;  // nj >= P + 1
  int ni, nj;
};

// height / width of a box in idim / jdim units; true when it is below (min0, min1)
__device__ __forceinline__ bool too_small(const Axes& ax, int i0, int i1, int j0, int j1, double min0, double min1) {
#pragma clang fp contract(off)
  const double height = ax.idim[i1 + 1] - ax.idim[i0];
  const double width = ax.jdim[j1 + 1] - ax.jdim[j0];
  return (height < min0) || (width < min1);
}

// np.argmin(abs(x - t)) of a nondecreasing x: the FIRST index of the smallest float64 |x[k] - t|.  |x[k] - t| as
// computed falls (weakly) up to the first x[k] >= t and rises (weakly) from there, so the minimum is at that entry or
// the one before; equal distances on the falling side are resolved to their first index by a second search.
__device__ int first_argmin_abs(const double* __restrict__ x, int n, double t) {
#pragma clang fp contract(off)
  int lo = 0, hi = n;  // first index with x >= t
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (x[mid] < t) lo = mid + 1; else hi = mid;
  }
  const int right = lo;
  if (right == 0) return 0;
  const double dl = fabs(x[right - 1] - t);
  if (right < n && fabs(x[right] - t) < dl) return right;
  lo = 0;
  hi = right - 1;  // first index whose distance is already dl
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (fabs(x[mid] - t) > dl) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(epa::kBlock) void sh_candidate_kernel(Table t, const unsigned long long* __restrict__ state,
                                                                   Axes ax, double mincan0, double mincan1) {
  const int n = comp_count(state, t.cap);
  const size_t cap = (size_t)t.cap;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
    const bool small = too_small(ax, t.box[c], t.box[cap + c], t.box[2 * cap + c], t.box[3 * cap + c], mincan0, mincan1);
    t.gpar[c] = small ? -1 : c;
  }
}

struct LinkBox {
  int i0, i1, j0, j1;  // [i0, i1) x [j0, j1)
};

__device__ LinkBox link_box(const Table& t, int c, const Axes& ax, long long P, long long S, double link0,
                            double link1) {
#pragma clang fp contract(off)
  const size_t cap = (size_t)t.cap;
  const int i_min = t.box[c], i_max = t.box[cap + c], j_min = t.box[2 * cap + c], j_max = t.box[3 * cap + c];
  LinkBox b;
  b.i0 = first_argmin_abs(ax.idim, ax.ni, ax.idim[i_min] - (link0 + 1.0));
  b.i1 = first_argmin_abs(ax.idim, ax.ni, ax.idim[i_max] + (link0 + 1.0)) + 1;
  b.j0 = first_argmin_abs(ax.jdim, ax.nj, ax.jdim[j_min] - (link1 + 1.0));
  b.j1 = first_argmin_abs(ax.jdim, ax.nj, ax.jdim[j_max] + (link1 + 1.0)) + 1;
  if (b.i1 > S) b.i1 = (int)S;  // the slice [i0:i1, j0:j1] of the plane
  if (b.j1 > P) b.j1 = (int)P;
  if (b.i0 > b.i1) b.i0 = b.i1;
  if (b.j0 > b.j1) b.j0 = b.j1;
  return b;
}

// One wave scans the pings [j0, j1) step jstep of a link box.  Every surviving component met is flagged and joined to
// the first one met (the anchor): the neighbour set of a box becomes one group.  *shared (a box scanned by many
// waves): the first wave to meet a component publishes it as the anchor of all.  A lane skips the component it joined
// last, which removes nearly every union inside a large school.
__device__ void scan_box(const long long* __restrict__ par, long long S, const LinkBox& b, int jfirst, int jstep,
                         Table t, int ncomp, int* shared, unsigned long long* err) {
  const int lane = threadIdx.x & 63;
  int anchor = -1, prev = -1;
  for (int j = jfirst; j < b.j1; j += jstep) {
    const long long* row = par + (long long)j * S;
    for (int base = b.i0; base < b.i1; base += 64) {
      const int i = base + lane;
      int id = -1;
      if (i < b.i1) {
        const long long code = row[i];
        if (code <= -2) {
          id = (int)(-code - 2);
          if (ld(t.gpar + id) < 0) id = -1;  // a removed candidate
        }
      }
      const unsigned long long found = __ballot(id >= 0);
      if (!found) continue;
      if (anchor < 0) {
        anchor = __shfl(id, __ffsll((long long)found) - 1, 64);
        if (shared) {
          int seen = anchor;
          if (lane == 0) {
            const int old = atomicCAS(shared, -1, anchor);
            if (old >= 0) seen = old;
          }
          anchor = __shfl(seen, 0, 64);
        }
      }
      if (id >= 0 && id != prev) {
        t.flag[id] = 1;
        if (id != anchor) uf_union(t.gpar, anchor, id, ncomp, err);
        prev = id;
      }
    }
  }
}

// one wave per surviving component; boxes above kBigArea pixels go to the queue of sh_link_big_kernel while it has room
__global__ __launch_bounds__(epa::kBlock) void sh_link_kernel(const long long* __restrict__ par, long long P, long long S,
                                                              Table t, Axes ax, double link0, double link1,
                                                              int* __restrict__ big, int bigcap,
                                                              unsigned long long* state) {
  const int lane = threadIdx.x & 63;
  const int n = comp_count(state, t.cap);
  for (long long c = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); c < n; c += (long long)gridDim.x * kWaves) {
    if (ld(t.gpar + c) < 0) continue;
    const LinkBox b = link_box(t, (int)c, ax, P, S, link0, link1);
    const long long area = (long long)(b.i1 - b.i0) * (long long)(b.j1 - b.j0);
    if (area == 0) continue;
    if (area > kBigArea) {
      int queued = 0;
      if (lane == 0) {
        const unsigned long long slot = atomicAdd(&state[kBig], 1ull);
        if (slot < (unsigned long long)bigcap) {
          big[2 * slot] = (int)c;
          big[2 * slot + 1] = -1;
          queued = 1;
        }
      }
      if (__shfl(queued, 0, 64)) continue;
    }
    scan_box(par, S, b, b.j0, 1, t, n, nullptr, &state[kError]);
  }
}

// the queued boxes one after another, the pings of each dealt over every wave of the grid
__global__ __launch_bounds__(epa::kBlock) void sh_link_big_kernel(const long long* __restrict__ par, long long P,
                                                                  long long S, Table t, Axes ax, double link0,
                                                                  double link1, int* big, int bigcap,
                                                                  unsigned long long* state) {
  const int n = comp_count(state, t.cap);
  const unsigned long long queued = state[kBig];
  const int nbig = queued < (unsigned long long)bigcap ? (int)queued : bigcap;
  const int wave = blockIdx.x * kWaves + (threadIdx.x >> 6), waves = gridDim.x * kWaves;
  for (int k = 0; k < nbig; ++k) {
    const LinkBox b = link_box(t, big[2 * k], ax, P, S, link0, link1);
    if (b.j0 + wave >= b.j1) continue;
    scan_box(par, S, b, b.j0 + wave, waves, t, n, big + 2 * k + 1, &state[kError]);
  }
}

// the box of a group: the members that a link box met fold their boxes into their root's (members' own boxes of
// non-roots are never written, and a root's only grows: in place)
__global__ __launch_bounds__(epa::kBlock) void sh_group_box_kernel(Table t, unsigned long long* state) {
  const int n = comp_count(state, t.cap);
  const size_t cap = (size_t)t.cap;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
    if (t.gpar[c] < 0 || !t.flag[c]) continue;
    const int g = uf_root(t.gpar, c, n, &state[kError]);
    if (g == c) continue;
    int* b = t.box;
    atomicMin(b + g, ld(b + c));
    atomicMax(b + cap + g, ld(b + cap + c));
    atomicMin(b + 2 * cap + g, ld(b + 2 * cap + c));
    atomicMax(b + 3 * cap + g, ld(b + 3 * cap + c));
  }
}

// flag: "met by a link box" -> "kept".  A component no box met (its own included) is kept whatever its size.
__global__ __launch_bounds__(epa::kBlock) void sh_group_keep_kernel(Table t, unsigned long long* state, Axes ax,
                                                                    double minsho0, double minsho1) {
  const int n = comp_count(state, t.cap);
  const size_t cap = (size_t)t.cap;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
    int keep = 0;
    if (t.gpar[c] >= 0) {
      keep = 1;
      if (t.flag[c]) {
        const int g = uf_root(t.gpar, c, n, &state[kError]);
        keep = too_small(ax, t.box[g], t.box[cap + g], t.box[2 * cap + g], t.box[3 * cap + g], minsho0, minsho1) ? 0 : 1;
      }
    }
    t.flag[c] = keep;
  }
}

// the boolean plane: foreground pixels of kept components
__global__ __launch_bounds__(epa::kBlock) void sh_final_kernel(const long long* __restrict__ par, long long n,
                                                               const int* __restrict__ flag,
                                                               unsigned char* __restrict__ plane) {
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    const long long code = par[q];
    plane[q] = (code <= -2 && flag[-code - 2]) ? 1 : 0;
  }
}

inline long long table_capacity(long long P, long long S, int connectivity) {
  return connectivity == 8 ? ((P + 1) / 2) * ((S + 1) / 2) : (P * S + 1) / 2;
}

}  // namespace

extern "C" int epa_shoal_threshold_fill(const void* sv, int dtype, long long P, long long S, double thr,
                                        long long maxvgap, long long maxhgap, unsigned char* plane,
                                        epa_stream_t stream) {
  const char* who = "epa_shoal_threshold_fill";
  EPA_CHECK_ARG(sv && plane, "%s: NULL array argument", who);
  EPA_CHECK_ARG(P > 0 && S > 0 && P < 0x7fffffffLL && S < 0x7fffffffLL, "%s: P=%lld S=%lld", who, P, S);
  EPA_CHECK_REAL(who, dtype);
  hipStream_t st = (hipStream_t)stream;
  if (maxvgap < 0) maxvgap = 0;  // no run is shorter than one sample,
  if (maxvgap > S) maxvgap = S;  // none longer than the axis
  if (maxhgap > P) maxhgap = P;
  const int rc = epa::dispatch_real(who, dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sh_threshold_vfill_kernel<T><<<blocks_for_waves(P), epa::kBlock, 0, st>>>((const T*)sv, P, S, thr, maxvgap, plane);
    return epa::check_launch("sh_threshold_vfill_kernel");
  });
  if (rc) return rc;
  if (maxhgap >= 1 && P > 2) {
    const long long chunks = (P + kHChunk - 1) / kHChunk;
    const dim3 grid((unsigned)((S + epa::kBlock - 1) / epa::kBlock), (unsigned)(chunks > 32768 ? 32768 : chunks));
    sh_hfill_kernel<<<grid, epa::kBlock, 0, st>>>(plane, P, S, maxhgap);
    if (int rc = epa::check_launch("sh_hfill_kernel")) return rc;
  }
  return EPA_OK;
}

static int check_table(const char* who, long long P, long long S, int connectivity, const int* box, const int* flag,
                       long long cap) {
  EPA_CHECK_ARG(P > 0 && S > 0 && P < 0x7fffffffLL && S < 0x7fffffffLL, "%s: P=%lld S=%lld", who, P, S);
  EPA_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity %d (4 or 8)", who, connectivity);
  EPA_CHECK_ARG(box && flag, "%s: NULL table argument", who);
  EPA_CHECK_ARG(cap >= table_capacity(P, S, connectivity) && cap <= 0x70000000LL,
                "%s: table capacity %lld (needs %lld, at most 0x70000000)", who, cap, table_capacity(P, S, connectivity));
  return EPA_OK;
}

extern "C" int epa_shoal_label(const unsigned char* plane, long long P, long long S, int connectivity,
                               long long* parent, int* box, int* flag, long long cap, unsigned long long* state,
                               epa_stream_t stream) {
  const char* who = "epa_shoal_label";
  EPA_CHECK_ARG(plane && parent && state, "%s: NULL array argument", who);
  if (int rc = check_table(who, P, S, connectivity, box, flag, cap)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const long long n = P * S;
  const int nb = blocks_for(n);
  const Table t{box, nullptr, flag, (int)cap};
  sh_cc_init_kernel<<<nb, epa::kBlock, 0, st>>>(plane, n, parent);
  if (int rc = epa::check_launch("sh_cc_init_kernel")) return rc;
  if (connectivity == 8) {
    sh_cc_merge_kernel<true><<<nb, epa::kBlock, 0, st>>>(parent, P, S, state + kError);
    if (int rc = epa::check_launch("sh_cc_merge_kernel<8>")) return rc;
  } else {
    sh_cc_merge_kernel<false><<<nb, epa::kBlock, 0, st>>>(parent, P, S, state + kError);
    if (int rc = epa::check_launch("sh_cc_merge_kernel<4>")) return rc;
  }
  sh_cc_compress_kernel<<<nb, epa::kBlock, 0, st>>>(parent, n, state + kError);
  if (int rc = epa::check_launch("sh_cc_compress_kernel")) return rc;
  sh_cc_number_kernel<<<nb, epa::kBlock, 0, st>>>(parent, n, t, state);
  if (int rc = epa::check_launch("sh_cc_number_kernel")) return rc;
  sh_box_kernel<<<blocks_for_waves(P * ((S + 63) / 64)), epa::kBlock, 0, st>>>(parent, P, S, t);
  return epa::check_launch("sh_box_kernel");
}

extern "C" int epa_shoal_weill_filter(const long long* parent, long long P, long long S, const int* box, int* flag,
                                      long long cap, double minvlen, double minhlen, unsigned long long* state,
                                      unsigned char* plane, epa_stream_t stream) {
  const char* who = "epa_shoal_weill_filter";
  EPA_CHECK_ARG(parent && plane && state, "%s: NULL array argument", who);
  if (int rc = check_table(who, P, S, 4, box, flag, cap)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const Table t{const_cast<int*>(box), nullptr, flag, (int)cap};
  sh_weill_keep_kernel<<<blocks_for(cap), epa::kBlock, 0, st>>>(t, state, minvlen, minhlen);
  if (int rc = epa::check_launch("sh_weill_keep_kernel")) return rc;
  sh_final_kernel<<<blocks_for(P * S), epa::kBlock, 0, st>>>(parent, P * S, flag, plane);
  return epa::check_launch("sh_final_kernel");
}

size_t epa::scratch::shoal_state(long long, long long, long long) {
  return sizeof(unsigned long long) * EPA_SHOAL_STATE_WORDS;
}
// the queue of large link boxes: two int32 words per box (sh_link_kernel fills it while it has room)
size_t epa::scratch::shoal_echoview_link_queue(long long, long long, long long) {
  return 2 * sizeof(int) * EPA_SHOAL_QUEUE_BOXES;
}

extern "C" int epa_shoal_echoview_link(const long long* parent, long long P, long long S, int* box, int* group,
                                       int* flag, long long cap, const double* idim, long long ni, const double* jdim,
                                       long long nj, double mincan0, double mincan1, double maxlink0,
                                       double maxlink1, double minsho0, double minsho1, int* queue, unsigned long long* state,
                                       unsigned char* plane, epa_stream_t stream) {
  const char* who = "epa_shoal_echoview_link";
  EPA_CHECK_ARG(parent && plane && state && group && queue && idim && jdim, "%s: NULL array argument", who);
  if (int rc = check_table(who, P, S, 8, box, flag, cap)) return rc;
  EPA_CHECK_ARG(ni > S && nj > P && ni < 0x7fffffffLL && nj < 0x7fffffffLL,
                "%s: idim needs at least S + 1 = %lld entries (has %lld), jdim P + 1 = %lld (has %lld)", who, S + 1, ni,
                P + 1, nj);
  hipStream_t st = (hipStream_t)stream;
  const Table t{box, group, flag, (int)cap};
  const Axes ax{idim, jdim, (int)ni, (int)nj};
  const int nc = blocks_for(cap);
  sh_candidate_kernel<<<nc, epa::kBlock, 0, st>>>(t, state, ax, mincan0, mincan1);
  if (int rc = epa::check_launch("sh_candidate_kernel")) return rc;
  sh_link_kernel<<<blocks_for_waves(cap), epa::kBlock, 0, st>>>(parent, P, S, t, ax, maxlink0, maxlink1, queue,
                                                               EPA_SHOAL_QUEUE_BOXES, state);
  if (int rc = epa::check_launch("sh_link_kernel")) return rc;
  sh_link_big_kernel<<<kBigBlocks, epa::kBlock, 0, st>>>(parent, P, S, t, ax, maxlink0, maxlink1, queue,
                                                        EPA_SHOAL_QUEUE_BOXES, state);
  if (int rc = epa::check_launch("sh_link_big_kernel")) return rc;
  sh_group_box_kernel<<<nc, epa::kBlock, 0, st>>>(t, state);
  if (int rc = epa::check_launch("sh_group_box_kernel")) return rc;
  sh_group_keep_kernel<<<nc, epa::kBlock, 0, st>>>(t, state, ax, minsho0, minsho1);
  if (int rc = epa::check_launch("sh_group_keep_kernel")) return rc;
  sh_final_kernel<<<blocks_for(P * S), epa::kBlock, 0, st>>>(parent, P * S, flag, plane);
  return epa::check_launch("sh_final_kernel");
}
