// Internal helpers shared by the HIP translation units of libechopype_amd.so (gfx950 only).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <atomic>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "echopype_amd.h"

namespace epa {

void set_error(const char* fmt, ...);

#define EPA_CHECK_ARG(cond, ...)       \
  do {                                 \
    if (!(cond)) {                     \
      ::epa::set_error(__VA_ARGS__);   \
      return EPA_EINVAL;               \
    }                                  \
  } while (0)

#define EPA_CHECK_HIP(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      ::epa::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,  \
                       __LINE__);                                                        \
      return EPA_EHIP;                                                                   \
    }                                                                                    \
  } while (0)

// ---- element type of the samples (EPA_F32 / EPA_F64), chosen in ONE place ------------------------------------------
// Kernels are templates on the sample type; an entry instantiates both from one body:
//   return epa::dispatch_real(who, dtype, [&](auto tag) {
//     using T = typename decltype(tag)::type;
//     kernel<T><<<grid, block, 0, st>>>((const T*)x, (T)threshold, ...);
//     return epa::check_launch("kernel");
//   });
template <typename T>
struct type_tag {
  using type = T;
};

// the way back, for a template that calls a C-ABI entry
template <typename T>
constexpr int dtype_of = sizeof(T) == 8 ? EPA_F64 : EPA_F32;

inline bool is_real(int dtype) { return dtype == EPA_F32 || dtype == EPA_F64; }

// the argument check, at the place it has among an entry's other checks ("<entry>: bad dtype %d")
#define EPA_CHECK_REAL(who, dtype) EPA_CHECK_ARG(::epa::is_real(dtype), "%s: bad dtype %d", who, dtype)
#define EPA_CHECK_REAL_OUT(who, dtype) EPA_CHECK_ARG(::epa::is_real(dtype), "%s: bad output dtype %d", who, dtype)

// f(type_tag<double>{}) or f(type_tag<float>{}); any other dtype is an error, never a silent default
template <typename F>
int dispatch_real(const char* who, int dtype, F&& f) {
  if (dtype == EPA_F64) return f(type_tag<double>{});
  if (dtype == EPA_F32) return f(type_tag<float>{});
  set_error("%s: bad dtype %d", who, dtype);
  return EPA_EINVAL;
}

// Boolean template flags of a kernel, chosen in ONE place: f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...).
//   return epa::dispatch_flags([&](auto w, auto r) { return launch<T, decltype(w)::value, decltype(r)::value>(...); },
//                              sv_out != nullptr, rmax_key != nullptr);
// Every combination of the flags it is given is instantiated: a launcher that serves only some of them selects those
// itself and hands dispatch_flags the flags that are free.
template <typename F>
auto dispatch_flags(F&& f) {
  return f();
}
template <typename F, typename... Rest>
auto dispatch_flags(F&& f, bool b0, Rest... rest) {
  return b0 ? dispatch_flags([&](auto... t) { return f(std::true_type{}, t...); }, rest...)
            : dispatch_flags([&](auto... t) { return f(std::false_type{}, t...); }, rest...);
}

// A launch with more than 64 KiB of dynamic LDS has to be allowed per kernel (the one definition of what each
// translation unit once wrote out as its own set_lds).
template <typename K>
int allow_lds(K kern, size_t bytes) {
  if (bytes > 64 * 1024)
    EPA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)bytes));
  return EPA_OK;
}

// Launch trace (epa_launch_trace in echopype_amd.h): while it is on, every kernel launch notes its name -- the tests
// assert WHICH kernel served a call (a specialised kernel silently declining a shape otherwise passes every
// "fast == generic" comparison as generic == generic).
extern std::atomic<bool> g_trace_on;
void note_launch(const char* what);
// epa_last_range_stats_filled (echopype_amd.h): did the last fused call on this thread leave the range statistics?
void note_range_stats_filled(int filled);

// every distinct kernel name launched by this process (epa_launch_seen): the test suite's kernel coverage
void note_seen(const char* what);

inline int check_launch(const char* what) {
  if (g_trace_on.load(std::memory_order_relaxed)) note_launch(what);
  note_seen(what);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch of %s failed: %s", what, hipGetErrorString(e));
    return EPA_EHIP;
  }
  return EPA_OK;
}

constexpr int kBlock = 256;  // 4 wavefronts of 64
constexpr int kMinmaxMaxGrid = 1024;  // the most workgroups (= partials in its workspace) of an epa_nanminmax launch

// the LDS tables of fast_math.h (build_math_tabs): 256 x f64 for 10^x, 128 x (f64, f64) for log10
constexpr int kExpTabN = 256;
constexpr int kLogTabN = 128;
constexpr size_t kExpTabBytes = kExpTabN * sizeof(double);
constexpr size_t kLogTabBytes = kLogTabN * 2 * sizeof(double);
constexpr size_t kMathTabBytes = kExpTabBytes + kLogTabBytes;  // 4 KiB

// Dynamic LDS of a kernel that bins into LDS accumulators: the accumulators, then (16-byte aligned) the math tables
struct BinLds {
  unsigned tab_off;
  size_t total;
};
inline BinLds bin_lds_layout(size_t acc_bytes) {
  const size_t tab_off = (acc_bytes + 15) & ~(size_t)15;
  return {(unsigned)tab_off, tab_off + kMathTabBytes};
}

// may the 16-byte accesses of a vectorised kernel be used on this buffer?  (an optional buffer that is not given: yes)
inline bool al16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- device math, templated on the compute type ------------------------------------------------
template <typename T>
struct M;
template <>
struct M<double> {
  static __device__ __forceinline__ double log10(double x) { return ::log10(x); }
  static __device__ __forceinline__ double exp10(double x) { return ::exp10(x); }
  static __device__ __forceinline__ double nan() { return __builtin_nan(""); }
};
template <>
struct M<float> {
  static __device__ __forceinline__ float log10(float x) { return ::log10f(x); }
  static __device__ __forceinline__ float exp10(float x) { return ::exp10f(x); }
  static __device__ __forceinline__ float nan() { return __builtin_nanf(""); }
};

// Per-(channel, ping) coefficient row (EPA_NCOEF doubles, 64 B): two 32-B halves so that a
// wave-uniform row read is two scalar s_load_dwordx8.
struct CoefRow {
  double ra, rb, r0, shift, alpha2, A0, g, d;
};
static_assert(sizeof(CoefRow) == EPA_NCOEF * sizeof(double), "coef row layout");

// Workgroups are dealt to the 8 XCDs round-robin by their linear id.  With this remap of a 1-D work index the
// workgroups of one XCD walk ONE contiguous eighth of the index range instead of every eighth item: on the streaming
// probe (scripts/probes/hbm_mix_probe.hip, 4 B read + 8 B written per sample by workgroups that each walk a long run)
// that is 6.1 instead of 5.5 TB/s.  Items past the last multiple of 8 keep their index.
__device__ __forceinline__ int xcd_contiguous(int x, int n) {
  const int per = n >> 3;
  return x < per * 8 ? (x & 7) * per + (x >> 3) : x;
}
// EPA_XCD_MAP=0 turns the remap off (development knob, read once)
inline bool xcd_map_enabled() {
  static const bool on = [] {
    const char* e = getenv("EPA_XCD_MAP");
    return !(e && e[0] == '0');
  }();
  return on;
}

// Uniform-edge bin index: edges e_i = i*bin (np.arange(0, stop, bin) evaluates 0 + i*bin in
// double), membership decided against those exact edge values (SURVEY A.6 caveat (i)).
// Returns -1 for NaN, out of range.
__device__ __forceinline__ int range_bin_index(double x, double bin, double inv_bin, int nbins,
                                               bool closed_right) {
  if (!(x == x)) return -1;
  double t = x * inv_bin;
  // clamp before the int conversion (inf / huge values)
  if (!(t > -2.0)) return -1;
  if (t > (double)nbins + 2.0) return -1;
  int i;
  if (!closed_right) {
    i = (int)floor(t);
    // fix-up against the true edges
    if (x < (double)i * bin) --i;
    else if (x >= (double)(i + 1) * bin) ++i;
  } else {
    i = (int)ceil(t) - 1;
    if (x <= (double)i * bin) --i;
    else if (x > (double)(i + 1) * bin) ++i;
  }
  return (i >= 0 && i < nbins) ? i : -1;
}

// echo_range of sample s in the reference's operation order (range.py:138: (s*si)*c/2)
__device__ __forceinline__ double row_range(const CoefRow& r, int s) {
  return ((double)s * r.ra) * r.rb + r.r0;
}

// depth of a sample (consolidate/api.py:221: transducer_depth + orientation * echo_range * echo_range_scaling): the
// product is rounded, then the sum -- NumPy's two operations, never one contracted fma -- in the array's own type, so
// that the depth array, and whatever is binned on it without writing it, hold the reference's bits.
// (contraction switched off for the two statements: hipcc's default -ffp-contract=fast turns even __dadd_rn(o, __dmul_rn(a, r))
// into one v_fma_f64)
__device__ __forceinline__ double depth_of(double scale, double offset, double range) {
#pragma clang fp contract(off)
  const double prod = scale * range;
  return offset + prod;
}
__device__ __forceinline__ float depth_of(float scale, float offset, float range) {
#pragma clang fp contract(off)
  const float prod = scale * range;
  return offset + prod;
}

// ---- scratch buffers: allocated by the caller, sized HERE (epa_scratch_bytes in echopype_amd.h) ----------------------
// One function per scratch parameter of the ABI, bytes for the sizes (a, b, c) the header's table names, defined in the
// translation unit that lays the buffer out and written with the constants and helpers its entry uses.  runtime.hip
// lists them by name.  An entry whose write extent follows from a launch plan checks it against its own function
// before it launches (EPA_CHECK_SCRATCH): an internal error, never a write past the buffer.
namespace scratch {
size_t sv_power_stats_workspace(long long S, long long, long long);               // sv_power.hip
size_t depth_rows_workspace(long long, long long, long long);                     // reduce_util.hip
size_t nanminmax_workspace(long long, long long, long long);                      // reduce_util.hip
size_t range_step_mean_workspace(long long C, long long P, long long);            // reduce_util.hip
size_t sv_complex_cw_stats_workspace(long long, long long, long long);            // ek80_complex.hip
size_t sv_complex_fft_workspace(long long W, long long P, long long S);           // ek80_fft.hip
size_t splitbeam_complex_fft_workspace(long long n, long long, long long);        // splitbeam.hip
size_t sv_mvbs_fused_depth_stats(long long, long long, long long);                // block_reduce.hip
size_t apply_masks_workspace(long long, long long, long long);                    // noise_masks.hip
size_t pool_sv_sum_ws(long long C, long long P, long long S);                     // noise_masks.hip
size_t pool_sv_cnt_ws(long long C, long long P, long long S);                     // noise_masks.hip
size_t pool_sv_value_ws_mean(long long C, long long P, long long S);              // noise_masks.hip
size_t pool_sv_value_ws_median(long long C, long long S, long long);              // noise_masks.hip
size_t nasc_workspace(long long C, long long n_dbins, long long n_rbins);         // nasc.hip
size_t seafloor_state(long long, long long, long long);                           // seafloor.hip
size_t seafloor_angle_mask_work(long long P, long long R, long long);             // seafloor.hip
size_t seafloor_median_hist(long long, long long, long long);                     // seafloor.hip
size_t shoal_state(long long, long long, long long);                              // shoal.hip
size_t shoal_echoview_link_queue(long long, long long, long long);                // shoal.hip
size_t transient_fielding_todo(long long C, long long P, long long);              // transient.hip
size_t transient_fielding_count(long long, long long, long long);                 // transient.hip
size_t transient_matecho_s_hi(long long C, long long P, long long);               // transient.hip
size_t transient_matecho_flag(long long C, long long P, long long);               // transient.hip
size_t time_rebuild_tile_workspace(long long N, long long, long long);            // qc.hip
size_t regrid_mask_out(long long G, long long n_tbins, long long n_rbins);        // mask_grid.hip
size_t target_spectra_table(long long R, long long F, long long);                 // target_spectrum.hip
size_t sv_spectrum_table(long long R, long long F, long long);                    // sv_spectrum.hip
}  // namespace scratch

// `used` bytes are about to be written to a scratch buffer the caller sized as `have` = its scratch:: function
#define EPA_CHECK_SCRATCH(who, what, used, have)                                                              \
  EPA_CHECK_ARG((size_t)(used) <= (size_t)(have), "%s: internal error: the launch plan writes %zu bytes of %s, sized %zu", \
                who, (size_t)(used), what, (size_t)(have))

}  // namespace epa

// reduce_util.hip: echo_range / depth from the coefficient rows as one-piece workgroups (-1: the shape is not served)
int epa_rows_piece_launch(const float* mask_raw, const void* x, const double* coef, const double* scale,
                          const double* offset, long long rows, int S, void* out, int dtype, double* workspace,
                          double* stats_out, hipStream_t st);
// reduce_util.hip: {min, max, NaN count} partials (3 doubles per workgroup) -> out[3]
int epa_minmax_final(const double* part, int nparts, double* out, hipStream_t st);
// block_reduce.hip: the {min, max, min, max} keys (ordered_key.h) of Sv_noise / Sv_corrected, four words: set to "nothing
// seen" before the pass that lowers and raises them (init_minmax_kernel), and turned into doubles in place after it, NaN
// where a key was never touched (decode_minmax_kernel)
int epa_minmax_keys_init(unsigned long long* keys, hipStream_t st);
int epa_minmax_keys_decode(double* keys, hipStream_t st);

// The fast paths that block_reduce.hip's planner hands the hot configurations to.
// fused_sv_mvbs.hip: raw power (float, or int16 with the recorded lengths) -> Sv + MVBS in one pass
int epa_fused_fast_path(const void* raw, int raw_is_i16, const int32_t* n_valid, const double* coef,
                        int C, int P, int S, double nspread,
                        unsigned cal_flags, const int32_t* bin_start, int n_tbins, double range_bin,
                        int n_rbins, unsigned bin_flags, double fill_value, void* sv_out,
                        void* mvbs_out, void* sum_out, uint32_t* cnt_out, int dtype,
                        size_t lds_bytes, unsigned cnt_off, unsigned long long* rmax_key,
                        unsigned long long* rstat, const double* dscale, const double* doffset, void* depth_out,
                        hipStream_t st);
// fused_sv_mvbs.hip: Sv with the echo_range from the coefficient rows -> MVBS
int epa_mvbs_rows_fast_path(const void* sv, const double* coef, int C, int P, int S, const int32_t* bin_start,
                            int n_tbins, double range_bin, int n_rbins, int as_stored, double fill_value,
                            void* mvbs_out, void* sum_out, uint32_t* cnt_out, int dtype, size_t lds_bytes,
                            unsigned cnt_off, hipStream_t st);
// chain_fast.hip: raw power -> Sv + the noise estimate
int epa_chain_fast_pass1(const float* raw, const double* coef, const double* alpha2, int C, int P, int S,
                         double nspread, int ping_num, int rsn, int ping_phase, double noise_max, void* sv_out,
                         double* noise_out, double* edge_sum_out, uint32_t* edge_cnt_out,
                         unsigned long long* rmax_key, unsigned long long* rstat, int dtype, hipStream_t st);
// chain_fast.hip: raw power + noise -> Sv_noise / Sv_corrected + MVBS of Sv_corrected
int epa_chain_fast_pass2(const float* raw, const double* coef, const double* alpha2, const double* noise, int C,
                         int P, int S, double nspread, int ping_num, int ping_phase, double snr,
                         const int32_t* bin_start, int n_tbins, double range_bin, int n_rbins, double fill_value,
                         void* noise_out, void* corr_out, void* mvbs_out, void* sum_out, uint32_t* cnt_out, int dtype,
                         size_t lds_acc_bytes, unsigned cnt_off, unsigned long long* mm_keys, hipStream_t st);
