/* echopype_amd -- C ABI of the MI355X (gfx950) hot path of echopype
 *
 *   calibrate.compute_Sv / compute_TS  ->  clean.remove_background_noise  ->  commongrid.compute_MVBS
 *
 * The reference (OSOceanAcoustics/echopype, pure Python) has no FFI for this path; its boundary is
 * a set of Python functions on xarray Datasets.  This header is the C-ABI those
 * functions bind to in the drop-in (echopype_amd/, ctypes; see INTEGRATION.md for the stub a
 * reference maintainer would add).  Each entry point cites the reference code it replaces
 * (paths relative to /root/reference/echopype).
 *
 * Conventions
 *   - every function returns an int status (EPA_OK = 0); epa_last_error() gives the message of the
 *     last failure on the calling thread.  Nothing throws, nothing aborts.
 *   - all array pointers are DEVICE pointers (HBM) unless the name ends in _host.  Arrays are
 *     C-contiguous with the reference's dimension order (channel, ping_time, range_sample[, beam]).
 *   - the library never allocates or frees result memory; the caller owns every buffer.  The only
 *     allocations are the explicit epa_malloc/epa_free helpers offered to callers without a device
 *     allocator of their own.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls are asynchronous
 *     with respect to the host; they are re-entrant and keep no global mutable state.
 *   - NaN in -> NaN out; numerical edge cases never raise (SURVEY.md 8b "Error conventions").
 */
#ifndef ECHOPYPE_AMD_H
#define ECHOPYPE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPA_VERSION 104 /* 0.1.4: epa_apply_masks */

typedef void* epa_stream_t;

enum epa_status { EPA_OK = 0, EPA_EINVAL = 1, EPA_EHIP = 2, EPA_ENOMEM = 3, EPA_EUNSUPPORTED = 4 };
enum epa_dtype { EPA_F32 = 0, EPA_F64 = 1 };
enum epa_cal_type { EPA_CAL_SV = 0, EPA_CAL_TS = 1 };
enum epa_sonar { EPA_SONAR_EK60 = 0, EPA_SONAR_EK80 = 1 };
/* how a per-ping parameter is laid out: one value, one per channel, one per (channel, ping),
 * or (gain / sa_correction only) a per-channel pulse-length table to be looked up per ping */
enum epa_param_mode { EPA_PM_SCALAR = 0, EPA_PM_CHANNEL = 1, EPA_PM_CHANNEL_PING = 2, EPA_PM_PULSE_TABLE = 3 };

/* ---- per-(channel, ping) coefficient row consumed by the power-sample kernels ------------------
 *   echo_range R(s) = fl(fl(s * ra) * rb) + r0     EK: ra = sample_interval, rb = sound_speed/2, r0 = 0
 *                                                  -- the reference's own operation order
 *                                                  (range.py:138), so echo_range is bit-identical and
 *                                                  bin membership can never differ by a rounding;
 *                                                  AZFP: ra = 1, rb = c/4*2N/f, r0 per range.py:81-89
 *   R'(s)          = R(s) - shift                  TVG range shift (range.py:176-199)
 *   out(s)         = g * raw(s) + n * log10(R') + alpha2 * R' + A           n = 20 (Sv) | 40 (TS)
 * with the spreading term evaluated in its separable form: R' = k * (s - d), k = ra * rb,
 * d = (shift - r0) / k, so n*log10(R') = n*log10(k) + n*log10(s - d).  d is (nearly always) the
 * same for every ping of a file -- exactly 2 for EK60, tau/(2*sample_interval) for EK80, -r0/k for
 * AZFP -- which lets the kernels evaluate log10(s - d) once per range column instead of once per
 * sample.  Slot A0 = A + n * log10(k) (so a row is specific to Sv or TS).
 */
#define EPA_NCOEF 8
enum epa_coef_slot { EPA_CF_RA = 0, EPA_CF_RB = 1, EPA_CF_R0 = 2, EPA_CF_SHIFT = 3, EPA_CF_ALPHA2 = 4,
                     EPA_CF_A0 = 5, EPA_CF_G = 6, EPA_CF_D = 7 };

/* flags of epa_sv_power / epa_sv_mvbs_fused */
#define EPA_FLAG_GUARD_POS 1u  /* R' <= 0 -> NaN (calibrate_ek.py:107); AZFP has no such guard  */
#define EPA_FLAG_MASK_RANGE 2u /* echo_range is NaN where the raw sample is NaN (range.py:143-148) */

/* flags of the binned reductions */
#define EPA_BIN_SKIPNA 1u       /* nanmean (skip NaN values) vs mean (NaN poisons the bin)            */
#define EPA_BIN_CLOSED_RIGHT 2u /* intervals (a, b] instead of [a, b)  (commongrid/utils.py:283-302) */
#define EPA_BIN_RANGE_AS_STORED 4u /* epa_mvbs with coefficient rows in place of the range array: round the range to
                                    * dtype before binning, i.e. bin exactly as on the echo_range array epa_sv_power
                                    * would have written (a no-op for EPA_F64)                                        */

/* ---- runtime ------------------------------------------------------------------------------------ */
int epa_version(void);
/* Hex digest (sha256, 32 characters) of the sources and compiler flags this library was built from
 * (echopype_amd/build.py:source_digest).  The binding recomputes it from the files beside it at import time and refuses
 * a library built from other sources: the shipped binary is the shipped code.  No reference counterpart. */
const char* epa_source_digest(void);
const char* epa_last_error(void);
/* Launch trace, test infrastructure: mode 1 clears the calling thread's trace and switches tracing on, mode 0 clears and
 * switches it off, any other mode leaves it as it is.  Returns the "kernel;kernel;..." names of the launches this thread
 * made since (2 KiB kept; the string is valid until the next call on the thread).  Lets a parity test assert WHICH
 * kernel served a call -- the reference has no counterpart. */
const char* epa_launch_trace(int mode);
/* 1 when the last epa_sv_mvbs_fused / epa_sv_noise_fused call on the calling thread was served by the kernel that leaves range_stats_out
 * {nanmin, nanmax, NaN count}; 0 when the generic kernel served it (it leaves the maximum only and writes NaN count -1).
 * The same fact as the -1 on the device, known on the host without waiting for the kernel. */
int epa_last_range_stats_filled(void);
/* Every distinct kernel name this PROCESS has launched so far, "name;name;..." (sorted; valid until the next call): the
 * test suite's kernel coverage (tests/conftest.py writes it out at the end of a GPU session). */
const char* epa_launch_seen(void);
int epa_device_count(int* n);
int epa_set_device(int dev);
int epa_device_name(int dev, char* buf, size_t len);
int epa_malloc(void** ptr, size_t bytes);
int epa_free(void* ptr);
int epa_memset(void* ptr, int value, size_t bytes, epa_stream_t stream);
int epa_memcpy_h2d(void* dst, const void* src_host, size_t bytes, epa_stream_t stream);
int epa_memcpy_d2h(void* dst_host, const void* src, size_t bytes, epa_stream_t stream);
int epa_stream_synchronize(epa_stream_t stream);
/* HIP-event timing on `stream` (used by bench.py for the roofline figure): record start/stop
 * around a region, then read the elapsed milliseconds.  Handles are opaque. */
int epa_timer_create(void** timer);
int epa_timer_destroy(void* timer);
int epa_timer_start(void* timer, epa_stream_t stream);
int epa_timer_stop(void* timer, epa_stream_t stream);
int epa_timer_elapsed_ms(void* timer, float* ms); /* synchronises on the stop event */

/* ---- scratch buffers: allocated by the caller, sized by the library ------------------------------------------------
 * Bytes of the scratch buffer `what` ("<entry>.<parameter>", table below) for the sizes a, b, c the table names (unused
 * ones 0).  Pure host arithmetic: no HIP call, usable without a GPU.  Unknown name: EPA_EINVAL.
 *
 * THESE FUNCTIONS ARE THE AUTHORITY on the size of every scratch parameter: each is defined beside the code that lays
 * its buffer out, and an entry whose write extent follows from a launch plan checks it against the same function
 * before launching.  The EPA_*_WS_* macros and the "f64 [n]" remarks further down give the same values and stay for C
 * callers that size at compile time.
 *
 *   what                                   a, b, c                       the buffer
 *   sv_power_stats.workspace               S                             f64 [EPA_SV_POWER_STATS_WS_DOUBLES(S)]
 *   depth_rows.workspace                   -                             f64 [EPA_DEPTH_ROWS_WS_DOUBLES]
 *   nanminmax.workspace                    -                             f64 [3072]
 *   sv_complex_cw_stats.workspace          -                             f64 [EPA_SV_COMPLEX_CW_STATS_WS_DOUBLES]
 *   sv_complex_fft.workspace               W = max(C, n_replicas), P, S  f64 [EPA_EK80_FFT_WS_DOUBLES(W, P, S)]
 *   sv_complex_fft_indexed.workspace       the same
 *   selftest_correlate.workspace           1, 1, 1                       the same
 *   splitbeam_complex_fft.workspace        n                             f64 [EPA_SPLITBEAM_FFT_WS_DOUBLES(n)]
 *   sv_mvbs_fused_depth.depth_stats_out    -                             f64 [64]
 *   apply_masks.workspace                  -                             f64 [EPA_APPLY_MASKS_WS_DOUBLES]
 *   range_step_mean.workspace              C, P                          f64 [2*C*P]
 *   pool_sv.sum_ws / pool_sv.cnt_ws        C, P, S                       f64 [C*P*S] / i32 [C*P*S] (nanmean)
 *   pool_sv_value.ws_mean                  C, P, S                       EPA_POOL_VALUE_WS_BYTES, rounded up to 8
 *   pool_sv_value.ws_median                C, S                          EPA_POOL_VALUE_MEDIAN_WS_BYTES
 *   nasc.workspace                         C, n_dbins, n_rbins           24 bytes per cell
 *   seafloor.state                         -                             u64 [EPA_SEAFLOOR_STATE_WORDS]
 *   seafloor_angle_mask.work               P, R                          f64 [2*P*R]
 *   seafloor_median.hist                   -                             u64 [512]
 *   shoal.state                            -                             u64 [EPA_SHOAL_STATE_WORDS]
 *   shoal_echoview_link.queue              -                             i32 [2 * EPA_SHOAL_QUEUE_BOXES]
 *   transient_fielding.todo / .count       C, P / -                      i64 [C*P] (`list`) / u32 [1]
 *   transient_matecho.s_hi / .flag         C, P                          i32 [C*P] / u8 [C*P]
 *   time_rebuild.tile_workspace            N                             i64 [ceil((N-1) / EPA_QC_SCAN_TILE)]
 *   regrid_mask.out                        G, n_tbins, n_rbins           the G*n_tbins*n_rbins cells, rounded up to 4 bytes
 */
int epa_scratch_bytes(const char* what, long long a, long long b, long long c, size_t* bytes_out);
/* Three decisions a caller has to know BEFORE a call, to allocate for it; each is answered by the rule the entry itself
 * uses.  Pure host arithmetic, as above.
 *   epa_mvbs_needs_partials: MAY epa_mvbs / epa_sv_mvbs_fused / epa_denoise_mvbs / epa_sv_denoise_mvbs need sum_out and
 *     cnt_out for this grid (few ping bins, or accumulators too large for LDS)?  A superset of the cases that do.
 *   epa_regrid_needs_global_flags: does epa_regrid_mask keep the flags of a time bin in `out` instead of LDS?
 *   epa_sv_power_vectorized: does epa_sv_power(_stats) take its 16-byte path on this input (needed for range statistics
 *     without the range array)? */
int epa_mvbs_needs_partials(int C, int n_tbins, int n_rbins, int dtype, int* yes);
int epa_regrid_needs_global_flags(int n_rbins, int* yes);
int epa_sv_power_vectorized(const void* raw, int S, int dtype, int* yes);

/* ---- K0: coefficient table for EK60 / EK80 power samples ------------------------------------------
 * Replaces the per-(channel, ping) arithmetic of
 *   calibrate/range.py:138 (k = sample_interval*sound_speed/2), :176-199 (TVG shift),
 *   calibrate/cal_params.py:261-324 (pulse-length table lookup of gain / sa_correction),
 *   calibrate/calibrate_ek.py:98,154-162 (CSv) and :176-181 (CSp).
 * sample_interval, tau_nominal, transmit_power: [C*P].  sound_speed / absorption / gain / sa:
 * pointer + epa_param_mode.  With EPA_PM_PULSE_TABLE, `gain`/`sa` are [C*K] tables matched against
 * pulse_length [C*K] by argmin_k |tau_nominal - pulse_length| (first minimum; NaN tau -> NaN).
 * psi (equivalent_beam_angle): pointer + epa_param_mode (scalar, [C] or [C*P]: calibrate_ek.py:154-162 broadcasts any
 * (channel, ping_time) cal parameter into CSv; Sv only).  f_nominal: [C].  tau_eff: [C] (EPA_PM_CHANNEL) or [C*P]
 * (EPA_PM_CHANNEL_PING: an EK80 file with several filter_time intervals has one effective pulse length per (channel,
 * interval), calibrate/api.py:125-197).  gpt: [C] bytes or NULL (EK80: channels with GPT transceivers).
 * coef out: [C*P*EPA_NCOEF].
 */
int epa_power_coef_ek(int C, int P, const double* sample_interval, const double* tau_nominal,
                      const double* transmit_power, const double* sound_speed, int ss_mode,
                      const double* absorption, int abs_mode, const double* gain, int gain_mode,
                      const double* sa_correction, int sa_mode, const double* pulse_length, int K,
                      const double* psi, int psi_mode, const double* f_nominal, const double* tau_eff,
                      int tau_eff_mode, const uint8_t* gpt, int sonar, int cal_type, double* coef, epa_stream_t stream);

/* The pulse-length table lookup on its own (calibrate/cal_params.py:261-324 get_vend_cal_params_power): out[c,p] =
 * table[c, argmin_k |tau_nominal[c,p] - pulse_length[c,k]|] (first minimum; NaN tau -> NaN).  What compute_Sv attaches to
 * its output as gain_correction / sa_correction (channel, ping_time) when the per-ping parameters live in HBM.
 * tau_nominal, out: f64 [C*P]; pulse_length, table: f64 [C*K]. */
int epa_pulse_table_lookup(const double* tau_nominal, const double* pulse_length, const double* table, int C, int P,
                           int K, double* out, epa_stream_t stream);

/* ---- K1: fused power-sample calibration (EK60, EK80 CW power, AZFP) ---------------------------------
 * Replaces calibrate/range.py:98-201 + calibrate/calibrate_ek.py:104-110,154-184 (EK) and
 * calibrate/range.py:69-95 + calibrate/calibrate_azfp.py:64-97 (AZFP): ~15 whole-array passes
 * become one.  raw: f32 [C*P*S] (backscatter_r).  out: Sv or TS, [C*P*S] of out_dtype.
 * range_out: echo_range [C*P*S] of out_dtype; may be NULL.
 */
int epa_sv_power(const float* raw, const double* coef, int C, int P, int S, int cal_type,
                 unsigned flags, void* out, void* range_out, int out_dtype, epa_stream_t stream);
/* The same with {nanmin, nanmax, NaN count} of the echo_range written as a by-product (range_stats_out f64 [3],
 * as epa_nanminmax would give): what compute_MVBS (api.py:108-110), compute_NASC and the masks ask of the range
 * variable next, without another sweep of it.  workspace: f64 [EPA_SV_POWER_STATS_WS_DOUBLES(S)]. */
#define EPA_SV_POWER_STATS_WS_DOUBLES(S) (3 * ((size_t)(S) / 256 + 8192 + 1024))
int epa_sv_power_stats(const float* raw, const double* coef, int C, int P, int S, int cal_type,
                       unsigned flags, void* out, void* range_out, int out_dtype, double* workspace,
                       double* range_stats_out, epa_stream_t stream);
/* range_out may be NULL there (S even for F64 / S % 4 == 0 for F32, 16-byte aligned buffers; EPA_EUNSUPPORTED
 * otherwise): the statistics are taken of the echo_range that WOULD be written and the array itself -- 8 of the 20
 * bytes per sample the pass moves -- is left to this entry for whoever asks for it later (the reference's echo_range is
 * just as lazy when the echodata is dask-backed; range.py:98-157 with the NaN mask of :143-148 under
 * EPA_FLAG_MASK_RANGE, then raw is read).  epa_mvbs / epa_noise_estimate / epa_noise_apply take the same coefficient
 * rows in place of the array. */
int epa_range_power(const float* raw, const double* coef, int C, int P, int S, unsigned flags, void* range_out,
                    int out_dtype, epa_stream_t stream);

/* ---- time-bin CSR for the binned reductions ----------------------------------------------------------
 * Replaces the pandas-resample bin assignment of commongrid/api.py:118-128.  ping_time: int64 ns,
 * sorted ascending, [P].  Bin b covers [t0 + b*dt, t0 + (b+1)*dt) (or (..] when closed right).
 * bin_start out: int32 [n_bins + 1]; pings bin_start[b] .. bin_start[b+1]-1 belong to bin b.
 */
int epa_time_bin_offsets(const int64_t* ping_time, int P, int64_t t0, int64_t dt, int n_bins,
                         unsigned flags, int32_t* bin_start, epa_stream_t stream);

/* ---- K1+K5: fused compute_Sv -> compute_MVBS -----------------------------------------------------------
 * One pass over the raw power: writes Sv (optional) and the MVBS grid.  Replaces K1's references
 * plus commongrid/utils.py:592,614-627 (flox group-by nanmean in the linear domain) and :92.
 *   bin_start  : int32 [n_tbins+1] (epa_time_bin_offsets);  ping_perm: int32 [.] or NULL (identity)
 *   range bins : edges e_i = i * range_bin, i = 0..n_rbins (np.arange(0, max+bin, bin), api.py:115)
 *   sv_out     : [C*P*S] of dtype or NULL;  range_out as in epa_sv_power or NULL
 *   mvbs_out   : f64/f32 [C*n_tbins*n_rbins] in dB (fill_value where a bin is empty)
 *   sum_out/cnt_out : optional raw linear sums (dtype) / counts (u32) per bin, same shape, for
 *                 cross-shard merges; may be NULL
 *   range_max_out : optional f64 [1]: nanmax(echo_range) as a by-product (what api.py:108-110 needs
 *                 to size the range grid: call with a conservative n_rbins, then trim); NULL if not
 *                 wanted.
 *   range_stats_out : optional f64 [3] (needs range_max_out): {nanmin, nanmax, NaN count} of the echo_range array
 *                 epa_range_power would write (rounded to dtype) -- what the next compute_MVBS / add_depth on
 *                 the same dataset asks of its range variable; {NaN, NaN, -1} when the configuration is served
 *                 by the generic kernel, which leaves the maximum only.
 */
int epa_sv_mvbs_fused(const float* raw, const double* coef, int C, int P, int S, int cal_type,
                      unsigned cal_flags, const int32_t* bin_start, const int32_t* ping_perm,
                      int n_tbins, double range_bin, int n_rbins, unsigned bin_flags,
                      double fill_value, void* sv_out, void* range_out, void* mvbs_out,
                      void* sum_out, uint32_t* cnt_out, double* range_max_out, double* range_stats_out,
                      int dtype, epa_stream_t stream);

/* Same pass fed with the instrument's own int16 power samples (SURVEY 8f "next" row 4; replaces the
 * ingest arithmetic of convert/parse_base.py:24,302 -- float32(int16) * float32(10*log10(2)/256) --
 * and the NaN padding of short pings, pad_shorter_ping): raw int16 [C*P*S], n_valid int32 [C*P] =
 * recorded length of each ping (samples at or beyond it are padding = NaN).  2 B/sample of input
 * instead of 4.  Default configuration only (R' <= 0 guard, echo_range masked by padding, skipna,
 * left-closed bins, sorted pings, S % 4 == 0); other arguments as epa_sv_mvbs_fused.
 */
int epa_sv_mvbs_fused_i16(const int16_t* raw, const int32_t* n_valid, const double* coef, int C, int P,
                          int S, int cal_type, const int32_t* bin_start, int n_tbins, double range_bin,
                          int n_rbins, double fill_value, void* sv_out, void* mvbs_out, void* sum_out,
                          uint32_t* cnt_out, double* range_max_out, int dtype, epa_stream_t stream);

/* The same pass binned on ``depth`` -- consolidate.add_depth between compute_Sv and compute_MVBS(range_var="depth")
 * (SURVEY 8f "next" row 1).  Replaces consolidate/api.py:221 (depth = transducer_depth + orientation * echo_range *
 * echo_range_scaling: one multiplication and one addition per sample, each rounded, in dtype) fused into K1+K5, so the
 * three reference calls cost the 12 B/sample of the two: the depth array is an affine function of the coefficient
 * rows and is written only when asked for (depth_out, +8 B/sample).
 *   depth_scale, depth_offset : f64 [C*P] -- orientation * echo_range_scaling and transducer_depth per (channel, ping)
 *   depth_out       : [C*P*S] of dtype or NULL (needs sv_out); NaN where the raw sample is, like the echo_range
 *   depth_stats_out : f64 [64], 128-byte aligned: {nanmin, nanmax, NaN count} of the depth array in slots 0..2 (the rest
 *                     is scratch) -- what sizes the range grid (commongrid/api.py:108-115): call with a conservative
 *                     n_rbins, then trim
 * Default configuration only (R' <= 0 guard, echo_range masked by NaN input, skipna, left-closed bins, sorted pings,
 * S % 4 == 0, grid within LDS): EPA_EUNSUPPORTED otherwise.  Other arguments as epa_sv_mvbs_fused.
 */
int epa_sv_mvbs_fused_depth(const float* raw, const double* coef, const double* depth_scale,
                            const double* depth_offset, int C, int P, int S, int cal_type, const int32_t* bin_start,
                            int n_tbins, double range_bin, int n_rbins, double fill_value, void* sv_out,
                            void* depth_out, void* mvbs_out, void* sum_out, uint32_t* cnt_out, double* depth_stats_out,
                            int dtype, epa_stream_t stream);

/* ---- K5: compute_MVBS on an existing Sv dataset -----------------------------------------------------------
 * Replaces commongrid/utils.py:504-628 (+ :92).  sv: [C*P*S] of dtype.  Range coordinate either
 * as a full array `range` ([C*P*S], f64 when dtype F64 else f32; echo_range or depth) or, when
 * `range` is NULL, as the affine form of `coef` (R = r0 + s*k, valid everywhere).
 */
int epa_mvbs(const void* sv, const void* range, const double* coef, int C, int P, int S,
             const int32_t* bin_start, const int32_t* ping_perm, int n_tbins, double range_bin,
             int n_rbins, unsigned bin_flags, double fill_value, void* mvbs_out, void* sum_out,
             uint32_t* cnt_out, int dtype, epa_stream_t stream);

/* Self-test hook: out[i] = 10^(u[i]/10) evaluated with the table-driven f64 routine the fused kernel
 * uses for the linear-domain average (_log2lin, utils/compute.py:14-27); u, out f64 [n]. */
int epa_selftest_lin_from_db(const double* u, double* out, size_t n, epa_stream_t stream);
/* Same for the table-driven f64 log10 used by _lin2log and the transmission-loss terms. */
int epa_selftest_log10(const double* x, double* out, size_t n, epa_stream_t stream);
/* The call-free variant of that log10 (every special case folded into selects) the chain kernels use. */
int epa_selftest_log10_inline(const double* x, double* out, size_t n, epa_stream_t stream);

/* Finalise merged partial sums: out = 10*log10(sum/cnt), fill_value where cnt == 0. */
int epa_mvbs_finalize(const void* sum, const uint32_t* cnt, size_t n, double fill_value, void* out,
                      int dtype, epa_stream_t stream);

/* ---- cross-shard edge exchange (no reference counterpart: the reference is single-process) -------------
 * A ping-sharded dataset sums an MVBS time bin over ALL its pings (commongrid/utils.py:614-627) and takes a background-
 * noise block's mean before the minimum over range blocks (clean/api.py:402-411): the raw linear (sum, count) rows of
 * the bins / blocks cut by a shard or tile edge are exchanged.  One step = epa_edge_pack -> ONE all-reduce(SUM) of
 * `buf` (torch.distributed: RCCL over xGMI, the buffer stays in HBM) -> epa_edge_gather.
 * buf: f64 [n_slots * 2 * C * R], slot layout (slot, {sum, count}, channel, range bin).
 * epa_edge_pack: HOST tables of n_rows device rows: element (c, r) of row i at sum_rows[i][c * chan_stride[i] + r]
 * (sum_dtype EPA_F32 / EPA_F64) and cnt_rows[i][...] (u32), written to slot slots[i]; zero_first clears the whole
 * buffer before (slots of absent edges must be 0 for the SUM).
 * epa_edge_gather: for local shared edge e, the sum of the slots group_slots[group_off[e] .. group_off[e+1]) (device
 * int32 tables built once per plan), added in table order -- the same order on every rank, so every holder of a bin
 * reads bit-identical totals.  Outputs (each optional): totals_out f64 [n_edges * 2 * C * R] (sum and count planes, what
 * epa_noise_finalize takes); sum_out [n_edges * C * R] of sum_dtype + cnt_out u32 [n_edges * C * R] (what
 * epa_mvbs_finalize takes).
 * epa_edge_finalize_mvbs: gather + 10 log10(sum / count) (fill_value where the count is 0; the arithmetic of
 * epa_mvbs_finalize on the totals rounded to dtype) of the listed edges (HOST tables: edges[i] = index into group_off,
 * dst_rows[i] = device row with element (c, r) at [c * chan_stride[i] + r] of dtype) -- the owner of a cut time bin
 * writes the bin's row of its MVBS array in one launch. */
int epa_edge_pack(const void* const* sum_rows, const uint32_t* const* cnt_rows, const long long* chan_stride,
                  const int* slots, int n_rows, int sum_dtype, int C, int R, int n_slots, int zero_first, double* buf,
                  epa_stream_t stream);
int epa_edge_gather(const double* buf, int n_slots, const int32_t* group_off, const int32_t* group_slots, int n_edges,
                    int C, int R, double* totals_out, void* sum_out, uint32_t* cnt_out, int sum_dtype,
                    epa_stream_t stream);
int epa_edge_finalize_mvbs(const double* buf, int n_slots, const int32_t* group_off, const int32_t* group_slots,
                           const int* edges, void* const* dst_rows, const long long* chan_stride, int n_rows, int C,
                           int R, double fill_value, int dtype, epa_stream_t stream);
/* nanmax(echo_range) of a shard before its all-reduce(MAX) over the ranks (commongrid/api.py:108-115 takes the maximum of
 * the WHOLE dataset): NaN (a shard without a valid range) -> -inf, in place, n device doubles. */
int epa_edge_prepare_max(double* values, int n, epa_stream_t stream);

/* ---- depth = offset[c,p] + scale[c,p] * echo_range -----------------------------------------------------------
 * The array pass of consolidate.add_depth (consolidate/api.py:226: transducer_depth +
 * orientation * echo_range * cos(tilt)); SURVEY 8f "next" row 1.  x, out: [C*P*S] of dtype;
 * scale, offset: f64 [C*P].
 */
int epa_affine_rows(const void* x, const double* scale, const double* offset, int C, int P, int S,
                    void* out, int dtype, epa_stream_t stream);
/* The same with (i) echo_range either as the array `range` or -- range NULL -- evaluated from the power-sample
 * coefficient rows `coef`, NaN where mask_raw (float [C*P*S], optional) is NaN: an echo_range left out of the sample
 * pass (epa_sv_power_stats with range_out = NULL) never has to be written for add_depth; (ii) {nanmin, nanmax, NaN
 * count} of the depth as a by-product (stats_out f64 [3], workspace f64 [EPA_DEPTH_ROWS_WS_DOUBLES]; both optional):
 * what compute_MVBS(range_var="depth") asks of the variable next (commongrid/api.py:108-110). */
#define EPA_DEPTH_ROWS_WS_DOUBLES (3 * 16384)
int epa_depth_rows(const void* range, const double* coef, const float* mask_raw, const double* scale,
                   const double* offset, int C, int P, int S, void* out, int dtype, double* workspace,
                   double* stats_out, epa_stream_t stream);

/* ---- NaN-skipping min/max of a device array ---------------------------------------------------------------
 * Replaces the reductions the reference forces with ds_Sv[range_var].max(skipna=True)
 * (commongrid/api.py:108-110) and the actual_range attributes (clean/utils.py:392-395,
 * commongrid/api.py:252-255).  x: [n] of dtype; workspace: f64 [3072]; out: f64 [3] = {min, max,
 * number of NaN elements} (min = max = NaN when no element is non-NaN).  The NaN count serves the
 * "coordinate array contain NaNs" warning of commongrid/utils.py:595-608 without another sweep.
 */
int epa_nanminmax(const void* x, size_t n, int dtype, double* workspace, double* out,
                  epa_stream_t stream);

/* ---- K5': compute_MVBS_index_binning ------------------------------------------------------------------------
 * Replaces commongrid/api.py:217-222 (coarsen(ping_num, range_sample_num, "pad").mean(skipna) in the
 * linear domain) and :232-238 (echo_range block min).  Outputs [C * ceil(P/ping_num) *
 * ceil(S/range_sample_num)].  range / range_min_out may be NULL.
 */
int epa_mvbs_index(const void* sv, const void* range, int C, int P, int S, int ping_num,
                   int range_sample_num, void* mvbs_out, void* range_min_out, int dtype,
                   epa_stream_t stream);

/* ---- K6: background-noise estimate (De Robertis & Higginbottom 2007) -------------------------------------------
 * Replaces clean/api.py:397-422: TL = 20log10(max(R,1) [NaN->1]) + 2*alpha*R; block mean of
 * 10^((Sv-TL)/10) over ping_num x range_sample_num (NaN-padded, NaN-skipping) -> dB -> min over
 * range blocks -> optional clamp to noise_max (NaN when noise_max is NaN = not given).
 * alpha2: 2*alpha per (c,p) [C*P] f64.
 * ping_phase (0 .. ping_num-1): the arrays hold a ping shard of a longer dataset whose first ping sits
 * `ping_phase` pings into a block (global ping index of the shard's first ping modulo ping_num; 0 for a whole
 * dataset): local ping p belongs to block (p + ping_phase) / ping_num.
 * noise_out: f64 [C * ceil((P + ping_phase) / ping_num)].
 * edge_sum_out / edge_cnt_out (optional, both or neither; f64 / u32 [2 * C * ceil(S/range_sample_num)], zeroed by the
 * caller): the raw linear (sum, count) per range block of the shard's FIRST (slot 0) and LAST (slot 1, written only
 * when it is another block) ping block -- blocks a shard edge may cut; the owner merges them across shards before the
 * mean and the min, then epa_noise_finalize.
 */
int epa_noise_estimate(const void* sv, const void* range, const double* coef, const double* alpha2,
                       int C, int P, int S, int ping_num, int range_sample_num, int ping_phase, double noise_max,
                       double* noise_out, double* edge_sum_out, uint32_t* edge_cnt_out, int dtype,
                       epa_stream_t stream);

/* Merged (sum, count) rows of noise blocks -> noise value per row (clean/api.py:402-422: mean -> dB -> min over the
 * range blocks -> clamp).  sum, cnt: f64 [rows * n_rblocks] (the counts travel through an all-reduce with the sums);
 * noise_out: f64 [rows]. */
int epa_noise_finalize(const double* sum, const double* cnt, int rows, int n_rblocks, double noise_max,
                       double* noise_out, epa_stream_t stream);

/* ---- K7: noise removal -------------------------------------------------------------------------------------------
 * Replaces clean/api.py:425-430 (ffill upsample + TL) and :485-487.  Writes Sv_noise and
 * Sv_corrected ([C*P*S] of dtype; either may be NULL).  snr_threshold in dB.  ping_phase as in
 * epa_noise_estimate (noise holds ceil((P + ping_phase) / ping_num) blocks per channel).  minmax_out (f64 [4],
 * optional): NaN-skipping {min, max} of Sv_noise and of Sv_corrected as a by-product (the actual_range
 * attributes of clean/utils.py:392-395 without two more sweeps).
 */
int epa_noise_apply(const void* sv, const void* range, const double* coef, const double* alpha2,
                    const double* noise, int C, int P, int S, int ping_num, int ping_phase, double snr_threshold,
                    void* sv_noise_out, void* sv_corrected_out, double* minmax_out, int dtype,
                    epa_stream_t stream);
/* The same on an Sv whose echo_range was left out of the sample pass (epa_sv_power_stats with range_out = NULL): the
 * range is evaluated from the power-sample coefficient rows and -- mask_raw, float [C*P*S], optional -- set to NaN
 * where the raw sample is NaN, as the echo_range array would be (range.py:143-148; Sv_noise is NaN there, api.py:425-430).
 * 4 B/sample of raw instead of 8 (or 4) of echo_range, and the array is never written. */
int epa_noise_apply_rows(const void* sv, const double* coef, const float* mask_raw, const double* alpha2,
                         const double* noise, int C, int P, int S, int ping_num, int ping_phase,
                         double snr_threshold, void* sv_noise_out, void* sv_corrected_out, double* minmax_out,
                         int dtype, epa_stream_t stream);

/* ---- K3+K4: EK80 complex samples (CW complex and BB pulse compression) ---------------------------------------------
 * Replaces calibrate/ek80_complex.py:285-369 (compress_pulse: matched filter with the transmit
 * replica per ping and sector), :372-391 (norm factor), calibrate_ek.py:483-490 (received power
 * from the sector mean) and :571-638 (Sv / TS chain).
 *   re, im   : backscatter_r / backscatter_i as stored by echopype: f64 (in_dtype F64) or f32,
 *              [C*P*S*B], beam innermost, NaN-padded
 *   replica  : float2-interleaved complex f32 [sum(taps)], conj NOT applied, per channel at
 *              replica_off[c] .. replica_off[c+1] (int32 [C+1], device); both NULL for CW (no
 *              pulse compression).  max_taps = longest replica (sizes the LDS tile).
 *   ccoef    : per-(c,p) rows of EPA_NCCOEF doubles, see enum below.  PSCALE excludes the
 *              1/||tx||^4 of the pulse-compression normalisation: the kernel computes ||tx||^2
 *              itself (wavefront shuffle reduction over the LDS-resident replica)
 *   out      : Sv/TS [C*P*S] of out_dtype; range_out, prx_out (same dtype) optional.  A sample whose beam-0 real
 *              part is NaN is NaN in out and range_out whatever its other sectors hold: the reference calibrates
 *              with the masked echo_range (range.py:143-148, calibrate_ek.py:571-576); prx_out is unaffected.
 *              F64 output accumulates the matched filter in f64, F32 in f32
 */
#define EPA_NCCOEF 8
/* echo_range R = fl(fl(s*RA)*RB) (RA = sample_interval, RB = sound_speed/2: range.py:138 order);
 * R' = R - SHIFT (<= 0 -> NaN); out = 10log10(prx) + n*log10(R') + ALPHA2*R' + A;
 * prx = PSCALE * |sector mean of the (pulse-compressed, normalised) samples|^2  (<= 0 -> NaN) */
enum epa_ccoef_slot { EPA_CC_RA = 0, EPA_CC_RB = 1, EPA_CC_SHIFT = 2, EPA_CC_ALPHA2 = 3, EPA_CC_A = 4,
                      EPA_CC_PSCALE = 5, EPA_CC_RSV0 = 6, EPA_CC_RSV1 = 7 };
/* The rows above built on the device from the per-(channel, ping) parameters (the EK80 counterpart of
 * epa_power_coef_ek; replaces the (channel, ping_time) arithmetic of calibrate_ek.py:483-490, 507-530, 583-638 and
 * range.py:180-199).  params / modes: HOST arrays of EPA_CCP_COUNT DEVICE pointers (f64) and their epa_param_mode
 * (SCALAR, CHANNEL [C] or CHANNEL_PING [C*P]), indexed by epa_ccoef_param; entries a mode does not use may be NULL
 * (the angle offsets / beamwidths without bb; sa_correction with bb or TS; psi with TS).  tau_eff: f64 [C] or [C*P] (device;
 * tau_eff_mode EPA_PM_CHANNEL / EPA_PM_CHANNEL_PING as for epa_power_coef_ek);
 * gpt: u8 [C] or NULL.  bb != 0: broadband (gain is compensated by B(theta, phi), no sa_correction). */
enum epa_ccoef_param { EPA_CCP_SAMPLE_INTERVAL = 0, EPA_CCP_TAU_NOMINAL, EPA_CCP_TRANSMIT_POWER, EPA_CCP_SOUND_SPEED,
                       EPA_CCP_ABSORPTION, EPA_CCP_GAIN, EPA_CCP_FREQ_CENTER, EPA_CCP_PSI, EPA_CCP_SA_CORRECTION,
                       EPA_CCP_Z_ER, EPA_CCP_Z_ET, EPA_CCP_ANGLE_OFFSET_ALONGSHIP, EPA_CCP_ANGLE_OFFSET_ATHWARTSHIP,
                       EPA_CCP_BEAMWIDTH_ALONGSHIP, EPA_CCP_BEAMWIDTH_ATHWARTSHIP, EPA_CCP_COUNT };
int epa_complex_coef_ek80(int C, int P, const double* const* params, const int* modes, const double* tau_eff,
                          int tau_eff_mode, const uint8_t* gpt, int B, int bb, int cal_type, double* ccoef,
                          epa_stream_t stream);

int epa_sv_complex(const void* re, const void* im, int in_dtype, const float* replica,
                   const int32_t* replica_off, int max_taps, const double* ccoef, int C, int P,
                   int S, int B, int cal_type, void* out, void* range_out, void* prx_out,
                   int out_dtype, epa_stream_t stream);
/* The same with one replica per (channel, filter interval) instead of one per channel -- an EK80 file with several
 * filter_time entries, which the reference calibrates slice by slice and merges (calibrate/api.py:125-197): ONE launch
 * over the whole (channel, ping_time) grid.  replica_off: int32 [n_replicas + 1]; replica_id: int32 [C*P], the replica
 * of every ping, -1 for a ping no interval covers (give it a NaN coefficient row: its output and range are NaN, the
 * outer join's fill). */
int epa_sv_complex_indexed(const void* re, const void* im, int in_dtype, const float* replica,
                           const int32_t* replica_off, const int32_t* replica_id, int n_replicas, int max_taps,
                           const double* ccoef, int C, int P, int S, int B, int cal_type, void* out, void* range_out,
                           void* prx_out, int out_dtype, epa_stream_t stream);

/* Same result for long replicas through an LDS-resident 2048-point FFT per tile (the matched filter as a
 * circular correlation; scipy.signal.convolve's method="auto" makes the same switch in the reference,
 * ek80_complex.py:310-313): ~11x fewer flops than the direct form at 177 taps, the kernel becomes HBM-bound
 * like CW.  Replicas of 1 .. EPA_EK80_NFFT/2 taps (EPA_EUNSUPPORTED beyond: use epa_sv_complex).
 *   fft_dtype  : arithmetic of the transform.  EPA_F64: errors ~1e-16 of the strongest echo of the 2048-sample
 *                tile (the reference convolves in complex128 and stores complex64, ek80_complex.py:304-313).
 *                EPA_F32: complex64 butterflies, errors ~3e-7 of the tile's strongest echo -- for float32 output.
 *   workspace  : f64 [EPA_EK80_FFT_WS_DOUBLES(C, P, S)] (twiddles; ||tx||^2, span of the non-zero taps and
 *                conj(FFT(tx))/N per channel; range-statistics slots; one bit per tile marking tiles with a
 *                partly-NaN sample, which a second launch redoes sector by sector; the time-varied gain
 *                n log10(R') + 2 alpha R' of each channel's first ping by sample index, read instead of computed
 *                by every ping with the same range numbers; the logarithm's lookup table; rebuilt by every call)
 *   range_stats_out : optional f64 [3] = {nanmin, nanmax, NaN count} of the echo_range (written to range_out, or --
 *                range_out NULL -- left to epa_range_complex for whoever reads the array later), a by-product of the
 *                same pass (what compute_MVBS, commongrid/api.py:108-110, asks next) */
#define EPA_EK80_NFFT 2048
#define EPA_EK80_FFT_WS_DOUBLES(C, P, S)                                              \
  (768 + 4 * (size_t)(C) + 3 * (size_t)(C) * EPA_EK80_NFFT + 3 * 1024 + 2 +          \
   ((size_t)(C) * (size_t)(P) * ((size_t)(S) / (EPA_EK80_NFFT / 2 + 1) + 1) + 63) / 64 + \
   (size_t)(C) * ((size_t)(S) + 4) + 256)
int epa_sv_complex_fft(const void* re, const void* im, int in_dtype, const float* replica,
                       const int32_t* replica_off, int max_taps, const double* ccoef, int C, int P,
                       int S, int B, int cal_type, void* out, void* range_out, void* prx_out,
                       int out_dtype, int fft_dtype, double* workspace, double* range_stats_out,
                       epa_stream_t stream);
/* Self-test hook: the raw complex output of that transform's circular correlation alone.  x, out: n_tiles tiles of
 * EPA_EK80_NFFT interleaved (re, im) samples of fft_dtype; replica: interleaved f32, replica_off: i32 [2] = {0, taps}
 * (device), taps <= EPA_EK80_NFFT; out[t][k] = sum_j x[t][(k + j) mod EPA_EK80_NFFT] conj(replica[j]), through the
 * spectrum the replica preparation of epa_sv_complex_fft builds.  workspace: f64 [EPA_EK80_FFT_WS_DOUBLES(1, 1, 1)].
 * A test hook: the caller guarantees replica_off[1] - replica_off[0] <= EPA_EK80_NFFT (the offsets live on the
 * device and are not read back) and an n_tiles the arrays hold; one workgroup per tile. */
int epa_selftest_correlate(const void* x, int n_tiles, const float* replica, const int32_t* replica_off,
                           int fft_dtype, void* out, double* workspace, epa_stream_t stream);
/* ... with one replica per (channel, filter interval), as epa_sv_complex_indexed.  workspace: f64
 * [EPA_EK80_FFT_WS_DOUBLES(max(C, n_replicas), P, S)]. */
int epa_sv_complex_fft_indexed(const void* re, const void* im, int in_dtype, const float* replica,
                               const int32_t* replica_off, const int32_t* replica_id, int n_replicas, int max_taps,
                               const double* ccoef, int C, int P, int S, int B, int cal_type, void* out,
                               void* range_out, void* prx_out, int out_dtype, int fft_dtype, double* workspace,
                               double* range_stats_out, epa_stream_t stream);

/* ---- split-beam angles: consolidate.add_splitbeam_angle (consolidate/split_beam_angle.py) ----------------
 * Outputs theta (angle_alongship) and phi (angle_athwartship), [C*P*S] of out_dtype each.  The angle parameters
 * come as HOST arrays of 4 DEVICE pointers (f64) + their epa_param_mode (scalar, [C] or [C*P]), in the order
 * angle_sensitivity_alongship, angle_sensitivity_athwartship, angle_offset_alongship, angle_offset_athwartship. */
#define EPA_I8 2 /* in_dtype of epa_splitbeam_power only: the int8 electrical-angle steps a file stores */

/* Power/angle samples (split_beam_angle.py:121-171): theta = (180/128) * angle_alongship / sensitivity - offset,
 * phi likewise.  along / athw: [C*P*S] of in_dtype EPA_I8, EPA_F32 or EPA_F64 (NaN padding stays NaN). */
int epa_splitbeam_power(const void* along, const void* athw, int in_dtype, const double* const* params_host,
                        const int* modes_host, int C, int P, int S, void* theta, void* phi, int out_dtype,
                        epa_stream_t stream);

/* Complex samples (split_beam_angle.py:34-118, 174-270): re / im [C*P*S*B] (beam innermost, B = 3 or 4) of
 * in_dtype F32 / F64.  beam_type_host: HOST [C] int32 -- 1, 17, 49, 65 or 81, or -1 for a channel to skip (its rows
 * are NaN); C <= 64.  Types 1 / 49 / 65 / 81 need B = 4.
 * replica / replica_off NULL: no pulse compression (CW; BB without pulse compression) -- a streaming kernel.
 * Otherwise the combinations of the zero-filled sectors are matched-filtered with the replica (interleaved complex64;
 * replica_off [n_replicas + 1] in complex elements; replica_id optional [C*P] int32 as in epa_sv_complex_indexed, -1
 * = no replica: NaN) in the direct form; an angle is NaN where any sector its beam type uses is NaN at the sample.
 * Computed in out_dtype arithmetic. */
int epa_splitbeam_complex(const void* re, const void* im, int in_dtype, const int32_t* beam_type_host,
                          const double* const* params_host, const int* modes_host, const float* replica,
                          const int32_t* replica_off, const int32_t* replica_id, int n_replicas, int max_taps, int C,
                          int P, int S, int B, void* theta, void* phi, int out_dtype, epa_stream_t stream);

/* The same with pulse compression through the LDS-resident 2048-point FFT per tile (as epa_sv_complex_fft): replicas
 * of 1 .. EPA_EK80_NFFT/2 taps.  fft_dtype: arithmetic of the transform.  workspace: f64
 * [EPA_SPLITBEAM_FFT_WS_DOUBLES(n)] with n = n_replicas when replica_id is given, C otherwise (twiddles and the
 * replica spectra; rebuilt by every call). */
#define EPA_SPLITBEAM_FFT_WS_DOUBLES(n) (768 + 3 * (size_t)(n) * EPA_EK80_NFFT)
int epa_splitbeam_complex_fft(const void* re, const void* im, int in_dtype, const int32_t* beam_type_host,
                              const double* const* params_host, const int* modes_host, const float* replica,
                              const int32_t* replica_off, const int32_t* replica_id, int n_replicas, int max_taps,
                              int C, int P, int S, int B, void* theta, void* phi, int out_dtype, int fft_dtype,
                              double* workspace, epa_stream_t stream);

/* epa_sv_complex on CW samples (no replica) with {nanmin, nanmax, NaN count} of the echo_range as a by-product
 * (range_stats_out f64 [3]; merged through 1024 slots of f64 atomics in workspace, f64
 * [EPA_SV_COMPLEX_CW_STATS_WS_DOUBLES]); range_out may be NULL: the statistics are then those of the array
 * epa_range_complex would write.  Other arguments as epa_sv_complex. */
#define EPA_SV_COMPLEX_CW_STATS_WS_DOUBLES 3072
int epa_sv_complex_cw_stats(const void* re, const void* im, int in_dtype, const double* ccoef, int C, int P, int S,
                            int B, int cal_type, void* out, void* range_out, void* prx_out, int out_dtype,
                            double* workspace, double* range_stats_out, epa_stream_t stream);

/* echo_range of complex samples alone (range.py:98-157: (range_sample * sample_interval) * sound_speed / 2, NaN where
 * the real part of sector 0 is, :143-148) -- what epa_sv_complex / epa_sv_complex_fft write as range_out, for a caller
 * that left it out of the sample pass.  re as there ([C*P*S*B], in_dtype), range_out [C*P*S] of out_dtype. */
int epa_range_complex(const void* re, int in_dtype, const double* ccoef, int C, int P, int S, int B,
                      void* range_out, int out_dtype, epa_stream_t stream);

/* ==== SURVEY 8f "next" row 2: Ryan et al. (2015) noise masks + apply_mask ==============================
 * Masks are uint8 [C*P*S] (1 = True) in the (channel, ping_time, range_sample) layout of Sv.        */

/* Depth-bin smoothing used by mask_impulse_noise: every sample takes 10*log10 of the NaN-skipping
 * linear mean of its depth bin within its own ping.  Replaces clean/utils.py:244-304
 * (index_binning_downsample_upsample_along_depth: coarsen(range_sample=nper, "pad").mean + ffill;
 * range == NULL, bin b = s / nper -- call per channel, nper is channel specific) and :173-241
 * (downsample_upsample_along_depth: flox nanmean over bins np.arange(r0, max + bin, bin) closed on
 * the left, np.digitize up-sampling; range != NULL, nbins = len(edges) - 1).
 * sv, range, up_out: [C*P*S] of dtype.  (A ping with more bins than the LDS accumulators hold, ~13 000, is processed
 * in segments of bins.) */
int epa_range_bin_smooth(const void* sv, const void* range, int C, int P, int S, int nper, double r0,
                         double bin, int nbins, void* up_out, int dtype, epa_stream_t stream);

/* Two-sided ping comparison (clean/utils.py:307-323 echopy_impulse_noise_mask):
 * mask = (up[p] - up[p+n] > thr) & (up[p] - up[p-n] > thr), NaN differences count as +inf. */
int epa_impulse_mask(const void* up, int C, int P, int S, int num_side_pings, double threshold,
                     uint8_t* mask_out, int dtype, epa_stream_t stream);

/* Pooled Sv of mask_transient_noise, index-binning variant (clean/utils.py:109-170: dask_image
 * generic_filter over a (2*num_side_pings+1) x (2*num_side_samples+1) window of the linear Sv,
 * mode="reflect", restricted to range_sample >= first_sample; NaN above) and the mask
 * Sv - pooled > threshold (clean/api.py:166).  func: EPA_POOL_NANMEAN (separable box sums; needs
 * ws_sum f64 [C*P*S] and ws_cnt int32 [C*P*S]) or EPA_POOL_NANMEDIAN (exact; the window carried from ping to
 * ping with its histogram when it is at most 256 samples wide and fits LDS, a radix selection per output
 * sample otherwise; workspaces unused).
 * pooled_out ([C*P*S] of dtype) and mask_out may each be NULL. */
enum epa_pool_func { EPA_POOL_NANMEAN = 0, EPA_POOL_NANMEDIAN = 1 };
int epa_pool_sv(const void* sv, int C, int P, int S, int first_sample, int num_side_pings,
                int num_side_samples, int func, double threshold, void* pooled_out, uint8_t* mask_out,
                double* ws_sum, int32_t* ws_cnt, int dtype, epa_stream_t stream);

/* Attenuated-signal mask (clean/utils.py:326-372 echopy_attenuated_signal_mask, per channel):
 * per ping, up / lw = argmin |range - limit| of that ping (first NaN if any, as np.argmin); when
 * p-n >= 0, p+n <= P-1 and Sv[p, up:lw] is not all NaN, the whole ping is masked if
 * 10log10(nanmedian lin Sv[p, up:lw]) - 10log10(nanmedian lin Sv[p-n:p+n, up:lw]) < threshold.
 * S % 4 == 0, S >= 16 and a 4-byte aligned mask_out take the carried-block route (mask_out's rows hold the
 * per-ping limits and medians between its two kernels), anything else two selections per ping. */
int epa_attenuated_mask(const void* sv, const void* range, int C, int P, int S, double upper_limit,
                        double lower_limit, int num_side_pings, double threshold, uint8_t* mask_out,
                        int dtype, epa_stream_t stream);

/* out[i] = mask[i % mask_period] ? src[i] : fill  (mask/api.py:428-432 xr.where(final_mask, Sv,
 * fill_value)); fill = fill_array[i % fill_period] when fill_array != NULL, else fill_value.
 * mask_period = P*S broadcasts a channel-less mask over the channels. */
int epa_apply_mask(const void* src, const uint8_t* mask, size_t n, size_t mask_period,
                   double fill_value, const void* fill_array, size_t fill_period, void* out,
                   int dtype, epa_stream_t stream);

/* out[i] = (masks[0][i % p0] & ... & masks[n_masks-1][..]) ? src[i] : fill -- mask/api.py:402-432 in ONE sweep for a LIST
 * of masks (np.logical_and.reduce over the broadcast masks, :405-408, then xr.where, :428-432): 1 <= n_masks <= 4 (AND
 * further ones with epa_mask_and first); ``masks`` / ``mask_periods`` are HOST arrays of device pointers / periods.
 * minmax_out != NULL: f64 [2] on the device = NaN-skipping {min, max} of what was written (the variable's actual_range,
 * mask/api.py:434-444 via clean/utils.py:392-395), with workspace = f64 [EPA_APPLY_MASKS_WS_DOUBLES] on the device. */
#define EPA_APPLY_MASKS_WS_DOUBLES 131072
int epa_apply_masks(const void* src, const uint8_t* const* masks, const size_t* mask_periods, int n_masks, size_t n,
                    double fill_value, const void* fill_array, size_t fill_period, void* out, double* workspace,
                    double* minmax_out, int dtype, epa_stream_t stream);

/* out = a & b[i % b_period]  (mask/api.py:405-408, np.logical_and.reduce over broadcast masks). */
int epa_mask_and(const uint8_t* a, const uint8_t* b, size_t n, size_t b_period, uint8_t* out,
                 epa_stream_t stream);

/* Mean range step per channel, np.nanmean(np.diff(range, axis=2), axis=(1, 2)) (clean/utils.py:131,
 * :258: sizes the per-channel index bins).  workspace: f64 [2*C*P]; out: f64 [C] (NaN: no finite step). */
int epa_range_step_mean(const void* range, int C, int P, int S, int dtype, double* workspace,
                        double* out, epa_stream_t stream);

/* Flat index of the first element that is not <= limit (NaN counts); n when there is none.
 * np.argmin(range <= exclude_above) of clean/utils.py:143.  x: [n] of dtype; out: uint64 [1]. */
int epa_first_not_le(const void* x, size_t n, double limit, int dtype, uint64_t* out,
                     epa_stream_t stream);

/* Row check of a range variable for the value-window pooling below: nvalid_out int32 [C*P] = index of
 * the first NaN of each (c,p) row (S if none); violations_out int32 [1] = number of rows that are not
 * non-decreasing over their valid prefix or hold a number after their first NaN. */
int epa_range_rows_check(const void* range, int C, int P, int S, int dtype, int32_t* nvalid_out,
                         int32_t* violations_out, epa_stream_t stream);

/* Pooled Sv of mask_transient_noise, value-window variant (clean/utils.py:29-106 pool_Sv, a triple
 * Python loop in the reference): for the sample at depth d of ping p, func over the linear Sv of pings
 * p-n..p+n (clipped to the data) with range in [d - depth_bin, d + depth_bin]; NaN where
 * d - bin < range_min, d + bin > range_max, d - bin < exclude_above, p - n < 0 or p + n > P.
 * range rows must pass epa_range_rows_check (nvalid from it).  func / threshold / outputs as epa_pool_sv. */
#define EPA_POOL_VALUE_WS_BYTES(C, P, S) \
  ((size_t)(C) * (P) * (S) * 40 + (size_t)(C) * (S) * 8 + (size_t)(C) * 8 + (size_t)(C) * (P))
/* ws (optional, nanmean only): EPA_POOL_VALUE_WS_BYTES bytes, 8-byte aligned.  With it a channel whose pings all share
 * one range vector (checked on the device) gets per-row interval sums (blocks of 16 samples, no subtraction) + a
 * sliding sum down every column, O(1) per sample; any other channel per-row running sums kept in double-double,
 * O(pings) per sample.  Without it every window is summed value by value.  Same results to rounding. */
/* ws for func = nanmedian (optional): EPA_POOL_VALUE_MEDIAN_WS_BYTES bytes, 4-byte aligned.  With it the channels whose
 * pings share one range vector carry their window from ping to ping (a histogram of the window kept up to date, the
 * median's bin ranked exactly): O(window columns) per sample instead of O(window).  Same results. */
#define EPA_POOL_VALUE_MEDIAN_WS_BYTES(C, S) (((size_t)(C) * (S) * 2 + (size_t)(C) * 2) * 4)
int epa_pool_sv_value(const void* sv, const void* range, const int32_t* nvalid, int C, int P, int S,
                      double depth_bin, int num_side_pings, double exclude_above, double range_min,
                      double range_max, int func, double threshold, void* pooled_out, uint8_t* mask_out,
                      void* ws, int dtype, epa_stream_t stream);

/* ==== SURVEY 8f "next" row 3: compute_NASC ==============================================================
 * Array pass of commongrid/utils.py:97-205 (compute_raw_NASC): NASC = sv_mean * h_mean * 4*pi*1852^2 with
 * sv_mean the (nan)mean of the linear Sv per (channel, distance bin, depth bin) and h_mean the nansum of
 * diff(depth) (labelled by its lower sample) per cell divided by the pings of the distance bin.
 *   sv, depth : [C*P*S] of dtype, pings ordered by cumulative distance
 *   bin_start : int32 [n_dbins+1], pings bin_start[d] .. bin_start[d+1]-1 belong to distance bin d
 *   depth bins: edges i*range_bin, i = 0..n_rbins (np.arange(0, max + bin, bin), api.py:351)
 *   bin_flags : EPA_BIN_SKIPNA, EPA_BIN_CLOSED_RIGHT (depth bins; the distance side is in bin_start)
 *   workspace : 24 * C*n_dbins*n_rbins bytes (zeroed by the call); a depth grid too fine for the LDS accumulators
 *               (> ~6500 bins) is accumulated straight into it with atomics
 *   nasc_out  : [C*n_dbins*n_rbins] of dtype; sv_mean_out / h_mean_out likewise, optional */
/* Along-track step of every ping for compute_NASC's distance bins: step_m_out[i] = WGS-84 geodesic length in metres
 * from ping i to ping i + 1 (Vincenty's inverse formula; NaN for the last ping and wherever a position is NaN), the
 * quantity commongrid/utils.py:208-231 takes from geopy.distance.distance ping by ping.  lat / lon: f64 [P], degrees. */
int epa_geodesic_steps(const double* lat, const double* lon, int P, double* step_m_out, epa_stream_t stream);
int epa_nasc(const void* sv, const void* depth, int C, int P, int S, const int32_t* bin_start, int n_dbins,
             double range_bin, int n_rbins, unsigned bin_flags, void* workspace, void* nasc_out,
             void* sv_mean_out, void* h_mean_out, int dtype, epa_stream_t stream);

/* ==== the whole north-star chain in two passes ==========================================================
 * compute_Sv -> remove_background_noise -> compute_MVBS as four separate calls moves 84 B/sample in
 * fp64 (K1 20, K6 16, K7 32, K5 16); these two entry points do the same arithmetic in 12 + 16..24.
 *
 * Pass 1 = K1 + K6: Sv (and optionally echo_range) written once, the noise estimate of
 * clean/api.py:397-422 accumulated from the Sv values still in registers (transmission loss from the
 * coefficient rows).  Arguments as epa_sv_power and epa_noise_estimate.  sv_out may be NULL;
 * range_max_out (f64 [1], optional) = nanmax(echo_range), which sizes the range grid of pass 2;
 * range_stats_out (f64 [3], optional, needs range_max_out) = {nanmin, nanmax, NaN count} of the echo_range as
 * epa_sv_mvbs_fused leaves them ({NaN, NaN, -1} when the generic kernel serves the configuration). */
/* A ping shard of a longer file: ping_phase = (global index of the shard's first ping) % ping_num, i.e. local
 * ping p belongs to noise block (p + ping_phase) / ping_num and noise_out has ceil((P + ping_phase) / ping_num) columns;
 * edge_sum_out f64 [2][C][Sb] / edge_cnt_out u32 [2][C][Sb] (optional, together; zero them first) receive the raw linear
 * (sum, count) per range block of the shard's FIRST and LAST ping block -- what a block cut by a shard edge contributes to
 * the mean over all its pings (clean/api.py:402-411); a shard with a single block fills slot 0 only.  As
 * epa_noise_estimate. */
int epa_sv_noise_fused(const float* raw, const double* coef, const double* alpha2, int C, int P, int S,
                       int cal_type, unsigned cal_flags, int ping_num, int range_sample_num, int ping_phase,
                       double noise_max, void* sv_out, void* range_out, double* noise_out, double* edge_sum_out,
                       uint32_t* edge_cnt_out, double* range_max_out, double* range_stats_out, int dtype,
                       epa_stream_t stream);

/* Pass 2 = K7 + K5: reads Sv once, applies clean/api.py:425-430,485-487 with the per-ping-block noise
 * of pass 1 and bins the CORRECTED Sv (commongrid/utils.py:592-627) in the same sweep.  Arguments as
 * epa_noise_apply (sv, range | coef, alpha2, noise, ping_num, snr_threshold) and epa_mvbs (bins,
 * outputs); sv_noise_out / sv_corrected_out ([C*P*S] of dtype) may each be NULL. */
/* (With `coef` instead of `range`, Sv_noise is finite at NaN-padded samples, where the reference's
 * echo_range -- and therefore its Sv_noise -- is NaN; Sv_corrected and the MVBS are unaffected.) */
int epa_denoise_mvbs(const void* sv, const void* range, const double* coef, const double* alpha2,
                     const double* noise, int C, int P, int S, int ping_num, double snr_threshold,
                     const int32_t* bin_start, const int32_t* ping_perm, int n_tbins, double range_bin,
                     int n_rbins, unsigned bin_flags, double fill_value, void* sv_noise_out,
                     void* sv_corrected_out, void* mvbs_out, void* sum_out, uint32_t* cnt_out, int dtype,
                     epa_stream_t stream);

/* Pass 2 fed with the RAW power again instead of Sv (4 B/sample read instead of 8, and the NaN padding
 * that masks echo_range is seen directly): Sv is recomputed in registers as in epa_sv_power, then as
 * epa_denoise_mvbs.  With pass 1 the chain costs 4 + 8 (Sv) and 4 + 8 (Sv_corrected) [+ 8 Sv_noise]
 * = 24..32 B/sample.  range_out optional as in epa_sv_power.  minmax_out (f64 [4], optional): NaN-skipping
 * {min, max} of Sv_noise and {min, max} of Sv_corrected as a by-product (the actual_range attributes of
 * clean/utils.py:392-395, otherwise one more sweep of each array). */
/* ping_phase as in epa_sv_noise_fused: the noise of local ping p is noise[c][(p + ping_phase) / ping_num]. */
int epa_sv_denoise_mvbs(const float* raw, const double* coef, const double* alpha2, const double* noise,
                        int C, int P, int S, int cal_type, unsigned cal_flags, int ping_num, int ping_phase,
                        double snr_threshold, const int32_t* bin_start, const int32_t* ping_perm,
                        int n_tbins, double range_bin, int n_rbins, unsigned bin_flags, double fill_value,
                        void* sv_noise_out, void* sv_corrected_out, void* range_out, void* mvbs_out,
                        void* sum_out, uint32_t* cnt_out, double* minmax_out, int dtype, epa_stream_t stream);

/* ---- seafloor detection: mask.detect_seafloor (mask/seafloor_detection/) -----------------------------------------
 * One channel's (ping, range) planes: sv / theta / phi / depth are [P*S] of dtype F32 / F64, row by ping.  A crop is
 * the range samples [r0, r0 + R) of every ping.  depth0: f64 [S], the channel's depth at ping 0.  state: u64
 * [EPA_SEAFLOOR_STATE_WORDS], zeroed by the caller: [0] pixels under the angle mask, [1] non-NaN Sv values under it,
 * [6] / [7] the lower / upper middle of those values (f64 bits), [8] union-find loops that reached their bound
 * (non-zero: the components are not to be trusted). */
#define EPA_SEAFLOOR_STATE_WORDS 16

/* utils.py:_check_inputs: *bad_pings (device int, zeroed by the caller) += the pings whose max over range of
 * |depth - depth[ping 0]| (NaN skipped) is not < 1e-16 in the array's type, or is NaN. */
int epa_seafloor_depth_uniform(const void* depth, int dtype, long long P, long long S, int* bad_pings,
                               epa_stream_t stream);

/* bottom_basic.py: out (f64 [P]) = depth0[s] - offset for the first s >= skip with tmin < sv < tmax (the bounds
 * rounded to dtype first, as NumPy compares them), s = skip where no sample matches; 0 <= skip < S. */
int epa_seafloor_basic(const void* sv, int dtype, long long P, long long S, long long skip, double tmin, double tmax,
                       const double* depth0, double offset, double* out, epa_stream_t stream);

/* bottom_blackwell.py, angle mask: mask (u8 [P*R]) = 1 where mean_w(theta)^2 > ttheta or mean_w(phi)^2 > tphi, the
 * means over wtheta^2 / wphi^2 windows of convolve2d(..., "same", boundary="symm") on the crop; state[0] += the
 * count.  work: f64 [2*P*R]. */
int epa_seafloor_angle_mask(const void* theta, const void* phi, int dtype, long long P, long long S, long long r0,
                            long long R, int wtheta, int wphi, double ttheta, double tphi, double* work,
                            unsigned char* mask, unsigned long long* state, epa_stream_t stream);

/* The one or two middle values of the non-NaN sv under mask (radix select on the crop): state[1], [6], [7].
 * hist: u64 [512]. */
int epa_seafloor_median(const void* sv, int dtype, long long P, long long S, long long r0, long long R,
                        const unsigned char* mask, unsigned long long* state, unsigned long long* hist,
                        epa_stream_t stream);

/* 8-connected components of sv > threshold (threshold rounded to dtype) on the crop: parent (i64 [P*R]) = the root
 * of each foreground pixel, -1 elsewhere; bit 1 of mask[root] set for every component with a pixel under the mask. */
int epa_seafloor_components(const void* sv, int dtype, long long P, long long S, long long r0, long long R,
                            double threshold, unsigned char* mask, long long* parent, unsigned long long* state,
                            epa_stream_t stream);

/* out [P] of out_dtype = depth0[r0 + i] - offset for the first crop sample i of each ping whose component is kept,
 * depth0[0] - offset where there is none; parent == NULL: depth0[0] - offset for every ping. */
int epa_seafloor_bottom(const long long* parent, const unsigned char* mask, long long P, long long R, long long r0,
                        const double* depth0, double offset, void* out, int out_dtype, epa_stream_t stream);

/* ---- shoal detection: mask.detect_shoal (mask/shoal_detection/) ---------------------------------------------------
 * One (ping, range) plane, row by ping: sv is [P*S] of dtype F32 / F64; plane is u8 [P*S] (0 / 1: it is the boolean
 * result in the end); parent is i64 [P*S].  The component table has cap entries, at least the
 * most components the plane can hold ((P*S + 1) / 2 with connectivity 4, ceil(P/2) * ceil(S/2) with 8) and at most 0x70000000: box i32 [4*cap] (min sample, max sample, min ping, max ping, one plane each),
 * flag i32 [cap], and for echoview group i32 [cap].  state: u64 [EPA_SHOAL_STATE_WORDS], zeroed by the caller:
 * [0] union-find loops that reached their bound (non-zero: the result is not to be trusted), [1] components. */
#define EPA_SHOAL_STATE_WORDS 8
#define EPA_SHOAL_QUEUE_BOXES 4096
/* the two state words a caller reads: [0] and [1] above */
#define EPA_SHOAL_STATE_ERROR 0
#define EPA_SHOAL_STATE_COUNT 1

/* plane = sv > thr (compared in f64: thr is not rounded to dtype; NaN background); then along range in every ping, runs of background of at
 * most maxvgap samples with foreground on both sides become foreground; then, on that result, the same along pings
 * at every sample with maxhgap. */
int epa_shoal_threshold_fill(const void* sv, int dtype, long long P, long long S, double thr, long long maxvgap,
                             long long maxhgap, unsigned char* plane, epa_stream_t stream);

/* Connected components (connectivity 4 or 8) of the non-zero bytes of plane: parent = -(id + 2) on the pixels of
 * component id (ids 0 .. state[1] - 1 in no particular order), -1 on background; box[.][id] its bounding box;
 * flag[id] = 0. */
int epa_shoal_label(const unsigned char* plane, long long P, long long S, int connectivity, long long* parent,
                    int* box, int* flag, long long cap, unsigned long long* state, epa_stream_t stream);

/* shoal_weill.py, size filter: plane = 1 on the pixels of the components whose extents (max - min + 1) are not below
 * minvlen (samples) / minhlen (pings), 0 elsewhere.  parent / box / flag: of epa_shoal_label(..., 4, ...). */
int epa_shoal_weill_filter(const long long* parent, long long P, long long S, const int* box, int* flag,
                           long long cap, double minvlen, double minhlen, unsigned long long* state,
                           unsigned char* plane, epa_stream_t stream);

/* shoal_echoview.py after the labelling (parent / box / flag: of epa_shoal_label(..., 8, ...); box and flag are
 * overwritten): candidates below mincan removed, the survivors linked through their boxes grown by maxlink + 1,
 * groups below minsho removed; plane = 1 on what is left.  idim (f64 [ni], ni >= S + 1) and jdim (f64 [nj],
 * nj >= P + 1) on the device, nondecreasing and finite.  queue: i32 [2 * EPA_SHOAL_QUEUE_BOXES]. */
int epa_shoal_echoview_link(const long long* parent, long long P, long long S, int* box, int* group, int* flag,
                            long long cap, const double* idim, long long ni, const double* jdim, long long nj,
                            double mincan0, double mincan1, double maxlink0, double maxlink1, double minsho0,
                            double minsho1, int* queue, unsigned long long* state, unsigned char* plane,
                            epa_stream_t stream);

/* ---- region tables: mask.label_regions, mask.region_statistics (mask/regions.py) -------------------------------------
 * code: the parent plane epa_shoal_label left, i64 [P*S]: -(id + 2) on the pixels of component id, -1 on background.
 * n: the number of components, state[EPA_SHOAL_STATE_COUNT] as the host read it (1 .. min(P*S, 0x70000000)).
 *
 * The per-(channel, id) table: EPA_REGION_WORDS 64-bit words per entry, counts as u64, sums as f64 bits, extrema as
 * order-preserving keys (key 0: nothing seen; else the f64 bits with the sign bit set for v >= 0, all bits inverted
 * for v < 0).  With sv = 10^(Sv / 10) in f64, r the range and dz[s] = r[s] - r[s-1] (dz[0] = dz[1]; NaN when S == 1),
 * every word skips the pixels where one of its own operands is NaN: */
enum epa_region_word {
  EPA_REGION_N_VALID = 0,        /* pixels whose Sv is not NaN */
  EPA_REGION_N_RANGE = 1,        /* pixels whose r is not NaN */
  EPA_REGION_SV_MAX = 2,         /* key of max Sv */
  EPA_REGION_RANGE_MIN = 3,      /* key of max(-r): the minimum of r, negated */
  EPA_REGION_RANGE_MAX = 4,      /* key of max r */
  EPA_REGION_SUM_SV = 5,         /* sum sv */
  EPA_REGION_SUM_RANGE = 6,      /* sum r */
  EPA_REGION_SUM_SV_RANGE = 7,   /* sum sv r, over the pixels with both */
  EPA_REGION_SUM_SV_AT_RANGE = 8,/* sum sv over the same pixels */
  EPA_REGION_SUM_DZ = 9,         /* sum dz */
  EPA_REGION_SUM_SV_DZ = 10      /* sum sv dz, over the pixels with both */
};
#define EPA_REGION_WORDS 11
/* The per-id table: EPA_REGION_ID_WORDS u64 words per entry. */
#define EPA_REGION_ID_SAMPLES 0 /* pixels of the component */
#define EPA_REGION_ID_FIRST 1   /* P*S - (its smallest linear pixel index ping * S + sample); 0: the id was never met */
#define EPA_REGION_ID_WORDS 2

/* One sweep over the code plane and the C planes of sv and range (dtype F32 / F64, converted to f64 exactly; every
 * sum is f64): stats u64 [C*n*EPA_REGION_WORDS] and ids u64 [n*EPA_REGION_ID_WORDS], both zeroed by the caller, are
 * added to.  sv is [C*P*S]; the sample (c, p, s) of the range is range[c * range_stride_c + p * range_stride_p + s]
 * (element strides >= 0; 0 shares a row between channels / pings: nothing has to be expanded).  C == 0: ids alone
 * (sv, range and stats may be NULL).  A code that names no id in [0, n) adds 1 to state[EPA_SHOAL_STATE_ERROR] and
 * writes nothing.  Updates are combined over runs of equal code inside a wave and along the pings a wave walks: the
 * tables take one update per run, not one per pixel.  Sums can differ in their last bits between two calls (the
 * order of the updates); counts and extrema cannot. */
int epa_region_stats(const long long* code, long long P, long long S, const void* sv, const void* range, int dtype,
                     long long C, long long range_stride_c, long long range_stride_p, long long n,
                     unsigned long long* stats, unsigned long long* ids, unsigned long long* state,
                     epa_stream_t stream);

/* labels i32 [P*S] = rank[id] on the pixels of component id (rank i32 [n]: the number the caller gives each id),
 * 0 on background and on codes that name no id in [0, n). */
int epa_region_labels(const long long* code, long long P, long long S, const int* rank, long long n, int* labels,
                      epa_stream_t stream);

/* ---- transient-noise detectors: clean.detect_transient (clean/transient_noise/) -------------------------------------
 * sv is [C*P*S] of dtype F32 / F64, mask_out u8 [C*P*S]: 1 = VALID, 0 = transient noise; written completely by the
 * call.  The scalars that depend on the range row alone come from the host, one row per channel, in device tables.
 *
 * Fielding (transient_fielding.py): chan i32 [C*4] = up, lw, rmin, sf.  Ping j is flagged when j - n >= 0,
 * j + n <= P - 1, its layer [up, lw) is not all NaN, 10log10(75th percentile of the linear layer) < maxts and
 * 10log10(nanmedian lin layer of j) - 10log10(nanmedian lin layer of pings [j-n, j+n)) > thr0; a flagged ping walks up
 * in steps of sf samples while the window start is above rmin, stops after the first window whose median difference
 * is below thr1, and is masked from one step above that window (Python slice semantics for a negative start).
 * up >= lw: the channel is left all-valid.  max_rows: the most samples any window has (bounds 2 * n * max_rows).
 * list i64 [C*P] and count u32 [1] are scratch. */
int epa_transient_fielding(const void* sv, int dtype, int C, int P, int S, const int* chan, int max_rows, int n,
                           double thr0, double thr1, double maxts, long long* list, unsigned* count,
                           uint8_t* mask_out, epa_stream_t stream);

/* Matecho (transient_matecho.py): range f64 [C*S], the channel's range row; chan_i i32 [C*2] = s_lo, s_top, the run of
 * samples inside [start_depth, start_depth + window_meter], nondecreasing in range; chan_d f64 [C*2] = r[1] - r[0],
 * r[-1].  bottom f64 [bottom_rows*P] with bottom_rows 1 or C, or NULL with 0; NaN entries count as r[-1].  For ping j,
 * h = half_window, j0 = max(0, j-h), j1 = min(P, j+h): the window samples are [s_lo, s_hi(j)), s_hi the first of the
 * run that is not below min(bottom[j0:j1]) (float64 comparison); skipped when there is none, when
 * (r[1]-r[0]) * count < min_window or when the ping has no value; flagged when 10log10(nanmean lin Sv[j, samples]) >
 * percentile (np.percentile, linear, of the non-NaN dB values of pings [j0, j1) x samples) + delta_db.  Flags are
 * dilated by extend_ping pings on each side; a flagged ping is masked over its whole column.
 * s_hi i32 [C*P] and flag u8 [C*P] are scratch. */
int epa_transient_matecho(const void* sv, int dtype, int C, int P, int S, const double* range, const int* chan_i,
                          const double* chan_d, const double* bottom, int bottom_rows, int half_window,
                          double percentile, double delta_db, int extend_ping, double min_window, int* s_hi,
                          uint8_t* flag, uint8_t* mask_out, epa_stream_t stream);

/* ---- masks from Sv differences and masks on the MVBS grid: mask.frequency_differencing / mask.regrid_mask ------------
 * mask_out[i] = (sv[chan_a*n + i] - sv[chan_b*n + i]) cmp diff (mask/api.py:593-608): sv [C*n] of dtype F32 / F64,
 * mask_out u8 [n].  NumPy's arithmetic for an array and a Python scalar: the difference is rounded in dtype and diff
 * is converted to dtype before the comparison (float32 data: fl32(a - b) against fl32(diff)).  NaN on either side and
 * inf - inf give 0 for all five operators. */
enum epa_cmp { EPA_CMP_GT = 0, EPA_CMP_LT = 1, EPA_CMP_LE = 2, EPA_CMP_GE = 3, EPA_CMP_EQ = 4 };
int epa_freq_diff_mask(const void* sv, int C, size_t n, int chan_a, int chan_b, int cmp, double diff,
                       uint8_t* mask_out, int dtype, epa_stream_t stream);

/* A mask on the (ping-time bin, range bin) grid of compute_MVBS (mask/api.py:759-841: a group-by mean followed by
 * == 1.0 / != 0.0, kept here as two flags per cell: did any sample fall into it, did any zero (AND) / any one (OR)).
 *   mask   : u8 [T*P*D] (T = 1 without a third dimension); the low bit of a byte is its value
 *   group  : i32 [T] on the device or NULL (identity): the output slice of every input slice; its values are exactly
 *            0 .. G-1, each at least once (slices with the same value merge their samples)
 *   range  : f64 [D], or [P*D] when range_per_ping != 0; NaN: the sample belongs to no cell
 *   bin_start : i32 [n_tbins+1] (epa_time_bin_offsets); range edges e_i = i*range_bin, i = 0..n_rbins, the side
 *            EPA_BIN_CLOSED_RIGHT of bin_flags selects closed; samples outside the edges are dropped
 *   func   : 0 = AND (1 where a cell holds samples and all are one), 1 = OR (1 where it holds a one); empty cells are 0
 *   out    : u8 [G*n_tbins*n_rbins], 4-byte aligned, in an allocation that reaches the next multiple of 4 bytes (the
 *            flags are merged with 32-bit atomics; bytes past the last cell keep their value)
 *   nonbinary_out : i32 [1], non-zero when a mask byte is neither 0 nor 1 (np.isin(mask, [1, 0]).all(), :752)
 * The result does not depend on the order in which workgroups finish. */
int epa_regrid_mask(const uint8_t* mask, const int32_t* group, int T, int P, int D, const double* range,
                    int range_per_ping, const int32_t* bin_start, int n_tbins, double range_bin, int n_rbins,
                    unsigned bin_flags, int func, uint8_t* out, int32_t* nonbinary_out, epa_stream_t stream);

/* ---- mask.line_mask: the samples between two lines ---------------------------------------------------------------------
 * out[c, p, s] = ub <= r < lb, or ub < r <= lb with EPA_LINE_CLOSED_RIGHT, for r the range of sample (c, p, s) and
 * ub = upper[c, p] + upper_offset, lb = lower[c, p] + lower_offset (one float64 addition each).  out u8 [C*P*S],
 * contiguous, any alignment; one launch, no scratch.  All comparisons are float64 on r promoted exactly from dtype, so
 * the result is NumPy's for r.astype(float64) against the float64 bounds: r NaN gives 0, +-inf compare as numbers.
 *   upper, lower : f64 on the device, element (c, p) at [c*stride_c + p*stride_p], a stride of 0 broadcasts (a scalar
 *            bound: one element, both strides 0); NULL: that bound is not tested (at least one is given).  A bound
 *            that is NaN at (c, p) makes the whole row 0, or, with EPA_LINE_NAN_IGNORE, is not tested in that row.
 *   the range, one of two forms:
 *     range : an array of dtype (F32 / F64), element (c, p, s) at [c*range_stride_c + p*range_stride_p +
 *            s*range_stride_s], a stride of 0 broadcasts: (S,), (C, S), (P, S) and (C, P, S) ranges are read where they lie
 *     coef  : f64 [C*P*EPA_NCOEF] power-sample coefficient rows: r = (dtype)(fl(fl(s*ra)*rb) + r0), NaN where nan_raw
 *            (f32 [C*P*S], or NULL) is NaN, then, when scale and offset (f64 [C*P], both or neither) are given,
 *            r = (dtype)offset + fl((dtype)scale * r) in dtype: the values epa_range_power / epa_depth_rows write, bit for
 *            bit, so the decisions are those on the written array, which is not needed
 * Negative strides, S > 2^30 and a NaN offset are refused. */
#define EPA_LINE_CLOSED_RIGHT 1u /* (ub, lb] instead of [ub, lb) */
#define EPA_LINE_NAN_IGNORE 2u   /* a NaN bound is not tested instead of emptying its row */
int epa_line_mask(const void* range, long long range_stride_c, long long range_stride_p, long long range_stride_s,
                  const double* coef, const float* nan_raw, const double* scale, const double* offset, int dtype,
                  const double* upper, long long upper_stride_c, long long upper_stride_p, double upper_offset,
                  const double* lower, long long lower_stride_c, long long lower_stride_p, double lower_offset,
                  unsigned flags, int C, int P, int S, uint8_t* out, epa_stream_t stream);

/* ---- commongrid.regrid_Sv: Sv onto one range grid, the echo integral kept ------------------------------------------------
 * Every row (c, p) of sv [C*P*S] (dtype F32 / F64, contiguous) is resampled onto the cells [j*range_bin, (j+1)*range_bin),
 * j = 0 .. n_rbins-1 (the edges of np.arange(0, max + bin, bin): compute_MVBS's grid).  For one row, with r the range
 * promoted to float64 (F32 promotes exactly) and v its Sv:
 *   n    = the length of the leading run of finite r (S if all are); samples behind it are ignored
 *   the row is REFUSED if n < 2 or r[0..n) decreases somewhere: its outputs are NaN / coverage 0, and it is counted
 *   m[i] = (r[i-1] + r[i]) / 2 for 0 < i < n, m[0] = r[0] - (r[1] - r[0]) / 2, m[n] = r[n-1] + (r[n-1] - r[n-2]) / 2:
 *          sample i stands for [m[i], m[i+1]); a cell of zero width contributes nothing
 *   o_ij = max(0, min(m[i+1], e[j+1]) - max(m[i], e[j])),  W_j = sum_i o_ij,  N_j = sum_i o_ij * 10^(v_i / 10), over the
 *          i < n with v_i not NaN and o_ij > 0, in ascending i (-inf is a sample of linear value 0, +inf gives +inf)
 *   sv_out[row*n_rbins + j] = 10 log10(N_j / W_j) where W_j > 0, else NaN;  coverage_out[...] = W_j / (e[j+1] - e[j])
 * All of it in float64, the two outputs rounded once to dtype.  One kernel launch, a workgroup per row, rows longer than
 * EPA_REGRID_TILE samples in tiles of that length; no scratch.  Every element of sv_out and (if given) coverage_out is
 * stored exactly once, nothing is pre-filled; n_unordered_out is set to 0 by a 4-byte memset in front of the launch.
 *   range : of range_dtype (F32 / F64, need not be dtype), element (c, p, s) at [c*range_stride_c + p*range_stride_p +
 *            s*range_stride_s] in elements, a stride of 0 broadcasts: (S,), (C, S) and (C, P, S) ranges are read where
 *            they lie
 *   coverage_out : of dtype [C*P*n_rbins], or NULL: not written
 *   n_unordered_out : i32 [1] on the device, the number of refused rows (also with n_rbins == 0)
 *   max_grid : the most workgroups to launch, 0: the library's choice (tests: the row loop at small shapes)
 * EPA_EINVAL (nothing is launched): a bad dtype; C, P or S negative; S or n_rbins above 2^30; range_bin not positive and
 * finite; a negative stride or max_grid; n_unordered_out NULL; sv or range NULL with C*P*S > 0; sv_out NULL with
 * C*P*n_rbins > 0. */
#define EPA_REGRID_TILE 2048 /* source samples of a row that lie in LDS at a time */
int epa_regrid_rows(const void* sv, int dtype, const void* range, int range_dtype, long long range_stride_c,
                    long long range_stride_p, long long range_stride_s, int C, int P, int S, double range_bin,
                    int n_rbins, void* sv_out, void* coverage_out, int32_t* n_unordered_out, int max_grid,
                    epa_stream_t stream);

/* ---- clean.window_filter: NaN-aware median, mean, min and max windows on Sv ----------------------------------------------
 * x [C*P*S] (dtype F32 / F64, contiguous) -> out of the same type and shape.  THE RULE.  With hp = ping_num / 2 and hs =
 * range_sample_num / 2 (both sizes odd, 1 .. EPA_WINDOW_FILTER_MAX), the window of (c, p, s) is the samples (c, p', s')
 * with |p' - p| <= hp and |s' - s| <= hs that lie inside the array: it shrinks at the edges (no reflection, no padding
 * value) and never crosses channels.  Its VALID values are those that are not NaN; -inf and +inf are values, ordered as
 * usual, in every method.  With n the number of valid values:
 *   EPA_WINDOW_MEDIAN : n odd: the middle valid value, an input bit for bit.  n even: with a <= b the two middle values,
 *                       a itself when a == b (no round trip through the exponential), else
 *                       10 log10((10^(a/10) + 10^(b/10)) / 2): the median of the linear values
 *   EPA_WINDOW_MEAN   : 10 log10(sum of 10^(v/10) over the valid v / n); -inf if all of them are -inf, +inf if any is +inf
 *   EPA_WINDOW_MIN / EPA_WINDOW_MAX : the smallest / largest valid value, an input bit for bit (erosion / dilation)
 *   out = NaN where n < min_valid (1 .. ping_num * range_sample_num; a window without a valid value is always NaN), and,
 *   with keep_nan != 0, where x itself is NaN whatever its neighbours hold; with keep_nan == 0 such a sample gets its
 *   window's result.
 * What is not a selection (the mean's exponentials, sum and logarithm; the even median's two exponentials and logarithm)
 * is float64 for both types and rounded once to dtype.  One kernel launch; a workgroup owns a tile of EPA_WINDOW_FILTER_TP
 * pings x EPA_WINDOW_FILTER_TS samples and reads it with its halo from LDS, where array positions outside the array are
 * NaN; every element of out is stored exactly once, nothing is pre-filled; no scratch.
 *   max_grid : the most workgroups to launch, 0: the library's choice (tests: the tile loop at small shapes)
 * EPA_EINVAL (nothing is launched): a bad dtype or method; C, P or S negative; an even size or one outside 1 ..
 * EPA_WINDOW_FILTER_MAX; min_valid outside 1 .. ping_num * range_sample_num; a negative max_grid; x or out NULL with
 * C*P*S > 0; out overlapping x (a neighbour's halo would read results); more than 2^31 - 1 tiles. */
enum epa_window_method { EPA_WINDOW_MEDIAN = 0, EPA_WINDOW_MEAN = 1, EPA_WINDOW_MIN = 2, EPA_WINDOW_MAX = 3 };
#define EPA_WINDOW_FILTER_MAX 15 /* the largest window size along either axis */
#define EPA_WINDOW_FILTER_TP 16 /* pings of a workgroup's tile */
#define EPA_WINDOW_FILTER_TS 64 /* samples of a workgroup's tile */
int epa_window_filter(const void* x, int dtype, int C, int P, int S, int method, int ping_num, int range_sample_num,
                      int min_valid, int keep_nan, void* out, int max_grid, epa_stream_t stream);

/* ---- echo summary statistics per row: metrics.abundance / center_of_mass / dispersion / evenness / aggregation --------
 * (metrics/summary_statistics.py).  sv [R*S] and range of dtype F32 / F64; range is [R*S] when range_per_row != 0,
 * else [S], shared by all rows.  For j = 1 .. S-1: dz_j = range_j - range_{j-1} rounded in dtype, 0 -> NaN;
 * lin_j = 10^(sv_j / 10) (F32: exp10f(sv_j * 0.1f)); w_j = lin_j dz_j.  In double, each sum skipping its NaN terms (an
 * all-NaN row, and S <= 1, sum to 0):  A = sum w_j,  B = sum range_j w_j,  Q = sum lin_j^2 dz_j,
 * I = sum (range_j - cm)^2 w_j with cm = B / A of the same row, or cm_in[row] when cm_in (f64 [R], device) is given.
 *   abundance = 10 log10 A, center_of_mass = B / A, dispersion = I / A, evenness = A^2 / Q, aggregation = Q / A^2,
 * each [R] of dtype, rounded once; a NULL output is not computed, at least one is wanted.  +-inf, negative dz and 0/0
 * follow IEEE.  Every array may start at any element.  A row is reduced by one wave (S <= 2048) or one workgroup, in a
 * fixed order: the result does not depend on scheduling, nor on which other outputs are asked for, nor on max_grid:
 * the most workgroups to launch, 1 .. 65536, 0 = 65536 (waves and workgroups beyond take further rows in a loop). */
int epa_echo_metrics(const void* sv, const void* range, int range_per_row, long long R, long long S,
                     const double* cm_in, void* abundance, void* center_of_mass, void* dispersion, void* evenness,
                     void* aggregation, int dtype, int max_grid, epa_stream_t stream);

/* ---- utils.align.align_to_ping_time / consolidate.add_location: values on an external clock brought onto ping_time ------
 * t_ext [N] int64 ns, strictly increasing, no NaT; y [V*N] f64, V rows of N values; ping_time [P] int64 ns in any order,
 * INT64_MIN = NaT; out [V*P] f64.  All device arrays.  One search per ping serves all V rows.
 * With x_i = (double)(t_ext[i] - t_ext[0]), q = (double)(ping_time[p] - t_ext[0]) (integer difference, one conversion)
 * and k = clamp(first i with x_i >= q, 1, N-1):
 *   mode 0, linear: out = ((y[k] - y[k-1]) / (x[k] - x[k-1])) * (q - x[k-1]) + y[k-1], every operation rounded on its own
 *     (no fma): scipy's interp1d(kind="linear", fill_value="extrapolate") bit for bit.  The end segments extrapolate; a NaN
 *     value makes the two segments it belongs to NaN.
 *   mode 1, nearest: y[k-1] when ping - t_ext[k-1] <= t_ext[k] - ping in int64 (ties to the earlier sample), else y[k];
 *     a ping outside the track takes the end sample.
 * A NaT ping gives NaN in both modes.  EPA_EINVAL: N < 2, V < 1, P < 1, a NULL array, a mode other than 0 or 1. */
int epa_align_to_ping_time(const int64_t* t_ext, int N, const double* y, int V, const int64_t* ping_time, int P, int mode,
                           double* out, epa_stream_t stream);

/* ---- qc.exist_reversed_time / coerce_increasing_time: a time coordinate that steps backwards, found and repaired ---------
 * (qc/api.py:12-85).  t [N] int64 ticks of a datetime64 coordinate in any unit, INT64_MIN = NaT; all arrays on the device;
 * all arithmetic is int64 and wraps like NumPy's, so the results are exact whatever order the wavefronts run in.
 * d[i] = t[i+1] - t[i], i = 0 .. N-2; difference i is a REVERSAL when d[i] < 0 and neither t[i] nor t[i+1] is NaT. */
#define EPA_QC_FACTS 4         /* int64 words of the facts */
#define EPA_QC_FIRST 0         /*   the smallest reversal index, -1 without a reversal */
#define EPA_QC_COUNT 1         /*   the number of reversals */
#define EPA_QC_NAT 2           /*   the number of NaT among the N times */
#define EPA_QC_SLOTS 3         /*   entries written to the list (EPA_QC_COUNT with a list, else 0) */
#define EPA_QC_MAX_WIN 1024    /* the longest median window (it lives in LDS) */
#define EPA_QC_MEDIAN_WAVES 1024 /* wavefronts of an epa_reversal_medians launch, whatever the number of reversals */
#define EPA_QC_SCAN_TILE 1024  /* differences per workgroup of epa_time_rebuild */

/* facts [EPA_QC_FACTS] int64 out (initialised here); list [N-1] out or NULL: the reversal indices, in no particular
 * order.  One launch, one thread per time; with list NULL this is all of exist_reversed_time (facts[EPA_QC_COUNT] != 0).
 * EPA_EINVAL: N < 1, t or facts NULL. */
int epa_time_reversals(const int64_t* t, long long N, int64_t* facts, long long* list, epa_stream_t stream);

/* sub[ni] = the median of the original differences d[max(0, ni - win_len) .. ni) for every listed reversal ni (facts and
 * list as epa_time_reversals left them; the count is read on the device: the launch is the same for any count).  The
 * differences are recomputed from t, so a reversal inside another one's window enters that median as it is.  An even
 * number of values gives the wrapping sum of the two middle ones divided by 2, truncated toward zero (np.median of
 * timedelta64: [3, 8] -> 5, [-3, -8] -> -5, [-3, 8] -> 2, [-8, 3] -> -2).  sub [N-1] int64: only the reversal positions
 * are written, the rest keeps whatever it held; ni = 0 (an empty window) gets INT64_MIN (NaT).  t must hold no NaT
 * (facts[EPA_QC_NAT] == 0): a NaT takes part as the integer it is.
 * EPA_EINVAL: N < 2, win_len outside 1 .. EPA_QC_MAX_WIN, a NULL array. */
int epa_reversal_medians(const int64_t* t, long long N, int win_len, const int64_t* facts, const long long* list,
                         int64_t* sub, epa_stream_t stream);

/* out [N] = the repaired times: with f = facts[EPA_QC_FIRST], out[j] = t[j] for j <= f and
 * out[i+1] = t[f] + sum of d'[f .. i] for i >= f, where d'[i] = sub[i] at a reversal and d[i] elsewhere; without a
 * reversal out = t.  Three launches on the stream -- the sum of every tile of EPA_QC_SCAN_TILE differences, one workgroup
 * that turns the tile sums into carries, the tiles again with their carries -- so no workgroup waits for another one.
 * tile_workspace: int64 [ceil((N-1) / EPA_QC_SCAN_TILE)], scratch.  out must not be t; t without NaT, as above.
 * EPA_EINVAL: N < 2, a NULL array, out == t. */
int epa_time_rebuild(const int64_t* t, long long N, const int64_t* facts, const int64_t* sub, int64_t* tile_workspace,
                     int64_t* out, epa_stream_t stream);

/* ---- combine_echodata: the (channel, ping, range_sample[, beam]) cubes of many files joined along ping into one volume ----
 * (echodata/combine.py:807-817, xr.concat with its outer join on range_sample).  One launch, whatever the number of files:
 * every source byte is read once and every output byte written once.
 *   out[c][first_i + p][w] = src_i[chan[i * C + c]][p][w]   for w < W_i,   NaN for W_i <= w < W_out
 * NaN is NumPy's np.nan bit for bit: 0x7FC00000 (f32), 0x7FF8000000000000 (f64). */
typedef struct epa_concat_seg {
  const void* base; /* the file's variable [C_i][P_i][W_i], C-contiguous, on the device */
  long long P;      /* its pings, >= 1 */
  long long W;      /* its row width in ELEMENTS (range_sample, or range_sample * beam), 1 .. W_out */
  long long first;  /* the output ping of its first ping: the sum of the P before it */
  long long C;      /* its channels (the bound of its chan entries and of the overlap check; the kernel does not read it) */
} epa_concat_seg;
enum epa_concat_type { EPA_CT_I8 = 0, EPA_CT_I16, EPA_CT_I32, EPA_CT_I64, EPA_CT_F32, EPA_CT_F64, EPA_CT_COUNT };
/* segs [nseg] and chan [nseg][C] (output channel -> source channel of that file) on the device; segs_host / chan_host
 * the same two tables on the host, which the checks below read -- the caller vouches for the pairs being equal.
 * src_type == out_type: a bitwise copy of 1-, 2-, 4- or 8-byte elements (NaN payloads, integer planes and any other type of
 * that size pass through untouched); converting: I8 -> F32, I16 -> F32, I32 -> F64, I64 -> F64 (round to nearest even).
 * out [C][sum P_i][W_out] of out_type.  A wavefront owns whole output rows and streams them in 16-byte chunks aligned in
 * the output; no access assumes more than element alignment of a source row.
 * EPA_EINVAL (nothing is launched): a NULL array; nseg, C or W_out < 1; P_i < 1; W_i outside 1 .. W_out; first_i not the sum
 * of the P before it; a chan entry outside 0 .. C_i-1; a type pair that is not served; W_i < W_out with an integer out_type
 * (a pad needs NaN); out overlapping a source. */
int epa_concat_rows(const epa_concat_seg* segs_host, const epa_concat_seg* segs, const int* chan_host, const int* chan,
                    int nseg, int C, long long W_out, int src_type, int out_type, void* out, epa_stream_t stream);

/* ---- convert.open_raw (EK60): a Simrad .raw file unpacked where it lies ----------------------------------------------
 * (convert/utils/ek_raw_io.py:242-349, ek_raw_parsers.py:1676-1714, parse_base.py:294-302,686-730, set_groups_ek60.py:646-704)
 * A .raw file is a sequence of [int32 size][body of size bytes][int32 size], little endian; every body starts with
 * char type[4]; uint32 low_date; uint32 high_date.  One record per datagram: */
typedef struct epa_raw_record {
  int64_t offset;     /* byte offset of the BODY (behind the leading size field) */
  int32_t size;       /* its size in bytes, >= 16 */
  uint32_t type;      /* the four type characters as one little-endian word ('R' | 'A' << 8 | 'W' << 16 | '0' << 24) */
  uint32_t low_date;  /* NT time: 100-ns intervals since 1601-01-01, low and high half */
  uint32_t high_date;
  uint32_t flags;     /* EPA_RAW_ZERO_TIME */
  uint32_t reserved;  /* 0 */
} epa_raw_record;
#define EPA_RAW_ZERO_TIME 1u /* the time stamp is (0, 0): the caller skips the datagram (ek_raw_io.py:267-275) */

/* The framing walk, on the HOST: no GPU call, no allocation.  Count, then fill: records_out [capacity] (NULL with
 * capacity 0) receives the first min(capacity, *n_records) records, *n_records is the number of complete datagrams in any
 * case.  A body or trailer that runs past n_bytes (a file cut while recording) ends the walk: *n_bytes_consumed is the
 * offset behind the last complete datagram (== n_bytes for a whole file), the datagrams before it stand.  No byte outside
 * [0, n_bytes) is read, whatever the bytes are.
 * EPA_EINVAL, with the byte offset in the message and *n_records / *n_bytes_consumed describing the datagrams in front:
 * a size below 16; a trailing size that differs from the leading one (the reference searches for the next datagram there,
 * ek_raw_io.py:325-337; this walk does not resynchronise).  Also a NULL argument or a negative length. */
int epa_raw_index(const uint8_t* bytes_host, long long n_bytes, epa_raw_record* records_out, long long capacity,
                  long long* n_records, long long* n_bytes_consumed);

/* power [C][P][S] f32 = float32(int16 at bytes[off_p + 2 s]) * float32(10 log10(2) / 256) for s < count, NaN behind it;
 * athwartship / alongship [C][P][S] = the int8 at bytes[off_a + 2 s] / bytes[off_a + 2 s + 1].  One launch; every
 * output element is written exactly once, nothing is pre-filled.
 * bytes: the file as it is on disk, on the device, n_bytes long in an allocation of n_alloc bytes -- 16-byte aligned,
 * n_alloc a multiple of 16 -- because the samples are read as the aligned dwords that hold them (a block starts at any
 * byte offset).  table [C * P][3] int64, row (c, p): off_p, off_a (-1: no such block, the row is NaN) and count;
 * table_host the same on the host, which the checks read -- the caller vouches for the pair being equal.
 * angle_type EPA_RAW_ANGLE_NONE: the planes are not touched (may be NULL); _I8: int8 planes, every row must have an angle
 * block of exactly S samples; _F32: float32 planes, NaN behind count and in rows without a block.  NaN is 0x7FC00000.
 * EPA_EINVAL (nothing is launched): a NULL array; C, P or S < 1; a count outside 0 .. S; a block that leaves
 * [0, n_bytes); a buffer or plane that is not 16-byte aligned; n_alloc not a multiple of 16 or below n_bytes; _I8 with a
 * short or missing row. */
enum epa_raw_angle { EPA_RAW_ANGLE_NONE = 0, EPA_RAW_ANGLE_I8 = 1, EPA_RAW_ANGLE_F32 = 2 };
int epa_raw0_unpack(const uint8_t* bytes, long long n_bytes, long long n_alloc, const int64_t* table_host,
                    const int64_t* table, int C, long long P, long long S, int angle_type, float* power,
                    void* athwartship, void* alongship, epa_stream_t stream);

/* convert.open_raw_ek80: the complex sample blocks of the RAW3 datagrams of an EK80 file (ek_raw_parsers.py:1745-1769,
 * parse_base.py:304-314).  backscatter_r / backscatter_i [C][P][S][B] f32: for row (c, p), sample s < count and sector
 * b < B_row, backscatter_r is the float32 at bytes[off + 8 (s B_row + b)] and backscatter_i the float32 4 bytes further on,
 * both bit copies -- except that an imaginary part equal to 0.0 (-0.0 included) becomes NaN, which is the reference's rule
 * (its NaN padding is a complex number whose imaginary part is 0, so it tests for 0).  Everything else is NaN (0x7FC00000):
 * samples behind count, sectors >= B_row, rows with off == -1.  One launch; every output element is written exactly once,
 * nothing is pre-filled.
 * bytes / n_bytes / n_alloc: the file as for epa_raw0_unpack.  table [C * P][3] int64, row (c, p): off (-1: no block),
 * count and B_row; table_host the same on the host, which the checks read.
 * EPA_EINVAL (nothing is launched): a NULL array; C, P or S < 1; B outside 1 .. 8; a count outside 0 .. S; a B_row outside
 * 0 .. B; a block (8 count B_row bytes) that leaves [0, n_bytes); a buffer or plane that is not 16-byte aligned; n_alloc not
 * a multiple of 16 or below n_bytes. */
int epa_raw3_unpack(const uint8_t* bytes, long long n_bytes, long long n_alloc, const int64_t* table_host,
                    const int64_t* table, int C, long long P, long long S, int B, float* backscatter_r, float* backscatter_i,
                    epa_stream_t stream);

/* Positions from the NMEA sentences of the file's NME0 datagrams, parsed where they lie in HBM (set_groups_base.py:180-239,
 * which calls pynmea2.parse once per sentence on the host; the rules are restated in echopype_amd/convert/parse_nmea.py).
 * bytes / n_bytes / n_alloc: the file as for epa_raw0_unpack.  table [n][2] int64: byte offset and length of the text of
 * each selected sentence, NULs stripped; table_host the same on the host, which the checks read.  Per sentence:
 * lat, lon [n] f64 in signed degrees and code [n], a status byte:
 *   0                       both values written
 *   EPA_NMEA_INVALID        the checksum does not hold: NaN, NaN
 *   EPA_NMEA_LAT_FAILED     bit: the latitude field is not DDMM.MMM: NaN        (the type bits are set as well)
 *   EPA_NMEA_LON_FAILED     bit: the longitude field is not DDDMM.MMM: NaN
 *   EPA_NMEA_UNDECIDED      not decided here, NaN, NaN: the caller applies the host rules (parse_nmea.parse_sentence)
 * and, unless the code is EPA_NMEA_INVALID or EPA_NMEA_UNDECIDED, the sentence type (enum epa_nmea_type) in the bits
 * EPA_NMEA_TYPE_MASK: (code & EPA_NMEA_TYPE_MASK) >> EPA_NMEA_TYPE_SHIFT.  NaN is 0x7FF8000000000000.
 * The kernel decides only the PLAIN FORM and never guesses: byte 0 is '$'; bytes 1-5 are ASCII letters or digits, byte 1
 * not 'P' / 'p', bytes 3-5 "GGA", "GLL" or "RMC"; byte 6 is ','; every byte is in 0x20..0x7E apart from a trailing run of
 * CR / LF / space / tab; at most one '*', then exactly two hex digits (either case) and only that run behind them; without
 * a '*', the four coordinate fields end at a comma or the run is empty; a latitude / longitude field has at most 64 bytes,
 * and where it has the form digits "." digits, its degrees and the digits of its minutes are integers below 10^15 with at
 * most 15 decimals -- under which the result equals Python's float(d) + float(m) / 60 bit for bit.
 * n == 0 launches nothing.  EPA_EINVAL (nothing is launched): a NULL array with n > 0; a negative n; a row that leaves
 * [0, n_bytes); n_alloc not a multiple of 16 or below n_bytes.  No reference counterpart as a function. */
enum epa_nmea_type { EPA_NMEA_GGA = 0, EPA_NMEA_GLL = 1, EPA_NMEA_RMC = 2 };
#define EPA_NMEA_INVALID 1
#define EPA_NMEA_LAT_FAILED 2
#define EPA_NMEA_LON_FAILED 4
#define EPA_NMEA_TYPE_SHIFT 3
#define EPA_NMEA_TYPE_MASK 0x18
#define EPA_NMEA_UNDECIDED 64
int epa_nmea_positions(const uint8_t* bytes, long long n_bytes, long long n_alloc, const int64_t* table_host,
                       const int64_t* table, long long n, double* lat, double* lon, uint8_t* code, epa_stream_t stream);

/* ---- single targets, split beam: targets.detect_single_targets (targets/api.py) -------------------------------------
 * The echoes of individual fish along every (channel, ping) row, by this project's restatement of the Echoview
 * single-target detection (split beam); targets/api.py states the six rules, and the two entries apply them alike.
 * ts, along, athw: [C*P*S] of dtype F32 / F64 (converted to f64 exactly; all arithmetic is f64); the sample (c, p, s) of
 * the range, of the same dtype, is range[c * range_stride_c + p * range_stride_p + s] (element strides >= 0; 0 shares a
 * row).  prm f64 [EPA_SINGLE_TARGET_PARAMS][C*P]: samples per pulse, beamwidth alongship / athwartship, angle offset
 * alongship / athwartship of every row.  limits: HOST f64 [7] = TS_threshold, pldl, min_norm_pulse_length,
 * max_norm_pulse_length, max_beam_compensation, max_std_alongship, max_std_athwartship.
 * A row belongs to one workgroup, which walks it in tiles of EPA_SINGLE_TARGET_TILE samples.
 *
 * count: n_targets i32 [C*P] is written completely; n_candidates u64 [C] and n_rejected u64 [C*4] (rules 1 .. 4), zeroed
 * by the caller, are added to.  C*P == 0 launches nothing; S == 0 zeroes n_targets. */
#define EPA_SINGLE_TARGET_TILE 1024
#define EPA_SINGLE_TARGET_PARAMS 5
#define EPA_SINGLE_TARGET_ICOLS 5 /* channel_index, ping_index, range_sample (the peak), sample_first, sample_last */
#define EPA_SINGLE_TARGET_FCOLS 9 /* TS_uncomp, TS_comp, beam_compensation, target_range, angle_alongship,
                                   * angle_athwartship, std_angle_alongship, std_angle_athwartship,
                                   * normalized_pulse_length */
int epa_single_target_count(const void* ts, const void* along, const void* athw, const void* range, int dtype,
                            long long C, long long P, long long S, long long range_stride_c, long long range_stride_p,
                            const double* prm, const double* limits, int* n_targets, unsigned long long* n_candidates,
                            unsigned long long* n_rejected, epa_stream_t stream);
/* emit: the same inputs, n_targets as count left it, offsets i64 [C*P] its exclusive scan over (channel, ping) and N its
 * sum.  icols i32 [EPA_SINGLE_TARGET_ICOLS][N] and fcols f64 [EPA_SINGLE_TARGET_FCOLS][N] take one column entry per
 * target, ordered by (channel, ping, sample); a row writes inside [offsets, offsets + n_targets) and below N only.
 * Rows whose n_targets is 0 are not read.  N == 0 launches nothing. */
int epa_single_target_emit(const void* ts, const void* along, const void* athw, const void* range, int dtype,
                           long long C, long long P, long long S, long long range_stride_c, long long range_stride_p,
                           const double* prm, const double* limits, const int* n_targets, const long long* offsets,
                           long long N, int* icols, double* fcols, epa_stream_t stream);

/* ---- target tracking: targets.track_targets (targets/track.py) -------------------------------------------------------
 * The single targets of one fish over consecutive pings grouped into tracks by gated nearest-neighbour linking in a fixed
 * number of propose / accept rounds; targets/track.py states the five rules.  The table has n rows ordered by
 * (channel_index, ping_index), i32 columns; range, along, athw, ts f64 [n].  All arithmetic is f64.  Every entry is
 * memory-safe on any content of the index columns; what it computes for a table that prepare finds bad is unspecified.
 * params: HOST f64 [EPA_TRACK_PARAMS] = gate_alongship, gate_athwartship, gate_range, max_ping_gap,
 * missed_ping_expansion, weight_alongship, weight_athwartship, weight_range, weight_TS, weight_ping_gap,
 * max_TS_difference (0: no TS gate).  n == 0 launches nothing, except in prepare.
 *
 * prepare: seg i32 [C*P + 1]: the first row whose (channel, ping) is not below the segment's; xyz f64 [3][n] (rule 1);
 * succ, pred i32 [n] set to -1; bad i32 [1], zeroed by the caller, set to 1 if a row's indices are outside [0, C) x [0, P)
 * or the rows are not ordered. */
#define EPA_TRACK_TILE 128   /* rows of a run a workgroup of propose / accept stages in LDS at a time */
#define EPA_TRACK_PARAMS 11
#define EPA_TRACK_ICOLS 6    /* channel_index, n_targets, ping_first, ping_last, target_first, target_last */
#define EPA_TRACK_FCOLS 13   /* TS_mean, TS_max, range_mean, x_first, y_first, z_first, x_last, y_last, z_last,
                              * path_length, displacement, tortuosity, delta_range */
int epa_track_prepare(const int* channel_index, const int* ping_index, const double* range, const double* along,
                      const double* athw, long long n, long long C, long long P, int* seg, double* xyz, int* succ,
                      int* pred, int* bad, epa_stream_t stream);
/* propose: prop i32 [n] of every row: the gated row without a predecessor that minimises (cost, row) among the rows of
 * the next 1 + max_ping_gap pings of its channel, -1 if there is none, the row has a successor or holds a NaN. */
int epa_track_propose(const int* channel_index, const int* ping_index, const double* xyz, const double* ts, long long n,
                      long long C, long long P, const int* seg, const double* params, const int* succ, const int* pred,
                      int* prop, epa_stream_t stream);
/* accept: every row without a predecessor takes, among the rows whose prop names it, the one minimising (cost, row):
 * pred of the row and succ of the taken row are set. */
int epa_track_accept(const int* channel_index, const int* ping_index, const double* xyz, const double* ts, long long n,
                     long long C, long long P, const int* seg, const double* params, const int* prop, int* succ,
                     int* pred, epa_stream_t stream);
/* roots: `passes` (1 .. 32) passes of pointer doubling over pred, one launch each; a chain of up to 2**passes rows is
 * resolved.  The pairs (ptr_a, rank_a) and (ptr_b, rank_b), i32 [n] each, are written in turn, a first: the last pass
 * leaves the first row of every row's chain and the row's position in it in a if passes is odd, in b if it is even. */
int epa_track_roots(const int* pred, long long n, int passes, int* ptr_a, int* rank_a, int* ptr_b, int* rank_b,
                    epa_stream_t stream);
/* chains: flag_len i32 [2][n], zeroed by the caller: [0][r] = 1 and [1][r] = the number of rows, at the first row r of
 * every chain that is a track (rule 5; a row holding a NaN is none). */
int epa_track_chains(const int* ping_index, const double* xyz, const double* ts, const int* succ, const int* root,
                     const int* rank, long long n, int min_targets, int min_pings, int* flag_len, epa_stream_t stream);
/* table: scans i64 [2][n] the inclusive scans of flag_len's two rows, T >= 1 and M their totals.  track_id i32 [n];
 * order i32 [M]: the rows of track 1 in chain order, then those of track 2, ...; start i32 [T]: where a track begins in
 * order; icols i32 [EPA_TRACK_ICOLS][T], fcols f64 [EPA_TRACK_FCOLS][T].  One wave per track: lane l adds the rows
 * l, l + 64, ... of the track in chain order, and the 64 partial sums are added in a fixed tree. */
int epa_track_table(const int* channel_index, const int* ping_index, const double* range, const double* ts,
                    const double* xyz, const int* root, const int* rank, const int* flag_len, const long long* scans,
                    long long n, long long T, long long M, int* track_id, int* order, int* start, int* icols,
                    double* fcols, epa_stream_t stream);

/* ---- target strength spectra: targets.target_spectra (targets/spectra.py) ---------------------------------------------
 * TS(f) of every row of a single-target table from the complex sector samples of EK80 FM pings, by this project's
 * restatement of Andersen et al. (2021); targets/spectra.py states the eight rules.  All arithmetic is f64.
 * re, im: [C*P*S*B] of in_dtype F32 / F64, the sectors of a sample adjacent.  replica: interleaved (re, im) f32 of
 * replica_len complex elements; replica r is [replica_off[r], replica_off[r+1]) (i32 [n_replicas + 1]) and may hold 1 ..
 * max_taps <= EPA_TARGET_SPECTRA_MAX_TAPS taps; ping (c, p) uses replica replica_id[c*P + p] (i32, optional; NULL: replica
 * c).  rep_dt f64 [n_replicas]: the sample interval of the pings of a replica.  fparams f64
 * [n_replicas][EPA_TARGET_SPECTRA_FPARAMS][F]: per replica and frequency f (Hz), absorption, gain, z_et, beamwidth
 * alongship / athwartship, angle offset alongship / athwartship.  pparams f64 [EPA_TARGET_SPECTRA_PPARAMS][C*P]:
 * transmit power, sound speed, z_er.  chan_map i32 [n_map]: the channel of the cubes a table channel stands for.
 * The table: t_channel, t_ping, t_sample i32 [N], t_range, t_along, t_athw f64 [N].  A row whose indices, replica index or
 * replica offsets lie outside what the arrays hold gives NaN and n_window 0; no byte outside the arrays is read, whatever
 * the table holds.
 * table: scratch, f64 [n_replicas][EPA_TARGET_SPECTRA_TABLE_ROWS][F], sized by
 * epa_scratch_bytes("target_spectra.table", n_replicas, F).  ts_out, ts_uncomp_out: [N][F] of out_dtype; n_window i32 [N]:
 * the samples of the window inside the ping with a valid sector.  N == 0 launches nothing. */
#define EPA_TARGET_SPECTRA_MAX_HALF_WINDOW 127
#define EPA_TARGET_SPECTRA_MAX_FREQ 1024
#define EPA_TARGET_SPECTRA_MAX_TAPS 2048
#define EPA_TARGET_SPECTRA_FPARAMS 8
#define EPA_TARGET_SPECTRA_PPARAMS 3
#define EPA_TARGET_SPECTRA_TABLE_ROWS 3
int epa_target_spectra(const void* re, const void* im, int in_dtype, long long C, long long P, long long S, int B,
                       const float* replica, const int32_t* replica_off, const int32_t* replica_id, int n_replicas,
                       long long replica_len, int max_taps, const double* rep_dt, const double* fparams, int F,
                       int half_window, const double* pparams, const int32_t* chan_map, int n_map,
                       const int32_t* t_channel, const int32_t* t_ping, const int32_t* t_sample, const double* t_range,
                       const double* t_along, const double* t_athw, long long N, double* table, void* ts_out,
                       void* ts_uncomp_out, int out_dtype, int32_t* n_window, epa_stream_t stream);

/* ---- volume backscattering spectra: calibrate.compute_Sv_spectrum (calibrate/sv_spectrum.py) --------------------------
 * Sv(f) of range cells (a short-time Fourier analysis of the pulse-compressed pings) from the complex sector samples of
 * EK80 FM pings, by this project's restatement of Andersen et al. (2021); calibrate/sv_spectrum.py states the ten rules.
 * All arithmetic is f64.  re, im, replica, replica_off, replica_id, rep_dt: as for epa_target_spectra, with max_taps <=
 * EPA_SV_SPECTRUM_MAX_TAPS.  fparams f64 [n_replicas][EPA_SV_SPECTRUM_FPARAMS][F]: per replica and frequency f (Hz),
 * absorption, gain, z_et, equivalent beam angle (dB).  pparams f64 [EPA_SV_SPECTRUM_PPARAMS][C*P]: transmit power, sound
 * speed, z_er, sample interval.  window f64 [window_samples]: the normalised window w~.  Cell m of a ping holds the
 * samples m * step_samples .. m * step_samples + window_samples - 1; M = (S - window_samples) / step_samples + 1 cells.
 * table: scratch, f64 [n_replicas][EPA_SV_SPECTRUM_TABLE_ROWS][F], sized by epa_scratch_bytes("sv_spectrum.table",
 * n_replicas, F).  sv_out [C*P][M][F] of out_dtype; range_out f64 [C*P][M]: the cell centres, written for every cell.  A
 * ping whose replica index or replica offsets lie outside what the arrays hold gives NaN cells; no byte outside the arrays
 * is read.  A workgroup serves a tile of consecutive cells of one ping: as many as keep its LDS within a third of a CU's
 * 160 KiB, at most EPA_SV_SPECTRUM_MAX_TILE_CELLS, evenly filled (epa_sv_spectrum_plan tells); one cell of the largest
 * window with the largest replica takes 107 KiB, so every combination within the limits is served. */
#define EPA_SV_SPECTRUM_MAX_WINDOW 1024
#define EPA_SV_SPECTRUM_MAX_FREQ 1024
#define EPA_SV_SPECTRUM_MAX_TAPS 2048
#define EPA_SV_SPECTRUM_MAX_TILE_CELLS 128
#define EPA_SV_SPECTRUM_FPARAMS 5
#define EPA_SV_SPECTRUM_PPARAMS 4
#define EPA_SV_SPECTRUM_TABLE_ROWS 3
int epa_sv_spectrum(const void* re, const void* im, int in_dtype, long long C, long long P, long long S, int B,
                    const float* replica, const int32_t* replica_off, const int32_t* replica_id, int n_replicas,
                    long long replica_len, int max_taps, const double* rep_dt, const double* fparams, int F,
                    const double* pparams, const double* window, int window_samples, long long step_samples, long long M,
                    double* table, void* sv_out, int out_dtype, double* range_out, epa_stream_t stream);
/* the tile epa_sv_spectrum takes for M cells per ping: cells of a tile, tiles of a ping, bytes of LDS of a workgroup */
int epa_sv_spectrum_plan(int max_taps, int window_samples, long long step_samples, long long M, int* tile_cells, int* tiles,
                         size_t* lds_bytes_out);

#ifdef __cplusplus
}
#endif
#endif /* ECHOPYPE_AMD_H */
