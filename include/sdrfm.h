/*
 * sdrfm.h — C-ABI of the MI355X-native IQ -> FM-audio path ("sdrfm").
 *
 * This is the drop-in boundary for the consumer hook that the reference firmware leaves empty:
 *   - the bulk-IN FSM fills `CommItf.buff` / `CommItf.buffSize` with interleaved uint8 I/Q
 *     (Middlewares/ST/STM32_USB_Host_Library/Class/RTLSDR/Inc/usbh_rtlsdr.h:165-173) and then does
 *     nothing in RTLSDR_XFER_COMPLETE (.../RTLSDR/Src/usbh_rtlsdr.c:1094-1097); the application-side
 *     poll of `xferState` is commented out (src/main.c:76-79).
 *   - sdrfm_process() is what either hook calls with (buff, USBH_LL_GetLastXferSize()) — see INTEGRATION.md.
 *
 * Conventions follow the reference's class-driver layer:
 *   - return value 0 == OK, same numeric values as USBH_StatusTypeDef for the first five codes
 *     (Middlewares/ST/STM32_USB_Host_Library/Core/Inc/usbh_def.h:303-311);
 *   - errors are returned, never thrown/aborted; a handle is not thread-safe (single superloop model,
 *     src/main.c:72-80); independent handles may be used concurrently;
 *   - the callee is finished with `iq` when the call returns (the reference re-arms the same buffer
 *     immediately, usbh_rtlsdr.c:1068-1077), except in SDRFM_F_DEVICE_PTRS mode (see below).
 *
 * Arithmetic (build-defined; the reference holds no DSP code — see DESIGN.md "Frozen spec"):
 *   x[n]  = ((float)I_n - 127.5f) + j((float)Q_n - 127.5f)
 *   y[m]  = sum_{k} h[k] * x[(m+1)*D - 1 - k]        x[n<0] = 0, fp32 FMA chain, oldest sample first
 *   d[m]  = atan2f(Im(y[m]*conj(y[m-1])), Re(...))   y[-1] = 0, d = 0 when both parts are exactly 0
 *   a[j]  = sum_{k} g[k] * d[(j+1)*Da - 1 - k]       d[m<0] = 0, fp32 FMA chain, oldest sample first
 * All state (FIR history, y[m-1], d history, decimator phases) persists across calls; chunk lengths need
 * not be multiples of D.
 * Which kernel evaluates this is chosen per call (sdrfm_kernel_name() tells): kernels that are bit-identical to the definition, or — for
 * machine-filling calls of whole audio periods with low-pass taps, unless the handle has SDRFM_CFG_BIT_EXACT — the matrix-pipe kernel
 * ("fast-q").  That one evaluates y exactly in integers from taps rounded to 24-bit fixed point, which is within ~1e-4 (absolute) of the
 * definition's fp32 chain, i.e. within 1e-6 of the definition's AUDIO wherever the phase of y[m] conj(y[m-1]) is well conditioned; where
 * it is not — |y| small (a deep fade: noise-only input gets there, a carrier does not) or d within reach of +-pi (the branch cut) — its
 * conditioning guard recomputes the affected d's with the definition's own chain from the raw bytes, so that they are the bit-identical
 * kernels' d's.  How far "within reach" goes rests on a bound E on |y_fast-q - y_definition|.  By default it is STATISTICAL:
 * E = 1.25 sqrt(T) 127.5 sum|h| 2^-24 (csrc/qtaps.c; 28 standard deviations of what uniform random bytes produce, 9 of a full-scale
 * carrier's).  So "fast-q" within the 1e-5 tolerance (|a - b| <= 1e-5 max(|b|, 1), for audio taps of about unit absolute sum) is by
 * default a MEASURED statement, not a proven one: no violation, worst 9.8e-7, in the device soaks over every input class — uniform random
 * bytes, constant and counter bytes, carriers, and the classes built to probe the bound (strong out-of-band carriers at one to three guard
 * radii, 2 - 8 LSB carriers, periodic byte patterns: tools/q_classes.py, profiles/r06_fuzz_q.txt).  What can be had beyond that, and its price:
 *   SDRFM_CFG_GUARD_WORST_CASE  the radius from the PROVEN worst case of E (every rounding the same way: 6.9 x at 64 taps).  Proves every
 *                               unrepaired d within 5e-6 / max|g| + 1.1e-6 of the definition's; the AUDIO bound that follows for arbitrary bytes is
 *                               sum|g| times that (4.6e-5 for the BASELINE audio taps: all 32 d's of a window at the radius, errors aligned), 1e-5
 *                               when at most one pair of a window is marginal.  Costs a carrier nothing measurable (profiles/r06_guard_worst_case.txt).
 *   SDRFM_CFG_BIT_EXACT         the guarantee: the bit-identical kernels only — 0.42 of the HBM roofline against 0.60 / 0.72 (bench.py: bit_exact_kernel).
 *                               A worst-case radius that PROVED 1e-5 for arbitrary bytes would be 2 sum|g| E_wc / 8e-6 = 180 of 127.5 full scale:
 *                               every output repaired, i.e. this flag at a higher price.
 * A stream whose windows of calls are mostly repair work (noise only) is moved to the bit-identical kernels for a while, per stream
 * (DESIGN.md 4.Q "routing").  Which kernel serves a stream at which call is a function of the bytes and the sequence of calls alone (round 6): a
 * window of 16 calls takes effect at the first call of the window four windows later, never "when noticed" — two runs of one capture give
 * the same bits.  Every choice is within the tolerance.
 *
 * There is NO CPU fallback in this library: every entry point that computes runs hand-written HIP kernels
 * on a gfx950 device and fails with SDRFM_NO_DEVICE when none is usable.
 */
#ifndef SDRFM_H
#define SDRFM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDRFM_ABI_VERSION 1u

/* status codes: first five numerically equal USBH_OK..USBH_UNRECOVERED_ERROR (usbh_def.h:303-311) */
enum {
  SDRFM_OK = 0,
  SDRFM_BUSY = 1,
  SDRFM_FAIL = 2,
  SDRFM_NOT_SUPPORTED = 3,
  SDRFM_UNRECOVERED_ERROR = 4,
  /* extensions */
  SDRFM_EINVAL = 16,      /* NULL pointer, zero sizes, bad struct_size, non-finite taps            */
  SDRFM_EODD = 17,        /* nbytes not a multiple of 2 (half an I/Q pair)                          */
  SDRFM_ECAPACITY = 18,   /* audio buffer / stride too small, or nbytes > max_bytes_per_call        */
  SDRFM_NO_DEVICE = 19,   /* no usable gfx950 HIP device, or HIP runtime error at create            */
  SDRFM_ENOMEM = 20
};

#define SDRFM_MAX_TAPS 256u       /* limit for fir_taps and audio_taps */
#define SDRFM_MAX_DECIM 64u

/* flags for sdrfm_config.flags */
#define SDRFM_CFG_FORCE_GENERIC 1u  /* never select a (T,D)-specialised kernel: run the generic kernel (tests) */
#define SDRFM_CFG_BIT_EXACT     4u  /* only kernels whose audio is bit-identical to the fp32 fmaf-chain definition above (the generic kernel's):
                                       never the matrix-pipe kernel ("fast-q"), whose audio is within the tolerance of that definition for any
                                       input (see above) but not bit-identical to it.  Without the flag "fast-q" serves low-pass channel
                                       filters of up to 64 taps (sum|h| <= 2 |sum h|: a performance rule, not a correctness condition) at
                                       D = 10, 32 audio taps / 5 (and at D = 8 / 8, D = 16 / 5) — but for the streams that turn out to be
                                       noise only, which the bit-identical kernels serve faster: those are routed to them per stream;
                                       every other configuration runs the bit-identical kernels anyway */
#define SDRFM_CFG_NO_ZEROCOPY   2u  /* URB-sized host calls use the staged H2D/D2H path instead of mapped host memory (tests) */
#define SDRFM_CFG_GUARD_WORST_CASE 8u  /* "fast-q": the conditioning guard's radius from the PROVEN worst case of |y_fast-q - y_definition| — every rounding of
                                       the definition's chain and of the recombination falling the same way at the largest partial sum, every tap's
                                       quantisation error against a full-scale byte: (T + 4) 127.5 sum|h| 2^-24 + 64 T q (csrc/qtaps.c) — instead of the
                                       statistical bound; 6.9 times the radius at 64 taps (|y| < 32 of 127.5 is recomputed by the definition's chain).
                                       With it every unrepaired discriminator output is PROVABLY within 5e-6 / max|g| + 1.1e-6 of the definition's;
                                       a carrier above a quarter of full scale never meets the guard and costs the same (profiles/r06_guard_worst_case.txt),
                                       weaker streams are repaired more often and then routed to the bit-identical kernels.  See the note above. */

/* flags for sdrfm_process_batch */
#define SDRFM_F_DEVICE_PTRS 1u    /* iq and audio are device pointers on cfg.device; call is enqueued on the
                                     handle's stream and returns without synchronising; it does not wait for the device either while the
                                     caller is less than 48 calls ahead of it ("fast-q" handles: the per-stream statistics of a window of 16
                                     calls are read back on a side stream and take effect at a fixed call three windows after the window
                                     closed — a caller further ahead than that waits there for the read-back, which is what makes the kernel
                                     assignment a function of the bytes and the calls and not of timing (so a caller whose stream is held back by
                                     work it has not issued yet must not run that far ahead of it);
                                     tests/test_route_gpu.py test_calls_return_without_waiting_for_the_device).  The handle's own stream is
                                     created non-blocking: it does NOT order itself against the null stream or any
                                     other stream, so work that produces iq or touches audio elsewhere must be
                                     synchronised by the caller, or the caller's stream given via sdrfm_set_stream */

#define SDRFM_F_OVERLAP 2u        /* (with SDRFM_F_DEVICE_PTRS) the call may run on the device CONCURRENTLY with the previous
                                     call made with this flag: a call's start-up then hides under the previous call's tail (12 % more
                                     calls per second on BASELINE configs[2]).  The call is ordered behind what the handle's stream
                                     holds when it is made (so iq may be produced there), but the handle's stream does not wait for
                                     it: sdrfm_flush / sdrfm_synchronize / any call without the flag order the stream behind all
                                     overlapped calls.  The caller promises, until the call has completed: (a) the PREVIOUS call's
                                     iq buffer stays intact — the call warms its streams up from that buffer's last bytes instead of
                                     waiting for the previous call's state —, and (b) audio is not a buffer the previous overlapped
                                     call writes (two audio buffers taken in turn).  Same audio, bit for bit, as without the flag.
                                     Calls that the matrix-pipe kernel does not serve (see SDRFM_CFG_BIT_EXACT), and the first call
                                     after create / reset / a host-pointer call / a call the matrix-pipe kernel did not serve, run
                                     as if the flag were absent */

typedef struct sdrfm_config {
  uint32_t struct_size;           /* = sizeof(sdrfm_config) */
  uint32_t n_streams;             /* independent IQ streams processed per call (>= 1) */
  uint32_t fir_taps;              /* T  : channel low-pass taps, 1..SDRFM_MAX_TAPS */
  uint32_t fir_decim;             /* D  : 1..SDRFM_MAX_DECIM (2.4 MS/s / 10 = 240 kS/s, the rate the firmware
                                          programs: usbh_rtlsdr.c:898) */
  const float* fir_coeffs;        /* h[0..T), copied at create */
  uint32_t audio_taps;            /* Ta : audio low-pass taps, 1..SDRFM_MAX_TAPS */
  uint32_t audio_decim;           /* Da : 1..SDRFM_MAX_DECIM (240 kS/s / 5 = 48 kHz) */
  const float* audio_coeffs;      /* g[0..Ta), copied at create */
  uint32_t max_bytes_per_call;    /* per-stream upper bound for nbytes (sizes device staging); 0 = 1 MiB */
  int32_t  device;                /* HIP device ordinal */
  uint32_t flags;                 /* SDRFM_CFG_* */
} sdrfm_config;

typedef struct sdrfm sdrfm_t;

/* Create / destroy. The handle owns its device buffers, streaming state and output staging — it plays the role
 * of the class handle malloc'd in InterfaceInit and freed in InterfaceDeInit (usbh_rtlsdr.c:182-183,635-638). */
int  sdrfm_create(const sdrfm_config* cfg, sdrfm_t** out);
void sdrfm_destroy(sdrfm_t* h);

/* Zero all streaming state (as after create). */
int  sdrfm_reset(sdrfm_t* h);

/* Number of audio samples per stream that the NEXT process call with `nbytes` will produce (depends on the
 * decimator phases carried in the handle). */
int  sdrfm_audio_count(const sdrfm_t* h, uint32_t nbytes, uint32_t* n_audio);

/* Single-stream hand-off (handle must have n_streams == 1): host buffer in, host audio out, synchronous.
 *   iq      : interleaved uint8 I0 Q0 I1 Q1 ... exactly as the RTL2832 bulk pipe delivers it
 *             (RTLSDR_CommItfTypedef.buff, usbh_rtlsdr.h:165-173)
 *   nbytes  : valid bytes (USBH_LL_GetLastXferSize, usbh_conf.c:350-353); must be even; 0 is a no-op
 *   audio   : receives *n_audio floats (radians per 240 kS/s sample, low-passed, at 48 kHz)            */
int  sdrfm_process(sdrfm_t* h, const uint8_t* iq, uint32_t nbytes,
                   float* audio, uint32_t audio_cap, uint32_t* n_audio);

/* Batched hand-off: n_streams buffers of nbytes_per_stream bytes, stream s at iq + s*iq_stride (bytes);
 * audio for stream s at audio + s*audio_stride (floats). All streams advance by the same amount, so
 * *n_audio (per stream) is one number. With SDRFM_F_DEVICE_PTRS the buffers are device memory and the work is
 * only enqueued (use sdrfm_synchronize or the stream). */
int  sdrfm_process_batch(sdrfm_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes_per_stream,
                         float* audio, size_t audio_stride, uint32_t* n_audio, uint32_t flags);

/* Run on a caller-owned HIP stream (hipStream_t passed as void*; NULL = the handle's own stream). */
int  sdrfm_set_stream(sdrfm_t* h, void* hip_stream);
int  sdrfm_synchronize(sdrfm_t* h);
/* Order the handle's stream behind every call made with SDRFM_F_OVERLAP so far (enqueues two event waits; does not block the host). */
int  sdrfm_flush(sdrfm_t* h);
/* The same for every overlapped call but the most recent one: a consumer of call k-1's audio that runs on the handle's stream is put behind
 * call k-1 only, so call k keeps running beside it (and call k+1, ordered behind the consumer, may reuse call k-1's audio buffer). */
int  sdrfm_flush_previous(sdrfm_t* h);
/* The same ordering given to ANOTHER stream of the caller's (hipStream_t): `hip_stream` is put behind every overlapped call but the most recent one, and the
 * handle's own stream is left alone — so a consumer of call k-1's audio on a stream of its own (the device PCM sink, a copy engine) runs beside call k, and call
 * k+1 is ordered behind nothing but its own inputs: the consumer loop of INTEGRATION.md at the demodulator's own rate (23 us per BASELINE configs[2] call with the
 * device PCM sink as the consumer; a consumer on the handle's stream holds every second call back: 43 us).  The caller orders its reuse of an audio buffer against
 * that consumer itself (three audio buffers and an event).  Non-blocking. */
int  sdrfm_wait_previous(sdrfm_t* h, void* hip_stream);

/* Introspection used by bench/tests: the kernel variant that served the LAST call (before any call: the one the
 * configuration selects), e.g. "fast T64 D10 R4 Ta32 Da5" or "generic T7 D3 Ta5 Da4 NA64". */
const char* sdrfm_kernel_name(const sdrfm_t* h);
uint32_t    sdrfm_abi_version(void);
const char* sdrfm_strerror(int status);

/* ------------------------------------------------------------------------------------------------------------------
 * Streaming front-end adapter: a ring of n_buffers pinned host buffers of buffer_bytes each — the multi-buffer scheme the
 * reference declares but never uses (DEFAULT_BUF_NUMBER 15 x DEFAULT_BUF_LENGTH 16*32*512, usbh_rtlsdr.h:277-278).
 * Single-stream handles only.  submit() copies the just-filled USB buffer into the next free slot and enqueues
 * H2D -> kernel -> D2H without waiting (the caller's buffer may be re-armed at once); collect() returns finished audio in
 * submission order.  Both are non-blocking and answer SDRFM_BUSY (ring full / nothing ready), like the reference's FSM
 * steps answer USBH_BUSY; collect(wait != 0) blocks for the oldest slot.  Do not mix with sdrfm_process on the same handle
 * while slots are in flight.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct sdrfm_ring sdrfm_ring_t;
int  sdrfm_ring_create(sdrfm_t* h, uint32_t n_buffers, uint32_t buffer_bytes, sdrfm_ring_t** out);
void sdrfm_ring_destroy(sdrfm_ring_t* r);
int  sdrfm_ring_submit(sdrfm_ring_t* r, const uint8_t* iq, uint32_t nbytes);
int  sdrfm_ring_collect(sdrfm_ring_t* r, float* audio, uint32_t audio_cap, uint32_t* n_audio, int wait);

/* ------------------------------------------------------------------------------------------------------------------
 * Multi-channel WBFM (BASELINE configs[4]): one wide capture (3.2 MS/s) -> 16-band critically-sampled polyphase
 * channelizer (prototype low-pass p[0..P), P a multiple of 16; each band at fs/16 = 200 kS/s) -> per-band FM
 * discriminator -> rational L/M resampler (6/25 -> 48 kHz) with prototype g[0..Tg) given at the L-times-upsampled rate.
 * Same hand-off contract as sdrfm_process_batch (buffer format, status codes, threading); arithmetic: DESIGN.md.
 * audio layout: audio[(stream * 16 + band) * band_stride + j].
 * ------------------------------------------------------------------------------------------------------------------ */
#define SDRFM_WBFM_BANDS 16
/* flags for sdrfm_wbfm_config.flags (all are test hooks; results do not depend on them) */
#define SDRFM_WBFM_CFG_FORCE_GENERIC 1u        /* never run a fused kernel */
#define SDRFM_WBFM_CFG_BRANCH_LANES 2u         /* fused kernel with one lane per polyphase branch instead of one lane per step */
#define SDRFM_WBFM_CFG_RUN_STEPS_SHIFT 8       /* flags >> 8 = fixed run length (steps, 64..8192) of the fused kernel, 0 = chosen per call */

typedef struct sdrfm_wbfm_config {
  uint32_t struct_size;           /* = sizeof(sdrfm_wbfm_config) */
  uint32_t n_streams;
  uint32_t proto_taps;            /* P: multiple of 16, <= 512 */
  const float* proto_coeffs;
  uint32_t resamp_taps;           /* Tg <= 512 */
  uint32_t resamp_up;             /* L <= 64 */
  uint32_t resamp_down;           /* M <= 256 */
  const float* resamp_coeffs;
  uint32_t max_bytes_per_call;    /* per stream; 0 = 1 MiB */
  int32_t  device;
  uint32_t flags;                 /* SDRFM_WBFM_CFG_* */
} sdrfm_wbfm_config;

typedef struct sdrfm_wbfm sdrfm_wbfm_t;

int  sdrfm_wbfm_create(const sdrfm_wbfm_config* cfg, sdrfm_wbfm_t** out);
void sdrfm_wbfm_destroy(sdrfm_wbfm_t* h);
int  sdrfm_wbfm_reset(sdrfm_wbfm_t* h);
int  sdrfm_wbfm_audio_count(const sdrfm_wbfm_t* h, uint32_t nbytes, uint32_t* n_audio_per_band);
int  sdrfm_wbfm_process_batch(sdrfm_wbfm_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes_per_stream,
                              float* audio, size_t band_stride, uint32_t* n_audio_per_band, uint32_t flags);
int  sdrfm_wbfm_set_stream(sdrfm_wbfm_t* h, void* hip_stream);
int  sdrfm_wbfm_synchronize(sdrfm_wbfm_t* h);
/* the kernel that served the LAST call (before any call: the one the configuration selects): starts with "wbfm-fused" (128-tap
   prototype, <= 10 resampler taps per phase; the kernel follows in brackets) or "wbfm-generic" (any shape, two kernels; also
   serves calls too short for a fused kernel) */
const char* sdrfm_wbfm_kernel_name(const sdrfm_wbfm_t* h);

/* ------------------------------------------------------------------------------------------------------------------
 * Broadcast FM stereo: the same hand-off contract as sdrfm_process_batch (buffer format, status codes,
 * threading), two audio channels L and R per stream.  K1-K3 (x, y, d, with the state carried across calls) are the definition
 * at the top of this file, unchanged; behind d, at fs/D, every FIR is an fp32 fmaf chain, oldest sample first, d[m < 0] = 0:
 *   pilot filter  q[m]  = sum_k b[k] * d[m-k]          P odd, 1 <= P <= 255, Δ = (P-1)/2; b[k] = (br[k], bi[k]) complex taps
 *                                                      given by the caller: two real chains qr, qi
 *   pilot power   pw    = fmaf(qr, qr, qi*qi)          pmin2 = pilot_min * pilot_min (fp32, once on the host; may be +inf;
 *                                                      a pilot_min whose pmin2 rounds to 0 is refused: SDRFM_EINVAL)
 *   38 kHz        c[m]  = pw >= pmin2 ? (-2.0f*(qr*qi)) / pw : 0.0f
 *   difference    s[m]  = (c[m] * diff_gain) * d[m-Δ]
 *   sum channel   am[j] = sum_k g[k] * d[(j+1)*Da - 1 - k - Δ]
 *   diff. channel as[j] = sum_k g[k] * s[(j+1)*Da - 1 - k]
 *   output        L[j]  = am[j] + as[j],  R[j] = am[j] - as[j]          (radians, like the mono audio)
 * The audio indexes and the per-call output count are the mono path's for the same (D, Da).  With taps from
 * taps.stereo_pilot_taps (b[k] = 2 w[k] exp(+j 2 pi f_pilot/fs_d (k - Δ)), w a unity-DC-gain low-pass) |q| is the pilot's
 * amplitude in radians, so pilot_min is in the unit of the audio.  d is the phase step over D inputs: a D-sample boxcar of the
 * instantaneous frequency, gain H_D(f) = sin(pi f D/fs) / (D sin(pi f/fs)); the L-R subcarrier at 38 kHz arrives H_D(38 kHz)
 * weaker than L+R (0.9597 at D = 10, 2.4 MS/s), so diff_gain = 2 / H_D(38 kHz) (taps.stereo_diff_gain) separates the channels by
 * 43-47 dB where the textbook 2 leaves about 32 dB.
 * Mono identity: where c = 0 and P - 1 = 2 K Da, L == R == a[j - K] bit for bit, a the mono audio of the same (h, g) (a[j < 0] = 0).
 * Parity unpinned like the rest: every kernel that serves it is bit-identical to this definition.
 * pilot_count (n_streams words, or NULL): per stream, how many of the call's new d's had pw >= pmin2 (a "stereo" indicator).
 * Host buffers: synchronous staged call.  SDRFM_F_DEVICE_PTRS: iq, left, right and pilot_count are device memory on cfg.device,
 * the call is only enqueued on the handle's stream.  SDRFM_F_OVERLAP is rejected (SDRFM_EINVAL).  Any even nbytes up to
 * max_bytes_per_call (else SDRFM_ECAPACITY).  Invalid configurations answer SDRFM_EINVAL before any device is looked for.
 * kernel name: "stereo-fast ..." (T = 64, D = 10, P = 101) or "stereo-generic ..." (every other shape); same bits either way.
 * ------------------------------------------------------------------------------------------------------------------ */
#define SDRFM_STEREO_MAX_PILOT_TAPS 255u
#define SDRFM_STEREO_CFG_FORCE_GENERIC 1u   /* never the fast kernel (tests) */

typedef struct sdrfm_stereo_config {
  uint32_t struct_size;           /* = sizeof(sdrfm_stereo_config) */
  uint32_t n_streams;
  uint32_t fir_taps;              /* T, as sdrfm_config */
  uint32_t fir_decim;             /* D, as sdrfm_config */
  const float* fir_coeffs;        /* h[0..T), copied at create */
  uint32_t pilot_taps;            /* P: odd, 1 .. SDRFM_STEREO_MAX_PILOT_TAPS */
  const float* pilot_coeffs;      /* 2P floats: (br[k], bi[k]) pairs, copied at create */
  float    pilot_min;             /* finite, > 0, pilot_min * pilot_min > 0 in fp32 (radians, the unit of |q|) */
  float    diff_gain;             /* finite; 2 = textbook, 2 / H_D(38 kHz) compensates the discriminator */
  uint32_t audio_taps;            /* Ta, as sdrfm_config */
  uint32_t audio_decim;           /* Da, as sdrfm_config */
  const float* audio_coeffs;      /* g[0..Ta), copied at create */
  uint32_t max_bytes_per_call;    /* per stream; 0 = 1 MiB */
  int32_t  device;
  uint32_t flags;                 /* 0 or SDRFM_STEREO_CFG_FORCE_GENERIC */
} sdrfm_stereo_config;

typedef struct sdrfm_stereo sdrfm_stereo_t;

int  sdrfm_stereo_create(const sdrfm_stereo_config* cfg, sdrfm_stereo_t** out);
void sdrfm_stereo_destroy(sdrfm_stereo_t* h);
int  sdrfm_stereo_reset(sdrfm_stereo_t* h);
int  sdrfm_stereo_audio_count(const sdrfm_stereo_t* h, uint32_t nbytes, uint32_t* n_audio);
/* left / right for stream s at left + s*audio_stride, right + s*audio_stride (floats) */
int  sdrfm_stereo_process_batch(sdrfm_stereo_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* left, float* right,
                                size_t audio_stride, uint32_t* pilot_count, uint32_t* n_audio, uint32_t flags);
/* sdrfm_stereo_set_stream, and sdrfm_rds_set_stream, sdrfm_bcast_set_stream and sdrfm_scan_set_stream likewise: run on a caller-owned HIP stream
 * (NULL: the handle's own again).  The call WAITS for the stream in use before it switches, as the PCM-side handles' set_stream does: a launch on the
 * old stream may still read the taps and write the carried state that a tune, a reset or a call behind the switch replaces.  _reset zeroes the
 * carried state in stream order and waits for the stream; _synchronize waits for it. */
int  sdrfm_stereo_set_stream(sdrfm_stereo_t* h, void* hip_stream);
int  sdrfm_stereo_synchronize(sdrfm_stereo_t* h);
const char* sdrfm_stereo_kernel_name(const sdrfm_stereo_t* h);

/* ------------------------------------------------------------------------------------------------------------------
 * Radio Data System, layer 1: IQ bytes in, the complex RDS baseband out.  The same hand-off contract as
 * sdrfm_stereo_process_batch (buffer format, status codes, threading).  K1-K3 (x, y, d, state carried across calls) and the pilot
 * filter are the stereo definition's, unchanged: q[m] = sum_k b[k] * d[m-k] as two real fp32 fmaf chains, oldest sample first,
 * P odd, Δ = (P-1)/2, pw = fmaf(qr, qr, qi*qi), pmin2 = pilot_min * pilot_min (a pmin2 that rounds to 0 is refused).  Behind it,
 * all fp32, every product and quotient rounded once, no contraction other than the fmafs written:
 *   pilot's 2nd harmonic, unit size   on = pw >= pmin2; u2r = fmaf(qr, qr, -(qi*qi)) / pw, u2i = (2.0f*(qr*qi)) / pw
 *   57 kHz carrier, size |q|          kr = fmaf(u2r, qr, -(u2i*qi)), ki = fmaf(u2r, qi, u2i*qr); kr = ki = 0.0f where !on
 *   mixed down                        zr[m] = (kr*rds_gain) * d[m-Δ], zi[m] = (ki*rds_gain) * d[m-Δ]; z[m<0] = 0, d[m<0] = 0
 *   decimating low-pass               wr[j] = sum_k g[k] * zr[(j+1)*Dr - 1 - k], wi[j] likewise: fmaf chains, oldest first
 *   output                            bb[stream*bb_stride + 2j] = wr[j], bb[... + 2j + 1] = wi[j] (floats), at fs/(D*Dr)
 * The carrier is |q| e^{j3φ} and not e^{j3φ}: the odd harmonic of a unit phasor needs a square root, and only fmaf, products and /
 * are known to match the fp32 reference bit for bit.  BPSK decoding is scale-free and the pilot's size is constant for a station,
 * so nothing is lost.  The standard lets the RDS subcarrier sit in phase or in quadrature with the pilot's third harmonic: the data
 * may arrive on any fixed axis of w, which is why the output is complex and why the decoder below finds the axis.
 * rds_gain = 2 / H_D(57 kHz) (taps.rds_gain) undoes the discriminator's boxcar at the subcarrier.
 * The per-call output count is the mono path's for (D, Dr).  pilot_count (n_streams words, or NULL): per stream, how many of the
 * call's new d's had pw >= pmin2.  Parity unpinned like the rest: every kernel that serves it is bit-identical to this definition.
 * Host buffers: synchronous staged call.  SDRFM_F_DEVICE_PTRS: iq, bb and pilot_count are device memory on cfg.device, the call is
 * only enqueued on the handle's stream.  SDRFM_F_OVERLAP is rejected (SDRFM_EINVAL).  Any even nbytes up to max_bytes_per_call
 * (else SDRFM_ECAPACITY).  Invalid configurations answer SDRFM_EINVAL before any device is looked for.
 * kernel name: "rds-fast ..." (T = 64, D = 10, P = 101, any Tr, Dr) or "rds-generic ..." (every other shape); same bits either way.
 * ------------------------------------------------------------------------------------------------------------------ */
#define SDRFM_RDS_CFG_FORCE_GENERIC 1u      /* never the fast kernel (tests) */

typedef struct sdrfm_rds_config {
  uint32_t struct_size;           /* = sizeof(sdrfm_rds_config) */
  uint32_t n_streams;
  uint32_t fir_taps;              /* T, as sdrfm_config */
  uint32_t fir_decim;             /* D, as sdrfm_config */
  const float* fir_coeffs;        /* h[0..T), copied at create */
  uint32_t pilot_taps;            /* P: odd, 1 .. SDRFM_STEREO_MAX_PILOT_TAPS */
  const float* pilot_coeffs;      /* 2P floats: (br[k], bi[k]) pairs, copied at create */
  float    pilot_min;             /* finite, > 0, pilot_min * pilot_min > 0 in fp32 (radians, the unit of |q|) */
  float    rds_gain;              /* finite; 2 / H_D(57 kHz) compensates the discriminator */
  uint32_t rds_taps;              /* Tr: 1 .. SDRFM_MAX_TAPS */
  uint32_t rds_decim;             /* Dr: 1 .. SDRFM_MAX_DECIM */
  const float* rds_coeffs;        /* g[0..Tr), copied at create */
  uint32_t max_bytes_per_call;    /* per stream; 0 = 1 MiB */
  int32_t  device;
  uint32_t flags;                 /* 0 or SDRFM_RDS_CFG_FORCE_GENERIC */
} sdrfm_rds_config;

typedef struct sdrfm_rds sdrfm_rds_t;

int  sdrfm_rds_create(const sdrfm_rds_config* cfg, sdrfm_rds_t** out);
void sdrfm_rds_destroy(sdrfm_rds_t* h);
int  sdrfm_rds_reset(sdrfm_rds_t* h);
/* complex outputs of the NEXT call of nbytes */
int  sdrfm_rds_count(const sdrfm_rds_t* h, uint32_t nbytes, uint32_t* n_out);
/* bb for stream s at bb + s*bb_stride (floats; 2 per output: bb_stride >= 2 * n_out) */
int  sdrfm_rds_process_batch(sdrfm_rds_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* bb, size_t bb_stride,
                             uint32_t* pilot_count, uint32_t* n_out, uint32_t flags);
int  sdrfm_rds_set_stream(sdrfm_rds_t* h, void* hip_stream);   /* waits for the stream in use, then switches: see sdrfm_stereo_set_stream */
int  sdrfm_rds_synchronize(sdrfm_rds_t* h);
const char* sdrfm_rds_kernel_name(const sdrfm_rds_t* h);

/* Layer 2 (plain C, host only, no GPU): the 1187.5 bit/s part.
 *   sdrfm_rds_checkword(info, offset) = (info * x^10 mod g(x)) XOR offset word, g(x) = x^10+x^8+x^7+x^5+x^4+x^3+1 (0x5B9);
 *                                       offset 0..4 = A 0x0FC, B 0x198, C 0x168, C' 0x350, D 0x1B4 (any other: 0xFFFF)
 *   sdrfm_rds_syndrome(block26)       = block26 mod g(x): syndrome((info << 10) | checkword(info, o)) is offset word o itself.
 * sdrfm_rds_sync_t is one stream's decoder: it finds the data axis of w, recovers the 1187.5 Hz bit clock and tracks it (a dongle
 * crystal is off by up to +-100 ppm), undoes the biphase symbol and the differential coding, acquires block synchronisation only
 * on two consecutive blocks whose syndromes are offset words in sequence 26 bits apart, drops it after a run of failed blocks, and
 * emits one sdrfm_rds_group per group: block[i] the 16 information bits of block i + 1, ok_mask bit i set where that block's
 * syndrome was its offset word (error detection only: no correction), version_b 1 where block 3 carried C'.
 * State persists across pushes: any cut of a baseband into pushes gives the same groups.  bb holds n (re, im) pairs; at most cap
 * groups are written (further ones of that push are dropped: give cap >= n / (104 * samples per bit) + 1). */
typedef struct sdrfm_rds_group {
  uint16_t block[4];
  uint8_t  ok_mask;
  uint8_t  version_b;
} sdrfm_rds_group;

typedef struct sdrfm_rds_sync_info {
  uint64_t bits;                  /* bits decided */
  uint64_t blocks_ok;             /* blocks with the expected syndrome, while in sync */
  uint64_t blocks_failed;
  uint32_t in_sync;
  uint32_t groups;                /* groups emitted */
} sdrfm_rds_sync_info;

typedef struct sdrfm_rds_sync sdrfm_rds_sync_t;

uint16_t sdrfm_rds_checkword(uint16_t info, int offset);
uint16_t sdrfm_rds_syndrome(uint32_t block26);
int  sdrfm_rds_sync_create(double sample_rate_hz, sdrfm_rds_sync_t** out);   /* 4 .. 64 samples per bit, else SDRFM_EINVAL */
void sdrfm_rds_sync_destroy(sdrfm_rds_sync_t* s);
int  sdrfm_rds_sync_reset(sdrfm_rds_sync_t* s);
int  sdrfm_rds_sync_push(sdrfm_rds_sync_t* s, const float* bb, uint32_t n, sdrfm_rds_group* out, uint32_t cap, uint32_t* n_out);
int  sdrfm_rds_sync_stats(const sdrfm_rds_sync_t* s, sdrfm_rds_sync_info* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Broadcast receiver: the stereo audio and the RDS baseband of the same streams from one kernel launch, for the
 * user who tunes a station and wants both.  There is no new arithmetic: L and R are the stereo definition's above, bb is the RDS
 * definition's, both evaluated on the same d and the same pilot filter output q, and pilot_count is the one number the two handles
 * agree on.  Every output bit equals what sdrfm_stereo_process_batch and sdrfm_rds_process_batch give for the same taps, pilot_min,
 * gains and sequence of calls; the launch walks K1-K3 and the pilot filter once where the two handles walk them twice.
 * The configuration is the union of the two; its limits and refusals are theirs (SDRFM_EINVAL before any device is looked for).
 * The two decimators' phases are carried separately: n_audio is the mono path's count for (D, Da), n_rds the one for (D, Dr).
 * The hand-off contract is sdrfm_stereo_process_batch's: host buffers make a synchronous staged call; with SDRFM_F_DEVICE_PTRS iq,
 * left, right, bb and pilot_count are device memory on cfg.device and the call is only enqueued on the handle's stream.
 * SDRFM_F_OVERLAP is rejected (SDRFM_EINVAL); odd nbytes: SDRFM_EODD; nbytes above max_bytes_per_call, or (with more than one
 * stream) iq_stride < nbytes, audio_stride < n_audio, bb_stride < 2 * n_rds: SDRFM_ECAPACITY.  left / right (bb) may be NULL only
 * when this call's n_audio (n_rds) is 0; pilot_count may be NULL.  nbytes == 0 is a no-op that zeroes pilot_count.  A refused call
 * leaves the state alone.
 * kernel name: "bcast-fast T64 D10 P101 Ta.. Da.. Tr.. Dr.." (T = 64, D = 10, P = 101, any Ta, Da, Tr, Dr whose step fits the
 * workgroup's memory) or "bcast-generic ..." (every other shape); same bits either way.
 * ------------------------------------------------------------------------------------------------------------------ */
#define SDRFM_BCAST_CFG_FORCE_GENERIC 1u    /* never the fast kernel (tests) */

typedef struct sdrfm_bcast_config {
  uint32_t struct_size;           /* = sizeof(sdrfm_bcast_config) */
  uint32_t n_streams;
  uint32_t fir_taps;              /* T, as sdrfm_config */
  uint32_t fir_decim;             /* D, as sdrfm_config */
  const float* fir_coeffs;        /* h[0..T), copied at create */
  uint32_t pilot_taps;            /* P: odd, 1 .. SDRFM_STEREO_MAX_PILOT_TAPS */
  const float* pilot_coeffs;      /* 2P floats: (br[k], bi[k]) pairs, copied at create */
  float    pilot_min;             /* finite, > 0, pilot_min * pilot_min > 0 in fp32 (radians, the unit of |q|) */
  float    diff_gain;             /* finite; as sdrfm_stereo_config */
  uint32_t audio_taps;            /* Ta: 1 .. SDRFM_MAX_TAPS */
  uint32_t audio_decim;           /* Da: 1 .. SDRFM_MAX_DECIM */
  const float* audio_coeffs;      /* g[0..Ta) of the stereo definition, copied at create */
  float    rds_gain;              /* finite; as sdrfm_rds_config */
  uint32_t rds_taps;              /* Tr: 1 .. SDRFM_MAX_TAPS */
  uint32_t rds_decim;             /* Dr: 1 .. SDRFM_MAX_DECIM */
  const float* rds_coeffs;        /* g[0..Tr) of the RDS definition, copied at create */
  uint32_t max_bytes_per_call;    /* per stream; 0 = 1 MiB */
  int32_t  device;
  uint32_t flags;                 /* 0 or SDRFM_BCAST_CFG_FORCE_GENERIC */
} sdrfm_bcast_config;

typedef struct sdrfm_bcast sdrfm_bcast_t;

int  sdrfm_bcast_create(const sdrfm_bcast_config* cfg, sdrfm_bcast_t** out);
void sdrfm_bcast_destroy(sdrfm_bcast_t* h);
int  sdrfm_bcast_reset(sdrfm_bcast_t* h);
/* audio outputs (per channel) and complex RDS outputs of the NEXT call of nbytes */
int  sdrfm_bcast_counts(const sdrfm_bcast_t* h, uint32_t nbytes, uint32_t* n_audio, uint32_t* n_rds);
/* left / right for stream s at left + s*audio_stride, right + s*audio_stride (floats); bb at bb + s*bb_stride (floats; 2 per output) */
int  sdrfm_bcast_process_batch(sdrfm_bcast_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* left, float* right,
                               size_t audio_stride, float* bb, size_t bb_stride, uint32_t* pilot_count, uint32_t* n_audio,
                               uint32_t* n_rds, uint32_t flags);
int  sdrfm_bcast_set_stream(sdrfm_bcast_t* h, void* hip_stream);   /* waits for the stream in use, then switches: see sdrfm_stereo_set_stream */
int  sdrfm_bcast_synchronize(sdrfm_bcast_t* h);
const char* sdrfm_bcast_kernel_name(const sdrfm_bcast_t* h);

/* Tuning: stream s of a broadcast handle receives the station at an offset f_s of its input — a 2.4 MS/s capture
 * holds up to a dozen stations beside the one at 0 Hz — and, with SDRFM_TUNE_SHARED_INPUT, all streams read one shared capture.
 * A tuned stream has complex channel taps hz[k] = (hr[k], hi[k]), k in [0, T), and a rotation rot, both fp32 and given by the caller
 * as the pilot taps are: the library computes no trigonometry.  The intended values, evaluated in float64 and rounded once, are
 *     hz[k] = h[k] exp(+j 2 pi f k / fs),      rot = 2 pi f D / fs wrapped into [-pi, pi]
 * (the low-pass h moved to f; the phase y gains over D inputs from the offset alone).
 *   K2  two of the frozen definition's real chains, each exactly K2 (fp32 fmaf, oldest sample first, the same x and history) with
 *       another tap set: A = sum hr[k] x[..] = (Ar, Ai), B = sum hi[k] x[..] = (Br, Bi); yr = Ar - Bi, yi = Ai + Br, one rounding each.
 *   K3  re, im as in the frozen K3; d = 0 where both are 0 (no rotation is subtracted: d[0] of a stream stays 0); otherwise
 *       v = atan2f(im, re) - rot, then v -= 2 pi if v > pi, else v += 2 pi if v < -pi (pi = 0x1.921fb6p+1f, 2 pi = 0x1.921fb6p+2f).
 * Everything behind d — pilot filter, carriers, audio and RDS chains, counts, decimator phases, the PCM one-call form — is untouched.
 * The carried state keeps its kind: the input history is raw x, the carried y is the tuned one, the carried d's are de-rotated.
 *
 * sdrfm_bcast_tune copies ctaps (n_streams x 2T floats: stream s's (hr[k], hi[k]) pairs at ctaps + s * 2T) and rot (n_streams floats),
 * takes effect with the next call and zeroes the carried state: a re-tune is a restart.  sdrfm_bcast_reset keeps the tuning.
 * ctaps == NULL with rot == NULL and flags 0 returns the handle to the untuned kernels and their bits.  Non-finite taps or rot,
 * |rot| > pi (the fp32 constant above), unknown flags, or only one of ctaps / rot NULL: SDRFM_EINVAL, and nothing is changed.
 * With SDRFM_TUNE_SHARED_INPUT every stream reads row 0 of iq and iq_stride is ignored; a host-buffer call stages that one row.
 * sdrfm_bcast_process_batch and sdrfm_bcast_process_batch_pcm take a tuned handle as they take any other; the kernel name then reads
 * "bcast-fast-tuned ..." or "bcast-generic-tuned ...", the same bits either way.
 * The mono handle, the stereo-only handle and the RDS-only handle have no tuning. */
#define SDRFM_TUNE_SHARED_INPUT 1u   /* every stream reads row 0 of iq; iq_stride is ignored */
int  sdrfm_bcast_tune(sdrfm_bcast_t* h, const float* ctaps, const float* rot, uint32_t flags);

/* ------------------------------------------------------------------------------------------------------------------
 * Scan: which offsets of a capture hold a station, how far off the tuning is, how strong the station is and whether
 * it carries a pilot.  A scan stream is a tuned stream of the section above up to d and the pilot filter — x, the tuned K2 (two real
 * fmaf chains, yr = Ar - Bi, yi = Ai + Br), sdrfm_discriminate_tuned's K3, the carried state (input history, y[-1], the last P - 1 d's)
 * and the pilot filter q[m] = sum_k b[k] d[m - k] as two fp32 fmaf chains, oldest first, d[m < 0] = 0 — and nothing behind q.
 * For every NEW d of a call, index m, five fp32 terms, each rounded once where written:
 *     p  = fmaf(yr, yr, yi*yi)        |y[m]|^2
 *     d  = d[m]
 *     e  = d*d
 *     pw = fmaf(qr, qr, qi*qi)        q = q[m]: the window that ENDS at the new d m
 *     g  = pw*pw
 * Each term becomes an integer by (int64) rintf(term * 2^k) — ties to even; the scaling by a power of two is exact and the conversion
 * of an integral float is exact — with k = 8 for p, 24 for d, e and pw, 20 for g, and the record of a stream is the sum over the call.
 * INTEGER SUMS ARE ASSOCIATIVE: the record does not depend on the workgroup split, on the order the waves arrive in, on which kernel
 * form ran, or on how a capture is cut into calls — the records of consecutive calls ADD UP EXACTLY (sdrfm_scan_meter_add) to the
 * record of the one call over the concatenated bytes.  That is the point of the fixed-point form.
 * Bounds that keep every sum inside int64, refused with SDRFM_EINVAL at create and at tune:
 *     sum_k (|hr[k]| + |hi[k]|) <= 16 per stream     |yr|, |yi| <= 2040, p <= 8 323 200
 *     sum_k (|br[k]| + |bi[k]|) <= 8                 |qr|, |qi| <= 8 pi, pw <= 1270
 *     max_bytes_per_call <= 4 MiB                    n <= 2^21 new d's per call
 * Worst-case sums of one call: |rf_q| < 2^52, |freq_q| < 2^47, dev_q < 2^49, pilot_q < 2^56, pilot2_q < 2^62.  (The intended taps have
 * sums of about 2 and 3.4.)  sdrfm_scan_meter_add adds without a check: the sum of many calls is the caller's to bound.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct sdrfm_scan_meter {   /* 64 bytes */
  uint64_t n;         /* new d's of the call (M) */
  uint64_t n_pilot;   /* those with pw >= pilot_min^2: what pilot_count counts */
  int64_t  rf_q;      /* sum rint(p  * 2^8)  */
  int64_t  freq_q;    /* sum rint(d  * 2^24) */
  int64_t  dev_q;     /* sum rint(e  * 2^24) */
  int64_t  pilot_q;   /* sum rint(pw * 2^24) */
  int64_t  pilot2_q;  /* sum rint(g  * 2^20) */
  uint64_t reserved;  /* 0 */
} sdrfm_scan_meter;

#define SDRFM_SCAN_CFG_FORCE_GENERIC 1u      /* tests: never the fast kernel */
#define SDRFM_SCAN_CFG_SHARED_INPUT  2u      /* every stream reads row 0 of iq; iq_stride ignored; a host call stages one row */
typedef struct sdrfm_scan_config {
  uint32_t struct_size;           /* = sizeof(sdrfm_scan_config) */
  uint32_t n_streams;             /* candidates */
  uint32_t fir_taps;              /* T */
  uint32_t fir_decim;             /* D */
  const float* ctaps;             /* n_streams x 2T, (hr[k], hi[k]) pairs, as sdrfm_bcast_tune's */
  const float* rot;               /* n_streams, |rot| <= pi */
  uint32_t pilot_taps;            /* P, odd */
  const float* pilot_coeffs;      /* 2P floats (re, im) */
  float    pilot_min;             /* the gate n_pilot counts with, as the stereo handle's */
  uint32_t max_bytes_per_call;    /* per stream; 0 = 1 MiB; at most 4 MiB */
  int32_t  device;
  uint32_t flags;                 /* SDRFM_SCAN_CFG_* */
} sdrfm_scan_config;

typedef struct sdrfm_scan sdrfm_scan_t;

/* The contract is sdrfm_bcast_process_batch's.  Host buffers: a synchronous staged call.  SDRFM_F_DEVICE_PTRS: iq and meters are device
 * memory (meters 8-byte aligned) and the call is only enqueued on the handle's stream.  SDRFM_F_OVERLAP and unknown flags: SDRFM_EINVAL.
 * Odd nbytes: SDRFM_EODD.  nbytes above the maximum, or iq_stride < nbytes on unshared rows of more than one stream: SDRFM_ECAPACITY.
 * meters (n_streams records) is OVERWRITTEN: zeroed on the handle's stream before the launch adds to it; nbytes == 0 gives zero records.
 * A refused call leaves the carried state alone.  Every refusal of create comes before any device is looked for.
 * sdrfm_scan_tune replaces both ctaps and rot and restarts the streams (either NULL, a non-finite value, |rot| > pi or a tap sum above
 * its bound: SDRFM_EINVAL, nothing changed); sdrfm_scan_reset zeroes the carried state and keeps the tuning.
 * Kernel name: "scan-fast T64 D10 P101" or "scan-generic T.. D.. P.."; the same records either way. */
int  sdrfm_scan_create(const sdrfm_scan_config* cfg, sdrfm_scan_t** out);
void sdrfm_scan_destroy(sdrfm_scan_t* h);
int  sdrfm_scan_reset(sdrfm_scan_t* h);
int  sdrfm_scan_tune(sdrfm_scan_t* h, const float* ctaps, const float* rot);
int  sdrfm_scan_process_batch(sdrfm_scan_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, sdrfm_scan_meter* meters, uint32_t flags);
int  sdrfm_scan_set_stream(sdrfm_scan_t* h, void* hip_stream);   /* waits for the stream in use, then switches: see sdrfm_stereo_set_stream */
int  sdrfm_scan_synchronize(sdrfm_scan_t* h);
const char* sdrfm_scan_kernel_name(const sdrfm_scan_t* h);

/* Host-only (plain C, no GPU): what a record says, in double.  fs is the input rate, D the handle's fir_decim, pilot_gain the gain
 * H_D(19 kHz) of the discriminator's D-sample boxcar at the pilot (sin(pi f D/fs) / (D sin(pi f/fs)); 0.98982 at D = 10, 2.4 MS/s).
 * With the means taken over the record's n:
 *     level_dbfs        10 log10(mean p / 127.5^2)
 *     freq_err_hz       mean d * fs / (2 pi D)                               the carrier's distance from the tuned offset
 *     dev_rms_hz        sqrt(mean e - (mean d)^2) * fs / (2 pi D)            the rms deviation about that carrier
 *     pilot_rms_rad     sqrt(mean pw)                                        rms |q|, the pilot's amplitude in d
 *     pilot_dev_hz      pilot_rms_rad * fs / (2 pi D) / pilot_gain           the pilot's deviation
 *     pilot_frac        n_pilot / n
 *     pilot_steadiness  n * sum g / (sum pw)^2 on the de-scaled sums         1 for a steady pilot, 2 for noise
 * n == 0: every field is NaN (SDRFM_OK).  NULL m or out, D == 0, fs or pilot_gain not finite and positive: SDRFM_EINVAL. */
typedef struct sdrfm_scan_report_t {
  double level_dbfs, freq_err_hz, dev_rms_hz, pilot_rms_rad, pilot_dev_hz, pilot_frac, pilot_steadiness;
} sdrfm_scan_report_t;
int  sdrfm_scan_report(const sdrfm_scan_meter* m, double fs, uint32_t D, double pilot_gain, sdrfm_scan_report_t* out);
/* acc += m, field by field (two's-complement wrap-around, no check); NULL: SDRFM_EINVAL */
int  sdrfm_scan_meter_add(sdrfm_scan_meter* acc, const sdrfm_scan_meter* m);

/* The deviation HISTOGRAM of a scan stream: the record's dev_q gives an rms deviation and nothing about peaks; modulation
 * monitoring (ITU-R SM.1268) asks for the peak deviation and how often it passes +-75 kHz.  For every NEW d of a call, index m:
 *     dq  = (int32) rintf(d * 2^24)          the integer freq_q sums
 *     bin = floor(dq / 2^18) + 256
 * |d| <= pi and one ulp more at the most, so dq lies in +-52 707 179 and bin in [54, 457]; the bins outside that range stay 0.  Bin b
 * spans [(b - 256) / 64, (b - 255) / 64) rad: 1/64 rad, 596.8 Hz at 2.4 MS/s and D = 10.  hist[s][bin] counts the call's new d's of
 * stream s in uint32 (n <= 2^21 per call: no count wraps); sum_b hist[s][b] == meters[s].n.  COUNTS ARE SUMS OF ONES: a row depends on
 * nothing but the bytes — not on the workgroup split, the kernel form, the step geometry or the cut of a capture into calls — and the rows
 * of consecutive calls add up exactly (sdrfm_scan_hist_add, in uint64) to the row of the one call.
 *
 * sdrfm_scan_process_batch_hist is sdrfm_scan_process_batch — the same refusals in the same order, the same flags, host buffers staged and
 * synchronous, SDRFM_F_DEVICE_PTRS only enqueued (hist is then device memory, 4-byte aligned), meters filled with the same integers — and
 * hist besides: n_streams rows of hist_stride uint32 words.  NULL hist or hist_stride < SDRFM_SCAN_HIST_BINS: SDRFM_EINVAL, with the NULL
 * handle and NULL meters, before anything else is looked at.  The first SDRFM_SCAN_HIST_BINS words of every row are OVERWRITTEN (zeroed on
 * the handle's stream before the launch adds to them); the words of a row behind them are not touched.  nbytes == 0 gives zero rows.  A
 * refused call leaves the state and both outputs alone.  The carried state is the plain call's: the two calls may alternate on a handle.
 * The device buffer behind host hist calls is allocated at the first one (SDRFM_ENOMEM if that fails).  sdrfm_scan_kernel_name names the
 * kernel of the last call: it ends in " + hist" after a hist call and not after a plain one. */
#define SDRFM_SCAN_HIST_BINS 512u
int  sdrfm_scan_process_batch_hist(sdrfm_scan_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, sdrfm_scan_meter* meters, uint32_t* hist,
                                   size_t hist_stride, uint32_t flags);

/* Host-only (plain C, no GPU).  acc512[b] += row512[b] for the SDRFM_SCAN_HIST_BINS bins; NULL: SDRFM_EINVAL. */
int  sdrfm_scan_hist_add(uint64_t* acc512, const uint32_t* row512);
/* What a histogram says, in double.  hist512 is one stream's accumulated row; m is the record of the same calls (sdrfm_scan_meter_add) or
 * NULL; fs and D as for sdrfm_scan_report; limit_hz the deviation limit (75e3 for broadcast FM).  With k = fs / (2 pi D) Hz per rad, bin b
 * spans k (b - 256) / 64 .. k (b - 255) / 64 Hz about the tuned offset (the half step 2^-25 rad of the fixed point is ignored), and
 *     n               sum hist
 *     centre_hz       with m: k * freq_q / (2^24 * m->n), sdrfm_scan_report's freq_err_hz; without: k * sum hist[b] (b - 255.5) / 64 / n
 *     peak_pos_hz     k * (upper edge of the highest non-empty bin) - centre_hz
 *     peak_neg_hz     k * (lower edge of the lowest non-empty bin) - centre_hz
 *     peak_hz         max(peak_pos_hz, -peak_neg_hz)
 *     over_min        the share of n in bins that lie WHOLLY outside centre_hz +- limit_hz
 *     over_max        the share of n in bins that lie AT LEAST PARTLY outside it
 *     mpx_power_dbr   with m: 10 log10(2 dev_rms_hz^2 / 19000^2), dev_rms_hz as sdrfm_scan_report's: the modulation power against ITU-R
 *                     BS.412's reference, a tone of +-19 kHz peak deviation (its 60 s window is the caller's, by sdrfm_scan_meter_add);
 *                     NaN without m
 * A deviation is outside iff it is MORE than limit_hz from the centre; a bin holds its lower edge and not its upper one.  So with lo and
 * hi a bin's edges less centre_hz: wholly outside iff lo > limit or hi <= -limit, partly iff hi > limit or lo < -limit.  over_min and
 * over_max bracket the truth; nothing is interpolated.  n == 0: every field but n is NaN (SDRFM_OK).  NULL hist512 or out, D == 0, fs not
 * finite and positive, limit_hz not finite or negative, or m given with m->n != n: SDRFM_EINVAL. */
typedef struct sdrfm_scan_hist_report_t {
  uint64_t n;
  double centre_hz, peak_pos_hz, peak_neg_hz, peak_hz, over_min, over_max, mpx_power_dbr;
} sdrfm_scan_hist_report_t;
int  sdrfm_scan_hist_report(const uint64_t* hist512, const sdrfm_scan_meter* m, double fs, uint32_t D, double limit_hz, sdrfm_scan_hist_report_t* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Spectrum view of the IQ buffer — the reference's own next task ("Perform some FFT on the samples to check what we are
 * receiving", README.md:29) on the same buffer contract (RTLSDR_CommItfTypedef.buff, usbh_rtlsdr.h:165-173): per stream
 * the windowed nfft-point power spectrum averaged over the consecutive, non-overlapping frames of the buffer, DC in the
 * middle: power[stream * power_stride + i], i = 0..nfft-1, bin i = frequency (i - nfft/2) * fs/nfft.  Stateless: each
 * call views the buffer it is given; a tail shorter than nfft is ignored (*n_frames = 0 -> all zeros).
 * Arithmetic (one fixed radix-2 DIT graph, fp32): DESIGN.md §4.6.  window = NULL selects a periodic Hann window.
 * SDRFM_FAIL from a host-buffer call or from sdrfm_spectrum_synchronize also reports a device-side time-out: the 512 / 1024-point kernel hands
 * a stream's running sum from wave to wave, and a wave that waited two seconds for its predecessor (a wait of ~100 us when nothing is wrong) sets
 * an error word instead of hanging or aborting the context; the powers of that call are not valid, the handle stays usable.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct sdrfm_spectrum_config {
  uint32_t struct_size;           /* = sizeof(sdrfm_spectrum_config) */
  uint32_t n_streams;
  uint32_t nfft;                  /* power of two, 64 .. 4096 */
  const float* window;            /* nfft floats or NULL */
  uint32_t max_bytes_per_call;    /* per stream; 0 = 1 MiB */
  int32_t  device;
  uint32_t flags;                 /* must be 0 */
} sdrfm_spectrum_config;

typedef struct sdrfm_spectrum sdrfm_spectrum_t;

int  sdrfm_spectrum_create(const sdrfm_spectrum_config* cfg, sdrfm_spectrum_t** out);
void sdrfm_spectrum_destroy(sdrfm_spectrum_t* h);
int  sdrfm_spectrum_process_batch(sdrfm_spectrum_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes_per_stream,
                                  float* power, size_t power_stride, uint32_t* n_frames, uint32_t flags);
int  sdrfm_spectrum_set_stream(sdrfm_spectrum_t* h, void* hip_stream);
int  sdrfm_spectrum_synchronize(sdrfm_spectrum_t* h);
/* The kernel the last call launched, as a profiler prints it (before the first call: the one a device buffer with even iq and iq_stride
 * gets).  Up to 1024 points a kernel that reads the samples as halves of aligned dwords serves the call; one whose iq or iq_stride is odd is
 * served by the typed-load kernel of the longer lengths.  Same results either way. */
const char* sdrfm_spectrum_kernel_name(const sdrfm_spectrum_t* h);

/* ------------------------------------------------------------------------------------------------------------------
 * Host-only helpers (no GPU): the two pure computations the reference performs when it programs the RTL2832 for this
 * stream, so that a non-MCU front end configures a dongle identically.
 *   sdrfm_rtl_pack_fir  : RTLSDR_set_fir, state RTLSDR_FIR_CALC (Class/RTLSDR/Src/usbh_rtlsdr.c:552-575): RTLSDR_FIR[16]
 *                         (8 x int8 then 8 x int12) -> 20 bytes for demod page 1 regs 0x1c..0x2f.
 *   sdrfm_rtl_resampler : RTLSDR_set_sample_rate state 0 (usbh_rtlsdr.c:676-691); xtal_hz = 28 800 000 for the stock dongle.
 *   sdrfm_e4k_pll_params: E4K_compute_pll_params (Class/RTLSDR/Src/tuner_e4k.c:689-737, band table :301-312): the E4000
 *                         synthesiser word for a wanted LO — band divider R and its SYNTH7 code, integer part Z, 16-bit
 *                         fraction X (Y = 65536) and the LO actually obtained, floor(fosc*(Z + X/Y) / R) in integers.
 * All return SDRFM_EINVAL where the firmware would only log (or, for the PLL, return 0).
 * ------------------------------------------------------------------------------------------------------------------ */
int sdrfm_rtl_pack_fir(const int* fir16, uint8_t* out20);
int sdrfm_rtl_resampler(uint32_t samp_rate, uint32_t xtal_hz, uint32_t* rsamp_ratio, uint32_t* real_rsamp_ratio,
                        double* real_rate);
/* Multi-GPU fan-out / fan-in of stream batches (streams are independent: one handle per GPU, no data-path collective): the contiguous
 * block [*first, *first + *count) of the n_streams streams that rank `rank` of `world` owns; the first n_streams % world ranks own one
 * stream more.  examples/multi_gpu_main.c (one C process, N devices, RCCL send/recv) and the Python fan-out use this one definition. */
int sdrfm_shard_range(uint32_t n_streams, uint32_t world, uint32_t rank, uint32_t* first, uint32_t* count);

typedef struct sdrfm_e4k_pll {   /* mirrors struct e4k_pll_params (Class/RTLSDR/Inc/tuner_e4k.h:227-236) */
  uint32_t fosc, intended_flo, flo;
  uint16_t x;
  uint8_t z, r, r_idx, threephase;
} sdrfm_e4k_pll;
int sdrfm_e4k_pll_params(uint32_t fosc_hz, uint32_t intended_flo_hz, sdrfm_e4k_pll* out);

/* Audio sink format of the reference board (host-side, plain C): de-emphasis y += alpha*(x - y) carried in *state, then
 * int16 stereo-interleaved PCM (L = R) as BSP_AUDIO_OUT_Play(uint16_t*, Size) takes it
 * (Utilities/STM32746G-Discovery/stm32746g_discovery_audio.c:224).  pcm_stereo receives 2*n samples. */
int   sdrfm_pcm_deemph_s16(const float* audio, uint32_t n, float alpha, float gain, float* state, int16_t* pcm_stereo);
float sdrfm_pcm_alpha(float fs_hz, float tau_s);   /* 1 - exp(-1/(fs*tau)); tau = 75e-6 (US) / 50e-6 (EU) */
/* The stereo form: each channel de-emphasised on its own (state[0] for L, state[1] for R) with the operations of
 * sdrfm_pcm_deemph_s16; pcm_stereo[2i] = L, pcm_stereo[2i+1] = R. */
int   sdrfm_pcm_deemph_stereo_s16(const float* left, const float* right, uint32_t n, float alpha, float gain, float* state,
                                  int16_t* pcm_stereo);

/* The same sink ON THE DEVICE for the batched path: audio[stream * audio_stride + i] (f32, as sdrfm_process_batch leaves it) ->
 * pcm[stream * pcm_stride + 2*i + {0,1}] (int16, L = R), de-emphasis state carried per stream in the handle.  pcm_stride is in int16
 * elements, even, >= 2*n.  With SDRFM_F_DEVICE_PTRS both buffers are device memory (pcm 4-byte aligned) and the call only
 * enqueues on the sink's stream; give it the demodulator's stream (or synchronise) so that it runs after the audio exists.
 * Two forms of the same recursion (csrc/sdrfm_sink.hip):
 *   default            a blocked scan — 256 lanes per stream walk chunks of the call, the carries between chunks by a scan, every chunk then
 *                      re-walked from its true carry-in with the exact form's own operations: PCM within 1 LSB of the exact form's (different only
 *                      where y * gain sits on a rounding boundary), carried state within 1e-6 relative; microseconds per 256 x 4800 call
 *                      (profiles/r06_sink.txt);
 *   SDRFM_PCM_F_EXACT  one lane per stream, the operations of sdrfm_pcm_deemph_s16 in its order: BIT-IDENTICAL to it (and to an exact-rational
 *                      restatement: tests/test_pcm_sink_gpu.py); latency-bound: 1.35 ms per 256 x 4800 call. */
#define SDRFM_PCM_F_EXACT 4u      /* flag for sdrfm_pcm_sink_process_batch (beside SDRFM_F_DEVICE_PTRS) */
typedef struct sdrfm_pcm_sink sdrfm_pcm_sink_t;
int  sdrfm_pcm_sink_create(uint32_t n_streams, float alpha, float gain, int32_t device, sdrfm_pcm_sink_t** out);
void sdrfm_pcm_sink_destroy(sdrfm_pcm_sink_t* k);
int  sdrfm_pcm_sink_reset(sdrfm_pcm_sink_t* k);
int  sdrfm_pcm_sink_process_batch(sdrfm_pcm_sink_t* k, const float* audio, size_t audio_stride, uint32_t n,
                                  int16_t* pcm, size_t pcm_stride, uint32_t flags);
int  sdrfm_pcm_sink_set_stream(sdrfm_pcm_sink_t* k, void* hip_stream);
int  sdrfm_pcm_sink_synchronize(sdrfm_pcm_sink_t* k);
int  sdrfm_pcm_sink_get_state(sdrfm_pcm_sink_t* k, float* state_out /* n_streams floats */);

/* ONE call of the demodulator and of the sink (round 6): sdrfm_process_batch(h, iq, ..., audio, ..., flags) and then the sink's default form over that
 * audio into pcm.  With SDRFM_F_DEVICE_PTRS the buffers are device memory and the call only enqueues (SDRFM_F_OVERLAP as for sdrfm_process_batch, with pcm
 * rotated like audio); without it they are host memory and the call stages, runs and copies back, synchronous like sdrfm_process_batch with host buffers — the
 * reference superloop's two steps on one filled CommItf.buff: demodulate it, hand int16 stereo to BSP_AUDIO_OUT_Play.
 * Where the matrix-pipe kernel serves the whole call, the sink's chain runs INSIDE its launch (csrc/sdrfm_sink_chain.h): the de-emphasis forgets — (1 - alpha)^64
 * is below rounding —, so every wave sinks the ~400 outputs it has just computed where they lie, publishes its end state in one word, and finishes its first 64
 * outputs with its neighbour's.  No second launch, no stream to order, nothing between two overlapped calls: the consumer loop of INTEGRATION.md section 3 runs
 * within 10 % of the demodulator's own rate (profiles/r06_sink.txt).  A batch with streams routed to the bit-exact kernels keeps the chain for the others (both
 * designs in one launch) and is followed, on the call's own queue, by the sink's kernel over the routed streams only (+4.5 us per call).  Any other call (the
 * bit-exact kernels alone, the first call of a stream, a sink whose alpha lies outside [0.231, 1 - 1.8e-5] — below it a run's end state still depends on its predecessor's; above it (1 - alpha)^8 is no normal float and (1 - alpha)^-7, by which a run's end state is published, overflows: at alpha = 1 the chain would publish NaN) is followed by the
 * sink's own kernel on the handle's stream, behind a join of the overlapped calls.
 * Same results either way up to the blocked scan's tolerance: PCM within 1 LSB of sdrfm_pcm_deemph_s16's, state within 1e-6 relative.
 * audio may be NULL: the PCM is then all the call leaves (a launch that holds the chain does not store the float audio at all; other calls use rows of the
 * library's own); otherwise the audio is written as by sdrfm_process_batch.
 * The sink must belong to h's device and have h's n_streams; between calls made this way and sdrfm_pcm_sink_process_batch calls on the same sink, synchronise
 * both (the chain of call c waits ON THE DEVICE for the sink's call c - 1, which must already be in a queue); sdrfm_pcm_sink_get_state, _reset and _destroy
 * after sdrfm_synchronize(h) (the launches hold pointers into the sink).  The wait on the device is bounded (2^19 polls: about a second): should it ever run out — a protocol error —
 * the run goes on from state 0 and sdrfm_pcm_sink_synchronize / _get_state answer SDRFM_FAIL from then on (until _reset).
 * kernel name: "... + pcm". */
int  sdrfm_process_batch_pcm(sdrfm_t* h, sdrfm_pcm_sink_t* sink, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* audio, size_t audio_stride,
                             int16_t* pcm, size_t pcm_stride, uint32_t* n_audio, uint32_t flags);

/* The STEREO sink on the device, for the L and R rows sdrfm_stereo_process_batch and sdrfm_bcast_process_batch leave:
 * left[stream * audio_stride + i], right[stream * audio_stride + i] (f32) -> pcm[stream * pcm_stride + 2*i] = L, [... + 2*i + 1] = R (int16), each channel
 * de-emphasised on its own with the operations of sdrfm_pcm_deemph_s16 in its order — what sdrfm_pcm_deemph_stereo_s16 does for one stream on the host.
 * The two de-emphasis states of a stream are carried in the handle.  The contract is sdrfm_pcm_sink_*'s:
 *   create   alpha outside (0, 1], a NaN gain, n_streams == 0 or out == NULL: SDRFM_EINVAL before any device is looked for; a missing or non-gfx950
 *            device: SDRFM_NO_DEVICE.
 *   process_batch   flags is a subset of SDRFM_F_DEVICE_PTRS | SDRFM_PCM_F_EXACT (else SDRFM_EINVAL); n == 0 is a no-op; left, right or pcm NULL with
 *            n > 0: SDRFM_EINVAL; with more than one stream audio_stride < n or pcm_stride < 2*n: SDRFM_ECAPACITY; pcm_stride (int16 elements) odd:
 *            SDRFM_EINVAL.  With SDRFM_F_DEVICE_PTRS the three buffers are device memory, pcm 4-byte aligned (else SDRFM_EINVAL), and the call only
 *            enqueues on the sink's stream; give it the demodulator's stream (or synchronise) so that it runs after the audio exists.  With host
 *            buffers the call stages, runs and copies back, and is synchronous.
 *   NULL handles answer SDRFM_EINVAL (destroy: nothing).
 * Two forms of the same recursion (csrc/sdrfm_sink_stereo.hip), both chains of a stream walked by the same lane:
 *   default            the blocked scan of sdrfm_pcm_sink_process_batch, per channel operation for operation: the even PCM slots are bit for bit what that
 *                      sink's default form leaves for the L rows, the odd slots what it leaves for the R rows; PCM within 1 LSB of the exact form's,
 *                      carried states within 1e-6 relative;
 *   SDRFM_PCM_F_EXACT  one lane per stream: BIT-IDENTICAL to sdrfm_pcm_deemph_stereo_s16, PCM and both states.
 * Unlike sdrfm_pcm_sink_t this sink takes no part in a demodulator's launch: its state is a plain float[n_streams][2] which a call reads at its start and
 * writes at its end, and calls are ordered by the HIP stream they are enqueued on — keep all calls on one sink on one stream, or synchronise between them.
 * sdrfm_pcm_stereo_sink_get_state synchronises the SINK's stream and copies the states: state_out[2s] = L, state_out[2s + 1] = R. */
typedef struct sdrfm_pcm_stereo_sink sdrfm_pcm_stereo_sink_t;
int  sdrfm_pcm_stereo_sink_create(uint32_t n_streams, float alpha, float gain, int32_t device, sdrfm_pcm_stereo_sink_t** out);
void sdrfm_pcm_stereo_sink_destroy(sdrfm_pcm_stereo_sink_t* k);
int  sdrfm_pcm_stereo_sink_reset(sdrfm_pcm_stereo_sink_t* k);
int  sdrfm_pcm_stereo_sink_process_batch(sdrfm_pcm_stereo_sink_t* k, const float* left, const float* right, size_t audio_stride, uint32_t n,
                                         int16_t* pcm, size_t pcm_stride, uint32_t flags);
int  sdrfm_pcm_stereo_sink_set_stream(sdrfm_pcm_stereo_sink_t* k, void* hip_stream);
int  sdrfm_pcm_stereo_sink_synchronize(sdrfm_pcm_stereo_sink_t* k);
int  sdrfm_pcm_stereo_sink_get_state(sdrfm_pcm_stereo_sink_t* k, float* state_out /* 2 * n_streams floats: [2s] = L, [2s+1] = R */);

/* ONE call from IQ bytes to playable stereo PCM: sdrfm_stereo_process_batch (sdrfm_bcast_process_batch) exactly as it stands — the same kernel with the
 * same arguments, so left, right, bb and pilot_count come out with the same bits — followed ON THE HANDLE'S STREAM by the stereo sink's default form over
 * this call's L and R rows into pcm.  Not fused: a second launch on the same queue costs microseconds beside a call of hundreds.
 * left and right may BOTH be NULL: the sink then reads the handle's own rows and the PCM is all the audio the call returns; only one of them NULL is
 * SDRFM_EINVAL.  The sink must belong to the handle's device and have its n_streams (else SDRFM_EINVAL).  pcm is checked as by
 * sdrfm_pcm_stereo_sink_process_batch against this call's n_audio (NULL only when that is 0); every other argument as by the handle's own call.  With
 * SDRFM_F_DEVICE_PTRS every buffer is device memory and the call only enqueues; with host buffers the PCM is copied back beside the rest and the call is
 * synchronous.  Every check is made before anything is enqueued: a refused call leaves the handle and the sink as they were.
 * These calls launch the sink — and behind it the audio, loudness and true-peak meter kernels of a sink that has them enabled — on the HANDLE's stream
 * and ignore sdrfm_pcm_stereo_sink_set_stream, while every control call of the sink waits for, and enqueues on, the SINK's stream.  Two arrangements
 * are in order.  Either both are given the SAME caller's stream (sdrfm_*_set_stream on the handle and sdrfm_pcm_stereo_sink_set_stream on the sink):
 * the sink's stream is then the one the launches are on, and every control call waits or enqueues as its own paragraph says, with calls pending.
 * Or the sink's control calls are made only after the handle's _synchronize.  That holds for EVERY control call of the sink, by what it does:
 *   read      _get_state, _meter_read, _truepeak_read (host or device out), _loudness_read, _loudness_get_state: else the copy is made before the
 *             launch has run;
 *   replace   _set_hicut, _meter_enable (the threshold), sdrfm_pcm_stereo_sink_process_batch on the same sink: else records and states that a
 *             pending launch still reads are replaced under it;
 *   zero      _reset, _meter_enable on an enabled sink, a _meter_read or _truepeak_read with SDRFM_AMETER_F_RESET: else the zeroes land in front
 *             of the launch and the launch's sums stay in the records;
 *   free      _meter_disable, _loudness_enable on an enabled sink, _loudness_disable, _truepeak_enable on an enabled sink, _truepeak_disable,
 *             _destroy: else memory a pending launch uses is freed.
 * _get_hicut and the sink's other answers from host memory touch no device and may be called at any time.  tests/test_stream_order_front_gpu.py
 * holds the first arrangement with a call pending. */
int  sdrfm_stereo_process_batch_pcm(sdrfm_stereo_t* h, sdrfm_pcm_stereo_sink_t* sink, const uint8_t* iq, size_t iq_stride, uint32_t nbytes,
                                    float* left, float* right, size_t audio_stride, int16_t* pcm, size_t pcm_stride,
                                    uint32_t* pilot_count, uint32_t* n_audio, uint32_t flags);
int  sdrfm_bcast_process_batch_pcm(sdrfm_bcast_t* h, sdrfm_pcm_stereo_sink_t* sink, const uint8_t* iq, size_t iq_stride, uint32_t nbytes,
                                   float* left, float* right, size_t audio_stride, int16_t* pcm, size_t pcm_stride,
                                   float* bb, size_t bb_stride, uint32_t* pilot_count, uint32_t* n_audio, uint32_t* n_rds, uint32_t flags);

/* The METERED broadcast call: either broadcast call above and, from the same launch, one sdrfm_scan_meter per stream —
 * level, tuning error, deviation and pilot quality of what the stream is receiving, so that a running receiver follows a drifting
 * crystal or a fading station without a second handle that walks the front end again.
 * The records are the scan section's, term for term, on this handle's own y, d and q: the 64 bytes per stream equal what a scan handle
 * gives for the same bytes, channel taps (an untuned handle: ctaps = (h[k], 0), rot = 0), pilot taps and pilot_min, in every field and
 * for any cut into calls; they add up with sdrfm_scan_meter_add and read with sdrfm_scan_report.  n is the call's new d's, n_pilot equals
 * pilot_count.  The call changes NO bit of left, right, bb, pcm, pilot_count, the counts or the carried state: metered and plain calls
 * mix freely in one sequence.
 *   sink == NULL   the contract of sdrfm_bcast_process_batch; pcm must then be NULL (SDRFM_EINVAL).
 *   sink != NULL   the contract of sdrfm_bcast_process_batch_pcm, left = right = NULL included.
 *   meters         n_streams records, never NULL (SDRFM_EINVAL).  Host memory for a host-buffer call; with SDRFM_F_DEVICE_PTRS device
 *                  memory; 8-byte aligned either way (else SDRFM_EINVAL).  OVERWRITTEN: zeroed on the handle's stream before the launch adds to it; nbytes == 0 gives
 *                  zero records; reserved stays 0.
 * The record's int64 bounds are the scan section's.  SDRFM_EINVAL for a handle whose CURRENT channel taps — sdrfm_bcast_tune's, or the
 * configuration's h on an untuned handle — have sum(|hr[k]| + |hi[k]|) > 16 for some stream, or whose pilot taps have
 * sum(|br[k]| + |bi[k]|) > 8 (looked at at create and at tune, not per call; the plain calls take such a handle as before);
 * SDRFM_ECAPACITY for nbytes > 4 MiB whatever max_bytes_per_call is.
 * These three refusals of the metered call's own come first (NULL handle, meters or counts; pcm without sink; the tap sums); every other
 * check is the chosen form's, in its order, the 4 MiB bound beside max_bytes_per_call's.  All of them before anything is enqueued: a
 * refused call leaves the handle and the sink as they were.
 * The kernel name does not change: sdrfm_bcast_kernel_name names the handle's kernel, and a metered call launches that kernel's
 * metered form. */
int  sdrfm_bcast_process_batch_metered(sdrfm_bcast_t* h, sdrfm_pcm_stereo_sink_t* sink /* or NULL */, const uint8_t* iq, size_t iq_stride,
                                       uint32_t nbytes, float* left, float* right, size_t audio_stride, int16_t* pcm, size_t pcm_stride,
                                       float* bb, size_t bb_stride, uint32_t* pilot_count, sdrfm_scan_meter* meters, uint32_t* n_audio,
                                       uint32_t* n_rds, uint32_t flags);

/* The HIST broadcast call: the metered call above and, from the same launch, the scan section's deviation histogram of
 * every stream — so that a running receiver monitors the modulation of the stations it plays (sdrfm_scan_hist_report, ITU-R SM.1268 /
 * BS.412) without a scan handle that walks the same bytes again.
 * Row s counts the call's new d's of stream s — the d's the record's n counts — by bin = floor(dq / 2^18) + 256 of
 * dq = (int32) rintf(d 2^24), the integer the record's freq_q sums.  It EQUALS, integer for integer, the row sdrfm_scan_process_batch_hist
 * gives on a scan handle with the same channel taps (an untuned handle: ctaps = (h[k], 0), rot = 0), pilot taps and pilot_min for the same
 * bytes, for any cut into calls, and depends on nothing else: not on the kernel form, the blend or gain, or a sink.  With the record of
 * the same call: sum_b hist[b] = n, and sum_b hist[b] (b - 256) 2^18 <= freq_q < sum_b hist[b] (b - 255) 2^18 for n > 0.
 *   hist          n_streams rows of hist_stride uint32 words, hist_stride >= SDRFM_SCAN_HIST_BINS.  Host memory for a host-buffer call; with
 *                 SDRFM_F_DEVICE_PTRS device memory, 4-byte aligned (else SDRFM_EINVAL).  The first SDRFM_SCAN_HIST_BINS words of every row
 *                 are OVERWRITTEN (zeroed on the handle's stream before the launch adds to them); words behind them are left alone;
 *                 nbytes == 0 gives zero rows.  Rows add up with sdrfm_scan_hist_add and read with sdrfm_scan_hist_report.
 * NULL h, meters or hist, or hist_stride < SDRFM_SCAN_HIST_BINS: SDRFM_EINVAL, before anything else is looked at.  Every other refusal is
 * the metered call's, in its order; a refused call writes nothing and leaves the handle and the sink as they were.
 * Every other output — left, right, bb, pcm, pilot_count, meters, the counts, the carried state — is the metered call's bit for bit:
 * plain, PCM, metered and hist calls mix freely in one sequence.  The device rows behind host hist calls (n_streams x 2048 bytes) are
 * allocated at the first one (SDRFM_ENOMEM if that fails): a handle that never makes a hist call allocates and launches what it did.
 * A hist call launches the hist form of the handle's kernel, which sdrfm_bcast_hist_kernel_name names: sdrfm_bcast_kernel_name's string
 * and " + hist".  Its bins take 2 KiB of the workgroup's local memory, so at shapes where that memory bounds the step its step is a few
 * d's shorter than the other calls' (and generic where only the plain form fits the fast kernel's step); no result depends on the step. */
int  sdrfm_bcast_process_batch_metered_hist(sdrfm_bcast_t* h, sdrfm_pcm_stereo_sink_t* sink /* or NULL */, const uint8_t* iq, size_t iq_stride,
                                            uint32_t nbytes, float* left, float* right, size_t audio_stride, int16_t* pcm, size_t pcm_stride,
                                            float* bb, size_t bb_stride, uint32_t* pilot_count, sdrfm_scan_meter* meters, uint32_t* hist,
                                            size_t hist_stride, uint32_t* n_audio, uint32_t* n_rds, uint32_t flags);
const char* sdrfm_bcast_hist_kernel_name(const sdrfm_bcast_t* h);

/* RE-TUNING a running broadcast receiver: new channel taps and rotations between two calls, the streams kept running.
 * sdrfm_bcast_tune is a restart of every stream; this call is what a drift correction, or the replacement of one station among many, uses.
 *
 * The re-tune takes effect between two calls, on the handle's stream: every call enqueued before it runs with the old tuning and every
 * call after it with the new one.  It WAITS for the handle's stream, as sdrfm_bcast_tune does, before it replaces the taps; the transform
 * of the carried state is then enqueued on that stream and the call returns.  It copies all four arrays before it returns.
 * It changes neither the input phase, nor the audio and RDS decimator phases, nor hist_x (the raw input history), nor any sink.
 *
 * Let rot_old[s] be the stream's current rotation, 0 on an untuned handle.  An untuned handle may be re-tuned; it becomes a tuned one.
 * The carried state has the same three kinds in both forms (the tuning section above).  Per stream:
 *   restart[s] != 0   the stream's hist_x, yprev and hist_d become 0, and nothing else changes.  This is the definition's stream whose
 *                     earlier x were all 0.0f: y = 0 gives d = 0, which K3 already defines.  The phases stay where they are, because they
 *                     belong to the handle.
 *   restart[s] == 0   all fp32, each operation rounded on its own except the fmaf's:
 *     yprev    if (cr, ci) is bitwise (1.0f, +0.0f), it is untouched.  Otherwise
 *                  t = yi*ci;  yr' = fmaf(yr, cr, -t);  u = yi*cr;  yi' = fmaf(yr, ci, u).
 *     hist_d   sh = rot_old - rot_new, then the tuning section's single wrap: sh -= 2 pi if sh > pi, else sh += 2 pi if sh < -pi, with
 *              that section's two constants.  If sh == 0.0f, hist_d is untouched.  Otherwise hist_d[i] = hist_d[i] + sh for all H
 *              entries.  The entries may then lie outside [-pi, pi]; they are history for FIR chains only.
 *     The two "untouched" rules are part of the definition.  They make the identity re-tune an exact no-op, signs of zero included.
 *     The transform is mechanical.  A re-tune before a stream's first d shifts the zeros of its hist_d; for that case use
 *     sdrfm_bcast_tune or restart[s] = 1.
 * Two re-tunes with no call between them compose: the carry is applied twice and the shifts add.
 * sdrfm_bcast_reset keeps the new tuning.  Whether the metered call takes the handle is decided again, as sdrfm_bcast_tune decides it.
 *
 * From the re-tune on, y[m] of a kept stream is bit for bit y[m] of a stream that had the new taps all along (hist_x holds raw x and the
 * tuned y carries no oscillator phase), so d[m] is from the second d on, and L, R and bb are once their windows have passed the switch.
 *
 * The intended values, evaluated in float64 and rounded once as everywhere in this library (the library computes no trigonometry):
 * ctaps and rot as sdrfm_bcast_tune's for the new offsets, and
 *     carry = exp(+j 2 pi (f_new - f_old) (T - 1) / 2 / fs)
 * — the phase by which the moved low-pass's y differs for a signal inside both passbands, for a symmetric h under the tuning section's
 * convention (tap k multiplies x[n - k]).  carry == NULL is (1, 0) everywhere; restart == NULL keeps every stream.
 *
 * SDRFM_EINVAL, with nothing changed and nothing enqueued: NULL handle, ctaps or rot (un-tuning stays sdrfm_bcast_tune's job);
 * non-finite ctaps, rot or carry; |rot| > pi; unknown flags; a restart byte above 1.
 * flags: SDRFM_TUNE_SHARED_INPUT or 0, as sdrfm_bcast_tune's — the setting is replaced, not kept. */
int  sdrfm_bcast_retune(sdrfm_bcast_t* h, const float* ctaps /* n_streams x 2T */, const float* rot /* n_streams */,
                        const float* carry /* n_streams x 2 (cr, ci), or NULL */, const uint8_t* restart /* n_streams, or NULL */,
                        uint32_t flags);

/* CONDITIONING the audio of a running broadcast receiver: a per-stream stereo blend and a per-stream output gain, applied
 * inside the handle's own launch where L and R are formed, both ramped per audio output so that a change never clicks.  The host sets them
 * from what the metered call's records say: blend a weak stereo station towards mono, mute a stream whose station has gone.
 *
 * State.  Per stream two integers in [0, 32768] (Q15, 32768 = 1.0): the blend b and the gain v, each with a target bt, vt; one handle-wide
 * slew in 1 .. 32768, the units either moves per audio output.  A handle is created with b = bt = v = vt = 32768.
 *
 * Ramp.  With b0 the blend at the last sdrfm_bcast_set_audio and J the audio outputs of the calls since then, output j (0-based) of the
 * next call uses
 *     k    = min(J + j + 1, cdiv(|bt - b0|, slew))
 *     b[j] = b0 + sgn(bt - b0) * min(k * slew, |bt - b0|)
 * — "move towards the target by at most slew per output" in closed form, in integers (k * slew < 65536), and so the same for any cut of a
 * capture into calls; v[j] likewise.  The ramp is evaluated from these values, not from carried device state.
 *
 * Audio.  With am and as exactly the two chains' results of the stereo section (sum and difference channel of output j), all fp32:
 *     beta = (float)b[j] * 2^-15,  mu = (float)v[j] * 2^-15        (exact)
 *     t = beta * as                                                (one rounding; never contracted into the sums below)
 *     L[j] = mu * (am + t),   R[j] = mu * (am - t)                 (each sum and each product rounded once)
 * beta = mu = 1 gives the plain kernels' bits; beta = 0 gives L == R == mu * am; a power-of-two beta is a plain handle whose diff_gain is
 * scaled by it; a power-of-two mu scales L and R exactly.  bb, pilot_count, the metered call's records, both decimator phases and all
 * carried state are untouched.  Every plain, PCM and metered call form works on a conditioned handle: the PCM forms sink the conditioned
 * L and R.
 *
 * sdrfm_bcast_set_audio WAITS for the handle's stream, as sdrfm_bcast_tune does; it moves b0, v0 to the values the ramps have reached,
 * takes the new targets (a NULL array keeps that kind's targets) and the new slew, sets J = 0 and takes effect with the next call.  From
 * then on the handle launches the blended forms of its kernels and sdrfm_bcast_kernel_name ends in " blend".  A slew of 32768 is a jump:
 * the next output is at its target.  sdrfm_bcast_set_audio(h, NULL, NULL, 0) returns the handle to the plain kernels, their name and their
 * bits: b = bt = v = vt = 32768.
 * sdrfm_bcast_reset and sdrfm_bcast_tune keep the settings and complete the ramps (b = bt, v = vt); sdrfm_bcast_retune leaves them running.
 * SDRFM_EINVAL, with nothing changed and before the device is touched: a NULL handle; a value above 32768; a slew of 0 with a non-NULL
 * array; a slew above 32768.
 *
 * sdrfm_bcast_get_audio gives, per stream, the values the next output starts from (b and v after the J outputs so far) and the targets;
 * each array holds n_streams entries and any may be NULL.  It touches no device. */
int  sdrfm_bcast_set_audio(sdrfm_bcast_t* h, const uint16_t* blend_q15 /* n_streams, or NULL: targets kept */,
                           const uint16_t* gain_q15 /* n_streams, or NULL: targets kept */, uint32_t slew_q15);
int  sdrfm_bcast_get_audio(const sdrfm_bcast_t* h, uint16_t* blend_q15, uint16_t* gain_q15, uint16_t* blend_target_q15,
                           uint16_t* gain_target_q15 /* any may be NULL */);

/* A per-stream, ramped HIGH-CUT in the stereo PCM sink: the step after the blend.  Once the blend has reached mono a weakening
 * station keeps losing audio SNR; a broadcast tuner then lengthens the de-emphasis time constant, which trades treble for hiss.  Here that is one
 * integer per stream that scales the sink's alpha, ramped per audio sample so that a change never clicks.
 *
 * State.  Per stream one Q15 integer h in [SDRFM_HICUT_MIN, 32768] with a target ht; one sink-wide slew in 1 .. 32768, the units h moves per audio
 * sample.  A sink is created with h = ht = 32768 and is then NOT conditioned: it launches the plain kernels.
 *
 * Definition.  With h0 the value at the last sdrfm_pcm_stereo_sink_set_hicut and J the samples the sink has taken since (saturating at 65536), sample
 * i (0-based) of the next call uses, all fp32,
 *     h[i]     = the ramp of sdrfm_bcast_set_audio: h0 moved towards ht by min(min(J + i + 1, 65536) * slew, |ht - h0|)
 *     alpha[i] = alpha * ((float)h[i] * 2^-15)        the inner product exact, the outer one rounded once, never contracted
 *     y[i]     = fmaf(alpha[i], x[i] - y[i-1], y[i-1])
 *     pcm[i]   = (int16) lrintf(clamp(y[i] * gain, -32768, 32767))
 * L and R of a stream use the same alpha[i]; each carries its own y.  The ramp is a function of values (h0, ht, slew, J), not of carried device
 * state: any cut of the samples into calls gives the same coefficients.  h = 32768 gives alpha * 1.0f == alpha: the plain recursion bit for bit.
 * The -3 dB corner of a settled stream is -ln(1 - alpha h / 32768) fs / (2 pi): at 75 us and 48 kHz 2122 Hz at h = 32768, about 480 Hz at h = 8192.
 *
 * sdrfm_pcm_deemph_stereo_hicut_s16 is the definition in plain C for one stream, and the reference of everything below.  SDRFM_EINVAL for what
 * sdrfm_pcm_deemph_stereo_s16 refuses, for h0 or ht outside [SDRFM_HICUT_MIN, 32768] and for a slew outside 1 .. 32768.  J above 65536 is 65536.
 *
 * sdrfm_pcm_stereo_sink_set_hicut WAITS for the sink's stream; it moves every h0 to the value its ramp has reached, takes the new targets (NULL:
 * the targets are kept) and the slew, sets J = 0 and takes effect with the next call.  From then on the sink is conditioned and every call form
 * launches the conditioned kernels: sdrfm_pcm_stereo_sink_process_batch in both forms, and the sink's launch behind sdrfm_stereo_process_batch_pcm,
 * sdrfm_bcast_process_batch_pcm and sdrfm_bcast_process_batch_metered.  J advances by n with every call that sinks n samples.  A slew of 32768 is a
 * jump.  (k, NULL, 0) returns the sink to the plain kernels and their bits: h = ht = 32768.  sdrfm_pcm_stereo_sink_reset keeps the settings and
 * completes the ramps (h = ht).
 * SDRFM_EINVAL, with nothing changed and before a device is touched: a NULL sink; a value outside [SDRFM_HICUT_MIN, 32768]; a slew of 0 with a
 * non-NULL array; a slew above 32768; and, for a slew other than 0, a sink whose alpha * 0.03125f < 0.001f — the smallest effective coefficient
 * then stays at or above 0.001; far below that the fp32 recursion stops being linear and no blocked scan follows it.
 *
 * Two forms, as for the plain sink (csrc/sdrfm_sink_hicut.h):
 *   SDRFM_PCM_F_EXACT  one lane per stream, the coefficient taken per sample: BIT-IDENTICAL to sdrfm_pcm_deemph_stereo_hicut_s16, PCM and both
 *                      states, at every alpha the set accepts.
 *   default            a blocked scan over affine maps: beside its chunk's contribution every lane carries the chunk's own decay, and the scan
 *                      combines the pairs.  PCM within 1 LSB of the exact form's, a share of differing outputs of at most 1e-3 + 2 / size, carried
 *                      states within 1e-6 max(|state|, 0.25): CLAIMED AND TESTED AT THE TWO BROADCAST ALPHAS ONLY, sdrfm_pcm_alpha(48 kHz, 50 us)
 *                      and (48 kHz, 75 us).  At other alphas the default form still runs and follows the exact one closely, but a prototype
 *                      at alpha = 0.05 with h = 2622 held flat left 1.55e-3 of the outputs 1 LSB off and a state 1.04e-6 off: use the exact
 *                      form there if the caps matter.
 *
 * sdrfm_pcm_stereo_sink_get_hicut gives, per stream, the value the next sample starts from and the target; *slew_q15 is 0 on a sink that is not
 * conditioned.  Any pointer may be NULL.  It touches no device.
 * Around the one-call forms, which launch on the HANDLE's stream, call set and get only after the handle's _synchronize — the rule of
 * the one-call forms at sdrfm_stereo_process_batch_pcm, which also allows them with both on one caller's stream. */
#define SDRFM_HICUT_MIN 1024u
int  sdrfm_pcm_deemph_stereo_hicut_s16(const float* left, const float* right, uint32_t n, float alpha, float gain, uint16_t h0, uint16_t ht,
                                       uint32_t slew, uint32_t J, float* state, int16_t* pcm_stereo);
int  sdrfm_pcm_stereo_sink_set_hicut(sdrfm_pcm_stereo_sink_t* k, const uint16_t* hicut_q15 /* n_streams, or NULL: targets kept */, uint32_t slew_q15);
int  sdrfm_pcm_stereo_sink_get_hicut(const sdrfm_pcm_stereo_sink_t* k, uint16_t* hicut_q15, uint16_t* target_q15, uint32_t* slew_q15);

/* A per-stream AUDIO METER on the stereo PCM sink: what the receiver plays, for the silence, dead-channel, anti-phase and
 * clipping alarms.  One integer record per stream, defined on the int16 stereo PCM rows the sink wrote — pcm[2i] = L, pcm[2i + 1] = R, i < n —
 * and on nothing else.  The input is int16, so every field is an exact integer and there is no rounding rule.
 *
 * Definition.  n counts sample pairs; sum_l, sum_r, sq_l, sq_r and cross are the sums of L, R, L^2, R^2 and L R; peak_* is the largest |x|
 * (0 .. 32768); clip_* counts the samples equal to -32768 or 32767.  The three sdrfm_audio_runs describe the predicates |L| <= quiet_lsb,
 * |R| <= quiet_lsb and both at once over the n pairs in their order: count = the pairs that satisfy it, lead = the length of the longest
 * prefix that satisfies it throughout, trail = that of the longest such suffix, longest = the longest run of consecutive pairs that satisfy
 * it.  A silence alarm needs the runs and not the count: programme audio passes through zero all the time.  All four are 0 for n = 0.
 *
 * The JOIN of a record a and the record b of the pairs that FOLLOW, sdrfm_audio_meter_add(acc = a, m = b): n, the sums, the rail counts and
 * every runs' count add, the peaks take the maximum, and per predicate
 *     lead    = a.lead + (a.lead == a.n ? b.lead : 0)
 *     trail   = b.trail + (b.trail == b.n ? a.trail : 0)
 *     longest = max(a.longest, b.longest, a.trail + b.lead)
 * The zero record is the identity on either side.  THE JOIN IS ASSOCIATIVE AND NOT COMMUTATIVE: acc comes before m.  Any cut of the pairs
 * into pieces joined in their order gives the same record — which is how the device computes it and how reads are accumulated.
 * EVERY FIELD IS EXACT WHILE THE ACCUMULATED n <= 2^32 (24.8 h at 48 kHz: sq <= 2^32 2^30 and |cross| <= 2^62).  Beyond that the unsigned
 * fields wrap and the signed ones are computed in unsigned arithmetic: nothing is undefined behaviour, and nothing is claimed.
 *
 * Host side, plain C with no GPU behind it (csrc/audio_meter.c):
 *   sdrfm_pcm_audio_meter_s16   joins the record of these n pairs onto *acc: the definition as code, and the routine a board-side host uses.
 *                               SDRFM_EINVAL for acc NULL, pcm_interleaved NULL with n > 0, quiet_lsb > 32767.
 *   sdrfm_audio_meter_add       the ordered join above; SDRFM_EINVAL for a NULL pointer.
 *   sdrfm_audio_meter_report    the record in physical units, computed in double.  *_dbfs are 20 log10(x / 32768), -inf for zero power; dc_*
 *                               are the means in LSB; rail_* and quiet_* are shares of n; longest_*_s and trail_*_s are seconds at fs_audio;
 *                               correlation = cross / sqrt(sq_l sq_r), NaN when a channel has no power; mid and side are the powers of
 *                               (L + R) / 2 and (L - R) / 2, (sq_l + sq_r +- 2 cross) / 4 / n, in dBFS, side_mid_db their ratio (NaN when
 *                               both are zero).  n = 0: every field NaN.  SDRFM_EINVAL for a NULL pointer or an fs_audio that is not
 *                               finite and positive.
 *
 * On the sink (csrc/sdrfm_sink_stereo.hip, the kernel's body in csrc/sdrfm_audio_meter.h).  A sink is created without a meter and then
 * allocates and launches exactly what it did before.
 *   _meter_enable   quiet_lsb > 32767 or a NULL sink: SDRFM_EINVAL before any device work.  Allocates n_streams records on the device
 *                   (SDRFM_ENOMEM), zeroed.  Enabling an enabled sink waits for the sink's stream, zeroes the records and takes the new threshold.
 *   _meter_disable  waits for the sink's stream and stops the metering; the records are gone.
 *   _meter_read     flags is a subset of SDRFM_F_DEVICE_PTRS | SDRFM_AMETER_F_RESET, out is 8-byte aligned and holds n_streams records, the sink
 *                   is enabled: else SDRFM_EINVAL.  Host out: synchronises the sink's stream, copies and, with SDRFM_AMETER_F_RESET, zeroes the
 *                   records.  Device out: the copy, and the zeroing, are enqueued on the sink's stream and nowhere else.
 *   sdrfm_pcm_stereo_sink_reset also zeroes the records of an enabled sink.
 * While enabled, EVERY launch of the sink — the default, exact, high-cut default and high-cut exact forms; sdrfm_pcm_stereo_sink_process_batch
 * and the sink's launch behind sdrfm_stereo_process_batch_pcm, sdrfm_bcast_process_batch_pcm, sdrfm_bcast_process_batch_metered and
 * sdrfm_bcast_process_batch_metered_hist; host and device buffers — is followed on the same stream by one launch of the meter kernel, which reads
 * the PCM rows just written and joins the call's record onto each stream's.  The sink kernels are the same kernels with the same arguments:
 * PCM, states and high-cut ramps keep their bits.  What lies in a row behind 2n is the caller's: it is neither read nor written.
 * Around the one-call forms, which launch on the HANDLE's stream, call enable, disable and read only after the handle's _synchronize — the
 * rule of the one-call forms at sdrfm_stereo_process_batch_pcm, which also allows them with both on one caller's stream. */
typedef struct sdrfm_audio_runs { uint64_t count, lead, trail, longest; } sdrfm_audio_runs;   /* 32 bytes */
typedef struct sdrfm_audio_meter {                 /* 192 bytes, 8-byte aligned */
  uint64_t n;                                       /* sample pairs */
  int64_t  sum_l, sum_r;                            /* sum L, sum R */
  uint64_t sq_l, sq_r;                              /* sum L^2, sum R^2 */
  int64_t  cross;                                   /* sum L R */
  uint32_t peak_l, peak_r;                          /* max |x|, 0 .. 32768 */
  uint64_t clip_l, clip_r;                          /* samples equal to -32768 or 32767 */
  sdrfm_audio_runs quiet_l, quiet_r, quiet_both;    /* predicate |x| <= quiet_lsb on L, on R, on both */
  uint64_t reserved[3];                             /* 0 */
} sdrfm_audio_meter;
typedef struct sdrfm_audio_report_t {
  double rms_l_dbfs, rms_r_dbfs, peak_l_dbfs, peak_r_dbfs, dc_l, dc_r, rail_l, rail_r;
  double quiet_l, quiet_r, quiet_both;
  double longest_l_s, longest_r_s, longest_both_s, trail_l_s, trail_r_s, trail_both_s;
  double correlation, mid_dbfs, side_dbfs, side_mid_db;
} sdrfm_audio_report_t;
#define SDRFM_AMETER_F_RESET 8u   /* flag for sdrfm_pcm_stereo_sink_meter_read (beside SDRFM_F_DEVICE_PTRS): zero the records behind the copy */
int  sdrfm_pcm_audio_meter_s16(const int16_t* pcm_interleaved, uint32_t n, uint32_t quiet_lsb, sdrfm_audio_meter* acc);
int  sdrfm_audio_meter_add(sdrfm_audio_meter* acc, const sdrfm_audio_meter* m);
int  sdrfm_audio_meter_report(const sdrfm_audio_meter* m, double fs_audio, sdrfm_audio_report_t* out);
int  sdrfm_pcm_stereo_sink_meter_enable(sdrfm_pcm_stereo_sink_t* k, uint32_t quiet_lsb);
int  sdrfm_pcm_stereo_sink_meter_disable(sdrfm_pcm_stereo_sink_t* k);
int  sdrfm_pcm_stereo_sink_meter_read(sdrfm_pcm_stereo_sink_t* k, sdrfm_audio_meter* out /* n_streams records */, uint32_t flags);

/* A per-stream PCM RATE MATCHER behind the sinks: the int16 stereo rows either PCM sink leaves, at the DONGLE's 48 kHz, resampled
 * per stream by an arbitrary ratio — a few ppm to lock onto the consumer's clock, or 48/44.1 — on the device.  All arithmetic is integer and
 * exact: the device and the host routine agree bit for bit, and any cut of a stream into calls gives the same outputs.
 *
 * Rows.  in[s * in_stride + 2i] = L, [... + 2i + 1] = R, i < n: what both sinks write (the mono sink's L = R rows as well); out likewise.
 * Per-stream state.  step, 32.32 fixed point: input pairs per output pair, 2^30 <= step <= 2^34, 2^32 after create.  pos, 32.32, measured against
 * the call's first new pair, and hist, the last n_taps - 1 input pairs: both 0 after create and reset.
 * Table, given at create: coef[(NPH + 1)][n_taps] int16 in Q15, NPH = 2^log2_phases, 4 <= log2_phases <= 8, n_taps a multiple of 4 in 4 .. 64.
 * Row p serves the fraction p / NPH; row NPH is there so that the interpolation never wraps.  A table is taken only if in every row the sum of
 * |coef| over the taps [0, n_taps / 2) is <= 65535 and likewise over [n_taps / 2, n_taps) (sdrfm_pcm_rate_check_coef): a half-row dot product
 * with any int16 input then fits an int32, which is what lets the kernel use 32-bit packed dot products and stay exact.
 *
 * One call of n <= 2^20 pairs, x[i] the new pairs for i >= 0 and hist for i < 0:
 *     cnt  = pos >= n 2^32 ? 0 : ceil((n 2^32 - pos) / step)
 *     for j < cnt:  P = pos + j step,  i = P >> 32,  f = P & 0xffffffff,  p = f >> (32 - log2_phases),  mu = (f >> (24 - log2_phases)) & 255
 *         per channel  A0 = sum_k coef[p][k] x[i - n_taps + 1 + k],  A1 the same with row p + 1
 *         y[j] = sat16((A0 (256 - mu) + A1 mu + 2^22) >> 23)         64-bit, arithmetic shift
 *     pos <- pos + cnt step - n 2^32;  hist <- the last n_taps - 1 pairs of (hist, the n new pairs), also for n < n_taps - 1
 * A new step takes effect at the next call's first output.  Output j sits at input time (i - n_taps / 2) + f / 2^32: the latency is n_taps / 2
 * input pairs.
 *
 * Host side, plain C with no GPU behind it (csrc/pcm_rate.c):
 *   sdrfm_pcm_rate_s16         one stream's call, the definition as code; the caller carries *pos and hist (2 (n_taps - 1) int16, zero at the start).
 *                              SDRFM_EINVAL: coef, pos, hist or n_out NULL, in NULL with n > 0, out NULL with outputs to write, a table shape, a
 *                              step or an n outside the ranges above.  SDRFM_ECAPACITY: the call yields more than out_cap_pairs — nothing is
 *                              written and *pos and hist stay.  It accumulates in 64 bits and so does not ask for the half-row bound.
 *   sdrfm_pcm_rate_check_coef  SDRFM_OK for a table the device takes, SDRFM_EINVAL otherwise.
 *
 * The handle follows sdrfm_pcm_stereo_sink_*'s contract:
 *   create    config or out NULL, n_streams == 0, flags != 0, a table shape outside the ranges or a table over the bound: SDRFM_EINVAL before any
 *             device is looked for; a missing or non-gfx950 device: SDRFM_NO_DEVICE.  The table is copied.
 *   set_step  one step per stream; any outside [2^30, 2^34]: SDRFM_EINVAL and every step stays.  Waits for the handle's stream.
 *   count     what the NEXT call of n pairs yields: n_out[s] per stream (or NULL) and *max_out, their maximum (or NULL); n > 2^20: SDRFM_EINVAL.
 *   process_batch   Every refusal is made before anything is enqueued and leaves the handle as it was: flags outside SDRFM_F_DEVICE_PTRS, n > 2^20,
 *             an odd in_stride or out_stride (int16 elements): SDRFM_EINVAL; then n == 0 is a no-op; then in or out NULL, or device rows that are
 *             not 4-byte aligned: SDRFM_EINVAL; with more than one stream in_stride < 2n or out_stride < 2 max cnt: SDRFM_ECAPACITY.  n_out (host
 *             memory, n_streams, or NULL) is filled at return even when the call only enqueues: cnt and pos are closed forms of (pos, step, n)
 *             and the handle keeps a host mirror of them.  Exactly 2 cnt[s] int16 are written per row; what lies behind them is the caller's.
 *             With SDRFM_F_DEVICE_PTRS the rows are device memory and the call only enqueues on the handle's stream: give it the sink's or the
 *             demodulator's stream (or synchronise) so that it runs after the PCM exists.  With host buffers the call stages, runs, copies back and
 *             is synchronous.
 *   get_state synchronises the handle's stream and gives the steps and the DEVICE's pos (either may be NULL); SDRFM_FAIL should the device's pos
 *             differ from the host mirror.
 *   reset     pos and hist to 0, the steps stay.
 *   NULL handles answer SDRFM_EINVAL (destroy: nothing; kernel_name: NULL).
 * The kernel (csrc/sdrfm_pcm_rate.hip, its body and the launch geometry in csrc/sdrfm_pcm_rate.h): one workgroup per stream and span of
 * consecutive outputs, the table and the span's input window in LDS.  pos and hist live on the device in two sets; a call reads one and writes the
 * other, and calls are ordered by the HIP stream they are enqueued on.  kernel name: "pcm-rate". */
typedef struct sdrfm_pcm_rate sdrfm_pcm_rate_t;
typedef struct sdrfm_pcm_rate_config { uint32_t n_streams, n_taps, log2_phases, flags; const int16_t* coef; int32_t device; } sdrfm_pcm_rate_config;
int  sdrfm_pcm_rate_create(const sdrfm_pcm_rate_config* config, sdrfm_pcm_rate_t** out);   /* every step starts at 2^32 */
void sdrfm_pcm_rate_destroy(sdrfm_pcm_rate_t* k);
int  sdrfm_pcm_rate_reset(sdrfm_pcm_rate_t* k);                                             /* pos, hist = 0; steps kept */
int  sdrfm_pcm_rate_set_step(sdrfm_pcm_rate_t* k, const uint64_t* step /* n_streams */);
int  sdrfm_pcm_rate_count(const sdrfm_pcm_rate_t* k, uint32_t n, uint32_t* n_out /* n_streams, or NULL */, uint32_t* max_out);
int  sdrfm_pcm_rate_process_batch(sdrfm_pcm_rate_t* k, const int16_t* in, size_t in_stride, uint32_t n, int16_t* out, size_t out_stride,
                                  uint32_t* n_out /* host, n_streams, or NULL */, uint32_t flags);
int  sdrfm_pcm_rate_get_state(sdrfm_pcm_rate_t* k, uint64_t* step, uint64_t* pos);          /* synchronises; the DEVICE's pos */
int  sdrfm_pcm_rate_set_stream(sdrfm_pcm_rate_t* k, void* hip_stream);
int  sdrfm_pcm_rate_synchronize(sdrfm_pcm_rate_t* k);
const char* sdrfm_pcm_rate_kernel_name(const sdrfm_pcm_rate_t* k);
int  sdrfm_pcm_rate_s16(const int16_t* in, uint32_t n, const int16_t* coef, uint32_t n_taps, uint32_t log2_phases, uint64_t step, uint64_t* pos,
                        int16_t* hist /* 2 * (n_taps - 1) */, int16_t* out, uint32_t out_cap_pairs, uint32_t* n_out);
int  sdrfm_pcm_rate_check_coef(const int16_t* coef, uint32_t n_taps, uint32_t log2_phases);

/* A per-stream K-WEIGHTED LOUDNESS METER on the stereo PCM sink: ITU-R BS.1770-4 / EBU R 128 momentary, short-term and
 * integrated loudness in LUFS and loudness range (EBU Tech 3342) of what the receiver plays.  The device filters the int16 stereo PCM rows the
 * sink wrote and leaves sub-block energies; a small host object turns those into M, S, I and LRA.  No PCM is copied to the host.
 *
 * Coefficients.  sdrfm_loudness_coef holds 10 doubles, two biquads with a0 = 1: c[0 .. 4] = b0 b1 b2 a1 a2 of the high shelf, c[5 .. 9] those of
 * the 38 Hz high-pass.  sdrfm_loudness_default_coef fills in the 48 kHz values printed in BS.1770-4; coefficients for another rate are the
 * caller's business.  sdrfm_loudness_check_coef: SDRFM_EINVAL for NULL, a non-finite value, or poles not strictly inside the unit circle
 * (|a2| < 1 and |a1| < 1 + a2 for either biquad).  The host routine is exact by definition for every set that check accepts.
 * sdrfm_loudness_check_domain says whether the DEVICE may be enabled with a set: SDRFM_OK, or SDRFM_EINVAL for a set check_coef refuses and
 * for a stable set outside the device's domain.  The device's scan over lanes loses to rounding an amount that depends on the coefficients, and
 * no simple function of them bounds it, so the call measures: it runs the kernel's order of operations in plain C on the host against the
 * definition over the rows on which the difference peaks (DC at the rail, a full-range burst followed by silence, full-range noise; sub-blocks
 * of 64 and 4800 pairs) and writes, where rel and abs_per_sample are not NULL, the worst |d| / e over the sub-blocks whose mean square is at
 * least 1e6 LSB^2 and the worst |d| / block_len over the others.  In domain: rel <= 6.25e-11 and abs_per_sample <= 6.25e-5, a sixteenth of
 * what one lost sample of a full-range row amounts to.  The default set and the K-weighting re-derived for 32, 44.1 and 96 kHz are in; the
 * one for 192 kHz, high-pass poles within a few milliradians of z = 1 at radius 0.999 or more, poles of either biquad within a hundredth of
 * a radian of z = -1 and a shelf with poles of radius 0.99 near z = 1 are out (tests/loudness_cases.py lists the sets measured and their
 * figures).  Pure host arithmetic, some 10 ms.
 *
 * State, per stream (sdrfm_loudness_state, 88 bytes): pos, the pairs consumed since enable or reset; z[channel][4], both biquads in TRANSPOSED
 * DIRECT FORM II, z = {shelf s1, shelf s2, high-pass s1, high-pass s2}; e[channel], the running energy of the open sub-block.
 *
 * Definition, one pair after the other, x in int16 LSB units with no scaling by 32768, every product and sum rounded on its own in double:
 *     y1 = b0 x + s1;   s1 = (b1 x - a1 y1) + s2;   s2 = b2 x - a2 y1        (shelf), then the same with x = y1 and the high-pass: y2
 *     e[ch] += y2 y2;   ++pos;   when pos is a multiple of block_len: emit {e[0], e[1]} and zero e
 * Sub-block k is pairs [k block_len, (k + 1) block_len) of the stream, counted from enable or reset; its record is sdrfm_loudness_block
 * {e_l, e_r} = the sums of y_L^2 and y_R^2 of the K-weighted samples, in LSB^2.
 *
 * Host side, plain C with no GPU behind it (csrc/loudness.c):
 *   sdrfm_pcm_loudness_s16   walks n pairs as above from *state: the definition as code, and the routine a board-side host runs.  SDRFM_EINVAL:
 *                            state, coef or n_blocks NULL, pcm_interleaved NULL with n > 0, coefficients sdrfm_loudness_check_coef refuses,
 *                            block_len outside 64 .. 2^20, out_blocks NULL when the call completes a sub-block.  SDRFM_ECAPACITY: the call
 *                            completes more than out_cap sub-blocks — nothing is written and *state stays.
 *   sdrfm_loudness_gate_*    one stream's gate.  _push takes CONSECUTIVE sub-block energies.  With z[k] = (e_l + e_r) / (block_len 32768^2):
 *                            momentary loudness M = -0.691 + 10 log10 of the mean of the last 4 z, short-term S the same over the last 30 z;
 *                            a gating block is every window of 4 consecutive sub-blocks (75 % overlap, one per sub-block from the fourth on);
 *                            integrated loudness I keeps the gating blocks above the absolute gate (> -70 LUFS), then those above the relative
 *                            gate (> 10 LU below the mean of the absolute-gated), and takes the mean of z over what remains; loudness range LRA
 *                            keeps the short-term values, one per sub-block from the thirtieth on, above the absolute gate and above 20 LU below
 *                            their absolute-gated power mean, and is their 95th minus their 10th percentile.  THE COUNTS 4 AND 30 MEAN 400 ms AND
 *                            3 s ONLY WHEN block_len IS A TENTH OF A SECOND (4800 at 48 kHz).  Memory is bounded: two histograms of 0.1 LU bins
 *                            over -70 .. +10 LUFS (louder values go into the last bin) with a count and a sum of z per bin; the relative gates
 *                            are applied at bin edges — the bin that holds the gate is kept whole — and a percentile is the mean loudness of
 *                            the bin that holds the element of rank round((n - 1) p).  _report: m, s, i, lra, max_m, max_s; NaN where there are
 *                            too few sub-blocks (fewer than 4 for m, max_m and i, fewer than 30 for s, max_s and lra; lra also when no
 *                            short-term value passed the absolute gate), -inf for zero power (i: no gating block passed the gates); n_blocks
 *                            pushed, n_gating gating blocks, n_abs and n_rel of them past either gate, n_short, n_short_abs, n_short_rel
 *                            likewise for the short-term values.  create: block_len outside 64 .. 2^20 or out NULL: SDRFM_EINVAL.  push: a
 *                            NULL gate, blocks NULL with n > 0, or an energy that is negative or not finite (nothing of the push is taken):
 *                            SDRFM_EINVAL.  _reset empties it, _free releases it (NULL: nothing).
 *
 * On the sink (csrc/sdrfm_sink_stereo.hip, the kernel's body in csrc/sdrfm_loudness.h).  A sink that never enables loudness allocates and
 * launches exactly what it did before.
 *   _loudness_enable   coef NULL means the default coefficients.  A NULL sink, coefficients sdrfm_loudness_check_coef refuses, a stable set that
 *                      sdrfm_loudness_check_domain refuses, block_len outside 64 .. 2^20, cap_blocks outside 1 .. 4096: SDRFM_EINVAL before
 *                      any device work, and an enabled sink goes on as it was.  Allocates per stream the state and a ring of cap_blocks
 *                      sdrfm_loudness_block, zeroed (SDRFM_ENOMEM), and computes on the host, in long double rounded to double, the powers of
 *                      the per-channel 4 x 4 transition matrix the kernel's scan uses.  Enabling an enabled sink waits for its stream and
 *                      starts over.
 *   _loudness_disable  waits for the sink's stream, stops the metering and frees the state and the ring.
 *   _loudness_read     flags must be 0, out is host memory, first_block and n_blocks are not NULL, the sink is enabled: else SDRFM_EINVAL.
 *                      Synchronises the sink's stream and copies, per stream, the sub-blocks completed and not yet read, laid out
 *                      out[s * (*n_blocks) + j]; *first_block is the stream-global index of the first one.  More than out_cap_blocks of them:
 *                      SDRFM_ECAPACITY and nothing is consumed.  out may be NULL when there is nothing to return.
 *   _loudness_get_state  synchronises the sink's stream and copies the n_streams device states.
 *   sdrfm_pcm_stereo_sink_reset also zeroes an enabled sink's loudness states and ring; sub-block indices start at 0 again.
 * Every stream of a sink receives the same n in every call, so sub-block boundaries coincide across streams and the host mirrors pos: it knows at
 * return how many sub-blocks a call completed.  The ring keeps the newest cap_blocks; a gap shows in *first_block; a single call that completes
 * more than cap_blocks stores exactly the newest cap_blocks, each slot written once.
 * While enabled, EVERY launch of the sink — its four forms; sdrfm_pcm_stereo_sink_process_batch with host or device buffers; the sink's launch
 * behind sdrfm_stereo_process_batch_pcm, sdrfm_bcast_process_batch_pcm, sdrfm_bcast_process_batch_metered and
 * sdrfm_bcast_process_batch_metered_hist — is followed on the same stream by one launch of k_pcm_loudness over the rows just written, behind the
 * audio meter's kernel if that is enabled too.  The sink's and the meter's kernels are the same kernels with the same arguments: PCM, states,
 * high-cut ramps and audio-meter records keep their bits.  What lies in a row behind 2n is the caller's: it is neither read nor written.
 * The kernel: one workgroup of 256 lanes per stream, a tile of 4864 pairs cut into 256 chunks of 19; each chunk filtered from zero state in
 * double, a scan over lanes with the matrix powers for the true incoming states, a second pass that sums y^2, and one lane per sub-block and
 * channel adding the chunks' pieces in lane order — no atomics, so the same call sequence gives the same bits.  Its energies differ
 * from the definition's by rounding, and how much depends on the coefficients: only the sets of the domain can be enabled, for which the
 * kernel's arithmetic restated on the host stays a factor of sixteen inside 1e-9 of a loud sub-block's energy and 1e-3 LSB^2 per sample of a
 * quiet one.  What is MEASURED on the device is the default set and the in-domain sets tests/loudness_cases.py lists, each held to 8 x its
 * own figures; for other sets of the domain the predicate's margin is the only statement.  pos and the block bookkeeping
 * are exact.
 * Around the one-call forms, which launch on the HANDLE's stream, call enable, disable, read and get_state only after the handle's _synchronize
 * — the rule of the one-call forms at sdrfm_stereo_process_batch_pcm, which also allows them with both on one caller's stream. */
typedef struct sdrfm_loudness_coef { double c[10]; } sdrfm_loudness_coef;                              /* shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 */
typedef struct sdrfm_loudness_state { uint64_t pos; double z[2][4]; double e[2]; } sdrfm_loudness_state;   /* 88 bytes */
typedef struct sdrfm_loudness_block { double e_l, e_r; } sdrfm_loudness_block;                         /* 16 bytes */
typedef struct sdrfm_loudness_report_t {
  double m, s, i, lra, max_m, max_s;                                                                   /* LUFS; lra in LU */
  uint64_t n_blocks, n_gating, n_abs, n_rel, n_short, n_short_abs, n_short_rel;
} sdrfm_loudness_report_t;
typedef struct sdrfm_loudness_gate sdrfm_loudness_gate_t;
int  sdrfm_loudness_default_coef(sdrfm_loudness_coef* out);
int  sdrfm_loudness_check_coef(const sdrfm_loudness_coef* coef);
int  sdrfm_loudness_check_domain(const sdrfm_loudness_coef* coef, double* rel /* or NULL */, double* abs_per_sample /* or NULL */);
int  sdrfm_pcm_loudness_s16(const int16_t* pcm_interleaved, uint32_t n, const sdrfm_loudness_coef* coef, uint32_t block_len,
                            sdrfm_loudness_state* state, sdrfm_loudness_block* out_blocks, uint32_t out_cap, uint32_t* n_blocks);
int  sdrfm_loudness_gate_create(uint32_t block_len, sdrfm_loudness_gate_t** out);
int  sdrfm_loudness_gate_push(sdrfm_loudness_gate_t* g, const sdrfm_loudness_block* blocks, uint32_t n);
int  sdrfm_loudness_gate_report(const sdrfm_loudness_gate_t* g, sdrfm_loudness_report_t* out);
int  sdrfm_loudness_gate_reset(sdrfm_loudness_gate_t* g);
void sdrfm_loudness_gate_free(sdrfm_loudness_gate_t* g);
int  sdrfm_pcm_stereo_sink_loudness_enable(sdrfm_pcm_stereo_sink_t* k, const sdrfm_loudness_coef* coef /* or NULL */, uint32_t block_len, uint32_t cap_blocks);
int  sdrfm_pcm_stereo_sink_loudness_disable(sdrfm_pcm_stereo_sink_t* k);
int  sdrfm_pcm_stereo_sink_loudness_read(sdrfm_pcm_stereo_sink_t* k, sdrfm_loudness_block* out /* [n_streams][*n_blocks] */, uint32_t out_cap_blocks,
                                         uint64_t* first_block, uint32_t* n_blocks, uint32_t flags);
int  sdrfm_pcm_stereo_sink_loudness_get_state(sdrfm_pcm_stereo_sink_t* k, sdrfm_loudness_state* out /* n_streams */);

/* A per-stream TRUE-PEAK METER on the stereo PCM sink: the maximum true peak of ITU-R BS.1770-4 Annex 2 / EBU R 128, in
 * dBTP, of what the receiver plays — the peak of the waveform an interpolator (the rate matcher, the consumer's DAC) reconstructs from the int16
 * samples, which a sample peak can understate by several dB.  A fixed polyphase FIR on int16 with int16 taps, all-integer and EXACT: the device
 * equals the host routine bit for bit, and any cut of a stream into calls gives the same record.  No PCM is copied to the host.
 *
 * Table.  coef[P][NT] int16 in Q15, given at enable: P = n_phases is 2, 4 or 8, NT = n_taps a multiple of 4 in 4 .. 64.  A table is taken only
 * if in every row the sum of |coef| over taps [0, NT/2) is <= 65535, and likewise over [NT/2, NT) — the rate matcher's half-row bound
 * (sdrfm_truepeak_check_coef: SDRFM_EINVAL for NULL, a shape outside the ranges or a half-row over the bound): half a row's dot product with any
 * int16 input then fits an int32.  sdrfm_truepeak_default_coef gives P = 4, NT = 12, the 48 coefficients of BS.1770-4 Annex 2 (multiples of
 * 2^-13, exact in Q15); out holds 48 int16, n_phases and n_taps may be NULL.
 *
 * One call is n pairs of one stream.  x[i] is the new pairs for i >= 0, hist for i < 0 — the last NT - 1 pairs before the call, zero after
 * enable and reset — and zero further back.  Per channel, for 0 <= i < n and 0 <= p < P:   A[i][p] = sum over k of coef[p][k] x[i - k],   taken
 * exactly; the bound gives |A| <= 2 * 65535 * 32768 < 2^32.  hist becomes the last NT - 1 pairs of (hist, new pairs), also for n < NT - 1.
 *
 * Record (sdrfm_truepeak, 64 bytes): n, the pairs covered; peak_*, the maximum over i and p of |A| in units of 2^-15 LSB, so 0 dBTP = 2^30;
 * at_*, the smallest i at which some phase attains peak_*, counted from the record's first pair, 0 when peak_* is 0; over_*, the number of
 * (i, p) with |A| > limit (strict); reserved, 0.
 * The JOIN of a record a and the record b of the pairs that FOLLOW, sdrfm_truepeak_add(acc = a, m = b): n and over_* add; where b.peak > a.peak
 * (strict) the peak is b's and at = a.n + b.at, otherwise a's stay.  The join is associative and the zero record is its identity, so any cut
 * of a stream into calls, joined in order, gives the stream's record.
 * limit is in the record's units, 0 .. 2^32 - 1.  sdrfm_truepeak_limit(dbtp) = floor(2^30 10^(dbtp / 20)) clamped to that range, 0 for a NaN;
 * -1 dBTP is the R 128 production limit.
 *
 * Host side, plain C with no GPU behind it (csrc/truepeak.c):
 *   sdrfm_pcm_truepeak_s16   the definition as code, accumulating in 64 bits (it does not need the bound): joins the call's record onto *acc
 *                            and advances hist.  SDRFM_EINVAL, with nothing written: acc, coef or hist NULL, pcm_interleaved NULL with n > 0,
 *                            a shape outside the ranges, limit > 2^32 - 1.
 *   sdrfm_truepeak_add       the ordered join above; SDRFM_EINVAL for a NULL pointer.
 *   sdrfm_truepeak_report    in double: dbtp_l, dbtp_r and dbtp (their maximum) = 20 log10(peak / 2^30), -inf for a zero peak; over_frac_* =
 *                            over / (n P); at_seconds_* = at / fs_audio.  Every field is NaN for a record of no pairs.  SDRFM_EINVAL: a NULL
 *                            pointer, n_phases not 2, 4 or 8, fs_audio not finite and positive.
 *
 * On the sink (csrc/sdrfm_sink_stereo.hip, the kernel's body in csrc/sdrfm_truepeak.h).  A sink that never enables true peak allocates and
 * launches exactly what it did before.
 *   _truepeak_enable   coef NULL means the default table, and n_phases and n_taps are then not looked at.  A NULL sink, a table
 *                      sdrfm_truepeak_check_coef refuses, limit > 2^32 - 1: SDRFM_EINVAL before any device work, and an enabled sink goes on
 *                      as it was.  Allocates per stream the record and the history, and the packed table, zeroed (SDRFM_ENOMEM).  Enabling an
 *                      enabled sink waits for its stream and starts over.
 *   _truepeak_disable  waits for the sink's stream, stops the metering and frees what enable allocated.
 *   _truepeak_read     flags is a subset of SDRFM_F_DEVICE_PTRS | SDRFM_AMETER_F_RESET, out is 8-byte aligned and holds n_streams records, the
 *                      sink is enabled: else SDRFM_EINVAL.  The semantics are _meter_read's.  SDRFM_AMETER_F_RESET zeroes the records behind
 *                      the copy and KEEPS THE HISTORY: the stream continues, and the reads' records join to the stream's.
 *   sdrfm_pcm_stereo_sink_reset also zeroes an enabled sink's records and history.
 * While enabled, EVERY launch of the sink — its four forms, host or device buffers, and its launch behind sdrfm_stereo_process_batch_pcm,
 * sdrfm_bcast_process_batch_pcm, sdrfm_bcast_process_batch_metered and sdrfm_bcast_process_batch_metered_hist — is followed on the same stream
 * by one launch of k_pcm_truepeak over the rows just written, behind the audio meter's and the loudness kernels if those are enabled.  Those
 * kernels, their arguments and their bits are untouched.  The kernel: one workgroup of 1024 lanes per stream, the row in tiles of 4864 pairs
 * staged in LDS as an L and an R plane of packed sample pairs behind their NT - 1 predecessors, the table in LDS tap-reversed and packed; a
 * lane takes a pair's P phases of both channels as packed 16-bit dot products, each half-row into an int32 and the two halves summed in 64
 * bits; per channel one 64-bit key (peak << 32 | ~index) reduced by max over lanes, waves and the workgroup — no atomics.
 * Around the one-call forms, which launch on the HANDLE's stream, call enable, disable and read only after the handle's _synchronize — the rule
 * of the one-call forms at sdrfm_stereo_process_batch_pcm, which also allows them with both on one caller's stream. */
typedef struct sdrfm_truepeak {                    /* 64 bytes, 8-byte aligned */
  uint64_t n;
  uint64_t peak_l, peak_r;
  uint64_t at_l, at_r;
  uint64_t over_l, over_r;
  uint64_t reserved;
} sdrfm_truepeak;
typedef struct sdrfm_truepeak_report_t {
  double dbtp_l, dbtp_r, dbtp;
  double over_frac_l, over_frac_r;
  double at_seconds_l, at_seconds_r;
} sdrfm_truepeak_report_t;
int  sdrfm_truepeak_default_coef(int16_t* out /* 48 */, uint32_t* n_phases, uint32_t* n_taps);
int  sdrfm_truepeak_check_coef(const int16_t* coef, uint32_t n_phases, uint32_t n_taps);
uint64_t sdrfm_truepeak_limit(double dbtp);
int  sdrfm_pcm_truepeak_s16(const int16_t* pcm_interleaved, uint32_t n, const int16_t* coef, uint32_t n_phases, uint32_t n_taps, uint64_t limit,
                            int16_t* hist /* 2 * (n_taps - 1) */, sdrfm_truepeak* acc);
int  sdrfm_truepeak_add(sdrfm_truepeak* acc, const sdrfm_truepeak* m);
int  sdrfm_truepeak_report(const sdrfm_truepeak* m, uint32_t n_phases, double fs_audio, sdrfm_truepeak_report_t* out);
int  sdrfm_pcm_stereo_sink_truepeak_enable(sdrfm_pcm_stereo_sink_t* k, const int16_t* coef /* or NULL */, uint32_t n_phases, uint32_t n_taps, uint64_t limit);
int  sdrfm_pcm_stereo_sink_truepeak_disable(sdrfm_pcm_stereo_sink_t* k);
int  sdrfm_pcm_stereo_sink_truepeak_read(sdrfm_pcm_stereo_sink_t* k, sdrfm_truepeak* out /* n_streams records */, uint32_t flags);

/* A per-stream LOOK-AHEAD PCM LIMITER with a ramped make-up gain, behind the sinks: the int16 stereo rows either PCM sink
 * leaves, raised by up to x 16 and held under a sample ceiling, on the device — the actuator for what the loudness and true-peak meters read.  A
 * handle of its own beside the rate matcher.  All arithmetic is integer and exact: the device and the host routine agree bit for bit, and any
 * cut of a stream into calls gives the same outputs, state and (joined) records.
 *
 * Rows.  in[s * in_stride + 2i] = L, [... + 2i + 1] = R, i < n; out likewise, and a call of n pairs writes exactly n pairs per stream.  out may
 * be in (same pointer and stride): a sink's rows limited in place.
 * Handle-wide, at create: log2_window LW in 2 .. 8, W = 2^LW pairs, D = W - 1 the latency in pairs; gain_slew in 1 .. 32768, Q12 units per pair.
 * Per stream: the ceiling C in 1 .. 32767 LSB; the release delta in 1 .. 2^23; the make-up gain, a ramp (gain0, gain_t) in Q12 in [0, 65536]
 * (4096 = unity, 65536 = x 16).  After create C = 29204 (-1 dBFS, floored), delta = 874 (0 -> 1 in about 0.2 s at 48 kHz), gain0 = gain_t = 4096.
 *
 * Pair u of a stream, counted from reset; J the pairs since the last set_gain (saturating at 65536) and i the pair's index in the call:
 *   1  G = ramp(gain0, gain_t, gain_slew, J + i + 1): towards gain_t by at most gain_slew per pair (the closed form of the broadcast receiver's
 *      audio ramps);  x'_c[u] = (x_c[u] G + 2^11) >> 12 per channel, arithmetic shift, |x'| <= 2^19
 *   2  a[u] = max(|x'_L|, |x'_R|);  g[u] = 32768 where a <= C, else floor(C 32768 / a)                    (Q15, 32-bit unsigned division)
 *   3  m[u] = min over k = 0 .. D of g[u - k]
 *   4  r[u] = min(256 m[u], r[u - 1] + delta)                                                             (Q23)
 *   5  S[u] = sum over k = 0 .. D of r[u - k] <= 2^31;  s[u] = S >> (LW + 8)                              (Q15)
 *   6  y_c[u] = (x'_c[u - D] s[u] + 2^14) >> 15, 64-bit product, arithmetic shift, stored as int16 with no saturation
 * Before the start x' = 0, g = 32768, r = 2^23.
 *   The ceiling holds: every r in S[u] is <= 256 g[u - D], so s[u] <= g[u - D] and, with the rounding, |y| <= C for every pair.
 *   Transparency: with G = 4096 and no |x| over C, y[u] = x[u - D] bit for bit.
 *   Cut invariance: any cut into calls, of 0 pairs and of fewer than D pairs as well, gives the stream's output and state.
 * State per stream, 4 D int32 words, oldest first: x'_L and x'_R of the last D pairs interleaved, then g of the last D pairs, then r of the last
 * D pairs; r[u - 1] is the last word.  Parameter changes apply to the pairs that enter from the next call on; state words already held keep
 * the values they were computed with.
 * Record (sdrfm_pcm_limit_rec, 32 bytes): n, the pairs covered; limited, the pairs with s < 32768; min_gain, the smallest s (32768 for none);
 * at, the smallest u at which it was attained, counted from the record's first pair (0 for none).  The JOIN of a record a and the record b of
 * the pairs that FOLLOW, sdrfm_pcm_limit_add(acc = a, m = b): n and limited add; where b.min_gain < a.min_gain (strict) the minimum is b's and
 * at = a.n + b.at.  The join is associative and (0, 0, 32768, 0) is its identity.
 *
 * Host side, plain C with no GPU behind it (csrc/limit.c):
 *   sdrfm_pcm_limit_s16          one stream's call, the definition as code: limits n pairs, advances state (sdrfm_pcm_limit_state_words int32;
 *                                sdrfm_pcm_limit_state_init gives the state before the start) and joins the call's record onto *acc.  out may be
 *                                in.  SDRFM_EINVAL, with nothing touched: p, state or acc NULL, in or out NULL with n > 0, n > 2^20, J > 65536,
 *                                or anything sdrfm_pcm_limit_check_params refuses.
 *   sdrfm_pcm_limit_state_words  4 D for a log2_window in 2 .. 8, else 0.
 *   sdrfm_pcm_limit_check_params SDRFM_OK for parameters the device takes, SDRFM_EINVAL for NULL or any value outside the ranges above.
 *   sdrfm_pcm_limit_add          the ordered join above; SDRFM_EINVAL for a NULL pointer.
 *   sdrfm_pcm_limit_report       in double: reduction_db = -20 log10(min_gain / 32768) (0 for none, +inf for a gain of 0), limited_frac =
 *                                limited / n, at_seconds = at / fs_audio; every field NaN for a record of no pairs.  SDRFM_EINVAL: a NULL
 *                                pointer, fs_audio not finite and positive.
 *   sdrfm_pcm_limit_ceiling      floor(32768 10^(dbfs / 20)) clamped to 1 .. 32767; 1 for a NaN.
 *
 * The handle follows sdrfm_pcm_rate_*'s contract:
 *   create     config or out NULL, n_streams == 0, flags != 0, log2_window or gain_slew outside the ranges: SDRFM_EINVAL before any device is
 *              looked for; a missing or non-gfx950 device: SDRFM_NO_DEVICE.
 *   set_params one ceiling and one release per stream, either array may be NULL (those stay), not both; any value outside its range:
 *              SDRFM_EINVAL and every parameter stays.  Waits for the handle's stream.
 *   set_gain   one target per stream in Q12; any above 65536 or a jump other than 0 and 1: SDRFM_EINVAL and every ramp stays.  Every stream's
 *              ramp restarts at the value it has reached (jump = 0) or at the target itself (jump = 1), towards its new target, and J becomes 0.
 *              Waits for the handle's stream.
 *   get_params the parameters as the next call uses them (out, n_streams, or NULL) and J (or NULL).
 *   process_batch   Every refusal is made before anything is enqueued and leaves the handle as it was: flags outside SDRFM_F_DEVICE_PTRS,
 *              n > 2^20, an odd in_stride or out_stride (int16 elements): SDRFM_EINVAL; then n == 0 is a no-op; then in or out NULL, or device rows
 *              that are not 4-byte aligned: SDRFM_EINVAL; with more than one stream in_stride < 2n or out_stride < 2n: SDRFM_ECAPACITY.  Exactly
 *              2n int16 are written per row.  With SDRFM_F_DEVICE_PTRS the rows are device memory and the call only enqueues on the handle's
 *              stream: give it the sink's stream (or synchronise) so that it runs after the PCM exists.  With host buffers the call stages,
 *              runs, copies back and is synchronous.
 *   read       flags is a subset of SDRFM_F_DEVICE_PTRS | SDRFM_AMETER_F_RESET and out is 8-byte aligned and holds n_streams records: else
 *              SDRFM_EINVAL.  Host out: synchronises, copies and, with SDRFM_AMETER_F_RESET, sets the records to the identity behind the copy;
 *              device out: the same, enqueued on the handle's stream.  The state is KEPT: the stream continues and the reads' records join
 *              to the stream's.
 *   get_state  synchronises the handle's stream and gives the device's state, n_streams x 4 D int32.
 *   reset      the state to the one before the start and the records to the identity; the parameters, the ramps and J stay.
 *   NULL handles answer SDRFM_EINVAL (destroy: nothing; kernel_name: NULL).
 * The kernel (csrc/sdrfm_pcm_limit.hip, its body and the launch geometry in csrc/sdrfm_limit.h): one workgroup of 1024 lanes per stream, the row
 * in tiles of SDRFM_PCM_LIMIT_TILE pairs staged whole in LDS behind their D pairs of lead-in before any output of the tile is stored; the window
 * minimum and the window sum by LW doubling steps, the release as a scan over (min, +) maps — a lane's five consecutive pairs, the wave by
 * shuffles, the sixteen waves through LDS — with its carry in a register between tiles; no atomics.  kernel name: "pcm-limit". */
#define SDRFM_PCM_LIMIT_TILE 5120u                 /* pairs of a tile of k_pcm_limit: the tests place their shapes around it */
typedef struct sdrfm_pcm_limit sdrfm_pcm_limit_t;
typedef struct sdrfm_pcm_limit_config { uint32_t n_streams, log2_window, gain_slew, flags; int32_t device; } sdrfm_pcm_limit_config;
typedef struct sdrfm_pcm_limit_params { uint32_t ceiling, release, gain0, gain_t; } sdrfm_pcm_limit_params;      /* 16 bytes */
typedef struct sdrfm_pcm_limit_rec { uint64_t n, limited, min_gain, at; } sdrfm_pcm_limit_rec;                     /* 32 bytes, 8-byte aligned */
typedef struct sdrfm_pcm_limit_report_t { double reduction_db, limited_frac, at_seconds; } sdrfm_pcm_limit_report_t;
int  sdrfm_pcm_limit_create(const sdrfm_pcm_limit_config* config, sdrfm_pcm_limit_t** out);
void sdrfm_pcm_limit_destroy(sdrfm_pcm_limit_t* k);
int  sdrfm_pcm_limit_reset(sdrfm_pcm_limit_t* k);
int  sdrfm_pcm_limit_set_params(sdrfm_pcm_limit_t* k, const uint32_t* ceiling /* n_streams, or NULL */, const uint32_t* release /* likewise */);
int  sdrfm_pcm_limit_set_gain(sdrfm_pcm_limit_t* k, const uint32_t* gain_q12 /* n_streams */, uint32_t jump /* 0 or 1 */);
int  sdrfm_pcm_limit_get_params(const sdrfm_pcm_limit_t* k, sdrfm_pcm_limit_params* out /* n_streams, or NULL */, uint32_t* J);
int  sdrfm_pcm_limit_process_batch(sdrfm_pcm_limit_t* k, const int16_t* in, size_t in_stride, uint32_t n, int16_t* out, size_t out_stride, uint32_t flags);
int  sdrfm_pcm_limit_read(sdrfm_pcm_limit_t* k, sdrfm_pcm_limit_rec* out /* n_streams records */, uint32_t flags);
int  sdrfm_pcm_limit_get_state(sdrfm_pcm_limit_t* k, int32_t* state /* n_streams x 4 D */);
int  sdrfm_pcm_limit_set_stream(sdrfm_pcm_limit_t* k, void* hip_stream);
int  sdrfm_pcm_limit_synchronize(sdrfm_pcm_limit_t* k);
const char* sdrfm_pcm_limit_kernel_name(const sdrfm_pcm_limit_t* k);
int  sdrfm_pcm_limit_s16(const int16_t* in, uint32_t n, uint32_t log2_window, uint32_t gain_slew, uint32_t J, const sdrfm_pcm_limit_params* p,
                         int32_t* state /* 4 D */, int16_t* out, sdrfm_pcm_limit_rec* acc);
uint32_t sdrfm_pcm_limit_state_words(uint32_t log2_window);
int  sdrfm_pcm_limit_state_init(uint32_t log2_window, int32_t* state /* 4 D */);
int  sdrfm_pcm_limit_check_params(const sdrfm_pcm_limit_params* p, uint32_t log2_window, uint32_t gain_slew);
int  sdrfm_pcm_limit_add(sdrfm_pcm_limit_rec* acc, const sdrfm_pcm_limit_rec* m);
int  sdrfm_pcm_limit_report(const sdrfm_pcm_limit_rec* m, double fs_audio, sdrfm_pcm_limit_report_t* out);
uint32_t sdrfm_pcm_limit_ceiling(double dbfs);

/* The limiter's TRUE-PEAK FORM: the same handle, parameters, records and calls, with a detector that sees the waveform BETWEEN
 * the samples — the true-peak meter's interpolator over x' — so that the ceiling reads as dBTP.  It is a second constructor, host routine and
 * kernel instance; a handle made by sdrfm_pcm_limit_create, sdrfm_pcm_limit_s16 and k_pcm_limit are what they were, bit for bit.
 *
 * Handle-wide, besides LW and gain_slew: a table coef[P][NT] under exactly sdrfm_truepeak_check_coef's rules (NULL: sdrfm_truepeak_default_coef's,
 * and n_phases and n_taps are then not looked at); H = NT / 2.  The window has to hold half a row, 2^LW >= NT / 2: then D + H >= NT - 1 and the x'
 * delay line is the interpolator's history as well.  The latency is D + H pairs.
 *
 * Pair u of a stream; steps 1 and 3 - 5 are the sample form's:
 *   1   G and x'[u] as above, |x'| <= 2^19
 *   1b  per channel c and phase p   A_c[u][p] = sum over k of coef[p][k] x'_c[u - k],   exactly, x' = 0 before the start; the table's bound gives
 *       |A| <= 2 * 65535 * 2^19 < 2^36.  T[u] = the maximum of |A| over c and p.  With the table's layout (taps.truepeak_coef) these are the
 *       waveform's values between pairs u - H and u - H + 1.
 *   2'  v = u - H, the DETECTOR PAIR;  a[v] = max(|x'_L[v]|, |x'_R[v]|, (T[u] + 32767) >> 15) — the oversampled peak rounded UP to an LSB, a < 2^22;
 *       g[v] = 32768 where a <= C, else floor(C 32768 / a), the same 32-bit unsigned division.  x'[v] = 0 for v < 0, and g = 32768 for v < -H.
 *   3 - 5  on index v: m[v], r[v], S[v], s[v] as above
 *   6'  y_c[u] = (x'_c[v - D] s[v] + 2^14) >> 15, stored as int16 with no saturation
 * The start-up is part of the definition: for -H <= v < 0 the rule 2' applies with x'[v] = 0, so what the interpolator rings AHEAD of a stream's
 * first pairs is held under the ceiling like any other value.  (The state carries no count of pairs; zeros before the start and zeros in the
 * stream are the same state, and cut invariance needs them to be.)
 *   The sample ceiling still holds, |y| <= C: a[v] >= the pair's sample magnitude.
 *   Transparency: with G = 4096, every |x| <= C and every T <= C 2^15, y[u] = x[u - D - H] bit for bit.
 *   Cut invariance: any cut into calls, of 0 pairs and of fewer than D + H pairs as well, gives the stream's output, state and joined records.
 *   At constant gain: where s is one value over an interpolated value's support, that value of the OUTPUT is at most
 *   C 2^15 + floor(max over p of sum over k of |coef[p][k]| / 2) in the true-peak record's units; the second term is the rounding of y.
 * State per stream, 4 D + 2 H = 4 D + NT int32 words, oldest first: x'_L and x'_R of the last D + H pairs interleaved, then g of the last D detector
 * pairs, then r of the last D detector pairs; before the start 0, 32768 and 2^23.  The record and its join are the sample form's: s of the call's
 * output pairs.
 *
 *   sdrfm_pcm_tplimit_s16          one stream's call, the definition as code with 64-bit accumulation; out may be in.  SDRFM_EINVAL, with nothing
 *                                  touched: whatever sdrfm_pcm_limit_s16 refuses, a table sdrfm_truepeak_check_coef refuses, 2^LW < NT / 2.  coef NULL
 *                                  means the default table here as well.
 *   sdrfm_pcm_tplimit_state_words  4 D + NT for a log2_window in 2 .. 8 and an n_taps the table rules and the window take, else 0.
 *   sdrfm_pcm_tplimit_state_init   the state before the start; SDRFM_EINVAL for NULL or where _state_words answers 0.
 *   sdrfm_pcm_tplimit_latency      D + NT / 2, 0 where _state_words answers 0.
 *   sdrfm_pcm_limit_add, _report, _check_params and _ceiling serve both forms; a ceiling here reads as dBTP.
 *   sdrfm_pcm_tplimit_create       sdrfm_pcm_limit_create's rules for config, flags == 0 included; then a table sdrfm_truepeak_check_coef refuses or
 *                                  2^LW < NT / 2: SDRFM_EINVAL — all before any device is looked for.  Every sdrfm_pcm_limit_* call works on such a
 *                                  handle under the same contract; get_state gives n_streams x (4 D + NT) words; kernel name: "pcm-limit-tp".
 *   sdrfm_pcm_tplimit_get_detector n_phases, n_taps and the latency in pairs (each may be NULL): P, NT and D + H, or 0, 0 and D for a handle made
 *                                  by sdrfm_pcm_limit_create.  SDRFM_EINVAL for a NULL handle.
 * (The names keep clear of the prefix sdrfm_pcm_limit_, whose set of declarations is the sample form's ABI.)
 * The kernel k_pcm_limit_tp is a second instance of k_pcm_limit's body: the x' planes behind D + H pairs of lead-in, the packed table in LDS
 * tap-reversed, and per pair the P phases of both channels as 64-bit multiply-adds (x' has 20 bits); no atomics. */
int  sdrfm_pcm_tplimit_create(const sdrfm_pcm_limit_config* config, const int16_t* coef /* or NULL */, uint32_t n_phases, uint32_t n_taps, sdrfm_pcm_limit_t** out);
int  sdrfm_pcm_tplimit_get_detector(const sdrfm_pcm_limit_t* k, uint32_t* n_phases, uint32_t* n_taps, uint32_t* latency);
int  sdrfm_pcm_tplimit_s16(const int16_t* in, uint32_t n, uint32_t log2_window, uint32_t gain_slew, uint32_t J, const sdrfm_pcm_limit_params* p,
                           const int16_t* coef, uint32_t n_phases, uint32_t n_taps, int32_t* state /* 4 D + NT */, int16_t* out, sdrfm_pcm_limit_rec* acc);
uint32_t sdrfm_pcm_tplimit_state_words(uint32_t log2_window, uint32_t n_taps);
int  sdrfm_pcm_tplimit_state_init(uint32_t log2_window, uint32_t n_taps, int32_t* state /* 4 D + NT */);
uint32_t sdrfm_pcm_tplimit_latency(uint32_t log2_window, uint32_t n_taps);

/* ------------------------------------------------------------------------------------------------------------------
 * Raw-capture IQ meter: what the BYTES say, in front of every filter — ADC level, rail hits, DC and I/Q imbalance — so that a
 * tuner's gain can be driven (rtlctl.c holds the control arithmetic) without copying the capture to the host.  A handle of its own beside the
 * scan handle, with no stream state.  The rows are every handle's: iq[s * iq_stride + 2i] = I, [... + 2i + 1] = Q, bytes, i < n = nbytes / 2.
 * With bI and bQ the raw bytes as unsigned integers (NO centring inside the sums), a call's record per stream is
 *     n                        pairs
 *     sum_i, sum_q             sum bI, sum bQ
 *     sum_ii, sum_qq, sum_iq   sum bI^2, sum bQ^2, sum bI bQ
 *     rail_i, rail_q           bytes equal to 0 or 255
 * and its histogram row, SDRFM_IQ_HIST_BINS uint32: the counts of bI = 0 .. 255, then of bQ = 0 .. 255.  The row is tied to the record exactly:
 * the sum of either half is n, sum b hist is sum_i or sum_q, sum b^2 hist is sum_ii or sum_qq, hist[0] + hist[255] is rail_i or rail_q; only
 * sum_iq is not a function of the row.  EVERYTHING IS A SUM OF SMALL INTEGERS OVER THE BYTES: records and rows depend on nothing but the bytes,
 * the device equals sdrfm_iq_meter_u8 integer for integer, and a capture cut at any even byte offset gives records (sdrfm_iq_meter_add) and
 * rows (sdrfm_iq_hist_add, uint32 into uint64) that add up to the one call's.  No sum wraps: 64 MiB of 255 give sum_ii = 2^25 * 65025 < 2^42.
 *
 * sdrfm_iq_meter_process_batch's contract is sdrfm_scan_process_batch's, point by point and in its order.  NULL handle or NULL meters:
 * SDRFM_EINVAL.  Host buffers: a synchronous staged call.  SDRFM_F_DEVICE_PTRS: iq, meters (8-byte aligned) and hist (4-byte aligned) are device
 * memory on the handle's device and the call is only enqueued on the handle's stream; a misaligned meters or hist: SDRFM_EINVAL.
 * SDRFM_F_OVERLAP and unknown flags: SDRFM_EINVAL.  Odd nbytes: SDRFM_EODD.  nbytes above the maximum, or iq_stride < nbytes with more than one
 * stream: SDRFM_ECAPACITY.  meters (n_streams records) and hist (n_streams rows of SDRFM_IQ_HIST_BINS uint32, or NULL for the record alone) are
 * OVERWRITTEN: zeroed on the handle's stream, then added to; nbytes == 0 gives zero records and rows.  Then iq NULL: SDRFM_EINVAL.  iq and
 * iq_stride may be any byte value, odd ones included.
 * sdrfm_iq_meter_create: NULL, a wrong struct_size, n_streams == 0 or above 65536, max_bytes_per_call above 64 MiB or flags != 0: SDRFM_EINVAL,
 * all before any device is looked for.  Kernel name: that of the last call, "iq-meter" (also before any call) or "iq-meter-hist". */
typedef struct sdrfm_iq_meter {   /* 64 bytes, all sums of the call's pairs */
  uint64_t n;                      /* pairs */
  uint64_t sum_i, sum_q;           /* sum bI, sum bQ */
  uint64_t sum_ii, sum_qq, sum_iq; /* sum bI^2, sum bQ^2, sum bI bQ */
  uint64_t rail_i, rail_q;         /* bytes equal to 0 or 255 */
} sdrfm_iq_meter;
#define SDRFM_IQ_HIST_BINS 512u    /* row: counts of bI = 0..255, then of bQ = 0..255; uint32 per call */
#define SDRFM_IQ_MAX_BYTES (64u << 20)

typedef struct sdrfm_iq_meter_config {
  uint32_t struct_size;           /* = sizeof(sdrfm_iq_meter_config) */
  uint32_t n_streams;
  uint32_t max_bytes_per_call;    /* per stream; 0 = 1 MiB; at most 64 MiB */
  int32_t  device;
  uint32_t flags;                 /* 0 */
} sdrfm_iq_meter_config;

typedef struct sdrfm_iq_meter_handle sdrfm_iq_meter_t;

int  sdrfm_iq_meter_create(const sdrfm_iq_meter_config* cfg, sdrfm_iq_meter_t** out);
void sdrfm_iq_meter_destroy(sdrfm_iq_meter_t* h);
int  sdrfm_iq_meter_process_batch(sdrfm_iq_meter_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, sdrfm_iq_meter* meters,
                                  uint32_t* hist /* n_streams x SDRFM_IQ_HIST_BINS, or NULL */, uint32_t flags);
int  sdrfm_iq_meter_set_stream(sdrfm_iq_meter_t* h, void* hip_stream);   /* does NOT wait for the stream in use (every call stands alone): synchronise first */
int  sdrfm_iq_meter_synchronize(sdrfm_iq_meter_t* h);
const char* sdrfm_iq_meter_kernel_name(const sdrfm_iq_meter_t* h);

/* Host-only (plain C99, no GPU).
 *   sdrfm_iq_meter_u8   the definition as code: the record of nbytes / 2 pairs ADDED onto acc, and their counts onto hist512 (uint64, may be NULL).
 *                       NULL acc, NULL iq with nbytes != 0: SDRFM_EINVAL; odd nbytes: SDRFM_EODD; nothing touched.
 *   sdrfm_iq_meter_add  acc += m, field by field.  sdrfm_iq_hist_add: acc512[b] += row512[b].  NULL: SDRFM_EINVAL. */
int  sdrfm_iq_meter_u8(const uint8_t* iq, size_t nbytes, sdrfm_iq_meter* acc, uint64_t* hist512);
int  sdrfm_iq_meter_add(sdrfm_iq_meter* acc, const sdrfm_iq_meter* m);
int  sdrfm_iq_hist_add(uint64_t* acc512, const uint32_t* row512);

/* What a record says, in double.  The central moments are formed as integers first, in unsigned __int128 — n sum b^2 - (sum b)^2 and
 * n sum bI bQ - sum bI sum bQ — and divided once by n^2, so a long quiet capture loses nothing to cancellation.  With var_i, var_q and cov those
 * moments in LSB^2:
 *     dc_i, dc_q            mean - 127.5, in LSB
 *     rms_dbfs              10 log10((var_i + var_q) / 127.5^2): 0 for a complex tone that just touches the rails
 *     total_dbfs            the same with the DC power dc_i^2 + dc_q^2 included
 *     rail_share_i, _q      rail_i / n, rail_q / n
 *     gain_db               10 log10(var_q / var_i)
 *     skew_rad              asin(cov / sqrt(var_i var_q)), the ratio clamped to +-1
 *     image_rejection_db    10 log10((1 + 2 g cos(skew) + g^2) / (1 - 2 g cos(skew) + g^2)), g = sqrt(var_q / var_i); +inf for g = 1 and no skew
 * THE LAST THREE ASSUME a capture whose content is circular — stations off centre, noise, or FM through many turns of the phase — for which I and Q
 * have equal power and no correlation before the front end's imbalance.  A carrier at centre, or a short capture of slow content, breaks the
 * assumption; they are estimates, not bounds.  n == 0: every field is NaN (SDRFM_OK), as the other report routines answer.  Zero variance
 * (var_i + var_q == 0): rms_dbfs is -inf; var_i == 0 or var_q == 0: the three imbalance fields are NaN.  NULL: SDRFM_EINVAL; so is a record no
 * capture can give (a negative variance). */
typedef struct sdrfm_iq_report_t {
  double dc_i, dc_q, rms_dbfs, total_dbfs, rail_share_i, rail_share_q, gain_db, skew_rad, image_rejection_db;
} sdrfm_iq_report_t;
int  sdrfm_iq_meter_report(const sdrfm_iq_meter* m, sdrfm_iq_report_t* out);

/* What an accumulated row says, per component c = I, Q, with the level of a code b its distance from mid-scale |2 b - 255| / 255 (1 at the rails):
 *     n                     sum of the I half (the Q half's differs: SDRFM_EINVAL)
 *     peak_c                the largest level among the codes used
 *     level999_c            the smallest level L such that at least 99.9 % of the samples have a level <= L
 *     codes_c               the number of codes used
 *     headroom_db_c         -20 log10(level999_c): the 99.9 % level against the rail (a level is at least 1 / 255)
 * n == 0: every field but n is NaN (SDRFM_OK).  NULL: SDRFM_EINVAL. */
typedef struct sdrfm_iq_hist_report_t {
  uint64_t n;
  double peak_i, peak_q, level999_i, level999_q, codes_i, codes_q, headroom_db_i, headroom_db_q;
} sdrfm_iq_hist_report_t;
int  sdrfm_iq_hist_report(const uint64_t* hist512, sdrfm_iq_hist_report_t* out);

/* ------------------------------------------------------------------------------------------------------------------
 * A PCM MIX BUS: n_bus output stereo rows formed from n_in input stereo rows on the device — station selection, crossfade and
 * channel routing without a click.  A handle of its own beside the rate matcher and the limiter.  Rows are theirs: row[2i] = L, row[2i + 1] = R,
 * int16, i < n.  All arithmetic is integer and exact: the device and the host routine agree bit for bit, and any cut of a run into calls gives
 * the same PCM and the same joined records.
 *
 * Handle-wide, at create: n_in and n_bus in 1 .. 65536; n_slots K in 1 .. 8; slew in 1 .. 32768, Q15 units per pair; an optional curve of
 * SDRFM_PCM_MIX_CURVE_LEN = 129 uint16 values t[0 .. 128] with t[0] = 0, t[128] = 32768 and no decrease (sdrfm_pcm_mix_check_curve).
 * Every bus has K slots.  A slot (sdrfm_pcm_mix_slot, 16 bytes) names a source row src < n_in, or SDRFM_PCM_MIX_NONE, which contributes nothing;
 * a channel mode; and a gain ramp (g0, gt), Q15 in [0, 32768].  With (L, R) the source pair the slot contributes (l, r):
 *     0 STEREO (2L, 2R)    1 MONO (L + R, L + R)    2 LEFT (2L, 2L)    3 RIGHT (2R, 2R)    4 SWAP (2R, 2L)
 * After create every slot is (NONE, STEREO, 0, 0).
 *
 * Pair i of a call; J the pairs since the last set_gains, saturating at 65536.  For a bus and each of its slots k:
 *   1  g_k = ramp(g0_k, gt_k, slew, J + i + 1): towards gt by at most slew per pair (the closed form of the broadcast receiver's audio ramps)
 *   2  c_k = g_k without a curve; with one c(32768) = t[128], else j = g >> 8, f = g & 255, c = t[j] + (((t[j + 1] - t[j]) f + 128) >> 8)
 *   3  acc_c = sum over k of c_k (l_k or r_k) per channel, exactly (|acc| <= 8 * 2^15 * 2^16 = 2^34: a 64-bit sum)
 *   4  v_c = (acc_c + 2^15) >> 16, arithmetic shift;  y_c = clamp(v_c, -32768, 32767)
 *   Unity: one STEREO slot at 32768 beside slots at 0 gives y = x bit for bit.
 *   Self-crossfade: without a curve (or with the linear one) two slots on one source and mode that ramp 32768 -> 0 and 0 -> 32768 from one
 *   set_gains give y = x bit for bit at every pair and slew: both have moved by min(n slew, 32768).
 *   MONO at 32768 is (L + R + 1) >> 1 and never clips.
 *   A slot with src = NONE or g0 = gt = 0 contributes 0 (c(0) = 0) and its row is never read.
 * Record per bus (sdrfm_pcm_mix_rec, 32 bytes, 8-byte aligned): n, the pairs covered; clipped_l and clipped_r, the outputs with v != y per channel;
 * peak, the largest |v| of both channels before the clamp (<= 2^18).  The join (sdrfm_pcm_mix_add): the counts add, peak is the maximum —
 * commutative, associative, identity (0, 0, 0, 0).
 *
 * Host side, plain C with no GPU behind it (csrc/pcm_mix.c):
 *   sdrfm_pcm_mix_s16          ONE bus's call, the definition as code: in is the n_in input rows (in_stride int16 apart, not looked at for
 *                              n_in == 1), slots the bus's n_slots slots, J as above; 2n int16 are written to out and the call's record is joined
 *                              onto *acc.  SDRFM_EINVAL, with nothing touched: slots or acc NULL, in or out NULL with n > 0, n_in, n_slots or slew
 *                              outside the ranges, n > 2^20, J > 65536, an odd in_stride, slots sdrfm_pcm_mix_check_slots refuses, a curve
 *                              sdrfm_pcm_mix_check_curve refuses; SDRFM_ECAPACITY: n_in > 1 and in_stride < 2n.  out must not overlap in.
 *   sdrfm_pcm_mix_check_slots  SDRFM_OK where every one of count slots has src < n_in or NONE, mode <= 4 and g0, gt <= 32768; else SDRFM_EINVAL
 *                              (also for NULL).
 *   sdrfm_pcm_mix_check_curve  SDRFM_OK for a table under the rules above; else SDRFM_EINVAL (also for NULL).
 *   sdrfm_pcm_mix_add          the join; SDRFM_EINVAL for a NULL pointer.
 *   sdrfm_pcm_mix_report       in double: peak_dbfs = 20 log10(peak / 32768) (-inf for 0), clipped_frac = (clipped_l + clipped_r) / (2n); every
 *                              field NaN for n = 0.  SDRFM_EINVAL for a NULL pointer.
 *
 * The handle follows sdrfm_pcm_limit_*'s contract; every refusal is made before anything is enqueued and leaves the handle as it was:
 *   create     config or out NULL, flags != 0, n_in, n_bus, n_slots or slew outside the ranges, a curve check_curve refuses: SDRFM_EINVAL before
 *              any device is looked for; a missing or non-gfx950 device: SDRFM_NO_DEVICE.  curve NULL: c = g.
 *   set_routes src and mode are n_bus x n_slots each; either may be NULL (those stay), not both; a src that is neither below n_in nor NONE, or a
 *              mode above 4: SDRFM_EINVAL and nothing changes.  Gains and J are untouched; takes effect with the next call.  Waits for the
 *              handle's stream.
 *   set_gains  one target per slot, n_bus x n_slots; any above 32768 or a jump other than 0 and 1: SDRFM_EINVAL and every ramp stays.  Every
 *              slot's ramp restarts at the value it has reached (jump = 0) or at its target (jump = 1), and J becomes 0.  Waits for the handle's
 *              stream.
 *   get_slots  the slots as the next call uses them (out, n_bus x n_slots, or NULL) and J (or NULL).
 *   process_batch   flags outside SDRFM_F_DEVICE_PTRS, n > 2^20, an odd in_stride or out_stride (int16 elements): SDRFM_EINVAL; then n == 0 is a
 *              no-op; then in or out NULL, or device rows that are not 4-byte aligned: SDRFM_EINVAL; n_in > 1 with in_stride < 2n, or n_bus > 1 with
 *              out_stride < 2n: SDRFM_ECAPACITY; then the byte range of the output rows overlapping that of the input rows: SDRFM_EINVAL — bus b
 *              writes while bus c reads, so there is no in-place form.  Exactly 2n int16 are written per bus row.  J advances by n, saturating,
 *              on success only.  With SDRFM_F_DEVICE_PTRS the rows are device memory and the call only enqueues on the handle's stream; with
 *              host buffers it stages, runs, copies back and is synchronous.
 *   read       flags is a subset of SDRFM_F_DEVICE_PTRS | SDRFM_AMETER_F_RESET and out is 8-byte aligned and holds n_bus records: else
 *              SDRFM_EINVAL.  Host out: synchronises, copies and, with SDRFM_AMETER_F_RESET, zeroes the records behind the copy; device out: the
 *              same, enqueued on the handle's stream.
 *   reset      the records to the identity; the slots, the ramps and J stay.
 *   NULL handles answer SDRFM_EINVAL (destroy: nothing; kernel_name: NULL).
 * The kernel (csrc/sdrfm_pcm_mix.hip, body and geometry in csrc/sdrfm_pcm_mix.h): n_bus x cdiv(n, SDRFM_PCM_MIX_SPAN) workgroups of 256 lanes, a
 * bus's slots read once per workgroup and a dead slot skipped by a uniform branch, ramp and curve evaluated per pair from values, the curve in
 * LDS, dword accesses throughout, the record by one 64-bit integer atomic per field and workgroup.  kernel name: "pcm-mix". */
#define SDRFM_PCM_MIX_SPAN 2048u                   /* pairs of a workgroup of k_pcm_mix: the tests place their shapes around it */
#define SDRFM_PCM_MIX_NONE 0xFFFFFFFFu             /* a slot's src: no source */
#define SDRFM_PCM_MIX_CURVE_LEN 129u
#define SDRFM_PCM_MIX_STEREO 0u
#define SDRFM_PCM_MIX_MONO 1u
#define SDRFM_PCM_MIX_LEFT 2u
#define SDRFM_PCM_MIX_RIGHT 3u
#define SDRFM_PCM_MIX_SWAP 4u
typedef struct sdrfm_pcm_mix sdrfm_pcm_mix_t;
typedef struct sdrfm_pcm_mix_config { uint32_t n_in, n_bus, n_slots, slew, flags; int32_t device; } sdrfm_pcm_mix_config;
typedef struct sdrfm_pcm_mix_slot { uint32_t src, mode, g0, gt; } sdrfm_pcm_mix_slot;                            /* 16 bytes */
typedef struct sdrfm_pcm_mix_rec { uint64_t n, clipped_l, clipped_r, peak; } sdrfm_pcm_mix_rec;                  /* 32 bytes, 8-byte aligned */
typedef struct sdrfm_pcm_mix_report_t { double peak_dbfs, clipped_frac; } sdrfm_pcm_mix_report_t;
int  sdrfm_pcm_mix_create(const sdrfm_pcm_mix_config* config, const uint16_t* curve /* 129, or NULL */, sdrfm_pcm_mix_t** out);
void sdrfm_pcm_mix_destroy(sdrfm_pcm_mix_t* k);
int  sdrfm_pcm_mix_reset(sdrfm_pcm_mix_t* k);
int  sdrfm_pcm_mix_set_routes(sdrfm_pcm_mix_t* k, const uint32_t* src /* n_bus x n_slots, or NULL */, const uint32_t* mode /* likewise */);
int  sdrfm_pcm_mix_set_gains(sdrfm_pcm_mix_t* k, const uint32_t* target /* n_bus x n_slots */, uint32_t jump /* 0 or 1 */);
int  sdrfm_pcm_mix_get_slots(const sdrfm_pcm_mix_t* k, sdrfm_pcm_mix_slot* out /* n_bus x n_slots, or NULL */, uint32_t* J);
int  sdrfm_pcm_mix_process_batch(sdrfm_pcm_mix_t* k, const int16_t* in, size_t in_stride, uint32_t n, int16_t* out, size_t out_stride, uint32_t flags);
int  sdrfm_pcm_mix_read(sdrfm_pcm_mix_t* k, sdrfm_pcm_mix_rec* out /* n_bus records */, uint32_t flags);
int  sdrfm_pcm_mix_set_stream(sdrfm_pcm_mix_t* k, void* hip_stream);
int  sdrfm_pcm_mix_synchronize(sdrfm_pcm_mix_t* k);
const char* sdrfm_pcm_mix_kernel_name(const sdrfm_pcm_mix_t* k);
int  sdrfm_pcm_mix_s16(const int16_t* in, size_t in_stride, uint32_t n_in, uint32_t n, const sdrfm_pcm_mix_slot* slots, uint32_t n_slots, uint32_t slew,
                       uint32_t J, const uint16_t* curve /* 129, or NULL */, int16_t* out, sdrfm_pcm_mix_rec* acc);
int  sdrfm_pcm_mix_check_slots(const sdrfm_pcm_mix_slot* slots, uint32_t count, uint32_t n_in);
int  sdrfm_pcm_mix_check_curve(const uint16_t* curve /* 129 */);
int  sdrfm_pcm_mix_add(sdrfm_pcm_mix_rec* acc, const sdrfm_pcm_mix_rec* m);
int  sdrfm_pcm_mix_report(const sdrfm_pcm_mix_rec* m, sdrfm_pcm_mix_report_t* out);

#ifdef __cplusplus
}
#endif
#endif /* SDRFM_H */
