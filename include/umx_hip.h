/*
 * umx_hip.h -- C-ABI of the MI355X (gfx950) Open-Unmix segment-inference engine.
 *
 * Drop-in boundary for the reference's src/inference.cpp.  The reference has no plugin / FFI
 * surface; the seam is the C++ call
 *     std::vector<Eigen::MatrixXf> umxcpp::umx_inference(umx_model&, const Eigen::MatrixXf audio,
 *         stft_buffers, std::array<lstm_data,4>& streaming_lstm_data);      (src/inference.hpp:20-23)
 * made once per segment from umx.cpp:226-227, plus load_umx_model (src/model.hpp:58) that fills
 * the model.  Each entry point below names what it replaces.  Plain pointers and sizes only:
 * no Eigen, no torch types.  Every function returns an int status (UMX_OK == 0); the library
 * never calls exit() (the reference exits or returns false: dsp.cpp:27-44, model.cpp:59-64).
 *
 * A (2,n) Eigen ColMajor MatrixXf is exactly n interleaved stereo frames, so "audio" and "out"
 * buffers here are bit-identical to the reference's waveform matrices.
 *
 * Threading: one caller thread per context (as the reference: not re-entrant per stream state).
 */
#ifndef UMX_HIP_H
#define UMX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UMX_OK 0
#define UMX_ERR_ARG 1     /* bad argument / shape (the reference: assert compiled out, or return false) */
#define UMX_ERR_HIP 2     /* a HIP runtime call failed; see umx_hip_last_error */
#define UMX_ERR_MODEL 3   /* missing / mis-shaped tensor (model.cpp:541-546, 582-591) */
#define UMX_ERR_TIMEOUT 4 /* persistent LSTM kernel gave up waiting (bounded spin) */
#define UMX_ERR_NODEVICE 5

#define UMX_DTYPE_F32 0
#define UMX_DTYPE_U8 1  /* model.cpp:578-619 load_single_matrix */
#define UMX_DTYPE_U16 2 /* model.cpp:623-665 load_single_matrix_uint16 */

/* flags of umx_hip_infer_segment* */
#define UMX_FLAG_NO_WIENER 0x1      /* BASELINE config 2: mix-phase estimate only (wiener.cpp:96-109) */
/* Wiener EM iterations per call (flag bits 16-19): the reference's `for (int it = 0; it < WIENER_ITERATIONS; ++it)` of
 * wiener.cpp:175, with WIENER_ITERATIONS = 1 at wiener.hpp:17; Open-Unmix's `niter`.  A field of 0 means 1 iteration, allowed are
 * 1 .. 15.  Iteration k >= 2 forms the PSD and the spatial covariances from iteration k - 1's filtered spectrograms and filters the
 * mixture again.  UMX_FLAG_NO_WIENER ignores it. */
#define UMX_FLAG_WIENER_ITERS_MASK 0xF0000u
#define UMX_FLAG_WIENER_ITERS(n) ((((unsigned)(n)) & 0xFu) << 16)
#define UMX_FLAG_SKIP_TARGET(t) (0x100 << (t)) /* BASELINE config 1 (vocals only = skip 0,1,2) */
/* Residual source: Open-Unmix's Separator(targets=[...], residual=True) -- no analogue in the reference, whose umx_inference
 * always runs all four models.  Together with UMX_FLAG_SKIP_TARGET: the LOWEST skipped target's slot r (umx_hip_residual_slot) carries one more
 * source, "everything else": its mask plane is rho = 1.0f - ((m_j1 + m_j2) + m_j3) over the active targets j1 < j2 < j3 (fp32, as many terms
 * as there are; may be negative), so its magnitude is rho |X| and its first estimate X - sum_j y_j (Open-Unmix's `mix_stft - sum of targets`);
 * from there on it is a source like any other in the EM, and out[4 * lane + r] receives its stem.  The other skipped targets stay silent.
 * Needs at least one skipped and one active target, else UMX_ERR_ARG (four targets + residual would be five sources: not supported).
 * "vocals + accompaniment" = UMX_FLAG_SKIP_TARGET(0) | (1) | (2) | UMX_FLAG_RESIDUAL: out[3] vocals, out[0] accompaniment, one network's cost. */
#define UMX_FLAG_RESIDUAL 0x8000
/* Soft mask: Open-Unmix's Separator(softmask=True) -- no analogue in the reference.  The first estimate of a source is
 * y_j = X g_j / (eps + sum_k g_k) with g_j = mask_j |X| instead of mask_j |X| X/|X|: the first estimates (and so the UMX_FLAG_NO_WIENER stems)
 * add up to the mixture, and no target's initial PSD counts more energy than the mixture holds.  Right after fc3 the mask planes of the ACTIVE
 * targets j1 < j2 < ... are rewritten in place, for every channel, frame and bin b <= 2048, in fp32:
 *     a = |X| (the one mix_magnitude of csrc/common.h)    g_j = m_j * a
 *     d = 1e-10f + (((g_j1 + g_j2) + g_j3) + g_j4)        (as many terms as there are; 1e-10 = WIENER_EPS = Open-Unmix's eps)
 *     m'_j = g_j / d                                      (the correctly rounded quotient)
 * and every consumer goes on forming m'_j a X/|X| = X g_j / (eps + sum g).  A silent bin (a = 0) gives m' = 0; a skipped target takes no part
 * in the sum and stays what it is (zero planes, or the residual); the "mask" and "target_mag" taps show m' and m' a.  With UMX_FLAG_RESIDUAL the
 * order is Open-Unmix's: normalise, then rho = 1 - sum m' from the normalised planes -- the residual's first estimate is then eps / (eps + sum g)
 * of the mixture, i.e. almost nothing, and only the EM iterations give it energy (Open-Unmix behaves the same).  A call without the flag
 * launches exactly what it launched before the flag existed.  Not supported by the multi-GPU driver in by-target mode (no rank holds every mask). */
#define UMX_FLAG_SOFTMASK 0x2
#define UMX_FLAG_LSTM_STEPWISE 0x10 /* one launch per timestep instead of the persistent kernel */
#define UMX_FLAG_DEBUG_TAPS 0x20    /* keep what only the taps read: the filtered spectrograms for umx_hip_read_tap("y") (the fused kernel does not
                                     * write them otherwise) and, in track-batched contexts, the fp32 rows of the recurrence's layers ("lstm",
                                     * "lstm_l0", "lstm_l1": the batched kernels write the next GEMM's fp16 planes instead, csrc/lstm_batch.h) */
#define UMX_FLAG_LSTM_FORCE_SAFE 0x40 /* persistent kernel: never take the intra-XCD fast protocol */
#define UMX_FLAG_LSTM_PROFILE 0x80  /* persistent kernel: record per-phase cycle counters */
#define UMX_FLAG_DEBUG_LSTM_ABORT 0x2000 /* testing: the persistent LSTM launch of layer 1 gives up half way, exactly as if a
                                          hidden-state poll had timed out (exercises the recovery of umx_hip_sync) */
#define UMX_FLAG_RESET_SEGMENTS 0x4000 /* umx_hip_split_inference / _shift_inference / _separate_tracks with ONE track on a context made by
                                        * umx_hip_create_tracks: RESET MODE -- every segment starts from a zero lstm_data instead of the one its
                                        * predecessor left (umx.cpp:167-171 creates it once per track, :226-227 passes it to every segment): a
                                        * DECLARED deviation from the reference, opt-in.  The track's segments are then independent and ride as
                                        * the track lanes of one call (a 600 s track = 14 lanes of one pass).  Equals split_inference with
                                        * umx_lstm_set_zero (lstm.cpp:86-99) in front of every segment. */
#define UMX_FLAG_PRECISE_ACT 0x1000 /* LSTM gates with the device-library expf/tanhf + IEEE division instead of
                                       the hardware v_exp_f32 / v_rcp_f32 forms (~1e-7 abs difference) */

/* One tensor of the ggml-style weight file, as stored (scripts/convert-umx-pth-to-ggml.py:146-160
 * record = {scale, offset, n_dims, name_len, ne[], name, data}).  dtype F32 means `data` is already
 * dequantised fp32 in PyTorch row-major order and scale/offset are ignored. */
typedef struct umx_tensor_view
{
    const char *name; /* "fc1.weight", "lstm.weight_hh_l2_reverse", ... */
    int target;       /* 0 = bass, 1 = drums, 2 = other, 3 = vocals (convert script :104) */
    int dtype;        /* UMX_DTYPE_* */
    int n_dims;
    int ne[2];        /* PyTorch shape reversed, as in the file */
    float scale, offset;
    const void *data;
} umx_tensor_view;

typedef struct umx_hip_ctx umx_hip_ctx;

/* Replaces the result of load_umx_model (model.cpp:42-574) living on the device: dequantises
 * (q*scale+offset, model.cpp:610-616), re-lays the weights out for the kernels and uploads them.
 * segment_samples = the stft_buffers size (umx.cpp:160: 60 s * 44100 = 2,646,000): every segment,
 * also a shorter last one, is processed as T = segment_samples/1024+1 frames (dsp.cpp:214-217).
 * Needs 4 x 43 tensors (model.cpp:240-539 name dispatch).  hidden_size % 128 == 0. */
int umx_hip_create(umx_hip_ctx **out, int device, int hidden_size, int segment_samples,
                   const umx_tensor_view *tensors, int n_tensors);
/* Weight residency (BASELINE config 5 / SURVEY 8(f)1).  Tensors handed over as u8 / u16 views (the ggml file's own
 * bytes: u8 fc1, W_ih, W_hh; u16 fc2, fc3 -- convert-umx-pth-to-ggml.py:127-160) stay that way in HBM by default
 * and q*scale+offset (model.cpp:610-616) is evaluated where they are consumed: in the GEMM's B-tile staging and in
 * the LSTM kernel's one-time W_hh register load.  139 MB of weights for UMX-L instead of 452 MB (fp32) / 630 MB
 * (three bf16 planes), bit-identical results, and measured FASTER (7.5 vs 8.0 ms per segment: the B operand moves
 * 1-2 bytes per weight instead of 6).  UMX_CREATE_DEQUANTISE_AT_LOAD (environment UMX_WEIGHTS_RESIDENT=expanded)
 * expands them at load time instead; fp32 views are always expanded.  UMX_CREATE_QUANTISED_RESIDENT is accepted
 * for compatibility and is the default. */
#define UMX_CREATE_QUANTISED_RESIDENT 0x1u
#define UMX_CREATE_DEQUANTISE_AT_LOAD 0x8u
/* The dense stack (fc1, W_ih, fc2, fc3 -- inference.cpp:86,127,143, lstm.cpp:132-135) runs on the 16-bit matrix cores
 * with split operands and fp32 accumulation (csrc/gemm_planes.h, csrc/gemm_bf16x3.h, below): the dropped terms are below
 * 2^-22 .. 2^-26 of a product, and against a float64 evaluation the result is as close as an fp32-MFMA kernel's (measured:
 * slightly closer; profiles/r02_accuracy_vs_float64.txt).  Rounds 1-2 also carried that fp32-MFMA flavour
 * (UMX_CREATE_GEMM_F32): removed in round 3; the flag is now refused with UMX_ERR_ARG. */
#define UMX_CREATE_GEMM_F32 0x4u
/* u8-resident weights (fc1, W_ih; W_hh in the batched LSTM kernel) on the bf16 matrix cores: q - c is an integer of at
 * most 255 and EXACT in bf16 and fp16 for any centre c in 0 .. 255 (gemm_bf16x3.h: the tensor's zero-weight code round(-o / s);
 * the plane GEMMs and the batched recurrences: 128), so by default the weight is ONE term (three products with the bf16-split
 * activation instead of six; two with the fp16 planes of csrc/gemm_planes.h) and the affine map of model.cpp:610-616 is applied to the accumulated sum:
 *     sum_k a_k (q_k s + o) = s sum_k a_k (q_k - c) + (o + c s) sum_k a_k.
 * The reference rounds q*s+o to fp32 per weight first; the two differ by exactly that rounding (~1e-7 of the dot
 * product, the size of one fp32 rounding of the sum).  UMX_CREATE_U8_DEQUANT (environment UMX_U8=dequant) keeps the
 * per-weight form (dequantise, split in three, six products): bit-identical to UMX_CREATE_DEQUANTISE_AT_LOAD. */
#define UMX_CREATE_U8_DEQUANT 0x20u
/* The split-operand GEMM flavour exists in two forms.  csrc/gemm_planes.h (default of track-batched contexts): every
 * activation matrix is split once, by a small kernel, into TWO fp16 planes of the row scaled by a power of two (+ row
 * sums and inverse scales), every weight matrix is re-encoded once at load time as exact fp16 integer planes (u8: 1,
 * u16: 2; fp32: 2 split terms), and the GEMM itself only moves 256 x 256 tiles global -> LDS by DMA, over all track lanes
 * at once, and issues matrix-core instructions (2 products per fp32 product for u8 weights, 4 for u16).
 * csrc/gemm_bf16x3.h (default of single-track contexts): keeps u8 / u16 weights as stored and splits both operands while
 * staging every 128 x 128 tile; small enough in registers and LDS to share the CUs with the two co-resident single-track
 * LSTM grids of the latency pipeline.  UMX_CREATE_GEMM_STAGED / UMX_CREATE_GEMM_PLANES (environment UMX_GEMM=bf16x3 /
 * planes) force one or the other. */
#define UMX_CREATE_GEMM_STAGED 0x40u
#define UMX_CREATE_GEMM_PLANES 0x80u
int umx_hip_create_ex(umx_hip_ctx **out, int device, int hidden_size, int segment_samples,
                      const umx_tensor_view *tensors, int n_tensors, unsigned create_flags);
/* Track batching.  The reference is one track per process (umx.cpp:26-97) and its LSTM is one
 * matrix-vector product per step (lstm.cpp:132-161) -- on a GPU that step is bound by the cross-CU hand-off latency,
 * not by arithmetic.  A context created for n_tracks (1..UMX_MAX_TRACKS = 64) independent tracks holds that many "track lanes", each
 * with its own streaming LSTM state (= its own std::array<lstm_data,4>, umx.cpp:167-171) and activation buffers;
 * umx_hip_infer_batch* runs one segment of every lane per call, and the recurrence of all lanes is ONE launch per
 * layer in which W_hh.h is a matrix-matrix product on the matrix cores (u8 W_hh as one exact fp16 plane against two fp16
 * planes of h, fp32 accumulate: csrc/lstm_batch.h).  The LSTM flavour is fixed per context: n_tracks > 1 (or UMX_CREATE_LSTM_BATCHED, environment
 * UMX_LSTM=batched, on a 1-track context) selects the batched kernel for every call, so a track's result never
 * depends on how many lanes a call uses or which lane it sits in (bitwise; tests/test_gpu_batch.py).  Against the
 * single-track kernel the results agree to fp32 rounding (different summation order), not bitwise.
 * Hidden 1024 (UMX-L) and 512 (umxhq) with the u8-resident W_hh of a quantised model, any number of lanes: csrc/lstm_batch8.h -- a
 * workgroup serves an octet of 8 lanes x 64 hidden units (N of the matrix instruction = 8 lanes x the 2 planes of h); hidden 1024: 32
 * lanes per launch with one octet per workgroup, 33 .. 64 with two octets per workgroup IN TURN (one octet's hand-off travels under
 * the other's matrix and gate phases); hidden 512: its 64 lanes side by side.  Other hidden sizes / fp32-resident W_hh:
 * lstm_batch_kernel of csrc/lstm_batch.h, a group of 16 lanes per launch, the groups of a larger context one launch after the other. */
#define UMX_CREATE_LSTM_BATCHED 0x10u
#define UMX_MAX_TRACKS 64
int umx_hip_create_tracks(umx_hip_ctx **out, int device, int hidden_size, int segment_samples,
                          const umx_tensor_view *tensors, int n_tensors, unsigned create_flags, int n_tracks);
int umx_hip_n_tracks(const umx_hip_ctx *ctx);
/* Segments the context keeps in flight (= its pipeline slots, each with its own stream): 2.  The buffers of that many
 * CONSECUTIVE asynchronous calls must be distinct (ordering contract of umx_hip_infer_segment_device below). */
int umx_hip_pipeline_depth(const umx_hip_ctx *ctx);
int umx_hip_lstm_is_batched(const umx_hip_ctx *ctx);
size_t umx_hip_weight_bytes(const umx_hip_ctx *ctx); /* HBM bytes held by the model's weight matrices */
void umx_hip_destroy(umx_hip_ctx *ctx);
const char *umx_hip_last_error(const umx_hip_ctx *ctx); /* never NULL; also valid for ctx == NULL (create errors) */

/* Streaming LSTM state = the h/c members of lstm_data (lstm.hpp:10-16), created zeroed once per
 * track (umx.cpp:167-171, lstm.cpp:82) and carried across segments.
 * Layout: [4 targets][3 layers][2 dirs][2: h, c][hidden/2] floats. */
size_t umx_hip_stream_floats(const umx_hip_ctx *ctx);
int umx_hip_stream_reset(umx_hip_ctx *ctx);                 /* create_lstm_data / umx_lstm_set_zero */
int umx_hip_stream_get(umx_hip_ctx *ctx, float *host_dst);  /* checkpoint / multi-GPU hand-off */
int umx_hip_stream_set(umx_hip_ctx *ctx, const float *host_src);
/* The same per track lane (the three above address lane 0); reset with track < 0 clears every lane. */
int umx_hip_track_stream_reset(umx_hip_ctx *ctx, int track);
int umx_hip_track_stream_get(umx_hip_ctx *ctx, int track, float *host_dst);
int umx_hip_track_stream_set(umx_hip_ctx *ctx, int track, const float *host_src);

/* NON-FINITE INPUT.  Audio is data: a NaN, a +-inf, or finite samples so large that they overflow inside the engine (3e38 does, in
 * the STFT) are no error.  What they may touch is the lane, the call and the track they came in with, and nothing else, bit for bit
 * (tests/test_gpu_poisoned_lanes.py):
 *   1. CONTAINMENT.  In any call, a lane whose audio holds such samples changes no bit of any other lane's outputs or of any other
 *      lane's carried LSTM state.  The call returns UMX_OK and launches what the call without those samples launches: the same
 *      recurrence (umx_hip_lstm_kernel_name, _lstm_was_persistent, _lstm_mode), the same GEMMs (umx_hip_gemm_kernel_name); the
 *      hand-off of the persistent recurrences goes by tags, never by values, so no timeout recovery is triggered.
 *   2. RECOVERY.  That lane's own outputs and its own LSTM state behind the call are UNSPECIFIED (they need not even be non-finite:
 *      the clamps of the gate functions and the ReLUs may swallow a NaN).  Once umx_hip_track_stream_reset(ctx, lane) -- on a
 *      one-track context umx_hip_stream_reset -- has cleared that lane's state, every later call on the context gives every lane,
 *      that one included, the bits it would have had if the call had never run: whatever n, lane set, target set, Wiener
 *      iteration count or filter the later calls use, and in whichever pipeline slot they land.  The track queue's admission of a
 *      job performs that reset.
 *   3. WHOLE TRACKS.  In umx_hip_separate_tracks* and umx_hip_separate_queue* a track with such samples changes no bit of any other
 *      track's outputs or measurement records (levels, loudness, hop energies, true peak) -- not of the tracks beside it, not of
 *      the job that takes its lane next, at any sample rate.  Its own record's `nonfinite` counts what its outputs hold. */

/* umx_inference (inference.cpp:12-207): one segment -> 4 stems.
 * audio: n interleaved stereo frames (2,n), 1 <= n <= segment_samples.  out[t]: (2,n) each.
 * Host-pointer form: H2D + kernels + D2H, synchronous (umx_inference returns its outputs). */
int umx_hip_infer_segment(umx_hip_ctx *ctx, const float *audio_host, int n, float *const out_host[4],
                          unsigned flags);
/* The same without the final wait: H2D and kernels are queued on the stream of the pipeline slot the segment runs in
 * (consecutive calls go round the slots), the D2H on a copy stream behind them.  With PINNED host buffers, and distinct
 * buffers for umx_hip_pipeline_depth() consecutive calls, one segment's transfers overlap the others' kernels.  Results
 * are valid after umx_hip_sync.
 * BUFFER CONTRACT: audio_host and out_host of every call queued since the last umx_hip_sync must stay valid and
 * unchanged until that sync returns -- the timeout recovery described there uploads the audio again. */
int umx_hip_infer_segment_async(umx_hip_ctx *ctx, const float *audio_host, int n, float *const out_host[4],
                                unsigned flags);
/* Device-pointer form: buffers already in HBM (audio 2*n floats, out[t] 2*n floats each); asynchronous.
 * ORDERING CONTRACT: consecutive calls are queued round-robin on umx_hip_pipeline_depth() internal streams (the
 * cross-segment pipeline), so (1) audio_dev and out_dev must stay untouched by the caller until umx_hip_sync -- or until
 * the caller's stream has been ordered behind the engine with umx_hip_order_before; (2) umx_hip_pipeline_depth()
 * CONSECUTIVE calls must be given DISTINCT out_dev buffers (that many segments are in flight together); (3) work the caller queued on a stream
 * of its own that produces audio_dev is ordered in front of the next call with umx_hip_order_after.
 * A caller that fences with umx_hip_order_before (and then recycles its buffers) gives up the timeout recovery for the
 * calls queued so far: a persistent-kernel timeout among them is reported as UMX_ERR_TIMEOUT by the next umx_hip_sync.
 * Track-batched contexts (umx_hip_create_tracks with more than one lane) run the KERNELS of consecutive calls one after the
 * other (their workgroups take whole CUs: side by side they only wait for each other); the slots' streams still let a
 * call's uploads and downloads run beside another call's kernels, and the contract above is unchanged. */
int umx_hip_infer_segment_device(umx_hip_ctx *ctx, const float *audio_dev, int n, float *const out_dev[4],
                                 unsigned flags);
/* One segment of each of n_tracks track lanes (lane i = the i-th track of the context, its LSTM state carries from
 * call to call): audio[i] = (2,n[i]) interleaved or NULL for a lane that sits this call out (its state is kept),
 * out[4*i + t] = stem t of track i.  Same three forms and the same ordering contract as above. */
int umx_hip_infer_batch(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *n,
                        float *const *out_host, unsigned flags);
int umx_hip_infer_batch_async(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *n,
                              float *const *out_host, unsigned flags);
int umx_hip_infer_batch_device(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_dev, const int *n,
                               float *const *out_dev, unsigned flags);
/* UMX_FLAG_RESIDUAL: the slot that carries the residual source = the lowest skipped target; -1 when the flag is not set, -2 for a
 * combination the entry points refuse (no target skipped, or all four).  Host arithmetic. */
int umx_hip_residual_slot(unsigned flags);
/* Waits for everything queued.  A persistent LSTM launch needs its whole grid co-resident; inside a process that is
 * guaranteed (launches of all contexts on a device pass one admission gate), but another PROCESS on the same GPU can
 * still occupy the CUs, in which case the launch gives up after a bounded spin instead of hanging.  umx_hip_sync then
 * RECOVERS: the stream state of every lane is restored to what it was before the first segment queued since the last
 * sync (a per-layer copy is kept for up to 8 queued calls), those segments are run again with the per-step driver
 * (bit-identical), and later calls of this context use that driver.  UMX_OK after a recovery; umx_hip_last_error then
 * starts with "recovered".  UMX_ERR_TIMEOUT (streaming state reset to zero) only when recovery is impossible: more
 * than 8 calls were queued since the last sync, or umx_hip_order_before released the caller's buffers of those calls.
 * The stream-state entry points (umx_hip_[track_]stream_{reset,get,set}) synchronise through this function, so a
 * sequence infer(A); stream_set; infer(B) replays A before the state is changed and B after it, never across it. */
int umx_hip_sync(umx_hip_ctx *ctx);
/* hip_stream = a hipStream_t of the caller.  order_after: everything queued by LATER calls on this context starts
 * only after what is on hip_stream now.  order_before: hip_stream waits for everything queued on the context so far. */
int umx_hip_order_after(umx_hip_ctx *ctx, void *hip_stream);
int umx_hip_order_before(umx_hip_ctx *ctx, void *hip_stream);
void *umx_hip_stream_handle(umx_hip_ctx *ctx); /* the internal hipStream_t the most recent segment was queued on */

/* The whole track on the device: shift_inference (umx.cpp:99-150) around split_inference (umx.cpp:152-295).
 * One upload of the (2,length) interleaved track, the 60 s segments (stride 0.75 * segment_samples,
 * umx.cpp:181) queued back to back so that consecutive segments overlap in the engine's two pipeline slots,
 * the triangular-weight overlap-add (umx.cpp:197-260) and the division by the weight sum (umx.cpp:264-273)
 * in HBM, one download of the 4 stems.  Resets the streaming state first (umx.cpp:167-171).  Bit-identical to
 * umx_split_inference / umx_shift_inference of umx_host.h driving umx_hip_infer_segment; sum_weight is zeroed
 * (SURVEY F4).  offset: samples of leading silence inside the MAX_SHIFT buffer (umx.cpp:115); < 0 = the
 * reference's unseeded rand() % 22050 = UMX_REFERENCE_SHIFT.  progress (may be NULL) is called once per QUEUED segment. */
#define UMX_MAX_SHIFT 22050 /* inference.hpp:14 MAX_SHIFT_SECS * 44100 */
/* umx.cpp:115 draws rand() % 22050 and the reference never seeds rand(): with glibc every run of its CLI shifts by these
 * 4033 samples.  "offset < 0" below means THIS value, not a call of rand() here -- in a process that links the HIP runtime
 * (or anything else that draws from rand() first) the first rand() is no longer the reference's (found by a test, round 3). */
#define UMX_REFERENCE_SHIFT 4033
int umx_hip_split_inference(umx_hip_ctx *ctx, const float *audio_host, int length, float *const out_host[4],
                            unsigned flags, void (*progress)(float, void *), void *progress_user);
int umx_hip_shift_inference(umx_hip_ctx *ctx, const float *audio_host, int length, int offset, float *const out_host[4],
                            unsigned flags, void (*progress)(float, void *), void *progress_user);

/* The same for n_tracks tracks at once, one per track lane of a context made by umx_hip_create_tracks: call s of the
 * segment loop runs segment s of EVERY track that still has one (their LSTM recurrences share one launch per layer),
 * a finished track's lane sits idle.  audio_host[i] (2,length[i]), out_host[4*i + t] (2,length[i]); shift_offset[i] < 0:
 * split_inference, >= 0: shift_inference with that offset.  Track i's stems are bit-identical to running it alone on a
 * context with the batched LSTM kernel. */
int umx_hip_separate_tracks(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *length,
                            const int *shift_offset, float *const *out_host, unsigned flags, void (*progress)(float, void *),
                            void *progress_user);

/* Any sample rate: Open-Unmix's preprocess resamples its input to the model's 44.1 kHz with torchaudio's default
 * windowed-sinc filter (sinc_interp_hann: 6 zero crossings, rolloff 0.99).  Here that filter runs on the device, into 44.1 kHz and
 * back out.  For rates r_in -> r_out (8000 .. 192000 Hz) with g = gcd, M = r_in / g, L = r_out / g, b = 0.99 min(M, L), W = 6:
 *     y[j] = sum_i x[i] (b / M) k(b (i / M - j / L)),  k(t) = sinc(t) cos^2(pi t / 2W) for |t| < W, else 0,
 * each channel on its own, x zero outside [0, n_in), no delay, y defined for every j >= 0.  Each output is the fp32 sum of its
 * taps (an fp32 table of L phases x K = 2D + 2 taps, D = ceil(W M / b), built in double) in a fixed order: launches of one or
 * four buffers give the same bits. */
#define UMX_RESAMPLE_MIN_RATE 8000
#define UMX_RESAMPLE_MAX_RATE 192000
/* the natural output length ceil(n L / M) (torchaudio's target_length); < 0 for a rate outside the range.  Host arithmetic. */
long long umx_hip_resampled_length(long long n, int rate_in, int rate_out);
/* n_buffers (1 .. 4) device buffers (2, n_in) -> (2, n_out), queued on hip_stream; writes exactly n_out frames of each output.
 * n_out may differ from the natural length: beyond it the formula goes on (a decaying tail, then zeros). */
int umx_hip_resample_device(umx_hip_ctx *ctx, int rate_in, int rate_out, int n_buffers, const float *const *in_dev, int n_in,
                            float *const *out_dev, int n_out, void *hip_stream);
/* Ranges.  Output j reads the input frames c - D .. c + D + 1, c = floor(j M / L): that is its whole window, zero taps
 * included, and nothing else decides its bits.  So a range of the outputs resampled on its own is, bit for bit, that range of the
 * whole launch, and the two directions of the rule are host arithmetic in 64-bit integers:
 *   umx_hip_resample_needs  the number of leading input frames that outputs [0, n_out_wanted) read: 0 for n_out_wanted == 0, else
 *                           min(n_in, floor((n_out_wanted - 1) M / L) + D + 2)
 *   umx_hip_resample_ready  the number of leading output frames whose whole window lies inside the first n_in_final input frames:
 *                           n_out if n_in_final >= n_in (beyond n_in the input is zeros), else ceil((n_in_final - D - 1) L / M)
 *                           clamped to 0 .. n_out (0 for n_in_final <= D + 1)
 * Both return < 0 for a rate outside the range or a negative count.  needs(ready(f)) <= f and ready(needs(w)) >= w. */
long long umx_hip_resample_needs(long long n_out_wanted, int rate_in, int rate_out, long long n_in);
long long umx_hip_resample_ready(long long n_in_final, int rate_in, int rate_out, long long n_in, long long n_out);
/* umx_hip_resample_device for the frames [first, first + count) of each n_out-frame output: it writes those frames and nothing
 * else, with the bits the whole call gives them; n_in and n_out are still the whole buffers' lengths.  count == 0 launches nothing.
 * `first` must be even (every 16-byte store stays as aligned as the whole call keeps it); UMX_ERR_ARG for an odd or negative first,
 * count < 0, first + count > n_out, and whatever umx_hip_resample_device refuses. */
int umx_hip_resample_range_device(umx_hip_ctx *ctx, int rate_in, int rate_out, int n_buffers, const float *const *in_dev, int n_in,
                                  float *const *out_dev, int n_out, int first, int count, void *hip_stream);
/* resampler launches of the context's last whole-track call or queue run: `forward` into 44.1 kHz, `backward` out of it (a
 * whole-buffer launch counts as one; a call without a resampled track gives 0 and 0).  UMX_ERR_ARG when there has been none. */
int umx_hip_debug_resample_launches(umx_hip_ctx *ctx, int *forward, int *backward);
/* umx_hip_shift_inference / umx_hip_separate_tracks for tracks at `rate`: the stems come back with the caller's length at the
 * caller's rate, aligned sample for sample with the input.  The track is resampled to n44 = umx_hip_resampled_length(length,
 * rate, 44100) frames, separated exactly as umx_hip_shift_inference / _separate_tracks separate n44 frames at 44.1 kHz
 * (offset / shift_offset count 44.1 kHz samples, same meaning), and the four stems (those n44 frames, zero outside them) are
 * resampled back: bit for bit that composition.  A track at 44100 is not resampled: bitwise today's entry points.  A rate outside
 * 8000 .. 192000 is UMX_ERR_ARG.  A resampled track goes in and out range by range: the native frames a segment's
 * 44.1 kHz frames read (umx_hip_resample_needs) go up and through the resampler with the call that needs them, and behind every
 * finished region the frames at the caller's rate that it completes (umx_hip_resample_ready) are resampled back and downloaded
 * while later segments run -- the same bits.  A rescaled track (UMX_CLIP_RESCALE) and the shift ensemble still leave whole. */
int umx_hip_shift_inference_rate(umx_hip_ctx *ctx, const float *audio_host, int length, int rate, int offset, float *const out_host[4],
                                 unsigned flags, void (*progress)(float, void *), void *progress_user);
int umx_hip_separate_tracks_rate(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *length, const int *rate,
                                 const int *shift_offset, float *const *out_host, unsigned flags, void (*progress)(float, void *),
                                 void *progress_user);
/* Shift ensemble: the "shift trick" with K offsets instead of one (Demucs --shifts=K).  ONE track is separated at K
 * shift offsets, shift k as track lane k of ONE pass over the segments, and the K results are averaged on the device.  With s_k[t] the
 * `length` frames of stem t that umx_hip_separate_tracks returns for lane k when every lane is given this track, lane k at
 * shift_offset[k] = offsets[k], with these flags, the result is, per channel and sample, in fp32
 *     out[t] = (((s_0 + s_1) + s_2) + ... + s_{K-1}) / (float)K
 * summed left to right in the order of `offsets`, one correctly rounded division.  K = 1 is umx_hip_shift_inference(_rate) with
 * offsets[0], the same call, on any context; two equal offsets give that single-shift result bit for bit.  The track is uploaded
 * once (and, at another rate, resampled once), placed into the other lanes device to device, nothing is downloaded before the mean
 * (taken at 44.1 kHz; its four buffers are resampled back once), and the four stems come back in one download of exactly `length`
 * frames each.  1 <= n_shifts <= umx_hip_n_tracks(ctx); offsets: n_shifts values in [0, UMX_MAX_SHIFT), duplicates allowed, NULL =
 * umx_hip_ensemble_offsets(n_shifts, -1); rate: 44100, or 8000 .. 192000 as umx_hip_shift_inference_rate.  Every flag goes to every
 * lane unchanged, except UMX_FLAG_RESET_SEGMENTS, which is refused (the lanes are taken).  UMX_ERR_ARG for arguments outside this. */
#define UMX_MAX_SHIFTS UMX_MAX_TRACKS
/* k-th default offset, host arithmetic, no context: (first + k * (UMX_MAX_SHIFT / n_shifts)) % UMX_MAX_SHIFT; first < 0 means
 * UMX_REFERENCE_SHIFT.  n_shifts == 1 gives { first }.  UMX_ERR_ARG for n_shifts outside 1 .. UMX_MAX_SHIFTS or first >= UMX_MAX_SHIFT. */
int umx_hip_ensemble_offsets(int n_shifts, int first, int *offsets_out);
int umx_hip_shift_ensemble(umx_hip_ctx *ctx, const float *audio_host, int length, int rate, int n_shifts, const int *offsets,
                           float *const out_host[4], unsigned flags, void (*progress)(float, void *), void *progress_user);
/* measuring: milliseconds shift_mean_kernel took in the context's last ensemble call with n_shifts > 1 (device events around its
 * launch); < 0 when there has been none. */
float umx_hip_debug_shift_mean_ms(umx_hip_ctx *ctx);
/* Stem mix matrix: weighted sums of the stems and of the input mixture, formed on the device, so that only the outputs
 * a caller wants cross PCIe -- Open-Unmix's aggregate_dict ("accompaniment" = drums + bass + other), Demucs' --two-stems, karaoke
 * ("mixture minus vocals", which is NOT the sum of the other three: Wiener stems do not add up to the mix), rebalancing ("vocals -6 dB").
 * A mix is n_out rows (1 .. UMX_MAX_MIX_OUTPUTS) of five fp32 gains, gains[m * 5 + c]:
 *     c = 0 .. 3   the four output slots exactly as the unmixed call with the same flags returns them (a residual slot and a skipped
 *                  target's slot of zeros included)
 *     c = 4        the input mixture; for a track at another sample rate its 44.1 kHz version (the mix is formed at 44.1 kHz, then
 *                  the n_out buffers are resampled back)
 * Per output m, channel and sample, in fp32: the terms are the columns with gains[m][c] != 0.0f in ascending c; each term is the
 * correctly rounded product g * s_c; the terms are added left to right, one rounding per addition; the first term is the product
 * itself (not 0 + product); there is no fused multiply-add; a row without a nonzero gain gives +0.0f.  A zero gain (+0 or -0) means
 * the column is not read: an inf or NaN there does not reach the output.  Gains must be finite, else UMX_ERR_ARG.  The identity
 * matrix returns the unmixed call's four stems bit for bit; a 0/1 row equals ((s_a + s_b) + s_c) of the downloaded stems in fp32.
 * Not offered by the multi-GPU driver (umx_mgpu.h), as the ensemble is not. */
#define UMX_MAX_MIX_OUTPUTS 4
#define UMX_MIX_COLUMNS 5
#define UMX_MIX_COLUMN_MIXTURE 4
/* host arithmetic, no context: the bitmask of the columns with any nonzero gain (bit 4: the mixture); -1 for n_out outside
 * 1 .. UMX_MAX_MIX_OUTPUTS, gains == NULL or a gain that is not finite */
int umx_hip_mix_columns(int n_out, const float *gains);
/* umx_hip_separate_tracks(_rate) with the mix behind it: out_host[n_out * i + m] (2,length[i]) is output m of track i; one matrix for
 * every lane.  rate == NULL: every track at 44100; shift_offset[i] < 0: split inference; n_tracks == 1 covers umx_hip_split_inference,
 * _shift_inference and _shift_inference_rate.  At 44.1 kHz the mix of a finished region is formed right behind its normalisation,
 * over the region's stems, and only the n_out buffers are downloaded, region by region; column 4 is the lane's own copy of the
 * input (the shift padding is never downloaded).  UMX_FLAG_RESET_SEGMENTS as for the unmixed call. */
int umx_hip_separate_tracks_mix(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *length, const int *rate,
                                const int *shift_offset, int n_out, const float *gains, float *const *out_host, unsigned flags,
                                void (*progress)(float, void *), void *progress_user);
/* umx_hip_shift_ensemble with the mix applied to the MEAN (column 4: the track), at 44.1 kHz, before the n_out buffers are
 * resampled back and downloaded; out_host: n_out buffers (2,length) */
int umx_hip_shift_ensemble_mix(umx_hip_ctx *ctx, const float *audio_host, int length, int rate, int n_shifts, const int *offsets, int n_out,
                               const float *gains, float *const *out_host, unsigned flags, void (*progress)(float, void *),
                               void *progress_user);
/* the kernel on the caller's device buffers, queued on hip_stream (per-segment callers, tests): stems_dev[c] and mix_dev are (2,n)
 * interleaved, float2-aligned, and may be NULL when no row uses their column (stems_dev itself too); UMX_ERR_ARG when a used
 * column's pointer is NULL.  Writes exactly n frames of each of the n_out buffers of out_dev.  out_dev[m] == stems_dev[m] is allowed
 * (every used input of a frame is read before any output of that frame is stored); other overlaps are not. */
int umx_hip_mix_stems_device(umx_hip_ctx *ctx, int n_out, const float *gains, const float *const stems_dev[4], const float *mix_dev, int n,
                             float *const *out_dev, void *hip_stream);
/* Track queue: a catalogue job -- more tracks than track lanes, of different lengths -- through ONE run of the segment
 * loop.  umx_hip_separate_tracks takes at most umx_hip_n_tracks tracks and a finished track's lane sits idle until the longest one
 * ends; here a lane is refilled with the next job the moment its track ends.  Every job's `out` is, bit for bit, what
 * umx_hip_separate_tracks (gains == NULL: four stems) or umx_hip_separate_tracks_mix (n_out, gains as that call takes them: n_out
 * buffers) returns for that ONE track on this context with these flags; every per-call flag goes to every job.
 * The schedule (umx_hip_queue_plan is its one statement in code; the driver walks the same object):
 *   - before each call of the segment loop every lane without a track asks `next` for one, in ascending lane order;
 *   - a job of S = ceil(padded length / stride) segments (padded length: length for shift_offset < 0, else length +
 *     max(UMX_MAX_SHIFT - shift_offset, shift_offset); stride = 0.75 segment_samples) holds its lane for S consecutive calls;
 *   - once `next` has returned 0 it is not called again; the run ends when no lane holds a track.
 * Both callbacks run on the caller's thread, inside the call.  done(j) comes after the last byte of job j is in its buffers; `audio` and
 * `out` of a job must stay valid from `next` to `done`.  done is called exactly once per job taken -- on an error return too, for
 * the jobs already complete, and only for those (a job in flight then is abandoned: its buffers hold anything).
 * UMX_ERR_ARG, with umx_hip_last_error naming the reason, for UMX_FLAG_RESET_SEGMENTS (the lanes are taken), a context that is not
 * track-batched (umx_hip_lstm_is_batched: a job's bits must not depend on its lane), a job with length < 1, shift_offset >=
 * UMX_MAX_SHIFT or a NULL buffer, and `next` returning < 0; the context stays usable.  A persistent-kernel timeout: as
 * umx_hip_separate_tracks, the jobs in flight are run again from their first segment, once (the run then makes more calls than the
 * plan); a second timeout is UMX_ERR_TIMEOUT.  A job may be at any sample rate umx_hip_separate_tracks_rate takes (`rate`): it
 * is bit for bit that call's result for the one track, holds its lane for the segments of its 44.1 kHz version (S above from
 * umx_hip_resampled_length(length, rate, 44100)), and a rate outside 8000 .. 192000 is UMX_ERR_ARG.  The shift ensemble is not offered
 * here, and the multi-GPU driver (umx_mgpu.h) does not offer the queue. */
typedef struct umx_queue_job
{
    const float *audio;                   /* (2,length) interleaved, at `rate` */
    int length, shift_offset;             /* as umx_hip_separate_tracks: < 0 split, >= 0 shift */
    float *out[UMX_MAX_MIX_OUTPUTS];      /* n_out buffers (2,length); 4 stems when gains == NULL */
    void *tag;                            /* the caller's, untouched */
    int rate;                             /* 0 or 44100: not resampled; else 8000 .. 192000: length and out are at this rate.  The struct is
                                             zeroed before `next`, so a caller that never sets it has 44.1 kHz jobs */
} umx_queue_job;
typedef int (*umx_queue_next_fn)(void *user, umx_queue_job *job);        /* 1: *job filled in, 0: no more jobs, < 0: stop with UMX_ERR_ARG */
typedef void (*umx_queue_done_fn)(void *user, const umx_queue_job *job); /* job's out buffers are complete */
int umx_hip_separate_queue(umx_hip_ctx *ctx, umx_queue_next_fn next, umx_queue_done_fn done, void *user, int n_out, const float *gains,
                           unsigned flags);
/* host arithmetic, no context: the schedule above for n_jobs jobs of seg_count[j] >= 1 calls each on n_lanes (1 .. UMX_MAX_TRACKS)
 * lanes: job j's lane, the call its first segment runs in, and the number of calls (each output may be NULL).  UMX_ERR_ARG otherwise. */
int umx_hip_queue_plan(int n_lanes, int n_jobs, const int *seg_count, int *lane_out, int *first_call_out, int *n_calls_out);
/* calls of the segment loop (infer_batch) the context's last queue run made; < 0 when there was none */
int umx_hip_debug_queue_calls(umx_hip_ctx *ctx);
/* 16-bit PCM in and out of the whole-track drivers.  Almost all audio is 16-bit PCM: kept as int16 across PCIe it is 4 B
 * per stereo frame up instead of 8 and 4 B per output buffer and frame down instead of 8, converted on the device.  The rules, to the bit:
 *   decode   x = (float)q / 32767.0f, the correctly rounded fp32 quotient -- what umx_wav_load gives for a 16-bit file, so an int16
 *            upload runs on the bits the float loader would have produced
 *   encode   of output buffer m (its index in the call's `out` list, 0 .. 3), channel ch, frame k of the CALLER's track at the
 *            caller's rate (k starts at 0; not a position in a region or in the padded signal):
 *                v = x * 32767.0f                      one fp32 rounding, no fused multiply-add
 *                if dither: v = v + d(seed, m, ch, k)  one fp32 rounding
 *                r = rintf(v)                          nearest, ties to even
 *                q = r is NaN ? 0 : (int16) min(max(r, -32768.f), 32767.f)
 *   dither   TPDF, deterministic and counter based, so that regions, lanes and a rerun after a timeout give the same bits: with
 *            h(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 in uint32,
 *                a = h(seed + 0x9e3779b9 * (2 m + ch + 1)),  w = h(a ^ (uint32) k),
 *                d = (((float)(w & 0xffff) + (float)(w >> 16)) - 65535.0f) * (1.0f / 65536.0f), in (-1, 1), every step exact.
 * encode(decode(q)) == q for every code without dither, within 1 LSB with it.
 * The _io forms below are the calls they are named after with the formats of the host buffers chosen per call; io == NULL, or
 * UMX_SAMPLE_F32 both ways, IS that call: the same launches, nothing allocated.  UMX_SAMPLE_S16 in: audio[i] points at length[i]
 * interleaved int16 stereo frames; out: every output buffer receives exactly length[i] such frames.  On the device a format costs 4 B
 * per frame of the track for the input and 4 B per frame and output buffer, only while it is used.  UMX_ERR_ARG, naming the reason
 * and leaving the context usable, for a format that is none of UMX_SAMPLE_F32, _S16 and _S24 (below), for dither != 0 with an fp32 output and for a NULL buffer.
 * Reset mode, other sample rates (the dither is indexed at the caller's rate), the mix matrix (gains == NULL: the four stems, n_out
 * ignored) and every per-call flag work as in the fp32 calls.  The shift ensemble, the multi-GPU driver (umx_mgpu.h) and the
 * per-segment infer calls do not offer the formats. */
#define UMX_SAMPLE_F32 0
#define UMX_SAMPLE_S16 1
typedef struct umx_sample_io
{
    int in_format, out_format; /* UMX_SAMPLE_* of the audio and of the output buffers */
    int dither;                /* != 0: TPDF dither before the rounding (UMX_SAMPLE_S16 and UMX_SAMPLE_S24 outputs only) */
    unsigned dither_seed;
} umx_sample_io;
/* umx_hip_separate_tracks_mix (rate == NULL: 44100 for all; gains == NULL: umx_hip_separate_tracks_rate) with the formats */
int umx_hip_separate_tracks_io(umx_hip_ctx *ctx, int n_tracks, const void *const *audio_host, const int *length, const int *rate,
                               const int *shift_offset, int n_out, const float *gains, void *const *out_host, unsigned flags,
                               const umx_sample_io *io, void (*progress)(float, void *), void *progress_user);
/* umx_hip_separate_queue with the formats: a job's audio and out[] are read as io says (the caller casts its int16 pointers) */
int umx_hip_separate_queue_io(umx_hip_ctx *ctx, umx_queue_next_fn next, umx_queue_done_fn done, void *user, int n_out, const float *gains,
                              unsigned flags, const umx_sample_io *io);
/* the two kernels on the caller's device buffers, queued on hip_stream: n int16 stereo frames (4-byte aligned) <-> (2,n) interleaved
 * fp32 (8-byte aligned); exactly n frames of every output are written.  Encode: 1 .. 4 buffers in one launch, buffer b is output b
 * of the rule above, its frame i frame first_frame + i; of io only dither and dither_seed are read (NULL: no dither). */
int umx_hip_pcm16_decode_device(umx_hip_ctx *ctx, const int16_t *in_dev, int n, float *out_dev, void *hip_stream);
int umx_hip_pcm16_encode_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                                const umx_sample_io *io, int16_t *const *out_dev, void *hip_stream);
/* the same rules on the host (no GPU, no context): n_values samples; n_frames stereo frames of output buffer `buffer` */
int umx_hip_pcm16_decode_host(const int16_t *q, long long n_values, float *x);
int umx_hip_pcm16_encode_host(const float *x, int n_frames, int buffer, long long first_frame, const umx_sample_io *io, int16_t *q);
/* Packed 24-bit PCM in and out of the same calls: UMX_SAMPLE_S24 on either side of a umx_sample_io, in any combination
 * with the two formats above.  Masters, stems handed to a mixer and most sources that are not 16-bit are 24-bit files; packed they
 * are 6 B per stereo frame each way, and 24-bit is the one integer format that fp32 carries without loss.  The rules, to the bit:
 *   layout   a sample is 3 bytes, little-endian, two's complement; a stereo frame is 6 bytes, L then R, exactly as a WAV data chunk
 *            holds it.  A buffer is length x 6 bytes.  A DEVICE buffer must be 2-byte aligned (frames are 6 bytes, so an even base
 *            is all it takes); the device entry points refuse an odd address with UMX_ERR_ARG.
 *   decode   x = (float)q * 2^-23, that is q / 8388608.f: exact, and what umx_wav_load gives for a 24-bit file, so a packed upload
 *            runs on the bits the float loader would have produced
 *   encode   of output buffer m, channel ch, frame k of the caller's track (as above):
 *                v = x * 8388608.0f                                       exact short of overflow
 *                r = rint((double)v + (dither ? (double)d(seed, m, ch, k) : 0.0))   the sum in double, ONE rounding (ties to even)
 *                q = r is NaN ? 0 : min(max(r, -8388608), 8388607)
 *            The sum is formed in double because at |v| >= 2^22 an fp32 v + d falls on a 0.5 grid before the rounding (rintf of the
 *            fp32 sum differs from this rule for 2.79 M of the 2^24 codes); the double sum is exact for every finite v below 2^24.
 *   dither   the d of the int16 rule: the same hash, the same keys (seed, m, ch), the same frame index k of the caller's track at the
 *            caller's rate; here it lies in (-1, 1) LSB of the 24-bit grid
 * encode(decode(q)) == q for all 2^24 codes without dither, within 1 LSB with it.  Full scale: the decode divides by 2^23 (the
 * loader's scale), so the largest code is (2^23 - 1) / 2^23 < 1 and +1.0f encodes to 8388607 AND counts as clipped (-1.0f is code
 * -8388608, not clipped).  clipped[m] of umx_levels, for a UMX_SAMPLE_S24 output: the samples with r > 8388607 or r < -8388608, r
 * with the dither term and over the rescale divisor, exactly as for int16; the divisor rule is unchanged, and with a finite peak
 * |v| <= 2^23 / 1.01 up to rounding (8305552.5), so nothing clamps and clipped is 0.  dither != 0 with an fp32 output stays refused.
 * On the device a format costs 6 B per frame of the track for the input and 6 B per frame and output buffer, only while it is used.
 * The kernels on the caller's device buffers, queued on hip_stream: n packed frames (2-byte aligned) <-> (2,n) interleaved fp32
 * (8-byte aligned); exactly 6 n bytes of every packed output are written and no neighbouring byte is touched.  Encode: as
 * umx_hip_pcm16_encode_device; encode_rescaled: as umx_hip_pcm16_encode_rescaled_device below (on x / g, adds what it clamps to
 * acc_dev's clipped).  The host forms: n_values samples of 3 bytes; n_frames stereo frames of output buffer `buffer`. */
#define UMX_SAMPLE_S24 3
int umx_hip_pcm24_decode_device(umx_hip_ctx *ctx, const void *in_dev, int n, float *out_dev, void *hip_stream);
int umx_hip_pcm24_encode_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                                const umx_sample_io *io, void *const *out_dev, void *hip_stream);
int umx_hip_pcm24_decode_host(const void *q, long long n_values, float *x);
int umx_hip_pcm24_encode_host(const float *x, int n_frames, int buffer, long long first_frame, const umx_sample_io *io, void *q);
/* Output levels and clip handling.  A separated stem is not bounded by the mixture: Wiener stems of a track mastered to
 * full scale, or a mix row such as mix - 0.5 vocals, pass 1.0, and the int16 encode clamps.  The levels of what leaves are measured
 * on the device, where every output frame is final before it is encoded or copied.  The rules, to the bit:
 *   levels of output buffer m, over both channels of the `length` frames that leave for the caller -- at the caller's rate, behind
 *   the mix, before any encode and before any rescale:
 *     peak[m]        the largest |x| over the samples that are not NaN (+inf counts: the peak is then inf); 0 when there is none.
 *                    Exact: an unsigned integer maximum over the bit patterns of |x|.
 *     over_unity[m]  the number of samples with |x| > 1.0f (NaN is not one of them, +-inf is)
 *     nonfinite[m]   the number of samples that are NaN or +-inf
 *     clipped[m]     0 for an fp32 output; for a UMX_SAMPLE_S16 output the number of samples whose rounded value r of the encode rule
 *                    above is > 32767.f or < -32768.f, that is, where the clamp changed the value.  r includes the dither term when
 *                    dither is on and the rescale divisor when rescale is on; +-inf is counted, NaN is not (it is in nonfinite).
 *   All four are maxima or integer counts: they do not depend on how the track is cut into regions, which lane a job rides in, the
 *   queue, reset mode or a rerun after a timeout.  (A sum of squares has no such form unless it is tied to fixed hops: umx_loudness below.)
 *   rescale (UMX_CLIP_RESCALE): one divisor per track, common to all of its outputs (the stems still add up to the mixture over it;
 *   Demucs' rescale is per file).  P = the maximum of peak[m] over the outputs that leave; g = 1.01f * P, one fp32 product.  If P is
 *   not finite, or if !(g > 1.0f), the divisor is 1 and the output is, bit for bit, the clamp-mode output.  Otherwise every sample
 *   becomes x / g, the correctly rounded fp32 quotient; for a UMX_SAMPLE_S16 output the unchanged encode rule follows (dither as
 *   before), for an fp32 output the quotient is what leaves.  With a finite P nothing clamps afterwards (|x / g| <= 1 / 1.01 up to
 *   rounding, |v| < 32443, the dither is below 1 in size): clipped is then 0.  The divisor is formed on the device from the peak
 *   words; it is reported as `gain` (1 in clamp mode).
 * The shift ensemble, the multi-GPU driver (umx_mgpu.h) and the per-segment umx_hip_infer_* calls do not offer levels or rescale. */
#define UMX_CLIP_CLAMP 0
#define UMX_CLIP_RESCALE 1
typedef struct umx_levels_acc /* the device record: zero it, let launches accumulate, copy it back */
{
    unsigned peak_bits[4]; /* bit pattern of peak[m] */
    unsigned long long over_unity[4], clipped[4], nonfinite[4];
} umx_levels_acc;
typedef struct umx_levels /* what a whole-track call reports per track */
{
    float peak[4];
    float gain;
    int n_out;
    unsigned long long over_unity[4], clipped[4], nonfinite[4];
} umx_levels;
/* umx_hip_separate_tracks_io with a clip mode and levels: n_tracks records, or NULL.  clip_mode == UMX_CLIP_CLAMP and levels == NULL
 * IS the _io call: the same launches, nothing allocated.  Clamp mode with levels adds one measuring launch per finished region; a
 * rescaled track leaves whole behind its last segment (mix, levels, rescaled encode or in-place division, one download per output).
 * UMX_ERR_ARG, naming the reason and leaving the context usable, for an unknown clip_mode and for everything the _io call refuses. */
int umx_hip_separate_tracks_levels(umx_hip_ctx *ctx, int n_tracks, const void *const *audio_host, const int *length, const int *rate,
                                   const int *shift_offset, int n_out, const float *gains, void *const *out_host, unsigned flags,
                                   const umx_sample_io *io, int clip_mode, umx_levels *levels, void (*progress)(float, void *),
                                   void *progress_user);
/* umx_hip_separate_queue_io with a clip mode; every job is measured and its done callback receives the record, valid during the
 * callback only.  A rescaled job is one whole-track region queued with its last segment. */
typedef void (*umx_queue_levels_fn)(void *user, const umx_queue_job *job, const umx_levels *levels);
int umx_hip_separate_queue_levels(umx_hip_ctx *ctx, umx_queue_next_fn next, umx_queue_levels_fn done, void *user, int n_out,
                                  const float *gains, unsigned flags, const umx_sample_io *io, int clip_mode);
/* the kernels on the caller's device buffers ((2,n) interleaved fp32, 8-byte aligned), queued on hip_stream; acc_dev: a
 * umx_levels_acc in device memory that the caller has zeroed, launches accumulate into it.
 * levels: buffer b of 1 .. 4 is output b, its frame i frame first_frame + i; io == NULL or an fp32 out_format: clipped stays as it
 * is, else the clamped samples of that format's plain encode are counted with io's dither.  Exactly the record is written.
 * pcm16_encode_rescaled: the encode of umx_hip_pcm16_encode_device on x / g, g formed from acc_dev's peak words by the rule; the
 * samples it clamps (possible only where the divisor is 1) are added to acc_dev's clipped.  rescale: x / g in place (nothing is
 * written where the divisor is 1). */
int umx_hip_levels_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                          const umx_sample_io *io, umx_levels_acc *acc_dev, void *hip_stream);
int umx_hip_pcm16_encode_rescaled_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                                         const umx_sample_io *io, int16_t *const *out_dev, umx_levels_acc *acc_dev, void *hip_stream);
int umx_hip_pcm24_encode_rescaled_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                                         const umx_sample_io *io, void *const *out_dev, umx_levels_acc *acc_dev, void *hip_stream);
int umx_hip_rescale_device(umx_hip_ctx *ctx, int n_buffers, float *const *bufs_dev, int n, const umx_levels_acc *acc_dev, void *hip_stream);
/* the same rules on the host (no GPU, no context): n_frames stereo frames of output buffer `buffer` accumulate into *acc; clipped is
 * counted for a UMX_SAMPLE_S16 or UMX_SAMPLE_S24 out_format of io (by that format's rule), on x / clip_divisor when clip_divisor != 1.  The divisor of peaks peak[0 .. n). */
int umx_hip_levels_host(const float *x, int n_frames, int buffer, long long first_frame, const umx_sample_io *io, float clip_divisor,
                        umx_levels_acc *acc);
float umx_hip_rescale_gain(const float *peak, int n);
/* Loudness of every output: ITU-R BS.1770-4 / EBU R128 integrated and momentary loudness, from K-weighted hop energies
 * measured on the device where every output frame is final.  A sum of squares is made independent of regions, lanes, the queue and
 * reset mode by tying it to fixed hops anchored at frame 0 of the caller's track and computing every hop in one fixed order.  The
 * rules, to the bit; all arithmetic in double, the inputs the fp32 samples umx_levels measures (at the caller's rate, behind the mix,
 * before any rescale and before any encode):
 *   hop        hop = (rate + 5) / 10 frames, integer arithmetic.  Hop b of output m is the frames [b hop, (b + 1) hop) of the caller's
 *              track; a last incomplete hop is not measured (BS.1770 measures no incomplete block): hops = length / hop.
 *   K-weight   two biquads per rate, formed on the host in double from the analogue prototypes, as libebur128 (ebur128_init_filter) does:
 *              shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / rate), Vh = 10^(G/20),
 *                Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2; b = [(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0],
 *                a = [1, 2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0]
 *              high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1], a as above with this stage's K and Q
 *              (at 48000 these are the seven coefficients of the BS.1770-4 table to 9e-16)
 *   E[m][ch][b]  the sum over hop b's frames of the squared output of the cascade (shelf, then high-pass) of channel ch.  The cascade
 *              starts from a ZERO state at frame max(0, b - 1) hop and runs sample by sample in transposed direct form II; per stage,
 *              with state (s1, s2): u = fma(b1, x, s2); y = fma(b0, x, s1); s1 = fma(-a1, y, u); s2 = fma(-a2, y, b2 * x).  The squares
 *              are added in frame order, E = fma(y, y, E).  One hop (100 ms) of warm-up stands for the filter's infinite history (the
 *              slowest pole has decayed by e^-24 by then; hop 0 is exact, the standard's filter starts from rest too): against the
 *              full-history filter every hop energy is within 1.2e-11 relative, integrated loudness within 2e-11 LU.  A hop is thus a
 *              function of 2 hop samples and of nothing else; a NaN reaches two hops and stops.
 *   blocks     block j is hops j .. j+3 (400 ms, 75 % overlap): P_j = sum over both channels (weights 1, 1) and the four hops of E,
 *              over 4 hop; l_j = -0.691 + 10 log10 P_j.  Absolute gate: l_j > -70.  Relative gate: G = -0.691 + 10 log10(mean of P_j
 *              over the absolutely gated blocks) - 10.  integrated = -0.691 + 10 log10(mean of P_j over the blocks with l_j > -70 and
 *              l_j > G); momentary_max = the maximum of l_j over all blocks.  Comparisons are IEEE: a NaN block passes no gate and is no
 *              maximum; an inf block passes the absolute gate and is the maximum (it puts G at inf, which no block is above:
 *              integrated is then -INFINITY with gated 0, and momentary_max = inf says why).  With no block, or none gated in, both are -INFINITY.  `blocks` and `gated` are the counts.
 * The shift ensemble, the multi-GPU driver (umx_mgpu.h) and the per-segment umx_hip_infer_* calls do not offer loudness. */
typedef struct umx_loudness /* what a whole-track call reports per track */
{
    double integrated[4], momentary_max[4]; /* LUFS */
    long long blocks[4], gated[4];
    long long hops; /* length / hop: measured hops per channel */
    int n_out;
    int hop; /* frames */
} umx_loudness;
/* umx_hip_separate_tracks_levels with loudness: n_tracks records, or NULL; hop_energy: NULL, or per track NULL or a buffer of
 * n_out * 2 * (length / hop) doubles that receives E, laid out [output][channel][hop] (the envelope, for activity detection).  The
 * rate of a track is rate[i], 44100 when rate == NULL.  loudness == NULL and hop_energy == NULL IS the _levels call: the same
 * launches, nothing allocated.  Otherwise one launch per finished region computes the hops that have become final (a track that
 * leaves whole -- rescaled, or at another rate: one launch, before the divisor), and E comes back once, behind the last region.
 * UMX_ERR_ARG, naming the reason and leaving the context usable, for the shift ensemble and for everything the _levels call refuses
 * (a rate outside 8000 .. 192000 among it). */
int umx_hip_separate_tracks_loudness(umx_hip_ctx *ctx, int n_tracks, const void *const *audio_host, const int *length, const int *rate,
                                     const int *shift_offset, int n_out, const float *gains, void *const *out_host, unsigned flags,
                                     const umx_sample_io *io, int clip_mode, umx_levels *levels, umx_loudness *loudness,
                                     double *const *hop_energy, void (*progress)(float, void *), void *progress_user);
/* umx_hip_separate_queue_levels whose done callback also receives the job's loudness record and its hop energies
 * (n_out * 2 * loudness->hops doubles, [output][channel][hop]); all three are valid during the callback only. */
typedef void (*umx_queue_loudness_fn)(void *user, const umx_queue_job *job, const umx_levels *levels, const umx_loudness *loudness,
                                      const double *hop_energy);
int umx_hip_separate_queue_loudness(umx_hip_ctx *ctx, umx_queue_next_fn next, umx_queue_loudness_fn done, void *user, int n_out,
                                    const float *gains, unsigned flags, const umx_sample_io *io, int clip_mode);
/* the kernel on the caller's device buffers, queued on hip_stream: 1 .. 4 buffers of (2,n) interleaved fp32 (8-byte aligned), frame 0
 * first; hops [first_hop, first_hop + n_hops) of each go to E_dev[(buffer * 2 + channel) * (n / hop) + b], and exactly those entries
 * are written (n_hops == 0: none).  UMX_ERR_ARG for a rate outside 8000 .. 192000, n > 2^30 - 1 and hops beyond n / hop. */
int umx_hip_kweight_hops_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, int rate, long long first_hop,
                                long long n_hops, double *E_dev, void *hip_stream);
/* the same rules on the host (no GPU, no context).  coeffs: b0 b1 b2 and 1 a1 a2 of the shelf (pb, pa) and the high-pass (rb, ra).
 * hops_host: one buffer, E[channel * (n / hop) + b].  gate: one output's two channels, E[channel * hops + b]. */
int umx_hip_kweight_coeffs(int rate, double pb[3], double pa[3], double rb[3], double ra[3]);
int umx_hip_kweight_hops_host(const float *x, int n, int rate, long long first_hop, long long n_hops, double *E);
int umx_hip_loudness_gate(const double *E, long long hops, int hop, double *integrated, double *momentary_max, long long *blocks,
                          long long *gated);
/* True peak of every output: the peak of the reconstructed waveform (dBTP = 20 log10), not of its samples, measured on
 * the device where every output frame is final.  A separated stem is not bounded by its mixture, and a track rescaled on its sample
 * peak can still overshoot between the samples: a tone at fs/4 with 45 degrees of phase reads 3.1 dB higher here than in peak[m].
 * The rules, to the bit; the inputs are the fp32 samples umx_levels measures (at the caller's rate, behind the mix, before any
 * rescale and before any encode), both channels of the `length` frames of output buffer m:
 *   factor     F = 4 for rate < 96000, 2 for 96000 <= rate < 192000, 1 for rate == 192000 (libebur128's factors); rates outside
 *              8000 .. 192000 are refused
 *   taps       49-tap Hann-windowed sinc (libebur128's interpolator restated), formed on the host in double: for i = 0 .. 48,
 *              m = i - 24: h[i] = (m == 0 ? 1 : sin(pi m / F) / (pi m / F)) * 0.5 (1 - cos(2 pi i / 48)), each rounded once to fp32.
 *              h[24] is exactly 1, h[0] = h[48] = 0 and every other tap of phase 0 is below 1e-15: phase 0 is the sample itself.
 *   y          frame k in [0, length), channel ch, phase f = 1 .. F-1: y = 0; for t = 0 .. 48/F - 1:
 *              y = fmaf(h[f + F t], x[k + 24/F - t], y) -- fp32, in that order, fused multiply-adds; frames outside [0, length)
 *              read as +0.  Frame k's values read frames k - (24/F - 1) .. k + 24/F: 12 frames at F = 4, 24 at F = 2.
 *   true_peak[m]  the largest of |x| over the samples (peak[m]'s rule: the unsigned maximum of the bit patterns, NaN contributes
 *              nothing, +inf counts) and of |y| over all interpolated values under the same rule.  true_peak[m] >= peak[m] always;
 *              at F = 1 they are equal.  A maximum of values that depend on fixed frames only: regions, lanes, the queue, reset
 *              mode and a rerun give the same bits.
 *   true-peak rescale (UMX_TRUE_PEAK_RESCALE, with UMX_CLIP_RESCALE): P of the rescale rule above is the maximum of true_peak[m]
 *              instead of peak[m]; everything else of that rule is unchanged (g = 1.01f * P; divisor 1 when P is not finite or
 *              !(g > 1.0f); x / g, then the unchanged encode).  Since true_peak >= peak nothing clamps afterwards, as before;
 *              umx_levels.gain reports that divisor.
 * The shift ensemble, the multi-GPU driver (umx_mgpu.h) and the per-segment umx_hip_infer_* calls do not offer it. */
#define UMX_TRUE_PEAK_OFF 0
#define UMX_TRUE_PEAK_MEASURE 1
#define UMX_TRUE_PEAK_RESCALE 2
typedef struct umx_true_peak /* what a whole-track call reports per track */
{
    float true_peak[4];
    int n_out;
    int factor;
} umx_true_peak;
/* umx_hip_separate_tracks_loudness with a true-peak mode: n_tracks records, or NULL (a mode other than OFF still measures).
 * UMX_TRUE_PEAK_OFF with true_peak == NULL IS the _loudness call: the same launches, nothing allocated.  Otherwise one launch per
 * finished region measures the frames whose window has become final -- all but the last 24/F of the region, and everything on a
 * track's last region; a track that leaves whole (rescaled, or both): one launch, before the divisor is formed.  UMX_ERR_ARG, naming
 * the reason and leaving the context usable, for an unknown mode, for UMX_TRUE_PEAK_RESCALE without UMX_CLIP_RESCALE (both checked
 * behind formats, clip mode and gains), for the shift ensemble and for everything the _loudness call refuses. */
int umx_hip_separate_tracks_true_peak(umx_hip_ctx *ctx, int n_tracks, const void *const *audio_host, const int *length, const int *rate,
                                      const int *shift_offset, int n_out, const float *gains, void *const *out_host, unsigned flags,
                                      const umx_sample_io *io, int clip_mode, umx_levels *levels, umx_loudness *loudness,
                                      double *const *hop_energy, int true_peak_mode, umx_true_peak *true_peak,
                                      void (*progress)(float, void *), void *progress_user);
/* umx_hip_separate_queue_loudness with a true-peak mode; the done callback also receives the job's true-peak record (all zero with
 * factor 0 under UMX_TRUE_PEAK_OFF); everything it receives is valid during the callback only. */
typedef void (*umx_queue_true_peak_fn)(void *user, const umx_queue_job *job, const umx_levels *levels, const umx_loudness *loudness,
                                       const double *hop_energy, const umx_true_peak *true_peak);
int umx_hip_separate_queue_true_peak(umx_hip_ctx *ctx, umx_queue_next_fn next, umx_queue_true_peak_fn done, void *user, int n_out,
                                     const float *gains, unsigned flags, const umx_sample_io *io, int clip_mode, int true_peak_mode);
/* the kernel on the caller's device buffers, queued on hip_stream: 1 .. 4 buffers of (2,n) interleaved fp32 (8-byte aligned) that
 * hold a track from frame 0; frames [first_frame, first_frame + n_frames) of buffer b accumulate (unsigned maximum) into
 * bits_dev[b], four words that the caller has zeroed; exactly those four words are written and nothing outside [0, n) of a buffer is
 * read.  UMX_ERR_ARG for a rate outside 8000 .. 192000, n > 2^30 - 1 and frames beyond n. */
int umx_hip_true_peak_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, int rate, long long first_frame,
                             long long n_frames, unsigned *bits_dev, void *hip_stream);
/* the same rules on the host (no GPU, no context).  taps: the 49 fp32 taps and the factor of a rate.  host: one buffer of n
 * interleaved stereo frames, frames [first_frame, first_frame + n_frames) accumulating into *bits. */
int umx_hip_true_peak_taps(int rate, float taps[49], int *factor);
int umx_hip_true_peak_host(const float *x, int n, int rate, long long first_frame, long long n_frames, unsigned *bits);
/* testing, host only: the fp32 tap table of a rate pair (taps[phase * K + d + D]; cap floats at most), its phase count L, taps
 * per phase K and first offset -D.  UMX_ERR_ARG for a bad rate or a too small cap (the sizes are still reported). */
int umx_hip_debug_resample_taps(int rate_in, int rate_out, float *taps, size_t cap, int *phases, int *taps_per_phase,
                                int *first_offset);

/* One segment phase by phase: front (STFT, fc1, W_ih layer 0) | LSTM layer 0 | 1 | 2 | back (fc2, fc3, Wiener,
 * iSTFT).  Same kernels and results as umx_hip_infer_segment; the cuts are where the reference's per-chain
 * (h, c) (lstm.cpp:116-161: read at the start of a layer, left behind at its end) crosses from the GPU that ran
 * the previous segment (SURVEY 8e "carry" mode): set layer l's state, run layer l, get it, pass it on.
 * Layer state layout: [4 targets][2 dirs][2: h, c][hidden/2] floats. */
size_t umx_hip_stream_layer_floats(const umx_hip_ctx *ctx);
int umx_hip_stream_get_layer(umx_hip_ctx *ctx, int layer, float *host_dst);
int umx_hip_stream_set_layer(umx_hip_ctx *ctx, int layer, const float *host_src);
int umx_hip_segment_begin(umx_hip_ctx *ctx, const float *audio_host, int n, unsigned flags);
int umx_hip_segment_lstm_layer(umx_hip_ctx *ctx, int layer); /* 0, 1, 2 in order */
int umx_hip_segment_end(umx_hip_ctx *ctx, float *const out_host[4]);

/* The same cut points for a driver that keeps everything in HBM and on ONE stream (host/mgpu.cpp: RCCL send / recv
 * of the state and of the weighted stems on device pointers, no host bounce).  None of these waits for the device;
 * all work is queued on umx_hip_phase_stream in call order, so a collective queued on that stream between two of
 * them is ordered against the kernels on both sides.
 *   umx_hip_segment_begin_device   front of a segment, audio already in HBM
 *   umx_hip_segment_lstm_layer     (as above)
 *   umx_hip_segment_end_device     back of the segment into 4 device buffers (2,n)
 *   umx_hip_stream_state_device    device address of track lane 0's stream state, [4 targets][3 layers][2 dirs][2: h, c][hidden/2]:
 *                                  layer l of target t is the 4 * hidden/2 floats at ((t * 3 + l) * 4) * hidden/2
 *   umx_hip_weight_stems_device    stems[t][k] *= transition weight of sample k (umx.cpp:197-206, 246), in place
 *   umx_hip_track_accumulate_device / _normalise_device   umx.cpp:234-273 on device buffers: track (2,length) x 4 +=
 *                                  already weighted stems at `offset`, sum_weight += weights; then track /= sum_weight */
/* The back of a segment in two halves, for the driver that shards a track by SOURCE MODEL (host/mgpu.cpp, target mode):
 * the per-target loop of umx_inference (inference.cpp:70-186) is independent per target until wiener_filter
 * (inference.cpp:192-193), so a GPU runs begin / lstm_layer x 3 / masks with the other targets skipped
 * (UMX_FLAG_SKIP_TARGET), the target magnitudes travel to the GPU that filters this segment, and that GPU finishes:
 *   umx_hip_segment_masks_device   fc2, fc3, mask x |X| of the targets that are not skipped (after layer 2)
 *   umx_hip_target_mag_device      device address of target t's MASK planes [2][T][2176] (2049 bins + padding per row;
 *                                  *floats = the size) of the phased segment -- the target magnitude is mask x |X|
 *                                  (inference.cpp:175-183), which _finish_device forms from its own spectrogram: read it
 *                                  after _masks_device, or write a peer's result there before _finish_device
 *   umx_hip_segment_finish_device  Wiener EM (or the mixture phase), inverse STFT, overlap-add from ALL four magnitude
 *                                  buffers as they are (a skipped target is NOT zero-filled here, and UMX_FLAG_RESIDUAL writes nothing
 *                                  here) into 4 device buffers
 *   umx_hip_segment_residual_device  UMX_FLAG_RESIDUAL of the open segment: writes the residual slot's mask planes from the active
 *                                  targets' (after _masks_device, before _finish_device); UMX_ERR_ARG without the flag
 * umx_hip_segment_end_device == _masks_device, zero-fill of the skipped targets (the residual slot: _residual_device), _finish_device. */
int umx_hip_segment_masks_device(umx_hip_ctx *ctx);
int umx_hip_segment_residual_device(umx_hip_ctx *ctx);
float *umx_hip_target_mag_device(umx_hip_ctx *ctx, int target, size_t *floats);
int umx_hip_segment_finish_device(umx_hip_ctx *ctx, float *const out_dev[4]);
int umx_hip_segment_discard(umx_hip_ctx *ctx); /* closes the phased segment where it stands (a rank that only contributes magnitudes) */
/* Persistent LSTM launches of every context on `device` leave `cus` compute units out of their co-residency budget
 * (the admission gate of umx_hip_sync's comment): room for kernels that are not this engine's and that may sit on a CU
 * for a long time -- RCCL's send / recv kernels in host/mgpu.cpp.  Process-wide, per device: cus > 0 files a request (the SUM of
 * the outstanding ones applies, at most half the chip: every driver keeps its own transfer kernels resident), -cus gives one
 * request of that size back (UMX_ERR_ARG if there is none), 0 drops every request (tests only). */
int umx_hip_gate_reserve(int device, int cus);
void *umx_hip_phase_stream(umx_hip_ctx *ctx);
float *umx_hip_stream_state_device(umx_hip_ctx *ctx);
int umx_hip_segment_begin_device(umx_hip_ctx *ctx, const float *audio_dev, int n, unsigned flags);
int umx_hip_segment_end_device(umx_hip_ctx *ctx, float *const out_dev[4]);
int umx_hip_weight_stems_device(umx_hip_ctx *ctx, float *const stems_dev[4], int n, void *hip_stream);
int umx_hip_track_accumulate_device(umx_hip_ctx *ctx, float *const track_dev[4], float *sum_weight_dev,
                                    const float *const weighted_dev[4], int offset, int n, void *hip_stream);
int umx_hip_track_normalise_device(umx_hip_ctx *ctx, float *const track_dev[4], const float *sum_weight_dev, int length,
                                   void *hip_stream);

/* Geometry */
int umx_hip_nb_frames(const umx_hip_ctx *ctx);       /* T = segment_samples/1024 + 1 (dsp.hpp:48) */
int umx_hip_segment_samples(const umx_hip_ctx *ctx);
int umx_hip_hidden(const umx_hip_ctx *ctx);

/* Stage taps for parity tests (D2H copy of an intermediate of the LAST inferred segment).
 * what: "spec" [2][T][2049] complex | "mix_mag" [2][T][2049] | "x" [T][2976] |
 *       "fc1" [T][H] | "lstm" [T][H] | "fc2" [T][H] | "mask" [T][4098] |
 *       "target_mag" [2][T][2049] | "y" [2][T][2049] complex (needs UMX_FLAG_DEBUG_TAPS; so does "lstm" in a track-batched
 *       context) | "max_abs" [1];
 *       ("mix_mag", "target_mag" and "mask" are not buffers of the engine any more -- fc3 writes the mask in a padded
 *       layout and the Wiener kernels form mask x |X| in registers -- a tap kernel computes them on demand with the
 *       device functions the hot kernels use, so they hold the bits the pipeline works with)
 *       suffix "#k" selects track lane k (default 0), "@s" pipeline slot s (default: the most recent)
 * Returns the number of floats written (or needed when dst == NULL), < 0 on error. */
long umx_hip_read_tap(umx_hip_ctx *ctx, const char *what, int target, float *dst, size_t capacity_floats);

/* Per-stage device time of the LAST segment, measured with hipEvents on the context's stream.
 * names/ms are filled up to `cap` entries; returns the number of stages. */
int umx_hip_stage_times(umx_hip_ctx *ctx, const char **names, float *ms, int cap);
/* Same for pipeline slot 0 or 1 (consecutive segments alternate slots; when two segments were queued
 * back to back their spans overlap, so a stage's time includes interference from the other slot). */
int umx_hip_stage_times_slot(umx_hip_ctx *ctx, int slot_index, const char **names, float *ms, int cap);
/* The same stages with the MAIN kernel alone where a stage launches a preparing kernel first (the GEMM stages of plane
 * contexts: split_planes_kernel, then the GEMM): the time from an event recorded between the two to the next stage's
 * event.  Stages without such a kernel report their stage time.  slot_index < 0: the slot of the last call. */
int umx_hip_stage_kernel_times_slot(umx_hip_ctx *ctx, int slot_index, float *ms, int cap);
/* 1 if the LSTM layers of the last segment ran in the persistent (one launch per layer) kernel,
 * 0 if the per-timestep driver was used (flag, unsupported hidden size, or grid not co-resident). */
int umx_hip_lstm_was_persistent(const umx_hip_ctx *ctx);
/* The recurrence kernel the last LSTM layer launch used: "lstm_persistent_kernel" / "lstm_step_kernel" (one track),
 * "lstm_batch8_kernel" (track-batched, hidden 1024 / 512, u8-resident W_hh), "lstm_batch_kernel" (every other track-batched context). */
const char *umx_hip_lstm_kernel_name(const umx_hip_ctx *ctx);
/* The GEMM kernel the last call launched for stage `mode` (0 fc1, 1 W_ih, 2 fc2, 3 fc3): "gemm_planes_ps_kernel" (persistent walk),
   "gemm_planes_pp_kernel", "gemm_planes_kernel", "gemm_bf16x3_kernel" or "none".  For bench.py's per-kernel figures: no reference analogue. */
const char *umx_hip_gemm_kernel_name(const umx_hip_ctx *ctx, int mode);
/* 0 = per-timestep driver, 1 = persistent kernel with the placement-independent (sc1) hand-off,
 * 2 = persistent kernel whose census found every chain on one XCD (intra-L2 hand-off); < 0 on error */
int umx_hip_lstm_mode(umx_hip_ctx *ctx);
/* UMX_FLAG_LSTM_PROFILE: shader-clock cycles summed over the T steps of each layer, for waves 0 and 1
 * of workgroup (chain 0, slice 0): out48[(layer*2 + wave)*8 + {0 poll, 1 dot, 2 barrier, 3 gates, 4 steps}] */
/* Testing: the per-bin arithmetic both Wiener filter kernels share (|X|, PSDs with F5, Cxx with F6, closed-form inverse, y_j =
 * v_j R_j (Cxx^-1 x) * max_abs; wiener.cpp:301-400) on caller-given bins: X [n][2][re, im], masks [n][4][2], R [n][4][R00, Re R01,
 * Im R01, R11], y [n][4][2][re, im]; max_abs >= 1 (wiener.cpp:51).  Host pointers; needs a current HIP device. */
int umx_hip_debug_wiener_bins(int n, const float *X, const float *masks, const float *R, float max_abs, float *y);
/* Testing: the gate functions of the recurrence kernels and of the fc1 epilogue on caller-given values, and one LSTM cell step per
 * wave.  x [n] -> fn [5][n]: tanh_epi (fc1 epilogue), tanh_hw, the fast sigmoid rcp(1 + exp(-x)), and the UMX_FLAG_PRECISE_ACT forms
 * tanhf and 1 / (1 + expf(-x)).  pre [n_waves][64]: a gate pre-activation per lane, lane = 4 * unit + gate (i, f, g, o); c [n_waves][16]
 * -> cell [4][n_waves][2][16]: the new (c, h) of every unit from the default cell of the per-step driver, from the branch-free cell
 * of the persistent kernel, from the PRECISE cell and from the one-lane cell of the batched recurrences.  n == 0 or n_waves == 0 skips that half (n <= 2^24, n_waves <= 2^16).  Host
 * pointers; needs a current HIP device, no context. */
int umx_hip_debug_gate_math(int n, const float *x, float *fn, int n_waves, const float *pre, const float *c, float *cell);
int umx_hip_debug_lstm_profile(umx_hip_ctx *ctx, unsigned long long *out48);
/* Where the workgroups of the last profiled one-track recurrence launch ran (UMX_FLAG_LSTM_PROFILE): out[i] for workgroup i =
 * XCC id << 48 | chain << 40 | slice << 32 | the 32-bit HW_ID register (CU, shader array, shader engine).  n <= 512. */
int umx_hip_debug_lstm_placement(umx_hip_ctx *ctx, unsigned long long *out, int n);
/* Debugging (tools/bx_guard.py): queue `launches` guard kernels on a private stream -- each workgroup keeps a 36 KB
 * pattern in LDS and re-verifies it `rounds` times -- beside whatever the caller queues next; launches == 0 waits
 * for them and returns {words found changed, events} in out2.  Used to show that no kernel of this engine writes
 * into another workgroup's LDS. */
int umx_hip_debug_lds_guard(umx_hip_ctx *ctx, int launches, int rounds, unsigned *out2);
/* Testing hook (no GPU needed): the host-side fp32 -> fp16 conversion (round to nearest even, subnormals, overflow to
 * infinity) with which weights are re-encoded as fp16 planes at load time (csrc/quant_planes.h); returns the 16 bits. */
unsigned umx_hip_debug_f16_bits(float x);
/* Testing (no GPU needed): the centre c of a u8 tensor's q - c in gemm_bf16x3's one-plane form (csrc/quant_planes.h quant_centre);
 * *o2 = offset + c scale, formed in double and rounded once. */
int umx_hip_debug_quant_centre(float scale, float offset, float *o2);
/* Testing (no GPU needed): the n codes q (elem_size 1: u8, 2: u16) of a file tensor with (scale, offset) as the plane GEMMs of
 * track-batched contexts hold them (csrc/quant_planes.h quant_planes): hi[n] = the fp16 bits of q - c and, for u16, lo[n] = the fp16
 * bits of the remainder (lo may be NULL for u8).  Returns the tensor's centre c (u8: 0 .. 255, u16: 31 .. 65504; 128 / 32896 for a
 * zero or non-finite scale), or -1 for a bad argument; *o2 = offset + c scale, formed in double and rounded once. */
int umx_hip_debug_quant_planes(const void *q, int elem_size, int n, float scale, float offset, unsigned short *hi, unsigned short *lo, float *o2);

#ifdef __cplusplus
}
#endif
#endif /* UMX_HIP_H */
