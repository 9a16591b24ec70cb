// engine_cabi.h -- part of engine.hip (one translation unit: the kernels inline into their launchers): the C-ABI of include/umx_hip.h.
// Included by engine.hip behind the definition of umx_hip_ctx; not a stand-alone header.
// ---------------------------------------------------------------- C-ABI
// The 1 .. 4 non-null device buffers of a kernel's entry point, as the kernel's frames (float2, or a word per int16 frame) -> p[];
// false: refused (set_error done)
template <class From, class To>
static bool device_buffers(umx_hip_ctx *ctx, const char *what, int n_buffers, From *const *bufs, int n, long long first_frame, To *p[4])
{
    if (n_buffers < 1 || n_buffers > 4 || !bufs || n < 1 || first_frame < 0)
    {
        ctx->set_error(std::string(what) + ": need 1 .. 4 buffers, n >= 1 and first_frame >= 0");
        return false;
    }
    for (int b = 0; b < n_buffers; ++b)
    {
        if (!bufs[b])
        {
            ctx->set_error(std::string(what) + ": null buffer");
            return false;
        }
        p[b] = reinterpret_cast<To *>(bufs[b]);
    }
    return true;
}

// ---------------------------------------------------------------- the integer sample formats behind their entry points (sample_format.h)
// the dither of an integer output as the kernels and their host restatements take it (io == NULL: none)
struct DitherArg
{
    bool on;
    uint32_t seed;
};
static DitherArg dither_of(const umx_sample_io *io) { return {io && io->dither, io ? io->dither_seed : 0u}; }

// a device buffer of `format`: at the alignment its trait asks for
static bool sample_aligned(umx_hip_ctx *ctx, const char *what, int format, int n_buffers, const void *const *bufs)
{
    return with_sample_format(format, [&](auto t) {
        for (int b = 0; b < n_buffers; ++b)
            if ((uintptr_t)bufs[b] & (uintptr_t)(decltype(t)::align - 1))
            {
                ctx->set_error(std::string(what) + ": " + decltype(t)::misaligned());
                return false;
            }
        return true;
    });
}

// The six device entry points of the two integer formats.  what: their name in messages ("pcm16 decode", "rescaled pcm24 encode").
static int decode_device(umx_hip_ctx *ctx, const char *what, int format, const void *in_dev, int n, float *out_dev, void *hip_stream)
{
    if (!ctx)
        return UMX_ERR_ARG;
    if (!in_dev || !out_dev || n < 1)
    {
        ctx->set_error(std::string(what) + ": need both buffers and n >= 1");
        return UMX_ERR_ARG;
    }
    if (!sample_aligned(ctx, what, format, 1, &in_dev))
        return UMX_ERR_ARG;
    UMX_HIP_CHECK_CTX(ctx, hipSetDevice(ctx->device));
    launch_decode(format, in_dev, reinterpret_cast<float2 *>(out_dev), n, (hipStream_t)hip_stream);
    UMX_HIP_CHECK_CTX(ctx, hipGetLastError());
    return UMX_OK;
}

// rescaled: over the divisor of the record acc_dev, which must be there (else acc_dev is not looked at: the plain encode)
static int encode_device(umx_hip_ctx *ctx, const char *what, int format, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                         const umx_sample_io *io, void *const *out_dev, bool rescaled, umx_levels_acc *acc_dev, void *hip_stream)
{
    if (!ctx)
        return UMX_ERR_ARG;
    const float2 *src[4] = {};
    uint8_t *dst[4] = {};
    if (!device_buffers(ctx, what, n_buffers, in_dev, n, first_frame, src) || !device_buffers(ctx, what, n_buffers, out_dev, n, first_frame, dst) ||
        !sample_aligned(ctx, what, format, n_buffers, out_dev))
        return UMX_ERR_ARG;
    if (rescaled && !acc_dev)
    {
        ctx->set_error(std::string(what) + ": null record");
        return UMX_ERR_ARG;
    }
    UMX_HIP_CHECK_CTX(ctx, hipSetDevice(ctx->device));
    const DitherArg d = dither_of(io);
    launch_encode(format, n_buffers, src, dst, n, first_frame, d.on, d.seed, rescaled ? acc_dev : nullptr, (hipStream_t)hip_stream);
    UMX_HIP_CHECK_CTX(ctx, hipGetLastError());
    return UMX_OK;
}

// the host restatements: n_values samples, and n_frames stereo frames of output buffer `buffer`
template <class T> static int decode_host(T t, const void *q, long long n_values, float *x)
{
    if (!q || !x || n_values < 0)
        return UMX_ERR_ARG;
    for (long long i = 0; i < n_values; ++i)
        x[i] = load_sample(t, q, (size_t)i);
    return UMX_OK;
}
template <class T> static int encode_host(T t, const float *x, int n_frames, int buffer, long long first_frame, const umx_sample_io *io, void *q)
{
    if (!x || !q || n_frames < 0 || buffer < 0 || buffer >= UMX_MAX_MIX_OUTPUTS || first_frame < 0)
        return UMX_ERR_ARG;
    const DitherArg d = dither_of(io);
    const uint32_t key[2] = {sample_dither_key(d.seed, buffer, 0), sample_dither_key(d.seed, buffer, 1)};
    for (int i = 0; i < n_frames; ++i)
        for (int ch = 0; ch < 2; ++ch)
            store_sample(t, q, 2 * (size_t)i + ch, T::clamp(T::round(x[2 * (size_t)i + ch], d.on, key[ch], first_frame + i)));
    return UMX_OK;
}

extern "C"
{

int umx_hip_create(umx_hip_ctx **out, int device, int hidden_size, int segment_samples,
                   const umx_tensor_view *tensors, int n_tensors)
{
    unsigned cf = 0;
    if (const char *e = getenv("UMX_WEIGHTS_RESIDENT")) // lets umx-cli switch without an API change
        if (std::string(e) == "expanded" || std::string(e) == "f32")
            cf |= UMX_CREATE_DEQUANTISE_AT_LOAD;
    if (const char *e = getenv("UMX_GEMM"))
    {
        if (std::string(e) == "f32")
            cf |= UMX_CREATE_GEMM_F32;
        if (std::string(e) == "bf16x3")
            cf |= UMX_CREATE_GEMM_STAGED;
        if (std::string(e) == "planes")
            cf |= UMX_CREATE_GEMM_PLANES;
    }
    if (const char *e = getenv("UMX_LSTM"))
        if (std::string(e) == "batched")
            cf |= UMX_CREATE_LSTM_BATCHED;
    if (const char *e = getenv("UMX_U8"))
        if (std::string(e) == "dequant")
            cf |= UMX_CREATE_U8_DEQUANT;
    return umx_hip_create_ex(out, device, hidden_size, segment_samples, tensors, n_tensors, cf);
}

size_t umx_hip_weight_bytes(const umx_hip_ctx *ctx) { return ctx ? ctx->weight_bytes : 0; }

int umx_hip_create_ex(umx_hip_ctx **out, int device, int hidden_size, int segment_samples,
                      const umx_tensor_view *tensors, int n_tensors, unsigned create_flags)
{
    return umx_hip_create_tracks(out, device, hidden_size, segment_samples, tensors, n_tensors, create_flags, 1);
}

int umx_hip_create_tracks(umx_hip_ctx **out, int device, int hidden_size, int segment_samples,
                          const umx_tensor_view *tensors, int n_tensors, unsigned create_flags, int n_tracks)
{
    if (!out || !tensors)
    {
        g_create_error = "umx_hip_create: null argument";
        return UMX_ERR_ARG;
    }
    *out = nullptr;
    umx_hip_ctx *c = new umx_hip_ctx;
    int rc = c->init(device, hidden_size, segment_samples, tensors, n_tensors, create_flags, n_tracks);
    if (rc != UMX_OK)
    {
        g_create_error = c->err;
        umx_hip_destroy(c);
        return rc;
    }
    *out = c;
    return UMX_OK;
}

int umx_hip_n_tracks(const umx_hip_ctx *ctx) { return ctx ? ctx->B : 0; }
int umx_hip_pipeline_depth(const umx_hip_ctx *ctx) { return ctx ? ctx->nslots : 0; }
int umx_hip_lstm_is_batched(const umx_hip_ctx *ctx) { return ctx && ctx->lstm_batched ? 1 : 0; }

unsigned umx_hip_debug_f16_bits(float x) { return f16_rne_bits(x); }
int umx_hip_debug_quant_centre(float scale, float offset, float *o2)
{
    const QuantCentre qc = quant_centre(scale, offset);
    if (o2)
        *o2 = qc.o2;
    return qc.c;
}
int umx_hip_debug_quant_planes(const void *q, int elem_size, int n, float scale, float offset, unsigned short *hi, unsigned short *lo, float *o2)
{
    if (!q || !hi || n < 0 || (elem_size != 1 && elem_size != 2) || (elem_size == 2 && !lo))
        return -1;
    const QuantCentre qc = quant_planes(q, elem_size, 1, n, nullptr, (size_t)n, scale, offset, hi, lo);
    if (o2)
        *o2 = qc.o2;
    return qc.c;
}

void umx_hip_destroy(umx_hip_ctx *ctx)
{
    if (!ctx)
        return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (void *p : ctx->allocs)
        (void)hipFree(p);
    for (hipEvent_t e : ctx->trk_acc_ev)
        if (e)
            (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ens_ev)
        if (e)
            (void)hipEventDestroy(e);
    for (const std::vector<umx_hip_ctx::TrackBufs> *sets : {&ctx->trk, &ctx->qpool})
        for (const umx_hip_ctx::TrackBufs &tb_ : *sets)
            if (tb_.in_ev)
                (void)hipEventDestroy(tb_.in_ev);
    if (ctx->order_ev)
        (void)hipEventDestroy(ctx->order_ev);
    if (ctx->copy_stream)
        (void)hipStreamDestroy(ctx->copy_stream);
    for (int si = 0; si < umx_hip_ctx::kMaxSlots; ++si)
        for (hipEvent_t e : {ctx->slot[si].k_done, ctx->slot[si].out_free})
            if (e)
                (void)hipEventDestroy(e);
    for (int si = 0; si < umx_hip_ctx::kMaxSlots; ++si)
    {
        Slot &sl = ctx->slot[si];
        for (int i = 0; i <= ST_COUNT; ++i)
        {
            if (sl.ev[i])
                (void)hipEventDestroy(sl.ev[i]);
            if (i < ST_COUNT && sl.evk[i])
                (void)hipEventDestroy(sl.evk[i]);
        }
        for (int l = 0; l < 3; ++l)
            if (sl.rec_done[l])
                (void)hipEventDestroy(sl.rec_done[l]);
        if (sl.stream)
            (void)hipStreamDestroy(sl.stream);
    }
    delete ctx;
}

const char *umx_hip_last_error(const umx_hip_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

size_t umx_hip_stream_floats(const umx_hip_ctx *ctx) { return ctx ? ctx->state_floats() : 0; }

// track < 0: every lane
int umx_hip_track_stream_reset(umx_hip_ctx *ctx, int track)
{
    if (!ctx || track >= ctx->B)
        return UMX_ERR_ARG;
    // through umx_hip_sync, not a bare stream wait: a timed-out launch among the calls queued so far is noticed (and
    // repaired by replaying them) BEFORE the state is changed, and the replay log starts afresh behind the change
    if (int rc = umx_hip_sync(ctx))
        return rc;
    const size_t per = ctx->state_floats();
    hipError_t e = track < 0 ? hipMemset(ctx->state, 0, sizeof(float) * per * ctx->B)
                             : hipMemset(ctx->state + per * track, 0, sizeof(float) * per);
    // hipMemset returns before the device has done it, and the slots' non-blocking streams do not order against the null
    // stream: the next segment's kernels must not meet the old state (found in round 3: a rare first-run mismatch)
    if (e == hipSuccess)
        e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess)
    {
        ctx->set_error(hipGetErrorString(e));
        return UMX_ERR_HIP;
    }
    ctx->clear_used(); // nothing in flight: no cross-segment dependency to wait for
    return UMX_OK;
}
int umx_hip_stream_reset(umx_hip_ctx *ctx) { return umx_hip_track_stream_reset(ctx, 0); }

int umx_hip_track_stream_get(umx_hip_ctx *ctx, int track, float *host_dst)
{
    if (!ctx || !host_dst || track < 0 || track >= ctx->B)
        return UMX_ERR_ARG;
    if (int rc = umx_hip_sync(ctx))
        return rc;
    const size_t per = ctx->state_floats();
    hipError_t e = hipMemcpy(host_dst, ctx->state + per * track, sizeof(float) * per, hipMemcpyDeviceToHost);
    if (e != hipSuccess)
    {
        ctx->set_error(hipGetErrorString(e));
        return UMX_ERR_HIP;
    }
    return UMX_OK;
}
int umx_hip_stream_get(umx_hip_ctx *ctx, float *host_dst) { return umx_hip_track_stream_get(ctx, 0, host_dst); }

int umx_hip_track_stream_set(umx_hip_ctx *ctx, int track, const float *host_src)
{
    if (!ctx || !host_src || track < 0 || track >= ctx->B)
        return UMX_ERR_ARG;
    if (int rc = umx_hip_sync(ctx))
        return rc;
    const size_t per = ctx->state_floats();
    hipError_t e = hipMemcpy(ctx->state + per * track, host_src, sizeof(float) * per, hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
        ctx->set_error(hipGetErrorString(e));
        return UMX_ERR_HIP;
    }
    ctx->clear_used();
    return UMX_OK;
}
int umx_hip_stream_set(umx_hip_ctx *ctx, const float *host_src) { return umx_hip_track_stream_set(ctx, 0, host_src); }

size_t umx_hip_stream_layer_floats(const umx_hip_ctx *ctx) { return ctx ? (size_t)4 * 4 * ctx->Hl : 0; }

// one layer's (h, c) of all chains of track lane 0: [target][dir][h|c][Hl]
static int stream_layer_copy(umx_hip_ctx *ctx, int layer, float *host, bool to_host)
{
    if (!ctx || !host || layer < 0 || layer > 2)
        return UMX_ERR_ARG;
    hipError_t e = hipStreamSynchronize(ctx->slot[0].stream);
    if (e == hipSuccess && ctx->ph_next < 0) // outside a phased segment other slots may be busy too
        if (int rc = ctx->sync_all())
            return rc;
    const size_t per = (size_t)4 * ctx->Hl;
    for (int tg = 0; tg < 4 && e == hipSuccess; ++tg)
    {
        float *dev = ctx->state + state_off(tg, layer, 0, 0, ctx->Hl);
        e = to_host ? hipMemcpy(host + tg * per, dev, per * sizeof(float), hipMemcpyDeviceToHost)
                    : hipMemcpy(dev, host + tg * per, per * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess)
    {
        ctx->set_error(hipGetErrorString(e));
        return UMX_ERR_HIP;
    }
    return UMX_OK;
}
int umx_hip_stream_get_layer(umx_hip_ctx *ctx, int layer, float *host_dst) { return stream_layer_copy(ctx, layer, host_dst, true); }
int umx_hip_stream_set_layer(umx_hip_ctx *ctx, int layer, const float *host_src)
{
    return stream_layer_copy(ctx, layer, const_cast<float *>(host_src), false);
}

// ---------------------------------------------------------------- the whole-track entry points
// The ladder umx_hip_separate_tracks, _rate, _mix, _io, _levels, _loudness, _true_peak and the one-track forms are ONE path: the options of the
// call are checked and recorded once (track_options_checked -> umx_hip_ctx::TrackOptions), the request is filled once (track_request;
// its checks are tracks_once's), and separate_tracks does both.  A rung is its own preconditions, then that path with the arguments it
// does not have at their neutral values -- NULL rate, gains and io, and of what is measured (MeasureArgs) only the fields
// the rung has, the others at the record's defaults -- so a wider rung with neutral arguments IS the rung below, field for field, by
// construction.  The queue entry points share queue_entry the same way.
struct MeasureArgs // what a whole-track call measures and where the results go: the defaults are the call that measures nothing
{
    int clip_mode = UMX_CLIP_CLAMP;       // levels.h, DESIGN 20
    umx_levels *levels = nullptr;         // n_tracks records, or NULL
    umx_loudness *loudness = nullptr;     // loudness.h, DESIGN 21: n_tracks records, or NULL
    double *const *hop_energy = nullptr;  // per track NULL or room for its hop energies
    int true_peak_mode = UMX_TRUE_PEAK_OFF; // true_peak.h, DESIGN 26
    umx_true_peak *true_peak = nullptr;   // n_tracks records, or NULL
};
static const char *mix_refusal(int n_out, const float *gains, MixSpec &spec) // (NULL gains are refused: who takes "no mix" asks before)
{
    return mix_spec_from(n_out, gains, &spec) >= 0 ? nullptr
                                                   : "mix: need 1 <= n_out <= 4 rows of five finite gains (bass, drums, other, vocals slots, mixture)";
}
static bool mix_checked(umx_hip_ctx *ctx, int n_out, const float *gains, MixSpec &spec)
{
    const char *why = mix_refusal(n_out, gains, spec);
    if (why)
        ctx->set_error(why);
    return !why;
}

// The options of a call, checked in this order: the sample formats (pcm16.h; io == NULL or fp32 both ways: the fp32 call itself), the
// clip mode (levels.h), the gains (stem_mix.h; NULL: no mix), the true-peak mode (true_peak.h).  true: `opt` holds them, `spec` the matrix behind opt.mix; false: the
// refusal is the context's error.
static bool track_options_checked(umx_hip_ctx *ctx, const umx_sample_io *io, const MeasureArgs &ma, int n_out, const float *gains, MixSpec &spec,
                                  umx_hip_ctx::TrackOptions &opt)
{
    const char *why = sample_io_refusal(io);
    if (!why)
        why = clip_mode_refusal(ma.clip_mode);
    if (!why && gains)
        why = mix_refusal(n_out, gains, spec);
    if (!why)
        why = true_peak_mode_refusal(ma.true_peak_mode, ma.clip_mode);
    if (why)
    {
        ctx->set_error(why);
        return false;
    }
    opt.true_peak = ma.true_peak_mode;
    opt.mix = gains ? &spec : nullptr;
    if (io)
        opt.io = *io;
    opt.clip_mode = ma.clip_mode;
    return true;
}

// (the request keeps its float pointers: the formats say how the driver reads them; a wanted record makes the tracks measure)
static umx_hip_ctx::TrackRequest track_request(int n_tracks, const void *const *audio_host, const int *length, const int *rate,
                                               const int *shift_offset, void *const *out_host, unsigned flags, void (*progress)(float, void *),
                                               void *progress_user, const umx_hip_ctx::TrackOptions &opt, const MeasureArgs &ma)
{
    umx_hip_ctx::TrackRequest rq = {n_tracks, reinterpret_cast<const float *const *>(audio_host), length, rate, shift_offset,
                                    reinterpret_cast<float *const *>(out_host), flags, progress, progress_user};
    rq.opt = opt;
    rq.opt.levels = ma.levels != nullptr;
    rq.opt.loudness = ma.loudness || ma.hop_energy; // the records or the energies themselves
    rq.opt.true_peak_record = ma.true_peak != nullptr; // DESIGN 26 (whether the tracks are measured: opt.true_peak, the mode)
    rq.levels = ma.levels;
    rq.loudness = ma.loudness;
    rq.hop_energy = ma.hop_energy;
    rq.true_peak = ma.true_peak;
    return rq;
}

static int separate_tracks(umx_hip_ctx *ctx, int n_tracks, const void *const *audio_host, const int *length, const int *rate,
                           const int *shift_offset, int n_out, const float *gains, void *const *out_host, unsigned flags,
                           const umx_sample_io *io, const MeasureArgs &ma, void (*progress)(float, void *), void *progress_user)
{
    if (!ctx)
        return UMX_ERR_ARG;
    MixSpec spec;
    umx_hip_ctx::TrackOptions opt;
    if (!track_options_checked(ctx, io, ma, n_out, gains, spec, opt))
        return UMX_ERR_ARG;
    return ctx->tracks(track_request(n_tracks, audio_host, length, rate, shift_offset, out_host, flags, progress, progress_user, opt, ma));
}
// the rungs without sample formats: fp32 buffers, no clip handling, nothing measured
static int separate_tracks_f32(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *length, const int *rate,
                               const int *shift_offset, int n_out, const float *gains, float *const *out_host, unsigned flags,
                               void (*progress)(float, void *), void *progress_user)
{
    return separate_tracks(ctx, n_tracks, reinterpret_cast<const void *const *>(audio_host), length, rate, shift_offset, n_out, gains,
                           reinterpret_cast<void *const *>(out_host), flags, nullptr, MeasureArgs(), progress, progress_user);
}

// A one-track entry point passes the addresses of its own arguments; shift offset < 0: no shift buffer (plain split_inference).
int umx_hip_split_inference(umx_hip_ctx *ctx, const float *audio_host, int length, float *const out_host[4],
                            unsigned flags, void (*progress)(float, void *), void *progress_user)
{
    const int no_shift = -1;
    return separate_tracks_f32(ctx, 1, &audio_host, &length, nullptr, &no_shift, 4, nullptr, out_host, flags, progress, progress_user);
}
int umx_hip_separate_tracks(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *length, const int *shift_offset,
                            float *const *out_host, unsigned flags, void (*progress)(float, void *), void *progress_user)
{
    return separate_tracks_f32(ctx, n_tracks, audio_host, length, nullptr, shift_offset, 4, nullptr, out_host, flags, progress, progress_user);
}
long long umx_hip_resampled_length(long long n, int rate_in, int rate_out) { return resampled_length(n, rate_in, rate_out); }
long long umx_hip_resample_needs(long long n_out_wanted, int rate_in, int rate_out, long long n_in)
{
    return resample_needs(n_out_wanted, rate_in, rate_out, n_in);
}
long long umx_hip_resample_ready(long long n_in_final, int rate_in, int rate_out, long long n_in, long long n_out)
{
    return resample_ready(n_in_final, rate_in, rate_out, n_in, n_out);
}

int umx_hip_resample_device(umx_hip_ctx *ctx, int rate_in, int rate_out, int n_buffers, const float *const *in_dev, int n_in,
                            float *const *out_dev, int n_out, void *hip_stream)
{
    return umx_hip_resample_range_device(ctx, rate_in, rate_out, n_buffers, in_dev, n_in, out_dev, n_out, 0, n_out, hip_stream);
}

int umx_hip_resample_range_device(umx_hip_ctx *ctx, int rate_in, int rate_out, int n_buffers, const float *const *in_dev, int n_in,
                                  float *const *out_dev, int n_out, int first, int count, void *hip_stream)
{
    if (!ctx)
        return UMX_ERR_ARG;
    if (n_buffers < 1 || n_buffers > 4 || !in_dev || !out_dev || n_in < 1 || n_out < 0)
    {
        ctx->set_error("resample: need 1 .. 4 buffers, n_in >= 1 and n_out >= 0");
        return UMX_ERR_ARG;
    }
    for (int b = 0; b < n_buffers; ++b)
        if (!in_dev[b] || !out_dev[b])
        {
            ctx->set_error("resample: null buffer");
            return UMX_ERR_ARG;
        }
    if (first < 0 || count < 0 || (first & 1) || (long long)first + count > (long long)n_out)
    {
        ctx->set_error("resample: a range needs an even first frame >= 0, count >= 0 and first + count <= n_out");
        return UMX_ERR_ARG;
    }
    ResampleGeom g;
    const float *taps = nullptr;
    UMX_HIP_CHECK_CTX(ctx, hipSetDevice(ctx->device));
    if (int rc = ctx->resample_plan(rate_in, rate_out, g, &taps))
        return rc;
    UMX_HIP_CHECK_CTX(ctx, launch_resample(g, taps, n_buffers, in_dev, n_in, out_dev, n_out, first, count, (hipStream_t)hip_stream));
    return UMX_OK;
}

int umx_hip_shift_inference_rate(umx_hip_ctx *ctx, const float *audio_host, int length, int rate, int offset, float *const out_host[4],
                                 unsigned flags, void (*progress)(float, void *), void *progress_user)
{
    if (offset < 0)
        offset = UMX_REFERENCE_SHIFT;
    return separate_tracks_f32(ctx, 1, &audio_host, &length, &rate, &offset, 4, nullptr, out_host, flags, progress, progress_user);
}
int umx_hip_separate_tracks_rate(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *length, const int *rate,
                                 const int *shift_offset, float *const *out_host, unsigned flags, void (*progress)(float, void *),
                                 void *progress_user)
{
    if (!ctx || !rate)
        return UMX_ERR_ARG;
    return separate_tracks_f32(ctx, n_tracks, audio_host, length, rate, shift_offset, 4, nullptr, out_host, flags, progress, progress_user);
}

int umx_hip_debug_resample_taps(int rate_in, int rate_out, float *taps, size_t cap, int *phases, int *taps_per_phase, int *first_offset)
{
    ResampleGeom g;
    if (!resample_geom(rate_in, rate_out, g))
        return UMX_ERR_ARG;
    if (phases)
        *phases = g.L;
    if (taps_per_phase)
        *taps_per_phase = g.K;
    if (first_offset)
        *first_offset = -g.D;
    if (!taps || cap < (size_t)g.L * g.K)
        return UMX_ERR_ARG;
    std::vector<float> t;
    resample_taps(g, t);
    std::copy(t.begin(), t.end(), taps);
    return UMX_OK;
}

int umx_hip_shift_inference(umx_hip_ctx *ctx, const float *audio_host, int length, int offset, float *const out_host[4],
                            unsigned flags, void (*progress)(float, void *), void *progress_user)
{
    if (offset < 0)
        offset = UMX_REFERENCE_SHIFT; // umx.cpp:115: rand() % 22050, never seeded in the reference (see umx_hip.h)
    return separate_tracks_f32(ctx, 1, &audio_host, &length, nullptr, &offset, 4, nullptr, out_host, flags, progress, progress_user);
}

// the default offsets of a K-shift ensemble: K steps of MAX_SHIFT / K from `first` on, wrapped into the shift buffer
int umx_hip_ensemble_offsets(int n_shifts, int first, int *offsets_out)
{
    if (n_shifts < 1 || n_shifts > UMX_MAX_SHIFTS || first >= UMX_MAX_SHIFT || !offsets_out)
        return UMX_ERR_ARG;
    if (first < 0)
        first = UMX_REFERENCE_SHIFT;
    for (int k = 0; k < n_shifts; ++k)
        offsets_out[k] = (first + k * (UMX_MAX_SHIFT / n_shifts)) % UMX_MAX_SHIFT;
    return UMX_OK;
}

// the one track as lanes 0 .. K-1 of the whole-track driver, lane k at offsets[k]; K = 1 IS umx_hip_shift_inference_rate
// mix (gains == NULL: none): out_host holds n_out buffers, the mix of the mean
static int shift_ensemble(umx_hip_ctx *ctx, const float *audio_host, int length, int rate, int n_shifts, const int *offsets, int n_out,
                          const float *gains, float *const *out_host, unsigned flags, void (*progress)(float, void *), void *progress_user)
{
    MixSpec spec;
    umx_hip_ctx::TrackOptions opt;
    if (!track_options_checked(ctx, nullptr, MeasureArgs(), n_out, gains, spec, opt))
        return UMX_ERR_ARG;
    if (!umx_hip_ctx::track_job_ok(audio_host, length, 0, out_host, opt.n_host()))
    {
        ctx->set_error(gains ? "shift ensemble: need audio, n_out outputs and length >= 1" : "shift ensemble: need audio, four outputs and length >= 1");
        return UMX_ERR_ARG;
    }
    if (n_shifts < 1 || n_shifts > UMX_MAX_SHIFTS || n_shifts > ctx->B)
    {
        ctx->set_error("shift ensemble: need 1 <= n_shifts <= the context's track count (umx_hip_create_tracks), at most " +
                       std::to_string(UMX_MAX_SHIFTS));
        return UMX_ERR_ARG;
    }
    if (flags & UMX_FLAG_RESET_SEGMENTS)
    {
        ctx->set_error("shift ensemble: UMX_FLAG_RESET_SEGMENTS does not go with it (the track lanes carry the shifts)");
        return UMX_ERR_ARG;
    }
    int off[UMX_MAX_SHIFTS];
    if (!offsets)
        (void)umx_hip_ensemble_offsets(n_shifts, -1, off);
    for (int k = 0; k < n_shifts && offsets; ++k)
    {
        if (offsets[k] < 0 || offsets[k] >= UMX_MAX_SHIFT)
        {
            ctx->set_error("shift ensemble: offsets must be 0 .. 22049");
            return UMX_ERR_ARG;
        }
        off[k] = offsets[k];
    }
    const void *audio[UMX_MAX_SHIFTS];
    int lengths[UMX_MAX_SHIFTS], rates[UMX_MAX_SHIFTS];
    for (int k = 0; k < n_shifts; ++k)
    {
        audio[k] = audio_host;
        lengths[k] = length;
        rates[k] = rate;
    }
    umx_hip_ctx::TrackRequest rq = track_request(n_shifts, audio, lengths, rates, off, reinterpret_cast<void *const *>(out_host), flags, progress,
                                                 progress_user, opt, MeasureArgs());
    rq.ensemble = n_shifts > 1;
    return ctx->tracks(rq);
}
int umx_hip_shift_ensemble(umx_hip_ctx *ctx, const float *audio_host, int length, int rate, int n_shifts, const int *offsets,
                           float *const out_host[4], unsigned flags, void (*progress)(float, void *), void *progress_user)
{
    return ctx ? shift_ensemble(ctx, audio_host, length, rate, n_shifts, offsets, 4, nullptr, out_host, flags, progress, progress_user) : UMX_ERR_ARG;
}

// ---------------------------------------------------------------- stem mix matrix (stem_mix.h)
int umx_hip_mix_columns(int n_out, const float *gains) { return mix_spec_from(n_out, gains, nullptr); }

// (the two entry points that ARE the mix refuse NULL gains, in the mix's words; the wider rungs read them as "no mix")
int umx_hip_separate_tracks_mix(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *length, const int *rate,
                                const int *shift_offset, int n_out, const float *gains, float *const *out_host, unsigned flags,
                                void (*progress)(float, void *), void *progress_user)
{
    MixSpec spec;
    if (!ctx || (!gains && !mix_checked(ctx, n_out, gains, spec)))
        return UMX_ERR_ARG;
    return separate_tracks_f32(ctx, n_tracks, audio_host, length, rate, shift_offset, n_out, gains, out_host, flags, progress, progress_user);
}

int umx_hip_shift_ensemble_mix(umx_hip_ctx *ctx, const float *audio_host, int length, int rate, int n_shifts, const int *offsets, int n_out,
                               const float *gains, float *const *out_host, unsigned flags, void (*progress)(float, void *),
                               void *progress_user)
{
    MixSpec spec;
    if (!ctx || (!gains && !mix_checked(ctx, n_out, gains, spec)))
        return UMX_ERR_ARG;
    return shift_ensemble(ctx, audio_host, length, rate, n_shifts, offsets, n_out, gains, out_host, flags, progress, progress_user);
}

// ---------------------------------------------------------------- track queue (engine_queue.h)
// The five queue entry points differ in their done callback, and with it in what every job measures: a levels, loudness or true-peak
// callback makes every job measure what it receives (QueueDone::measures, ::loudness).  Their options are checked
// as a track call's.
static int queue_entry(umx_hip_ctx *ctx, umx_queue_next_fn next, const umx_hip_ctx::QueueDone &done, void *user, int n_out, const float *gains,
                       unsigned flags, const umx_sample_io *io, int clip_mode, int true_peak_mode)
{
    if (!ctx)
        return UMX_ERR_ARG;
    MeasureArgs ma;
    ma.clip_mode = clip_mode;
    ma.true_peak_mode = true_peak_mode;
    MixSpec spec;
    umx_hip_ctx::TrackOptions opt;
    if (!track_options_checked(ctx, io, ma, n_out, gains, spec, opt))
        return UMX_ERR_ARG;
    opt.levels = done.measures();
    opt.loudness = done.loudness();
    opt.true_peak_record = done.with_true_peak != nullptr;
    return ctx->queue(next, done, user, opt, flags);
}
int umx_hip_separate_queue(umx_hip_ctx *ctx, umx_queue_next_fn next, umx_queue_done_fn done, void *user, int n_out, const float *gains,
                           unsigned flags)
{
    return queue_entry(ctx, next, {done}, user, n_out, gains, flags, nullptr, UMX_CLIP_CLAMP, UMX_TRUE_PEAK_OFF);
}

// ---------------------------------------------------------------- 16-bit PCM in and out (pcm16.h)
// io == NULL or fp32 both ways: the fp32 call itself
int umx_hip_separate_tracks_io(umx_hip_ctx *ctx, int n_tracks, const void *const *audio_host, const int *length, const int *rate,
                               const int *shift_offset, int n_out, const float *gains, void *const *out_host, unsigned flags,
                               const umx_sample_io *io, void (*progress)(float, void *), void *progress_user)
{
    return separate_tracks(ctx, n_tracks, audio_host, length, rate, shift_offset, n_out, gains, out_host, flags, io, MeasureArgs(), progress,
                           progress_user);
}

int umx_hip_separate_queue_io(umx_hip_ctx *ctx, umx_queue_next_fn next, umx_queue_done_fn done, void *user, int n_out, const float *gains,
                              unsigned flags, const umx_sample_io *io)
{
    return queue_entry(ctx, next, {done}, user, n_out, gains, flags, io, UMX_CLIP_CLAMP, UMX_TRUE_PEAK_OFF);
}

int umx_hip_pcm16_decode_device(umx_hip_ctx *ctx, const int16_t *in_dev, int n, float *out_dev, void *hip_stream)
{
    return decode_device(ctx, "pcm16 decode", UMX_SAMPLE_S16, in_dev, n, out_dev, hip_stream);
}
int umx_hip_pcm16_encode_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                                const umx_sample_io *io, int16_t *const *out_dev, void *hip_stream)
{
    return encode_device(ctx, "pcm16 encode", UMX_SAMPLE_S16, n_buffers, in_dev, n, first_frame, io, reinterpret_cast<void *const *>(out_dev), false,
                         nullptr, hip_stream);
}
int umx_hip_pcm16_decode_host(const int16_t *q, long long n_values, float *x) { return decode_host(SampleS16(), q, n_values, x); }
int umx_hip_pcm16_encode_host(const float *x, int n_frames, int buffer, long long first_frame, const umx_sample_io *io, int16_t *q)
{
    return encode_host(SampleS16(), x, n_frames, buffer, first_frame, io, q);
}

// ---------------------------------------------------------------- packed 24-bit PCM in and out (pcm24.h)
int umx_hip_pcm24_decode_device(umx_hip_ctx *ctx, const void *in_dev, int n, float *out_dev, void *hip_stream)
{
    return decode_device(ctx, "pcm24 decode", UMX_SAMPLE_S24, in_dev, n, out_dev, hip_stream);
}
int umx_hip_pcm24_encode_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                                const umx_sample_io *io, void *const *out_dev, void *hip_stream)
{
    return encode_device(ctx, "pcm24 encode", UMX_SAMPLE_S24, n_buffers, in_dev, n, first_frame, io, out_dev, false, nullptr, hip_stream);
}
int umx_hip_pcm24_encode_rescaled_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                                         const umx_sample_io *io, void *const *out_dev, umx_levels_acc *acc_dev, void *hip_stream)
{
    return encode_device(ctx, "rescaled pcm24 encode", UMX_SAMPLE_S24, n_buffers, in_dev, n, first_frame, io, out_dev, true, acc_dev, hip_stream);
}
// n_values samples of 3 bytes each
int umx_hip_pcm24_decode_host(const void *q, long long n_values, float *x) { return decode_host(SampleS24(), q, n_values, x); }
int umx_hip_pcm24_encode_host(const float *x, int n_frames, int buffer, long long first_frame, const umx_sample_io *io, void *q)
{
    return encode_host(SampleS24(), x, n_frames, buffer, first_frame, io, q);
}

// the output format whose plain encode clamps what levels count as clipped (io == NULL or an fp32 output: none)
static int clip_format_of(const umx_sample_io *io) { return io ? io->out_format : UMX_SAMPLE_F32; }
// ---------------------------------------------------------------- output levels and clip handling (levels.h)
// clip_mode == UMX_CLIP_CLAMP and levels == NULL: the request of umx_hip_separate_tracks_io, field for field
int umx_hip_separate_tracks_levels(umx_hip_ctx *ctx, int n_tracks, const void *const *audio_host, const int *length, const int *rate,
                                   const int *shift_offset, int n_out, const float *gains, void *const *out_host, unsigned flags,
                                   const umx_sample_io *io, int clip_mode, umx_levels *levels, void (*progress)(float, void *),
                                   void *progress_user)
{
    const MeasureArgs ma = {clip_mode, levels};
    return separate_tracks(ctx, n_tracks, audio_host, length, rate, shift_offset, n_out, gains, out_host, flags, io, ma, progress, progress_user);
}

int umx_hip_separate_queue_levels(umx_hip_ctx *ctx, umx_queue_next_fn next, umx_queue_levels_fn done, void *user, int n_out,
                                  const float *gains, unsigned flags, const umx_sample_io *io, int clip_mode)
{
    return queue_entry(ctx, next, {nullptr, done}, user, n_out, gains, flags, io, clip_mode, UMX_TRUE_PEAK_OFF);
}

int umx_hip_levels_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                          const umx_sample_io *io, umx_levels_acc *acc_dev, void *hip_stream)
{
    if (!ctx)
        return UMX_ERR_ARG;
    const float2 *src[4] = {};
    if (!device_buffers(ctx, "levels", n_buffers, in_dev, n, first_frame, src))
        return UMX_ERR_ARG;
    if (!acc_dev)
    {
        ctx->set_error("levels: null record");
        return UMX_ERR_ARG;
    }
    UMX_HIP_CHECK_CTX(ctx, hipSetDevice(ctx->device));
    const DitherArg d = dither_of(io);
    launch_stem_levels(n_buffers, src, n, first_frame, clip_format_of(io), d.on, d.seed, acc_dev, (hipStream_t)hip_stream);
    UMX_HIP_CHECK_CTX(ctx, hipGetLastError());
    return UMX_OK;
}

int umx_hip_pcm16_encode_rescaled_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, long long first_frame,
                                         const umx_sample_io *io, int16_t *const *out_dev, umx_levels_acc *acc_dev, void *hip_stream)
{
    return encode_device(ctx, "rescaled pcm16 encode", UMX_SAMPLE_S16, n_buffers, in_dev, n, first_frame, io, reinterpret_cast<void *const *>(out_dev),
                         true, acc_dev, hip_stream);
}

int umx_hip_rescale_device(umx_hip_ctx *ctx, int n_buffers, float *const *bufs_dev, int n, const umx_levels_acc *acc_dev, void *hip_stream)
{
    if (!ctx)
        return UMX_ERR_ARG;
    float2 *p[4] = {};
    if (!device_buffers(ctx, "rescale", n_buffers, bufs_dev, n, 0, p))
        return UMX_ERR_ARG;
    if (!acc_dev)
    {
        ctx->set_error("rescale: null record");
        return UMX_ERR_ARG;
    }
    UMX_HIP_CHECK_CTX(ctx, hipSetDevice(ctx->device));
    launch_stem_rescale(n_buffers, p, n, levels_peak_words(acc_dev), (hipStream_t)hip_stream);
    UMX_HIP_CHECK_CTX(ctx, hipGetLastError());
    return UMX_OK;
}

int umx_hip_levels_host(const float *x, int n_frames, int buffer, long long first_frame, const umx_sample_io *io, float clip_divisor,
                        umx_levels_acc *acc)
{
    if (!x || !acc || n_frames < 0 || buffer < 0 || buffer >= UMX_MAX_MIX_OUTPUTS || first_frame < 0)
        return UMX_ERR_ARG;
    const DitherArg d = dither_of(io);
    levels_host(x, n_frames, buffer, first_frame, clip_format_of(io), d.on, d.seed, clip_divisor, *acc);
    return UMX_OK;
}

float umx_hip_rescale_gain(const float *peak, int n)
{
    uint32_t p = 0;
    for (int m = 0; peak && m < n; ++m)
        p = std::max(p, levels_abs_bits(peak[m]));
    return levels_divisor(p);
}

// ---------------------------------------------------------------- loudness of every output (loudness.h)
// loudness == NULL and hop_energy == NULL: the request of umx_hip_separate_tracks_levels, field for field
int umx_hip_separate_tracks_loudness(umx_hip_ctx *ctx, int n_tracks, const void *const *audio_host, const int *length, const int *rate,
                                     const int *shift_offset, int n_out, const float *gains, void *const *out_host, unsigned flags,
                                     const umx_sample_io *io, int clip_mode, umx_levels *levels, umx_loudness *loudness,
                                     double *const *hop_energy, void (*progress)(float, void *), void *progress_user)
{
    const MeasureArgs ma = {clip_mode, levels, loudness, hop_energy};
    return separate_tracks(ctx, n_tracks, audio_host, length, rate, shift_offset, n_out, gains, out_host, flags, io, ma, progress, progress_user);
}

int umx_hip_separate_queue_loudness(umx_hip_ctx *ctx, umx_queue_next_fn next, umx_queue_loudness_fn done, void *user, int n_out,
                                    const float *gains, unsigned flags, const umx_sample_io *io, int clip_mode)
{
    return queue_entry(ctx, next, {nullptr, nullptr, done}, user, n_out, gains, flags, io, clip_mode, UMX_TRUE_PEAK_OFF);
}

// ---------------------------------------------------------------- true peak of every output (true_peak.h)
// UMX_TRUE_PEAK_OFF and true_peak == NULL: the request of umx_hip_separate_tracks_loudness, field for field
int umx_hip_separate_tracks_true_peak(umx_hip_ctx *ctx, int n_tracks, const void *const *audio_host, const int *length, const int *rate,
                                      const int *shift_offset, int n_out, const float *gains, void *const *out_host, unsigned flags,
                                      const umx_sample_io *io, int clip_mode, umx_levels *levels, umx_loudness *loudness,
                                      double *const *hop_energy, int true_peak_mode, umx_true_peak *true_peak,
                                      void (*progress)(float, void *), void *progress_user)
{
    const MeasureArgs ma = {clip_mode, levels, loudness, hop_energy, true_peak_mode, true_peak};
    return separate_tracks(ctx, n_tracks, audio_host, length, rate, shift_offset, n_out, gains, out_host, flags, io, ma, progress, progress_user);
}

int umx_hip_separate_queue_true_peak(umx_hip_ctx *ctx, umx_queue_next_fn next, umx_queue_true_peak_fn done, void *user, int n_out,
                                     const float *gains, unsigned flags, const umx_sample_io *io, int clip_mode, int true_peak_mode)
{
    return queue_entry(ctx, next, {nullptr, nullptr, nullptr, done}, user, n_out, gains, flags, io, clip_mode, true_peak_mode);
}

int umx_hip_true_peak_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, int rate, long long first_frame,
                             long long n_frames, unsigned *bits_dev, void *hip_stream)
{
    if (!ctx)
        return UMX_ERR_ARG;
    if (!true_peak_rate_ok(rate))
    {
        ctx->set_error("true peak: sample rate outside 8000 .. 192000 Hz");
        return UMX_ERR_ARG;
    }
    const float2 *src[4] = {};
    if (!device_buffers(ctx, "true peak", n_buffers, in_dev, n, first_frame, src))
        return UMX_ERR_ARG;
    if (!bits_dev || n > 0x7fffffff / 2 || n_frames < 0 || first_frame > n || n_frames > n - first_frame)
    {
        ctx->set_error("true peak: need the record, n <= 2^30 - 1 and 0 <= first_frame, first_frame + n_frames <= n");
        return UMX_ERR_ARG;
    }
    UMX_HIP_CHECK_CTX(ctx, hipSetDevice(ctx->device));
    launch_true_peak(n_buffers, src, n, rate, first_frame, n_frames, bits_dev, (hipStream_t)hip_stream);
    UMX_HIP_CHECK_CTX(ctx, hipGetLastError());
    return UMX_OK;
}

int umx_hip_true_peak_taps(int rate, float taps[49], int *factor)
{
    if (!true_peak_rate_ok(rate) || !taps || !factor)
        return UMX_ERR_ARG;
    *factor = true_peak_factor(rate);
    const TruePeakTaps tp = true_peak_taps(*factor);
    std::copy(tp.h, tp.h + TP_TAPS, taps);
    return UMX_OK;
}

int umx_hip_true_peak_host(const float *x, int n, int rate, long long first_frame, long long n_frames, unsigned *bits)
{
    if (!x || !bits || n < 1 || !true_peak_rate_ok(rate) || first_frame < 0 || n_frames < 0 || first_frame > n || n_frames > n - first_frame)
        return UMX_ERR_ARG;
    *bits = true_peak_host(x, n, rate, first_frame, n_frames, *bits);
    return UMX_OK;
}

int umx_hip_kweight_hops_device(umx_hip_ctx *ctx, int n_buffers, const float *const *in_dev, int n, int rate, long long first_hop,
                                long long n_hops, double *E_dev, void *hip_stream)
{
    if (!ctx)
        return UMX_ERR_ARG;
    if (!kweight_rate_ok(rate))
    {
        ctx->set_error("k-weighted hops: sample rate outside 8000 .. 192000 Hz");
        return UMX_ERR_ARG;
    }
    const float2 *src[4] = {};
    if (!device_buffers(ctx, "k-weighted hops", n_buffers, in_dev, n, 0, src))
        return UMX_ERR_ARG;
    const int hop = kweight_hop(rate);
    const long long hops_total = n / hop;
    if (!E_dev || n > 0x7fffffff / 2 || first_hop < 0 || n_hops < 0 || first_hop > hops_total || n_hops > hops_total - first_hop)
    {
        ctx->set_error("k-weighted hops: need E, n <= 2^30 - 1 and 0 <= first_hop, first_hop + n_hops <= n / hop");
        return UMX_ERR_ARG;
    }
    UMX_HIP_CHECK_CTX(ctx, hipSetDevice(ctx->device));
    launch_kweight_hops(n_buffers, src, kweight_coeffs(rate), hop, hops_total, first_hop, n_hops, E_dev, (hipStream_t)hip_stream);
    UMX_HIP_CHECK_CTX(ctx, hipGetLastError());
    return UMX_OK;
}

int umx_hip_kweight_coeffs(int rate, double pb[3], double pa[3], double rb[3], double ra[3])
{
    if (!kweight_rate_ok(rate) || !pb || !pa || !rb || !ra)
        return UMX_ERR_ARG;
    const KWeight k = kweight_coeffs(rate);
    pa[0] = ra[0] = 1.0;
    for (int i = 0; i < 3; ++i)
    {
        pb[i] = k.pb[i];
        rb[i] = k.rb[i];
    }
    for (int i = 0; i < 2; ++i)
    {
        pa[1 + i] = k.pa[i];
        ra[1 + i] = k.ra[i];
    }
    return UMX_OK;
}

int umx_hip_kweight_hops_host(const float *x, int n, int rate, long long first_hop, long long n_hops, double *E)
{
    if (!x || !E || n < 1 || !kweight_rate_ok(rate))
        return UMX_ERR_ARG;
    const long long hops_total = n / kweight_hop(rate);
    if (first_hop < 0 || n_hops < 0 || first_hop > hops_total || n_hops > hops_total - first_hop)
        return UMX_ERR_ARG;
    kweight_hops_host(x, n, rate, first_hop, n_hops, E);
    return UMX_OK;
}

int umx_hip_loudness_gate(const double *E, long long hops, int hop, double *integrated, double *momentary_max, long long *blocks,
                          long long *gated)
{
    if ((!E && hops > 0) || hops < 0 || hop < 1 || !integrated || !momentary_max || !blocks || !gated)
        return UMX_ERR_ARG;
    loudness_gate(E, hops, hop, *integrated, *momentary_max, *blocks, *gated);
    return UMX_OK;
}

int umx_hip_queue_plan(int n_lanes, int n_jobs, const int *seg_count, int *lane_out, int *first_call_out, int *n_calls_out)
{
    return queue_plan(n_lanes, n_jobs, seg_count, lane_out, first_call_out, n_calls_out);
}
int umx_hip_debug_queue_calls(umx_hip_ctx *ctx) { return ctx ? ctx->queue_calls : -1; }
int umx_hip_debug_resample_launches(umx_hip_ctx *ctx, int *forward, int *backward)
{
    if (!ctx || ctx->rs_launches[0] < 0)
        return UMX_ERR_ARG;
    if (forward)
        *forward = ctx->rs_launches[0];
    if (backward)
        *backward = ctx->rs_launches[1];
    return UMX_OK;
}

// the kernel on the caller's device buffers: (2,n) interleaved stems and mixture -> n_out buffers (2,n), queued on hip_stream
int umx_hip_mix_stems_device(umx_hip_ctx *ctx, int n_out, const float *gains, const float *const stems_dev[4], const float *mix_dev, int n,
                             float *const *out_dev, void *hip_stream)
{
    if (!ctx)
        return UMX_ERR_ARG;
    MixSpec spec;
    if (!mix_checked(ctx, n_out, gains, spec))
        return UMX_ERR_ARG;
    if (n < 1 || !out_dev)
    {
        ctx->set_error("mix: need n >= 1 and n_out output buffers");
        return UMX_ERR_ARG;
    }
    const float2 *src[MIX_COLUMNS] = {};
    float2 *dst[UMX_MAX_MIX_OUTPUTS] = {};
    for (int c = 0; c < MIX_COLUMNS; ++c)
    {
        const float *p = c == MIX_MIXTURE ? mix_dev : (stems_dev ? stems_dev[c] : nullptr);
        if ((spec.cols >> c & 1u) && !p)
        {
            ctx->set_error("mix: a column with a nonzero gain has no buffer");
            return UMX_ERR_ARG;
        }
        src[c] = reinterpret_cast<const float2 *>(p);
    }
    for (int m = 0; m < n_out; ++m)
    {
        if (!out_dev[m])
        {
            ctx->set_error("mix: need n >= 1 and n_out output buffers");
            return UMX_ERR_ARG;
        }
        dst[m] = reinterpret_cast<float2 *>(out_dev[m]);
    }
    UMX_HIP_CHECK_CTX(ctx, hipSetDevice(ctx->device));
    launch_stem_mix(spec, src, dst, n, (hipStream_t)hip_stream);
    UMX_HIP_CHECK_CTX(ctx, hipGetLastError());
    return UMX_OK;
}

// measuring: shift_mean_kernel's time in the last umx_hip_shift_ensemble call with more than one shift (events around its launch)
float umx_hip_debug_shift_mean_ms(umx_hip_ctx *ctx)
{
    float ms = -1.f;
    if (!ctx || !ctx->ens_timed || ctx->sync_all() != UMX_OK || hipEventElapsedTime(&ms, ctx->ens_ev[0], ctx->ens_ev[1]) != hipSuccess)
        return -1.f;
    return ms;
}

// testing: the per-bin arithmetic of the Wiener filter -- mix_magnitude, wiener_bin_setup, wiener_bin_apply, the
// functions BOTH filter kernels call -- on caller-given bins, so that a test can hold it against an independent float64
// restatement of wiener.cpp:301-400 in the reference's own operation order (the fused-vs-unfused test compares two callers of
// the same functions).  X [n][2 channels][re, im], masks [n][4 sources][2 channels], R [n][4][R00, Re R01, Im R01, R11],
// y out [n][4][2][re, im].  Needs a current device; no context.
__global__ void debug_wiener_bins_kernel(int n, const float *X, const float *masks, const float *R, float max_abs, float *y)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n)
        return;
    const float2 X0 = make_float2(X[b * 4 + 0], X[b * 4 + 1]), X1 = make_float2(X[b * 4 + 2], X[b * 4 + 3]);
    const float h0 = mix_magnitude(X0), h1 = mix_magnitude(X1);
    float m0[4], m1[4];
    float4 rc[4];
    for (int s = 0; s < 4; ++s)
    {
        m0[s] = masks[(b * 4 + s) * 2 + 0] * h0; // inference.cpp:175-183
        m1[s] = masks[(b * 4 + s) * 2 + 1] * h1;
        rc[s] = make_float4(R[(b * 4 + s) * 4 + 0], R[(b * 4 + s) * 4 + 1], R[(b * 4 + s) * 4 + 2], R[(b * 4 + s) * 4 + 3]);
    }
    WienerBin wb;
    wiener_bin_setup(X0, X1, m0, m1, rc, max_abs, 1.0f / max_abs, wb);
    for (int s = 0; s < 4; ++s)
    {
        float2 o[2];
        wiener_bin_apply(wb, s, rc[s], max_abs, o);
        y[((b * 4 + s) * 2 + 0) * 2 + 0] = o[0].x;
        y[((b * 4 + s) * 2 + 0) * 2 + 1] = o[0].y;
        y[((b * 4 + s) * 2 + 1) * 2 + 0] = o[1].x;
        y[((b * 4 + s) * 2 + 1) * 2 + 1] = o[1].y;
    }
}
int umx_hip_debug_wiener_bins(int n, const float *X, const float *masks, const float *R, float max_abs, float *y)
{
    if (n < 1 || !X || !masks || !R || !y || !(max_abs >= 1.0f))
        return UMX_ERR_ARG;
    float *d = nullptr;
    const size_t nx = (size_t)n * 4, nm = (size_t)n * 8, nr = (size_t)n * 16, ny = (size_t)n * 16;
    if (hipMalloc(reinterpret_cast<void **>(&d), (nx + nm + nr + ny) * sizeof(float)) != hipSuccess)
        return UMX_ERR_HIP;
    bool ok = hipMemcpy(d, X, nx * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d + nx, masks, nm * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + nx + nm, R, nr * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok)
    {
        hipLaunchKernelGGL(debug_wiener_bins_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, d, d + nx, d + nx + nm, max_abs, d + nx + nm + nr);
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(y, d + nx + nm + nr, ny * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    return ok ? UMX_OK : UMX_ERR_HIP;
}

// testing: the gate functions and the cell step on caller-given values (gate_debug.h)
int umx_hip_debug_gate_math(int n, const float *x, float *fn, int n_waves, const float *pre, const float *c, float *cell)
{
    if (n < 0 || n_waves < 0 || (n > 0 && (!x || !fn)) || (n_waves > 0 && (!pre || !c || !cell)) || n > (1 << 24) || n_waves > (1 << 16))
        return UMX_ERR_ARG;
    const size_t nx = (size_t)n, nf = (size_t)5 * n, np_ = (size_t)n_waves * 64, nc = (size_t)n_waves * 16, no = (size_t)n_waves * 128;
    if (nx + np_ == 0)
        return UMX_OK;
    float *d = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d), (nx + nf + np_ + nc + no) * sizeof(float)) != hipSuccess)
        return UMX_ERR_HIP;
    float *dx = d, *dfn = dx + nx, *dpre = dfn + nf, *dc = dpre + np_, *dcell = dc + nc;
    bool ok = true;
    if (n > 0)
    {
        ok = hipMemcpy(dx, x, nx * 4, hipMemcpyHostToDevice) == hipSuccess;
        if (ok)
            hipLaunchKernelGGL(debug_gate_fn_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, n, dx, dfn);
    }
    if (ok && n_waves > 0)
    {
        ok = hipMemcpy(dpre, pre, np_ * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dc, c, nc * 4, hipMemcpyHostToDevice) == hipSuccess;
        if (ok)
        {
            hipLaunchKernelGGL(debug_gate_cell_kernel<0>, dim3(n_waves), dim3(64), 0, nullptr, dpre, dc, dcell);
            hipLaunchKernelGGL(debug_gate_cell_kernel<1>, dim3(n_waves), dim3(64), 0, nullptr, dpre, dc, dcell + nc * 2);
            hipLaunchKernelGGL(debug_gate_cell_kernel<2>, dim3(n_waves), dim3(64), 0, nullptr, dpre, dc, dcell + nc * 4);
            hipLaunchKernelGGL(debug_gate_cell_kernel<3>, dim3(n_waves), dim3(64), 0, nullptr, dpre, dc, dcell + nc * 6);
        }
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (ok && n > 0)
        ok = hipMemcpy(fn, dfn, nf * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && n_waves > 0)
        ok = hipMemcpy(cell, dcell, no * 4, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d);
    return ok ? UMX_OK : UMX_ERR_HIP;
}

// debugging: queue `launches` LDS-guard kernels on a private stream (they run beside whatever the caller
// queues next); read the counters back with launches == 0 (returns words corrupted, events in out2[0..1])
int umx_hip_debug_lds_guard(umx_hip_ctx *ctx, int launches, int rounds, unsigned *out2)
{
    static hipStream_t gs = nullptr;
    static unsigned *errs = nullptr;
    if (!ctx)
        return UMX_ERR_ARG;
    if (!gs)
    {
        if (hipStreamCreateWithFlags(&gs, hipStreamNonBlocking) != hipSuccess || hipMalloc(&errs, 8) != hipSuccess)
            return UMX_ERR_HIP;
        (void)hipMemset(errs, 0, 8);
    }
    for (int i = 0; i < launches; ++i)
        hipLaunchKernelGGL(lds_guard_kernel, dim3(512), dim3(256), 0, gs, errs, rounds);
    if (launches == 0 && out2)
    {
        (void)hipStreamSynchronize(gs);
        (void)hipMemcpy(out2, errs, 8, hipMemcpyDeviceToHost);
        (void)hipMemset(errs, 0, 8);
    }
    return UMX_OK;
}

int umx_hip_segment_begin(umx_hip_ctx *ctx, const float *audio_host, int n, unsigned flags)
{
    return ctx ? ctx->phase_begin(audio_host, n, flags) : UMX_ERR_ARG;
}
int umx_hip_segment_lstm_layer(umx_hip_ctx *ctx, int layer) { return ctx ? ctx->phase_layer(layer) : UMX_ERR_ARG; }
int umx_hip_segment_end(umx_hip_ctx *ctx, float *const out_host[4]) { return ctx ? ctx->phase_end(out_host) : UMX_ERR_ARG; }

void *umx_hip_phase_stream(umx_hip_ctx *ctx) { return ctx ? (void *)ctx->slot[0].stream : nullptr; }
float *umx_hip_stream_state_device(umx_hip_ctx *ctx) { return ctx ? ctx->state : nullptr; }
int umx_hip_segment_begin_device(umx_hip_ctx *ctx, const float *audio_dev, int n, unsigned flags)
{
    return ctx ? ctx->phase_begin_device(audio_dev, n, flags) : UMX_ERR_ARG;
}
int umx_hip_segment_end_device(umx_hip_ctx *ctx, float *const out_dev[4]) { return ctx ? ctx->phase_end_device(out_dev) : UMX_ERR_ARG; }
int umx_hip_segment_masks_device(umx_hip_ctx *ctx) { return ctx ? ctx->phase_masks() : UMX_ERR_ARG; }
int umx_hip_segment_residual_device(umx_hip_ctx *ctx) { return ctx ? ctx->phase_residual() : UMX_ERR_ARG; }
int umx_hip_residual_slot(unsigned flags) { return residual_slot_of(flags); }
int umx_hip_segment_discard(umx_hip_ctx *ctx)
{
    if (!ctx)
        return UMX_ERR_ARG;
    stage_range(-1);
    ctx->ph_next = -1; // whatever was queued runs to its end; the next segment may begin
    ctx->cur = 0;
    ctx->clear_used();
    return UMX_OK;
}
int umx_hip_segment_finish_device(umx_hip_ctx *ctx, float *const out_dev[4]) { return ctx ? ctx->phase_finish_device(out_dev) : UMX_ERR_ARG; }
float *umx_hip_target_mag_device(umx_hip_ctx *ctx, int target, size_t *floats)
{
    if (!ctx || target < 0 || target > 3)
        return nullptr;
    if (floats)
        *floats = (size_t)2 * ctx->T * MAGP;
    return ctx->slot[0].lane[0].ta[target].mag;
}
int umx_hip_gate_reserve(int device, int cus)
{
    if (device < 0)
        return UMX_ERR_ARG;
    LstmGate &g = g_gate[device & 15];
    std::lock_guard<std::mutex> lock(g.m);
    if (cus > 0)
        g.reservations.push_back(cus);
    else if (cus < 0) // gives ONE request of that size back: another driver's request on the same device stays
    {
        auto it = std::find(g.reservations.begin(), g.reservations.end(), -cus);
        if (it == g.reservations.end())
            return UMX_ERR_ARG;
        g.reservations.erase(it);
    }
    else
        g.reservations.clear();
    // every driver keeps its OWN send / recv kernels resident: what must stay free is the SUM of the outstanding requests
    // (lstm_gate_launch clamps it to half the chip)
    g.reserved = 2 * std::accumulate(g.reservations.begin(), g.reservations.end(), 0);
    return UMX_OK;
}

static Stems4 stems4(float *const p[4])
{
    Stems4 s;
    for (int t = 0; t < 4; ++t)
        s.p[t] = reinterpret_cast<float2 *>(p[t]);
    return s;
}
int umx_hip_weight_stems_device(umx_hip_ctx *ctx, float *const stems_dev[4], int n, void *hip_stream)
{
    if (!ctx || !stems_dev || n < 1)
        return UMX_ERR_ARG;
    hipLaunchKernelGGL(track_weight_kernel, dim3((n + 255) / 256, 4), dim3(256), 0, (hipStream_t)hip_stream, stems4(stems_dev), n, ctx->N);
    return hipGetLastError() == hipSuccess ? UMX_OK : UMX_ERR_HIP;
}
int umx_hip_track_accumulate_device(umx_hip_ctx *ctx, float *const track_dev[4], float *sum_weight_dev,
                                    const float *const weighted_dev[4], int offset, int n, void *hip_stream)
{
    if (!ctx || !track_dev || !sum_weight_dev || !weighted_dev || n < 1 || offset < 0)
        return UMX_ERR_ARG;
    float *w[4] = {const_cast<float *>(weighted_dev[0]), const_cast<float *>(weighted_dev[1]), const_cast<float *>(weighted_dev[2]),
                   const_cast<float *>(weighted_dev[3])};
    hipLaunchKernelGGL(track_add_weighted_kernel, dim3((n + 255) / 256, 4), dim3(256), 0, (hipStream_t)hip_stream, stems4(track_dev),
                       sum_weight_dev, stems4(w), offset, n, ctx->N);
    return hipGetLastError() == hipSuccess ? UMX_OK : UMX_ERR_HIP;
}
int umx_hip_track_normalise_device(umx_hip_ctx *ctx, float *const track_dev[4], const float *sum_weight_dev, int length,
                                   void *hip_stream)
{
    if (!ctx || !track_dev || !sum_weight_dev || length < 1)
        return UMX_ERR_ARG;
    hipLaunchKernelGGL(track_normalise_kernel, dim3((length + 255) / 256, 4), dim3(256), 0, (hipStream_t)hip_stream, stems4(track_dev),
                       sum_weight_dev, 0, length);
    return hipGetLastError() == hipSuccess ? UMX_OK : UMX_ERR_HIP;
}

int umx_hip_infer_segment_device(umx_hip_ctx *ctx, const float *audio_dev, int n, float *const out_dev[4],
                                 unsigned flags)
{
    if (!ctx || !out_dev)
        return UMX_ERR_ARG;
    return ctx->infer_device(audio_dev, n, out_dev, flags);
}

int umx_hip_infer_batch_device(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_dev, const int *n,
                               float *const *out_dev, unsigned flags)
{
    if (!ctx)
        return UMX_ERR_ARG;
    return ctx->infer_batch(n_tracks, audio_dev, n, out_dev, flags);
}

// Ordering against the caller's own HIP streams (the engine alternates between two internal streams)
int umx_hip_order_after(umx_hip_ctx *ctx, void *hip_stream)
{
    if (!ctx)
        return UMX_ERR_ARG;
    hipError_t e = hipSuccess;
    if (!ctx->order_ev)
        e = hipEventCreateWithFlags(&ctx->order_ev, hipEventDisableTiming);
    if (e == hipSuccess)
        e = hipEventRecord(ctx->order_ev, (hipStream_t)hip_stream);
    for (int si = 0; si < ctx->nslots && e == hipSuccess; ++si)
        e = hipStreamWaitEvent(ctx->slot[si].stream, ctx->order_ev, 0);
    if (e != hipSuccess)
    {
        ctx->set_error(hipGetErrorString(e));
        return UMX_ERR_HIP;
    }
    return UMX_OK;
}
int umx_hip_order_before(umx_hip_ctx *ctx, void *hip_stream)
{
    if (!ctx)
        return UMX_ERR_ARG;
    // the caller may recycle the buffers of the calls queued so far once its stream is ordered behind them: they can no
    // longer be replayed, so a timeout among them ends as UMX_ERR_TIMEOUT at the next umx_hip_sync (and the log of
    // queued calls stops growing for callers that never call umx_hip_sync)
    if (!ctx->pending.empty())
    {
        ctx->pending_lost = true;
        ctx->pending.clear();
    }
    hipError_t e = hipSuccess;
    if (!ctx->order_ev)
        e = hipEventCreateWithFlags(&ctx->order_ev, hipEventDisableTiming);
    for (int si = 0; si < ctx->nslots && e == hipSuccess; ++si)
    {
        e = hipEventRecord(ctx->order_ev, ctx->slot[si].stream);
        if (e == hipSuccess)
            e = hipStreamWaitEvent((hipStream_t)hip_stream, ctx->order_ev, 0);
    }
    // the host-pointer calls download their stems on a stream of their own: "everything queued so far" includes those copies
    if (ctx->copy_stream && e == hipSuccess)
    {
        e = hipEventRecord(ctx->order_ev, ctx->copy_stream);
        if (e == hipSuccess)
            e = hipStreamWaitEvent((hipStream_t)hip_stream, ctx->order_ev, 0);
    }
    if (e != hipSuccess)
    {
        ctx->set_error(hipGetErrorString(e));
        return UMX_ERR_HIP;
    }
    return UMX_OK;
}

int umx_hip_sync(umx_hip_ctx *ctx)
{
    if (!ctx)
        return UMX_ERR_ARG;
    if (int rc = ctx->sync_all())
        return rc;
    for (int si = 0; si < ctx->nslots; ++si)
    {
        unsigned *dev_status = ctx->slot[si].status;
        if (!dev_status)
            continue;
        unsigned st = 0;
        hipError_t e = hipMemcpy(&st, dev_status, sizeof st, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
        {
            ctx->set_error(hipGetErrorString(e));
            return UMX_ERR_HIP;
        }
        if (st != 0)
        {
            const std::string what = st == 0x80000000u
                                         ? std::string("persistent LSTM kernel: grid barrier timed out (grid not co-resident)")
                                         : "persistent LSTM kernel timed out waiting for a hidden-state granule (code " + std::to_string(st) + ")";
            for (int sj = 0; sj < ctx->nslots; ++sj)
                (void)hipMemset(ctx->slot[sj].status, 0, sizeof(unsigned));
            (void)hipStreamSynchronize(nullptr); // (null-stream memsets are not ordered against the slots' non-blocking streams)
            ctx->persistent_ok = false; // later launches use the per-step driver
            const size_t ncalls = ctx->pending.size();
            if (!ctx->no_recovery && !ctx->pending_lost && ncalls >= 1 && ncalls <= (size_t)umx_hip_ctx::kBackupCalls)
            {
                const int rc = ctx->recover();
                if (rc == UMX_OK)
                {
                    ctx->set_error("recovered: " + what + "; " + std::to_string(ncalls) + " queued segment call(s) were run again with the "
                                   "per-step LSTM driver (bit-identical), which later calls of this context use as well");
                    return UMX_OK;
                }
            }
            // no way back: the aborted launch left a mix of updated and stale chains behind
            (void)hipMemset(ctx->state, 0, sizeof(float) * ctx->state_floats() * ctx->B);
            (void)hipStreamSynchronize(nullptr);
            ctx->clear_used();
            ctx->pending.clear();
            ctx->pending_lost = false;
            ctx->set_error(what + "; the streaming LSTM state was reset to zero, later segments run the per-step driver");
            return UMX_ERR_TIMEOUT;
        }
    }
    ctx->pending.clear();
    ctx->pending_lost = false;
    return UMX_OK;
}

// Host-pointer forms.  H2D, kernels and D2H are queued on the stream of the pipeline slot the segment runs in, so
// with PINNED host buffers consecutive _async calls overlap one segment's transfers with the other's kernels.
int umx_hip_infer_batch_async(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *n,
                              float *const *out_host, unsigned flags)
{
    if (!ctx || !audio_host || !n || !out_host || n_tracks < 1 || n_tracks > ctx->B)
    {
        if (ctx)
            ctx->set_error("infer: bad arguments");
        return UMX_ERR_ARG;
    }
    if (int rc = ctx->check_flags(flags)) // (before anything is uploaded)
        return rc;
    const int si = ctx->next_slot();
    if (int rc = ctx->ensure_staging())
        return rc;
    Slot &sl = ctx->slot[si];
    hipStream_t st = sl.stream;
    const float *ain[LSTMB_MAX_TRACKS] = {};
    for (int ln = 0; ln < n_tracks; ++ln)
    {
        if (!audio_host[ln])
            continue;
        if (n[ln] < 1 || n[ln] > ctx->N)
        {
            ctx->set_error("infer_segment: need 1 <= n <= segment_samples");
            return UMX_ERR_ARG;
        }
        float *dst = ctx->stage_in[si] + (size_t)2 * ctx->N * ln;
        hipError_t e = hipMemcpyAsync(dst, audio_host[ln], sizeof(float) * 2 * (size_t)n[ln], hipMemcpyHostToDevice, st);
        if (e != hipSuccess)
        {
            ctx->set_error(hipGetErrorString(e));
            return UMX_ERR_HIP;
        }
        ain[ln] = dst;
    }
    if (int rc = ctx->infer_batch(n_tracks, ain, n, ctx->stage_out[si], flags))
        return rc;
    UMX_HIP_CHECK_CTX(ctx, hipEventRecord(sl.k_done, st));
    if (!ctx->pending_lost && !ctx->pending.empty())
    {
        for (int k = 0; k < 4 * n_tracks; ++k)
            ctx->pending.back().host_out[k] = out_host[k];
        for (int ln = 0; ln < n_tracks; ++ln)
            ctx->pending.back().host_audio[ln] = ain[ln] ? audio_host[ln] : nullptr;
    }
    // the stems go out on the copy stream as soon as they are complete, beside whatever runs next (see queue_download)
    umx_hip_ctx::DeferredDownload d;
    d.valid = true;
    d.si = si;
    d.nb = n_tracks;
    for (int ln = 0; ln < n_tracks; ++ln)
    {
        d.n[ln] = ain[ln] ? n[ln] : 0;
        for (int s = 0; s < 4; ++s)
            d.host[4 * ln + s] = out_host[4 * ln + s];
    }
    return ctx->queue_download(d, ctx->copy_stream);
}

int umx_hip_infer_batch(umx_hip_ctx *ctx, int n_tracks, const float *const *audio_host, const int *n, float *const *out_host,
                        unsigned flags)
{
    if (int rc = umx_hip_infer_batch_async(ctx, n_tracks, audio_host, n, out_host, flags))
        return rc;
    return umx_hip_sync(ctx);
}

int umx_hip_infer_segment_async(umx_hip_ctx *ctx, const float *audio_host, int n, float *const out_host[4], unsigned flags)
{
    if (!ctx || !audio_host || !out_host)
    {
        if (ctx)
            ctx->set_error("infer_segment: bad arguments");
        return UMX_ERR_ARG;
    }
    return umx_hip_infer_batch_async(ctx, 1, &audio_host, &n, out_host, flags);
}

int umx_hip_infer_segment(umx_hip_ctx *ctx, const float *audio_host, int n, float *const out_host[4], unsigned flags)
{
    if (int rc = umx_hip_infer_segment_async(ctx, audio_host, n, out_host, flags))
        return rc;
    return umx_hip_sync(ctx); // umx_inference returns its outputs: synchronous
}

void *umx_hip_stream_handle(umx_hip_ctx *ctx) { return ctx ? (void *)ctx->slot[ctx->cur].stream : nullptr; }
int umx_hip_nb_frames(const umx_hip_ctx *ctx) { return ctx ? ctx->T : 0; }
int umx_hip_segment_samples(const umx_hip_ctx *ctx) { return ctx ? ctx->N : 0; }
int umx_hip_hidden(const umx_hip_ctx *ctx) { return ctx ? ctx->H : 0; }

long umx_hip_read_tap(umx_hip_ctx *ctx, const char *what, int target, float *dst, size_t cap)
{
    if (!ctx || !what || target < 0 || target > 3)
        return -1;
    std::string w = what;
    const int T = ctx->T, H = ctx->H;
    int which = ctx->cur, lane = 0;
    {
        const size_t hash = w.find('#'); // "name#k": track lane k (default 0)
        if (hash != std::string::npos)
        {
            lane = atoi(w.c_str() + hash + 1);
            const size_t at = w.find('@', hash);
            w = w.substr(0, hash) + (at == std::string::npos ? "" : w.substr(at));
            if (lane < 0 || lane >= ctx->B)
                return -1;
        }
    }
    if (w.size() > 2 && w[w.size() - 2] == '@') // "name@s": pipeline slot s instead of the most recent one
    {
        which = w.back() - '0';
        w = w.substr(0, w.size() - 2);
        if (which < 0 || which >= ctx->nslots)
            return -1;
    }
    const Lane &sl = ctx->slot[which].lane[lane];
    const void *src = nullptr;
    size_t nfl = 0, src_ld = 0, rows = 0, cols = 0; // strided copy when src_ld != cols
    int computed = 0; // 1 |X|, 2 mask x |X|, 3 mask as (T, 4098): formed by a tap kernel into ctx->tap_tmp
    if (w == "spec") { src = sl.spec; nfl = (size_t)2 * 2 * T * NBINS; }
    else if (w == "mix_mag") { src = sl.spec; computed = 1; nfl = (size_t)2 * T * NBINS; }
    else if (w == "x") { src = sl.x; nfl = (size_t)T * KX; }
    else if (w == "fc1") { src = sl.ta[target].cat; rows = T; cols = H; src_ld = 2 * H; nfl = rows * cols; }
    else if (w == "lstm") { src = sl.ta[target].cat + H; rows = T; cols = H; src_ld = 2 * H; nfl = rows * cols; }
    else if (w == "lstm_l0") { src = sl.ta[target].la; nfl = (size_t)T * H; }
    else if (w == "lstm_l1") { src = sl.ta[target].lb; nfl = (size_t)T * H; }
    else if (w == "proj") { src = sl.ta[target].P; nfl = (size_t)T * 4 * H; }
    else if (w == "fc2") { src = sl.ta[target].a2; nfl = (size_t)T * H; }
    else if (w == "mask") { src = sl.ta[target].mag; computed = 3; nfl = (size_t)T * NOUT; }
    else if (w == "target_mag") { src = sl.ta[target].mag; computed = 2; nfl = (size_t)2 * T * NBINS; }
    else if (w == "y") { src = sl.y + (size_t)target * 2 * T * NBINS; nfl = (size_t)2 * 2 * T * NBINS; }
    else if (w == "max_abs") { src = sl.maxabs; nfl = 1; }
    else return -1;
    // the recurrence of a track-batched context writes the fp32 rows of a layer only under UMX_FLAG_DEBUG_TAPS when it also writes
    // the next GEMM's planes: without the flag these taps would be stale rows of an earlier call -- unavailable, like "y"
    if ((w == "lstm" && !ctx->slot[which].lstm_rows_f32[2]) || (w == "lstm_l0" && !ctx->slot[which].lstm_rows_f32[0]) ||
        (w == "lstm_l1" && !ctx->slot[which].lstm_rows_f32[1]))
        return -2;
    if (!src)
        return -2;
    if (!dst)
        return (long)nfl;
    if (cap < nfl)
        return -3;
    if (ctx->sync_all() != UMX_OK)
        return -4;
    if (computed)
    {
        if (!ctx->tap_tmp && ctx->dalloc(&ctx->tap_tmp, (size_t)2 * T * NBINS) != UMX_OK)
            return -4;
        const unsigned blocks = (unsigned)((nfl + 255) / 256);
        if (computed == 1)
            hipLaunchKernelGGL(tap_mix_mag_kernel, dim3(blocks), dim3(256), 0, nullptr, sl.spec, nfl, ctx->tap_tmp);
        else if (computed == 2)
            hipLaunchKernelGGL(tap_target_mag_kernel, dim3(blocks), dim3(256), 0, nullptr, sl.spec, sl.ta[target].mag, nfl, ctx->tap_tmp);
        else
            hipLaunchKernelGGL(tap_mask_kernel, dim3(blocks), dim3(256), 0, nullptr, sl.ta[target].mag, T, ctx->tap_tmp);
        if (hipDeviceSynchronize() != hipSuccess)
            return -4;
        src = ctx->tap_tmp;
    }
    hipError_t e;
    if (rows)
        e = hipMemcpy2D(dst, cols * sizeof(float), src, src_ld * sizeof(float), cols * sizeof(float), rows,
                        hipMemcpyDeviceToHost);
    else
        e = hipMemcpy(dst, src, nfl * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess)
    {
        ctx->set_error(hipGetErrorString(e));
        return -4;
    }
    if (w == "max_abs")
    {
        unsigned bits;
        memcpy(&bits, dst, 4);
        float m;
        memcpy(&m, &bits, 4);
        dst[0] = std::max(1.0f, m / WIENER_SCALE);
    }
    return (long)nfl;
}

int umx_hip_stage_times_slot(umx_hip_ctx *ctx, int slot_index, const char **names, float *ms, int cap);
int umx_hip_stage_times(umx_hip_ctx *ctx, const char **names, float *ms, int cap)
{
    return ctx ? umx_hip_stage_times_slot(ctx, ctx->cur, names, ms, cap) : 0;
}

int umx_hip_stage_times_slot(umx_hip_ctx *ctx, int slot_index, const char **names, float *ms, int cap)
{
    if (!ctx || slot_index < 0 || slot_index >= ctx->nslots)
        return 0;
    Slot &sl = ctx->slot[slot_index];
    if (!sl.have_times || ctx->sync_all() != UMX_OK)
        return 0;
    int n = std::min(cap, (int)ST_COUNT);
    for (int i = 0; i < n; ++i)
    {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, sl.ev[i], sl.ev[i + 1]);
        if (names)
            names[i] = kStageNames[i];
        if (ms)
            ms[i] = t;
    }
    return ST_COUNT;
}

// per stage: the time from the event recorded BEHIND the stage's split kernel to the next stage's event, i.e. the stage's main
// kernel alone (GEMM stages of plane contexts); the stage time where there is no such event.  Same conventions as umx_hip_stage_times_slot.
int umx_hip_stage_kernel_times_slot(umx_hip_ctx *ctx, int slot_index, float *ms, int cap)
{
    if (ctx && slot_index < 0)
        slot_index = ctx->cur;
    if (!ctx || slot_index >= ctx->nslots)
        return 0;
    Slot &sl = ctx->slot[slot_index];
    if (!sl.have_times || ctx->sync_all() != UMX_OK)
        return 0;
    const int n = std::min(cap, (int)ST_COUNT);
    for (int i = 0; i < n; ++i)
    {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, sl.evk_set[i] ? sl.evk[i] : sl.ev[i], sl.ev[i + 1]);
        if (ms)
            ms[i] = t;
    }
    return ST_COUNT;
}

const char *umx_hip_lstm_kernel_name(const umx_hip_ctx *ctx) { return ctx ? ctx->lstm_kernel_last : "none"; }

const char *umx_hip_gemm_kernel_name(const umx_hip_ctx *ctx, int mode) { return ctx && mode >= 0 && mode < 4 ? ctx->gemm_kernel_last[mode] : "none"; }

int umx_hip_lstm_was_persistent(const umx_hip_ctx *ctx) { return ctx && ctx->slot[ctx->cur].last_persistent ? 1 : 0; }

int umx_hip_lstm_mode(umx_hip_ctx *ctx)
{
    if (!ctx || !ctx->slot[ctx->cur].last_persistent)
        return 0;
    unsigned st[2] = {0, 0};
    const unsigned *src = ctx->slot[ctx->cur].status;
    if (ctx->sync_all() != UMX_OK || hipMemcpy(st, src, sizeof st, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return st[1] ? 2 : 1;
}

int umx_hip_debug_lstm_profile(umx_hip_ctx *ctx, unsigned long long *out48)
{
    if (!ctx || !out48)
        return UMX_ERR_ARG;
    if (ctx->sync_all() != UMX_OK ||
        hipMemcpy(out48, ctx->slot[ctx->cur].lprof, sizeof(unsigned long long) * 48, hipMemcpyDeviceToHost) != hipSuccess)
        return UMX_ERR_HIP;
    return UMX_OK;
}

// where the workgroups of the last profiled one-track recurrence launch ran: out[i] = xcc << 48 | chain << 40 | slice << 32 | HW_ID
int umx_hip_debug_lstm_placement(umx_hip_ctx *ctx, unsigned long long *out, int n)
{
    if (!ctx || !out || n < 0 || n > 960 + 64 * 8 * 5)
        return UMX_ERR_ARG;
    if (ctx->sync_all() != UMX_OK ||
        hipMemcpy(out, ctx->slot[ctx->cur].lprof + 64, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost) != hipSuccess)
        return UMX_ERR_HIP;
    return UMX_OK;
}

} // extern "C"
