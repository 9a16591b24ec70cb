// engine_tracks.h -- part of engine.hip (one translation unit: the kernels inline into their launchers): whole tracks on the device.
// What every whole-track driver shares, stated once each -- the checks of a job (track_job_ok), its padded geometry (track_geometry),
// the grow-only buffers (grow_only, on dfree, the one release beside dalloc), the admission of a job with the options of its call
// (admit_job: what grows, in which order, and the by_region / whole_region rules; TrackOptions, engine.hip), the measuring side of a job
// (its state TrackMeasure, engine.hip; track_measure_grow, what it checks and allocates; track_measure_spans, what it zeroes;
// track_report, what comes back), what a finished span goes through on its way out (track_leave), the body of one segment call
// (track_call) and the list of finished regions that owns its events (TrackRegions, engine.hip) -- and the driver of
// umx_hip_split_inference / umx_hip_shift_inference / umx_hip_separate_tracks* / umx_hip_shift_ensemble* (tracks, tracks_once): one
// track per lane, or the segments of one track as the lanes (reset mode).
// The track queue is the other driver (engine_queue.h).  Included by engine.hip behind the definition of umx_hip_ctx; not a
// stand-alone header.
// ---------------------------------------------------------------- whole track
// shift_inference (umx.cpp:99-150) around split_inference (umx.cpp:152-295) for rq.n_tracks tracks at once, one per track
// lane: the tracks stay in HBM, call s runs segment s of every track that still has one (a finished track's lane sits
// idle; with one track the segments are queued back to back through the pipeline slots, so consecutive segments overlap exactly as
// in bench.py), the weighted overlap-add and the normalisation run per lane on the device, finished regions are downloaded
// while later segments run.  n_tracks == 1 is umx_hip_split_inference / umx_hip_shift_inference.
int umx_hip_ctx::tracks(const TrackRequest &rq)
{
    // A persistent-kernel timeout inside a track cannot be repaired segment by segment (the overlap-add has consumed
    // the stems): everything is run again, once, with the per-step driver the timeout switches the context to.
    TrackRun run(*this);
    int rc = tracks_once(rq);
    if (rc == UMX_ERR_TIMEOUT) // (a resampled track is resampled again from its host copy, an ensemble placed in its lanes and averaged
                               // again, a mix formed again from fresh accumulators: tracks_once starts from scratch)
        rc = tracks_once(rq);
    return rc;
}

// ---------------------------------------------------------------- what the whole-track drivers share (tracks_once, engine_queue.h)
// The checks of one job: its audio, n_host outputs (`out` itself may be missing), length >= 1, shift offset < UMX_MAX_SHIFT (< 0:
// no shift).  The caller names the refusal.
bool umx_hip_ctx::track_job_ok(const float *audio, int length, int shift_offset, float *const *out, int n_host)
{
    bool ok = audio && out && length >= 1 && shift_offset < UMX_MAX_SHIFT;
    for (int m = 0; ok && m < n_host; ++m)
        ok = out[m] != nullptr;
    return ok;
}

// The padded signal of a track of `length` frames: `lead` frames of silence (the shift), the track, silence up to L2 frames; `segs`
// segments start in it, `stride` frames apart.  false: too long (j is then undefined).
bool umx_hip_ctx::track_geometry(int length, int shift_offset, int stride, TrackJob &j)
{
    // umx.cpp:120-122: length + max_shift - offset -- which the reference overruns for offset > max_shift / 2 (its
    // block write is [offset, offset + length)); the same size where the reference is defined, large enough elsewhere
    const long long l2 = shift_offset < 0 ? (long long)length : (long long)length + std::max(UMX_MAX_SHIFT - shift_offset, shift_offset);
    if (l2 > 0x7fffffff / 2)
        return false;
    j.length = length;
    j.lead = shift_offset < 0 ? 0 : shift_offset;
    j.L2 = (int)l2;
    j.segs = (int)((l2 + stride - 1) / stride); // umx.cpp:214-217
    j.uploaded = j.done44 = j.out_done = 0;
    return true;
}

// The grow-only device buffers of the whole-track drivers (declared in engine.hip): the accumulators and stagings (floats per frame), the
// integer side (words: a frame's bytes rounded up), the hop energies (doubles).
template <class T_> int umx_hip_ctx::grow_only(std::initializer_list<std::pair<T_ **, int>> bufs, size_t &cap, size_t units)
{
    if (units <= cap)
        return UMX_OK;
    for (const auto &b : bufs)
        if (*b.first)
            if (int rc = dfree(*b.first))
                return rc;
    cap = 0;
    const size_t want = units + units / 8;
    for (const auto &b : bufs)
        if (int rc = dalloc(b.first, (size_t)b.second * want, false))
            return rc;
    cap = want;
    return UMX_OK;
}

// the accumulators of one track: the (shifted) track, 4 stems, the weight sum, `frames` frames each
int umx_hip_ctx::track_bufs_grow(TrackBufs &tb_, size_t frames)
{
    return grow_only<float>({{&tb_.in, 2}, {&tb_.out[0], 2}, {&tb_.out[1], 2}, {&tb_.out[2], 2}, {&tb_.out[3], 2}, {&tb_.sumw, 1}}, tb_.cap, frames);
}

// the integer side of an accumulator set for a job of `frames` frames at the caller's rate -- sample_frame_bytes of
// the format a frame, rounded up to whole words: the staging of its upload, n_host outputs, each grow-only on its own
int umx_hip_ctx::track_int_grow(TrackBufs &tb_, const umx_sample_io &io, size_t frames, int n_host)
{
    auto words = [&](int format) { return (sample_frame_bytes(format) * frames + 3) / 4; };
    if (io.in_format != UMX_SAMPLE_F32)
        if (int rc = grow_only<uint32_t>({{&tb_.in_int, 1}}, tb_.cap_in_int, words(io.in_format)))
            return rc;
    for (int t = 0; t < n_host && io.out_format != UMX_SAMPLE_F32; ++t)
        if (int rc = grow_only<uint32_t>({{&tb_.out_int[t], 1}}, tb_.cap_out_int[t], words(io.out_format)))
            return rc;
    return UMX_OK;
}

// `count` frames of the first n_host of `src` from frame src_start on -> the set's integer outputs from frame first_frame on, which is
// their frame number in the caller's track (the k of the dither), at byte frame_bytes x first_frame; the kernel is the output
// format's (launch_encode).  acc: over the divisor of `words` (nullptr: of that record's peak words), counting what clamps into it
// (acc nullptr: the plain encode).
void umx_hip_ctx::track_encode(const TrackBufs &tb_, const umx_sample_io &io, int n_host, float *const src[4], size_t src_start, int count,
                               long long first_frame, umx_levels_acc *acc, hipStream_t st, const uint32_t *words)
{
    const float2 *s[4] = {};
    uint8_t *d[4] = {};
    for (int t = 0; t < n_host; ++t)
    {
        s[t] = reinterpret_cast<const float2 *>(src[t]) + src_start;
        d[t] = reinterpret_cast<uint8_t *>(tb_.out_int[t]) + sample_frame_bytes(io.out_format) * (size_t)first_frame;
    }
    launch_encode(io.out_format, n_host, s, d, count, first_frame, io.dither != 0, io.dither_seed, acc, st, words);
}

// What every finished span of a job goes through behind its mix, on its way out: `count` frames of the first n_host of `src` from
// frame src_start on, which are the frames from first_frame on of the caller's track.  They are measured (a job with levels), then
// encoded into the set's int16 outputs (track_encode), or -- a rescaled job, whose span is the whole track, so that the record's
// peaks are final -- encoded over the track's divisor, an fp32 output divided in place.  A job without levels or rescale: track_encode alone.
// A job with loudness: first of all, and before any divisor, the hops that these frames complete are launched -- hop b once
// frame (b + 1) hop - 1 is final.  Their warm-up reads frames of the spans before this one: those are still in `src`, at their frame
// numbers (the int16 copy goes elsewhere, a mix was written in place before its span left), so frame 0 is at src_start - first_frame.
void umx_hip_ctx::track_leave(TrackJob &j, float *const src[4], size_t src_start, int count, long long first_frame, hipStream_t st)
{
    const TrackBufs &tb_ = *j.acc;
    const umx_sample_io &io = j.opt.io;
    const int n_host = j.opt.n_host();
    const bool integer = io.out_format != UMX_SAMPLE_F32, rescale = j.opt.rescale();
    TrackMeasure &m = j.m;
    const long long end = first_frame + count;
    const float2 *s0[4] = {}; // frame 0 of the caller's track
    for (int t = 0; t < n_host; ++t)
        s0[t] = reinterpret_cast<const float2 *>(src[t]) + src_start - first_frame;
    if (j.opt.loudness)
    {
        const int hop = kweight_hop(m.rate);
        const long long final_hops = std::min<long long>(end / hop, m.hops);
        if (final_hops > m.hops_done)
        {
            launch_kweight_hops(n_host, s0, kweight_coeffs(m.rate), hop, m.hops, m.hops_done, final_hops - m.hops_done, tb_.hopE, st);
            m.hops_done = final_hops;
        }
    }
    // A job with a true peak: next, and before any divisor, the frames whose window these frames complete -- frame k once
    // frame k + 24/F is final, every frame on the job's last span (what lies behind the track reads as +0).  The window reaches back
    // into the spans before this one, which are still in `src` as above; the launch is told that the buffers end where this span does.
    if (j.opt.measures_true_peak())
    {
        const long long fin = end >= m.length ? m.length : std::max<long long>(end - true_peak_reach(true_peak_factor(m.rate)), 0);
        if (fin > m.tp_done)
        {
            launch_true_peak(n_host, s0, (int)std::min(end, m.length), m.rate, m.tp_done, fin - m.tp_done, tb_.tp, st);
            m.tp_done = fin;
        }
    }
    if (!j.opt.measures())
    {
        if (integer)
            track_encode(tb_, io, n_host, src, src_start, count, first_frame, nullptr, st);
        return;
    }
    const float2 *s[4] = {};
    float2 *sw[4] = {};
    for (int t = 0; t < n_host; ++t)
        s[t] = sw[t] = reinterpret_cast<float2 *>(src[t]) + src_start;
    // (a rescaled integer track: its encode counts what it clamps itself, with the divisor it forms)
    launch_stem_levels(n_host, s, count, first_frame, rescale ? UMX_SAMPLE_F32 : io.out_format, io.dither != 0, io.dither_seed, tb_.lev, st);
    // the words the divisor comes from: the record's peak words, or (UMX_TRUE_PEAK_RESCALE) the true-peak record, final by now
    const uint32_t *words = j.opt.true_peak_rescale() ? tb_.tp : levels_peak_words(tb_.lev);
    if (integer)
        track_encode(tb_, io, n_host, src, src_start, count, first_frame, rescale ? tb_.lev : nullptr, st, words);
    else if (rescale)
        launch_stem_rescale(n_host, sw, count, words, st);
}

// What a job measured, to the host (its last launch has finished: the caller has waited for the job's last region), as the call
// reports it -- whatever j.opt says was measured, in this order: the levels record (under UMX_TRUE_PEAK_RESCALE the gain
// is the divisor of the true-peak words), the hop energies and the loudness record formed from them, the
// true-peak words (where the record is wanted).
hipError_t umx_hip_ctx::track_report(const TrackJob &j, int n_host, TrackReport &r)
{
    const TrackOptions &opt = j.opt;
    uint32_t words[4] = {};
    hipError_t e = hipSuccess;
    if (opt.levels)
    {
        umx_levels_acc acc;
        e = hipMemcpy(&acc, j.acc->lev, sizeof acc, hipMemcpyDeviceToHost);
        if (e == hipSuccess && opt.true_peak_rescale())
            e = hipMemcpy(words, j.acc->tp, sizeof words, hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            levels_report(acc, n_host, opt.rescale(), opt.true_peak_rescale() ? words : acc.peak_bits, r.lv);
    }
    if (e == hipSuccess && opt.loudness)
    {
        r.hopE.assign((size_t)n_host * 2 * (size_t)j.m.hops, 0.0);
        if (!r.hopE.empty())
            e = hipMemcpy(r.hopE.data(), j.acc->hopE, sizeof(double) * r.hopE.size(), hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            loudness_report(r.hopE.data(), j.m.hops, kweight_hop(j.m.rate), n_host, r.ld);
    }
    if (e == hipSuccess && opt.measures_true_peak() && opt.true_peak_record)
    {
        e = hipMemcpy(words, j.acc->tp, sizeof words, hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            true_peak_report(words, n_host, true_peak_factor(j.m.rate), r.tp);
    }
    return e;
}

// The measuring side of an accumulator set for a job at the caller's `rate`, over its length_at_rate frames there (DESIGN 20, 21,
// 26), checked and grown in this order: the record of what leaves (112 bytes, once a job measures), the hop energies (n_host x 2 x
// hops doubles, grow-only, once a job measures loudness), the four true-peak words (once a job measures its true peak).  The driver
// zeroes them with the accumulators (track_measure_spans).
int umx_hip_ctx::track_measure_grow(TrackBufs &tb_, TrackJob &j, int rate, int length_at_rate)
{
    const TrackOptions &opt = j.opt;
    // (the kernels count frames in an int, with room for a workgroup's rows or a tile and its halo beyond the last)
    auto refused = [&](const char *what, bool rate_ok) {
        if (rate_ok && length_at_rate <= 0x7fffffff / 2)
            return false;
        set_error(std::string(what) + (rate_ok ? ": track too long" : ": sample rate outside 8000 .. 192000 Hz"));
        return true;
    };
    if (opt.measures() && !tb_.lev)
        if (int rc = dalloc(&tb_.lev, 1, true))
            return rc;
    if (opt.loudness)
    {
        if (refused("loudness", kweight_rate_ok(rate)))
            return UMX_ERR_ARG;
        j.m.begin(rate, length_at_rate);
        if (int rc = grow_only<double>({{&tb_.hopE, 1}}, tb_.cap_hopE, j.m.hop_doubles(opt.n_host())))
            return rc;
    }
    if (opt.measures_true_peak())
    {
        if (refused("true peak", true_peak_rate_ok(rate)))
            return UMX_ERR_ARG;
        j.m.begin(rate, length_at_rate);
        if (!tb_.tp)
            return dalloc(&tb_.tp, 4, true);
    }
    return UMX_OK;
}

// What a measuring job zeroes before its first segment, in this order: the levels record, the hop energies, the true-peak words.
// Returns how many of `spans` are filled.  tracks_once zeroes them with the accumulators, the queue on the stream of the job's first call.
int umx_hip_ctx::track_measure_spans(const TrackJob &j, ZeroSpan spans[3])
{
    int n = 0;
    if (j.opt.measures())
        spans[n++] = {j.acc->lev, sizeof(umx_levels_acc)};
    if (j.opt.loudness)
        spans[n++] = {j.acc->hopE, sizeof(double) * j.m.hop_doubles(j.opt.n_host())};
    if (j.opt.measures_true_peak())
        spans[n++] = {j.acc->tp, 4 * sizeof(unsigned)};
    return n;
}

// A job at `rate` != 44.1 kHz: n44, the length of its 44.1 kHz version, which the segments see, and the record that
// admit_job and the two edges of the segment loop need.  too_long: the caller's words for a track that does not fit.
int umx_hip_ctx::track_rate_plan(int rate, int length_at_rate, const char *too_long, TrackResample &rs, int &n44)
{
    const long long n = resampled_length(length_at_rate, rate, RS_MODEL_RATE);
    if (n < 1 || n > 0x7fffffff / 2)
    {
        set_error(n < 1 ? "track: sample rate outside 8000 .. 192000 Hz" : too_long);
        return UMX_ERR_ARG;
    }
    n44 = (int)n;
    rs.rate = rate;
    rs.length = length_at_rate;
    if (int rc = resample_plan(rate, RS_MODEL_RATE, rs.fwd, &rs.fwd_taps))
        return rc;
    return resample_plan(RS_MODEL_RATE, rate, rs.back, &rs.back_taps);
}

// The admission of a job, for both drivers (tracks_once; the queue, engine_queue.h): `j` has its geometry (track_geometry) and, at
// another rate, its j.rs (track_rate_plan); `acc` is the accumulator set it will write, `audio` its host audio of length_at_rate
// frames at `rate` -- the rate and length the caller sees --, leaves_whole: it is an ensemble lane.  The set grows by what the job
// needs, in this order (a failed allocation returns at once): accumulators, native-rate staging (a job with j.rs), int16 side, the
// measuring side (track_measure_grow: levels record, hop energies, true-peak words); then the job is filled.  When the driver zeroes
// what, and on which stream, is the driver's; what a measuring job zeroes is track_measure_spans.
int umx_hip_ctx::admit_job(TrackJob &j, TrackBufs &acc, const TrackOptions &opt, const float *audio, int rate, int length_at_rate, bool leaves_whole)
{
    j.opt = opt;
    if (int rc = track_bufs_grow(acc, (size_t)j.L2))
        return rc;
    if (j.rs.rate)
        if (int rc = grow_only<float>({{&acc.rs.in, 2}, {&acc.rs.out[0], 2}, {&acc.rs.out[1], 2}, {&acc.rs.out[2], 2}, {&acc.rs.out[3], 2}}, acc.rs.cap,
                                      (size_t)j.rs.length))
            return rc;
    if (int rc = track_int_grow(acc, opt.io, (size_t)length_at_rate, opt.n_host())) // (nothing for an fp32 call)
        return rc;
    if (int rc = track_measure_grow(acc, j, rate, length_at_rate)) // (nothing for a call that measures nothing)
        return rc;
    j.audio = audio;
    j.acc = &acc;
    // Its final regions are mixed in place and leave region by region (a resampled job's through the way back, range by range: DESIGN
    // 23) -- unless it leaves whole behind its last segment: an ensemble lane (its mean leaves: leaves_whole of tracks_once), a rescaled
    // track (its divisor needs every peak).  The last is finished by track_call itself as ONE region.
    j.by_region = !leaves_whole && !opt.rescale();
    j.whole_region = opt.rescale() && !leaves_whole;
    return UMX_OK;
}

// The track goes up segment by segment (round 6): a call needs the samples up to the end of its last segment, and the rest of a
// pageable upload (14 GB/s: 15 ms for ten minutes of stereo) runs while the device is busy with the segments before it -- the
// slots' streams do not wait for the null stream, and launches are queued ahead of the copy.
// Samples of the job's padded signal (the track behind `lead` frames of silence) below `padded_end` must be there.
// An int16 track goes into the set's staging buffer, at its frame number, and is decoded from there into the padded signal
// on `st`, the stream of the call that needs these frames.  A track at another rate goes into the set's native-rate
// staging, as far as the wanted 44.1 kHz frames read it (resample_needs), and that range of the padded signal is resampled from there
// on `st`.  Unlike the fp32 copy these kernels are not finished when this returns, and a LATER call reads the last quarter of these
// frames too (segments overlap) -- on another slot stream, which on a one-track context is not ordered behind this one before its
// STFT.  So every call's stream first waits for the set's `in_ev`, recorded behind the most recent kernel that wrote the set's `in`:
// each such kernel is then behind all earlier ones, and every reader behind every writer queued before it.  (A set's event may stem
// from its previous job: that work has long finished.)
hipError_t umx_hip_ctx::track_upload_until(TrackJob &j, long long padded_end, hipStream_t st)
{
    const bool integer = j.opt.io.in_format != UMX_SAMPLE_F32;
    TrackBufs &tb_ = *j.acc;
    if ((integer || j.rs.rate) && tb_.in_ev)
        if (hipError_t e = hipStreamWaitEvent(st, tb_.in_ev, 0))
            return e;
    // what is wanted of the track as the segments see it, and what that needs of the host's frames
    long long want = std::min<long long>(j.length, padded_end - j.lead), host_want = want;
    if (j.rs.rate)
    {
        if (want < j.length) // (a range starts at an even frame: resample.h)
            want += want & 1;
        if (want <= j.done44)
            return hipSuccess;
        host_want = resample_needs(want, j.rs.rate, RS_MODEL_RATE, j.rs.length);
    }
    hipError_t e = hipSuccess;
    if (host_want > j.uploaded)
    {
        const size_t from = (size_t)j.uploaded, count = (size_t)(host_want - j.uploaded);
        float *const dst = j.rs.rate ? tb_.rs.in + 2 * from : tb_.in + 2 * ((size_t)j.lead + from); // where host frame `from` goes as fp32
        if (integer)
        {
            // (the staging holds the host's bytes at their own offsets: 4 or 6 x frame)
            const size_t fb = sample_frame_bytes(j.opt.io.in_format);
            uint8_t *const stage = reinterpret_cast<uint8_t *>(tb_.in_int) + fb * from;
            e = hipMemcpy(stage, reinterpret_cast<const uint8_t *>(j.audio) + fb * from, fb * count, hipMemcpyHostToDevice);
            if (e == hipSuccess && !tb_.in_ev)
                e = hipEventCreateWithFlags(&tb_.in_ev, hipEventDisableTiming);
            if (e == hipSuccess)
            {
                launch_decode(j.opt.io.in_format, stage, reinterpret_cast<float2 *>(dst), (int)count, st);
                e = hipEventRecord(tb_.in_ev, st);
            }
        }
        else
            e = hipMemcpy(dst, j.audio + 2 * from, sizeof(float) * 2 * count, hipMemcpyHostToDevice);
        j.uploaded = host_want;
    }
    if (j.rs.rate && e == hipSuccess) // (want > done44)
    {
        const float *src = tb_.rs.in;
        float *out = tb_.in + 2 * (size_t)j.lead;
        if (!tb_.in_ev)
            e = hipEventCreateWithFlags(&tb_.in_ev, hipEventDisableTiming);
        if (e == hipSuccess)
            e = launch_resample(j.rs.fwd, j.rs.fwd_taps, 1, &src, j.rs.length, &out, j.length, (int)j.done44, (int)(want - j.done44), st);
        if (e == hipSuccess)
            e = hipEventRecord(tb_.in_ev, st);
        ++rs_launches[0];
        j.done44 = want;
    }
    return e;
}

// the mix of `count` frames from padded frame `stem_start` on, written over the first n_out of the four stem buffers there
// (the track's accumulators, or an ensemble's means from frame 0 on); column 4 is `in` (the track's padded input) from in_start on
void umx_hip_ctx::track_mix(const MixSpec &mix, float *const stems[4], size_t stem_start, const float *in, size_t in_start, int count, hipStream_t st)
{
    const float2 *src[MIX_COLUMNS];
    float2 *dst[UMX_MAX_MIX_OUTPUTS];
    for (int t = 0; t < 4; ++t)
    {
        src[t] = reinterpret_cast<const float2 *>(stems[t]) + stem_start;
        dst[t] = reinterpret_cast<float2 *>(stems[t]) + stem_start;
    }
    src[MIX_MIXTURE] = reinterpret_cast<const float2 *>(in) + in_start;
    launch_stem_mix(mix, src, dst, count, st);
}

// umx.cpp:136-147: a finished region without the shift, to its job's n_host host buffers, once it is ready.  A resampled job's region
// is the range of frames at the caller's rate that left with it, in the set's staging at their frame numbers.
hipError_t umx_hip_ctx::track_region_download(const TrackRegion &r, float *const *out_host)
{
    const TrackJob &j = *r.job;
    const int n_host = j.opt.n_host();
    const long long lo = std::max<long long>(r.start, j.lead), hi = std::min<long long>((long long)r.start + r.count, (long long)j.lead + j.length);
    const size_t first = j.rs.rate ? (size_t)r.rs_first : (size_t)(lo - j.lead); // in the caller's track
    const long long n = j.rs.rate ? r.rs_count : hi - lo;
    if (n <= 0)
        return hipSuccess;
    hipError_t cerr = hipEventSynchronize(r.ready);
    const size_t count = (size_t)n;
    for (int t = 0; t < n_host && cerr == hipSuccess; ++t)
        if (j.opt.io.out_format != UMX_SAMPLE_F32) // (encoded behind the region's normalisation and mix, at its frame number: track_call)
        {
            const size_t fb = sample_frame_bytes(j.opt.io.out_format); // 4 or 6 x frame on both sides
            cerr = hipMemcpy(reinterpret_cast<uint8_t *>(out_host[t]) + fb * first, reinterpret_cast<const uint8_t *>(j.acc->out_int[t]) + fb * first,
                             fb * count, hipMemcpyDeviceToHost);
        }
        else if (j.rs.rate)
            cerr = hipMemcpy(out_host[t] + 2 * first, j.acc->rs.out[t] + 2 * first, sizeof(float) * 2 * count, hipMemcpyDeviceToHost);
        else
            cerr = hipMemcpy(out_host[t] + 2 * first, j.acc->out[t] + 2 * (size_t)lo, sizeof(float) * 2 * count, hipMemcpyDeviceToHost);
    return cerr;
}

// One call of infer_batch for the whole-track drivers: lane ln runs the segment of lanes[ln].job that starts at padded frame
// lanes[ln].start.  Which job sits in which lane is the caller's: a track per lane (tracks_once), segment k of the one track in
// lane k (its reset mode), whatever job the lane holds (the queue).  The segment's stems are the lane's (trk[ln].seg of the slot), the
// accumulators the job's.  Whatever the caller zeroes for this call it has queued on slot[next_slot()].stream, which is the stream
// of this call: next_slot() moves on with infer_batch.  last_slot: the slot of the previous call of the run (-1: none), then this one.
int umx_hip_ctx::track_call(const TrackLane *lanes, int nl, unsigned flags, int &last_slot, TrackRegions &regions)
{
    const int si = next_slot(), stride = track_stride();
    const hipStream_t st = slot[si].stream;
    if (!trk_acc_ev[0])
        for (int s = 0; s < nslots; ++s)
            UMX_HIP_CHECK(hipEventCreateWithFlags(&trk_acc_ev[s], hipEventDisableTiming));
    const float *ain[LSTMB_MAX_TRACKS] = {};
    int nn[LSTMB_MAX_TRACKS] = {};
    float *outs[4 * LSTMB_MAX_TRACKS] = {};
    for (int ln = 0; ln < nl; ++ln)
    {
        TrackJob *j = lanes[ln].job;
        if (!j)
            continue;
        if (!trk[ln].seg[0][0]) // the lane's per-slot segment stems, on first use
            for (int s = 0; s < nslots; ++s)
                for (int t = 0; t < 4; ++t)
                    if (int rc = dalloc(&trk[ln].seg[s][t], (size_t)2 * N, false))
                        return rc;
        if (track_upload_until(*j, lanes[ln].start + N, st) != hipSuccess)
        {
            set_error("track: upload failed");
            return UMX_ERR_HIP;
        }
        ain[ln] = j->acc->in + 2 * (size_t)lanes[ln].start;
        nn[ln] = (int)std::min<long long>(N, j->L2 - lanes[ln].start);
        for (int t = 0; t < 4; ++t)
            outs[4 * ln + t] = trk[ln].seg[si][t];
    }
    if (int rc = infer_batch(nl, ain, nn, outs, flags))
        return rc;
    if (last_slot >= 0) // accumulate in segment order (two segments overlap by a quarter)
        (void)hipStreamWaitEvent(st, trk_acc_ev[last_slot], 0);
    for (int ln = 0; ln < nl; ++ln)
    {
        TrackJob *j = lanes[ln].job;
        if (!j)
            continue;
        // The segment's stems (nn frames at padded frame `start`) are blended into the job's accumulators.  A sample is final once
        // the segment that starts at or before it and the one before that have been blended in: region [start_i, start_{i+1}) right
        // after segment i.  It is normalised there and then (and mixed over its stems, before `ready`), and the host downloads it
        // while the GPU is already busy with the following segments.
        const TrackBufs &tb_ = *j->acc;
        Stems4 tk, seg;
        for (int t = 0; t < 4; ++t)
        {
            tk.p[t] = reinterpret_cast<float2 *>(tb_.out[t]);
            seg.p[t] = reinterpret_cast<float2 *>(trk[ln].seg[si][t]);
        }
        TrackRegion rg = {j, (int)lanes[ln].start, 0, nullptr};
        rg.count = (int)std::min<long long>((long long)rg.start + stride, j->L2) - rg.start;
        hipLaunchKernelGGL(track_accumulate_kernel, dim3((nn[ln] + 255) / 256, 4), dim3(256), 0, st, tk, tb_.sumw, seg, rg.start, nn[ln], N);
        hipLaunchKernelGGL(track_normalise_kernel, dim3((rg.count + 255) / 256, 4), dim3(256), 0, st, tk, tb_.sumw, rg.start, rg.count);
        if (!j->by_region)
        {
            // a rescaled track is ONE region, behind its last segment's overlap-add (its divisor needs every peak)
            if (!j->whole_region || (long long)rg.start + stride < j->L2)
                continue;
            rg.start = j->lead;
            rg.count = j->length;
        }
        const TrackOptions &opt = j->opt;
        if (opt.mix)
            track_mix(*opt.mix, tb_.out, (size_t)rg.start, tb_.in, (size_t)rg.start, rg.count, st);
        if (j->rs.rate)
        {
            // DESIGN 23, the way back: the frames at the caller's rate whose whole window lies in what is final now (resample_ready; an even
            // count, or all) are resampled from the accumulators into the set's staging and leave from there, at the caller's frame
            // numbers; the range may be empty, the region stays one.  This stream is behind every earlier call's (trk_acc_ev), so the
            // accumulators below the region and the staging's earlier frames (a loudness warm-up reads them) are there.
            const long long fin = std::min<long long>(std::max<long long>((long long)rg.start + rg.count - j->lead, 0), j->length);
            long long r = resample_ready(fin, RS_MODEL_RATE, j->rs.rate, j->length, j->rs.length);
            if (r < j->rs.length)
                r &= ~1LL;
            rg.rs_first = (int)j->out_done;
            rg.rs_count = (int)std::max<long long>(r - j->out_done, 0);
            if (rg.rs_count > 0)
            {
                const float *src[4] = {};
                for (int t = 0; t < opt.n_host(); ++t)
                    src[t] = tb_.out[t] + 2 * (size_t)j->lead;
                if (launch_resample(j->rs.back, j->rs.back_taps, opt.n_host(), src, j->length, tb_.rs.out, j->rs.length, rg.rs_first, rg.rs_count, st) != hipSuccess)
                {
                    set_error("track: resampling a region failed");
                    return UMX_ERR_HIP;
                }
                ++rs_launches[1];
                track_leave(*j, tb_.rs.out, (size_t)rg.rs_first, rg.rs_count, rg.rs_first, st);
                j->out_done = r;
            }
        }
        else if (opt.leaves_measured()) // the region's frames of the caller's track, as they will leave (an int16 copy
        {                               // is not written over the accumulators: the next segment's overlap-add still reads its neighbours)
            const long long lo = std::max<long long>(rg.start, j->lead), hi = std::min<long long>((long long)rg.start + rg.count, (long long)j->lead + j->length);
            if (hi > lo)
                track_leave(*j, tb_.out, (size_t)lo, (int)(hi - lo), lo - j->lead, st);
        }
        if (hipEventCreateWithFlags(&rg.ready, hipEventDisableTiming) != hipSuccess)
        {
            set_error("track: event creation failed");
            return UMX_ERR_HIP;
        }
        regions.v.push_back(rg); // (the list owns the event from here on)
        if (hipEventRecord(rg.ready, st) != hipSuccess)
        {
            set_error("track: event creation failed");
            return UMX_ERR_HIP;
        }
    }
    (void)hipEventRecord(trk_acc_ev[si], st);
    last_slot = si;
    return UMX_OK;
}

int umx_hip_ctx::tracks_once(const TrackRequest &rq)
{
    // ensemble: the caller (umx_hip_shift_ensemble) has repeated the one track's audio pointer, length and rate per lane
    // and checked the offsets; rq.out holds that track's buffers
    // mix: a checked matrix; a track has n_host = mix->n_out host buffers instead of four
    const TrackOptions &opt = rq.opt;
    const int nt = rq.n_tracks, n_host = opt.n_host();
    const int *const length_in = rq.length;
    const bool ensemble = rq.ensemble;
    const MixSpec *const mix = opt.mix;
    if (nt < 1 || nt > B || !rq.audio || !length_in || !rq.shift_offset)
    {
        set_error("tracks: need 1 <= n_tracks <= the context's track count and non-null argument arrays");
        return UMX_ERR_ARG;
    }
    if (int rc = check_flags(rq.flags))
        return rc;
    const std::pair<bool, const char *> not_in_ensemble[] = {// DESIGN 20, 21, 26
                                                             {opt.measures(), "track: the shift ensemble does not offer levels or rescale"},
                                                             {opt.loudness, "track: the shift ensemble does not offer loudness"},
                                                             {opt.measures_true_peak(), "track: the shift ensemble does not offer the true peak"}};
    for (const auto &asked : not_in_ensemble)
        if (asked.first && ensemble)
        {
            set_error(asked.second);
            return UMX_ERR_ARG;
        }
    for (int ln = 0; ln < nt; ++ln)
        if (!track_job_ok(rq.audio[ln], length_in[ln], rq.shift_offset[ln], rq.out && !ensemble ? rq.out + n_host * ln : rq.out, n_host))
        {
            set_error("track: need audio, outputs, length >= 1 and shift offset < 22050");
            return UMX_ERR_ARG;
        }
    // A track at another rate runs as the n44 = ceil(length L / M) frames of its 44.1 kHz version: `length` below is
    // that length, length_in the caller's.
    int length[LSTMB_MAX_TRACKS];
    TrackResample rs[LSTMB_MAX_TRACKS];
    for (int ln = 0; ln < nt; ++ln)
    {
        length[ln] = length_in[ln];
        if (rq.rate && rq.rate[ln] != RS_MODEL_RATE)
            if (int rc = track_rate_plan(rq.rate[ln], length_in[ln], "track: too long", rs[ln], length[ln]))
                return rc;
    }
    if (ph_next != -1)
    {
        set_error("track: a phased segment is open (umx_hip_segment_end first)");
        return UMX_ERR_ARG;
    }
    // Reset mode (UMX_FLAG_RESET_SEGMENTS, SURVEY 8(e)'s mode table): every segment starts from a ZERO lstm_data instead of the one
    // the previous segment left behind (umx.cpp:167-171 makes it once per track, :226-227 hands it to every call) -- a declared
    // deviation, opt-in.  The segments of a track are then independent, and up to B of them ride as the track lanes of ONE call.
    const bool reset_lanes = (rq.flags & UMX_FLAG_RESET_SEGMENTS) != 0;
    const unsigned flags = rq.flags & ~(unsigned)UMX_FLAG_RESET_SEGMENTS;
    if (reset_lanes && (nt != 1 || !lstm_batched || B < 2 || ensemble))
    {
        set_error("track: UMX_FLAG_RESET_SEGMENTS takes ONE track on a context made by umx_hip_create_tracks with at least 2 lanes");
        return UMX_ERR_ARG;
    }
    UMX_HIP_CHECK(hipSetDevice(device));
    if (int rc = sync_all())
        return rc;
    const int stride = track_stride();
    TrackJob job[LSTMB_MAX_TRACKS]; // lane ln's track
    int L2max = 0, max_segs = 0;
    for (int ln = 0; ln < nt; ++ln)
    {
        TrackJob &j = job[ln];
        if (!track_geometry(length[ln], rq.shift_offset[ln], stride, j))
        {
            set_error("track: too long");
            return UMX_ERR_ARG;
        }
        L2max = std::max(L2max, j.L2);
        max_segs = std::max(max_segs, j.segs);
        if (!ensemble || ln == 0) // (an ensemble's one track is staged and resampled once, by lane 0; the other lanes get its 44.1 kHz frames)
            j.rs = rs[ln];
    }
    rs_launches[0] = rs_launches[1] = 0;
    // lanes whose per-segment stem buffers are needed: one per track, or (reset mode) one per segment of a call
    const int seg_lanes = reset_lanes ? std::min(B, max_segs) : nt;
    if (trk.size() < (size_t)seg_lanes)
        trk.resize(seg_lanes);
    for (int ln = 0; ln < nt; ++ln)
        if (int rc = admit_job(job[ln], trk[ln], opt, rq.audio[ln], rq.rate ? rq.rate[ln] : RS_MODEL_RATE, length_in[ln], ensemble))
            return rc;
    if (ensemble) // the mean of the lanes' stems: n44 frames
        if (int rc = grow_only<float>({{&ens_out[0], 2}, {&ens_out[1], 2}, {&ens_out[2], 2}, {&ens_out[3], 2}}, ens_cap, (size_t)length[0]))
            return rc;
    // umx.cpp:167-171: a fresh, zeroed lstm_data per track; umx.cpp:186-195: zeroed accumulators (and F4)
    UMX_HIP_CHECK(hipMemset(state, 0, sizeof(float) * state_floats() * (reset_lanes ? B : nt)));
    clear_used();
    for (int ln = 0; ln < nt; ++ln) // (reset mode: nt = 1)
    {
        const TrackBufs &tb_ = trk[ln];
        const size_t frames = (size_t)job[ln].L2;
        UMX_HIP_CHECK(hipMemset(tb_.in, 0, sizeof(float) * 2 * frames));
        for (int t = 0; t < 4; ++t)
            UMX_HIP_CHECK(hipMemset(tb_.out[t], 0, sizeof(float) * 2 * frames));
        UMX_HIP_CHECK(hipMemset(tb_.sumw, 0, sizeof(float) * frames));
        ZeroSpan spans[3];
        for (int k = 0, n = track_measure_spans(job[ln], spans); k < n; ++k)
            UMX_HIP_CHECK(hipMemset(spans[k].p, 0, spans[k].bytes));
    }
    // A resampled track goes up and through the resampler range by range, with the call that needs the frames (track_upload_until) --
    // but an ensemble's: whole, now, in one launch, on the null stream.
    if (ensemble && job[0].rs.rate)
        if (track_upload_until(job[0], job[0].L2, nullptr) != hipSuccess)
        {
            set_error("track: upload failed");
            return UMX_ERR_HIP;
        }
    // an ensemble's track crosses PCIe once, whole, into lane 0 (unless the resampler has just written it there); the other lanes
    // get it from lane 0, device to device, behind their own shift's zeros (the memsets above)
    if (ensemble)
    {
        float *first = trk[0].in + 2 * (size_t)job[0].lead;
        const size_t bytes = sizeof(float) * 2 * (size_t)length[0];
        if (!job[0].rs.rate)
            UMX_HIP_CHECK(hipMemcpy(first, rq.audio[0], bytes, hipMemcpyHostToDevice));
        for (int ln = 1; ln < nt; ++ln)
            UMX_HIP_CHECK(hipMemcpy(trk[ln].in + 2 * (size_t)job[ln].lead, first, bytes, hipMemcpyDeviceToDevice));
    }
    UMX_HIP_CHECK(hipDeviceSynchronize());
    for (int ln = 0; ln < nt && ensemble; ++ln) // (on the device whole already)
        if (!job[ln].rs.rate)
            job[ln].uploaded = length[ln];

    const float total_reps = std::ceil((float)L2max / (float)stride); // umx.cpp:208 (of the longest track)
    float done = 0.f;
    TrackRegions regions;
    int last_slot = -1;
    const int per_call = reset_lanes ? seg_lanes : 1; // segments of a track per call
    const int nl = reset_lanes ? per_call : nt;        // lanes of a call: lane = track (its segment at `off`), or lane k = segment k of the call
    for (long long off = 0; off < L2max; off += (long long)stride * per_call)
    {
        TrackLane lanes[LSTMB_MAX_TRACKS];
        int queued = 0; // segments of the longest track in this call
        for (int ln = 0; ln < nl; ++ln)
        {
            TrackJob &j = job[reset_lanes ? 0 : ln];
            const long long so = reset_lanes ? off + (long long)ln * stride : off;
            if (so >= j.L2) // this track has no segment here any more (umx.cpp:214-217)
                continue;
            lanes[ln].job = &j;
            lanes[ln].start = so;
            queued = reset_lanes ? queued + 1 : 1;
        }
        if (reset_lanes && off > 0) // every segment from a zero state: the previous call has left its own behind
        {
            // (the samples of this call go up first, while the device is still busy with the previous one)
            if (track_upload_until(job[0], off + (long long)stride * (per_call - 1) + N, slot[next_slot()].stream) != hipSuccess)
            {
                set_error("track: upload failed");
                return UMX_ERR_HIP;
            }
            if (int rc = sync_all())
                return rc;
            UMX_HIP_CHECK(hipMemset(state, 0, sizeof(float) * state_floats() * B));
            UMX_HIP_CHECK(hipDeviceSynchronize());
        }
        if (int rc = track_call(lanes, nl, flags, last_slot, regions))
            return rc;
        // umx.cpp:229, once per QUEUED segment (queued, not finished: the device runs behind the host here) of the longest track: one
        // per call, or (reset mode) one per lane of the call
        for (int q = 0; q < queued; ++q)
        {
            done += 1.0f / total_reps;
            if (rq.progress)
                rq.progress(done, rq.progress_user);
        }
    }
    // What leaves whole, behind the last segment's overlap-add -- an ensemble's mean: its four buffers from frame `start` on are mixed
    // at 44.1 kHz (column 4: lane 0's padded input), a resampled track's n_host buffers go back to the caller's rate in one launch
    // into lane 0's staging, and `whole` notes where the host finds them.
    hipError_t cerr = hipSuccess;
    const hipStream_t last_st = slot[last_slot].stream;
    float *whole[LSTMB_MAX_TRACKS][4] = {};
    bool any_whole = false;
    auto leaves_whole = [&](int ln, float *const stems[4], size_t start) {
        TrackJob &j = job[ln];
        if (mix)
            track_mix(*mix, stems, start, j.acc->in, (size_t)j.lead, j.length, last_st);
        const float *src[4];
        for (int t = 0; t < 4; ++t)
            src[t] = whole[ln][t] = stems[t] + 2 * start;
        if (j.rs.rate)
        {
            cerr = launch_resample(j.rs.back, j.rs.back_taps, n_host, src, j.length, j.acc->rs.out, length_in[ln], 0, length_in[ln], last_st);
            ++rs_launches[1];
            std::copy(j.acc->rs.out, j.acc->rs.out + 4, whole[ln]);
        }
        if (cerr == hipSuccess) // at the caller's rate and length, frame 0 first: measured, encoded, rescaled as the job says
        {
            track_leave(j, whole[ln], 0, length_in[ln], 0, last_st);
            for (int t = 0; t < n_host && opt.io.out_format != UMX_SAMPLE_F32; ++t)
                whole[ln][t] = reinterpret_cast<float *>(j.acc->out_int[t]);
        }
        any_whole = true;
    };
    if (ensemble)
    {
        // Every lane's last overlap-add is ordered before this stream's (trk_acc_ev chains the calls).  The mean of the lanes' `length`
        // frames from their shifts on goes to ens_out, from frame 0 on; it leaves as a single track's stems would (column 4 of its
        // mix: lane 0's copy of the track).
        ShiftMeanLanes mean_of = {};
        Stems4 mean;
        for (int t = 0; t < 4; ++t)
        {
            for (int ln = 0; ln < nt; ++ln)
                mean_of.src[ln][t] = reinterpret_cast<const float2 *>(trk[ln].out[t]) + job[ln].lead;
            mean.p[t] = reinterpret_cast<float2 *>(ens_out[t]);
        }
        for (hipEvent_t &e : ens_ev)
            if (!e)
                UMX_HIP_CHECK(hipEventCreate(&e));
        (void)hipEventRecord(ens_ev[0], last_st);
        launch_shift_mean(mean_of, nt, mean, length[0], last_st);
        (void)hipEventRecord(ens_ev[1], last_st);
        ens_timed = true;
        leaves_whole(0, ens_out, 0);
    }
    for (const TrackRegion &rg : regions.v) // umx.cpp:136-147: drop the shift
        if (cerr == hipSuccess)
            cerr = track_region_download(rg, rq.out + n_host * (rg.job - job));
    if (any_whole && cerr == hipSuccess)
        cerr = hipStreamSynchronize(last_st);
    for (int ln = 0; ln < nt; ++ln)
        for (int t = 0; t < n_host && whole[ln][0] && cerr == hipSuccess; ++t) // (an ensemble's one result: lane 0)
            cerr = hipMemcpy(rq.out[n_host * ln + t], whole[ln][t], sample_frame_bytes(opt.io.out_format) * (size_t)length_in[ln],
                             hipMemcpyDeviceToHost);
    // what every job measured, once: its last measuring launch is behind its last region, which the host has
    std::vector<TrackReport> reports(nt);
    for (int ln = 0; ln < nt && cerr == hipSuccess; ++ln)
        cerr = track_report(job[ln], n_host, reports[ln]);
    if (cerr != hipSuccess)
    {
        set_error(hipGetErrorString(cerr));
        return UMX_ERR_HIP;
    }
    UMX_HIP_CHECK(hipGetLastError());
    if (int rc = umx_hip_sync(this)) // surfaces a persistent-kernel timeout
        return rc;
    for (int ln = 0; ln < nt; ++ln) // (only what a run without a timeout measured is handed out)
    {
        const TrackReport &r = reports[ln];
        if (rq.levels)
            rq.levels[ln] = r.lv;
        if (rq.loudness)
            rq.loudness[ln] = r.ld;
        if (rq.hop_energy && rq.hop_energy[ln])
            std::copy(r.hopE.begin(), r.hopE.end(), rq.hop_energy[ln]);
        if (rq.true_peak && opt.measures_true_peak())
            rq.true_peak[ln] = r.tp;
    }
    return UMX_OK;
}

// the tap table of a rate pair, built on the host in double and kept in HBM for the context's lifetime
int umx_hip_ctx::resample_plan(int rate_in, int rate_out, ResampleGeom &g, const float **taps_dev)
{
    if (!resample_geom(rate_in, rate_out, g))
    {
        set_error("resample: sample rates must be 8000 .. 192000 Hz");
        return UMX_ERR_ARG;
    }
    auto it = rs_taps.find({rate_in, rate_out});
    if (it == rs_taps.end())
    {
        UMX_HIP_CHECK(hipSetDevice(device));
        std::vector<float> taps;
        resample_taps(g, taps);
        float *d = nullptr;
        if (int rc = upload(&d, taps))
            return rc;
        it = rs_taps.emplace(std::make_pair(rate_in, rate_out), d).first;
    }
    *taps_dev = it->second;
    return UMX_OK;
}
