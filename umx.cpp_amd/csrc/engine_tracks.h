// engine_tracks.h -- part of engine.hip (one translation unit: the kernels inline into their launchers): whole tracks on the device: split_inference / shift_inference for one track or one per lane.
// Included by engine.hip behind the definition of umx_hip_ctx; not a stand-alone header.
// ---------------------------------------------------------------- whole track
// shift_inference (umx.cpp:99-150) around split_inference (umx.cpp:152-295) with the track resident in HBM:
// one upload, the segments queued back to back through the two pipeline slots (so consecutive segments
// overlap exactly as in bench.py), the weighted overlap-add and the final normalisation on the device, one
// download.  shift_offset < 0: no shift buffer (plain split_inference).
int umx_hip_ctx::track(const float *audio_host, int length, int shift_offset, float *const out_host[4], unsigned flags,
                       void (*progress)(float, void *), void *progress_user)
{
    if (!out_host)
    {
        set_error("track: need audio, outputs, length >= 1 and shift offset < 22050");
        return UMX_ERR_ARG;
    }
    return tracks(1, &audio_host, &length, &shift_offset, out_host, flags, progress, progress_user);
}

// shift_inference (umx.cpp:99-150) around split_inference (umx.cpp:152-295) for `nt` tracks at once, one per track
// lane: the tracks stay in HBM, call s runs segment s of every track that still has one (a finished track's lane sits
// idle), the weighted overlap-add and the normalisation run per lane on the device, finished regions are downloaded
// while later segments run.  nt == 1 is umx_hip_split_inference / umx_hip_shift_inference.
int umx_hip_ctx::tracks(int nt, const float *const *audio_host, const int *length, const int *shift_offset, float *const *out_host,
                        unsigned flags, void (*progress)(float, void *), void *progress_user, const int *rate, bool ensemble,
                        const MixSpec *mix)
{
    // A persistent-kernel timeout inside a track cannot be repaired segment by segment (the overlap-add has consumed
    // the stems): everything is run again, once, with the per-step driver the timeout switches the context to.
    no_recovery = true;
    int rc = tracks_once(nt, audio_host, length, shift_offset, out_host, flags, progress, progress_user, rate, ensemble, mix);
    if (rc == UMX_ERR_TIMEOUT) // (a resampled track is resampled again from its host copy, an ensemble placed in its lanes and averaged
                               // again, a mix formed again from fresh accumulators: tracks_once starts from scratch)
        rc = tracks_once(nt, audio_host, length, shift_offset, out_host, flags, progress, progress_user, rate, ensemble, mix);
    no_recovery = false;
    pending.clear();
    pending_lost = false;
    return rc;
}

// ---------------------------------------------------------------- what the whole-track drivers share (tracks_once, engine_queue.h)
// grow-only accumulators of one track: the (shifted) track, 4 stems, the weight sum, `frames` frames each
int umx_hip_ctx::track_bufs_grow(TrackBufs &tb_, size_t frames)
{
    if (frames <= tb_.cap)
        return UMX_OK;
    const size_t cap = frames + frames / 8;
    for (float **p : {&tb_.in, &tb_.out[0], &tb_.out[1], &tb_.out[2], &tb_.out[3], &tb_.sumw})
        if (*p)
        {
            allocs.erase(std::find(allocs.begin(), allocs.end(), (void *)*p));
            (void)hipFree(*p);
            *p = nullptr;
        }
    tb_.cap = 0;
    if (int rc = dalloc(&tb_.in, 2 * cap, false))
        return rc;
    for (int t = 0; t < 4; ++t)
        if (int rc = dalloc(&tb_.out[t], 2 * cap, false))
            return rc;
    if (int rc = dalloc(&tb_.sumw, cap, false))
        return rc;
    tb_.cap = cap;
    return UMX_OK;
}

// the per-slot segment stems of a track lane
int umx_hip_ctx::track_bufs_segs(TrackBufs &tb_)
{
    if (!tb_.seg[0][0])
        for (int s = 0; s < nslots; ++s)
            for (int t = 0; t < 4; ++t)
                if (int rc = dalloc(&tb_.seg[s][t], (size_t)2 * N, false))
                    return rc;
    return UMX_OK;
}

// The track goes up segment by segment (round 6): a call needs the samples up to the end of its last segment, and the rest of a
// pageable upload (14 GB/s: 15 ms for ten minutes of stereo) runs while the device is busy with the segments before it -- the
// slots' streams do not wait for the null stream, and launches are queued ahead of the copy.
// Samples of the padded signal `in_dev` (the track behind `lead` frames of silence) below `padded_end` must be there; `uploaded`:
// host samples of the track already on the device.
hipError_t umx_hip_ctx::track_upload_until(float *in_dev, const float *audio_host, int length, int lead, long long &uploaded, long long padded_end)
{
    const long long want = std::min<long long>(length, padded_end - lead);
    if (want <= uploaded)
        return hipSuccess;
    const hipError_t e = hipMemcpy(in_dev + 2 * ((size_t)lead + (size_t)uploaded), audio_host + 2 * (size_t)uploaded,
                                   sizeof(float) * 2 * (size_t)(want - uploaded), hipMemcpyHostToDevice);
    uploaded = want;
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

// A segment's stems `seg` (nn frames at padded frame `offset` of a track of L2 padded frames) blended into the track's accumulators.
// A sample is final once the segment that starts at or before it and the one before that have been blended in: region
// [offset, offset + stride) right after this segment.  It is normalised there and then and, with `mix`, mixed (over its stems).
// Returns the region's frame count.
int umx_hip_ctx::track_region(const TrackBufs &tb_, float *const seg_stems[4], int offset, int nn, int L2, int stride, const MixSpec *mix, hipStream_t st)
{
    Stems4 tk, seg;
    for (int t = 0; t < 4; ++t)
    {
        tk.p[t] = reinterpret_cast<float2 *>(tb_.out[t]);
        seg.p[t] = reinterpret_cast<float2 *>(seg_stems[t]);
    }
    hipLaunchKernelGGL(track_accumulate_kernel, dim3((nn + 255) / 256, 4), dim3(256), 0, st, tk, tb_.sumw, seg, offset, nn, N);
    const int count = (int)std::min<long long>((long long)offset + stride, L2) - offset;
    hipLaunchKernelGGL(track_normalise_kernel, dim3((count + 255) / 256, 4), dim3(256), 0, st, tk, tb_.sumw, offset, count);
    if (mix)
        track_mix(*mix, tb_.out, (size_t)offset, tb_.in, (size_t)offset, count, st);
    return count;
}

// umx.cpp:136-147: a finished region without the shift, to the track's n_host host buffers, once `ready` has passed
hipError_t umx_hip_ctx::track_region_download(const TrackBufs &tb_, int start, int count, int lead, int length, int n_host, float *const *out_host,
                                              hipEvent_t ready)
{
    const long long lo = std::max<long long>(start, lead), hi = std::min<long long>((long long)start + count, (long long)lead + length);
    if (hi <= lo)
        return hipSuccess;
    hipError_t cerr = hipEventSynchronize(ready);
    for (int t = 0; t < n_host && cerr == hipSuccess; ++t)
        cerr = hipMemcpy(out_host[t] + 2 * (size_t)(lo - lead), tb_.out[t] + 2 * (size_t)lo, sizeof(float) * 2 * (size_t)(hi - lo), hipMemcpyDeviceToHost);
    return cerr;
}

int umx_hip_ctx::tracks_once(int nt, const float *const *audio_host, const int *length_in, const int *shift_offset, float *const *out_host,
                             unsigned flags, void (*progress)(float, void *), void *progress_user, const int *rate, bool ensemble,
                             const MixSpec *mix)
{
    // ensemble: the caller (umx_hip_shift_ensemble) has repeated the one track's audio pointer, length and rate per lane
    // and checked the offsets; out_host holds that track's 4 stems
    // mix: a checked matrix; a track has n_host = mix->n_out host buffers instead of four, out_host[n_host * lane + m]
    const int n_host = mix ? mix->n_out : 4;
    if (nt < 1 || nt > B || !audio_host || !length_in || !shift_offset || !out_host)
    {
        set_error("tracks: need 1 <= n_tracks <= the context's track count and non-null argument arrays");
        return UMX_ERR_ARG;
    }
    if (int rc = check_flags(flags))
        return rc;
    for (int ln = 0; ln < nt; ++ln)
    {
        bool ok = audio_host[ln] && length_in[ln] >= 1 && shift_offset[ln] < UMX_MAX_SHIFT;
        for (int m = 0; m < n_host; ++m)
            ok = ok && out_host[(ensemble ? 0 : n_host * ln) + m];
        if (!ok)
        {
            set_error("track: need audio, outputs, length >= 1 and shift offset < 22050");
            return UMX_ERR_ARG;
        }
    }
    // A track at another rate runs as the n44 = ceil(length L / M) frames of its 44.1 kHz version: `length` below is
    // that length, length_in the caller's.
    int length[LSTMB_MAX_TRACKS];
    bool resampled[LSTMB_MAX_TRACKS] = {};
    ResampleGeom rs_fwd[LSTMB_MAX_TRACKS], rs_back[LSTMB_MAX_TRACKS];
    const float *rs_fwd_taps[LSTMB_MAX_TRACKS] = {}, *rs_back_taps[LSTMB_MAX_TRACKS] = {};
    for (int ln = 0; ln < nt; ++ln)
    {
        length[ln] = length_in[ln];
        if (!rate || rate[ln] == RS_MODEL_RATE)
            continue;
        const long long n44 = resampled_length(length_in[ln], rate[ln], RS_MODEL_RATE);
        if (n44 < 1 || n44 > 0x7fffffff / 2)
        {
            set_error(n44 < 1 ? "track: sample rate outside 8000 .. 192000 Hz" : "track: too long");
            return UMX_ERR_ARG;
        }
        length[ln] = (int)n44;
        resampled[ln] = true;
        if (int rc = resample_plan(rate[ln], RS_MODEL_RATE, rs_fwd[ln], &rs_fwd_taps[ln]))
            return rc;
        if (int rc = resample_plan(RS_MODEL_RATE, rate[ln], rs_back[ln], &rs_back_taps[ln]))
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
    const bool reset_lanes = (flags & UMX_FLAG_RESET_SEGMENTS) != 0;
    flags &= ~(unsigned)UMX_FLAG_RESET_SEGMENTS;
    if (reset_lanes && (nt != 1 || !lstm_batched || B < 2 || ensemble))
    {
        set_error("track: UMX_FLAG_RESET_SEGMENTS takes ONE track on a context made by umx_hip_create_tracks with at least 2 lanes");
        return UMX_ERR_ARG;
    }
    UMX_HIP_CHECK(hipSetDevice(device));
    if (int rc = sync_all())
        return rc;
    int lead[LSTMB_MAX_TRACKS], L2[LSTMB_MAX_TRACKS], L2max = 0;
    for (int ln = 0; ln < nt; ++ln)
    {
        lead[ln] = shift_offset[ln] < 0 ? 0 : shift_offset[ln];
        // umx.cpp:120-122: length + max_shift - offset -- which the reference overruns for offset > max_shift / 2 (its
        // block write is [offset, offset + length)); the same size where the reference is defined, large enough elsewhere
        const long long l2 = shift_offset[ln] < 0 ? (long long)length[ln]
                                                  : (long long)length[ln] + std::max(UMX_MAX_SHIFT - shift_offset[ln], shift_offset[ln]);
        if (l2 > 0x7fffffff / 2)
        {
            set_error("track: too long");
            return UMX_ERR_ARG;
        }
        L2[ln] = (int)l2;
        L2max = std::max(L2max, L2[ln]);
    }
    const int stride = (int)((1 - 0.25f) * N); // umx.cpp:181, inference.hpp:15
    // lanes whose per-segment stem buffers are needed: one per track, or (reset mode) one per segment of a call
    const int seg_lanes = reset_lanes ? (int)std::min<long long>(B, ((long long)L2max + stride - 1) / stride) : nt;
    if (trk.size() < (size_t)seg_lanes)
        trk.resize(seg_lanes);
    for (int ln = 0; ln < seg_lanes; ++ln)
    {
        if (ln < nt)
            if (int rc = track_bufs_grow(trk[ln], (size_t)L2[ln]))
                return rc;
        if (int rc = track_bufs_segs(trk[ln]))
            return rc;
    }
    if (!trk_acc_ev[0])
        for (int s = 0; s < nslots; ++s)
            UMX_HIP_CHECK(hipEventCreateWithFlags(&trk_acc_ev[s], hipEventDisableTiming));
    if (ensemble && (size_t)length[0] > ens_cap) // the mean of the lanes' stems: n44 frames, grow-only
    {
        for (float *&p : ens_out)
            if (p)
            {
                allocs.erase(std::find(allocs.begin(), allocs.end(), (void *)p));
                (void)hipFree(p);
                p = nullptr;
            }
        ens_cap = 0;
        const size_t cap = (size_t)length[0] + (size_t)length[0] / 8;
        for (float *&p : ens_out)
            if (int rc = dalloc(&p, 2 * cap, false))
                return rc;
        ens_cap = cap;
    }
    // umx.cpp:167-171: a fresh, zeroed lstm_data per track; umx.cpp:186-195: zeroed accumulators (and F4)
    UMX_HIP_CHECK(hipMemset(state, 0, sizeof(float) * state_floats() * (reset_lanes ? B : nt)));
    clear_used();
    for (int ln = 0; ln < nt; ++ln) // (reset mode: nt = 1)
    {
        TrackBufs &tb_ = trk[ln];
        UMX_HIP_CHECK(hipMemset(tb_.in, 0, sizeof(float) * 2 * (size_t)L2[ln]));
        for (int t = 0; t < 4; ++t)
            UMX_HIP_CHECK(hipMemset(tb_.out[t], 0, sizeof(float) * 2 * (size_t)L2[ln]));
        UMX_HIP_CHECK(hipMemset(tb_.sumw, 0, sizeof(float) * (size_t)L2[ln]));
    }
    // a resampled track goes up whole at its own rate, into a grow-only staging buffer, and is resampled straight into the padded
    // 44.1 kHz signal (upload_until below then has nothing left to do for it)
    if (rs_stage.size() < (size_t)nt)
        rs_stage.resize(nt);
    for (int ln = 0; ln < (ensemble ? 1 : nt); ++ln) // (an ensemble's one track: staged and resampled once, into lane 0)
    {
        if (!resampled[ln])
            continue;
        RsStage &rs = rs_stage[ln];
        if ((size_t)length_in[ln] > rs.cap)
        {
            for (float **p : {&rs.in, &rs.out[0], &rs.out[1], &rs.out[2], &rs.out[3]})
                if (*p)
                {
                    allocs.erase(std::find(allocs.begin(), allocs.end(), (void *)*p));
                    (void)hipFree(*p);
                    *p = nullptr;
                }
            rs.cap = 0;
            const size_t cap = (size_t)length_in[ln] + (size_t)length_in[ln] / 8;
            for (float **p : {&rs.in, &rs.out[0], &rs.out[1], &rs.out[2], &rs.out[3]})
                if (int rc = dalloc(p, 2 * cap, false))
                    return rc;
            rs.cap = cap;
        }
        UMX_HIP_CHECK(hipMemcpy(rs.in, audio_host[ln], sizeof(float) * 2 * (size_t)length_in[ln], hipMemcpyHostToDevice));
        const float *src = rs.in;
        float *dst = trk[ln].in + 2 * (size_t)lead[ln];
        UMX_HIP_CHECK(launch_resample(rs_fwd[ln], rs_fwd_taps[ln], 1, &src, length_in[ln], &dst, length[ln], nullptr));
    }
    // an ensemble's track crosses PCIe once, whole, into lane 0 (unless the resampler has just written it there); the other lanes
    // get it from lane 0, device to device, behind their own shift's zeros (the memsets above)
    if (ensemble)
    {
        float *first = trk[0].in + 2 * (size_t)lead[0];
        const size_t bytes = sizeof(float) * 2 * (size_t)length[0];
        if (!resampled[0])
            UMX_HIP_CHECK(hipMemcpy(first, audio_host[0], bytes, hipMemcpyHostToDevice));
        for (int ln = 1; ln < nt; ++ln)
            UMX_HIP_CHECK(hipMemcpy(trk[ln].in + 2 * (size_t)lead[ln], first, bytes, hipMemcpyDeviceToDevice));
    }
    UMX_HIP_CHECK(hipDeviceSynchronize());
    // The track goes up segment by segment (round 6): a call needs the samples up to the end of its last segment, and the rest of a
    // pageable upload (14 GB/s: 15 ms for ten minutes of stereo) runs while the device is busy with the segments before it -- the
    // slots' streams do not wait for the null stream, and launches are queued ahead of the copy.
    long long uploaded[LSTMB_MAX_TRACKS] = {}; // host samples of each track already on the device
    for (int ln = 0; ln < nt; ++ln)
        if (resampled[ln] || ensemble)
            uploaded[ln] = length[ln];
    auto upload_until = [&](int ti, long long padded_end) -> hipError_t { // samples of the padded signal below `padded_end` must be there
        return track_upload_until(trk[ti].in, audio_host[ti], length[ti], lead[ti], uploaded[ti], padded_end);
    };

    // the mix of `count` frames of lane ln (track_mix); column 4 is the lane's own padded input at the same index
    auto queue_mix = [&](int ln, float *const stems[4], size_t stem_start, size_t in_start, int count, hipStream_t st) {
        track_mix(*mix, stems, stem_start, trk[ln].in, in_start, count, st);
    };

    const float total_reps = std::ceil((float)L2max / (float)stride); // umx.cpp:208 (of the longest track)
    float done = 0.f;
    // A sample is final once the segment that starts at or before it and the one before that have been blended
    // in: region [offset_i, offset_{i+1}) right after segment i.  It is normalised there and then, and the host
    // downloads it while the GPU is already busy with the following segments.
    struct Region
    {
        int lane, start, count;
        hipEvent_t ready;
    };
    std::vector<Region> regions;
    auto cleanup = [&]() {
        for (Region &r : regions)
            (void)hipEventDestroy(r.ready);
    };
    int last_slot = -1, iseg = 0;
    const int per_call = reset_lanes ? seg_lanes : 1; // segments of a track per call
    for (long long off = 0; off < L2max; off += (long long)stride * per_call, ++iseg)
    {
        const int si = next_slot();
        const float *ain[LSTMB_MAX_TRACKS] = {};
        int nn[LSTMB_MAX_TRACKS] = {}, seg_off[LSTMB_MAX_TRACKS] = {};
        float *outs[4 * LSTMB_MAX_TRACKS] = {};
        const int nl = reset_lanes ? per_call : nt; // lanes of this call: lane = track (its segment at `off`), or lane k = segment k of the call
        for (int ln = 0; ln < nl; ++ln)
        {
            const int ti = reset_lanes ? 0 : ln;
            const long long so = reset_lanes ? off + (long long)ln * stride : off;
            if (so < L2[ti]) // this track still has a segment here (umx.cpp:214-217)
            {
                seg_off[ln] = (int)so;
                ain[ln] = trk[ti].in + 2 * (size_t)so;
                nn[ln] = std::min(N, L2[ti] - (int)so);
                if (upload_until(ti, so + N) != hipSuccess)
                {
                    cleanup();
                    set_error("track: upload failed");
                    return UMX_ERR_HIP;
                }
                for (int t = 0; t < 4; ++t)
                    outs[4 * ln + t] = trk[ln].seg[si][t];
            }
        }
        if (reset_lanes && iseg > 0) // every segment from a zero state: the previous call has left its own behind
        {
            if (int rc = sync_all())
            {
                cleanup();
                return rc;
            }
            UMX_HIP_CHECK(hipMemset(state, 0, sizeof(float) * state_floats() * B));
            UMX_HIP_CHECK(hipDeviceSynchronize());
        }
        const int rc = infer_batch(nl, ain, nn, outs, flags);
        if (rc)
        {
            cleanup();
            return rc;
        }
        hipStream_t st = slot[si].stream;
        if (last_slot >= 0) // accumulate in segment order (two segments overlap by a quarter)
            (void)hipStreamWaitEvent(st, trk_acc_ev[last_slot], 0);
        for (int ln = 0; ln < nl; ++ln)
        {
            if (!ain[ln])
                continue;
            const int ti = reset_lanes ? 0 : ln, offset = seg_off[ln];
            Region rg;
            rg.lane = ti;
            rg.start = offset;
            // the region is final: its mix goes over its stems right here, before `ready` (a resampled track is mixed whole, below;
            // an ensemble's lanes are averaged behind the last segment, nothing is downloaded region by region)
            rg.count = track_region(trk[ti], trk[ln].seg[si], offset, nn[ln], L2[ti], stride, mix && !ensemble && !resampled[ti] ? mix : nullptr, st);
            if (ensemble)
                continue;
            if (hipEventCreateWithFlags(&rg.ready, hipEventDisableTiming) != hipSuccess || hipEventRecord(rg.ready, st) != hipSuccess)
            {
                cleanup();
                set_error("track: event creation failed");
                return UMX_ERR_HIP;
            }
            regions.push_back(rg);
        }
        (void)hipEventRecord(trk_acc_ev[si], st);
        last_slot = si;
        done += 1.0f / total_reps; // umx.cpp:229 (queued, not finished: the device runs behind the host here)
        if (progress)
            progress(done, progress_user);
    }
    // a resampled track's four stems: n44 frames from the shift on, back to the caller's rate in one launch behind the last
    // segment's overlap-add (they are downloaded whole below, not region by region)
    hipError_t cerr = hipSuccess;
    const hipStream_t last_st = slot[last_slot].stream;
    if (ensemble)
    {
        // Every lane's last overlap-add is ordered before this stream's (trk_acc_ev chains the calls).  The mean of the lanes' `length`
        // frames from their shifts on goes to ens_out; a resampled track's four means (n44 frames) then go back to the caller's rate
        // in one launch, as a single resampled track's stems would.
        ShiftMeanLanes lanes = {};
        Stems4 mean;
        for (int t = 0; t < 4; ++t)
        {
            for (int ln = 0; ln < nt; ++ln)
                lanes.src[ln][t] = reinterpret_cast<const float2 *>(trk[ln].out[t]) + lead[ln];
            mean.p[t] = reinterpret_cast<float2 *>(ens_out[t]);
        }
        for (hipEvent_t &e : ens_ev)
            if (!e)
                UMX_HIP_CHECK(hipEventCreate(&e));
        (void)hipEventRecord(ens_ev[0], last_st);
        launch_shift_mean(lanes, nt, mean, length[0], last_st);
        (void)hipEventRecord(ens_ev[1], last_st);
        ens_timed = true;
        if (mix) // the mix of the MEAN, over the means (column 4: lane 0's copy of the track); what follows handles n_host buffers
            queue_mix(0, ens_out, 0, (size_t)lead[0], length[0], last_st);
        float *const *result = ens_out;
        if (resampled[0])
        {
            const float *src[4] = {ens_out[0], ens_out[1], ens_out[2], ens_out[3]};
            cerr = launch_resample(rs_back[0], rs_back_taps[0], n_host, src, length[0], rs_stage[0].out, length_in[0], last_st);
            result = rs_stage[0].out;
        }
        if (cerr == hipSuccess)
            cerr = hipStreamSynchronize(last_st);
        for (int t = 0; t < n_host && cerr == hipSuccess; ++t)
            cerr = hipMemcpy(out_host[t], result[t], sizeof(float) * 2 * (size_t)length_in[0], hipMemcpyDeviceToHost);
    }
    for (int ln = 0; ln < nt && cerr == hipSuccess && !ensemble; ++ln)
        if (resampled[ln])
        {
            if (mix) // the n44 frames are mixed at 44.1 kHz, then its n_host buffers go back
                queue_mix(ln, trk[ln].out, (size_t)lead[ln], (size_t)lead[ln], length[ln], last_st);
            const float *src[4];
            for (int t = 0; t < 4; ++t)
                src[t] = trk[ln].out[t] + 2 * (size_t)lead[ln];
            cerr = launch_resample(rs_back[ln], rs_back_taps[ln], n_host, src, length[ln], rs_stage[ln].out, length_in[ln], last_st);
        }
    for (const Region &rg : regions) // umx.cpp:136-147: drop the shift
    {
        const int ln = rg.lane;
        if (resampled[ln])
            continue;
        if (cerr == hipSuccess)
            cerr = track_region_download(trk[ln], rg.start, rg.count, lead[ln], length[ln], n_host, out_host + n_host * ln, rg.ready);
    }
    cleanup();
    bool synced = false;
    for (int ln = 0; ln < nt && cerr == hipSuccess && !ensemble; ++ln)
        if (resampled[ln])
        {
            if (!synced)
                cerr = hipStreamSynchronize(last_st);
            synced = true;
            for (int t = 0; t < n_host && cerr == hipSuccess; ++t)
                cerr = hipMemcpy(out_host[n_host * ln + t], rs_stage[ln].out[t], sizeof(float) * 2 * (size_t)length_in[ln], hipMemcpyDeviceToHost);
        }
    if (cerr != hipSuccess)
    {
        set_error(hipGetErrorString(cerr));
        return UMX_ERR_HIP;
    }
    UMX_HIP_CHECK(hipGetLastError());
    if (int rc = umx_hip_sync(this)) // surfaces a persistent-kernel timeout
        return rc;
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
