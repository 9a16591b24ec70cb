// engine_queue.h -- part of engine.hip (one translation unit: the kernels inline into their launchers): the track queue,
// umx_hip_separate_queue: more tracks than lanes, of different lengths, a lane refilled with the next track the moment one ends.
// This file holds what only a queue has: the schedule (QueueSchedule, umx_hip_queue_plan), the pool of accumulator sets lent to the
// jobs in flight, the in-stream zeroing of a refilled lane, the download of the previous call's regions behind every call, and the
// restart after a timeout.  A job's checks, geometry and admission, the body of a call and the region list are those of engine_tracks.h
// (track_job_ok, track_geometry, admit_job, track_call, TrackRegions), and so is what a job measures: what is zeroed in
// stream order (track_measure_spans), what a restart resets (TrackMeasure::restart) and what is read back (track_report) are stated
// there; what the run's done callback implies and receives is QueueDone's (engine.hip).  The options of a run are the TrackOptions
// record of engine.hip, which every job keeps.  Included by engine.hip behind engine_tracks.h; not a stand-alone header.
// ---------------------------------------------------------------- track queue
namespace
{
// The schedule of include/umx_hip.h (umx_hip_separate_queue), stated once: umx_hip_queue_plan walks it over known segment counts, the
// driver below over the jobs its `next` callback hands out.  Before each call every lane that wants() a job is offered one, in
// ascending lane order (take); step() is one call of infer_batch: every busy lane runs one segment.
struct QueueSchedule
{
    int n_lanes, call = 0, left[LSTMB_MAX_TRACKS] = {}; // left: calls a lane's job still needs
    explicit QueueSchedule(int n) : n_lanes(n) {}
    bool wants(int lane) const { return left[lane] == 0; }
    void take(int lane, int segs) { left[lane] = segs; }
    bool busy() const
    {
        for (int ln = 0; ln < n_lanes; ++ln)
            if (left[ln] > 0)
                return true;
        return false;
    }
    void step()
    {
        for (int ln = 0; ln < n_lanes; ++ln)
            if (left[ln] > 0)
                --left[ln];
        ++call;
    }
    void reset()
    {
        for (int ln = 0; ln < n_lanes; ++ln)
            left[ln] = 0;
    }
};

int queue_plan(int n_lanes, int n_jobs, const int *seg_count, int *lane_out, int *first_call_out, int *n_calls_out)
{
    if (n_lanes < 1 || n_lanes > LSTMB_MAX_TRACKS || n_jobs < 1 || !seg_count)
        return UMX_ERR_ARG;
    for (int j = 0; j < n_jobs; ++j)
        if (seg_count[j] < 1)
            return UMX_ERR_ARG;
    QueueSchedule sched(n_lanes);
    int j = 0;
    for (;;)
    {
        for (int ln = 0; ln < n_lanes && j < n_jobs; ++ln)
            if (sched.wants(ln))
            {
                if (lane_out)
                    lane_out[j] = ln;
                if (first_call_out)
                    first_call_out[j] = sched.call;
                sched.take(ln, seg_count[j++]);
            }
        if (!sched.busy())
            break;
        sched.step();
    }
    if (n_calls_out)
        *n_calls_out = sched.call;
    return UMX_OK;
}
} // namespace

int umx_hip_ctx::queue(umx_queue_next_fn next, const QueueDone &done, void *user, const TrackOptions &opt, unsigned flags)
{
    if (!next || !done)
    {
        set_error("queue: need the next and the done callback");
        return UMX_ERR_ARG;
    }
    if (flags & UMX_FLAG_RESET_SEGMENTS)
    {
        set_error("queue: UMX_FLAG_RESET_SEGMENTS does not go with it (the track lanes carry the jobs)");
        return UMX_ERR_ARG;
    }
    if (!lstm_batched)
    {
        set_error("queue: needs a track-batched context (umx_hip_create_tracks with 2+ lanes, or UMX_CREATE_LSTM_BATCHED): a job's stems "
                  "must not depend on its lane");
        return UMX_ERR_ARG;
    }
    if (int rc = check_flags(flags))
        return rc;
    if (ph_next != -1)
    {
        set_error("queue: a phased segment is open (umx_hip_segment_end first)");
        return UMX_ERR_ARG;
    }
    UMX_HIP_CHECK(hipSetDevice(device));
    if (int rc = sync_all())
        return rc;
    // As tracks(): a persistent-kernel timeout cannot be repaired segment by segment (the overlap-add has consumed the stems); the
    // jobs in flight are run again from their first segment (queue_run).  No call is logged for a replay: `pending` stays empty.
    TrackRun run(*this);
    pending.clear();
    pending_lost = true;
    return queue_run(next, done, user, opt, flags);
}

int umx_hip_ctx::queue_run(umx_queue_next_fn next, const QueueDone &done, void *user, const TrackOptions &opt, unsigned flags)
{
    const int n_host = opt.n_host();
    const int stride = track_stride();
    const size_t n_sets = (size_t)B + 2;
    if (qpool.size() < n_sets)
        qpool.resize(n_sets);
    if (trk.size() < (size_t)B) // (the per-slot segment stems stay with the lane)
        trk.resize(B);

    struct Job : TrackJob // a job in flight = the accumulator set it borrowed: jobs[set].acc == &qpool[set]
    {
        umx_queue_job job;
        int regions_left = 0;
        unsigned long long seq = 0; // order in which `next` handed the jobs out
        bool live = false;
    };
    std::vector<Job> jobs(n_sets);
    TrackLane lanes[LSTMB_MAX_TRACKS]; // a lane's job and where its next segment starts
    QueueSchedule sched(B);
    TrackRegions prev, cur; // finished regions of the previous call and of the one being queued
    std::vector<Job *> redo; // after a timeout: the jobs to run again, ahead of `next`
    bool exhausted = false, retried = false;
    int last_slot = -1;
    unsigned long long seq = 0;
    queue_calls = 0;
    rs_launches[0] = rs_launches[1] = 0;

    auto fail = [&](int rc) { // nothing of this run may still be running, or be copied, when the caller has its buffers back
        const std::string why = err;
        (void)sync_all();
        set_error(why);
        return rc;
    };
    // a timeout among the calls so far: umx_hip_sync has drained the device, zeroed the state and switched to the per-step driver;
    // every job in flight starts again, in the order the jobs were taken
    auto restart = [&]() {
        prev.clear();
        cur.clear();
        redo.clear();
        for (Job &jb : jobs)
            if (jb.live)
                redo.push_back(&jb);
        std::sort(redo.begin(), redo.end(), [](const Job *a, const Job *b) { return a->seq < b->seq; });
        for (Job *jb : redo)
        {
            jb->uploaded = jb->done44 = jb->out_done = 0; // (a resampled job goes through the resampler again, from its host copy)
            jb->m.restart(); // (what it measured is zeroed with its accumulators and measured again)
            jb->regions_left = jb->by_region ? jb->segs : 1;
        }
        for (int ln = 0; ln < B; ++ln)
            lanes[ln] = TrackLane();
        sched.reset();
        last_slot = -1;
        pending_lost = true;
    };
    // The regions in v to the host (event wait, then copy; the event goes as soon as it is consumed).  A job whose last region has
    // arrived is complete -- once no launch up to its last call has timed out: done(), and its set goes back to the pool.
    // 0: fine; > 0: an error code (set_error done); < 0: a timeout was met for the first time and the jobs in flight start again
    auto drain = [&](TrackRegions &v) -> int {
        std::vector<Job *> finished;
        hipError_t e = hipSuccess;
        for (TrackRegion &r : v.v)
        {
            Job &jb = *static_cast<Job *>(r.job);
            if (e == hipSuccess) // (also for a region that is all shift padding: the set is not lent again while the device works on it)
                e = hipEventSynchronize(r.ready);
            if (e == hipSuccess)
                e = track_region_download(r, jb.job.out);
            (void)hipEventDestroy(r.ready);
            r.ready = nullptr;
            if (--jb.regions_left == 0)
                finished.push_back(&jb);
        }
        v.clear();
        if (e != hipSuccess)
        {
            set_error(std::string("queue: download failed: ") + hipGetErrorString(e));
            return UMX_ERR_HIP;
        }
        if (finished.empty())
            return 0;
        bool timed_out = false;
        for (int si = 0; si < nslots && slot[si].status; ++si)
        {
            unsigned st = 0;
            if (hipMemcpy(&st, slot[si].status, sizeof st, hipMemcpyDeviceToHost) != hipSuccess)
            {
                set_error("queue: reading the recurrence's status failed");
                return UMX_ERR_HIP;
            }
            timed_out = timed_out || st != 0;
        }
        if (timed_out)
        {
            const int rc = umx_hip_sync(this); // UMX_ERR_TIMEOUT under no_recovery
            if (rc != UMX_ERR_TIMEOUT)
                return rc ? rc : UMX_ERR_HIP;
            if (retried)
                return rc;
            retried = true;
            restart();
            return -1;
        }
        for (Job *jb : finished)
        {
            TrackReport report; // what the job measured, behind its last region
            if ((e = track_report(*jb, n_host, report)) != hipSuccess)
            {
                set_error(std::string("queue: reading a job's levels failed: ") + hipGetErrorString(e));
                return UMX_ERR_HIP;
            }
            done.call(user, &jb->job, report);
            jb->live = false;
        }
        return 0;
    };

    for (;;)
    {
        // ---- every lane without a track asks for one, in ascending lane order
        bool restarted = false;
        for (int ln = 0; ln < B && !restarted; ++ln)
        {
            if (!sched.wants(ln) || (redo.empty() && exhausted))
                continue;
            Job *jb = nullptr;
            if (!redo.empty())
            {
                jb = redo.front();
                redo.erase(redo.begin());
            }
            else
            {
                auto free_set = [&](size_t need) { // the smallest free set that is large enough, else the largest free one (it grows)
                    int best = -1;
                    for (size_t s = 0; s < n_sets; ++s)
                    {
                        if (jobs[s].live)
                            continue;
                        if (best < 0)
                            best = (int)s;
                        const size_t cb = qpool[best].cap, cs = qpool[s].cap;
                        if (cb >= need ? (cs >= need && cs < cb) : cs > cb)
                            best = (int)s;
                    }
                    return best;
                };
                if (free_set(0) < 0) // every set is lent: the previous call's regions go to the host before this call is queued
                {
                    const int d = drain(prev);
                    if (d > 0)
                        return fail(d);
                    if (d < 0)
                    {
                        restarted = true;
                        break;
                    }
                }
                umx_queue_job j;
                memset(&j, 0, sizeof j);
                const int r = next(user, &j);
                if (r == 0)
                {
                    exhausted = true; // (and next is not called again)
                    continue;
                }
                if (r < 0)
                {
                    set_error("queue: the next callback stopped the run");
                    return fail(UMX_ERR_ARG);
                }
                if (!track_job_ok(j.audio, j.length, j.shift_offset, j.out, n_host))
                {
                    set_error("queue: a job needs audio, its n_out outputs, length >= 1 and shift offset < 22050");
                    return fail(UMX_ERR_ARG);
                }
                // A job at another rate (rate 0: 44.1 kHz) runs as the n44 frames of its 44.1 kHz version, as in tracks_once:
                // its geometry, its set's size and the spans zeroed below are in those frames, its int16 side and loudness in its own.
                const int rate = j.rate ? j.rate : RS_MODEL_RATE;
                TrackResample rs;
                int n44 = j.length;
                if (rate != RS_MODEL_RATE)
                    if (int rc = track_rate_plan(rate, j.length, "queue: a job is too long", rs, n44))
                        return fail(rc);
                TrackJob tj; // (the geometry first: the set is chosen by its size)
                if (!track_geometry(n44, j.shift_offset, stride, tj))
                {
                    set_error("queue: a job is too long");
                    return fail(UMX_ERR_ARG);
                }
                tj.rs = rs;
                const int set = free_set((size_t)tj.L2);
                // (a rescaled job is one whole-track region, queued with its last segment)
                if (int rc = admit_job(tj, qpool[set], opt, j.audio, rate, j.length, false))
                    return fail(rc);
                jb = &jobs[set];
                static_cast<TrackJob &>(*jb) = tj;
                jb->job = j;
                jb->regions_left = tj.by_region ? tj.segs : 1;
                jb->seq = seq++;
                jb->live = true;
            }
            lanes[ln].job = jb;
            lanes[ln].start = 0;
            sched.take(ln, jb->segs);
        }
        if (restarted)
            continue;
        if (!sched.busy()) // no lane holds a track: what is left is the last call's regions
        {
            if (prev.v.empty())
                break;
            const int d = drain(prev);
            if (d > 0)
                return fail(d);
            continue;
        }

        // ---- one call: the next segment of every lane's job
        const hipStream_t st = slot[next_slot()].stream;
        int nl = 0;
        bool waited = false;
        for (int ln = 0; ln < B; ++ln)
        {
            const TrackJob *jb = lanes[ln].job;
            if (!jb)
                continue;
            if (lanes[ln].start == 0)
            {
                // A refilled lane starts clean, in stream order: behind the previous call (the lane's previous occupant has run its last
                // recurrence) the lane's state slice, the set's accumulators and the shift padding of its padded input are zeroed in one
                // launch.  The set itself is free: the host has its last region.  The span of `in` the uploads fill is not touched, so they
                // need no ordering against this kernel.
                if (!waited && last_slot >= 0)
                    (void)hipStreamWaitEvent(st, trk_acc_ev[last_slot], 0);
                waited = true;
                const TrackBufs &tb_ = *jb->acc;
                TrackBeginSpans sp = {};
                for (int t = 0; t < 4; ++t)
                {
                    sp.p[t] = tb_.out[t];
                    sp.n[t] = 2 * (unsigned long long)jb->L2;
                }
                sp.p[4] = tb_.sumw;
                sp.n[4] = (unsigned long long)jb->L2;
                sp.p[5] = tb_.in;
                sp.n[5] = 2 * (unsigned long long)jb->lead;
                sp.p[6] = tb_.in + 2 * ((size_t)jb->lead + (size_t)jb->length);
                sp.n[6] = 2 * (unsigned long long)(jb->L2 - jb->lead - jb->length);
                sp.p[7] = state + state_floats() * (size_t)ln;
                sp.n[7] = state_floats();
                sp.count = TRACK_BEGIN_SPANS;
                launch_track_begin(sp, st);
                ZeroSpan spans[3]; // ... and what the job measures into (also on a restart: it measures from zero again)
                for (int k = 0, n = track_measure_spans(*jb, spans); k < n; ++k)
                    (void)hipMemsetAsync(spans[k].p, 0, spans[k].bytes, st);
            }
            nl = ln + 1;
        }
        pending_lost = true;
        if (int rc = track_call(lanes, nl, flags, last_slot, cur))
            return fail(rc);
        ++queue_calls;
        for (int ln = 0; ln < nl; ++ln)
            if (lanes[ln].job && (lanes[ln].start += stride) >= lanes[ln].job->L2)
                lanes[ln] = TrackLane(); // the lane is free for the next call; the job lives on until its regions are down
        sched.step();
        // ---- while the device runs this call: the regions of the one before
        const int d = drain(prev);
        if (d > 0)
            return fail(d);
        if (d < 0)
            continue;
        prev.v.swap(cur.v);
    }
    UMX_HIP_CHECK(hipGetLastError());
    return umx_hip_sync(this);
}
