// umx_batch.cpp -- `umx-batch <model file> <out dir> <wav file> [<wav file> ...]`: the reference's CLI (umx.cpp:26-97) for
// up to 16 files at a time.  The reference is one track per process; on the GPU the LSTM recurrence of one track is
// bound by hand-off latency, not arithmetic, so the engine runs several tracks as track lanes of ONE context
// (umx_hip_create_tracks / umx_hip_separate_tracks): per file the same shift_inference -> split_inference, the same
// four stems, written to <out dir>/<wav stem>/target_{0..3}.wav.  More files than track lanes (at most 64; UMX_BATCH_LANES=<1..64> caps
// them) go through the track queue (umx_hip_separate_queue): a lane takes the next file the moment its file ends, one
// thread decodes files ahead (at most lanes + 2 decoded files in memory), one writes the stems, and the GPU waits for neither.
// UMX_BATCH_QUEUE=0 forces the pass-by-pass loop (`lanes` files decoded, run for as long as the longest, written).  Either way a
// file's stems and its output directory are the same.
// Environment: UMX_DEVICE, UMX_NO_WIENER, UMX_WIENER_ITERS, UMX_SHIFT_OFFSET, UMX_RESAMPLE (as umx-cli: files of any rate of
// 8 .. 192 kHz, mixed rates in one run -- a queue job carries its file's rate, the loop goes through umx_hip_separate_tracks_rate --,
// stems written at each file's rate), UMX_TARGETS and
// UMX_RESIDUAL (as umx-cli: target_<t>.wav of the chosen targets and residual.wav per file; host/targets_env.h), UMX_SOFTMASK (as umx-cli),
// UMX_MIX (as umx-cli, host/mix_env.h: the same matrix for every file, <out dir>/<wav stem>/<name>.wav and no target_*.wav),
// UMX_PCM16 and UMX_PCM16_DITHER (as umx-cli, DESIGN 19: every output a 16-bit PCM WAV quantised on the device, through the queue and
// the pass-by-pass loop alike; the files go up as int16 when ALL of them are 16-bit PCM -- a run has one input format -- else as fp32).
// UMX_PCM24 and UMX_PCM24_DITHER (as umx-cli, DESIGN 24: every output a 24-bit PCM WAV; one input format per run: packed 24-bit when
// every file's head says 24-bit PCM, else int16 when every file is 16-bit PCM, else fp32; not together with UMX_PCM16).
// UMX_CLIP and UMX_LEVELS (as umx-cli; host/clip_env.h): rescale instead of clamp, and one `levels <file> ...` line per
// file written, through the queue (umx_hip_separate_queue_levels) and the pass-by-pass loop (umx_hip_separate_tracks_levels) alike.
// UMX_LOUDNESS (as umx-cli): one `loudness <file> ...` line per file written, through the queue
// (umx_hip_separate_queue_loudness) and the pass-by-pass loop (umx_hip_separate_tracks_loudness) alike.
// UMX_TRUE_PEAK (as umx-cli): one `true_peak <file> ...` line per file written, through the queue
// (umx_hip_separate_queue_true_peak) and the pass-by-pass loop (umx_hip_separate_tracks_true_peak) alike; rescale needs UMX_CLIP=rescale.
#include "../../include/umx_host.h"
#include "clip_env.h"
#include "mix_env.h"
#include "pcm_env.h"
#include "shifts_env.h"
#include "targets_env.h"

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <filesystem>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

static int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// The track queue's two ends.  A decoded file waits in `decoded` until a lane takes it (next); its stems wait in `unwritten` from the
// moment they are complete (done) until the writer has written them.  `permits` bounds the decoded files in memory (waiting or in a
// lane) to lanes + 2 -- as many as the engine can have in flight, so the reader can always decode the file `next` waits for --
// and max_unwritten the finished ones: done waits for the writer rather than let stems pile up.
struct FileJob
{
    int index = 0, n = 0, rate = UMX_SAMPLE_RATE; // (the file's own rate with UMX_RESAMPLE=1)
    float *audio = nullptr;
    int16_t *audio16 = nullptr; // UMX_PCM16 / UMX_PCM24 with integer PCM files: the file's samples as they are (int16 frames, or packed
                                // 24-bit frames of 6 bytes behind this pointer: load_int below)
    std::vector<std::vector<float>> stems;
    std::vector<std::vector<int16_t>> stems16; // UMX_PCM16 / UMX_PCM24: the outputs as they are written (2 or 3 int16 units a frame)
    umx_measured measured;                     // UMX_CLIP / UMX_LEVELS, UMX_LOUDNESS, UMX_TRUE_PEAK: what the queue measured
};
struct BatchQueue
{
    std::mutex m;
    std::condition_variable cv;
    std::deque<FileJob *> decoded, unwritten;
    int permits = 0, per_file = 4, shift_offset = 0;
    umx_sample_io io = {UMX_SAMPLE_F32, UMX_SAMPLE_F32, 0, 0};
    size_t max_unwritten = 0;
    bool reader_done = false, no_more_stems = false;
    double audio_secs = 0;
    std::string error; // the first thing that went wrong, on any thread: the run stops

    static int next(void *user, umx_queue_job *job)
    {
        BatchQueue &q = *static_cast<BatchQueue *>(user);
        FileJob *fj = nullptr;
        {
            std::unique_lock<std::mutex> lock(q.m);
            q.cv.wait(lock, [&]() { return !q.decoded.empty() || q.reader_done || !q.error.empty(); });
            if (!q.error.empty())
                return -1;
            if (q.decoded.empty())
                return 0;
            fj = q.decoded.front();
            q.decoded.pop_front();
        }
        fj->stems.resize(q.per_file);
        fj->stems16.resize(q.per_file);
        for (int t = 0; t < q.per_file; ++t)
            if (q.io.out_format != UMX_SAMPLE_F32) // (read as the formats say: the caller casts)
            {
                fj->stems16[t].resize(int_units(q.io.out_format) * fj->n);
                job->out[t] = reinterpret_cast<float *>(fj->stems16[t].data());
            }
            else
            {
                fj->stems[t].resize((size_t)2 * fj->n);
                job->out[t] = fj->stems[t].data();
            }
        job->audio = fj->audio16 ? reinterpret_cast<const float *>(fj->audio16) : fj->audio;
        job->length = fj->n;
        job->shift_offset = q.shift_offset;
        job->rate = fj->rate;
        job->tag = fj;
        return 1;
    }
    static void done(void *user, const umx_queue_job *job)
    {
        BatchQueue &q = *static_cast<BatchQueue *>(user);
        FileJob *fj = static_cast<FileJob *>(job->tag);
        umx_wav_free(fj->audio);
        umx_wav_free_pcm16(fj->audio16);
        fj->audio = nullptr;
        fj->audio16 = nullptr;
        std::unique_lock<std::mutex> lock(q.m);
        ++q.permits;
        q.cv.notify_all();
        q.cv.wait(lock, [&]() { return q.unwritten.size() < q.max_unwritten || !q.error.empty(); });
        q.unwritten.push_back(fj);
        q.cv.notify_all();
    }
    // the measuring queues' callbacks: the records they are given (valid during the callback only) are kept with the file
    static void done_measured(void *user, const umx_queue_job *job, const umx_levels *levels, const umx_loudness *loudness,
                              const umx_true_peak *true_peak)
    {
        umx_measured &m = static_cast<FileJob *>(job->tag)->measured;
        m.levels = *levels;
        if (loudness)
            m.loudness = *loudness;
        if (true_peak)
            m.true_peak = *true_peak;
        done(user, job);
    }
    static void done_levels(void *user, const umx_queue_job *job, const umx_levels *levels) { done_measured(user, job, levels, nullptr, nullptr); }
    static void done_loudness(void *user, const umx_queue_job *job, const umx_levels *levels, const umx_loudness *loudness, const double *)
    {
        done_measured(user, job, levels, loudness, nullptr);
    }
    static void done_true_peak(void *user, const umx_queue_job *job, const umx_levels *levels, const umx_loudness *loudness, const double *,
                               const umx_true_peak *true_peak)
    {
        done_measured(user, job, levels, loudness, true_peak);
    }
};

int main(int argc, const char **argv)
{
    if (argc < 4)
    {
        fprintf(stderr, "Usage: %s <model file> <out dir> <wav file> [<wav file> ...]\n", argv[0]);
        return 1;
    }
    const std::string model_file = argv[1], out_dir = argv[2];
    const int nfiles = argc - 3;
    const int lanes_cap = env_int("UMX_BATCH_LANES", UMX_MAX_TRACKS);
    if (lanes_cap < 1 || lanes_cap > UMX_MAX_TRACKS)
    {
        fprintf(stderr, "UMX_BATCH_LANES: need 1 .. %d, got %d\n", UMX_MAX_TRACKS, lanes_cap);
        return 1;
    }
    int lanes = std::min(std::min(nfiles, UMX_MAX_TRACKS), lanes_cap);
    char err[UMX_ERRLEN] = "";
    umx_target_choice choice;
    if (!umx_targets_from_env(choice))
        return 1;
    int shifts = 1;
    if (!umx_shifts_from_env(shifts))
        return 1;
    if (shifts > 1) // (files x shifts in one pass is not offered)
    {
        fprintf(stderr, "UMX_SHIFTS=%d: umx-batch runs one FILE per track lane and has none left for shifts; use umx-cli per file\n", shifts);
        return 1;
    }
    umx_mix_choice mixc;
    const int mixed = umx_mix_from_env(mixc, (choice.flags & UMX_FLAG_RESIDUAL) ? umx_hip_residual_slot(choice.flags) : -1);
    if (mixed < 0)
        return 1;
    if (mixed && umx_mix_silent_source(mixc, choice.write))
    {
        fprintf(stderr, "UMX_MIX: source \"%s\" does not run (UMX_TARGETS) and is not the residual's slot\n", umx_mix_silent_source(mixc, choice.write));
        return 1;
    }
    const int per_file = mixed ? mixc.n_out : 4; // buffers of a file
    umx_pcm_choice pcmc;
    if (!umx_pcm_from_env(pcmc, nullptr))
        return 1;
    umx_clip_choice clipc;
    if (!umx_clip_from_env(clipc, nullptr))
        return 1;
    const bool resample = env_int("UMX_RESAMPLE", 0) != 0;
    umx_sample_io io = pcmc.io;
    // one input format per run: packed 24-bit when every file's head says 24-bit PCM (UMX_PCM24 only), else int16 when every file's head
    // says 16-bit PCM, else fp32 (whatever is wrong with a file, the float loader reports it)
    auto every_file_is = [&](int bits) {
        for (int f = 0; f < nfiles; ++f)
        {
            int n = 0, ch = 0, rate = 0;
            if (load_int(bits == 24 ? UMX_SAMPLE_S24 : UMX_SAMPLE_S16, argv[3 + f], nullptr, &n, &ch, resample ? &rate : nullptr, err))
                return false;
        }
        return true;
    };
    if (pcmc.pcm24 && every_file_is(24))
        io.in_format = UMX_SAMPLE_S24;
    else if (pcmc.active() && every_file_is(16))
        io.in_format = UMX_SAMPLE_S16;
    const bool in16 = io.in_format != UMX_SAMPLE_F32; // (the files go up as they are: int16, or packed 24-bit)
    const bool int_out = pcmc.active();
    umx_model *model = nullptr;
    if (umx_model_load(model_file.c_str(), &model, err)) // umx.cpp:63-70
    {
        fprintf(stderr, "Error loading model: %s\n", err);
        return 1;
    }
    umx_hip_ctx *ctx = nullptr;
    int rc = umx_hip_create_tracks(&ctx, env_int("UMX_DEVICE", 0), umx_model_hidden(model), UMX_SEGMENT_SAMPLES, umx_model_views(model),
                                   umx_model_n_tensors(model), 0, lanes);
    if (rc && lanes > 16) // more than 16 lanes need the u8-resident W_hh of a quantised model: an f32 model gets 16
    {
        lanes = 16;
        rc = umx_hip_create_tracks(&ctx, env_int("UMX_DEVICE", 0), umx_model_hidden(model), UMX_SEGMENT_SAMPLES, umx_model_views(model),
                                   umx_model_n_tensors(model), 0, lanes);
    }
    if (rc)
    {
        fprintf(stderr, "umx_hip_create_tracks: %s\n", umx_hip_last_error(nullptr));
        return 1;
    }
    umx_model_free(model);
    const int wiener_iters = env_int("UMX_WIENER_ITERS", 1); // Wiener EM iterations (wiener.cpp:175; Open-Unmix's niter)
    if (wiener_iters < 1 || wiener_iters > 15)
    {
        fprintf(stderr, "UMX_WIENER_ITERS: need 1 .. 15, got %d\n", wiener_iters);
        return 1;
    }
    const unsigned flags = choice.flags | (env_int("UMX_NO_WIENER", 0) ? UMX_FLAG_NO_WIENER : 0) | (wiener_iters > 1 ? UMX_FLAG_WIENER_ITERS(wiener_iters) : 0u);
    double audio_secs = 0, wall = 0;
    const int first_rand_shift = UMX_REFERENCE_SHIFT; // glibc's first unseeded rand() % 22050 (not rand() here: umx_hip.h)
    // output directories are named after the file's stem, in argument order: a/x.wav and b/x.wav must not collide (the second is x_2)
    std::set<std::string> used_names;
    std::vector<std::string> names(nfiles);
    for (int f = 0; f < nfiles; ++f)
    {
        names[f] = std::filesystem::path(argv[3 + f]).stem().string();
        for (int k = 2; !used_names.insert(names[f]).second; ++k)
            names[f] = std::filesystem::path(argv[3 + f]).stem().string() + "_" + std::to_string(k);
    }
    // umx.cpp:75-96: the buffers of file f to its directory
    auto write_file = [&](int f, float *const *bufs, int16_t *const *bufs16, int n, int rate_, const umx_measured &measured, char *err_) -> bool {
        const std::filesystem::path dir = std::filesystem::path(out_dir) / names[f];
        std::error_code ec;
        std::filesystem::create_directories(dir, ec);
        for (int t = 0; t < per_file; ++t)
        {
            if (!mixed && !choice.write[t]) // a target that did not run (UMX_TARGETS): a silent slot
                continue;
            const std::string p = (dir / (mixed ? mixc.name[t] + ".wav" : choice.file[t])).string();
            if (int_out    ? write_int(io.out_format, p.c_str(), bufs16[t], n, rate_, err_)
                : resample ? umx_wav_write_f32_rate(p.c_str(), bufs[t], n, rate_, err_)
                           : umx_wav_write_f32(p.c_str(), bufs[t], n, err_))
                return false;
            umx_measured_print(p.c_str(), clipc, measured, t);
        }
        return true;
    };
    const int shift_offset = env_int("UMX_SHIFT_OFFSET", -1) < 0 ? first_rand_shift : env_int("UMX_SHIFT_OFFSET", -1);
    // more files than lanes: the track queue (a one-lane context is not track-batched and keeps the loop)
    const bool queued = nfiles > lanes && env_int("UMX_BATCH_QUEUE", 1) != 0 && umx_hip_lstm_is_batched(ctx);
    if (queued)
    {
        BatchQueue q;
        q.permits = lanes + 2;
        q.max_unwritten = (size_t)lanes + 2;
        q.per_file = per_file;
        q.shift_offset = shift_offset;
        q.io = io;
        std::thread reader([&]() {
            for (int f = 0; f < nfiles; ++f)
            {
                {
                    std::unique_lock<std::mutex> lock(q.m);
                    q.cv.wait(lock, [&]() { return q.permits > 0 || !q.error.empty(); });
                    if (!q.error.empty())
                        break;
                    --q.permits;
                }
                FileJob *fj = new FileJob;
                fj->index = f;
                int ch = 0;
                char rerr[UMX_ERRLEN] = "";
                const bool bad = (in16       ? load_int(io.in_format, argv[3 + f], &fj->audio16, &fj->n, &ch, resample ? &fj->rate : nullptr, rerr)
                                  : resample ? umx_wav_load_rate(argv[3 + f], &fj->audio, &fj->n, &ch, &fj->rate, rerr)
                                             : umx_wav_load(argv[3 + f], &fj->audio, &fj->n, &ch, rerr)) != 0; // umx.cpp:56
                std::lock_guard<std::mutex> lock(q.m);
                if (bad)
                {
                    q.error = std::string(argv[3 + f]) + ": " + rerr;
                    delete fj;
                    break;
                }
                q.audio_secs += fj->n / (double)fj->rate;
                q.decoded.push_back(fj);
                q.cv.notify_all();
            }
            std::lock_guard<std::mutex> lock(q.m);
            q.reader_done = true;
            q.cv.notify_all();
        });
        std::thread writer([&]() {
            for (;;)
            {
                FileJob *fj = nullptr;
                {
                    std::unique_lock<std::mutex> lock(q.m);
                    q.cv.wait(lock, [&]() { return !q.unwritten.empty() || q.no_more_stems; });
                    if (q.unwritten.empty())
                        return;
                    fj = q.unwritten.front();
                }
                char werr[UMX_ERRLEN] = "";
                float *bufs[UMX_MAX_MIX_OUTPUTS];
                int16_t *bufs16[UMX_MAX_MIX_OUTPUTS];
                for (int t = 0; t < per_file; ++t)
                {
                    bufs[t] = fj->stems[t].data();
                    bufs16[t] = fj->stems16[t].data();
                }
                const bool ok = write_file(fj->index, bufs, bufs16, fj->n, fj->rate, fj->measured, werr);
                std::lock_guard<std::mutex> lock(q.m);
                q.unwritten.pop_front(); // (counted until it is written: the stems are in memory until then)
                if (!ok && q.error.empty())
                    q.error = werr;
                delete fj;
                q.cv.notify_all();
            }
        });
        const auto t0 = std::chrono::steady_clock::now();
        const int qrc = clipc.true_peak != UMX_TRUE_PEAK_OFF
                            ? umx_hip_separate_queue_true_peak(ctx, BatchQueue::next, BatchQueue::done_true_peak, &q, mixc.n_out,
                                                               mixed ? mixc.gains : nullptr, flags, &io, clipc.clip_mode, clipc.true_peak)
                        : clipc.loudness ? umx_hip_separate_queue_loudness(ctx, BatchQueue::next, BatchQueue::done_loudness, &q, mixc.n_out,
                                                                         mixed ? mixc.gains : nullptr, flags, &io, clipc.clip_mode)
                        : clipc.active() ? umx_hip_separate_queue_levels(ctx, BatchQueue::next, BatchQueue::done_levels, &q, mixc.n_out,
                                                                       mixed ? mixc.gains : nullptr, flags, &io, clipc.clip_mode)
                        : int_out ? umx_hip_separate_queue_io(ctx, BatchQueue::next, BatchQueue::done, &q, mixc.n_out, mixed ? mixc.gains : nullptr, flags, &io)
                              : umx_hip_separate_queue(ctx, BatchQueue::next, BatchQueue::done, &q, mixc.n_out, mixed ? mixc.gains : nullptr, flags);
        wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        {
            std::lock_guard<std::mutex> lock(q.m);
            if (qrc && q.error.empty())
                q.error = std::string("inference failed: ") + umx_hip_last_error(ctx);
            q.no_more_stems = true;
            q.cv.notify_all();
        }
        reader.join();
        writer.join();
        for (FileJob *fj : q.decoded) // (decoded ahead of a run that stopped)
        {
            umx_wav_free(fj->audio);
            umx_wav_free_pcm16(fj->audio16);
            delete fj;
        }
        if (!q.error.empty())
        {
            fprintf(stderr, "%s\n", q.error.c_str());
            return 1;
        }
        audio_secs = q.audio_secs;
    }
    for (int f0 = 0; !queued && f0 < nfiles; f0 += lanes) // pass by pass: `lanes` files decoded, run as long as the longest, written
    {
        const int nb = std::min(lanes, nfiles - f0);
        std::vector<float *> audio(nb, nullptr);
        std::vector<int16_t *> audio16(nb, nullptr);
        std::vector<std::vector<int16_t>> stems16(per_file * nb);
        std::vector<int16_t *> out16(per_file * nb);
        std::vector<const void *> in_io(nb);
        // umx.cpp:115 draws rand() % 22050 once per PROCESS, and the reference never seeds rand(): every run of its CLI
        // shifts by the same 4033 samples.  Every file here gets that value too (not a fresh draw per batch of lanes),
        // so a file's stems do not depend on where in the argument list it stands; UMX_SHIFT_OFFSET overrides it.
        std::vector<int> n(nb, 0), shift(nb, shift_offset);
        std::vector<std::vector<float>> stems(per_file * nb);
        std::vector<float *> out(per_file * nb);
        std::vector<int> rate(nb, UMX_SAMPLE_RATE);
        std::vector<umx_levels> levels(nb);
        std::vector<umx_loudness> loudness(nb);
        std::vector<umx_true_peak> true_peak(nb);
        std::vector<void *> out_io(per_file * nb); // (read as the formats say)
        for (int i = 0; i < nb; ++i)
        {
            int ch = 0;
            if (in16       ? load_int(io.in_format, argv[3 + f0 + i], &audio16[i], &n[i], &ch, resample ? &rate[i] : nullptr, err)
                : resample ? umx_wav_load_rate(argv[3 + f0 + i], &audio[i], &n[i], &ch, &rate[i], err)
                           : umx_wav_load(argv[3 + f0 + i], &audio[i], &n[i], &ch, err)) // umx.cpp:56
            {
                fprintf(stderr, "%s: %s\n", argv[3 + f0 + i], err);
                return 1;
            }
            in_io[i] = in16 ? (const void *)audio16[i] : (const void *)audio[i];
            audio_secs += n[i] / (double)rate[i];
            for (int t = 0; t < per_file; ++t)
            {
                if (int_out)
                    stems16[per_file * i + t].resize(int_units(io.out_format) * n[i]);
                else
                    stems[per_file * i + t].resize((size_t)2 * n[i]);
                out[per_file * i + t] = stems[per_file * i + t].data();
                out16[per_file * i + t] = stems16[per_file * i + t].data();
                out_io[per_file * i + t] = int_out ? (void *)out16[per_file * i + t] : (void *)out[per_file * i + t];
            }
        }
        const auto t0 = std::chrono::steady_clock::now();
        // one call for every run: what a run does not ask for at its neutral value (NULL rates, gains, records, fp32 formats, clamp) is the
        // narrower entry point's request (include/umx_hip.h)
        if (umx_hip_separate_tracks_true_peak(ctx, nb, in_io.data(), n.data(), resample ? rate.data() : nullptr, shift.data(), mixc.n_out,
                                              mixed ? mixc.gains : nullptr, out_io.data(), flags, &io, clipc.clip_mode,
                                              clipc.levels ? levels.data() : nullptr, clipc.loudness ? loudness.data() : nullptr, nullptr,
                                              clipc.true_peak, clipc.true_peak != UMX_TRUE_PEAK_OFF ? true_peak.data() : nullptr, nullptr, nullptr))
        {
            fprintf(stderr, "inference failed: %s\n", umx_hip_last_error(ctx));
            return 1;
        }
        wall += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (int i = 0; i < nb; ++i)
        {
            if (!write_file(f0 + i, &out[per_file * i], &out16[per_file * i], n[i], rate[i], {levels[i], loudness[i], true_peak[i]}, err))
            {
                fprintf(stderr, "%s\n", err);
                return 1;
            }
            umx_wav_free(audio[i]);
            umx_wav_free_pcm16(audio16[i]);
        }
    }
    printf("Separated %d file(s), %.2f s of audio in %.3f s (%.1fx realtime, host buffers in/out, %d track lanes)\n", nfiles, audio_secs, wall,
           audio_secs / wall, lanes);
    umx_hip_destroy(ctx);
    return 0;
}
