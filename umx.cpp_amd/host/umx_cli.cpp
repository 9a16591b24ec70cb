// umx_cli.cpp -- `umx-cli <model file> <wav file> <out dir>`: the reference's CLI (umx.cpp:26-97)
// over the MI355X engine.  Loads the wav, loads the ggml weight file, creates the device context,
// runs shift_inference -> split_inference on the device (umx_hip_shift_inference: track resident in HBM,
// segments pipelined; UMX_CLI_PER_SEGMENT=1 selects the host drivers over umx_hip_infer_segment), writes
// target_{0..3}.wav (0 = bass, 1 = drums, 2 = other, 3 = vocals).  Exit code 1 on any failure,
// like the reference.  Extra knobs come from the environment only, so the 3 positionals stay:
//   UMX_DEVICE=<n>   UMX_NO_WIENER=1   UMX_WIENER_ITERS=<1..15>   UMX_SHIFT_OFFSET=<n>   UMX_LSTM_STEPWISE=1   UMX_CLI_PER_SEGMENT=1
//   UMX_WEIGHTS_RESIDENT=expanded   UMX_GEMM=f32
//   UMX_RESAMPLE=1   any rate of 8 .. 192 kHz: resampled to 44.1 kHz and back on the device (umx_hip_shift_inference_rate,
//                    DESIGN 13); the stems are written at the input's rate and length
//   UMX_TARGETS=<comma list of bass,drums,other,vocals>   only these targets run and are written (target_<t>.wav)
//   UMX_RESIDUAL=1   with UMX_TARGETS: residual.wav = everything else in the mix (UMX_FLAG_RESIDUAL; host/targets_env.h)
//   UMX_SOFTMASK=1   Open-Unmix's softmask=True: first estimates that add up to the mixture (UMX_FLAG_SOFTMASK; host/targets_env.h)
//   UMX_SHIFTS=<1..64>   Demucs' --shifts: the mean of that many separations at the offsets umx_hip_ensemble_offsets(K, UMX_SHIFT_OFFSET)
//                    (umx_hip_shift_ensemble; host/shifts_env.h), as track lanes of a context made like umx-batch's (create
//                    flags 0: UMX_WEIGHTS_RESIDENT and UMX_GEMM do not apply); goes with every knob above except UMX_CLI_PER_SEGMENT.
//                    1 or unset: one shift, the path and the files of a run without it
//   UMX_MIX=<name=expr;...>   the stem mix matrix (grammar in host/mix_env.h): <out dir>/<name>.wav for each of the 1 .. 4
//                    outputs, weighted sums of the stems and of the input formed on the device, and no target_*.wav; goes with every
//                    knob above except UMX_CLI_PER_SEGMENT; a source whose target does not run (UMX_TARGETS) is refused.  Unset or
//                    empty: the path and the files of a run without it
//   UMX_PCM16=1      16-bit PCM across PCIe (umx_hip_separate_tracks_io): the stems, or the UMX_MIX outputs, are written as
//                    16-bit PCM WAVs under the same names, quantised on the device, and a 16-bit PCM input goes up as int16 (any other
//                    encoding as fp32); UMX_PCM16_DITHER=<seed> adds TPDF dither with that seed.  Goes with UMX_RESAMPLE, UMX_TARGETS /
//                    UMX_RESIDUAL, UMX_MIX and the other knobs; not with UMX_SHIFTS > 1 or UMX_CLI_PER_SEGMENT.  Unset: today's files
//   UMX_PCM24=1      packed 24-bit PCM across PCIe (UMX_SAMPLE_S24): the outputs are written as 24-bit PCM WAVs under the same
//                    names, quantised on the device; a 24-bit PCM input goes up packed, a 16-bit one as int16, any other encoding as
//                    fp32; UMX_PCM24_DITHER=<seed> adds TPDF dither with that seed.  Goes where UMX_PCM16 goes, not together with it.
//                    Unset: today's files
//   UMX_CLIP=clamp|rescale, UMX_LEVELS=1   what happens to outputs beyond full scale, and one `levels <file> ...` line per file written
//                    (umx_hip_separate_tracks_levels; host/clip_env.h); with and without UMX_PCM16 and the knobs it goes
//                    with; not with UMX_SHIFTS > 1 or UMX_CLI_PER_SEGMENT.  Unset (or clamp, 0): today's files
//   UMX_LOUDNESS=1   one `loudness <file> integrated=<LUFS> momentary_max=<LUFS> blocks=<n> gated=<n>` line per file written, BS.1770-4 /
//                    R128 loudness measured on the device (umx_hip_separate_tracks_loudness; host/clip_env.h); goes where
//                    UMX_LEVELS goes.  Unset or 0: today's output
//   UMX_TRUE_PEAK=1|rescale   one `true_peak <file> dbtp=<dBTP> linear=<x> factor=<F>` line per file written, the oversampled peak
//                    measured on the device (umx_hip_separate_tracks_true_peak; host/clip_env.h); rescale: UMX_CLIP=rescale
//                    (required) divides by the true peak instead of the sample peak.  Goes where UMX_LOUDNESS goes.  Unset or 0: today's output
#include "../../include/umx_host.h"
#include "clip_env.h"
#include "mix_env.h"
#include "pcm_env.h"
#include "shifts_env.h"
#include "targets_env.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <string>
#include <vector>

namespace
{
struct HipBackend
{
    umx_hip_ctx *ctx;
    unsigned flags;
};
int hip_segment(void *user, const float *audio, int n, float *const out[4])
{
    HipBackend *b = static_cast<HipBackend *>(user);
    int rc = umx_hip_infer_segment(b->ctx, audio, n, out, b->flags);
    if (rc)
        fprintf(stderr, "umx_hip_infer_segment: %s\n", umx_hip_last_error(b->ctx));
    return rc;
}
int hip_reset(void *user) { return umx_hip_stream_reset(static_cast<HipBackend *>(user)->ctx); }
void print_progress(float p, void *) { fprintf(stdout, "inference progress: %.1f %%\n", 100.f * p); }
int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}
} // namespace

int main(int argc, const char **argv)
{
    if (argc != 4) // umx.cpp:28-33
    {
        fprintf(stderr, "Usage: %s <model file> <wav file> <out dir>\n", argv[0]);
        return 1;
    }
    const std::string model_file = argv[1], wav_file = argv[2], out_dir = argv[3];
    char err[UMX_ERRLEN] = "";
    umx_target_choice choice;
    if (!umx_targets_from_env(choice))
        return 1;
    int shifts = 1, shift_offsets[UMX_MAX_SHIFTS];
    if (!umx_shifts_from_env(shifts))
        return 1;
    if (shifts > 1 && env_int("UMX_CLI_PER_SEGMENT", 0))
    {
        fprintf(stderr, "UMX_SHIFTS=%d: the shifts run as track lanes on the device, UMX_CLI_PER_SEGMENT=1 does not go with it\n", shifts);
        return 1;
    }
    if (shifts > 1 && umx_hip_ensemble_offsets(shifts, env_int("UMX_SHIFT_OFFSET", -1), shift_offsets))
    {
        fprintf(stderr, "UMX_SHIFT_OFFSET: need an offset below %d\n", UMX_MAX_SHIFT);
        return 1;
    }
    umx_mix_choice mixc;
    const int mixed = umx_mix_from_env(mixc, (choice.flags & UMX_FLAG_RESIDUAL) ? umx_hip_residual_slot(choice.flags) : -1);
    if (mixed < 0)
        return 1;
    if (mixed && env_int("UMX_CLI_PER_SEGMENT", 0))
    {
        fprintf(stderr, "UMX_MIX: the mix is formed on the device behind the overlap-add, UMX_CLI_PER_SEGMENT=1 does not go with it\n");
        return 1;
    }
    if (mixed && umx_mix_silent_source(mixc, choice.write))
    {
        fprintf(stderr, "UMX_MIX: source \"%s\" does not run (UMX_TARGETS) and is not the residual's slot\n", umx_mix_silent_source(mixc, choice.write));
        return 1;
    }
    umx_pcm_choice pcmc;
    if (!umx_pcm_from_env(pcmc, shifts > 1 || env_int("UMX_CLI_PER_SEGMENT", 0)
                                    ? "the shift ensemble (UMX_SHIFTS > 1) and UMX_CLI_PER_SEGMENT=1 do not offer"
                                    : nullptr))
        return 1;
    umx_clip_choice clipc;
    if (!umx_clip_from_env(clipc, shifts > 1 || env_int("UMX_CLI_PER_SEGMENT", 0)
                                      ? "the shift ensemble (UMX_SHIFTS > 1) and UMX_CLI_PER_SEGMENT=1 do not offer levels or rescale"
                                      : nullptr))
        return 1;
    umx_measured measured;
    umx_sample_io io = pcmc.io;
    printf("umx-cli (MI355X / gfx950) main driver program\n");

    float *audio = nullptr;
    int16_t *audio_int = nullptr; // the file's samples as they are, in io.in_format (load_int)
    int n = 0, ch = 0, rate = UMX_SAMPLE_RATE;
    const bool resample = env_int("UMX_RESAMPLE", 0) != 0;
    if (pcmc.pcm24 && load_int(UMX_SAMPLE_S24, wav_file.c_str(), &audio_int, &n, &ch, resample ? &rate : nullptr, err) == UMX_OK)
        io.in_format = UMX_SAMPLE_S24;
    else if (pcmc.active() && load_int(UMX_SAMPLE_S16, wav_file.c_str(), &audio_int, &n, &ch, resample ? &rate : nullptr, err) == UMX_OK)
        io.in_format = UMX_SAMPLE_S16; // (any other encoding, and every other failure, is the float loader's to take or to report)
    else if (resample ? umx_wav_load_rate(wav_file.c_str(), &audio, &n, &ch, &rate, err) : umx_wav_load(wav_file.c_str(), &audio, &n, &ch, err)) // umx.cpp:56
    {
        fprintf(stderr, "%s\n", err);
        return 1;
    }
    printf("Input Samples: %d\nLength in seconds: %f\nNumber of channels: %d\n", n * ch, n / (double)rate, ch);
    if (resample && rate != UMX_SAMPLE_RATE)
        printf("Sample rate: %d Hz (resampled to 44100 Hz and back on the device)\n", rate);

    const auto t0 = std::chrono::steady_clock::now();
    umx_model *model = nullptr;
    if (umx_model_load(model_file.c_str(), &model, err)) // umx.cpp:63-70
    {
        fprintf(stderr, "Error loading model: %s\n", err);
        return 1;
    }
    const auto t1 = std::chrono::steady_clock::now();
    printf("Loaded model (%d tensors, %6.2f MB) in %f s\n", umx_model_n_tensors(model),
           umx_model_data_bytes(model) / 1024.0 / 1024.0, std::chrono::duration<double>(t1 - t0).count());

    umx_hip_ctx *ctx = nullptr;
    if (shifts > 1 ? umx_hip_create_tracks(&ctx, env_int("UMX_DEVICE", 0), umx_model_hidden(model), UMX_SEGMENT_SAMPLES,
                                           umx_model_views(model), umx_model_n_tensors(model), 0, shifts) // one track lane per shift
                   : umx_hip_create(&ctx, env_int("UMX_DEVICE", 0), umx_model_hidden(model), UMX_SEGMENT_SAMPLES,
                                    umx_model_views(model), umx_model_n_tensors(model)))
    {
        fprintf(stderr, "umx_hip_create: %s\n", umx_hip_last_error(nullptr));
        return 1;
    }
    umx_model_free(model); // weights now live in HBM

    HipBackend hb{ctx, choice.flags};
    if (env_int("UMX_NO_WIENER", 0))
        hb.flags |= UMX_FLAG_NO_WIENER;
    const int wiener_iters = env_int("UMX_WIENER_ITERS", 1); // Wiener EM iterations (wiener.cpp:175; Open-Unmix's niter)
    if (wiener_iters < 1 || wiener_iters > 15)
    {
        fprintf(stderr, "UMX_WIENER_ITERS: need 1 .. 15, got %d\n", wiener_iters);
        return 1;
    }
    if (wiener_iters > 1)
        hb.flags |= UMX_FLAG_WIENER_ITERS(wiener_iters);
    if (env_int("UMX_LSTM_STEPWISE", 0))
        hb.flags |= UMX_FLAG_LSTM_STEPWISE;
    umx_backend be{hip_segment, hip_reset, &hb};
    std::vector<float> stems[4];
    std::vector<int16_t> stems_int[4]; // the outputs as they are written, in io.out_format (int_units a frame)
    float *out[4];
    for (int t = 0; t < (mixed ? mixc.n_out : 4); ++t)
    {
        if (pcmc.active())
            stems_int[t].resize(int_units(io.out_format) * n);
        else
            stems[t].resize((size_t)2 * n);
        out[t] = stems[t].data();
    }
    const auto t2 = std::chrono::steady_clock::now();
    const bool per_segment = env_int("UMX_CLI_PER_SEGMENT", 0) != 0;
    if (per_segment && rate != UMX_SAMPLE_RATE)
    {
        fprintf(stderr, "UMX_CLI_PER_SEGMENT=1 takes 44100 Hz audio only (this file is %d Hz): unset it to resample on the device\n", rate);
        return 1;
    }
    if (per_segment)
    {
        if (umx_shift_inference(&be, audio, n, UMX_SEGMENT_SAMPLES, env_int("UMX_SHIFT_OFFSET", -1), out,
                                print_progress, nullptr, err)) // umx.cpp:72-73
        {
            fprintf(stderr, "inference failed: %s\n", err);
            return 1;
        }
    }
    else if (shifts > 1) // the shift ensemble: another driver (no 16-bit transfers, levels or loudness: refused above)
    {
        if (mixed ? umx_hip_shift_ensemble_mix(ctx, audio, n, rate, shifts, shift_offsets, mixc.n_out, mixc.gains, out, hb.flags, print_progress,
                                               nullptr)
                  : umx_hip_shift_ensemble(ctx, audio, n, rate, shifts, shift_offsets, out, hb.flags, print_progress, nullptr))
        {
            fprintf(stderr, "inference failed: %s\n", umx_hip_last_error(ctx));
            return 1;
        }
    }
    else
    {
        // umx.cpp:72-73.  One call for every run: what a run does not ask for at its neutral value (NULL rate, gains, records, fp32
        // formats, clamp) is the narrower entry point's request (include/umx_hip.h)
        const int offset = env_int("UMX_SHIFT_OFFSET", -1) < 0 ? UMX_REFERENCE_SHIFT : env_int("UMX_SHIFT_OFFSET", -1);
        const void *in = audio_int ? (const void *)audio_int : (const void *)audio;
        void *out_io[4]; // (read as the formats say)
        for (int t = 0; t < 4; ++t)
            out_io[t] = pcmc.active() ? (void *)stems_int[t].data() : (void *)stems[t].data();
        if (umx_hip_separate_tracks_true_peak(ctx, 1, &in, &n, resample ? &rate : nullptr, &offset, mixc.n_out, mixed ? mixc.gains : nullptr, out_io,
                                              hb.flags, &io, clipc.clip_mode, clipc.levels ? &measured.levels : nullptr,
                                              clipc.loudness ? &measured.loudness : nullptr, nullptr, clipc.true_peak,
                                              clipc.true_peak != UMX_TRUE_PEAK_OFF ? &measured.true_peak : nullptr, print_progress, nullptr))
        {
            fprintf(stderr, "inference failed: %s\n", umx_hip_last_error(ctx));
            return 1;
        }
    }
    const auto t3 = std::chrono::steady_clock::now();
    const double secs = std::chrono::duration<double>(t3 - t2).count();
    printf("Separated %.2f s of audio in %.3f s (%.1fx realtime, host buffers in/out, %s)\n", n / (double)rate, secs,
           n / (double)rate / secs, per_segment ? "one segment at a time" : "track resident in HBM");
    if (shifts > 1)
        printf("Mean of %d shifts (offsets %d, %d, ...)\n", shifts, shift_offsets[0], shift_offsets[1]);

    std::error_code ec;
    std::filesystem::create_directories(out_dir, ec); // umx.cpp:84-86
    for (int t = 0; t < (mixed ? mixc.n_out : 4); ++t) // umx.cpp:75-96
    {
        if (!mixed && !choice.write[t]) // a target that did not run (UMX_TARGETS): a silent slot
            continue;
        const std::string p = (std::filesystem::path(out_dir) / (mixed ? mixc.name[t] + ".wav" : choice.file[t])).string();
        printf("Writing wav file %s\n", p.c_str());
        if (pcmc.active() ? write_int(io.out_format, p.c_str(), stems_int[t].data(), n, rate, err)
            : resample    ? umx_wav_write_f32_rate(p.c_str(), out[t], n, rate, err)
                          : umx_wav_write_f32(p.c_str(), out[t], n, err))
        {
            fprintf(stderr, "%s\n", err);
            return 1;
        }
        umx_measured_print(p.c_str(), clipc, measured, t);
    }
    umx_wav_free(audio);
    umx_wav_free_pcm16(audio_int);
    umx_hip_destroy(ctx);
    return 0;
}
