// clip_env.h -- UMX_CLIP and UMX_LEVELS of umx-cli and umx-batch: what happens to outputs beyond full scale, and whether the levels
// of what was written are printed (output levels and clip handling; include/umx_hip.h).
//   UMX_CLIP=clamp|rescale   clamp (the default, and unset or empty): today's files byte for byte -- a 16-bit PCM output clamps, a
//                            float one keeps its samples beyond 1.0.  rescale (Demucs' --clip-mode rescale, per track instead of per
//                            file): every output of a file is divided by max(1.01 * peak over the file's outputs, 1) on the device.
//   UMX_LEVELS=1             one line per output file on stdout, measured on the device:
//                            levels <file> peak=<%.9g> over_unity=<n> clipped=<n> nonfinite=<n> gain=<%.9g>
//   UMX_LOUDNESS=1           one more line per output file, its ITU-R BS.1770-4 / EBU R128 loudness measured on the device:
//                            loudness <file> integrated=<LUFS> momentary_max=<LUFS> blocks=<n> gated=<n>      (-inf is printed as -inf)
//                            UMX_MIX="m=mix" gives the loudness of the input itself.
//   UMX_TRUE_PEAK=1|rescale  one more line per output file, its true peak measured on the device:
//                            true_peak <file> dbtp=<dBTP> linear=<%.9g> factor=<F>                            (-inf is printed as -inf)
//                            rescale: also, UMX_CLIP=rescale divides by 1.01 * the largest TRUE peak of the file's outputs instead of
//                            their sample peak; refused without UMX_CLIP=rescale.
// All go with UMX_PCM16, UMX_MIX, UMX_TARGETS / UMX_RESIDUAL and UMX_RESAMPLE, through umx-batch's queue and its pass-by-pass loop;
// not with UMX_SHIFTS > 1 or UMX_CLI_PER_SEGMENT (the shift ensemble and the per-segment calls do not offer them).
#pragma once
#include "../../include/umx_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

struct umx_clip_choice
{
    int clip_mode = UMX_CLIP_CLAMP;
    bool levels = false;
    bool loudness = false;
    int true_peak = UMX_TRUE_PEAK_OFF;
    bool active() const { return clip_mode != UMX_CLIP_CLAMP || levels || loudness || true_peak != UMX_TRUE_PEAK_OFF; } // false: the calls and the files of a run without the four
};

// false, with a message that names the variable, for a value outside the grammar above (nullptr: unset)
inline bool umx_clip_parse(const char *clip, const char *levels, umx_clip_choice &c, std::string &err)
{
    c = umx_clip_choice();
    if (clip && *clip)
    {
        if (!strcmp(clip, "rescale"))
            c.clip_mode = UMX_CLIP_RESCALE;
        else if (strcmp(clip, "clamp"))
        {
            err = std::string("UMX_CLIP: need clamp or rescale, got \"") + clip + "\"";
            return false;
        }
    }
    if (levels && *levels)
    {
        if (strcmp(levels, "0") && strcmp(levels, "1"))
        {
            err = std::string("UMX_LEVELS: need 0 or 1, got \"") + levels + "\"";
            return false;
        }
        c.levels = levels[0] == '1';
    }
    return true;
}

// false: refused, message on stderr.  not_offered: the reason this run cannot take the two (nullptr: it can)
inline bool umx_clip_from_env(umx_clip_choice &c, const char *not_offered)
{
    std::string err;
    if (!umx_clip_parse(getenv("UMX_CLIP"), getenv("UMX_LEVELS"), c, err))
    {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    if (c.active() && not_offered)
    {
        fprintf(stderr, "UMX_CLIP / UMX_LEVELS: %s\n", not_offered);
        return false;
    }
    if (const char *loud = getenv("UMX_LOUDNESS"))
        if (*loud)
        {
            if (strcmp(loud, "0") && strcmp(loud, "1"))
            {
                fprintf(stderr, "UMX_LOUDNESS: need 0 or 1, got \"%s\"\n", loud);
                return false;
            }
            c.loudness = loud[0] == '1';
            if (c.loudness && not_offered)
            {
                fprintf(stderr, "UMX_LOUDNESS: %s (nor loudness)\n", not_offered);
                return false;
            }
        }
    if (const char *tp = getenv("UMX_TRUE_PEAK"))
        if (*tp)
        {
            if (strcmp(tp, "0") && strcmp(tp, "1") && strcmp(tp, "rescale"))
            {
                fprintf(stderr, "UMX_TRUE_PEAK: need 0, 1 or rescale, got \"%s\"\n", tp);
                return false;
            }
            c.true_peak = !strcmp(tp, "rescale") ? UMX_TRUE_PEAK_RESCALE : tp[0] == '1' ? UMX_TRUE_PEAK_MEASURE : UMX_TRUE_PEAK_OFF;
            if (c.true_peak != UMX_TRUE_PEAK_OFF && not_offered)
            {
                fprintf(stderr, "UMX_TRUE_PEAK: %s (nor the true peak)\n", not_offered);
                return false;
            }
            if (c.true_peak == UMX_TRUE_PEAK_RESCALE && c.clip_mode != UMX_CLIP_RESCALE)
            {
                fprintf(stderr, "UMX_TRUE_PEAK=rescale: needs UMX_CLIP=rescale (it says which peak the divisor comes from)\n");
                return false;
            }
        }
    return true;
}

// the line of output m of a track, written to `file`
inline void umx_levels_print(const char *file, const umx_levels &lv, int m)
{
    printf("levels %s peak=%.9g over_unity=%llu clipped=%llu nonfinite=%llu gain=%.9g\n", file, (double)lv.peak[m], lv.over_unity[m], lv.clipped[m],
           lv.nonfinite[m], (double)lv.gain);
}

// the loudness line of output m of a track, written to `file`
inline void umx_loudness_print(const char *file, const umx_loudness &ld, int m)
{
    auto lufs = [](double v, char *buf, size_t cap) { // (-inf by name: printf's spelling of it is the C library's)
        if (std::isinf(v))
            snprintf(buf, cap, v < 0 ? "-inf" : "inf");
        else
            snprintf(buf, cap, "%.6f", v);
    };
    char a[40], b[40];
    lufs(ld.integrated[m], a, sizeof a);
    lufs(ld.momentary_max[m], b, sizeof b);
    printf("loudness %s integrated=%s momentary_max=%s blocks=%lld gated=%lld\n", file, a, b, ld.blocks[m], ld.gated[m]);
}

// the true-peak line of output m of a track, written to `file`
inline void umx_true_peak_print(const char *file, const umx_true_peak &tp, int m)
{
    const double v = tp.true_peak[m];
    char a[40];
    if (v == 0 || std::isinf(v)) // (-inf by name, as the loudness line)
        snprintf(a, sizeof a, "%s", v == 0 ? "-inf" : "inf");
    else
        snprintf(a, sizeof a, "%.6f", 20.0 * std::log10(v));
    printf("true_peak %s dbtp=%s linear=%.9g factor=%d\n", file, a, v, tp.factor);
}
