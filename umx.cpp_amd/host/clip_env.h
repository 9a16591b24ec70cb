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

// One of the switches above: unset or empty leaves `value` alone, "0" / "1" (and, where `third` names one, that word) set it to 0 / 1
// / 2; false, with a message that names the variable, for anything else
inline bool umx_switch_parse(const char *name, const char *text, const char *third, int &value, std::string &err)
{
    if (!text || !*text)
        return true;
    if (strcmp(text, "0") && strcmp(text, "1") && !(third && !strcmp(text, third)))
    {
        err = std::string(name) + ": need 0" + (third ? std::string(", 1 or ") + third : std::string(" or 1")) + ", got \"" + text + "\"";
        return false;
    }
    value = text[0] == '0' ? 0 : text[0] == '1' ? 1 : 2;
    return true;
}

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
    int on = 0;
    if (!umx_switch_parse("UMX_LEVELS", levels, nullptr, on, err))
        return false;
    c.levels = on != 0;
    return true;
}

// false: refused, message on stderr.  not_offered: the reason this run cannot take the two (nullptr: it can).  The variables are read
// in this order, each parsed and then refused where the run cannot offer it: UMX_CLIP and UMX_LEVELS, UMX_LOUDNESS, UMX_TRUE_PEAK.
inline bool umx_clip_from_env(umx_clip_choice &c, const char *not_offered)
{
    auto refuse = [](const std::string &why) {
        fprintf(stderr, "%s\n", why.c_str());
        return false;
    };
    const std::string no = not_offered ? not_offered : "";
    std::string err;
    int loud = 0, tp = 0;
    if (!umx_clip_parse(getenv("UMX_CLIP"), getenv("UMX_LEVELS"), c, err))
        return refuse(err);
    if (c.active() && not_offered)
        return refuse("UMX_CLIP / UMX_LEVELS: " + no);
    if (!umx_switch_parse("UMX_LOUDNESS", getenv("UMX_LOUDNESS"), nullptr, loud, err))
        return refuse(err);
    c.loudness = loud != 0;
    if (c.loudness && not_offered)
        return refuse("UMX_LOUDNESS: " + no + " (nor loudness)");
    if (!umx_switch_parse("UMX_TRUE_PEAK", getenv("UMX_TRUE_PEAK"), "rescale", tp, err))
        return refuse(err);
    c.true_peak = tp == 2 ? UMX_TRUE_PEAK_RESCALE : tp == 1 ? UMX_TRUE_PEAK_MEASURE : UMX_TRUE_PEAK_OFF;
    if (c.true_peak != UMX_TRUE_PEAK_OFF && not_offered)
        return refuse("UMX_TRUE_PEAK: " + no + " (nor the true peak)");
    if (c.true_peak == UMX_TRUE_PEAK_RESCALE && c.clip_mode != UMX_CLIP_RESCALE)
        return refuse("UMX_TRUE_PEAK=rescale: needs UMX_CLIP=rescale (it says which peak the divisor comes from)");
    return true;
}

// what a run measured of one track: the records its choice asked for are filled
struct umx_measured
{
    umx_levels levels = {};
    umx_loudness loudness = {};
    umx_true_peak true_peak = {};
};

// the lines of output m of a track, written to `file`, that the run asked for: levels, loudness, true peak
inline void umx_measured_print(const char *file, const umx_clip_choice &c, const umx_measured &rec, int m)
{
    auto named = [](double v, bool none, char *buf, size_t cap) { // (-inf by name: printf's spelling of it is the C library's)
        if (none || std::isinf(v))
            snprintf(buf, cap, "%s", none || v < 0 ? "-inf" : "inf");
        else
            snprintf(buf, cap, "%.6f", v);
    };
    char a[40], b[40];
    if (c.levels)
    {
        const umx_levels &lv = rec.levels;
        printf("levels %s peak=%.9g over_unity=%llu clipped=%llu nonfinite=%llu gain=%.9g\n", file, (double)lv.peak[m], lv.over_unity[m], lv.clipped[m],
               lv.nonfinite[m], (double)lv.gain);
    }
    if (c.loudness)
    {
        const umx_loudness &ld = rec.loudness;
        named(ld.integrated[m], false, a, sizeof a);
        named(ld.momentary_max[m], false, b, sizeof b);
        printf("loudness %s integrated=%s momentary_max=%s blocks=%lld gated=%lld\n", file, a, b, ld.blocks[m], ld.gated[m]);
    }
    if (c.true_peak != UMX_TRUE_PEAK_OFF)
    {
        const double v = rec.true_peak.true_peak[m];
        named(20.0 * std::log10(v), v == 0, a, sizeof a); // (a true peak of 0: -inf dBTP)
        printf("true_peak %s dbtp=%s linear=%.9g factor=%d\n", file, a, v, rec.true_peak.factor);
    }
}
