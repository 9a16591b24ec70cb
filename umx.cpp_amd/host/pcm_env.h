// pcm_env.h -- UMX_PCM16, UMX_PCM24 and their _DITHER of umx-cli and umx-batch: integer PCM across PCIe and in the files written
// (include/umx_hip.h), and the integer buffers of both programs behind one int16 pointer plus the format.
//   UMX_PCM16=1 / UMX_PCM24=1     every output a 16-bit / 24-bit PCM WAV quantised on the device; not both in one run
//   UMX_PCM16_DITHER=<seed> / UMX_PCM24_DITHER=<seed>   TPDF dither with that seed; needs its format
#pragma once
#include "../../include/umx_host.h"

#include <cstdio>
#include <cstdlib>

struct umx_pcm_choice
{
    umx_sample_io io = {UMX_SAMPLE_F32, UMX_SAMPLE_F32, 0, 0}; // out_format, dither and dither_seed from the environment; in_format is the caller's
    bool pcm16 = false, pcm24 = false;
    bool active() const { return pcm16 || pcm24; }
};

// false: refused, message on stderr.  not_offered: why this run cannot take integer transfers (nullptr: it can), up to "... do not offer"
inline bool umx_pcm_from_env(umx_pcm_choice &c, const char *not_offered)
{
    auto on = [](const char *name) {
        const char *v = getenv(name);
        return v && *v && atoi(v) != 0;
    };
    c = umx_pcm_choice();
    c.pcm16 = on("UMX_PCM16");
    if (c.pcm16 && not_offered)
    {
        fprintf(stderr, "UMX_PCM16: %s 16-bit PCM transfers\n", not_offered);
        return false;
    }
    if (!c.pcm16 && getenv("UMX_PCM16_DITHER"))
    {
        fprintf(stderr, "UMX_PCM16_DITHER: needs UMX_PCM16=1\n");
        return false;
    }
    c.pcm24 = on("UMX_PCM24");
    if (c.pcm24 && c.pcm16)
    {
        fprintf(stderr, "UMX_PCM24: does not go with UMX_PCM16=1 (one output format per run)\n");
        return false;
    }
    if (c.pcm24 && not_offered)
    {
        fprintf(stderr, "UMX_PCM24: %s 24-bit PCM transfers\n", not_offered);
        return false;
    }
    if (!c.pcm24 && getenv("UMX_PCM24_DITHER"))
    {
        fprintf(stderr, "UMX_PCM24_DITHER: needs UMX_PCM24=1\n");
        return false;
    }
    c.io.out_format = c.pcm24 ? UMX_SAMPLE_S24 : c.pcm16 ? UMX_SAMPLE_S16 : UMX_SAMPLE_F32;
    if (const char *seed = getenv(c.pcm24 ? "UMX_PCM24_DITHER" : "UMX_PCM16_DITHER"))
    {
        c.io.dither = 1;
        c.io.dither_seed = (unsigned)strtoul(seed, nullptr, 0);
    }
    return true;
}

// int16 units of an integer frame (4 bytes of int16, 6 bytes of packed 24-bit PCM); 0 for fp32
inline size_t int_units(int format) { return format == UMX_SAMPLE_S24 ? 3 : format == UMX_SAMPLE_S16 ? 2 : 0; }
// a file in an integer format as it is, behind an int16 pointer (free: umx_wav_free_pcm16); audio == nullptr: the head alone
inline int load_int(int format, const char *path, int16_t **audio, int *n, int *ch, int *rate, char *err)
{
    if (format != UMX_SAMPLE_S24)
        return umx_wav_load_pcm16(path, audio, n, ch, rate, err);
    unsigned char *p = nullptr;
    const int rc = umx_wav_load_pcm24(path, audio ? &p : nullptr, n, ch, rate, err);
    if (audio)
        *audio = reinterpret_cast<int16_t *>(p);
    return rc;
}
// n frames of an integer format behind an int16 pointer, to a WAV of that format
inline int write_int(int format, const char *path, const int16_t *buf, int n, int rate, char *err)
{
    return format == UMX_SAMPLE_S24 ? umx_wav_write_pcm24_rate(path, reinterpret_cast<const unsigned char *>(buf), n, rate, err)
                                    : umx_wav_write_pcm16_rate(path, buf, n, rate, err);
}
