// targets_env.h -- UMX_TARGETS / UMX_RESIDUAL / UMX_SOFTMASK of umx-cli and umx-batch (Open-Unmix's `--targets`, `--residual` and
// `softmask`; the reference's CLI always writes all four stems, umx.cpp:75-96): which targets run, whether one more stem holds the
// rest of the mix, and how the first estimates are formed.
//   UMX_TARGETS=<comma list of bass,drums,other,vocals>   the active targets (default: all four)
//   UMX_RESIDUAL=1                                        the residual source (UMX_FLAG_RESIDUAL) -> residual.wav
//   UMX_SOFTMASK=1                                        first estimates X g_j / (eps + sum g) (UMX_FLAG_SOFTMASK); same files
// Written: target_<t>.wav for every active target and residual.wav; nothing for a silent slot.
#pragma once
#include "../../include/umx_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

struct umx_target_choice
{
    unsigned flags = 0;        // UMX_FLAG_SKIP_TARGET of the targets left out, UMX_FLAG_RESIDUAL, UMX_FLAG_SOFTMASK
    bool write[4] = {};        // the slot holds a stem to write ...
    std::string file[4];       // ... under this name
};

// false (message on stderr, naming the variable) for an unknown name, an empty list, or a residual with all four or no targets
inline bool umx_targets_from_env(umx_target_choice &c)
{
    static const char *const names[4] = {"bass", "drums", "other", "vocals"}; // convert-umx-pth-to-ggml.py:104
    bool active[4] = {true, true, true, true};
    const char *list = getenv("UMX_TARGETS");
    if (list)
    {
        for (bool &a : active)
            a = false;
        const std::string s = list;
        for (size_t i = 0; i <= s.size();) // (an empty list is one empty name: refused below)
        {
            const size_t e = std::min(s.find(',', i), s.size());
            const std::string tok = s.substr(i, e - i);
            int t = 0;
            while (t < 4 && tok != names[t])
                ++t;
            if (t == 4)
            {
                fprintf(stderr, "UMX_TARGETS: need a comma list of bass,drums,other,vocals; got \"%s\" in \"%s\"\n", tok.c_str(), list);
                return false;
            }
            active[t] = true;
            i = e + 1;
        }
    }
    const char *rv = getenv("UMX_RESIDUAL");
    const bool residual = rv && *rv && atoi(rv) != 0;
    int nact = 0;
    for (int t = 0; t < 4; ++t)
    {
        nact += active[t];
        if (!active[t])
            c.flags |= UMX_FLAG_SKIP_TARGET(t);
        c.write[t] = active[t];
        c.file[t] = "target_" + std::to_string(t) + ".wav";
    }
    if (residual)
    {
        c.flags |= UMX_FLAG_RESIDUAL;
        const int r = umx_hip_residual_slot(c.flags);
        if (r < 0)
        {
            fprintf(stderr, "UMX_RESIDUAL=1: needs UMX_TARGETS with one to three of the four targets (%d selected): the residual takes the "
                            "place of a target that does not run\n", nact);
            return false;
        }
        c.write[r] = true;
        c.file[r] = "residual.wav";
    }
    const char *sv = getenv("UMX_SOFTMASK");
    if (sv && *sv && atoi(sv) != 0)
        c.flags |= UMX_FLAG_SOFTMASK;
    return true;
}
