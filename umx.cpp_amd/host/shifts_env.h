// shifts_env.h -- UMX_SHIFTS of umx-cli and umx-batch (Demucs' `--shifts`): how many time-shifted separations of a track are averaged
// (umx_hip_shift_ensemble).
//   UMX_SHIFTS=<1..64>   unset, empty or 1: one shift, the reference's behaviour
#pragma once
#include "../../include/umx_hip.h"

#include <cstdio>
#include <cstdlib>

// false (message on stderr, naming the variable) for a value that is no number or lies outside 1 .. UMX_MAX_SHIFTS
inline bool umx_shifts_from_env(int &shifts)
{
    shifts = 1;
    const char *v = getenv("UMX_SHIFTS");
    if (!v || !*v)
        return true;
    char *end = nullptr;
    const long k = strtol(v, &end, 10);
    if (end == v || *end || k < 1 || k > UMX_MAX_SHIFTS)
    {
        fprintf(stderr, "UMX_SHIFTS: need a number of shifts 1 .. %d, got \"%s\"\n", UMX_MAX_SHIFTS, v);
        return false;
    }
    shifts = (int)k;
    return true;
}
