// mix.cpp -- umx_mix_parse of include/umx_host.h: the UMX_MIX grammar of host/mix_env.h for callers of the library (the
// Python package, other front ends).  Host arithmetic only.
#include "../../include/umx_host.h"
#include "mix_env.h"

#include <cstring>

extern "C" int umx_mix_parse(const char *spec, int residual_slot, int *n_out, char *names, float *gains, char *err)
{
    umx_mix_choice c;
    std::string msg;
    if (!spec || !n_out || !names || !gains)
        msg = "UMX_MIX: need a specification and room for the result";
    else if (umx_mix_parse_spec(spec, residual_slot, c, msg))
    {
        *n_out = c.n_out;
        memset(names, 0, (size_t)UMX_MAX_MIX_OUTPUTS * UMX_MIX_NAME_LEN);
        for (int m = 0; m < c.n_out; ++m)
            memcpy(names + (size_t)m * UMX_MIX_NAME_LEN, c.name[m].c_str(), c.name[m].size()); // (at most 63 characters)
        memcpy(gains, c.gains, sizeof(c.gains));
        return 0;
    }
    if (err)
        snprintf(err, UMX_ERRLEN, "%s", msg.c_str());
    return UMX_ERR_ARG;
}
