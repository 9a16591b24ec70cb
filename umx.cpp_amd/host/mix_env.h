// mix_env.h -- UMX_MIX of umx-cli and umx-batch (Open-Unmix's `--aggregate`, Demucs' `--two-stems`): which weighted sums of the
// stems and of the input mixture are written instead of the four stems (the stem mix matrix; include/umx_hip.h).
//   UMX_MIX="vocals=vocals;accompaniment=bass+drums+other;karaoke=mix-vocals;quiet=mix-0.5*vocals"
// Outputs are separated by `;`, each `name=expr` (1 .. 4 of them, written as <name>.wav); expr is a sequence of signed terms
// [+|-][<number>*]<source> (the first sign may be left out), source = bass | drums | other | vocals | mix | residual.  `residual`
// stands for the slot the residual source takes (UMX_RESIDUAL=1, umx_hip_residual_slot); without one it is refused.  A source may
// appear once per expression; names match [A-Za-z0-9_-]{1,63} and are unique.  Blanks are ignored.  <number> is a decimal literal
// (digits, one '.', an exponent), rounded to the nearest float; hex, inf / nan, an overflow and a nonzero literal that rounds to zero
// are refused.
// The parser is also exported from libumx_host.so as umx_mix_parse (include/umx_host.h, host/mix.cpp).
#pragma once
#include "../../include/umx_hip.h"

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

struct umx_mix_choice
{
    int n_out = 0;
    std::string name[UMX_MAX_MIX_OUTPUTS];
    float gains[UMX_MAX_MIX_OUTPUTS * UMX_MIX_COLUMNS] = {}; // gains[m * 5 + c], as umx_hip_separate_tracks_mix takes them
};

// false, with a message that names UMX_MIX and the offending piece, for anything outside the grammar above
inline bool umx_mix_parse_spec(const char *spec_in, int residual_slot, umx_mix_choice &c, std::string &err)
{
    static const char *const sources[6] = {"bass", "drums", "other", "vocals", "mix", "residual"}; // columns 0 .. 4, then the residual's slot
    c = umx_mix_choice();
    std::string spec;
    for (const char *p = spec_in ? spec_in : ""; *p; ++p)
        if (*p != ' ' && *p != '\t')
            spec += *p;
    auto fail = [&](const std::string &what, const std::string &piece) {
        err = "UMX_MIX: " + what + " \"" + piece + "\"";
        return false;
    };
    if (spec.empty())
        return fail("need 1 .. 4 outputs name=expr separated by ';', got", spec);
    for (size_t i = 0; i <= spec.size();)
    {
        const size_t e = std::min(spec.find(';', i), spec.size());
        const std::string piece = spec.substr(i, e - i);
        i = e + 1;
        const size_t eq = piece.find('=');
        if (eq == std::string::npos)
            return fail("an output is name=expr, got", piece);
        const std::string name = piece.substr(0, eq), expr = piece.substr(eq + 1);
        bool good = !name.empty() && name.size() <= 63;
        for (char ch : name)
            good = good && ((ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || (ch >= '0' && ch <= '9') || ch == '_' || ch == '-');
        if (!good)
            return fail("an output's name is 1 .. 63 characters of A-Z a-z 0-9 _ -, got", name);
        for (int m = 0; m < c.n_out; ++m)
            if (c.name[m] == name)
                return fail("output named twice:", name);
        if (c.n_out == UMX_MAX_MIX_OUTPUTS)
            return fail("at most 4 outputs; one too many:", piece);
        if (expr.empty())
            return fail("empty expression in", piece);
        float *row = c.gains + c.n_out * UMX_MIX_COLUMNS;
        bool seen[UMX_MIX_COLUMNS] = {};
        for (size_t k = 0; k < expr.size();)
        {
            float sign = 1.0f;
            if (expr[k] == '+' || expr[k] == '-')
                sign = expr[k++] == '-' ? -1.0f : 1.0f;
            else if (k > 0)
                return fail("terms are joined by + or -, in", piece);
            float gain = 1.0f;
            if (k < expr.size() && ((expr[k] >= '0' && expr[k] <= '9') || expr[k] == '.'))
            {
                // <number> is decimal: digits[.digits][e[+|-]digits] or .digits[...] and nothing else (no hex, no inf / nan, no
                // locale: std::from_chars), read to the nearest float; one that overflows, or is not zero as written but rounds
                // to zero (the term would vanish without a word), is refused
                auto digit = [&](size_t i) { return i < expr.size() && expr[i] >= '0' && expr[i] <= '9'; };
                size_t stop = k;
                bool digits = false, nonzero = false;
                for (; digit(stop); ++stop, digits = true)
                    nonzero = nonzero || expr[stop] != '0';
                if (stop < expr.size() && expr[stop] == '.')
                    for (++stop; digit(stop); ++stop, digits = true)
                        nonzero = nonzero || expr[stop] != '0';
                if (digits && stop < expr.size() && (expr[stop] == 'e' || expr[stop] == 'E'))
                {
                    const size_t e0 = stop + 1 + (stop + 1 < expr.size() && (expr[stop + 1] == '+' || expr[stop + 1] == '-'));
                    if (digit(e0))
                        for (stop = e0; digit(stop); ++stop)
                            ;
                }
                const std::from_chars_result r = std::from_chars(expr.data() + k, expr.data() + stop, gain);
                if (!digits || stop >= expr.size() || expr[stop] != '*' || r.ec != std::errc() || r.ptr != expr.data() + stop ||
                    !std::isfinite(gain) || (nonzero && gain == 0.0f))
                    return fail("bad number (want <decimal number>*<source>, finite and not rounding to zero) in", piece);
                k = stop + 1;
            }
            size_t w = k;
            while (w < expr.size() && expr[w] != '+' && expr[w] != '-')
                ++w;
            const std::string src = expr.substr(k, w - k);
            k = w;
            int col = 0;
            while (col < 6 && src != sources[col])
                ++col;
            if (col == 6)
                return fail(src.empty() ? std::string("a term without a source in") : "unknown source \"" + src + "\" (bass, drums, other, vocals, mix, residual) in", piece);
            if (col == 5)
            {
                if (residual_slot < 0 || residual_slot > 3)
                    return fail("there is no residual source (UMX_RESIDUAL=1 with UMX_TARGETS) for", piece);
                col = residual_slot;
            }
            if (seen[col])
                return fail("source \"" + src + "\" named twice in", piece);
            seen[col] = true;
            row[col] = sign * gain;
        }
        c.name[c.n_out++] = name;
    }
    return true;
}

// 0: UMX_MIX is unset or empty (today's path); 1: parsed into c; -1: refused, message on stderr
inline int umx_mix_from_env(umx_mix_choice &c, int residual_slot)
{
    const char *v = getenv("UMX_MIX");
    if (!v || !*v)
        return 0;
    std::string err;
    if (!umx_mix_parse_spec(v, residual_slot, c, err))
    {
        fprintf(stderr, "%s\n", err.c_str());
        return -1;
    }
    return 1;
}

// a stem column of the matrix whose slot holds nothing (`write` of host/targets_env.h: its target does not run and it is not the
// residual's slot): its name, or nullptr
inline const char *umx_mix_silent_source(const umx_mix_choice &c, const bool write[4])
{
    static const char *const names[4] = {"bass", "drums", "other", "vocals"};
    for (int m = 0; m < c.n_out; ++m)
        for (int t = 0; t < 4; ++t)
            if (c.gains[m * UMX_MIX_COLUMNS + t] != 0.0f && !write[t])
                return names[t];
    return nullptr;
}
