// tools/flac_in_fuzz.cpp -- the host side of csrc/flac_decode.h under AddressSanitizer and UBSan.  The host decoder and the
// kernels share the parse functions, so an unbounded read shows here, without a GPU.  A stand-alone program, nothing of it is loaded
// into Python:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I include -I umx.cpp_amd/csrc -o flac_in_fuzz tools/flac_in_fuzz.cpp
//   ./flac_in_fuzz [stream.flac ...]
// Without arguments it encodes streams of its own (16 and 24 bits, FIXED and LPC).  Every stream is decoded as it is, cut short at
// 64 lengths, and with `ROUNDS` single-byte corruptions (a random byte XORed with a random nonzero value).  It prints how many decodes
// were accepted and refused; it ends clean or the sanitizer ends it.
#include "umx_hip.h"
#include "sample_format.h"
#include "pcm16.h"
#include "pcm24.h"
#include "levels.h"
#include "flac_decode.h"
#include <cstdio>
#include <random>

using namespace umx;

static const int ROUNDS = 4000;
static long accepted = 0, refused = 0;

static void decode(const std::vector<uint8_t> &bytes)
{
    // (an exact-size copy, so that a read past the stream is a read past an allocation)
    std::vector<uint8_t> held(bytes);
    umx_flac_info info = {};
    if (flac_probe(held.data(), held.size(), info) != FLAC_IN_OK || info.n_frames > (1ll << 24))
    {
        ++refused;
        return;
    }
    std::vector<float> x(2 * (size_t)info.n_frames);
    long long frame = 0;
    (flac_decode_host(held.data(), held.size(), info, x.data(), &frame) == FLAC_IN_OK ? accepted : refused) += 1;
}

static void torture(const std::vector<uint8_t> &good, std::mt19937 &rng)
{
    const long before = accepted;
    decode(good);
    if (accepted != before + 1)
    {
        std::printf("a stream of %zu bytes does not decode as it is\n", good.size());
        std::exit(2);
    }
    for (int k = 1; k <= 64; ++k)
        decode(std::vector<uint8_t>(good.begin(), good.begin() + (size_t)((double)good.size() * k / 65.0)));
    for (int k = 0; k < ROUNDS; ++k)
    {
        std::vector<uint8_t> bad(good);
        bad[rng() % bad.size()] ^= (uint8_t)(1 + rng() % 255);
        decode(bad);
    }
}

int main(int argc, char **argv)
{
    std::mt19937 rng(20240531);
    for (int i = 1; i < argc; ++i)
    {
        std::vector<uint8_t> bytes;
        if (FILE *f = std::fopen(argv[i], "rb"))
        {
            for (int c; (c = std::fgetc(f)) != EOF;)
                bytes.push_back((uint8_t)c);
            std::fclose(f);
        }
        if (bytes.empty())
        {
            std::printf("%s: cannot read\n", argv[i]);
            return 2;
        }
        torture(bytes, rng);
    }
    for (int bits : {16, 24})
        for (int lpc : {0, 12})
        {
            if (argc > 1)
                break;
            const long long n = 2 * 4096 + 17;
            std::vector<float> x(2 * n);
            for (long long i = 0; i < n; ++i)
            {
                x[2 * i] = 0.4f * std::sin(0.43f * i) + 0.01f * ((int)(rng() % 2001) - 1000) / 1000.f;
                x[2 * i + 1] = i < 4096 ? 0.25f : ((int)(rng() % 2001) - 1000) / 1000.f; // CONSTANT, then noise
            }
            std::vector<uint8_t> out(flac_bound(n, bits));
            out.resize(bits == 16 ? flac_encode_host<SampleS16>(x.data(), n, 44100, 0, false, 0, lpc, out.data())
                                  : flac_encode_host<SampleS24>(x.data(), n, 44100, 0, false, 0, lpc, out.data()));
            torture(out, rng);
        }
    std::printf("flac_in_fuzz: %ld decodes accepted, %ld refused, no finding\n", accepted, refused);
    return 0;
}
