// quant_planes_check.cpp -- a stand-alone check of csrc/quant_planes.h (host code: no GPU, no HIP runtime), meant to be built with the
// address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/quant_planes_check.cpp -o quant_planes_check
// Every buffer is a heap allocation of exactly the size the engine's load_weight gives quant_planes, so that a write past a
// plane, a row or the padding is a sanitizer report.  What it runs:
//   * u8 and u16 tensors into matrices with padded columns (cols_pad > cols): planes exact, padding untouched;
//   * a two-source matrix (W_ih: forward and reverse tensor stacked) with a row permutation and rows nothing maps to, each source
//     with its own centre;
//   * degenerate scales and offsets (0, -0, inf, nan): the centre stays 128 / 32896;
//   * centres at both clamps (u8 0 and 255, u16 31 and 65504) with every code 0 .. 65535: every plane value finite.
// Exit status 0 and "quant_planes_check: ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../umx.cpp_amd/csrc/quant_planes.h"

using namespace umx;

static int failures = 0;
#define CHECK(cond)                                                      \
    do                                                                   \
    {                                                                    \
        if (!(cond))                                                     \
        {                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static const unsigned short UNTOUCHED = 0; // the caller's zeros

// nsrc source tensors of rows x cols codes -> one matrix [nsrc * dst_rows][cols_pad] per plane, as load_weight lays it out
static void run_matrix(int esz, int nsrc, int rows, int cols, int dst_rows, int cols_pad, const std::vector<int> *dst_row, const float *s, const float *o,
                       const int *want_c, std::mt19937 &rng)
{
    const size_t n = (size_t)nsrc * dst_rows * cols_pad;
    std::vector<unsigned short> planes((size_t)esz * n, UNTOUCHED);
    std::vector<std::vector<unsigned char>> q(nsrc);
    QuantCentre qc[2];
    for (int k = 0; k < nsrc; ++k)
    {
        q[k].resize((size_t)rows * cols * esz);
        for (unsigned char &b : q[k])
            b = (unsigned char)(rng() & 255u);
        unsigned short *hi = planes.data() + (size_t)k * dst_rows * cols_pad;
        qc[k] = quant_planes(q[k].data(), esz, rows, cols, dst_row ? dst_row->data() : nullptr, (size_t)cols_pad, s[k], o[k], hi, esz == 2 ? hi + n : nullptr);
        CHECK(qc[k].c == want_c[k]);
        const float o2 = (float)((double)o[k] + (double)qc[k].c * (double)s[k]);
        CHECK(std::memcmp(&o2, &qc[k].o2, 4) == 0);
    }
    std::vector<char> mapped((size_t)nsrc * dst_rows, 0);
    for (int k = 0; k < nsrc; ++k)
        for (int r = 0; r < rows; ++r)
        {
            const size_t row = (size_t)k * dst_rows + (dst_row ? (*dst_row)[r] : r);
            mapped[row] = 1;
            for (int j = 0; j < cols_pad; ++j)
            {
                const size_t i = row * cols_pad + j;
                if (j >= cols)
                {
                    CHECK(planes[i] == UNTOUCHED && (esz == 1 || planes[n + i] == UNTOUCHED));
                    continue;
                }
                unsigned code = q[k][((size_t)r * cols + j) * esz];
                if (esz == 2)
                    code |= (unsigned)q[k][((size_t)r * cols + j) * 2 + 1] << 8; // little endian, as the file and the engine's hosts are
                const double hi = f16_bits_to_float(planes[i]), lo = esz == 2 ? f16_bits_to_float(planes[n + i]) : 0.0;
                CHECK(std::isfinite(hi) && std::isfinite(lo));
                CHECK(hi + lo == (double)code - qc[k].c);
                CHECK(std::fabs(lo) <= 16.0 && std::fabs(lo) <= std::ldexp(std::fabs(hi), -11));
            }
        }
    for (size_t row = 0; row < mapped.size(); ++row)
        if (!mapped[row])
            for (int j = 0; j < cols_pad; ++j)
                CHECK(planes[row * cols_pad + j] == UNTOUCHED && (esz == 1 || planes[n + row * cols_pad + j] == UNTOUCHED));
}

int main()
{
    std::mt19937 rng(1);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    // padded columns, one source: u8 (zero-weight code 35) and u16 (9039)
    {
        const float s8 = 0.01f, o8 = -0.35f, s16 = 1e-4f, o16 = -0.9039f;
        const int c8 = 35, c16 = 9039;
        run_matrix(1, 1, 5, 7, 5, 32, nullptr, &s8, &o8, &c8, rng);
        run_matrix(2, 1, 5, 7, 5, 32, nullptr, &s16, &o16, &c16, rng);
        run_matrix(1, 1, 3, 32, 3, 32, nullptr, &s8, &o8, &c8, rng); // no padding at all: the last write is the buffer's last element
        run_matrix(2, 1, 3, 32, 3, 32, nullptr, &s16, &o16, &c16, rng);
    }
    // two sources, a row permutation into 16 destination rows of which 12 are mapped (fc3 leaves such rows too); each source its centre
    {
        std::vector<int> perm = {13, 2, 7, 0, 15, 4, 9, 6, 11, 1, 8, 3};
        const float s[2] = {0.02f, 0.005f}, o[2] = {-0.7f, -0.99f};
        const int c[2] = {35, 198};
        run_matrix(1, 2, 12, 10, 16, 32, &perm, s, o, c, rng);
        const float s2[2] = {2e-4f, 1e-4f}, o2[2] = {-1.8078f, -5.0971f};
        const int c2[2] = {9039, 50971};
        run_matrix(2, 2, 12, 10, 16, 32, &perm, s2, o2, c2, rng);
    }
    // degenerate scales and offsets keep the middle of the range
    for (int esz = 1; esz <= 2; ++esz)
    {
        const int mid = esz == 1 ? 128 : 32896;
        const float bad[][2] = {{0.f, 1.f}, {-0.f, 1.f}, {inf, 1.f}, {-inf, 1.f}, {nan, 1.f}, {0.5f, inf}, {0.5f, -inf}, {0.5f, nan}};
        for (const auto &p : bad)
        {
            CHECK(quant_centre(p[0], p[1], esz).c == mid);
            unsigned char q[4] = {0, 255, 7, 200};
            unsigned short hi[2], lo[2];
            const QuantCentre qc = quant_planes(q, esz, 1, 2, nullptr, 2, p[0], p[1], hi, esz == 2 ? lo : nullptr);
            CHECK(qc.c == mid);
        }
        CHECK(quant_centre(0.f, 1.f, esz).o2 == 1.f);
    }
    // both clamps, every code: plane values finite and exact
    {
        const float one = 1.f;
        struct { int esz; float o; int c; } clamps[] = {{1, 10.f, 0}, {1, -1000.f, 255}, {1, 0.f, 0}, {1, -255.f, 255},
                                                        {2, 5.f, 31}, {2, -31.f, 31}, {2, -70000.f, 65504}, {2, -65504.f, 65504}, {2, -65504.5f, 65504}, {2, -30.5f, 31}};
        for (const auto &cl : clamps)
        {
            const int ncodes = cl.esz == 1 ? 256 : 65536;
            std::vector<unsigned char> q((size_t)ncodes * cl.esz);
            for (int v = 0; v < ncodes; ++v)
            {
                q[(size_t)v * cl.esz] = (unsigned char)(v & 255);
                if (cl.esz == 2)
                    q[(size_t)v * 2 + 1] = (unsigned char)(v >> 8);
            }
            std::vector<unsigned short> hi(ncodes), lo(cl.esz == 2 ? ncodes : 0);
            const QuantCentre qc = quant_planes(q.data(), cl.esz, 1, ncodes, nullptr, (size_t)ncodes, one, cl.o, hi.data(), cl.esz == 2 ? lo.data() : nullptr);
            CHECK(qc.c == cl.c);
            for (int v = 0; v < ncodes; ++v)
            {
                const double h = f16_bits_to_float(hi[v]), l = cl.esz == 2 ? f16_bits_to_float(lo[v]) : 0.0;
                CHECK(std::isfinite(h) && h + l == (double)v - qc.c && std::fabs(l) <= 16.0);
            }
        }
        // the clamp keeps |q - c| <= 65504, the largest finite fp16; the rounding reaches infinity at |q - c| = 65520 (c = 15 / 65520)
        CHECK(!std::isfinite(f16_bits_to_float(f16_rne_bits(65535.f - 15.f))) && !std::isfinite(f16_bits_to_float(f16_rne_bits(-65520.f))));
        CHECK(std::isfinite(f16_bits_to_float(f16_rne_bits(65535.f - 31.f))) && std::isfinite(f16_bits_to_float(f16_rne_bits(-65504.f))));
    }
    if (failures)
    {
        std::printf("quant_planes_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("quant_planes_check: ok\n");
    return 0;
}
