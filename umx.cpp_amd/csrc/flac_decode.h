// flac_decode.h -- FLAC in: a .flac file's bytes become the fp32 frames that the int16 / packed 24-bit upload of the same
// codes would have produced, decoded on the device.  Every rule of the bit stream is stated once below, in __host__ __device__
// functions that the host decoder (flac_decode_host) and the kernels both call:
//   probe      an optional ID3v2 tag, "fLaC", STREAMINFO first, every other metadata block skipped by its length (flac_probe, host only)
//   header     flac_parse_frame_header: sync 0xFFF8 (fixed block size), every block size and sample rate code, the reserved codes, the
//              UTF-8 frame number, the fields against STREAMINFO, number * max_block + block <= total, CRC-8
//   bits       FlacBits: an MSB-first window of up to 64 bits in registers, refilled by four bounds-checked byte loads.  A read beyond the
//              frame's limit yields zero bits and marks the reader; a unary run ends at the limit at the latest.
//   subframe   flac_sub_step: ONE sample of a subframe per call -- at sample 0 the subframe header (type, wasted bits), at sample
//              `order` the predictor (LPC precision, shift, coefficients) and the residual's method and partition order, at a partition's
//              first sample its parameter (or the escape width); CONSTANT, VERBATIM, FIXED 0-4, LPC 1-32 with 64-bit sums and an
//              arithmetic shift, RICE / RICE2.  The predictor history is a ring of 32 samples, the coefficients 32 words: the caller's
//              memory (flac_decode_host: arrays; the kernel: LDS), so that a frame's decode is the same loop over samples on both sides.
//   frame      flac_frame_close: zero bits to the byte, the CRC-16 field; the frame ends behind it
//   channels   flac_undo_assign (mid/side with the side's parity bit) and flac_code_to_float: decode() of sample_format.h's traits
// A frame is refused when it is longer than flac_frame_limit (twice its two VERBATIM subframes): that bounds what a false candidate
// or a damaged file can make a lane read.
//
// The kernels (launch_flac_decode; all on one stream, no host round trip):
//   clear      the counters
//   scan       a thread per byte position, tiles of 256 positions and a 16-byte halo staged in LDS; at FF F8 the whole header is parsed
//              and checked.  A position that passes is a CANDIDATE and gets a dense index (an atomic counter); it is not yet a frame:
//              a CRC-8 passes by chance once in 256 syncs, so the scan alone never decides.
//   decode     one lane per candidate, 64 candidates a wave, in lock-step by sample (a frame is sequential; the parallelism is the
//              thousands of frames).  A lane's bit window lives in registers, its history and coefficients in LDS ([32][64] words at a
//              pitch of 65: conflict-free by lane and by row).  Every 32 samples the wave stores the 64 lanes' history rings as full
//              128-byte rows: int32 into the candidate's row of the scratch, [candidate][2 channels as coded][max_block].
//   CRC-16     a wave per candidate over [start, end): 64 pieces of 132 bytes aligned to the frame's END, a piece per lane, combined
//              pairwise by the compile-time advance factors of flac.h; longer frames chunk by chunk.  The CRC over a frame and its own
//              CRC field is zero.  A candidate that parsed and whose CRC-16 holds is VALID, and is counted under its frame number.
//   tile       a thread per frame number: exactly one valid candidate, frame 0 at audio_offset, every frame where its predecessor ended;
//              the first number that fails goes to a word (atomic min)
//   output     a thread per sample: the assignment undone, the sample rule, float2 stores.  A stream that is not valid writes the
//              status word and nothing else.
// All stores are ordinary vector stores; no inline assembly.
#pragma once
#include "common.h"
#include "flac.h"
#include "sample_format.h"

namespace umx
{

constexpr int FLAC_IN_MIN_BLOCK = 16, FLAC_IN_MAX_BLOCK = 16384, FLAC_IN_MAX_ORDER = 32, FLAC_IN_THREADS = 256, FLAC_IN_HALO = 16;
constexpr unsigned FLAC_IN_NONE = 0xffffffffu;

// what a stream or a frame is refused for (flac_reason)
enum
{
    FLAC_IN_OK = 0,
    FLAC_IN_SHORT,
    FLAC_IN_MARKER,
    FLAC_IN_STREAMINFO,
    FLAC_IN_VARIABLE,
    FLAC_IN_CHANNELS,
    FLAC_IN_BITS,
    FLAC_IN_TOTAL,
    FLAC_IN_BLOCK,
    FLAC_IN_RATE,
    FLAC_IN_METADATA,
    FLAC_IN_SYNC,
    FLAC_IN_RESERVED,
    FLAC_IN_MISMATCH,
    FLAC_IN_NUMBER,
    FLAC_IN_CRC8,
    FLAC_IN_SUBFRAME,
    FLAC_IN_CRC16
};
inline const char *flac_reason(int r)
{
    static const char *const text[] = {"ok",
                                       "the stream ends early",
                                       "no fLaC marker",
                                       "the first metadata block must be STREAMINFO (34 bytes)",
                                       "variable-blocksize streams are not supported (sync 0xFFF9)",
                                       "only 2-channel streams are supported",
                                       "only 16 and 24 bits per sample are supported",
                                       "the total sample count is unknown (0)",
                                       "block size outside 16 .. 16384, or minimum and maximum block size differ",
                                       "sample rate 0 or beyond 655350 Hz",
                                       "a metadata block runs beyond the stream",
                                       "no frame sync (0xFFF8)",
                                       "a reserved code in the frame header",
                                       "the frame header disagrees with STREAMINFO",
                                       "the frame number or block size does not fit the stream",
                                       "header CRC-8 mismatch",
                                       "a subframe does not parse",
                                       "frame CRC-16 mismatch"};
    return text[r];
}

__host__ __device__ inline int flac_in_blocks(long long n, int max_block) { return (int)((n + max_block - 1) / max_block); }
// the bytes a frame of bs frames may take here: twice its header, two VERBATIM subframes (one a bit wider) and the CRC-16
__host__ __device__ inline size_t flac_frame_limit(int bs, int bps) { return 2 * (size_t)(16 + (2 * 8 + bs * (2 * bps + 1) + 7) / 8 + 2) + 64; }
// candidates the scratch has room for
inline size_t flac_in_capacity(long long n, int max_block)
{
    const size_t nb = (size_t)flac_in_blocks(n, max_block);
    return nb + nb / 64 + 16;
}

// ---------------------------------------------------------------- probe (host)
inline int flac_probe(const uint8_t *p, size_t n, umx_flac_info &info)
{
    size_t at = 0;
    if (n >= 10 && p[0] == 'I' && p[1] == 'D' && p[2] == '3') // ID3v2: 10 bytes, a 28-bit synchsafe size, 10 more when a footer is flagged
    {
        const size_t size = ((size_t)(p[6] & 127) << 21) | ((size_t)(p[7] & 127) << 14) | ((size_t)(p[8] & 127) << 7) | (size_t)(p[9] & 127);
        at = 10 + size + ((p[5] & 0x10) ? 10 : 0);
    }
    if (at > n || n - at < 4)
        return FLAC_IN_SHORT;
    if (p[at] != 'f' || p[at + 1] != 'L' || p[at + 2] != 'a' || p[at + 3] != 'C')
        return FLAC_IN_MARKER;
    at += 4;
    if (n - at < 4 + 34)
        return FLAC_IN_SHORT;
    if ((p[at] & 127) != 0 || p[at + 1] != 0 || p[at + 2] != 0 || p[at + 3] != 34)
        return FLAC_IN_STREAMINFO;
    const uint8_t *s = p + at + 4;
    const int min_block = (s[0] << 8) | s[1], max_block = (s[2] << 8) | s[3];
    unsigned long long v = 0;
    for (int i = 10; i < 18; ++i)
        v = (v << 8) | s[i];
    info.rate = (int)(v >> 44);
    info.channels = (int)((v >> 41) & 7) + 1;
    info.bits = (int)((v >> 36) & 31) + 1;
    info.n_frames = (long long)(v & ((1ull << 36) - 1));
    info.max_block = max_block;
    bool last = (p[at] & 128) != 0;
    at += 4 + 34;
    while (!last)
    {
        if (n - at < 4)
            return FLAC_IN_METADATA;
        last = (p[at] & 128) != 0;
        const size_t len = ((size_t)p[at + 1] << 16) | ((size_t)p[at + 2] << 8) | p[at + 3];
        if (n - at - 4 < len)
            return FLAC_IN_METADATA;
        at += 4 + len;
    }
    info.audio_offset = (long long)at;
    if (info.channels != 2)
        return FLAC_IN_CHANNELS;
    if (info.bits != 16 && info.bits != 24)
        return FLAC_IN_BITS;
    if (info.n_frames == 0)
        return FLAC_IN_TOTAL;
    if (min_block != max_block || max_block < FLAC_IN_MIN_BLOCK || max_block > FLAC_IN_MAX_BLOCK)
        return FLAC_IN_BLOCK;
    if (!flac_rate_ok(info.rate))
        return FLAC_IN_RATE;
    // (a variable-blocksize stream says so in its first frame's sync)
    if (n - at >= 2 && p[at] == 0xff && p[at + 1] == 0xf9)
        return FLAC_IN_VARIABLE;
    return FLAC_IN_OK;
}
// what the entry points ask of a caller's info record before a kernel reads it
inline bool flac_info_ok(const umx_flac_info &i, size_t n_bytes)
{
    return i.channels == 2 && (i.bits == 16 || i.bits == 24) && i.n_frames >= 1 && i.n_frames <= 0x7fffffff / 2 && i.max_block >= FLAC_IN_MIN_BLOCK &&
           i.max_block <= FLAC_IN_MAX_BLOCK && flac_rate_ok(i.rate) && i.audio_offset >= 0 && (size_t)i.audio_offset <= n_bytes && n_bytes <= 0x7fffffffu;
}

// ---------------------------------------------------------------- the frame header
struct FlacFrameHead
{
    uint32_t number;
    int bs, assign /* 0 independent, 1 left/side, 2 side/right, 3 mid/side */, bytes /* with the CRC-8 */;
};
// get(i): byte i of the candidate, i < 16 (zero beyond the stream: the CRC-8 then fails or the frame does).  FLAC_IN_OK, or the reason.
template <class Get> __host__ __device__ inline int flac_parse_frame_header(const Get &get, const umx_flac_info &info, FlacFrameHead &h)
{
    if (get(0) != 0xff || (get(1) & 0xfe) != 0xf8)
        return FLAC_IN_SYNC;
    if (get(1) & 1)
        return FLAC_IN_VARIABLE;
    const int bcode = get(2) >> 4, rcode = get(2) & 15, ccode = get(3) >> 4, scode = (get(3) >> 1) & 7;
    if (bcode == 0 || rcode == 15 || (get(3) & 1) || scode == 3 || ccode > 10)
        return FLAC_IN_RESERVED;
    if (ccode != 1 && ccode < 8)
        return FLAC_IN_CHANNELS;
    const int sbits = scode == 0 ? info.bits : scode == 1 ? 8 : scode == 2 ? 12 : scode == 4 ? 16 : scode == 5 ? 20 : scode == 6 ? 24 : 32;
    if (sbits != info.bits)
        return FLAC_IN_MISMATCH;
    h.assign = ccode == 1 ? 0 : ccode - 7;
    int n = 4;
    const uint32_t lead = get(n++);
    int extra = 0;
    while (extra < 7 && (lead & (0x80u >> extra)))
        ++extra; // leading ones: 0 (one byte), 2 .. 6 (that many bytes); a fixed-blocksize number has 31 bits at most
    if (extra == 1 || extra > 6)
        return FLAC_IN_RESERVED;
    uint32_t num = extra ? lead & (0x7fu >> extra) : lead;
    for (int i = 1; i < extra; ++i)
    {
        const uint32_t c = get(n++);
        if ((c & 0xc0) != 0x80)
            return FLAC_IN_RESERVED;
        num = (num << 6) | (c & 0x3f);
    }
    h.number = num;
    int bs = bcode == 1 ? 192 : bcode <= 5 ? 576 << (bcode - 2) : bcode >= 8 ? 256 << (bcode - 8) : 0;
    if (bcode == 6)
        bs = (int)get(n++) + 1;
    else if (bcode == 7)
    {
        bs = (int)get(n) * 256 + (int)get(n + 1) + 1;
        n += 2;
    }
    h.bs = bs;
    const int table[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    int rate = rcode == 0 ? info.rate : rcode < 12 ? table[rcode] : 0;
    if (rcode == 12)
        rate = (int)get(n++) * 1000;
    else if (rcode == 13 || rcode == 14)
    {
        rate = ((int)get(n) * 256 + (int)get(n + 1)) * (rcode == 14 ? 10 : 1);
        n += 2;
    }
    if (rate != info.rate)
        return FLAC_IN_MISMATCH;
    // a fixed-blocksize stream: every frame max_block frames but the last, which holds the rest
    const long long first = (long long)num * info.max_block, rest = info.n_frames - first;
    if (rest < 1 || bs != (rest < info.max_block ? (int)rest : info.max_block))
        return FLAC_IN_NUMBER;
    uint32_t crc = 0;
    for (int i = 0; i < n; ++i)
    {
        crc ^= get(i);
        for (int b = 0; b < 8; ++b)
            crc = ((crc << 1) ^ ((crc & 0x80) ? 0x07u : 0u)) & 0xffu;
    }
    if (crc != get(n))
        return FLAC_IN_CRC8;
    h.bytes = n + 1;
    return FLAC_IN_OK;
}

// ---------------------------------------------------------------- the bit window
struct FlacBits
{
    const uint8_t *p;
    size_t pos, limit; // the next byte to load; reads at or beyond `limit` (<= the stream's bytes) give zero
    unsigned long long acc;
    int cnt; // valid bits, at the top of acc
    __host__ __device__ void open(const uint8_t *bytes, size_t at, size_t lim)
    {
        p = bytes;
        pos = at;
        limit = lim;
        acc = 0;
        cnt = 0;
    }
    __host__ __device__ void refill() // to more than 32 bits
    {
        if (cnt > 32)
            return;
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w = (w << 8) | (pos + i < limit ? (uint32_t)p[pos + i] : 0u);
        pos += 4;
        acc |= (unsigned long long)w << (32 - cnt);
        cnt += 32;
    }
    __host__ __device__ size_t bit() const { return pos * 8 - (size_t)cnt; } // the next bit's position in the stream
    __host__ __device__ bool over() const { return bit() > limit * 8; }      // consumed beyond the limit
    __host__ __device__ uint32_t u(int n) // 0 .. 32 bits
    {
        refill();
        const uint32_t v = n ? (uint32_t)(acc >> (64 - n)) : 0u;
        acc = n ? acc << n : acc;
        cnt -= n;
        return v;
    }
    __host__ __device__ int32_t s(int n) // 1 .. 32 bits, two's complement
    {
        const uint32_t v = u(n);
        return (int32_t)(v << (32 - n)) >> (32 - n);
    }
    // zeros in front of the next one bit, which is consumed; the run ends at the limit at the latest (then over() holds)
    __host__ __device__ uint32_t unary()
    {
        uint32_t q = 0;
        for (;;)
        {
            refill();
            const uint32_t top = (uint32_t)(acc >> 32);
            if (top)
            {
                const int z = __builtin_clz(top);
                acc <<= z + 1;
                cnt -= z + 1;
                return q + (uint32_t)z;
            }
            acc <<= 32;
            cnt -= 32;
            q += 32;
            if (over())
                return q;
        }
    }
};

// ---------------------------------------------------------------- a subframe, sample by sample
struct FlacSub
{
    int type, order, wasted, width, shift, pbits, psize, k, part_end;
    int32_t constant;
    bool escape, bad;
};
// M: the caller's memory of this subframe's lane: int32_t &hist(int k), k < 32; int32_t &coef(int j), j < 32
template <class M> __host__ __device__ inline void flac_sub_open(FlacSub &s, FlacBits &r, M &m, int bs)
{
    if (s.type == FLAC_LPC)
    {
        const int precision = (int)r.u(4) + 1;
        s.shift = r.s(5);
        s.bad |= precision == 16 || s.shift < 0;
        for (int j = 0; j < s.order; ++j)
            m.coef(j) = s.bad ? 0 : r.s(precision);
    }
    const int method = (int)r.u(2), porder = (int)r.u(4);
    s.pbits = 4 + method;
    s.psize = bs >> porder;
    s.part_end = 0;
    s.bad |= method > 1 || (s.psize << porder) != bs || s.psize < s.order || s.psize < 1;
}
__host__ __device__ inline void flac_sub_partition(FlacSub &s, FlacBits &r) // a partition's parameter, or its escape width
{
    s.k = (int)r.u(s.pbits);
    s.escape = s.k == (1 << s.pbits) - 1;
    if (s.escape)
        s.k = (int)r.u(5);
    s.part_end += s.psize;
}
// sample i of a subframe of bs samples, `width` bits wide as coded: the value, or 0 once the subframe is bad
template <class M> __host__ __device__ inline int32_t flac_sub_step(FlacSub &s, FlacBits &r, M &m, int i, int bs, int width)
{
    if (i == 0)
    {
        s = FlacSub{};
        s.bad = r.u(1) != 0;
        const int kind = (int)r.u(6);
        if (r.u(1))
            s.wasted = (int)r.unary() + 1;
        s.width = width - s.wasted;
        s.type = kind == 0 ? FLAC_CONSTANT : kind == 1 ? FLAC_VERBATIM : kind >= 8 && kind <= 12 ? FLAC_FIXED : kind >= 32 ? FLAC_LPC : -1;
        s.order = s.type == FLAC_FIXED ? kind - 8 : s.type == FLAC_LPC ? kind - 31 : 0;
        s.bad |= s.type < 0 || s.width < 1 || s.order > bs || r.over();
        if (!s.bad && s.type == FLAC_CONSTANT)
            s.constant = r.s(s.width);
    }
    if (s.bad)
        return 0;
    int32_t x;
    if (s.type == FLAC_CONSTANT)
        x = s.constant;
    else if (s.type == FLAC_VERBATIM || i < s.order)
        x = r.s(s.width);
    else
    {
        if (i == s.order)
            flac_sub_open(s, r, m, bs);
        while (!s.bad && i >= s.part_end)
            flac_sub_partition(s, r);
        if (s.bad)
            return 0;
        int32_t e;
        if (s.escape)
            e = s.k ? r.s(s.k) : 0;
        else
        {
            const unsigned long long q = r.unary();
            s.bad |= (q >> (32 - s.k)) != 0; // (k <= 30: the code (q << k) | low has 32 bits)
            const uint32_t c = ((uint32_t)q << s.k) | r.u(s.k);
            e = (int32_t)(c >> 1) ^ -(int32_t)(c & 1);
        }
        uint32_t pred;
        if (s.type == FLAC_FIXED)
        {
            const uint32_t h1 = (uint32_t)m.hist((i - 1) & 31), h2 = (uint32_t)m.hist((i - 2) & 31), h3 = (uint32_t)m.hist((i - 3) & 31),
                           h4 = (uint32_t)m.hist((i - 4) & 31);
            pred = s.order == 0 ? 0u : s.order == 1 ? h1 : s.order == 2 ? 2 * h1 - h2 : s.order == 3 ? 3 * h1 - 3 * h2 + h3 : 4 * h1 - 6 * h2 + 4 * h3 - h4;
        }
        else
        {
            long long sum = 0;
            for (int j = 0; j < s.order; ++j)
                sum += (long long)m.coef(j) * m.hist((i - 1 - j) & 31);
            pred = (uint32_t)(sum >> s.shift);
        }
        x = (int32_t)(pred + (uint32_t)e);
    }
    s.bad |= r.over();
    m.hist(i & 31) = x;
    return (int32_t)((uint32_t)x << s.wasted);
}
// behind a subframe's last sample: a predictor as long as the block still has its (empty) residual in the stream
template <class M> __host__ __device__ inline void flac_sub_close(FlacSub &s, FlacBits &r, M &m, int bs)
{
    if (!s.bad && (s.type == FLAC_FIXED || s.type == FLAC_LPC) && s.order == bs)
    {
        flac_sub_open(s, r, m, bs);
        if (!s.bad)
            flac_sub_partition(s, r);
    }
    s.bad |= r.over();
}
// the width of subframe c (0, 1) as coded, and behind both: zero bits to the byte and the CRC-16 field.  Returns the byte behind the frame, 0: bad.
__host__ __device__ inline int flac_sub_width(int bps, int assign, int c) { return bps + ((assign == 1 && c == 1) || (assign == 2 && c == 0) || (assign == 3 && c == 1) ? 1 : 0); }
__host__ __device__ inline size_t flac_frame_close(FlacBits &r)
{
    const int pad = (int)((8 - (r.bit() & 7)) & 7);
    const bool clean = r.u(pad) == 0;
    r.u(16);
    return clean && !r.over() ? r.bit() / 8 : 0;
}
// the two channels as coded -> left, right
__host__ __device__ inline void flac_undo_assign(int assign, int32_t a, int32_t b, int32_t &l, int32_t &rr)
{
    if (assign == 3)
    {
        const int32_t mid = (int32_t)(((uint32_t)a << 1) | ((uint32_t)b & 1u));
        l = (mid + b) >> 1;
        rr = (mid - b) >> 1;
    }
    else
    {
        l = assign == 2 ? a + b : a;
        rr = assign == 1 ? a - b : b;
    }
}
// the sample rule: the decode of sample_format.h's trait of that width
__host__ __device__ inline float flac_code_to_float(int32_t q, int bits) { return bits == 16 ? SampleS16::decode((int16_t)q) : SampleS24::decode(q); }

// ---------------------------------------------------------------- the host restatement
struct FlacHostMem
{
    int32_t h[32], c[32];
    int32_t &hist(int k) { return h[k]; }
    int32_t &coef(int j) { return c[j]; }
};
// (2, n) interleaved fp32 at x.  FLAC_IN_OK, or the reason with the frame it belongs to in *frame
inline int flac_decode_host(const uint8_t *p, size_t n_bytes, const umx_flac_info &info, float *x, long long *frame)
{
    const int nblocks = flac_in_blocks(info.n_frames, info.max_block);
    size_t at = (size_t)info.audio_offset;
    std::vector<int32_t> ch[2];
    for (int blk = 0; blk < nblocks; ++blk)
    {
        *frame = blk;
        FlacFrameHead h;
        const size_t start = at;
        if (start >= n_bytes)
            return FLAC_IN_SHORT;
        if (int why = flac_parse_frame_header([&](int i) { return start + i < n_bytes ? (uint32_t)p[start + i] : 0u; }, info, h))
            return why;
        if (h.number != (uint32_t)blk)
            return FLAC_IN_NUMBER;
        FlacBits r;
        r.open(p, start + h.bytes, std::min(n_bytes, start + flac_frame_limit(h.bs, info.bits)));
        FlacHostMem m;
        bool bad = false;
        for (int c = 0; c < 2; ++c)
        {
            FlacSub s;
            ch[c].resize(h.bs);
            for (int i = 0; i < h.bs; ++i)
                ch[c][i] = flac_sub_step(s, r, m, i, h.bs, flac_sub_width(info.bits, h.assign, c));
            flac_sub_close(s, r, m, h.bs);
            bad |= s.bad;
        }
        const size_t end = flac_frame_close(r);
        if (bad || !end)
            return r.over() ? FLAC_IN_SHORT : FLAC_IN_SUBFRAME;
        uint32_t crc = 0;
        for (size_t i = start; i < end; ++i)
            crc = flac_crc16_byte(crc, p[i]);
        if (crc)
            return FLAC_IN_CRC16;
        for (int i = 0; i < h.bs; ++i)
        {
            int32_t l, rr;
            flac_undo_assign(h.assign, ch[0][i], ch[1][i], l, rr);
            const size_t k = (size_t)blk * info.max_block + i;
            x[2 * k] = flac_code_to_float(l, info.bits);
            x[2 * k + 1] = flac_code_to_float(rr, info.bits);
        }
        at = end;
    }
    return FLAC_IN_OK;
}

// ---------------------------------------------------------------- the kernels
// the scratch of one decode, in words: [0] candidates found, [1] the first frame number that fails, [2 .. 4) spare; then per candidate
// its first byte, the byte behind it (0: bad) and number << 2 | assignment; per frame number its valid candidates and one of them; the samples
struct FlacInArgs
{
    const uint8_t *bytes;
    unsigned *ctrl, *cand_pos, *cand_end, *cand_meta, *nvalid, *chosen;
    int32_t *samples; // [candidate][2][max_block]
    float2 *out;
    unsigned *status;
    umx_flac_info info;
    unsigned n_bytes, cap;
    int nblocks;
};
inline size_t flac_in_scratch_words(long long n, int max_block)
{
    const size_t cap = flac_in_capacity(n, max_block), nb = (size_t)flac_in_blocks(n, max_block);
    return 4 + 3 * cap + 2 * nb + cap * 2 * (size_t)max_block;
}

__global__ __launch_bounds__(FLAC_IN_THREADS) void flac_in_clear_kernel(FlacInArgs a)
{
    const int i = blockIdx.x * FLAC_IN_THREADS + threadIdx.x;
    if (i < 4)
        a.ctrl[i] = i == 1 ? FLAC_IN_NONE : 0u;
    if (i < a.nblocks)
    {
        a.nvalid[i] = 0;
        a.chosen[i] = 0;
    }
}

__global__ __launch_bounds__(FLAC_IN_THREADS) void flac_in_scan_kernel(FlacInArgs a)
{
    __shared__ uint8_t tile[FLAC_IN_THREADS + FLAC_IN_HALO];
    const unsigned base = (unsigned)a.info.audio_offset + blockIdx.x * FLAC_IN_THREADS, t = threadIdx.x;
    for (unsigned i = t; i < FLAC_IN_THREADS + FLAC_IN_HALO; i += FLAC_IN_THREADS)
        tile[i] = base + i < a.n_bytes ? a.bytes[base + i] : (uint8_t)0;
    __syncthreads();
    if (base + t >= a.n_bytes || tile[t] != 0xff || tile[t + 1] != 0xf8)
        return;
    FlacFrameHead h;
    if (flac_parse_frame_header([&](int i) { return (uint32_t)tile[t + i]; }, a.info, h) != FLAC_IN_OK)
        return;
    const unsigned id = atomicAdd(&a.ctrl[0], 1u);
    if (id < a.cap)
        a.cand_pos[id] = base + t;
}

// a lane's history and coefficients: [32][64] words at a pitch of 65
struct FlacLaneMem
{
    int32_t *h, *c;
    int lane;
    __device__ int32_t &hist(int k) { return h[k * 65 + lane]; }
    __device__ int32_t &coef(int j) { return c[j * 65 + lane]; }
};

__global__ __launch_bounds__(64) void flac_in_decode_kernel(FlacInArgs a)
{
    __shared__ int32_t hist[32 * 65], coef[32 * 65];
    __shared__ int lane_bs[64], lane_wasted[64];
    const int lane = threadIdx.x;
    const unsigned ncand = min(a.ctrl[0], a.cap), id = blockIdx.x * 64 + lane;
    if (blockIdx.x * 64 >= ncand)
        return;
    const bool live = id < ncand;
    FlacFrameHead h = {};
    FlacBits r;
    r.open(a.bytes, 0, 0);
    bool bad = !live;
    if (live)
    {
        const unsigned start = a.cand_pos[id];
        bad = flac_parse_frame_header([&](int i) { return start + i < a.n_bytes ? (uint32_t)a.bytes[start + i] : 0u; }, a.info, h) != FLAC_IN_OK;
        const size_t lim = (size_t)start + flac_frame_limit(h.bs, a.info.bits);
        r.open(a.bytes, start + h.bytes, lim < a.n_bytes ? lim : (size_t)a.n_bytes);
    }
    const int bs = bad ? 0 : h.bs, mb = a.info.max_block;
    lane_bs[lane] = bs;
    int bsmax = bs;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        bsmax = max(bsmax, __shfl_xor(bsmax, d, 64));
    FlacLaneMem m{hist, coef, lane};
    __syncthreads();
    for (int c = 0; c < 2; ++c)
    {
        FlacSub s = {};
        const int width = flac_sub_width(a.info.bits, h.assign, c);
        for (int i0 = 0; i0 < bsmax; i0 += 32)
        {
            for (int i = i0; i < min(i0 + 32, bsmax); ++i)
                if (i < bs)
                    (void)flac_sub_step(s, r, m, i, bs, width); // (the sample goes to the lane's ring)
            // the ring holds what prediction needs, the value before the wasted bits return; what leaves is shifted by them
            lane_wasted[lane] = s.bad ? 0 : s.wasted;
            __syncthreads();
            // 64 rows of 32 samples: two rows an iteration, lanes 0 .. 31 one and lanes 32 .. 63 the next
            for (int it = 0; it < 32; ++it)
            {
                const int l = 2 * it + (lane >> 5), k = lane & 31;
                const unsigned cid = blockIdx.x * 64 + l;
                if (cid < ncand && i0 + k < lane_bs[l])
                    a.samples[((size_t)cid * 2 + c) * mb + i0 + k] = (int32_t)((uint32_t)hist[k * 65 + l] << lane_wasted[l]);
            }
            __syncthreads();
        }
        if (bs)
            flac_sub_close(s, r, m, bs);
        bad |= s.bad;
    }
    if (live)
    {
        const size_t end = bad ? 0 : flac_frame_close(r);
        a.cand_end[id] = (unsigned)end;
        a.cand_meta[id] = (h.number << 2) | (unsigned)h.assign;
    }
}

// a wave per candidate, four a workgroup: the CRC-16 over [start, end), and a valid candidate is filed under its number
__global__ __launch_bounds__(FLAC_IN_THREADS) void flac_in_crc_kernel(FlacInArgs a)
{
    __shared__ uint16_t crctab[256];
    const int t = threadIdx.x, lane = t & 63;
    {
        uint32_t c = (uint32_t)t << 8;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            c = ((c << 1) ^ ((c & 0x8000) ? 0x8005u : 0u)) & 0xffffu;
        crctab[t] = (uint16_t)c;
    }
    __syncthreads();
    const unsigned ncand = min(a.ctrl[0], a.cap), id = blockIdx.x * 4 + (t >> 6);
    if (id >= ncand)
        return;
    const unsigned start = a.cand_pos[id], end = min(a.cand_end[id], a.n_bytes);
    if (end <= start)
        return;
    constexpr int CHUNK = 64 * FLAC_CRC_PIECE;
    const int len = (int)(end - start), chunks = (len + CHUNK - 1) / CHUNK, lead = chunks * CHUNK - len; // `lead` zero bytes in front move nothing
    const uint8_t *__restrict__ p = a.bytes + start;
    uint32_t all = 0;
    for (int ck = 0; ck < chunks; ++ck)
    {
        const int r0 = ck * CHUNK + lane * FLAC_CRC_PIECE - lead; // the piece's first byte in the frame
        uint32_t crc = 0;
        if (r0 + FLAC_CRC_PIECE > 0)
            for (int i = max(0, -r0); i < FLAC_CRC_PIECE; ++i)
                crc = ((crc << 8) & 0xffffu) ^ crctab[(crc >> 8) ^ p[r0 + i]];
#pragma unroll
        for (int s = 0; s < 6; ++s)
        {
            constexpr uint32_t adv[6] = {flac_crc16_advance(0), flac_crc16_advance(1), flac_crc16_advance(2),
                                         flac_crc16_advance(3), flac_crc16_advance(4), flac_crc16_advance(5)};
            const uint32_t other = (uint32_t)__shfl_xor((int)crc, 1 << s, 64);
            const bool left = (lane & (1 << s)) == 0;
            crc = flac_crc16_mul(left ? crc : other, adv[s]) ^ (left ? other : crc);
        }
        constexpr uint32_t adv6 = flac_crc16_advance(6);
        all = flac_crc16_mul(all, adv6) ^ crc;
    }
    if (lane == 0 && all == 0)
    {
        const unsigned number = a.cand_meta[id] >> 2;
        atomicAdd(&a.nvalid[number], 1u);
        a.chosen[number] = id;
    }
}

__global__ __launch_bounds__(FLAC_IN_THREADS) void flac_in_tile_kernel(FlacInArgs a)
{
    const int n = blockIdx.x * FLAC_IN_THREADS + threadIdx.x;
    if (n >= a.nblocks)
        return;
    bool good = a.nvalid[n] == 1;
    if (good && n == 0)
        good = a.cand_pos[a.chosen[0]] == (unsigned)a.info.audio_offset;
    if (good && n > 0 && a.nvalid[n - 1] == 1) // (a predecessor that fails reports itself)
        good = a.cand_pos[a.chosen[n]] == a.cand_end[a.chosen[n - 1]];
    if (!good)
        atomicMin(&a.ctrl[1], (unsigned)n);
    if (n == 0 && a.ctrl[0] > a.cap) // more candidates than the scratch holds: reported as the frame behind the last
        atomicMin(&a.ctrl[1], (unsigned)a.nblocks);
}

__global__ __launch_bounds__(FLAC_IN_THREADS) void flac_in_output_kernel(FlacInArgs a)
{
    const long long k = (long long)blockIdx.x * FLAC_IN_THREADS + threadIdx.x;
    const unsigned first_bad = a.ctrl[1];
    if (k == 0)
        *a.status = first_bad == FLAC_IN_NONE ? 0u : 1u + first_bad;
    if (first_bad != FLAC_IN_NONE || k >= a.info.n_frames)
        return;
    const int mb = a.info.max_block, n = (int)(k / mb), i = (int)(k - (long long)n * mb);
    const unsigned id = a.chosen[n];
    const int32_t *row = a.samples + (size_t)id * 2 * mb;
    int32_t l, r;
    flac_undo_assign((int)(a.cand_meta[id] & 3), row[i], row[mb + i], l, r);
    a.out[k] = make_float2(flac_code_to_float(l, a.info.bits), flac_code_to_float(r, a.info.bits));
}

// the caller has checked info (flac_info_ok) and the scratch (flac_in_scratch_words words)
inline void launch_flac_decode(const uint8_t *bytes, size_t n_bytes, const umx_flac_info &info, unsigned *scratch, float2 *out, unsigned *status, hipStream_t st)
{
    FlacInArgs a = {};
    const size_t cap = flac_in_capacity(info.n_frames, info.max_block);
    a.nblocks = flac_in_blocks(info.n_frames, info.max_block);
    a.bytes = bytes;
    a.ctrl = scratch;
    a.cand_pos = scratch + 4;
    a.cand_end = a.cand_pos + cap;
    a.cand_meta = a.cand_end + cap;
    a.nvalid = a.cand_meta + cap;
    a.chosen = a.nvalid + a.nblocks;
    a.samples = reinterpret_cast<int32_t *>(a.chosen + a.nblocks);
    a.out = out;
    a.status = status;
    a.info = info;
    a.n_bytes = (unsigned)n_bytes;
    a.cap = (unsigned)cap;
    const auto blocks = [](size_t n, size_t per) { return dim3((unsigned)std::max<size_t>((n + per - 1) / per, 1)); };
    const size_t span = n_bytes - (size_t)info.audio_offset;
    hipLaunchKernelGGL(flac_in_clear_kernel, blocks((size_t)a.nblocks + 4, FLAC_IN_THREADS), dim3(FLAC_IN_THREADS), 0, st, a);
    hipLaunchKernelGGL(flac_in_scan_kernel, blocks(span, FLAC_IN_THREADS), dim3(FLAC_IN_THREADS), 0, st, a);
    hipLaunchKernelGGL(flac_in_decode_kernel, blocks(cap, 64), dim3(64), 0, st, a);
    hipLaunchKernelGGL(flac_in_crc_kernel, blocks(cap, 4), dim3(FLAC_IN_THREADS), 0, st, a);
    hipLaunchKernelGGL(flac_in_tile_kernel, blocks((size_t)a.nblocks, FLAC_IN_THREADS), dim3(FLAC_IN_THREADS), 0, st, a);
    hipLaunchKernelGGL(flac_in_output_kernel, blocks((size_t)info.n_frames, FLAC_IN_THREADS), dim3(FLAC_IN_THREADS), 0, st, a);
}

} // namespace umx
