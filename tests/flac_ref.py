"""A plain FLAC decoder, written from the format (RFC 9639) and not from the encoder: the independent reference of the FLAC tests.
It covers what DESIGN 29 emits and refuses everything else: marker and STREAMINFO, fixed-blocksize frame headers with the UTF-8
number and both block size fields, the four stereo channel assignments, CONSTANT / VERBATIM / FIXED 0-4 subframes, RICE and RICE2
residuals with partitions and the escape code, CRC-8 and CRC-16 verified on every frame, and STREAMINFO's sizes and total checked
against what was parsed.  decode(bytes) -> (info dict, (2, n) int32 codes).  Behind it: the sizes and signals both FLAC test files share."""
import numpy as np


def _crc_table(poly, width):
    top, mask, table = 1 << (width - 1), (1 << width) - 1, []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly if c & top else c << 1) & mask
        table.append(c)
    return table


_CRC8, _CRC16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data):
    c = 0
    for b in data:
        c = _CRC8[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


class _Bits:
    """MSB-first reader over a string of '0' / '1' (a frame is at most 25 KB: plain text is fast enough and leaves nothing to get wrong)."""

    def __init__(self, data, pos):
        self.s = "".join(f"{b:08b}" for b in data)
        self.p = 8 * pos

    def u(self, n):
        assert self.p + n <= len(self.s), "flac_ref: the stream ends inside a frame"
        v = int(self.s[self.p:self.p + n], 2) if n else 0
        self.p += n
        return v

    def s_(self, n):
        v = self.u(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self):
        q = self.s.index("1", self.p) - self.p
        self.p += q + 1
        return q


def _residual(br, bs, order):
    method = br.u(2)
    assert method in (0, 1), "flac_ref: reserved residual coding method"
    pbits, escape = (4, 15) if method == 0 else (5, 31)
    porder = br.u(4)
    assert bs % (1 << porder) == 0 and (bs >> porder) > order - (porder == 0), "flac_ref: partition order does not fit the block"
    out = []
    for j in range(1 << porder):
        n = (bs >> porder) - (order if j == 0 else 0)
        k = br.u(pbits)
        if k == escape:
            w = br.u(5)
            out += [br.s_(w) if w else 0 for _ in range(n)]
            continue
        for _ in range(n):
            u = (br.unary() << k) | br.u(k)
            out.append((u >> 1) ^ -(u & 1))
    return out, method


_FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}


def _subframe(br, bs, width, stats):
    assert br.u(1) == 0, "flac_ref: subframe padding bit"
    kind = br.u(6)
    assert br.u(1) == 0, "flac_ref: wasted bits are not part of this subset"
    if kind == 0:
        stats["constant"] += 1
        return [br.s_(width)] * bs
    if kind == 1:
        stats["verbatim"] += 1
        return [br.s_(width) for _ in range(bs)]
    assert 8 <= kind <= 12, f"flac_ref: subframe type {kind} is not part of this subset"
    order = kind - 8
    assert order <= bs
    x = [br.s_(width) for _ in range(order)]
    res, method = _residual(br, bs, order)
    stats["fixed"][order] += 1
    stats["rice2"] += method
    c = _FIXED[order]
    for r in res:
        x.append(r + sum(ci * x[-1 - i] for i, ci in enumerate(c)))
    return x


def decode(data):
    data = bytes(bytearray(np.asarray(data, np.uint8))) if not isinstance(data, (bytes, bytearray)) else bytes(data)
    assert data[:4] == b"fLaC", "flac_ref: no fLaC marker"
    assert data[4] == 0x80 and int.from_bytes(data[5:8], "big") == 34, "flac_ref: one STREAMINFO block, flagged last"
    si = data[8:42]
    v = int.from_bytes(si[10:18], "big")
    info = {"min_block": int.from_bytes(si[0:2], "big"), "max_block": int.from_bytes(si[2:4], "big"),
            "min_frame": int.from_bytes(si[4:7], "big"), "max_frame": int.from_bytes(si[7:10], "big"),
            "rate": v >> 44, "channels": ((v >> 41) & 7) + 1, "bits": ((v >> 36) & 31) + 1, "total": v & ((1 << 36) - 1),
            "md5": si[18:34]}
    assert info["channels"] == 2 and info["bits"] in (16, 24) and info["md5"] == bytes(16)
    bps, block = info["bits"], info["max_block"]
    stats = {"constant": 0, "verbatim": 0, "fixed": [0] * 5, "rice2": 0, "assign": [0] * 4, "frames": []}
    pos, number, left, right = 42, 0, [], []
    while pos < len(data):
        start = pos
        assert data[pos] == 0xFF and data[pos + 1] == 0xF8, "flac_ref: frame sync of a fixed-blocksize stream"
        bcode, rcode = data[pos + 2] >> 4, data[pos + 2] & 15
        ccode, scode = data[pos + 3] >> 4, (data[pos + 3] >> 1) & 7
        assert rcode == 0 and data[pos + 3] & 1 == 0 and scode == {16: 4, 24: 6}[bps]
        pos += 4
        lead = data[pos]
        extra = 0 if lead < 0x80 else next(n for n in range(1, 7) if not lead & (0x40 >> n))
        num = lead if not extra else lead & (0x3F >> extra)
        for i in range(extra):
            assert data[pos + 1 + i] >> 6 == 2, "flac_ref: UTF-8 continuation byte"
            num = (num << 6) | (data[pos + 1 + i] & 0x3F)
        pos += 1 + extra
        assert num == number, "flac_ref: frame numbers count up from 0"
        if bcode == 6:
            bs, pos = data[pos] + 1, pos + 1
        elif bcode == 7:
            bs, pos = int.from_bytes(data[pos:pos + 2], "big") + 1, pos + 2
        else:
            assert bcode >= 8, f"flac_ref: block size code {bcode}"
            bs = 256 << (bcode - 8)
        assert crc8(data[start:pos]) == data[pos], "flac_ref: header CRC-8"
        pos += 1
        assert ccode in (1, 8, 9, 10), f"flac_ref: channel assignment {ccode}"
        br = _Bits(data[start:start + 16 + 2 * (1 + (bs * (bps + 1) + 7) // 8) + 64], pos - start)
        a = _subframe(br, bs, bps + (ccode == 9), stats)
        b = _subframe(br, bs, bps + (ccode in (8, 10)), stats)
        if ccode == 8:
            b = [x - y for x, y in zip(a, b)]
        elif ccode == 9:
            a = [x + y for x, y in zip(a, b)]
        elif ccode == 10:
            mid = [(m << 1) | (s & 1) for m, s in zip(a, b)]
            a, b = [(m + s) >> 1 for m, s in zip(mid, b)], [(m - s) >> 1 for m, s in zip(mid, b)]
        stats["assign"][{1: 0, 8: 1, 9: 2, 10: 3}[ccode]] += 1
        assert br.u(-br.p % 8) == 0, "flac_ref: padding to the byte is zero"
        pos = start + br.p // 8
        assert crc16(data[start:pos]) == int.from_bytes(data[pos:pos + 2], "big"), "flac_ref: frame CRC-16"
        pos += 2
        stats["frames"].append((bs, pos - start))
        left += a
        right += b
        number += 1
    sizes = [f for _, f in stats["frames"]]
    assert all(b == block for b, _ in stats["frames"][:-1]) and 1 <= stats["frames"][-1][0] <= block
    assert info["min_block"] == block and info["total"] == len(left)
    assert info["min_frame"] == min(sizes) and info["max_frame"] == max(sizes)
    info["stats"] = stats
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    assert all(lo <= x <= hi for x in left) and all(lo <= x <= hi for x in right), "flac_ref: a decoded sample outside the stream's width"
    return info, np.array([left, right], np.int32)


# ---------------------------------------------------------------- what the FLAC tests encode
# blocks shorter than the predictor orders; the block edge; the 8-bit against the 16-bit last-blocksize field; a short last block
SIZES = [1, 3, 4, 4095, 4096, 4097, 4096 + 256, 4096 + 257, 2 * 4096 + 17]
RATE = 44100


def signal(name, n):
    rng = np.random.default_rng(1234 + n)
    t = np.arange(n, dtype=np.float64)
    one = {"silence": lambda: np.zeros(n), "sine": lambda: 0.5 * np.sin(2 * np.pi * 440.0 * t / RATE),
           "noise": lambda: 0.9 * rng.uniform(-1, 1, n), "alternating": lambda: np.where(t % 2 == 0, 1.0, -1.0),
           "noise24": lambda: rng.uniform(-1, 1, n), "noise24_quiet": lambda: 0.05 * rng.uniform(-1, 1, n)}
    if name == "equal":
        l = 0.3 * rng.uniform(-1, 1, n)
        x = np.stack([l, l])
    elif name == "opposite":
        l = 0.3 * rng.uniform(-1, 1, n)
        x = np.stack([l, -l])
    elif name == "nonfinite":
        x = np.stack([1.7 * np.sin(0.01 * t), rng.uniform(-3, 3, n)])
        x[0, 0::7], x[1, 1::11], x[0, 2::13] = np.nan, np.inf, -np.inf
    else:
        x = np.stack([one[name](), one[name]()[::-1]])
    return x.astype(np.float32)
