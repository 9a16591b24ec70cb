"""The LPC subframe (RFC 9639 section 9.2.6) added to the independent decoder of tests/flac_ref.py, whose bit reader, residual, CRCs and
frame code it uses as they are: decode(bytes) -> (info, codes) as there, info["stats"]["lpc"][order] counting the LPC subframes.
Behind it: the signals the LPC tests add."""
import numpy as np

import flac_ref
from flac_ref import RATE

SIZES = [4096, 4097, 2 * 4096 + 17]  # one full block; a full block and a last block of one sample; two and a short one
_plain_subframe = flac_ref._subframe


def _subframe(br, bs, width, stats):
    start = br.p
    head = br.u(8)
    if (head >> 1) & 63 < 32:
        br.p = start
        return _plain_subframe(br, bs, width, stats)
    assert head >> 7 == 0 and head & 1 == 0, "flac_lpc_ref: padding bit, no wasted bits"
    order = ((head >> 1) & 63) - 31
    assert order < bs
    x = [br.s_(width) for _ in range(order)]
    precision = br.u(4) + 1
    assert precision != 16, "flac_lpc_ref: reserved coefficient precision"
    shift = br.s_(5)
    assert shift >= 0, "flac_lpc_ref: a negative shift is forbidden"
    c = [br.s_(precision) for _ in range(order)]
    res, method = flac_ref._residual(br, bs, order)
    stats["lpc"][order] += 1
    stats["rice2"] += method
    for r in res:  # (Python integers: the prediction is exact, >> floors as an arithmetic shift does)
        x.append(r + (sum(ci * x[-1 - i] for i, ci in enumerate(c)) >> shift))
    return x


def decode(data):
    """flac_ref.decode with the subframe reader above in place of its own for the length of the call"""
    counts = [0] * 33

    def sub(br, bs, width, stats):
        stats.setdefault("lpc", counts)
        return _subframe(br, bs, width, stats)

    flac_ref._subframe = sub
    try:
        info, codes = flac_ref.decode(data)
    finally:
        flac_ref._subframe = _plain_subframe
    info["stats"].setdefault("lpc", counts)
    return info, codes


def signal(name, n):
    t = np.arange(n, dtype=np.float64)
    if name == "two_tones":
        one = 0.4 * np.sin(2 * np.pi * 3000.0 * t / RATE) + 0.3 * np.sin(2 * np.pi * 7000.0 * t / RATE + 1.0)
    elif name == "resonance":  # y[i] = 1.2 y[i-1] - 0.8 y[i-2] + noise: a pole pair of radius 0.894
        e = np.random.default_rng(4321 + n).standard_normal(n)
        one = np.zeros(n)
        for i in range(n):
            one[i] = e[i] + (1.2 * one[i - 1] if i >= 1 else 0.0) - (0.8 * one[i - 2] if i >= 2 else 0.0)
        one *= 0.5 / np.abs(one).max()
    else:
        return flac_ref.signal(name, n)
    return np.stack([one, one[::-1]]).astype(np.float32)
