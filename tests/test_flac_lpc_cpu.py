"""FLAC with LPC subframes, the host side: umx_hip_flac_encode_host_lpc decoded by tests/flac_lpc_ref.py must give exactly
the codes its flac_lpc = 0 stream decodes to, in frames that are never larger.  No GPU."""
import numpy as np
import pytest

import flac_lpc_ref
import flac_ref
from flac_lpc_ref import SIZES, signal
from flac_ref import RATE

SIGNALS = ["two_tones", "resonance", "sine", "noise", "silence", "nonfinite", "noise24_quiet"]
_plain = {}  # (name, bits, n) -> the flac_lpc = 0 stream, its info and its codes: decoded once, by the decoder without LPC


def plain(pkg, name, bits, n):
    if (name, bits, n) not in _plain:
        stream = pkg.flac_encode_host(signal(name, n), RATE, bits, buffer=1, lpc=None)  # (the entry point without flac_lpc)
        _plain[name, bits, n] = (stream,) + flac_ref.decode(stream)
    return _plain[name, bits, n]


@pytest.mark.parametrize("lpc", [1, 4, 12])
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("name", SIGNALS)
@pytest.mark.parametrize("n", SIZES)
def test_the_lpc_stream_decodes_to_the_fixed_streams_codes_in_no_larger_frames(pkg, n, name, bits, lpc):
    x = signal(name, n)
    base, info0, want = plain(pkg, name, bits, n)
    assert np.array_equal(pkg.flac_encode_host(x, RATE, bits, buffer=1, lpc=0), base)  # 0 through the new entry point: the old bytes
    stream = pkg.flac_encode_host(x, RATE, bits, buffer=1, lpc=lpc)
    info, got = flac_lpc_ref.decode(stream)
    assert (info["rate"], info["bits"], info["total"]) == (RATE, bits, n) and np.array_equal(got, want)
    frames, frames0 = info["stats"]["frames"], info0["stats"]["frames"]
    assert len(frames) == len(frames0) and all(f <= f0 for (_, f), (_, f0) in zip(frames, frames0)), (frames, frames0)
    used = info["stats"]["lpc"]
    assert sum(used[lpc + 1:]) == 0 and sum(used) <= 2 * (n // pkg.FLAC_BLOCK)  # no order above the cap; two subframes a full block at most
    if n % pkg.FLAC_BLOCK:  # a short last block never tries LPC: its frame is the FIXED-only stream's, byte for byte
        assert frames[-1] == frames0[-1] and np.array_equal(stream[-frames[-1][1]:], base[-frames[-1][1]:])
    # No FIXED order predicts two tones at 3 and 7 kHz; linear prediction from the second order on does (measured at 2 x 4096 + 17
    # frames, 16 bits: 30297 bytes FIXED-only, 28722 / 27130 / 6502 under a cap of 2 / 3 / 4).  Under a cap of ONE the exact-bits rule
    # must keep FIXED order 4: one tap leaves a residual power of about 0.049 of the signal's, FIXED order 4 about 0.032.
    if name == "two_tones" and lpc >= 4:
        assert sum(used) > 0 and stream.size < base.size
    elif name == "two_tones":
        assert np.array_equal(stream, base)


def test_the_refusals(pkg):
    x = signal("two_tones", 4096)
    for bits, lpc, why in [(16, 13, "flac_lpc must be 0 .. 12"), (24, -1, "flac_lpc must be 0 .. 12"), (0, 4, "flac_lpc needs bits")]:
        with pytest.raises(pkg.UmxError) as e:
            pkg.flac_encode_host(x, RATE, bits, lpc=lpc)
        assert e.value.code == pkg.ERR_ARG and why in str(e.value), (bits, lpc, str(e.value))
