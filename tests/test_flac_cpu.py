"""FLAC out, the host side: umx_hip_flac_encode_host decoded by the independent decoder of tests/flac_ref.py must give
exactly the codes of umx_hip_pcm16_encode_host / umx_hip_pcm24_encode_host for the same fp32 input.  No GPU."""
import numpy as np
import pytest

import flac_ref
from flac_ref import RATE, SIZES, signal

CASES = [(s, 16) for s in ("silence", "equal", "opposite", "sine", "noise", "alternating", "nonfinite")] + [("noise24", 24), ("noise24_quiet", 24), ("sine", 24), ("nonfinite", 24)]


@pytest.mark.parametrize("dither", [None, 77])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,bits", CASES)
def test_the_host_stream_decodes_to_the_pcm_codes(pkg, name, bits, n, dither):
    x = signal(name, n)
    stream = pkg.flac_encode_host(x, RATE, bits, buffer=2, dither_seed=dither)
    want = (pkg.pcm16_encode_host if bits == 16 else pkg.pcm24_encode_host)(x, buffer=2, dither_seed=dither).astype(np.int32)
    info, got = flac_ref.decode(stream)
    assert (info["rate"], info["bits"], info["total"], info["max_block"]) == (RATE, bits, n, pkg.FLAC_BLOCK)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert stream.size <= pkg.flac_bound(n, bits)
    assert np.array_equal(stream, pkg.flac_encode_host(x, RATE, bits, buffer=2, dither_seed=dither))  # deterministic
    st = info["stats"]
    if name == "silence" and dither is None:
        assert st["constant"] == 2 * len(st["frames"]) and st["assign"][0] == len(st["frames"])  # ties go to independent
    if name == "sine" and n >= 4095:
        assert stream.size < n * 2 * bits // 8 and sum(st["fixed"][2:]) > 0  # smaller than its PCM bytes; a high order wins
    if name == "noise24" and n >= 4095:
        assert st["rice2"] + st["verbatim"] > 0  # full range: parameters above 14, unless VERBATIM (24 bits a sample) is smaller still
    if name == "noise24_quiet" and n >= 4095:
        assert st["rice2"] > 0 and st["verbatim"] == 0  # 19 significant bits: parameters above 14, so RICE2
    if name == "equal" and dither is None and n > 4:
        ones = sum(1 for bs, _ in st["frames"] if bs == 1)  # (a block of one sample: two CONSTANTs, and L, R are a bit narrower than S)
        assert st["assign"][0] == ones and st["constant"] >= len(st["frames"])  # elsewhere the constant side channel is taken


def test_the_block_size_fields_and_the_refusals(pkg):
    x = signal("noise", 4096 + 257)
    for n, last in [(4096 + 256, 256), (4096 + 257, 257), (4096, 4096)]:
        info, _ = flac_ref.decode(pkg.flac_encode_host(x[:, :n], 48000, 16))
        assert info["stats"]["frames"][-1][0] == last and info["rate"] == 48000
    assert pkg.flac_bound(1, 12) == 0 and pkg.flac_bound(4097, 24) > pkg.flac_bound(4096, 24) > 4096 * 6
    for bad in [dict(bits=12), dict(bits=16, cap=pkg.flac_bound(4096, 16) - 1), dict(bits=16, buffer=4), dict(bits=24, rate=0)]:
        with pytest.raises(pkg.UmxError):
            pkg.flac_encode_host(x[:, :4096], bad.pop("rate", RATE), **bad)
