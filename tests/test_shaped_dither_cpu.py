"""Noise-shaped dither for 16-bit outputs, the host side: umx_hip_pcm16_encode_host with UMX_DITHER_SHAPED against the
float32 restatement of tests/shaped_ref.py bit for bit, the properties of the rule, the refusals, and its spectrum against the
noise transfer function in float64.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import shaped_ref as ref

NS = [1, 5, 4095, 4096, 4097, 2 * 4096 + 17]


def _signal(kind, n):
    if kind == "silence":
        return np.zeros((2, n), np.float32)
    if kind == "sine":  # -60 dBFS, 1 kHz
        t = np.arange(n) / 44100.0
        return np.stack([1e-3 * np.sin(2 * np.pi * 1000 * t), 1e-3 * np.cos(2 * np.pi * 1000 * t)]).astype(np.float32)
    return (np.random.default_rng(n).standard_normal((2, n)) * 0.6).astype(np.float32)  # full scale and beyond +-1


@pytest.mark.parametrize("first", [0, 3 * 4096])
@pytest.mark.parametrize("kind", ["silence", "sine", "noise"])
@pytest.mark.parametrize("n", NS)
def test_host_rule_equals_the_restatement(pkg, n, kind, first):
    x = _signal(kind, n)
    for m, seed in ((0, 7), (3, 0xFFFFFFFF)):
        q = pkg.pcm16_encode_host(x, m, first, seed, shaped=True)
        want, clipped = ref.encode(x, m, first, seed)
        assert np.array_equal(q, want), (m, seed, np.flatnonzero((q != want).any(axis=0))[:4])
        assert kind != "noise" or n < 4095 or clipped > 0
        # where nothing clamps the code stays within the rounding, the dither and the fed-back errors of the sample
        free = np.abs(32767.0 * x.astype(np.float64)) < 32000
        assert np.all(np.abs(q - 32767.0 * x.astype(np.float64))[free] <= 0.5 + 1 + 1.5 * sum(abs(float(c)) for c in ref.C))


def test_mode_one_is_unchanged(pkg):
    x = _signal("noise", 9000)
    io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, 5)
    assert (io.dither, pkg.DITHER_TPDF, pkg.DITHER_SHAPED) == (1, 1, 2) and pkg.sample_io(shaped=True, dither_seed=5).dither == 2
    import pcm16_ref
    assert np.array_equal(pkg.pcm16_encode_host(x, 1, 77, 5, shaped=False), pcm16_ref.encode(x, 1, 77, 5))
    assert not np.array_equal(pkg.pcm16_encode_host(x, 1, 0, 5, shaped=True), pkg.pcm16_encode_host(x, 1, 0, 5))


def test_nan_and_inf_do_not_outlive_their_sample(pkg):
    x = _signal("sine", 300)
    x[0, 100], x[1, 100], x[0, 200] = np.nan, np.inf, -np.inf
    q = pkg.pcm16_encode_host(x, 0, 0, 3, shaped=True)
    assert (q[0, 100], q[1, 100], q[0, 200]) == (0, 32767, -32768)
    want, clipped = ref.encode(x, 0, 0, 3)
    assert clipped == 2 and np.array_equal(q, want)  # (the samples behind them included: their error was dropped, not fed back)
    assert np.abs(q[:, 101:106].astype(np.float64) - 32767.0 * x[:, 101:106]).max() < 16


def test_refusals_and_their_reasons(pkg):
    lib = pkg.hip_lib()
    x = np.zeros((2, 8), np.float32)

    def reason(call):
        with pytest.raises(pkg.UmxError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG
        return str(e.value)

    assert "4096" in reason(lambda: pkg.pcm16_encode_host(x, 0, 5, 1, shaped=True))
    assert "16-bit" in reason(lambda: pkg._encode_host(24, x, 0, 0, 1, shaped=True))
    a, q = np.zeros(16, np.float32), np.zeros(16, np.int16)
    last = lambda: lib.umx_hip_last_error(None).decode()
    io = pkg.SampleIO(pkg.SAMPLE_F32, pkg.SAMPLE_S16, 3, 0)
    assert lib.umx_hip_pcm16_encode_host(a.ctypes.data_as(pkg._fp), 8, 0, 0, C.byref(io), q.ctypes.data_as(pkg._i16p)) == pkg.ERR_ARG
    assert "unknown dither mode" in last()
    io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, 1, shaped=True)
    reason(lambda: pkg.levels_host(x, io=io))
    assert "levels" in last() and "16-bit" in last()
    out, got = np.zeros(pkg.flac_bound(8, 16), np.uint8), C.c_size_t(0)
    assert lib.umx_hip_flac_encode_host(a.ctypes.data_as(pkg._fp), 8, 44100, 16, 0, C.byref(io), out.ctypes.data_as(pkg._u8p), out.size,
                                        C.byref(got)) == pkg.ERR_ARG
    assert "16-bit" in last() and "FLAC" in last()
    assert np.array_equal(pkg.pcm16_encode_host(x, 0, 4096, 1, shaped=True), ref.encode(x, 0, 4096, 1)[0])  # and a good call afterwards


def _band_ratios(pkg, seed, n=1 << 18):
    x = _signal("sine", n)
    ideal = 32767.0 * x[0].astype(np.float64)
    err = [pkg.pcm16_encode_host(x, 0, 0, seed, shaped=s)[0].astype(np.float64) - ideal for s in (True, False)]
    p = [np.abs(np.fft.rfft(e)) ** 2 for e in err]
    f = np.fft.rfftfreq(n, 1 / 44100.0)
    return [float(p[0][(f >= lo) & (f <= hi)].sum() / p[1][(f >= lo) & (f <= hi)].sum()) for lo, hi in ((0, 4000), (16000, 22050))]


def test_spectrum_follows_the_noise_transfer_function(pkg):
    """Error power shaped / TPDF in 0 - 4 kHz and 16 - 22.05 kHz against the band mean of |N(f)|^2 in float64.  Measured on the host
    rule over seeds 1, 2, 3: ratio / theory - 1 is +0.0397, +0.0469, +0.0367 in the low band (the five unshaped frames
    behind every block's reset add white error where the shaped error is 2 % of it) and -0.0079, -0.0039, -0.0001 in the high band;
    the bound is twice the worst, 0.094."""
    theory = [ref.ntf_band_mean(0, 4000), ref.ntf_band_mean(16000, 22050)]
    assert theory[0] < 0.1 and theory[1] > 20  # the power leaves the band the ear is most sensitive in for the top octave
    for seed in (1, 2, 3):
        for got, want in zip(_band_ratios(pkg, seed), theory):
            assert abs(got / want - 1) <= 0.094, (seed, got, want)
