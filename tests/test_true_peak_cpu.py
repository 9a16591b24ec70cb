"""True peak of every output (csrc/true_peak.h) without a GPU: the taps and the host statement of the rule
(umx_hip_true_peak_taps, umx_hip_true_peak_host) against the float64 rule of tests/true_peak_ref.py, the fs/4 tone table, the
invariants of a maximum over fixed windows, the divisor over the true-peak words, and the surface of the new entry points."""
import ctypes as C

import numpy as np
import pytest

import true_peak_ref as ref

RATES = [8000, 44100, 48000, 96000, 192000]
# the fs/4 tone, 0.5 s at amplitude 0.5 with a hard onset, computed in float64 by the rule (dB, two decimals)
TABLE = {"phase": (0.0, 45.0, 60.0, 67.5), "sample": (-6.02, -9.03, -7.27, -6.71), "tp4": (-6.02, -5.92, -6.00, -5.91),
         "tp2": (-6.02, -5.92, -6.08, -6.40)}
WORST = {"fraction": 0.0}  # the largest observed |host - float64| / bound, over this module


def _tp(pkg, x, rate, first=0, count=None, bits=0):
    return pkg.true_peak_host(x, rate, first, count, bits)


def _f(pkg, bits):
    return float(pkg.true_peak_float(bits))


def _peak_bits(x):
    """levels.h's peak rule on (2, n) float32: the unsigned maximum of the bit patterns of |x| over what is not NaN"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0x7fffffff)
    u = u[u <= 0x7f800000]
    return np.uint32(u.max()) if u.size else np.uint32(0)


@pytest.mark.parametrize("rate,factor", list(zip(RATES, (4, 4, 4, 2, 1))))
def test_taps(pkg, rate, factor):
    h, F = pkg.true_peak_taps(rate)
    want, Fw = ref.taps(rate)
    assert F == factor == Fw and h.dtype == np.float32 and h.shape == (49,)
    err = float(np.max(np.abs(h.astype(np.float64) - want)))
    print("taps", rate, "largest deviation from float64", err)
    assert err <= 6e-8
    assert h[24] == np.float32(1.0) and h[0] == 0 and h[48] == 0
    assert np.all(np.abs(want[np.arange(0, 49, F)][np.arange(0, 49, F) != 24]) < 1e-15)  # phase 0 is the sample itself
    for rate_ in (7999, 192001):
        with pytest.raises(pkg.UmxError):
            pkg.true_peak_taps(rate_)


@pytest.mark.parametrize("rate", RATES)
def test_host_against_float64(pkg, rate):
    """noise + DC + a 40 dB step: the whole track's maximum, and frame by frame over the step, within the fp32 round-off of the sums
    plus the tap rounding (ref.bound: computed, not chosen; |max a - max b| <= max |a - b|)"""
    n = 1500
    x = ref.stepped(rate, n, 5 + rate % 7)
    tol = ref.bound(x, rate)
    got, want = _f(pkg, _tp(pkg, x, rate)), ref.true_peak(x, rate)
    frac = [abs(got - want) / tol if tol else float(got != want)]
    assert abs(got - want) <= tol, (rate, got, want, tol)
    y, _ = ref.interpolated(x, rate)
    for k in list(range(0, 40)) + list(range(n // 2 - 30, n // 2 + 30)) + list(range(n - 40, n)):
        g = _f(pkg, _tp(pkg, x, rate, k, 1))
        w = max(float(np.max(np.abs(x[:, k]))), float(np.max(np.abs(y[:, :, k]))) if y.size else 0.0)
        assert abs(g - w) <= tol, (rate, k, g, w, tol)
        frac.append(abs(g - w) / tol if tol else float(g != w))
    WORST["fraction"] = max(WORST["fraction"], max(frac))
    print("host against float64", rate, "bound", tol, "largest |host - float64| / bound", max(frac), "largest so far", WORST["fraction"])


@pytest.mark.parametrize("rate", [44100, 48000])
def test_tone_table(pkg, rate):
    for i, ph in enumerate(TABLE["phase"]):
        x = ref.tone(rate, ph).astype(np.float32)
        want = ref.db(ref.true_peak(x, rate))
        got = ref.db(_f(pkg, _tp(pkg, x, rate)))
        sample = ref.db(ref.sample_peak(x))
        print("tone", rate, ph, "sample peak", sample, "true peak float64", want, "host", got)
        assert abs(want - TABLE["tp4"][i]) <= 0.006 and abs(sample - TABLE["sample"][i]) <= 0.006
        assert abs(got - want) <= 0.01
        assert -6.4 <= got <= -5.8  # EBU Tech 3341: -6.0 +0.2 / -0.4


def test_tone_table_at_96k(pkg):
    for i, ph in enumerate(TABLE["phase"]):
        x = ref.tone(96000, ph).astype(np.float32)
        want, got = ref.db(ref.true_peak(x, 96000)), ref.db(_f(pkg, _tp(pkg, x, 96000)))
        assert abs(want - TABLE["tp2"][i]) <= 0.006 and abs(got - want) <= 0.01, (ph, want, got)


@pytest.mark.parametrize("rate", RATES)
def test_true_peak_is_at_least_the_peak(pkg, rate):
    for seed in range(3):
        x = ref.stepped(rate, 700 + seed, seed)
        t, p = _tp(pkg, x, rate), _peak_bits(x)
        assert t >= p
        if rate == 192000:
            assert t == p
    x = ref.tone(rate, 45.0, 0.01).astype(np.float32)
    assert (_tp(pkg, x, rate) > _peak_bits(x)) == (rate != 192000)


@pytest.mark.parametrize("rate", [44100, 96000])
def test_short_tracks_and_the_edges(pkg, rate):
    F = ref.factor_of(rate)
    reach = 24 // F
    one = np.array([[0.75], [-0.25]], np.float32)
    got = _f(pkg, _tp(pkg, one, rate))  # n = 1: the sample, and the taps beside the centre times it
    assert abs(got - ref.true_peak(one, rate)) <= ref.bound(one, rate) and got >= 0.75
    for n in (2, 5, reach, 2 * reach - 1):  # shorter than the window
        x = ref.stepped(rate, n, n)
        assert abs(_f(pkg, _tp(pkg, x, rate)) - ref.true_peak(x, rate)) <= ref.bound(x, rate), n
    # an inter-sample peak in the first and in the last 24/F frames: the 45 degree tone cut to a few frames at either end of silence
    burst = ref.tone(rate, 45.0, 8 / rate).astype(np.float32)
    for at in (0, 400 - burst.shape[1]):
        x = np.zeros((2, 400), np.float32)
        x[:, at:at + burst.shape[1]] = burst
        got, want = _f(pkg, _tp(pkg, x, rate)), ref.true_peak(x, rate)
        assert abs(got - want) <= ref.bound(x, rate) and got > ref.sample_peak(x) * 1.05, (at, got, want)


@pytest.mark.parametrize("rate", [44100, 96000, 192000])
def test_a_nan_and_an_inf(pkg, rate):
    x = ref.stepped(rate, 600, 3)
    x[0, 100] = 0.9  # the track's peak, far from the NaN
    clean = _tp(pkg, x, rate)
    bad = x.copy()
    bad[1, 400] = np.nan
    got = _tp(pkg, bad, rate)
    assert got == clean and got >= _peak_bits(x)  # the NaN and the values it reaches contribute nothing
    bad = x.copy()
    bad[1, 400] = -np.inf
    assert _tp(pkg, bad, rate) == np.uint32(0x7f800000)
    assert _tp(pkg, np.full((2, 30), np.nan, np.float32), rate) == 0


@pytest.mark.parametrize("rate", [8000, 96000])
def test_a_span_in_three_pieces_is_the_whole(pkg, rate):
    x = ref.tone(rate, 45.0, 900 / rate).astype(np.float32) + ref.stepped(rate, 900, 1)
    whole = _tp(pkg, x, rate, 17, 800)
    bits = 0
    for a, b in ((500, 817), (17, 18), (18, 500)):
        bits = _tp(pkg, x, rate, a, b - a, bits)
    assert bits == whole
    assert _tp(pkg, x, rate, 17, 0, 123) == 123  # an empty span accumulates nothing
    assert _tp(pkg, x, rate) >= whole


def test_the_divisor_over_the_true_peak_words(pkg):
    """DESIGN 20's divisor rule, P the largest true peak: g = 1.01f P; 1 when P is not finite or !(g > 1)"""
    x = (ref.tone(44100, 45.0, 0.01) * 2.4).astype(np.float32)  # sample peak 0.85, true peak about 1.2
    tp = pkg.true_peak_float(_tp(pkg, x, 44100))
    assert ref.sample_peak(x) < 1 / 1.01 < 1 < tp
    assert pkg.rescale_gain([ref.sample_peak(x)]) == np.float32(1.0)
    g = pkg.rescale_gain([0.1, tp, 0.5])
    assert g == np.float32(1.01) * tp and g > 1
    y = (x / g).astype(np.float32)  # correctly rounded fp32 quotients
    assert pkg.true_peak_float(_tp(pkg, y, 44100)) <= 1.0
    assert pkg.rescale_gain([np.inf]) == 1 and pkg.rescale_gain([0.5]) == 1


def test_entry_points(pkg):
    lib = pkg.hip_lib()
    for name in ("umx_hip_separate_tracks_true_peak", "umx_hip_separate_queue_true_peak", "umx_hip_true_peak_device", "umx_hip_true_peak_taps",
                 "umx_hip_true_peak_host"):
        assert name in pkg.HIP_SYMBOLS and getattr(lib, name) is not None
    assert (pkg.TRUE_PEAK_OFF, pkg.TRUE_PEAK_MEASURE, pkg.TRUE_PEAK_RESCALE) == (0, 1, 2)
    assert C.sizeof(pkg.TruePeak) == 4 * 4 + 4 + 4
    for method in ("separate_many_true_peak", "true_peak_device"):
        assert hasattr(pkg.Engine, method)
    import inspect
    assert "true_peak" in inspect.signature(pkg.Engine.separate_queue).parameters
    # a NULL context is refused before anything else is looked at
    callbacks = (pkg.QUEUE_NEXT_FN, pkg.QUEUE_TRUE_PEAK_FN)
    for name in ("umx_hip_separate_tracks_true_peak", "umx_hip_separate_queue_true_peak", "umx_hip_true_peak_device"):
        fn = getattr(lib, name)
        args = [(7 if t in (C.c_int, C.c_uint, C.c_longlong) else t() if t in callbacks else None) for t in fn.argtypes[1:]]
        assert fn(None, *args) == pkg.ERR_ARG, name
    # the host forms refuse what they cannot read
    bits = C.c_uint(0)
    x = np.zeros(8, np.float32)
    xp = x.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.umx_hip_true_peak_host(None, 4, 44100, 0, 4, C.byref(bits)) == pkg.ERR_ARG
    assert lib.umx_hip_true_peak_host(xp, 4, 44100, 0, 4, None) == pkg.ERR_ARG
    assert lib.umx_hip_true_peak_host(xp, 4, 44100, 1, 4, C.byref(bits)) == pkg.ERR_ARG
    assert lib.umx_hip_true_peak_host(xp, 4, 44100, -1, 1, C.byref(bits)) == pkg.ERR_ARG
    assert lib.umx_hip_true_peak_host(xp, 4, 7999, 0, 4, C.byref(bits)) == pkg.ERR_ARG
    assert lib.umx_hip_true_peak_host(xp, 4, 44100, 0, 4, C.byref(bits)) == pkg.UMX_OK and bits.value == 0
