"""The measurement layer behind levels, loudness and true peak as a matrix: driver (one lane, three lanes of unequal
length, the queue on two lanes with a refilled lane) x what is asked (each record alone, the energies alone, all at once, both
rescales) x output format (fp32, int16) x rate (44.1 kHz, 48 kHz through the resampler).  Every case is held to the narrowest rung of
the ladder that can express it -- outputs bit for bit, records byte for byte --, the queue's jobs to the one-track call, and what
was measured to the host statements of the rules (umx_hip_kweight_hops_host, umx_hip_true_peak_host), exactly, over the fp32 outputs
of the call that measures nothing.

The tracks come from the code's own quantities: A has three segments and a last partial hop (hop = kweight_hop(rate) = 4410 / 4800
frames), B is shorter than one hop (no hop: the max(1, ...) allocation and the empty report), C is shorter than the true-peak
reach of 24 / F = 6 frames."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 16 * 1024  # segment_samples: stride 12288
SEED = 7
LENGTHS = (30000, 3000, 4)  # A, B, C
SHIFTS = (None, 4033, 0)  # (B and C behind a shift's padding: two segments each)
GAINS = np.array([[0, 0, 0, 0, 3], [0, 0, 0, 0, 0.25], [0, 0, 0, 1, 0]], np.float32)  # as tests/test_gpu_levels.py: output 0 leaves above 1
RATES = (44100, 48000)
FORMATS = ("f32", "s16")
OFF, MEASURE, TP_RESCALE = 0, 1, 2  # pkg.TRUE_PEAK_*
CLAMP, RESCALE = 0, 1  # pkg.CLIP_*

# what is asked: the arguments of the widest rung (separate_many_true_peak) and the narrowest rung that can express it with its own
ASKS = {
    "levels": (dict(true_peak=OFF, levels=True, records=False), "levels", dict(levels=True)),
    "loudness records": (dict(true_peak=OFF, levels=False, loudness=True, records=False), "loudness", dict(levels=False, loudness=True, envelopes=False)),
    "hop energies": (dict(true_peak=OFF, levels=False, envelopes=True, records=False), "loudness", dict(levels=False, loudness=False, envelopes=True)),
    "true peak, no records": (dict(true_peak=MEASURE, levels=False, records=False), "io", dict()),
    "true peak": (dict(true_peak=MEASURE, levels=False, records=True), None, None),
    "all": (dict(true_peak=MEASURE, levels=True, loudness=True, envelopes=True, records=True), None, None),
    "rescale": (dict(true_peak=OFF, clip=RESCALE, levels=True, records=False), "levels", dict(clip=RESCALE, levels=True)),
    "rescale on the true peak": (dict(true_peak=TP_RESCALE, clip=RESCALE, levels=True, records=True), None, None),
}
# the queue's entry points: the arguments of separate_queue and the one-track call that is the same job
QUEUE_ASKS = {
    "levels": (dict(levels=True), "levels", dict(levels=True)),
    "loudness": (dict(loudness=True), "loudness", dict()),
    "true peak": (dict(true_peak=MEASURE), "true_peak", dict(true_peak=MEASURE, levels=True, loudness=True, envelopes=True, records=True)),
    "rescale": (dict(clip=RESCALE), "levels", dict(clip=RESCALE, levels=True)),
    "rescale on the true peak": (dict(clip=RESCALE, true_peak=TP_RESCALE), "true_peak",
                                 dict(true_peak=TP_RESCALE, clip=RESCALE, levels=True, loudness=True, envelopes=True, records=True)),
}


@pytest.fixture(scope="module")
def engines(pkg, model_small):
    es = {lanes: pkg.Engine.from_file(model_small[0], N, tracks=lanes) if lanes > 1 else pkg.Engine.from_file(model_small[0], N) for lanes in (1, 2, 3)}
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def tracks(pkg):
    x = pkg.ggml.synth_audio(LENGTHS[0] + 2000, 71)
    return [np.ascontiguousarray(x[:, 500 * i:500 * i + n]) for i, n in enumerate(LENGTHS)]


def _io(pkg, fmt):
    return pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, SEED) if fmt == "s16" else pkg.sample_io()


def _same(got, want, what):
    assert len(got) == len(want), what
    for m, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, m, g.shape, w.shape, g.dtype, w.dtype)
        raw = {2: np.uint16, 4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
        bad = np.flatnonzero(g.view(raw).ravel() != w.view(raw).ravel())
        assert bad.size == 0, (what, m, int(bad.size), bad[:4], g.ravel()[bad[:4]], w.ravel()[bad[:4]])


def _call(eng, rung, xs, shifts, rate, io, **kw):
    """one call of a rung of the ladder over the tracks xs -> per track {"outs", "lv", "ld", "env", "tp"} (None: the rung has none, or
    NULL was passed)"""
    common = dict(io=io, shift_offsets=list(shifts), rates=[rate] * len(xs), gains=GAINS)
    if rung == "io":
        r = (eng.separate_many_io(xs, **common),)
    else:
        r = getattr(eng, "separate_many_" + rung)(xs, **common, **kw)
    r = tuple(r) + (None,) * (5 - len(r))
    return [{k: (None if v is None else v[t]) for k, v in zip(("outs", "lv", "ld", "env", "tp"), r)} for t in range(len(xs))]


_CACHE = {}


def _run(engines, driver, rung, xs, rate, fmt, pkg, **kw):
    """a rung over the three tracks through a driver -- "one": a one-lane context, track by track; "three": a three-lane context, one
    call; "alone": track by track on the queue's two-lane context -- computed once per distinct request"""
    key = (driver, rung, rate, fmt, tuple(sorted(kw.items())))
    if key not in _CACHE:
        io = _io(pkg, fmt)
        if driver == "three":
            _CACHE[key] = _call(engines[3], rung, xs, SHIFTS, rate, io, **kw)
        else:
            eng = engines[1 if driver == "one" else 2]
            _CACHE[key] = [_call(eng, rung, [x], [s], rate, io, **kw)[0] for x, s in zip(xs, SHIFTS)]
    return _CACHE[key]


def _records_equal(got, want, what):
    """every record `want` has is byte for byte the one `got` has"""
    for k in ("lv", "ld", "tp"):
        if want[k] is not None:
            assert got[k] is not None and bytes(got[k]) == bytes(want[k]), (what, k)
    if want["env"] is not None:
        assert got["env"] is not None, what
        _same([got["env"]], [want["env"]], (what, "hop energies"))


def _held_to_the_host(pkg, r, plain, rate, what):
    """what a call measured against the host rules over `plain`, the fp32 outputs of the call that measures nothing (measured before
    any encode or divisor: the same for every format and clip mode)"""
    n_out, L = len(plain), plain[0].shape[1]
    hop = (rate + 5) // 10
    hops = L // hop
    if r["env"] is not None:
        want = np.stack([pkg.kweight_hops_host(o, rate) for o in plain])
        assert r["env"].shape == (n_out, 2, hops) == want.shape, (what, r["env"].shape)
        if want.size:
            print("hop energies", what, "largest relative deviation", float(np.max(np.abs(r["env"] - want) / np.maximum(np.abs(want), 1e-300))))
        _same([r["env"]], [want], (what, "hop energies against the host"))
    if r["ld"] is not None:
        ld = r["ld"]
        assert (ld.n_out, ld.hop, ld.hops) == (n_out, hop, hops), (what, ld.n_out, ld.hop, ld.hops)
        for m in range(n_out):
            want = pkg.loudness_gate(pkg.kweight_hops_host(plain[m], rate), hop)
            assert (ld.integrated[m], ld.momentary_max[m], ld.blocks[m], ld.gated[m]) == want, (what, m, want)
        if hops == 0:  # shorter than one hop: the empty report
            assert list(ld.integrated) == [-np.inf] * 4 and list(ld.blocks) == [0] * 4 and list(ld.gated) == [0] * 4, what
    if r["tp"] is not None:
        tp = r["tp"]
        assert (tp.n_out, tp.factor) == (n_out, 4), (what, tp.n_out, tp.factor)
        for m in range(4):
            want = int(pkg.true_peak_host(plain[m], rate)) if m < n_out else 0
            got = int(np.array([tp.true_peak[m]], np.float32).view(np.uint32)[0])
            assert got == want, (what, m, got, want)


def _gain_held(pkg, r, mode, what):
    """the divisor of a rescaled track: rescale_gain of the peaks it comes from"""
    lv = r["lv"]
    peaks = r["tp"].true_peak[:lv.n_out] if mode == TP_RESCALE else lv.peak[:lv.n_out]
    print("rescale", what, "gain", lv.gain, "peaks", list(peaks))
    assert np.float32(lv.gain) == pkg.rescale_gain(peaks), (what, lv.gain, list(peaks))


@pytest.mark.parametrize("ask", list(ASKS))
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("driver", ["one", "three"])
def test_wider_rung_is_the_narrowest(pkg, engines, tracks, driver, rate, fmt, ask):
    wide_kw, rung, narrow_kw = ASKS[ask]
    wide = _run(engines, driver, "true_peak", tracks, rate, fmt, pkg, **wide_kw)
    narrow = wide if rung is None else _run(engines, driver, rung, tracks, rate, fmt, pkg, **narrow_kw)
    plain = _run(engines, driver, "io", tracks, rate, "f32", pkg)
    unscaled = _run(engines, driver, "io", tracks, rate, fmt, pkg)
    rescaled = wide_kw.get("clip", CLAMP) == RESCALE
    for t, (w, n) in enumerate(zip(wide, narrow)):
        what = (driver, rate, fmt, ask, "track", t)
        _same(w["outs"], n["outs"], what)
        _records_equal(w, n, what)
        if not rescaled:  # measuring changes no bit of what leaves
            _same(w["outs"], unscaled[t]["outs"], (what, "against the call that measures nothing"))
        _held_to_the_host(pkg, w, plain[t]["outs"], rate, what)
        if rescaled:
            _gain_held(pkg, w, wide_kw["true_peak"], what)
        # asked for and not: the records that come back
        assert (w["lv"] is not None) == wide_kw.get("levels", False) and (w["ld"] is not None) == wide_kw.get("loudness", False), what
        assert (w["env"] is not None) == wide_kw.get("envelopes", False) and (w["tp"] is not None) == wide_kw["records"], what
    if ask == "all":  # every record of the widest call is the one its own narrower rung returns
        for rung_, kw in (("levels", dict(levels=True)), ("loudness", dict(levels=False, loudness=True, envelopes=True))):
            for t, n in enumerate(_run(engines, driver, rung_, tracks, rate, fmt, pkg, **kw)):
                _records_equal(wide[t], n, (driver, rate, fmt, "all against", rung_, t))
        for t, n in enumerate(_run(engines, driver, "true_peak", tracks, rate, fmt, pkg, **ASKS["true peak"][0])):
            _records_equal(wide[t], n, (driver, rate, fmt, "all against the true peak alone", t))


@pytest.mark.parametrize("ask", list(QUEUE_ASKS))
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("rate", RATES)
def test_queue_job_is_the_one_track_call(pkg, engines, tracks, rate, fmt, ask):
    """three jobs on two lanes: A keeps lane 0 for its three calls, B ends after two and C takes its lane"""
    queue_kw, rung, kw = QUEUE_ASKS[ask]
    eng = engines[2]
    got = eng.separate_queue(tracks, shift_offsets=list(SHIFTS), mix=GAINS, io=_io(pkg, fmt), rates=[rate] * 3, **queue_kw)
    assert eng.queue_calls() == 4  # (the condition: a lane was refilled)
    got = tuple(got) + (None,) * (5 - len(got))
    alone = _run(engines, "alone", rung, tracks, rate, fmt, pkg, **kw)
    plain = _run(engines, "alone", "io", tracks, rate, "f32", pkg)
    for j in range(3):
        what = ("queue", rate, fmt, ask, "job", j)
        q = {k: (None if v is None else v[j]) for k, v in zip(("outs", "lv", "ld", "env", "tp"), got)}
        _same(q["outs"], alone[j]["outs"], what)
        assert q["lv"] is not None
        _records_equal(q, alone[j], what)
        _held_to_the_host(pkg, q, plain[j]["outs"], rate, what)
        if queue_kw.get("clip", CLAMP) == RESCALE:
            _gain_held(pkg, q, queue_kw.get("true_peak", OFF), what)


def test_refusal_precedence_of_options(pkg, engines, tracks):
    """the options of a call are checked in one order on every rung: sample formats, clip mode, gains, true-peak mode; the first that
    is wrong is named, and nothing is written"""
    import ctypes as C
    eng = engines[3]
    bad_gains = np.full(5, np.nan, np.float32)
    good = dict(fmt=pkg.SAMPLE_F32, clip=pkg.CLIP_CLAMP, gains=None, mode=OFF)
    wrong = [("fmt", 9, "sample io"), ("clip", 2, "clip mode"), ("gains", bad_gains, "mix:"), ("mode", 3, "true peak mode")]
    m = pkg._TrackArgs([tracks[1]], pkg.sample_io(), 4, [4033], None)
    for o in m.outs[0]:
        o[:] = 123.0
    for first in range(len(wrong)):  # everything from `first` on is wrong: `first` is named
        a = dict(good, **{k: v for k, v, _ in wrong[first:]})
        io = pkg.sample_io()
        io.out_format = a["fmt"]
        g = None if a["gains"] is None else a["gains"].ctypes.data_as(C.POINTER(C.c_float))
        tp = (pkg.TruePeak * 1)()
        rc = eng.lib.umx_hip_separate_tracks_true_peak(eng.h, 1, m.a, m.n, m.rt, m.sh, 1 if g else 4, g, m.o, 0, C.byref(io), a["clip"], None, None,
                                                       None, a["mode"], tp, None, None)
        assert rc == pkg.ERR_ARG and wrong[first][2] in eng.last_error(), (first, eng.last_error())
        for _, _, later in wrong[first + 1:]:
            assert later not in eng.last_error(), (first, eng.last_error())
        assert all((o == 123.0).all() for o in m.outs[0]) and bytes(tp[0]) == bytes(pkg.TruePeak())
    # UMX_TRUE_PEAK_RESCALE without UMX_CLIP_RESCALE: the last check of all
    io = pkg.sample_io()
    rc = eng.lib.umx_hip_separate_tracks_true_peak(eng.h, 1, m.a, m.n, m.rt, m.sh, 4, None, m.o, 0, C.byref(io), pkg.CLIP_CLAMP, None, None, None,
                                                   TP_RESCALE, None, None, None)
    assert rc == pkg.ERR_ARG and "UMX_CLIP_RESCALE" in eng.last_error(), eng.last_error()
