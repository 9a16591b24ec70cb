"""Output levels and the rescale rule, the host side: the library's restatement of the rules (umx_hip_levels_host,
umx_hip_rescale_gain, csrc/levels.h -- the functions the kernels call) against tests/levels_ref.py bit for bit, and the properties
the rules promise: the record adds up over spans, a rescaled encode never clamps.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import levels_ref as ref
import pcm16_ref as pcm

F32 = np.float32


def _rec(acc, m):
    return {"peak_bits": int(acc.peak_bits[m]), "over_unity": int(acc.over_unity[m]), "clipped": int(acc.clipped[m]),
            "nonfinite": int(acc.nonfinite[m])}


def _want(r):
    return {k: r[k] for k in ("peak_bits", "over_unity", "clipped", "nonfinite")}


def _check(pkg, x, m, first, seed, s16, divisor=1.0):
    io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16 if s16 else pkg.SAMPLE_F32, seed if s16 else None)
    acc = pkg.levels_host(x, m, first, io, divisor)
    want = ref.levels(x, m, first, s16, seed if s16 else None, divisor)
    assert _rec(acc, m) == _want(want), (m, first, seed, s16, divisor)
    for other in range(4):  # exactly buffer m's entries are touched
        if other != m:
            assert _rec(acc, other) == {"peak_bits": 0, "over_unity": 0, "clipped": 0, "nonfinite": 0}
    return want


def test_struct_layouts_are_the_headers(pkg):
    assert C.sizeof(pkg.LevelsAcc) == 112 and pkg.LevelsAcc.over_unity.offset == 16
    assert C.sizeof(pkg.Levels) == 24 + 96 and pkg.Levels.gain.offset == 16 and pkg.Levels.over_unity.offset == 24
    assert (pkg.CLIP_CLAMP, pkg.CLIP_RESCALE) == (0, 1)


def test_fixed_values(pkg):
    one = F32(1.0)
    up = np.nextafter(one, F32(2))
    x = np.array([[0.0, -0.0, 1e-45, one, -one, up, np.nan], [-1e-39, 0.5, -0.75, -up, np.inf, -np.inf, -np.nan]], F32)
    r = _check(pkg, x, 0, 0, None, True)
    assert (r["peak"], r["over_unity"], r["nonfinite"], r["clipped"]) == (np.inf, 4, 4, 2)  # +-up and +-inf are beyond unity; +-up still rounds to +-32767
    r = _check(pkg, x[:, :5], 1, 0, None, True)
    assert (r["peak"], r["over_unity"], r["nonfinite"], r["clipped"]) == (np.inf, 2, 1, 1)
    r = _check(pkg, np.array([[one, 0.5, 0.0], [-0.25, -one, 1e-45]], F32), 2, 0, None, True)  # +-1.0 is code +-32767: not beyond unity, not clamped
    assert (r["peak"], r["over_unity"], r["nonfinite"], r["clipped"]) == (one, 0, 0, 0)
    r = _check(pkg, np.full((2, 3), np.nan, F32), 3, 0, None, True)
    assert (r["peak_bits"], r["over_unity"], r["nonfinite"], r["clipped"]) == (0, 0, 6, 0)
    r = _check(pkg, np.array([[-3.5], [0.25]], F32), 0, 0, None, False)  # negative peak; an fp32 output counts no clipped
    assert (r["peak"], r["over_unity"], r["clipped"]) == (F32(3.5), 1, 0)
    assert _rec(pkg.levels_host(np.zeros((2, 0), F32)), 0)["peak_bits"] == 0


def test_encode_thresholds(pkg):
    """the floats around 32767.5 / 32767 and -32768.5 / 32767: a tie rounds to even, so 32767.5 -> 32768 clamps, -32768.5 -> -32768 does not"""
    hi, lo = pcm.preimage(32767.5), -pcm.preimage(32768.5)
    assert F32(hi * F32(32767.0)) == F32(32767.5) and F32(lo * F32(32767.0)) == F32(-32768.5)
    for x, clipped in ((hi, 1), (np.nextafter(hi, F32(0)), 0), (np.nextafter(hi, F32(2)), 1),
                       (lo, 0), (np.nextafter(lo, F32(0)), 0), (np.nextafter(lo, F32(-2)), 1)):
        a = np.array([[x], [0.0]], F32)
        r = _check(pkg, a, 0, 0, None, True)
        assert r["clipped"] == clipped and r["over_unity"] == 1, (x, r)
        # the count is the clamp's: the encoder's code differs from the rounded value exactly there
        rr = ref.rounded(a)[0, 0]
        assert (F32(pcm.encode(a)[0, 0]) != rr) == bool(clipped)


@pytest.mark.parametrize("seed", [None, 0, 12345])
def test_awkward_and_random_values(pkg, seed):
    x = ref.awkward_floats()
    for m in range(4):
        _check(pkg, x, m, 3, seed, True)
        _check(pkg, x, m, 3, None, False)
    rng = np.random.default_rng(23)
    for m in range(4):
        y = (rng.standard_normal((2, 1 << 16)) * 0.4).astype(F32)
        y[:, ::97] *= 4
        for first in (0, (1 << 31) - 70000):
            r = _check(pkg, y, m, first, seed, True)
            assert r["clipped"] > 0 and r["over_unity"] >= r["clipped"] - 64  # (dither moves a few across the threshold)
        _check(pkg, y, m, 5, seed, True, divisor=1.7)


def test_record_accumulates_over_spans(pkg):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 5000)) * 0.6).astype(F32)
    x[:, [7, 4000]] = [[np.inf, np.nan], [-2.5, 9.0]]
    for seed in (None, 9):
        io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, seed)
        whole = pkg.levels_host(x, 1, 100, io)
        acc = pkg.levels_host(x[:, :1234], 1, 100, io)
        acc = pkg.levels_host(x[:, 1234:], 1, 100 + 1234, io, acc=acc)
        assert _rec(acc, 1) == _rec(whole, 1) == _want(ref.levels(x, 1, 100, True, seed))
        assert _rec(acc, 1) == _want(ref.add(ref.levels(x[:, :1234], 1, 100, True, seed), ref.levels(x[:, 1234:], 1, 1334, True, seed)))
        other = pkg.levels_host(x[:, ::-1], 3, 0, io, acc=acc)  # another buffer into the same record
        assert _rec(other, 1) == _rec(whole, 1) and _rec(other, 3)["nonfinite"] == 2


def test_rescale_gain(pkg):
    inv = F32(1.0) / F32(1.01)
    above = inv  # the two sides of 1 / 1.01: the smallest peak whose fp32 product with 1.01f exceeds 1, and its neighbour below
    while F32(1.01) * above > F32(1.0):
        above = np.nextafter(above, F32(0))
    while not F32(1.01) * above > F32(1.0):
        above = np.nextafter(above, F32(2))
    below = np.nextafter(above, F32(0))
    assert abs(float(above) - 1 / 1.01) < 1e-6
    for p, want in ((0.0, 1.0), (below, 1.0), (above, F32(1.01) * above), (1.0, F32(1.01)), (1.5, F32(1.01) * F32(1.5)), (np.inf, 1.0),
                    (np.nan, 1.0), (1e30, F32(1.01) * F32(1e30))):
        got = pkg.rescale_gain([p])
        assert got.view(np.uint32) == F32(want).view(np.uint32) == ref.gain([p]).view(np.uint32), (p, got, want)
    assert pkg.rescale_gain([0.25, 1.5, 0.5, 0.0]) == F32(1.01) * F32(1.5) == ref.gain([0.25, 1.5, 0.5, 0.0])
    assert pkg.rescale_gain([1.5, np.inf]) == 1.0 and pkg.rescale_gain([1.5, np.nan, 0.1]) == 1.0 == ref.gain([1.5, np.nan, 0.1])
    assert pkg.rescale_gain(np.zeros(0, F32)) == 1.0


def test_a_rescaled_encode_never_clamps(pkg):
    """|x / g| <= 1 / 1.01 up to rounding, so |v| < 32443 and the dither (below 1 in size) cannot reach the clamp: for finite peaks up
    to 1e30 the rescaled record has clipped == 0 and the codes stay inside +-32443"""
    rng = np.random.default_rng(31)
    for peak in (1.0, 1.000001, 1.5, 32.0, 1e5, 1e30):
        x = (rng.uniform(-1, 1, (2, 4096)) * peak).astype(F32)
        x[0, 17], x[1, 4000] = peak, -peak
        g = ref.gain([ref.levels(x)["peak"]])
        assert g > 1 and pkg.rescale_gain([np.abs(x).max()]) == g
        for seed in (None, 0, 77):
            io = pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16, seed)
            acc = pkg.levels_host(x, 2, 11, io, g)
            assert _rec(acc, 2) == _want(ref.levels(x, 2, 11, True, seed, g)) and acc.clipped[2] == 0
            q = pcm.encode(ref.rescaled(x, g), 2, 11, seed)
            assert np.abs(q.astype(np.int32)).max() <= 32443 + 1
            assert np.array_equal(q, pkg.pcm16_encode_host(ref.rescaled(x, g), 2, 11, seed))
    recs, g, left = ref.track([x, 0.25 * x], True, 3, rescale=True)
    assert g == ref.gain([1e30]) and all(r["clipped"] == 0 for r in recs) and recs[0]["over_unity"] > 0


def test_host_entry_point_refuses_bad_arguments(pkg):
    lib = pkg.hip_lib()
    x = np.zeros(4, F32)
    fp = x.ctypes.data_as(pkg._fp)
    acc = pkg.LevelsAcc()
    assert lib.umx_hip_levels_host(None, 2, 0, 0, None, 1.0, C.byref(acc)) == pkg.ERR_ARG
    assert lib.umx_hip_levels_host(fp, 2, 0, 0, None, 1.0, None) == pkg.ERR_ARG
    assert lib.umx_hip_levels_host(fp, 2, 4, 0, None, 1.0, C.byref(acc)) == pkg.ERR_ARG  # buffers are 0 .. 3
    assert lib.umx_hip_levels_host(fp, -1, 0, 0, None, 1.0, C.byref(acc)) == pkg.ERR_ARG
    assert lib.umx_hip_levels_host(fp, 2, 0, -1, None, 1.0, C.byref(acc)) == pkg.ERR_ARG
    assert lib.umx_hip_levels_host(fp, 2, 0, 0, None, 1.0, C.byref(acc)) == 0  # io NULL: an fp32 output
    assert bytes(acc) == bytes(112)


# ---------------------------------------------------------------- the CLIs' environment (host/clip_env.h)
def _run(tool, args, **env):
    import os
    import subprocess
    keep = {k: v for k, v in os.environ.items() if not k.startswith("UMX_")}
    return subprocess.run([str(tool)] + [str(a) for a in args], capture_output=True, text=True, env={**keep, **env}, timeout=120)


def test_cli_environment_parsing(pkg, tmp_path):
    """both tools read UMX_CLIP and UMX_LEVELS before they open a file: a bad value, or a run that cannot offer them, ends with exit
    code 1 and a message that names the variable; a good value gets as far as the missing input file"""
    from pathlib import Path
    cli, batch = Path(pkg.HERE) / "umx-cli", Path(pkg.HERE) / "umx-batch"
    missing = tmp_path / "missing.wav"
    for tool, args in ((cli, ["no-model", missing, tmp_path / "out"]), (batch, ["no-model", tmp_path / "out", missing])):
        for env, word in (({"UMX_CLIP": "limit"}, "UMX_CLIP: need clamp or rescale"), ({"UMX_CLIP": "Rescale"}, "UMX_CLIP"),
                          ({"UMX_LEVELS": "2"}, "UMX_LEVELS: need 0 or 1"), ({"UMX_LEVELS": "yes", "UMX_CLIP": "rescale"}, "UMX_LEVELS")):
            r = _run(tool, args, **env)
            assert r.returncode == 1 and word in r.stderr, (tool, env, r.stderr)
        for env in ({"UMX_CLIP": "rescale", "UMX_LEVELS": "1"}, {"UMX_CLIP": "clamp"}, {"UMX_CLIP": "", "UMX_LEVELS": "0"}, {"UMX_LEVELS": ""}):
            r = _run(tool, args, **env)
            assert r.returncode == 1 and "UMX_CLIP" not in r.stderr and "UMX_LEVELS" not in r.stderr, (tool, env, r.stderr)
        assert not (tmp_path / "out").exists()
    for env in ({"UMX_CLIP": "rescale"}, {"UMX_LEVELS": "1"}):  # as UMX_PCM16: not with the shift ensemble or the per-segment driver
        for other, word in (({"UMX_SHIFTS": "2"}, "UMX_SHIFTS"), ({"UMX_CLI_PER_SEGMENT": "1"}, "UMX_CLI_PER_SEGMENT")):
            r = _run(cli, ["no-model", missing, tmp_path / "out"], **env, **other)
            assert r.returncode == 1 and "UMX_CLIP / UMX_LEVELS" in r.stderr and word in r.stderr, (env, other, r.stderr)
    r = _run(cli, ["no-model", missing, tmp_path / "out"], UMX_CLIP="clamp", UMX_LEVELS="0", UMX_SHIFTS="2")  # neither is asked for
    assert r.returncode == 1 and "UMX_CLIP" not in r.stderr
