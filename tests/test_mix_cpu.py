"""The stem mix matrix's host side: the definition the GPU tests compare against (tests/mix_ref.py), the column mask
(umx_hip_mix_columns), the UMX_MIX grammar (umx_mix_parse of the host library), and the entry points in the headers, the libraries
and the Python package."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import mix_ref as mr

ROOT = Path(__file__).resolve().parent.parent
FP = C.POINTER(C.c_float)
f32 = np.float32


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _awkward(seed, n=4096):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(np.float32)
    tiny = np.array([1, 2, 3, 0x7FFFFF, 0x800000, 0x800001], np.uint32).view(np.float32)  # subnormals, the smallest normals
    a[:12] = np.concatenate([tiny, -tiny])
    a[12:16] = [0.0, -0.0, np.finfo(np.float32).max / 4, -np.finfo(np.float32).max / 4]
    return a


# ---------------------------------------------------------------- the reference itself
def test_terms_are_added_left_to_right():
    one, eps = np.array([1.0], f32), np.array([2.0 ** -24], f32)
    row = [[1, 1, 1, 0, 0]]
    # (1 + 2^-24) rounds back to 1 (ties to even) twice; the other order first forms 2^-23, which survives
    assert mr.mix_fp32([one, eps, eps, None], None, row)[0][0] == f32(1.0)
    assert mr.mix_fp32([eps, eps, one, None], None, row)[0][0] == f32(1.0 + 2.0 ** -23)
    # ascending COLUMN order, the mixture last, whatever the row looks like
    assert mr.mix_fp32([None, eps, None, eps], one, [[0, 1, 0, 1, 1]])[0][0] == f32(1.0 + 2.0 ** -23)
    x = [_awkward(s) for s in (2, 3, 4)]
    want = ((x[0].astype(np.float64) + x[1]).astype(f32).astype(np.float64) + x[2]).astype(f32)
    assert np.array_equal(_bits(mr.mix_fp32([x[0], None, x[1], x[2]], None, [[1, 0, 1, 1, 0]])[0]), _bits(want))


def test_product_is_rounded_before_the_add():
    g, s = f32(1.0 + 2.0 ** -12), np.array([1.0 + 2.0 ** -12], f32)
    a = np.array([1.0 + 2.0 ** -11], f32)
    exact = float(g) * float(s[0])  # 1 + 2^-11 + 2^-24: a tie, rounds to 1 + 2^-11
    assert exact == 1.0 + 2.0 ** -11 + 2.0 ** -24 and f32(exact) == a[0]
    got = mr.mix_fp32([a, s, None, None], None, [[-1, g, 0, 0, 0]])[0][0]
    fused = f32(exact - float(a[0]))  # what fma(g, s, -a) would give
    assert got == f32(0.0) and fused == f32(2.0 ** -24) and got != fused
    # gains in general: two roundings, against float64 (a product of two float32 is exact in float64)
    x, y = _awkward(5), _awkward(6)
    gx, gy = f32(0.7), f32(-1.3)
    with np.errstate(all="ignore"):
        px = (np.float64(gx) * x.astype(np.float64)).astype(f32)
        py = (np.float64(gy) * y.astype(np.float64)).astype(f32)
        want = (px.astype(np.float64) + py.astype(np.float64)).astype(f32)
    assert np.array_equal(_bits(mr.mix_fp32([x, y, None, None], None, [[gx, gy, 0, 0, 0]])[0]), _bits(want))


def test_zero_gains_skip_their_columns_and_minus_zero_is_zero():
    a = _awkward(7)
    bad = np.full_like(a, np.nan)
    bad[::2] = np.inf
    for zero in (0.0, -0.0):
        out = mr.mix_fp32([a, bad, bad, bad], bad, [[2, zero, zero, zero, zero], [zero] * 5])
        assert np.array_equal(_bits(out[0]), _bits(f32(2) * a))
        assert np.array_equal(_bits(out[1]), np.zeros(a.size, np.uint32))  # an empty row: +0.0, not -0.0
    assert mr.mix_fp32([a, None, None, None], None, [[-0.0, 0, 0, 0, 0]])[0].dtype == np.float32


def test_first_term_is_the_product_itself():
    z = np.array([-0.0, 0.0], f32)
    out = mr.mix_fp32([None, None, z, None], None, [[0, 0, 1, 0, 0]])[0]
    assert np.array_equal(_bits(out), _bits(z))  # 0 + (-0) would be +0
    assert np.array_equal(_bits(mr.mix_fp32([None, None, z, None], None, [[0, 0, -1, 0, 0]])[0]), _bits(-z))


def test_subnormals_survive_and_the_identity_is_exact():
    stems = [_awkward(s) for s in (8, 9, 10, 11)]
    mix = _awkward(12)
    out = mr.mix_fp32(stems, mix, mr.IDENTITY)
    assert len(out) == 4
    for t in range(4):
        assert np.array_equal(_bits(out[t]), _bits(stems[t])), t
    tiny = np.array([1, 2, 3], np.uint32).view(np.float32)
    assert np.array_equal(_bits(mr.mix_fp32([tiny, tiny, None, None], None, [[1, 1, 0, 0, 0]])[0]), np.array([2, 4, 6], np.uint32))
    assert np.array_equal(_bits(mr.mix_fp32([tiny, None, None, None], None, [[0.5, 0, 0, 0, 0]])[0]), np.array([0, 1, 2], np.uint32))  # ties to even
    acc = mr.mix_fp32(stems, mix, mr.AGGREGATE)
    assert np.array_equal(_bits(acc[0]), _bits(stems[3])) and np.array_equal(_bits(acc[1]), _bits((stems[0] + stems[1]) + stems[2]))
    assert np.array_equal(_bits(mr.mix_fp32(stems, mix, mr.KARAOKE)[0]), _bits(-stems[3] + mix))


# ---------------------------------------------------------------- umx_hip_mix_columns
def _columns(lib, n_out, gains):
    g = None if gains is None else np.ascontiguousarray(gains, np.float32).ravel()
    return lib.umx_hip_mix_columns(n_out, None if g is None else g.ctypes.data_as(FP))


def test_mix_columns_masks(pkg):
    lib = pkg.hip_lib()
    assert _columns(lib, 4, mr.IDENTITY) == 0b01111 == pkg.mix_columns(mr.IDENTITY)
    assert _columns(lib, 2, mr.AGGREGATE) == 0b01111
    assert _columns(lib, 1, mr.AGGREGATE[1:]) == 0b00111 == pkg.mix_columns(mr.AGGREGATE[1:])
    assert _columns(lib, 1, mr.KARAOKE) == 0b11000 == pkg.mix_columns(mr.KARAOKE)
    assert _columns(lib, 1, [[0, -0.0, 0, 0, 0]]) == 0  # -0 counts as zero
    assert _columns(lib, 2, [[0, 0, 0, 0, 1e-45], [0, -0.5, 0, 0, 0]]) == 0b10010  # a subnormal gain is a gain


def test_mix_columns_refusals(pkg):
    lib = pkg.hip_lib()
    five = np.zeros((5, 5), np.float32)
    assert _columns(lib, 0, five) == -1 and _columns(lib, 5, five) == -1 and _columns(lib, -1, five) == -1
    assert _columns(lib, 1, None) == -1
    for bad in (np.inf, -np.inf, np.nan):
        g = mr.IDENTITY.copy()
        g[3, 4] = bad
        assert _columns(lib, 4, g) == -1, bad
        assert _columns(lib, 3, g) == 0b00111  # (the row that holds it is not part of a 3-row matrix)
        with pytest.raises(pkg.UmxError) as e:
            pkg.mix_columns(g)
        assert e.value.code == pkg.ERR_ARG
    with pytest.raises(ValueError):
        pkg.mix_columns(np.zeros((2, 4), np.float32))


# ---------------------------------------------------------------- umx_mix_parse
EXAMPLE = "vocals=vocals;accompaniment=bass+drums+other;karaoke=mix-vocals;quiet=mix-0.5*vocals"


def test_parse_the_examples(pkg):
    names, gains = pkg.mix_parse(EXAMPLE)
    assert names == ["vocals", "accompaniment", "karaoke", "quiet"]
    assert gains.dtype == np.float32 and gains.shape == (4, 5)
    assert gains.tolist() == [[0, 0, 0, 1, 0], [1, 1, 1, 0, 0], [0, 0, 0, -1, 1], [0, 0, 0, -0.5, 1]]
    names, gains = pkg.mix_parse("a-1_B = -drums + 1e-3*bass - .25*mix")
    assert names == ["a-1_B"] and gains.tolist() == [[f32(1e-3), -1, 0, 0, f32(-0.25)]]
    names, gains = pkg.mix_parse("x=+2*other")
    assert names == ["x"] and gains.tolist() == [[0, 0, 2, 0, 0]]
    assert pkg.mix_parse("n" * 63 + "=mix")[0] == ["n" * 63]
    # <number>: digits, one '.', an exponent; nearest float; a zero written as zero stays a (zero) gain
    assert pkg.mix_parse("x=1E2*mix-5.*bass+.5e+1*drums+0*other-0.0*vocals")[1].tolist() == [[-5, 5, 0, -0.0, 100]]
    assert pkg.mix_parse("x=0.1*mix")[1][0, 4] == f32(0.1) and pkg.mix_parse("x=1e-45*mix")[1][0, 4] == f32(1e-45)  # (a subnormal is not zero)
    assert pkg.mix_parse("x=3.4028235e38*mix")[1][0, 4] == np.finfo(np.float32).max


def test_parse_residual_needs_a_slot(pkg):
    names, gains = pkg.mix_parse("rest=residual;v=vocals-0.5*residual", residual_slot=0)
    assert names == ["rest", "v"] and gains.tolist() == [[1, 0, 0, 0, 0], [-0.5, 0, 0, 1, 0]]
    assert pkg.mix_parse("rest=residual", residual_slot=2)[1].tolist() == [[0, 0, 1, 0, 0]]
    with pytest.raises(pkg.HostError) as e:
        pkg.mix_parse("rest=residual")
    assert "UMX_MIX" in str(e.value) and "rest=residual" in str(e.value)
    with pytest.raises(pkg.HostError) as e:  # the residual's slot IS bass's column here
        pkg.mix_parse("x=bass+residual", residual_slot=0)
    assert "UMX_MIX" in str(e.value)


@pytest.mark.parametrize("spec, piece", [
    ("x=guitar", "guitar"),                       # unknown source
    ("x=vocals+vocals", "vocals"),                # duplicate source
    ("x=mix-0.5*mix", "mix"),
    ("x=vocals;x=drums", "x"),                    # duplicate name
    ("a=mix;b=mix;c=mix;d=mix;e=mix", "e=mix"),   # five outputs
    ("x=", "x="),                                 # empty expression
    ("x=vocals;", ""),                            # ... and an empty output
    ("", ""),
    ("x=0.5.5*vocals", "x=0.5.5*vocals"),         # bad numbers
    ("x=abc*vocals", "abc*vocals"),
    ("x=1e99*vocals", "x=1e99*vocals"),
    ("x=0.5vocals", "x=0.5vocals"),
    ("x=0x10*mix", "x=0x10*mix"),                 # decimal literals only
    ("x=1e-50*mix", "x=1e-50*mix"),               # a nonzero literal that rounds to zero would drop the term silently
    ("x=0.0000000000000000000000000000000000000000000000001*mix", "0000001*mix"),
    ("x=1e*mix", "x=1e*mix"),
    ("x=1.5e+*mix", "x=1.5e+*mix"),
    ("x=.*mix", "x=.*mix"),
    ("x=1,5*mix", "x=1,5*mix"),
    ("x=inf*mix", "inf*mix"),
    ("x=nan*mix", "nan*mix"),
    ("x=2*", "x=2*"),
    ("x=vocals drums", "vocalsdrums"),            # (blanks are dropped: one unknown source)
    ("x=-", "x=-"),
    ("x=--vocals", "x=--vocals"),
    ("bad name!=mix", "badname!"),                # bad names
    ("=mix", ""),
    ("n" * 64 + "=mix", "n" * 64),
    ("vocals", "vocals"),                         # no '='
])
def test_parse_refusals_name_the_variable_and_the_piece(pkg, spec, piece):
    with pytest.raises(pkg.HostError) as e:
        pkg.mix_parse(spec)
    assert "UMX_MIX" in str(e.value) and piece in str(e.value), str(e.value)


def test_parse_refusal_writes_nothing(pkg):
    lib = pkg.host_lib()
    n_out = C.c_int(-7)
    names = C.create_string_buffer(b"\x55" * 256, 256)
    gains = np.full(20, 9.0, np.float32)
    err = C.create_string_buffer(256)
    assert lib.umx_mix_parse(b"a=mix;b=nothing", -1, C.byref(n_out), names, gains.ctypes.data_as(FP), err) == pkg.ERR_ARG
    assert n_out.value == -7 and names.raw == b"\x55" * 256 and (gains == 9.0).all() and b"UMX_MIX" in err.value
    assert lib.umx_mix_parse(None, -1, C.byref(n_out), names, gains.ctypes.data_as(FP), err) == pkg.ERR_ARG
    assert lib.umx_mix_parse(b"a=mix", -1, C.byref(n_out), names, gains.ctypes.data_as(FP), None) == 0
    assert n_out.value == 1 and names.raw[:2] == b"a\0" and gains[4] == 1.0 and (gains[:4] == 0).all() and (gains[5:] == 0).all()


# ---------------------------------------------------------------- the surface
def test_headers_declare_libraries_export_and_python_offers_the_mix(pkg):
    hip_h = (ROOT / "include" / "umx_hip.h").read_text()
    host_h = (ROOT / "include" / "umx_host.h").read_text()
    assert re.search(r"#define\s+UMX_MAX_MIX_OUTPUTS\s+4\b", hip_h)
    assert re.search(r"int\s+umx_hip_mix_columns\(int n_out, const float \*gains\);", hip_h)
    assert re.search(r"int\s+umx_hip_separate_tracks_mix\(umx_hip_ctx \*ctx, int n_tracks, const float \*const \*audio_host, const int \*length, "
                     r"const int \*rate,\s+const int \*shift_offset, int n_out, const float \*gains, float \*const \*out_host, unsigned flags,", hip_h)
    assert re.search(r"int\s+umx_hip_shift_ensemble_mix\(umx_hip_ctx \*ctx, const float \*audio_host, int length, int rate, int n_shifts, "
                     r"const int \*offsets, int n_out,\s+const float \*gains, float \*const \*out_host, unsigned flags,", hip_h)
    assert re.search(r"int\s+umx_hip_mix_stems_device\(umx_hip_ctx \*ctx, int n_out, const float \*gains, const float \*const stems_dev\[4\], "
                     r"const float \*mix_dev, int n,\s+float \*const \*out_dev, void \*hip_stream\);", hip_h)
    assert re.search(r"int\s+umx_mix_parse\(const char \*spec, int residual_slot,", host_h)
    hip, host = pkg.hip_lib(), pkg.host_lib()
    for name in ("umx_hip_mix_columns", "umx_hip_separate_tracks_mix", "umx_hip_shift_ensemble_mix", "umx_hip_mix_stems_device"):
        assert name in pkg.HIP_SYMBOLS
        assert getattr(hip, name) is not None
    assert "umx_mix_parse" in pkg.HOST_SYMBOLS and host.umx_mix_parse is not None
    for method in ("separate_mix", "separate_many_mix", "mix_stems_device", "separate_ensemble"):
        assert hasattr(pkg.Engine, method), method
    import inspect
    assert "gains" in inspect.signature(pkg.Engine.separate_ensemble).parameters
    assert list(inspect.signature(pkg.Engine.separate_mix).parameters)[1:] == ["wave", "gains", "flags", "shift_offset", "rate"]
    assert callable(pkg.mix_columns) and callable(pkg.mix_parse)
    assert pkg.MAX_MIX_OUTPUTS == 4
