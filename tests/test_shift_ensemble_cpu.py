"""The shift ensemble's host side: the default offsets, the definition of the mean the GPU tests compare against
(tests/shift_ensemble_ref.py), and the two entry points in the header and in the library."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import shift_ensemble_ref as ser

ROOT = Path(__file__).resolve().parent.parent
MAX_SHIFT, REFERENCE_SHIFT = 22050, 4033


def _formula(k_shifts, first):
    return [(first + k * (MAX_SHIFT // k_shifts)) % MAX_SHIFT for k in range(k_shifts)]


@pytest.mark.parametrize("k_shifts", [1, 2, 10, 64])
def test_default_offsets_follow_the_formula(pkg, k_shifts):
    for first, start in ((None, REFERENCE_SHIFT), (0, 0), (700, 700), (22049, 22049)):
        got = pkg.ensemble_offsets(k_shifts, first)
        assert got == _formula(k_shifts, start), (k_shifts, first)
        assert all(0 <= o < MAX_SHIFT for o in got)
        assert len(set(got)) == k_shifts
    if k_shifts == 1:
        assert pkg.ensemble_offsets(1) == [4033]


def test_default_offsets_refuse_bad_arguments(pkg):
    assert pkg.MAX_SHIFTS == pkg.MAX_TRACKS == 64
    lib = pkg.hip_lib()
    out = (C.c_int * 80)(*([-7] * 80))
    for k_shifts, first in ((0, -1), (-1, -1), (65, -1), (2, 22050), (1, 1 << 20)):
        assert lib.umx_hip_ensemble_offsets(k_shifts, first, out) == pkg.ERR_ARG, (k_shifts, first)
        with pytest.raises(pkg.UmxError) as e:
            pkg.ensemble_offsets(k_shifts, None if first < 0 else first)
        assert e.value.code == pkg.ERR_ARG
    assert lib.umx_hip_ensemble_offsets(2, -1, None) == pkg.ERR_ARG
    assert list(out) == [-7] * 80  # a refused call writes nothing
    assert lib.umx_hip_ensemble_offsets(3, -1, out) == 0 and list(out)[:4] == [4033, 4033 + 7350, 4033 + 14700, -7]


def _awkward(seed, n=4096):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(np.float32)
    tiny = np.array([1, 2, 3, 0x7FFFFF, 0x800000, 0x800001], np.uint32).view(np.float32)  # subnormals, the smallest normals
    a[:12] = np.concatenate([tiny, -tiny])
    a[12:16] = [0.0, -0.0, np.finfo(np.float32).max / 4, -np.finfo(np.float32).max / 4]
    return a


def test_mean_of_one_array_is_that_array_and_of_two_equal_ones_too():
    a = _awkward(1)
    assert np.array_equal(ser.mean_fp32([a]).view(np.uint32), a.view(np.uint32))
    assert np.array_equal(ser.mean_fp32([a, a]).view(np.uint32), a.view(np.uint32))  # (s + s) / 2 is exact, subnormals included
    assert ser.mean_fp32([a, a]).dtype == np.float32


def test_mean_is_summed_left_to_right_in_fp32_and_divided_once():
    a, b, c = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    # (1 + 2^-24) rounds back to 1 (ties to even) twice; the other order first forms 2^-23, which survives
    assert ser.mean_fp32([np.array([a]), np.array([b]), np.array([c])])[0] == np.float32(1.0) / np.float32(3)
    assert ser.mean_fp32([np.array([b]), np.array([c]), np.array([a])])[0] == np.float32(1.0 + 2.0 ** -23) / np.float32(3)
    x = [_awkward(s) for s in (2, 3, 4)]
    want = ((x[0].astype(np.float64) + x[1]).astype(np.float32).astype(np.float64) + x[2]).astype(np.float32)
    assert np.array_equal(ser.mean_fp32(x), (want.astype(np.float64) / 3.0).astype(np.float32))  # double rounding cannot bite: 3 is exact


def test_header_declares_and_library_exports_the_ensemble(pkg):
    header = (ROOT / "include" / "umx_hip.h").read_text()
    assert re.search(r"#define\s+UMX_MAX_SHIFTS\s+UMX_MAX_TRACKS", header)
    assert re.search(r"int\s+umx_hip_ensemble_offsets\(int n_shifts, int first, int \*offsets_out\);", header)
    assert re.search(r"int\s+umx_hip_shift_ensemble\(umx_hip_ctx \*ctx, const float \*audio_host, int length, int rate, int n_shifts, "
                     r"const int \*offsets,", header)
    lib = pkg.hip_lib()
    for name in ("umx_hip_ensemble_offsets", "umx_hip_shift_ensemble"):
        assert name in pkg.HIP_SYMBOLS
        assert getattr(lib, name) is not None
    assert hasattr(pkg.Engine, "separate_ensemble")
