"""The invariant the three-product form of the two-plane GEMMs rests on (csrc/gemm_planes.h).

csrc/quant_planes.h::quant_planes stores a u16 weight q (model.cpp:610-616: w = q * scale + offset) as two fp16 planes
P_hi = fp16(q - c), P_lo = (q - c) - P_hi, c the tensor's own centre (quant_centre: the zero-weight code, 31 .. 65504; 32896 for a
degenerate scale, and for every tensor before the per-tensor centre), and the kernels form a1 P_hi + a1 P_lo + a2 P_hi but not
a2 P_lo.  That is only as accurate as four products if, for EVERY q and every centre the rule can give,
  * P_hi + P_lo is exactly q - c (the affine map's constants then need no change),
  * P_lo is itself an fp16 number (an integer of at most 16), and
  * |P_lo| <= 2^-11 |P_hi|, so that the product that is not formed is 2^-22 of the sum.
numpy's float16 is IEEE binary16 with round-to-nearest-even: the rounding f16_rne_bits (csrc/quant_planes.h) implements."""
import numpy as np
import pytest


def test_u16_weight_planes_are_exact_and_the_low_plane_is_eleven_bits_down():
    q = np.arange(65536, dtype=np.float64) - 32896.0
    hi = q.astype(np.float16)
    assert np.all(np.isfinite(hi))
    lo = q - hi.astype(np.float64)
    lo16 = lo.astype(np.float16)
    assert np.array_equal(lo16.astype(np.float64), lo)          # the remainder is an fp16 number ...
    assert np.array_equal(lo, np.round(lo)) and np.abs(lo).max() <= 16  # ... an integer of at most 16
    assert np.array_equal(hi.astype(np.float64) + lo16.astype(np.float64), q)  # the planes' sum is the file's integer
    nz = hi != 0
    assert np.all(np.abs(lo[nz]) <= np.abs(hi[nz].astype(np.float64)) * 2.0 ** -11)
    assert np.all(lo[~nz] == 0)
    # the planes of rounds 2-4 (the two bytes) would not do: their low plane is only eight bits down
    old_lo = (np.arange(65536) & 255) - 128.0
    old_hi = 256.0 * ((np.arange(65536) >> 8) - 128.0)
    assert np.array_equal(old_hi + old_lo, q)
    assert np.abs(old_lo).max() == 128 and np.abs(old_lo[old_hi != 0] / old_hi[old_hi != 0]).max() > 2.0 ** -9


def test_u8_weights_need_one_plane():
    q = np.arange(256, dtype=np.float64) - 128.0
    assert np.array_equal(q.astype(np.float16).astype(np.float64), q)


def _u16_plane_invariants(c):
    """-> (all planes finite, sum exact, remainder an fp16 integer of at most 16, remainder eleven bits down) over every code q."""
    q = np.arange(65536, dtype=np.float64) - float(c)
    with np.errstate(over="ignore"):
        hi = q.astype(np.float16)
    finite = bool(np.all(np.isfinite(hi)))
    with np.errstate(invalid="ignore"):
        lo = q - hi.astype(np.float64)
        lo16 = lo.astype(np.float16)
        exact = bool(np.array_equal(hi.astype(np.float64) + lo16.astype(np.float64), q))
        small = bool(np.array_equal(lo16.astype(np.float64), lo) and np.array_equal(lo, np.round(lo)) and np.abs(lo).max() <= 16)
        nz = hi != 0
        down = bool(np.all(np.abs(lo[nz]) <= np.abs(hi[nz].astype(np.float64)) * 2.0 ** -11) and np.all(lo[~nz] == 0))
    return finite, exact, small, down


# both clamps and their neighbours, the zero-weight codes of tests/skewed_weights.py's variants (9039, 50971), a symmetric tensor's
# (32767), the centre of every tensor before the per-tensor rule (32896), and 64 more drawn from the rule's range
CENTRES = [31, 32, 9039, 32767, 32896, 50971, 65503, 65504] + sorted(int(c) for c in np.random.default_rng(7).integers(31, 65505, 64))


@pytest.mark.parametrize("c", CENTRES)
def test_u16_planes_hold_the_three_invariants_at_every_centre_of_the_rule(c):
    assert 31 <= c <= 65504
    assert _u16_plane_invariants(c) == (True, True, True, True), c


def test_where_fp16_of_q_minus_c_stops_being_finite():
    """The clamp 31 .. 65504 keeps |q - c| <= 65504, the largest finite fp16 number.  fp16 rounds to infinity from 65520 on, so the
    first centres that break finiteness are c = 15 (q = 65535) and c = 65520 (q = 0); one code outside the clamp (c = 30, c = 65505:
    |q - c| = 65505 rounds DOWN to 65504, remainder 1) every invariant still holds -- the clamp has a margin of 15 codes, it is not
    the last finite centre."""
    for c in (15, 65520, 0, 65535):
        assert not _u16_plane_invariants(c)[0], c
    for c in (16, 30, 65505, 65519):
        assert _u16_plane_invariants(c) == (True, True, True, True), c


def test_u8_weights_need_one_plane_at_every_centre():
    for c in range(256):
        q = np.arange(256, dtype=np.float64) - c
        assert np.array_equal(q.astype(np.float16).astype(np.float64), q), c
