"""Loudness of every output, the host side: the library's statement of the rule (umx_hip_kweight_coeffs,
umx_hip_kweight_hops_host, umx_hip_loudness_gate -- csrc/loudness.h, the functions the kernel and the drivers use) against
tests/loudness_ref.py, the rule against the full-history filter it stands in for, and the standard's own check signals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import loudness_ref as ref

RATES = (8000, 44100, 48000, 192000)


def _sine(rate, seconds, dbfs, freq=1000.0, channels=(1, 1)):
    t = np.arange(int(round(rate * seconds))) / rate
    s = 10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * freq * t)
    return np.stack([s * channels[0], s * channels[1]]).astype(np.float32)


def _loudness(pkg, x, rate):
    return pkg.loudness_gate(pkg.kweight_hops_host(x, rate), ref.hop_of(rate))


def test_struct_layout_is_the_headers(pkg):
    assert C.sizeof(pkg.Loudness) == 8 * 4 * 4 + 8 + 4 + 4
    assert (pkg.Loudness.momentary_max.offset, pkg.Loudness.blocks.offset, pkg.Loudness.gated.offset) == (32, 64, 96)
    assert (pkg.Loudness.hops.offset, pkg.Loudness.n_out.offset, pkg.Loudness.hop.offset) == (128, 136, 140)


def test_coefficients_are_the_standards_table_at_48k(pkg):
    pb, pa, rb, ra = pkg.kweight_coeffs(48000)
    t = ref.BS1770_48K
    got = list(pb) + list(pa[1:]) + list(ra[1:])
    want = list(t["shelf_b"]) + list(t["shelf_a"]) + list(t["hp_a"])
    assert len(got) == 7
    for g, w in zip(got, want):
        print("coefficient", g, w, abs(g - w))
        assert abs(g - w) <= 1e-12
    assert pa[0] == 1.0 and ra[0] == 1.0 and list(rb) == [1.0, -2.0, 1.0]


@pytest.mark.parametrize("rate", RATES)
def test_coefficients_are_the_references_at_every_rate(pkg, rate):
    for got, want in zip(pkg.kweight_coeffs(rate), ref.coeffs(rate)):
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)  # (tan and pow of two libraries)


def test_coefficients_refuse_a_bad_rate(pkg):
    for rate in (7999, 192001, 0, -1):
        with pytest.raises(pkg.UmxError):
            pkg.kweight_coeffs(rate)
    pkg.kweight_coeffs(8000), pkg.kweight_coeffs(192000)


@pytest.mark.parametrize("rate", RATES)
def test_host_hops_are_the_references_rule(pkg, rate):
    hop = ref.hop_of(rate)
    assert hop == {8000: 800, 44100: 4410, 48000: 4800, 192000: 19200}[rate]
    x = ref.stepped_noise(rate, 7 * hop + 123, rate)
    want = ref.hop_energies(x, rate)
    got = pkg.kweight_hops_host(x, rate)
    assert got.shape == want.shape == (2, 7)
    dev = np.abs(got - want) / ref.tolerance(want)
    print("rate", rate, "largest deviation / tolerance", dev.max(), "relative", (np.abs(got - want) / want).max())
    assert (dev <= 1.0).all()
    # a span of hops is those hops, and nothing else is written
    part = pkg.kweight_hops_host(x, rate, 2, 3)
    assert np.array_equal(part[:, 2:5], got[:, 2:5]) and np.isnan(part[:, :2]).all() and np.isnan(part[:, 5:]).all()


@pytest.mark.parametrize("rate", RATES)
def test_rule_against_the_full_history_filter(pkg, rate):
    hop = ref.hop_of(rate)
    x = ref.stepped_noise(rate, 7 * hop + 123, rate)
    full = ref.gate(ref.hop_energies_full_history(x, rate), hop)
    rule = _loudness(pkg, x, rate)
    print("rate", rate, "integrated: rule", rule[0], "full history", full[0], "difference", abs(rule[0] - full[0]))
    assert abs(rule[0] - full[0]) <= 1e-6
    assert rule[2:] == full[2:]


def test_calibration_997_hz_full_scale_in_one_channel(pkg):
    got = _loudness(pkg, _sine(48000, 5.0, 0.0, 997.0, (1, 0)), 48000)
    print("997 Hz full scale, one channel:", got)
    assert abs(got[0] - -3.01) <= 0.005


def _tech3341(parts):
    return np.concatenate([_sine(48000, s, db) for s, db in parts], axis=1)


def test_ebu_tech_3341_cases_1_3_4(pkg):
    c1 = _loudness(pkg, _tech3341([(20, -23.0)]), 48000)
    c3 = _loudness(pkg, _tech3341([(10, -36.0), (60, -23.0), (10, -36.0)]), 48000)
    c4 = _loudness(pkg, _tech3341([(10, -72.0), (10, -36.0), (60, -23.0), (10, -36.0), (10, -72.0)]), 48000)
    print("Tech 3341 case 1", c1, "case 3", c3, "case 4", c4)
    assert abs(c1[0] - -23.0) <= 0.1
    assert abs(c3[0] - -23.0) <= 0.1
    assert abs(c4[0] - -23.0) <= 0.1
    assert abs(c4[0] - c3[0]) <= 1e-9 and c4[3] == c3[3]  # the absolute gate removes the -72 dBFS blocks
    assert c4[2] == c3[2] + 200


def test_gate_against_the_reference_gate(pkg):
    rng = np.random.default_rng(5)
    for hops in (4, 5, 13, 40):
        E = 4410 * 10.0 ** rng.uniform(-9, -1, (2, hops))
        got, want = pkg.loudness_gate(E, 4410), ref.gate(E, 4410)
        assert got[2:] == want[2:] and abs(got[0] - want[0]) <= 1e-9 and abs(got[1] - want[1]) <= 1e-9, (hops, got, want)


def test_gate_edges(pkg):
    hop = 4410
    ninf = -np.inf
    loud = hop * 0.01  # a hop at mean square 0.01 per channel: -0.691 + 10 log10(0.02) = -17.68 LUFS
    # fewer than four hops: no block
    for hops in (0, 1, 3):
        assert pkg.loudness_gate(np.full((2, hops), loud), hop) == (ninf, ninf, 0, 0)
    # exactly four: one block
    i, m, b, g = pkg.loudness_gate(np.full((2, 4), loud), hop)
    assert (b, g) == (1, 1) and abs(i - (-0.691 + 10 * np.log10(0.02))) < 1e-12 and m == i
    # all silent: blocks, none gated, log10(0) = -inf is no maximum above -inf
    assert pkg.loudness_gate(np.zeros((2, 13)), hop) == (ninf, ninf, 10, 0)
    # below the absolute gate everywhere: a momentary maximum, nothing integrated
    i, m, b, g = pkg.loudness_gate(np.full((2, 13), hop * 1e-9), hop)
    assert i == ninf and (b, g) == (10, 0) and abs(m - (-0.691 + 10 * np.log10(2e-9))) < 1e-9
    # a NaN hop: its four blocks pass no gate and are no maximum
    E = np.full((2, 13), loud)
    E[1, 6] = np.nan
    i, m, b, g = pkg.loudness_gate(E, hop)
    assert (b, g) == (10, 6) and abs(i - (-0.691 + 10 * np.log10(0.02))) < 1e-12 and abs(m - i) < 1e-12
    assert pkg.loudness_gate(E, hop)[2:] == ref.gate(E, hop)[2:]
    # an inf hop: its block passes the absolute gate and is the maximum; the relative gate is then at inf - 10 = inf, which by IEEE
    # comparison no block is above, the inf one included
    E = np.full((2, 13), loud)
    E[0, 0] = np.inf
    assert pkg.loudness_gate(E, hop) == (ninf, np.inf, 10, 0) and ref.gate(E, hop) == (ninf, np.inf, 10, 0)
    E[0, 0] = 1e300  # (finite, however large: it is gated in, alone)
    i, m, b, g = pkg.loudness_gate(E, hop)
    assert (b, g) == (10, 1) and i == m and np.isfinite(i)
    # the relative gate: eight loud blocks, five 30 dB below them (above -70): blocks 13, gated only the loud ones and the mixed ones above the gate
    E = np.concatenate([np.full((2, 8), loud), np.full((2, 8), loud * 1e-3)], axis=1)
    got, want = pkg.loudness_gate(E, hop), ref.gate(E, hop)
    assert got[2] == 13 and got[3] == want[3] and 5 <= got[3] < 13 and abs(got[0] - want[0]) < 1e-9
