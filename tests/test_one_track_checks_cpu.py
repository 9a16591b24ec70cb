"""The float64 checks of tests/test_gpu_one_track_f64.py have teeth at the real widths, without a GPU: the numpy emulation of
gemm_bf16x3_kernel (tests/bf16x3_emu.py) is fed through skewed_weights.cpu_activations and the stage references at hidden 512 and
1024 (fixtures h512_all / h1024_all, T = 24, target 0 -- skewed "high" -- and the control target 3, plain U(-k, k) weights), each
stage held by skewed_weights.check_both exactly as the GPU tests hold the kernel.

  * The complete form passes every stage at every K: at most 0.58 of its bound (measured: fc1 0.33 - 0.45, lstm 0.13 - 0.23,
    fc2 0.46 - 0.51 at K = 1024 and 0.50 - 0.58 at K = 2048, mask 0.17 - 0.22; as a multiple of the float32 evaluation's distance
    0.6 - 2.8).  On an MI355X the kernel measures the same (fc2 at K = 2048: 0.57 - 0.61 of the bound, 2.8 - 3.1 times float32): the
    length of the fp32 accumulation chain at K = 2048 is inside the bound, and the emulation accounts for the kernel's figure.
  * A dropped second-order term, a2 b2 or a3 b1, FAILS fc2 at K = 1024 (hidden 512: 1.6 - 2.0 times the bound) and at K = 2048
    (hidden 1024: 1.34 - 1.76), and a3 p dropped from the one-plane form fails fc1 (K = 2974: 1.4 - 1.8), while its relative L2
    against float64 is 1.6e-6 - 2.2e-6: below test_gpu_batch.REG_STAGE (5e-6) and TOL_STAGE (2e-5), so the comparisons with the fp32
    oracle pass it.
  * The centre fixed at 128 and the row sum over the bf16-rounded a1 fail fc1 on the skewed target (51 - 61 and 6.5 - 7.9 times the
    bound) and the lstm stage behind W_ih (K = 512 / 1024: 1.3 - 2.2 and 17 - 29).  On the control target both are invisible (they
    pass even this check, at 0.45): the oracle comparisons, which run plain synthetic weights only, pass them.  On the skewed target
    they are 8.1e-5 - 8.7e-5 and 5.2e-6 - 5.6e-6 from float64 at fc1, past REG_STAGE -- had an oracle test used such weights it could
    have seen them; none does.
  * Where the check is NOT sharp, recorded and not asserted: the mask (fc3, K = 512 / 1024) sees a dropped term at 0.86 - 1.08 of its
    bound -- relu(bn3 x scale + mean) adds an offset that dilutes the product's error -- and the lstm stage sees a3 p dropped from W_ih
    at 0.75 - 1.09.  fc3 runs the same main loop as fc2 (BQ_U16) under another epilogue, so a fault in the six-term loop's source
    shows at fc2; one confined to fc3's instantiation of it would not be seen at the mask.
"""
import numpy as np
import pytest

import bf16x3_emu as emu
import skewed_weights as sw
import stage_f64 as sf
import test_gpu_batch

T = 24
STAGES = ("fc1", "lstm", "fc2", "mask")
SKEWED, CONTROL = 0, sw.CONTROL_TARGET
U8X, SIX = ("fc1", "lstm"), ("fc2", "mask")  # the stages behind the one-plane form (fc1, W_ih) and behind the six-term form (fc2, fc3)
FAULT_STAGES = {None: STAGES, "drop_a2b2": SIX, "drop_a3b1": STAGES, "centre_128": U8X, "rowsum_a1": U8X}


def _measure(ggml, tmp, H):
    """(target, fault, stage) -> the two rows (arithmetic, parity) of check_both."""
    Hh, fams, targets = sw.make_fixture(ggml, f"h{H}_all", tmp)
    assert Hh == H and fams == sw.ALL
    out = {}
    for t in (SKEWED, CONTROL):
        acts = sw.cpu_activations(ggml, targets[t], H, T)
        fns = sw.stage_functions(H, *acts)
        refs = {k: sw.stage_refs(targets[t], f) for k, f in fns.items()}
        for fault, stages in FAULT_STAGES.items():
            em = emu.one_track_stages(targets[t], H, *acts, fault=fault, stages=stages)
            for k in stages:
                rows = sw.check_both(k, em[k], *refs[k], where=f"[hidden {H}, target {t}, {fault or 'complete'}]")
                assert all(r["gap_ok"] and (r["failure"] is None) == (r["excess"] <= 1.0) for r in rows), rows  # never the caps or the gap
                out[t, fault, k] = rows
                print(f"hidden {H} target {t} {fault or 'complete'} {k}: excess {rows[0]['excess']:.2f} / {rows[1]['excess']:.2f}, "
                      f"rel L2 {rows[0]['rel']:.2e}, ratio to float32 {rows[0]['ratio_rel']:.1f} / {rows[0]['ratio_blk']:.1f}")
    return out


@pytest.fixture(scope="module")
def measured(pkg, tmp_path_factory):
    made = {}

    def get(H):
        if H not in made:
            made[H] = _measure(pkg.ggml, tmp_path_factory.mktemp(f"one_track_cpu_{H}"), H)
        return made[H]
    return get


def _excess(rows):
    return min(r["excess"] for r in rows)


WIDTHS = pytest.mark.parametrize("H", [512, 1024])


def test_split3_is_exact_to_two_to_the_minus_26():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(100_000) * np.exp(rng.uniform(-20, 20, 100_000))).astype(np.float32)
    x1, x2, x3 = emu.split3(x)
    for p in (x1, x2, x3):
        assert not (p.view(np.uint32) & np.uint32(0xFFFF)).any()  # bf16 values
    res = np.abs(x.astype(np.float64) - x1.astype(np.float64) - x2.astype(np.float64) - x3.astype(np.float64))
    assert (res <= 2.0 ** -26 * np.abs(x)).all()
    assert np.array_equal(emu.bf16(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)), np.array([1.0, 1.0 + 2.0 ** -6], np.float32))  # ties to even


def test_products_are_the_products(pkg):
    """Both forms against float64 on random operands: the complete forms to fp32 accuracy, the u8 form whatever the centre."""
    rng = np.random.default_rng(1)
    a = np.tanh(rng.standard_normal((5, 200))).astype(np.float32)  # (K = 200: padded to 208)
    w = rng.uniform(-0.1, 0.1, (7, 200)).astype(np.float32)
    ref = a.astype(np.float64) @ w.astype(np.float64).T
    assert np.abs(emu.product_six(a, w) - ref).max() <= 4e-7 * np.abs(ref).max()
    assert np.abs(emu.product_six(a, w, "drop_a2b2") - ref).max() > 4e-7 * np.abs(ref).max()
    q, s, o = pkg.ggml.quantize(w, np.uint8)
    ref = a.astype(np.float64) @ (q.astype(np.float64) * float(s) + float(o)).T
    for fault in (None, "centre_128"):
        assert np.abs(emu.product_u8x(a, q, s, o, fault) - ref).max() <= 1e-6 * np.abs(ref).max(), fault
    rs = emu.staging_rowsum(np.pad(a, ((0, 0), (0, 8))))
    assert np.abs(rs - a.astype(np.float64).sum(axis=1)).max() <= 1e-5


@WIDTHS
def test_the_complete_form_passes_every_stage(measured, H):
    m = measured(H)
    for t in (SKEWED, CONTROL):
        for k in STAGES:
            for r in m[t, None, k]:
                assert r["failure"] is None and r["excess"] <= 1.0, r


@WIDTHS
@pytest.mark.parametrize("fault", ["drop_a2b2", "drop_a3b1"])
def test_a_dropped_second_order_term_fails_fc2_and_passes_the_oracle_bounds(measured, H, fault):
    """fc2's K is 1024 at hidden 512 and 2048 at hidden 1024; a3 p dropped from the one-plane form also fails fc1 (K = 2974)."""
    m = measured(H)
    for t in (SKEWED, CONTROL):
        for k in ("fc2",) + (("fc1",) if fault == "drop_a3b1" else ()):
            rows = m[t, fault, k]
            assert _excess(rows) > 1.0 and all(r["failure"] and r["failure"].startswith(k) for r in rows), (H, t, k, rows)
        for k in FAULT_STAGES[fault]:  # the fp32 oracle's bounds pass the fault at every stage
            for r in m[t, fault, k]:
                assert r["rel"] < test_gpu_batch.REG_STAGE < test_gpu_batch.TOL_STAGE, (H, t, k, r["rel"])


@WIDTHS
def test_a_fixed_centre_and_a_row_sum_over_rounded_values_fail_on_the_skewed_target_only(measured, H):
    m = measured(H)
    assert _excess(m[SKEWED, "centre_128", "fc1"]) > 10, m[SKEWED, "centre_128", "fc1"]
    assert _excess(m[SKEWED, "rowsum_a1", "fc1"]) > 3, m[SKEWED, "rowsum_a1", "fc1"]
    assert _excess(m[SKEWED, "rowsum_a1", "lstm"]) > 5, m[SKEWED, "rowsum_a1", "lstm"]  # W_ih: K = 512 / 1024
    assert _excess(m[SKEWED, "centre_128", "lstm"]) > 1.0, m[SKEWED, "centre_128", "lstm"]
    for fault in ("centre_128", "rowsum_a1"):
        for k in U8X:  # plain weights: invisible to this check, and all the more to the oracle's bounds
            for r in m[CONTROL, fault, k]:
                assert r["failure"] is None and r["rel"] < test_gpu_batch.REG_STAGE, (H, fault, k, r)
