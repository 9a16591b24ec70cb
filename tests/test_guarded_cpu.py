"""The guarded-buffer helper of tests/guarded.py (CPU only): a clean buffer passes, every planted defect is reported where it is, and
the post-guard of every buffer the GPU module hands out covers the furthest store any kernel could issue for its context."""
import numpy as np
import pytest

import guarded as gd
import stage_f64 as sf

HOP = gd.HOP
N_CUS = 256  # MI355X


def _written(layout, seed=0):
    """A buffer as a correct kernel leaves it: guards intact, the payload finite."""
    w = gd.make(layout)
    w[layout.body] = np.random.default_rng(seed).uniform(-1, 1, layout.payload).astype(np.float32).view(np.int32)
    return w


@pytest.mark.parametrize("misalign", [0, 8])
def test_a_clean_buffer_passes(misalign):
    lay = gd.stem_layout(1000, 4096, misalign)
    assert gd.check(_written(lay), lay).ok
    audio = np.random.default_rng(1).uniform(-1, 1, 2000).astype(np.float32)
    before = gd.make(lay, audio)
    assert gd.check(before.copy(), lay, before).ok
    assert gd.untouched(before.copy(), before) is None
    assert str(gd.check(before.copy(), lay, before)) == "clean"


def test_planted_defects_are_reported_where_they_are():
    lay = gd.stem_layout(1000, 4096, 8)
    P = lay.payload
    one = np.int32(np.float32(0.25).view(np.int32))
    cases = {  # word offset from the payload start -> the report it must give
        P: ("post", (P, P, 1)),                            # one word past the payload
        -1: ("pre", (-1, -1, 1)),                          # one word before it
        lay.payload + lay.post - 1: ("post", (P + lay.post - 1,) * 2 + (1,)),  # the far end of the post-guard
        -lay.pre: ("pre", (-lay.pre, -lay.pre, 1)),        # the first word of the allocation
    }
    for off, (field, span) in cases.items():
        w = _written(lay)
        w[lay.pre + off] = one
        r = gd.check(w, lay)
        assert not r.ok and getattr(r, field) == span, (off, str(r))
        assert all(getattr(r, f) is None for f in ("pre", "post", "holes", "nonfinite", "changed") if f != field), (off, str(r))
    # a single hole: reported as a hole (and as non-finite: FILL is a NaN)
    w = _written(lay)
    w[lay.pre + 517] = gd.FILL
    r = gd.check(w, lay)
    assert r.holes == (517, 517, 1) and r.nonfinite == (517, 517, 1) and r.pre is None and r.post is None
    # a written Inf is non-finite but no hole
    w = _written(lay)
    w[lay.pre + 3] = np.float32(np.inf).view(np.int32)
    r = gd.check(w, lay)
    assert r.nonfinite == (3, 3, 1) and r.holes is None
    # a run of overrun words: first, last and count
    w = _written(lay)
    w[lay.pre + P:lay.pre + P + 2048] = one
    assert gd.check(w, lay).post == (P, P + 2047, 2048)
    # inputs / in-place updates: one changed payload word, and an idle lane's buffer with one word written
    audio = np.random.default_rng(2).uniform(-1, 1, P).astype(np.float32)
    before = gd.make(lay, audio)
    w = before.copy()
    w[lay.pre + P - 1] ^= 1
    r = gd.check(w, lay, before)
    assert r.changed == (P - 1, P - 1, 1) and r.pre is None and r.post is None
    idle = gd.make(lay)
    w = idle.copy()
    w[lay.pre + 10] = one
    assert gd.untouched(w, idle) == (lay.pre + 10, lay.pre + 10, 1)


def test_guard_patterns_are_nan_and_distinct():
    g, f = np.array([gd.GUARD, gd.FILL], np.int32).view(np.float32)
    assert np.isnan(g) and np.isnan(f) and gd.GUARD != gd.FILL


def _module_cases():
    """(N, n) of every buffer tests/test_gpu_device_buffers.py hands out, and N of every geometry case."""
    cases = []
    for N, lanes in gd.BATCH_CONTEXTS.values():
        T = gd.n_frames(N)
        cases += [(N, n) for n in gd.ragged_ns(N, *sf.fused_run_split(T, lanes, N_CUS))]
    N = gd.SINGLE_N
    cases += [(N, n) for n in gd.ragged_ns(N, *sf.fused_run_split(gd.n_frames(N), 1, N_CUS))]
    for N in sf.geometries(N_CUS).values():
        for lanes in (1, 3, 64):
            cases += [(N, n) for n in gd.ragged_ns(N, *sf.fused_run_split(gd.n_frames(N), lanes, N_CUS))]
    return cases


def test_every_post_guard_covers_the_furthest_store():
    cases = _module_cases()
    assert len(cases) > 300
    for N, n in cases:
        assert 1 <= n <= N, (N, n)
        T = gd.n_frames(N)
        far = gd.furthest_stem_sample(N)
        assert far >= (T - 2) * HOP - 1 and far >= N + 1024 - 1, (N, far)  # the fused in-loop store and the run-end flush
        for misalign in (0, 8):
            lay = gd.stem_layout(n, N, misalign)
            assert lay.payload == 2 * n
            assert lay.pre * 4 >= 4096 and (lay.pre * 4) % 256 == misalign
            assert lay.total % 64 == 0  # the next allocation starts 256-byte aligned
            end = lay.payload + lay.post  # words from the payload start to the end of the allocation
            assert end >= 2 * (far + 1) and end >= 2 * (N + 2048), (N, n, end)


def test_ragged_ns_hit_the_run_boundaries():
    N, lanes = gd.BATCH_CONTEXTS["T201x3"]
    run_len, nruns = sf.fused_run_split(gd.n_frames(N), lanes, N_CUS)
    assert (run_len, nruns) == (9, 23)
    ns = gd.ragged_ns(N, run_len, nruns)
    for n in (N, N - 1, N - 1023, 2049, 2048, 1025, 1024, 1):
        assert n in ns
    for k in (1, 2, 11, 22):
        b = k * run_len * HOP - 2048
        assert {b - 1, b, b + 1} <= set(ns), k
    assert any(n % HOP == 0 and n + 1 in ns and 2048 < n < N - HOP for n in ns)
    # an end inside a run's first three blocks, a run after the first
    assert any((n + 2048) // HOP % run_len in (1, 2) and (n + 2048) // HOP > run_len for n in ns)
    assert 517 in gd.ragged_ns(4096, *sf.fused_run_split(5, 3, N_CUS))
    calls = gd.lanes_of(ns, 3)
    assert all(len(c) == 3 for c in calls) and sorted(set(sum(calls, []))) == ns
