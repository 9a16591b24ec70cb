"""tests/poison.py without a GPU: the poison patterns change what they say and nothing else, the reference's STFT (the oracle) turns
non-finite in exactly the frames that read a poisoned sample -- for the finite 3e38 pattern too --, the clean waves of every schedule
of tests/test_gpu_poisoned_lanes.py are finite with finite reference spectra, and every schedule has pipeline_depth + 1 clean calls
behind each poisoned one."""
import numpy as np
import pytest

import poison as ps

FRAMES = (5, 6)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("pattern", ps.PATTERNS)
@pytest.mark.parametrize("n", [5120, 5120 - 62, 6144 - 31])
def test_patterns_change_only_their_samples(pkg, pattern, n):
    clean = pkg.ggml.synth_audio(n, 77)
    before = clean.copy()
    got = ps.apply(pattern, clean, seed=3)
    assert got is not clean and got.dtype == np.float32 and got.shape == clean.shape
    assert np.array_equal(_bits(clean), _bits(before))  # the clean wave is left as it is
    where = ps.poisoned_samples(pattern, n)
    touched = np.zeros((2, n), bool)
    for c, idx in where.items():
        touched[c, idx] = True
    assert touched.any()
    assert np.array_equal(_bits(got)[~touched], _bits(clean)[~touched])  # every other sample bit for bit
    if pattern == "huge":
        assert np.isfinite(got).all() and np.array_equal(np.abs(got), np.full((2, n), ps.HUGE))
        assert (got > 0).any() and (got < 0).any()
    elif pattern == "inf_pair":
        assert got[0, where[0][0]] == np.inf and got[1, where[1][0]] == -np.inf and np.isinf(got).sum() == 2
    else:
        assert np.isnan(got[touched]).all()
    if pattern == "nan_last":
        assert where == {0: [n - 1], 1: [n - 1]}
    if pattern == "nan_mid":
        assert n // 4 < where[0][0] < 3 * n // 4 and list(where) == [0]
    with pytest.raises(ValueError):
        ps.poisoned_samples("nan_first", n)


def test_covering_frames_by_hand():
    N = 5 * 1024  # T = 6; sample s sits at padded position s + 2048, frame f reads padded [1024 f, 1024 f + 4096)
    assert ps.n_frames(N) == 6
    assert ps.covering_frames(N, [2560 + 7]) == [1, 2, 3, 4]  # padded 4615: frames 1 .. 4
    assert ps.covering_frames(N, [0]) == [0, 1, 2]  # padded 2048 and its mirror image 2047
    assert ps.covering_frames(N, [2047]) == [0, 1, 2, 3]  # padded 4095 (frames 0 .. 3) and its mirror image 0 (frame 0)
    assert ps.covering_frames(N, [2048]) == [1, 2, 3, 4]  # padded 4096 exactly: frame 0 ends before it, and no mirror image
    assert ps.covering_frames(N, [N - 1]) == [3, 4, 5]  # padded 7167 and its mirror image 7168
    assert ps.covering_frames(N, [N - 32]) == [3, 4, 5]  # (n = N - 31: the last valid sample; the mirror image is 7199, frames 4 and 5)
    assert ps.poisoned_frames("nan_lane", N - 31, N) == list(range(6)) == ps.poisoned_frames("huge", N - 62, N)


@pytest.mark.parametrize("frames", FRAMES, ids=lambda f: f"T{f + 1}")
@pytest.mark.parametrize("pattern", ps.PATTERNS)
def test_oracle_stft_is_nonfinite_in_exactly_the_covering_frames(pkg, po, pattern, frames):
    N = frames * 1024
    for k, n in enumerate((N, N - 31, N - 124)):
        if pattern == "nan_last" and n == N:
            continue  # (e) is the edge of the zero-padded tail: n < N
        clean = pkg.ggml.synth_audio(n, 300 + k)
        bad = ps.apply(pattern, clean, seed=k)
        if pattern == "huge":
            assert np.isfinite(bad).all()  # it turns non-finite only inside the transform
        any_bad, all_bad = ps.nonfinite_frames(po.stft(bad, N))
        want = set(ps.poisoned_frames(pattern, n, N))
        assert want and want <= set(range(frames + 1))
        assert any_bad == want, (pattern, n, sorted(any_bad), sorted(want))
        assert all_bad == want, (pattern, n, "a covering frame with a finite bin", sorted(want - all_bad))
        ok, _ = ps.nonfinite_frames(po.stft(clean, N))
        assert not ok


def test_flag_words_and_waves_are_the_packages(pkg):
    import test_gpu_sparse_lanes as sl
    assert (ps.FLAG_SOFTMASK, ps.FLAG_LSTM_STEPWISE, ps.FLAG_RESIDUAL) == (pkg.FLAG_SOFTMASK, pkg.FLAG_LSTM_STEPWISE, pkg.FLAG_RESIDUAL)
    assert ps.SKIP(0, 1, 2) == pkg.flags_for_targets(["vocals"]) and ps.SKIP(1) == pkg.FLAG_SKIP_TARGET(1)
    assert ps.ITERS(3) == pkg.FLAG_WIENER_ITERS(3)
    lab = sl.Lab(pkg, None)
    assert np.array_equal(lab.audio(5120, 16, 2), ps.clean_wave(pkg, 5120, 16, 2))
    assert (ps.HOP, ps.NFFT) == (pkg.HOP, pkg.NFFT)


def test_builder_puts_depth_plus_one_clean_calls_behind_every_poisoned_one():
    for depth in (1, 2, 3):
        s = ps.build(range(3), {1: "nan_mid"}, depth)
        (i,) = s.poisoned_calls()
        assert s.clean_calls_behind(i) == depth + 1 and isinstance(s.steps[i + 1], ps.Reset) and s.steps[i + 1].lane == 1
        assert s.counts == {0: depth + 3, 1: depth + 3, 2: depth + 3}
        # the poisoned lane: one clean call, then (behind the reset) a new epoch; its poisoned segment (1) is in neither
        assert s.clean_sequence(1) == (((0, 0, False),), tuple((k, 0, False) for k in range(2, depth + 3)))
        assert s.clean_sequence(0) == (tuple((k, 0, False) for k in range(depth + 3)),)
        assert s.reference_index(i, 0) == (0, 1) and s.reference_index(i + 2, 1) == (1, 0)
    with pytest.raises(AssertionError, match="too few clean calls"):
        ps.build(range(3), {1: "nan_mid"}, 2, behind=2)
    with pytest.raises(AssertionError, match="not reset"):
        ps.PoisonSchedule([ps.Call(frozenset({0, 1}), {1: "nan_lane"}, 0, False)] + [ps.Call(frozenset({0}), {}, 0, False)] * 3, 2)
    with pytest.raises(AssertionError, match="before its reset"):
        ps.PoisonSchedule([ps.Call(frozenset({0, 1}), {1: "nan_lane"}, 0, False), ps.Call(frozenset({0, 1}), {}, 0, False)], 2)
    with pytest.raises(AssertionError, match="not poisoned"):
        ps.PoisonSchedule([ps.Call(frozenset({0, 1}), {}, 0, False), ps.Reset(1)], 2)
    s = ps.build(range(4), {3: "huge"}, 2, behind_active=[{0, 1}], behind_flags=[None, ps.ITERS(2)], behind_short=True)
    assert [sorted(c.active) for c in s.steps if isinstance(c, ps.Call)] == [[0, 1, 2, 3]] * 2 + [[0, 1], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert [c.flags for c in s.steps if isinstance(c, ps.Call)] == [0, 0, 0, ps.ITERS(2), 0]
    assert [c.short for c in s.steps if isinstance(c, ps.Call)] == [False, False, True, True, True]
    assert s.clean_sequence(3) == ((((0, 0, False)),), ((2, ps.ITERS(2), True), (3, 0, True)))  # idle in the sparse call


def test_every_schedule_of_the_gpu_file(pkg, po):
    cat = ps.catalogue()
    assert len(cat) >= 20
    patterns_by_kernel = {}
    seen_waves = set()
    for name, e in cat.items():
        s = e.schedule
        assert s.depth == ps.PIPELINE_DEPTH
        assert max(s.lanes()) < e.tracks <= 64
        for i in s.poisoned_calls():
            assert s.clean_calls_behind(i) >= ps.PIPELINE_DEPTH + 1, name
            patterns_by_kernel.setdefault((e.kernel, e.tracks == 1), set()).update(s.steps[i].poison.values())
        for frames in FRAMES:  # every clean wave is finite and so is its reference spectrum (each distinct wave once)
            N = frames * 1024
            for ln in s.lanes():
                for k in range(s.counts[ln]):
                    if (N, ln, k) in seen_waves:
                        continue
                    seen_waves.add((N, ln, k))
                    w = ps.clean_wave(pkg, N, ln, k)
                    assert w.shape[1] <= N and np.isfinite(w).all()
                    assert not ps.nonfinite_frames(po.stft(w, N))[0], (name, N, ln, k)
            for i in s.poisoned_calls():  # (e) needs n < N: the edge of the zero-padded tail
                for ln, pattern in s.steps[i].poison.items():
                    n = ps.clean_wave(pkg, N, ln, s.segment[i][ln]).shape[1]
                    assert pattern != "nan_last" or n < N, (name, ln)
    # every pattern at least once per kernel family
    for fam in ((ps.BG, False), (ps.B8, False)):
        assert patterns_by_kernel[fam] == set(ps.PATTERNS), (fam, patterns_by_kernel[fam])
    assert patterns_by_kernel[(ps.P1, True)] >= {"nan_mid", "inf_pair", "nan_lane", "huge"}


def test_schedules_reach_the_lane_positions_they_are_named_for():
    """Through tests/lane_masks.py: the group and octet a poisoned lane falls into, and how many octets a workgroup serves in turn."""
    import lane_masks as lm
    cat = ps.catalogue()

    def plan(name):
        e = cat[name]
        (i,) = e.schedule.poisoned_calls()
        call = e.schedule.steps[i]
        return lm.lstm_launch_plan(e.hidden, call.active), call

    for name, groups, nbp in (("h128_3_nan_mid", [0], 4), ("h256_3_nan_last", [0], 4), ("h128_17_inf_pair", [0, 1], 16), ("h256_17_huge", [0, 1], 16)):
        p, call = plan(name)
        assert (p.kernel, p.groups, p.nbp) == (ps.BG, groups, nbp), name  # one group with the small layout, two with the full one
    assert set(plan("h128_17_inf_pair")[1].poison) == {16} == set(plan("h256_17_huge")[1].poison)  # the first lane of the second group
    a, b = sorted(plan("h256_17_two_in_a_group")[1].poison)
    assert a // lm.GROUP_TRACKS == b // lm.GROUP_TRACKS
    for name, octs, on in (("h512_8_nan_lane_first", 1, [0]), ("h512_8_inf_pair_last", 1, [0]), ("h512_9_huge_second_octet", 1, [0, 1]),
                           ("h1024_33_nan_mid_31", 2, [0, 1, 2, 3]), ("h1024_33_nan_last_32", 2, [0, 1, 2, 3]),
                           ("h1024_64_pair_boundary_and_last", 2, [0, 1, 2, 3])):
        p, call = plan(name)
        assert p.kernel == ps.B8 and p.octs == octs and len(p.launches) == 1, name
        assert [k for k, pair in enumerate(p.launches[0][2]) if not lm.returns_early(pair)] == on, name
    # 33 lanes: lanes 0 .. 7 and lane 32 are the two octets of workgroup-octet 0, the other three serve their first octet only
    assert lm.workgroup_pairs(plan("h1024_33_nan_mid_31")[0]) == [(True, True)] + [(True, False)] * 3
    assert sorted(plan("h512_8_nan_lane_first")[1].poison) == [0] and sorted(plan("h512_8_inf_pair_last")[1].poison) == [7]
    assert sorted(plan("h512_9_huge_second_octet")[1].poison) == [8]
    assert sorted(plan("h1024_64_pair_boundary_and_last")[1].poison) == [31, 32, 63]
    for name in ("h512_9_two_in_an_octet", "h1024_64_two_in_an_octet"):
        call = plan(name)[1]
        a, b = sorted(call.poison)
        assert a // lm.LSTM8_TRACKS == b // lm.LSTM8_TRACKS and sorted(call.poison.values()) == ["nan_lane", "nan_mid"]
    # the sparse calls leave the poisoned lane's group / octet out of the launch
    e = cat["sparse_h256_17"]
    assert lm.lstm_launch_plan(256, e.schedule.steps[3].active).groups == [0] and 16 not in e.schedule.steps[3].active
    e = cat["sparse_h1024_64"]
    assert e.schedule.steps[3].active == {3, 63} and lm.workgroup_pairs(lm.lstm_launch_plan(1024, {3, 63})) == [(True, False), (False, False), (False, False), (False, True)]


def test_not_vacuous_covers_every_pattern_and_recurrence():
    import lane_masks as lm
    cat = ps.catalogue()
    pats, kinds = set(), set()
    for nm in ps.NOT_VACUOUS:
        (i,) = cat[nm].schedule.poisoned_calls()
        call = cat[nm].schedule.steps[i]
        pats |= set(call.poison.values())
        kinds.add((cat[nm].kernel, cat[nm].tracks == 1, bool(call.flags & ps.FLAG_LSTM_STEPWISE),
                   lm.lstm_launch_plan(cat[nm].hidden, call.active).octs if cat[nm].tracks > 1 else 0))
    assert pats == set(ps.PATTERNS)
    assert kinds == {(ps.BG, False, False, 1), (ps.B8, False, False, 1), (ps.B8, False, False, 2), (ps.P1, True, False, 0), (ps.P1, True, True, 0)}
    assert ps.AGAINST_F64 in cat and cat[ps.AGAINST_F64].hidden == 512 and ps.AGAINST_F64 not in ps.NOT_VACUOUS
