"""Sparse sets of active track lanes at the widths that ship (hidden 256 / 512 / 1024).  The track queue leaves lanes idle in
arbitrary positions, and everything one call launches follows from its lane mask (tests/lane_masks.py restates it): how many octets a
workgroup of lstm_batch8_kernel serves in turn, which of them are absent, which workgroups return right after the census, which parts
or 16-lane groups are not launched at all, the LDS layout of lstm_batch_kernel, and over which runs of consecutive lanes -- hence with
which tile kind -- the plane GEMMs go.  A lane's bits must not depend on any of it.

Every schedule here is a few calls on ONE context: all lanes, then the pattern, then another pattern or all lanes again, so that lanes
leave and return and their state is carried across a change of kernel instantiation.  A lane's k-th active call consumes that lane's
k-th segment.  The reference of a lane is its segment sequence ALONE on a one-lane context of the same model (tracks=1, the batched
recurrence, plane GEMMs), computed once per lane and shared by all schedules.  Per call:
  (a) every active lane's stems and its carried state after the call are the reference's, bit for bit;
  (b) an idle lane's entry is None and its state is bitwise what it was before the call;
  (c) a plain call ran the persistent recurrence;
  (d) the model of tests/lane_masks.py confirms that the schedule contains the condition it is named for.
Bitwise equality cannot see an error the sparse call and its reference share, so the pattern calls of three schedules are also held to
float64 stage by stage (tests/stage_f64.py, C_DEFAULT and FLOOR as everywhere), and the queue runs on the octet kernel against
Engine.separate of every job alone.  Segments of 5 and 6 hops (T = 6 and 7: the end rows of the forward and the backward chains differ).

UMX_STAGE_F64_REPORT=<file>: append every float64 check's distances to that file (JSON lines)."""
import os

import numpy as np
import pytest

import lane_masks as lm
import stage_f64 as sf
from test_gpu_geometry_f64 import _finish, check_front_back, check_network
from test_gpu_queue import LENGTHS, SHIFTS, _bits_equal, _padded

pytestmark = pytest.mark.gpu

FRAMES = (5, 6)
MODEL_SEED = 91
R = lambda a, b: set(range(a, b + 1))  # noqa: E731  (lanes a .. b)


class Lab:
    """One model per width, one sparse context at a time (kept while consecutive tests ask for the same one), the one-lane reference
    contexts and the references they gave: computed once, never changed."""

    def __init__(self, pkg, directory):
        self.pkg, self.dir = pkg, directory
        self.models, self.refs, self.ref_engines = {}, {}, {}
        self.key, self.eng = None, None
        self.waves = {}

    def model(self, hidden):
        if hidden not in self.models:
            path = str(self.dir / f"m{hidden}.bin")
            self.pkg.ggml.write_model(path, self.pkg.ggml.synth_weights(hidden, seed=MODEL_SEED), hidden, compress=False)
            self.models[hidden] = (path, self.pkg.ggml.read_model(path)[1])
        return self.models[hidden]

    @staticmethod
    def env_key():
        return os.environ.get("UMX_LSTM8_PAIRED"), os.environ.get("UMX_LSTM8_MIN_LANES")

    def engine(self, hidden, N, B):
        """The sparse context (the two environment variables are read when it is created: they are part of its key)."""
        key = (hidden, N, B) + self.env_key()
        if key != self.key:
            if self.eng is not None:
                self.eng.close()
            self.key, self.eng = None, None
            self.eng = self.pkg.Engine(self.model(hidden)[1], hidden, N, tracks=B)
            self.key = key
        self.eng.track_stream_reset(-1)
        return self.eng

    def audio(self, N, lane, k):
        key = (N, lane, k)
        if key not in self.waves:
            self.waves[key] = self.pkg.ggml.synth_audio(N - 31 * ((lane + 2 * k) % 5), 9000 + 8 * lane + k)
        return self.waves[key]

    def reference(self, hidden, N, flags, lane, count, kernel):
        """[(stems, state after)] of the lane's first `count` segments alone, from a zero state."""
        min_lanes = self.env_key()[1]
        key = (hidden, N, min_lanes, flags, lane)
        if len(self.refs.get(key, ())) < count:
            ek = (hidden, N, min_lanes)
            if ek not in self.ref_engines:
                self.ref_engines[ek] = self.pkg.Engine(self.model(hidden)[1], hidden, N, tracks=1, lstm_batched=True, gemm="planes")
            one = self.ref_engines[ek]
            one.track_stream_reset(-1)
            out = []
            for k in range(count):
                stems = one.infer_batch([self.audio(N, lane, k)], flags)[0]
                out.append((stems, one.track_stream_get(0)))
            assert one.lstm_kernel_name() == kernel and one.lstm_was_persistent()  # the same form of the recurrence as the sparse context
            self.refs[key] = out
        return self.refs[key]

    def close(self):
        for e in [self.eng] + list(self.ref_engines.values()):
            if e is not None:
                e.close()
        self.eng, self.key, self.ref_engines = None, None, {}


@pytest.fixture(scope="module")
def lab(pkg, tmp_path_factory):
    lb = Lab(pkg, tmp_path_factory.mktemp("sparse_lanes"))
    yield lb
    lb.close()


@pytest.fixture(scope="module", params=FRAMES, ids=lambda f: f"T{f + 1}")
def frames(request):
    """Hops per segment.  Module scope: the tests of one length run together, on the contexts that length already has."""
    return request.param


@pytest.fixture(scope="module")
def n_cus():
    import torch
    torch.zeros(1).cuda()
    return sf.device_cu_count(0)


def _env(monkeypatch, paired=None, min_lanes=None):
    for name, v in (("UMX_LSTM8_PAIRED", paired), ("UMX_LSTM8_MIN_LANES", min_lanes)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _nact(flags):
    return 4 - bin((flags >> 8) & 0xF).count("1")


def run_schedule(pkg, lab, n_cus, hidden, frames, B, calls, kernel, *, flags=0, tapped=None, on_tapped=None):
    """The calls of one schedule on the context of (hidden, frames, B) with assertions (a), (b), (c) after every call, the recurrence's
    name, and the plane GEMM every stage launched last against gemm_kind for the call's last run of lanes.  tapped: the call taken with
    FLAG_DEBUG_TAPS; on_tapped(eng, active, waves, stems, state_before) runs right after it (the taps are that call's)."""
    N = frames * 1024
    sched = lm.Schedule(calls)
    eng = lab.engine(hidden, N, B)
    stepwise = bool(flags & pkg.FLAG_LSTM_STEPWISE)
    ref_flags = flags & ~pkg.FLAG_LSTM_STEPWISE  # the per-step driver is held to the persistent reference's bits
    Tp = max(eng.T, 256)
    assert eng.T == frames + 1
    before = [eng.track_stream_get(b) for b in range(B)]
    assert all(not s.any() for s in before)
    for i, act in enumerate(sched.calls):
        assert max(act) < B
        waves = [lab.audio(N, b, sched.segment(i, b)) if b in act else None for b in range(B)]
        got = eng.infer_batch(waves, flags | (pkg.FLAG_DEBUG_TAPS if i == tapped else 0))
        assert eng.lstm_kernel_name() == kernel, (i, eng.lstm_kernel_name())
        assert eng.lstm_was_persistent() == (not stepwise), i  # (c)
        l0, nl = lm.gemm_runs(act)[-1]
        for mode in range(4):
            assert eng.gemm_kernel_name(mode) == lm.gemm_kind(mode, hidden, nl, Tp, _nact(flags), n_cus), (i, mode, l0, nl)
        after = [eng.track_stream_get(b) for b in range(B)]
        for b in range(B):
            if b not in act:  # (b)
                assert got[b] is None, (i, b)
                assert _same(after[b], before[b]), ("idle lane's state", i, b)
                continue
            k = sched.segment(i, b)
            assert k == sched.consumed_before(i, b)
            stems, state = lab.reference(hidden, N, ref_flags, b, sched.counts[b], kernel)[k]
            for t in range(4):  # (a)
                assert _same(got[b][t], stems[t]), ("stems", i, sorted(act) if len(act) < B else "dense", b, t,
                                                    float(np.abs(got[b][t] - stems[t]).max()))
            assert _same(after[b], state), ("state", i, sorted(act) if len(act) < B else "dense", b)
            assert np.abs(after[b]).max() > 0 and all(np.abs(s).max() > 0 for s in stems[3:])
        if i == tapped and on_tapped is not None:
            on_tapped(eng, act, waves, got, before)
        before = after
    return sched


def _f64_hook(lab, n_cus, hidden, rep, lanes, fb_lane, where):
    """check_network on `lanes` (targets 0 and 3) and check_front_back on fb_lane, from the taps of the pattern call."""
    targets = lab.model(hidden)[1]

    def hook(eng, act, waves, stems, state_before):
        for b in lanes:
            assert b in act
            check_network(rep, eng, b, targets, state_before[b], where, which=(0, 3))
        run_len = sf.fused_run_split(eng.T, len(act), n_cus)[0]
        check_front_back(rep, eng, fb_lane, waves[fb_lane], stems[fb_lane], False, where, run_len)
    return hook


# ---------------------------------------------------------------- hidden 1024, 64 lanes: two octets per workgroup in turn
def _pairs(hidden, act, **kw):
    return lm.workgroup_pairs(lm.lstm_launch_plan(hidden, act, **kw))


@pytest.mark.parametrize("stepwise", [True, False], ids=["stepwise", "persistent"])  # (the per-step driver first: it cannot spin)
def test_only_the_second_octet_of_a_pair(pkg, lab, n_cus, monkeypatch, frames, stepwise):
    """{32..39}: workgroup-octet 0 serves an absent first octet and a present second one; the other three return after the census.
    The persistent pattern call also against float64 (lanes 32 and 39)."""
    _env(monkeypatch)
    pat = R(32, 39)
    plan = lm.lstm_launch_plan(1024, pat)
    assert plan.octs == 2 and plan.launches[0][2][0] == (False, True) and sum(map(lm.returns_early, plan.launches[0][2])) == 3
    rep = sf.Report()
    hook = None if stepwise else _f64_hook(lab, n_cus, 1024, rep, (32, 39), 39, "second octet only {32..39}")
    run_schedule(pkg, lab, n_cus, 1024, frames, 64, [range(64), pat, range(64)], "lstm_batch8_kernel",
                 flags=pkg.FLAG_LSTM_STEPWISE if stepwise else 0, tapped=None if stepwise else 1, on_tapped=hook)
    if not stepwise:
        assert len(rep.rows) > 20
        _finish(rep, f"sparse_1024_second_octet_T{frames + 1}")


@pytest.mark.parametrize("stepwise", [True, False], ids=["stepwise", "persistent"])
def test_first_only_and_second_only_workgroups(pkg, lab, n_cus, monkeypatch, frames, stepwise):
    """{3, 63}: a workgroup with its first octet only, one with its second only, two that exit after the census.  The persistent pattern
    call also against float64 (lanes 3 and 63)."""
    _env(monkeypatch)
    pairs = _pairs(1024, {3, 63})
    assert pairs == [(True, False), (False, False), (False, False), (False, True)]
    rep = sf.Report()
    hook = None if stepwise else _f64_hook(lab, n_cus, 1024, rep, (3, 63), 63, "first-only and second-only {3, 63}")
    run_schedule(pkg, lab, n_cus, 1024, frames, 64, [range(64), {3, 63}, range(64)], "lstm_batch8_kernel",
                 flags=pkg.FLAG_LSTM_STEPWISE if stepwise else 0, tapped=None if stepwise else 1, on_tapped=hook)
    if not stepwise:
        assert len(rep.rows) > 20
        _finish(rep, f"sparse_1024_first_and_second_only_T{frames + 1}")


def test_one_lane_whose_first_octet_is_absent(pkg, lab, n_cus, monkeypatch, frames):
    _env(monkeypatch)
    pairs = _pairs(1024, {37})
    assert pairs[0] == (False, True) and all(lm.returns_early(x) for x in pairs[1:])
    run_schedule(pkg, lab, n_cus, 1024, frames, 64, [range(64), {37}, {3, 63}], "lstm_batch8_kernel")


def test_one_octet_per_workgroup_inside_a_64_lane_context(pkg, lab, n_cus, monkeypatch, frames):
    """{0..7} u {16..20}: top <= 32, the NO = 1 instantiation with an absent octet, between two dense calls (NO = 2)."""
    _env(monkeypatch)
    pat = R(0, 7) | R(16, 20)
    plan = lm.lstm_launch_plan(1024, pat)
    assert plan.octs == 1 and plan.top <= plan.per and lm.returns_early(plan.launches[0][2][1])
    assert lm.lstm_launch_plan(1024, range(64)).octs == 2
    run_schedule(pkg, lab, n_cus, 1024, frames, 64, [range(64), pat, range(64)], "lstm_batch8_kernel")


def test_mixed_lanes_and_mixed_gemm_kinds_in_one_call(pkg, lab, n_cus, monkeypatch, frames):
    """{5, 12, 40..47, 50}: one-lane runs and a long run of the plane GEMMs in ONE call -- for W_ih they must be different kernels (the
    run grows downwards until the model says so on this device) -- then the long run alone, whose kernel the engine then reports."""
    _env(monkeypatch)
    lo = 40
    kind = lambda nl: lm.gemm_kind(lm.G_IH, 1024, nl, 256, 4, n_cus)  # noqa: E731
    while kind(47 - lo + 1) == kind(1) and lo > 14:
        lo -= 1
    assert kind(47 - lo + 1) != kind(1) == "gemm_planes_kernel", (n_cus, lo)
    pat = {5, 12, 50} | R(lo, 47)
    assert lm.gemm_runs(pat) == [(5, 1), (12, 1), (lo, 48 - lo), (50, 1)]
    pairs = _pairs(1024, pat)
    assert (True, True) in pairs and (False, True) in pairs
    run_schedule(pkg, lab, n_cus, 1024, frames, 64, [range(64), pat, R(lo, 47)], "lstm_batch8_kernel")


def test_vocals_only_chain_exit_combines_with_the_mask_exit(pkg, lab, n_cus, monkeypatch, frames):
    """{3, 63} with every target but vocals skipped: nchains = 2, so workgroups leave for `chain >= nchains` as well as for their mask."""
    _env(monkeypatch)
    flags = pkg.FLAG_SKIP_TARGET(0) | pkg.FLAG_SKIP_TARGET(1) | pkg.FLAG_SKIP_TARGET(2)
    assert _nact(flags) == 1 and sum(map(lm.returns_early, _pairs(1024, {3, 63}))) == 2
    run_schedule(pkg, lab, n_cus, 1024, frames, 64, [range(64), {3, 63}, range(64)], "lstm_batch8_kernel", flags=flags)


def test_unpaired_context_skips_a_part(pkg, lab, n_cus, monkeypatch, frames):
    """UMX_LSTM8_PAIRED=0: two launches of 32 lanes; {40..47} launches only the second (lane_base 32), {3, 63} both."""
    _env(monkeypatch, paired=0)
    plan = lm.lstm_launch_plan(1024, R(40, 47), paired=False)
    assert plan.parts == 2 and [b for b, _, _ in plan.launches] == [32]
    assert [b for b, _, _ in lm.lstm_launch_plan(1024, {3, 63}, paired=False).launches] == [0, 32]
    run_schedule(pkg, lab, n_cus, 1024, frames, 64, [range(64), R(40, 47), {3, 63}], "lstm_batch8_kernel")


def test_group_kernel_at_hidden_1024_skips_groups(pkg, lab, n_cus, monkeypatch, frames):
    """UMX_LSTM8_MIN_LANES=99, 40 lanes: lstm_batch_kernel on the u8-resident W_hh at K = 512; {35} launches group 2 only, {1, 39}
    groups 0 and 2."""
    _env(monkeypatch, min_lanes=99)
    assert lm.lstm_launch_plan(1024, {35}, lstm8=False).groups == [2]
    assert lm.lstm_launch_plan(1024, {1, 39}, lstm8=False).groups == [0, 2]
    run_schedule(pkg, lab, n_cus, 1024, frames, 40, [range(40), {35}, {1, 39}], "lstm_batch_kernel")


# ---------------------------------------------------------------- hidden 512: eight octets side by side
def test_hidden_512_absent_octets_side_by_side(pkg, lab, n_cus, monkeypatch, frames):
    """{9, 63}, {56..63}, {0..7} u {24}: one octet per workgroup whatever the mask; six, seven and six of the eight workgroup-octets
    return after the census.  The first pattern call also against float64 (lanes 9 and 63)."""
    _env(monkeypatch)
    pats = [{9, 63}, R(56, 63), R(0, 7) | {24}]
    for pat, on in zip(pats, ([1, 7], [7], [0, 3])):
        plan = lm.lstm_launch_plan(512, pat)
        assert plan.octs == 1 and len(plan.launches) == 1
        assert [i for i, x in enumerate(plan.launches[0][2]) if not lm.returns_early(x)] == on
    rep = sf.Report()
    run_schedule(pkg, lab, n_cus, 512, frames, 64, [range(64)] + pats, "lstm_batch8_kernel", tapped=1,
                 on_tapped=_f64_hook(lab, n_cus, 512, rep, (9, 63), 9, "hidden 512 {9, 63}"))
    assert len(rep.rows) > 20
    _finish(rep, f"sparse_512_T{frames + 1}")


# ---------------------------------------------------------------- hidden 256: lstm_batch_kernel, three groups of 16 lanes
def test_hidden_256_skipped_groups(pkg, lab, n_cus, monkeypatch, frames):
    _env(monkeypatch)
    pats = [{20}, {2, 47}, R(16, 31)]
    assert [lm.lstm_launch_plan(256, p).groups for p in pats] == [[1], [0, 2], [1]]
    assert lm.lstm_launch_plan(256, range(48)).groups == [0, 1, 2]
    run_schedule(pkg, lab, n_cus, 256, frames, 48, [range(48)] + pats, "lstm_batch_kernel")


# ---------------------------------------------------------------- the queue on the octet kernel
def _queue_calls(pkg, lanes, counts):
    """The active lanes of every call of the queue's plan."""
    lane, first, calls = pkg.queue_plan(lanes, counts)
    return [sorted(lane[j] for j in range(len(counts)) if first[j] <= c < first[j] + counts[j]) for c in range(calls)]


def _queue(pkg, lab, hidden, B, njobs, flags):
    N = 16 * 1024
    eng = lab.engine(hidden, N, B)
    jobs = [pkg.ggml.synth_audio(LENGTHS[j % 7], 7000 + j) for j in range(njobs)]
    shifts = [SHIFTS[j % 7] for j in range(njobs)]
    counts = [len(pkg.segment_plan(_padded(x.shape[1], s), N)[0]) for x, s in zip(jobs, shifts)]
    alone = [eng.separate(x, flags=flags, shift_offset=s) for x, s in zip(jobs, shifts)]
    for run in range(2):  # the second run meets the state the first left
        got = eng.separate_queue(jobs, shift_offsets=shifts, flags=flags)
        assert eng.queue_calls() == pkg.queue_plan(B, counts)[2]
        for j in range(njobs):
            _bits_equal(got[j], alone[j], (hidden, hex(flags), run, j))
    assert all(np.abs(alone[1][t]).max() > 0 for t in range(4) if not flags & pkg.FLAG_SKIP_TARGET(t))
    return _queue_calls(pkg, B, counts)


@pytest.mark.parametrize("flagged", [False, True], ids=["plain", "vocals_residual_softmask_em2"])
def test_queue_on_the_octet_kernel(pkg, lab, n_cus, monkeypatch, flagged):
    """Hidden 1024, 40 lanes, 56 jobs: every job bit for bit Engine.separate of it alone (lane 0, top = 1: NO = 1 and 128-row tiles),
    while the queue's calls mix NO = 2, absent octets, NO = 1 and runs of several lanes."""
    _env(monkeypatch)
    flags = (pkg.flags_for_targets(["vocals"], residual=True, softmask=True) | pkg.FLAG_WIENER_ITERS(2)) if flagged else 0
    calls = _queue(pkg, lab, 1024, 40, 56, flags)
    plans = [lm.lstm_launch_plan(1024, c) for c in calls]
    assert any(p.octs == 2 and any(map(lm.returns_early, lm.workgroup_pairs(p))) for p in plans)  # two in turn, a workgroup without lanes
    assert any(p.octs == 1 and any(map(lm.returns_early, lm.workgroup_pairs(p))) for p in plans) and plans[0].octs == 2
    if not flagged:  # (one active target: every run of this plan takes the 128-row tiles)
        assert any(len({lm.gemm_kind(lm.G_IH, 1024, nl, 256, 4, n_cus) for _, nl in lm.gemm_runs(c)}) > 1 for c in calls)


def test_queue_on_the_group_kernel(pkg, lab, monkeypatch):
    """Hidden 256, 20 lanes, 30 jobs: lstm_batch_kernel; the tail of the run launches group 0 only, with a smaller layout."""
    _env(monkeypatch)
    calls = _queue(pkg, lab, 256, 20, 30, 0)
    plans = [lm.lstm_launch_plan(256, c) for c in calls]
    assert plans[0].groups == [0, 1] and plans[-1].groups == [0] and len({p.lanes_arg for p in plans}) > 1
