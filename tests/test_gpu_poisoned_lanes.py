"""Non-finite audio stays in its own lane, call and track, bit for bit (include/umx_hip.h "Non-finite input").  One context
carries up to 64 unrelated tracks through a call; with finite audio a value that crosses a lane boundary through a product with an
exact zero is invisible (0 * stale = 0, but 0 * NaN = NaN), so every schedule here poisons a lane -- a NaN sample, +-inf, a lane of NaN,
finite 3e38 samples that overflow inside the STFT, the last valid sample (tests/poison.py) -- and holds every OTHER lane to the bits
it has without the poison:
  containment  in the poisoned call every clean lane's stems and carried LSTM state are bitwise those of the lane's segment sequence
               ALONE on a one-lane context of the same model that has never seen a non-finite value; the call returns UMX_OK, ran
               the recurrence and the GEMMs the clean call before it on the same lanes ran, and no timeout recovery took place;
  recovery     behind track_stream_reset(lane) every lane, that one included, has the bits it would have had if the poisoned call
               had never run -- over pipeline_depth() + 1 clean calls (both slots revisited), at the smallest n (rows the poisoned
               call left in the lane's buffers), on sparse lane sets that leave the lane idle, under other target sets, under other
               Wiener EM iteration counts, and under UMX_WIENER=stats4;
  whole tracks a poisoned track changes no bit of another track's stems or measurement records in separate_many and separate_queue,
               nor of the job that takes its lane next, nor when it is the one resampled job of the run.
Nothing is asserted about the poisoned lane's own outputs and state (the clamps of the gate functions and the ReLUs may swallow a NaN),
except that its `nonfinite` counts are those of the outputs it returned.  Not vacuous: in the poisoned call of one schedule per
recurrence the poisoned lane's `spec` tap is non-finite in every bin of exactly the frames that read the poison, and every tap of
every clean lane is finite.  The first clean call behind the poison of one hidden-512 schedule is also held to float64 stage by stage
(tests/stage_f64.py, C_DEFAULT and FLOOR as everywhere).  Segments of 5 and 6 hops; the lane sets are the table of DESIGN 28.

One multi-lane context is alive at a time (the open fault in umx_hip_destroy); the one-lane reference contexts stay.

UMX_STAGE_F64_REPORT=<file>: append the float64 check's distances to that file (JSON lines)."""
import ctypes as C
import os

import numpy as np
import pytest

import lane_masks as lm
import poison as ps
import stage_f64 as sf
from test_gpu_geometry_f64 import _finish, check_front_back, check_network
from test_gpu_queue import _bits_equal
from test_gpu_sparse_lanes import FRAMES, Lab, _nact, _same

pytestmark = pytest.mark.gpu

CAT = ps.catalogue()
TAPS = ("spec", "mix_mag", "x")
TARGET_TAPS = ("fc1", "lstm", "fc2", "mask", "target_mag", "y")
NOT_VACUOUS, AGAINST_F64 = ps.NOT_VACUOUS, ps.AGAINST_F64


class PoisonLab(Lab):
    """Lab with UMX_WIENER in the key of a context, the one-track context (tracks = 1: gemm_bf16x3_kernel, lstm_persistent_kernel) beside
    the lane contexts, and references of sequences with epochs, flags and lengths per call."""

    @staticmethod
    def env_key():
        return Lab.env_key() + (os.environ.get("UMX_WIENER"),)

    def engine(self, hidden, N, B):
        if B > 1:
            return super().engine(hidden, N, B)
        key = (hidden, N, 1) + self.env_key()
        if key != self.key:
            if self.eng is not None:
                self.eng.close()
            self.key, self.eng = None, None
            self.eng = self.pkg.Engine(self.model(hidden)[1], hidden, N)
            self.key = key
        self.eng.stream_reset()
        return self.eng

    def reference(self, entry, N, lane, sequence):
        """[[(stems, state after, kernel names)] per epoch] of the lane's clean calls alone: a one-lane context with the batched
        recurrence and the plane GEMMs for a lane context, a second one-track context for the one-track context."""
        one_track = entry.tracks == 1
        ek = (entry.hidden, N, one_track) + self.env_key()
        key = ek + (lane, sequence)
        if key not in self.refs:
            if ek not in self.ref_engines:
                kw = {} if one_track else {"tracks": 1, "lstm_batched": True, "gemm": "planes"}
                self.ref_engines[ek] = self.pkg.Engine(self.model(entry.hidden)[1], entry.hidden, N, **kw)
            one = self.ref_engines[ek]
            out = []
            for epoch in sequence:
                one.stream_reset() if one_track else one.track_stream_reset(-1)
                rows = []
                for seg, flags, short in epoch:
                    w = self.audio(N, lane, seg)
                    w = w[:, :1] if short else w
                    stems = one.infer_segment(w, flags) if one_track else one.infer_batch([w], flags)[0]
                    assert all(np.isfinite(s).all() for s in stems)
                    rows.append((stems, one.stream_get() if one_track else one.track_stream_get(0), _names(one)))
                out.append(rows)
            self.refs[key] = out
        return self.refs[key]


def _names(eng):
    return (eng.lstm_kernel_name(), eng.lstm_was_persistent(), eng.lstm_mode()) + tuple(eng.gemm_kernel_name(m) for m in range(4))


@pytest.fixture(scope="module")
def lab(pkg, tmp_path_factory):
    lb = PoisonLab(pkg, tmp_path_factory.mktemp("poisoned_lanes"))
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


def _by_context(names):
    return sorted(names, key=lambda nm: (CAT[nm].tracks == 1, CAT[nm].hidden, CAT[nm].tracks, sorted(CAT[nm].env.items())))


def run_poison_schedule(pkg, lab, n_cus, monkeypatch, name, frames, tapped=None):
    """The steps of CAT[name] on its context, with the assertions of the module's docstring after every call.  tapped: {step: hook}, the
    calls taken with FLAG_DEBUG_TAPS; hook(eng, call, waves, stems, state_before) runs right behind its call."""
    e, tapped = CAT[name], tapped or {}
    s, N, B = e.schedule, frames * 1024, e.tracks
    for var in ("UMX_LSTM8_PAIRED", "UMX_LSTM8_MIN_LANES", "UMX_WIENER"):
        monkeypatch.delenv(var, raising=False)
    for var, v in e.env.items():
        monkeypatch.setenv(var, v)
    eng = lab.engine(e.hidden, N, B)
    assert eng.T == frames + 1 and eng.pipeline_depth() == ps.PIPELINE_DEPTH == s.depth
    Tp = max(eng.T, 256)
    refs = {ln: lab.reference(e, N, ln, s.clean_sequence(ln)) for ln in s.lanes()}
    state_of = (lambda b: eng.stream_get()) if B == 1 else eng.track_stream_get
    before = [state_of(b) for b in range(B)]
    assert all(not st.any() for st in before)
    names_of = {}  # (lanes, active targets, per-step driver) -> what the first call of that kind ran
    for i, st in enumerate(s.steps):
        if isinstance(st, ps.Reset):
            eng.stream_reset() if B == 1 else eng.track_stream_reset(st.lane)
            before = [state_of(b) for b in range(B)]
            assert not before[st.lane].any(), ("the reset lane's state", i)
            continue
        waves = [None] * B
        for ln in st.active:
            w = lab.audio(N, ln, s.segment[i][ln])
            w = w[:, :1] if st.short else w
            waves[ln] = ps.apply(st.poison[ln], w, seed=ln) if ln in st.poison else w
        flags = st.flags | (pkg.FLAG_DEBUG_TAPS if i in tapped else 0)
        got = [eng.infer_segment(waves[0], flags)] if B == 1 else eng.infer_batch(waves, flags)  # (anything but UMX_OK raises)
        assert "recovered" not in eng.last_error() and "timed out" not in eng.last_error(), (i, eng.last_error())
        stepwise = bool(st.flags & pkg.FLAG_LSTM_STEPWISE)
        names = _names(eng)
        assert names[1] == (not stepwise) and (stepwise or names[0] == e.kernel), (i, names)
        kind = (st.active, _nact(st.flags), stepwise)
        assert names_of.setdefault(kind, names) == names, ("another kernel than the clean call of these lanes ran", i, names_of[kind], names)
        if st.poison:
            assert kind in names_of and i > 0 and not s.steps[i - 1].poison and s.steps[i - 1].active == st.active  # (a clean call came first)
        if B > 1:
            l0, nl = lm.gemm_runs(st.active)[-1]
            for mode in range(4):
                assert names[3 + mode] == lm.gemm_kind(mode, e.hidden, nl, Tp, _nact(st.flags), n_cus), (i, mode, l0, nl)
        else:
            assert set(names[3:]) == {"gemm_bf16x3_kernel"}, names
        after = [state_of(b) for b in range(B)]
        for b in range(B):
            if b not in st.active:
                assert got[b] is None, (i, b)
                assert _same(after[b], before[b]), ("idle lane's state", name, i, b)
                continue
            if b in st.poison:  # unspecified: only that the call handed the lane's buffers back
                assert all(got[b][t].shape == waves[b].shape for t in range(4))
                continue
            ep, k = s.reference_index(i, b)
            stems, state, ref_names = refs[b][ep][k]
            assert ref_names[:2] == names[:2] or B == 1, (i, b, ref_names, names)  # the same form of the recurrence as the reference
            what = (name, f"step {i}", "poisoned call" if st.poison else "clean call", f"lane {b}", sorted(st.poison.items()))
            for t in range(4):
                bad = int(np.count_nonzero(~np.isfinite(got[b][t])))
                assert _same(got[b][t], stems[t]), ("stems",) + what + (t, f"{bad} non-finite samples" if bad else float(np.abs(got[b][t] - stems[t]).max()))
            assert _same(after[b], state), ("state",) + what
            if not st.short:
                assert np.abs(after[b]).max() > 0 and all(np.abs(x).max() > 0 for x in stems[3:])
        if i in tapped and tapped[i] is not None:
            tapped[i](eng, st, waves, got, before)
        before = after
    return s


def _plain(names):
    special = set(NOT_VACUOUS) | {AGAINST_F64}
    return _by_context([nm for nm in names if nm not in special])


@pytest.mark.parametrize("name", _plain(nm for nm in CAT if not nm.startswith(("short_", "sparse_", "skip_", "em_"))))
def test_containment_and_recovery_on_the_same_geometry(pkg, lab, n_cus, monkeypatch, frames, name):
    """A clean call, the poisoned call, the reset of the poisoned lanes, pipeline_depth() + 1 clean calls."""
    run_poison_schedule(pkg, lab, n_cus, monkeypatch, name, frames)


@pytest.mark.parametrize("name", _plain(nm for nm in CAT if nm.startswith(("short_", "sparse_", "skip_", "em_"))))
def test_recovery_after_a_change_of_shape(pkg, lab, n_cus, monkeypatch, frames, name):
    """short_: clean calls of one sample behind the poisoned call at full n (the unfused filter under UMX_WIENER=stats4 as well);
    sparse_: a lane set that leaves the poisoned lane idle, then all lanes; skip_: four targets poisoned, then vocals only, vocals with
    residual and soft mask, three targets with a residual, all four; em_: three Wiener EM iterations poisoned, then one, then three."""
    s = run_poison_schedule(pkg, lab, n_cus, monkeypatch, name, frames)
    calls = [st for st in s.steps if isinstance(st, ps.Call)]
    (p,) = [k for k, st in enumerate(calls) if st.poison]
    if name.startswith("short_"):
        assert not calls[p].short and all(st.short for st in calls[p + 1:])
    if name.startswith("sparse_"):
        assert not set(calls[p].poison) & calls[p + 1].active and calls[p + 2].active == calls[p].active
    if name.startswith("skip_"):
        assert [_nact(st.flags) for st in calls[p:]] == [4, 1, 1, 3, 4]
    if name.startswith("em_"):
        assert [st.flags >> 16 for st in calls[p:]] == [3, 1, 3, 3]


def _sfx(B, lane):
    return "" if B == 1 else f"#{lane}"


@pytest.mark.parametrize("name", _by_context(NOT_VACUOUS))
def test_the_poison_reaches_the_spectrum_and_no_clean_tap(pkg, lab, n_cus, monkeypatch, frames, name):
    """The schedule as above, its poisoned call with FLAG_DEBUG_TAPS: the poisoned lanes' spec is non-finite in every bin of exactly the
    frames that read a poisoned sample, every tap of every clean lane is finite."""
    e = CAT[name]
    N, B = frames * 1024, e.tracks
    seen = []

    def hook(eng, call, waves, stems, state_before):
        for ln, pattern in sorted(call.poison.items()):
            any_bad, all_bad = ps.nonfinite_frames(eng.tap("spec" + _sfx(B, ln)))
            want = set(ps.poisoned_frames(pattern, waves[ln].shape[1], N))
            assert want and any_bad == want and all_bad == want, (name, ln, pattern, sorted(any_bad), sorted(all_bad), sorted(want))
            seen.append(pattern)
        for ln in sorted(call.active - set(call.poison)):
            for tap in TAPS:
                assert np.isfinite(eng.tap(tap + _sfx(B, ln)).view(np.float32)).all(), (name, ln, tap)
            for tap in TARGET_TAPS:
                for t in range(4):
                    assert np.isfinite(eng.tap(tap + _sfx(B, ln), t).view(np.float32)).all(), (name, ln, tap, t)

    (i,) = e.schedule.poisoned_calls()
    run_poison_schedule(pkg, lab, n_cus, monkeypatch, name, frames, tapped={i: hook})
    assert sorted(seen) == sorted(e.schedule.steps[i].poison.values())


def test_first_clean_call_behind_the_poison_against_float64(pkg, lab, n_cus, monkeypatch, frames):
    """Hidden 512, nine lanes, lane 8 (the second octet's only lane) poisoned with 3e38 samples: the first clean call behind its reset,
    fc1 .. target_mag of lanes 8 and 0 and the front and back end of lane 8 against float64."""
    e = CAT[AGAINST_F64]
    (p,) = e.schedule.poisoned_calls()
    first_clean = next(i for i in range(p + 1, len(e.schedule.steps)) if isinstance(e.schedule.steps[i], ps.Call))
    targets = lab.model(e.hidden)[1]
    rep = sf.Report()

    def hook(eng, call, waves, stems, state_before):
        where = "first clean call behind a poisoned lane 8"
        assert not state_before[8].any() and state_before[0].any()
        for b in (8, 0):
            check_network(rep, eng, b, targets, state_before[b], where, which=(0, 3))
        check_front_back(rep, eng, 8, waves[8], stems[8], False, where, sf.fused_run_split(eng.T, len(call.active), n_cus)[0])

    run_poison_schedule(pkg, lab, n_cus, monkeypatch, AGAINST_F64, frames, tapped={first_clean: hook})
    assert len(rep.rows) > 30
    _finish(rep, f"poisoned_512_T{frames + 1}")


# ---------------------------------------------------------------- whole tracks: three lanes, hidden 128
NQ = 16 * 1024
JOB_LENGTHS = [55000, 20000, 40000, 24577, 9000, 30000]  # segments: 5, 2, 4, 3, 1, 3; job 1 is the poisoned one
POISONED_JOB, POISON_AT = 1, 18000  # in the job's second segment only: [12288, 20000) but not [0, 16384)


@pytest.fixture(scope="module")
def tracks(pkg, lab):
    """(clean jobs, the jobs with job 1 poisoned, every job alone with its records) -- the references computed on the three-lane
    context BEFORE it has seen a non-finite sample, once, never changed."""
    for var in ("UMX_LSTM8_PAIRED", "UMX_LSTM8_MIN_LANES", "UMX_WIENER"):
        assert var not in os.environ
    eng = lab.engine(128, NQ, 3)
    clean = [pkg.ggml.synth_audio(L, 640 + j) for j, L in enumerate(JOB_LENGTHS)]
    offs, lens = pkg.segment_plan(JOB_LENGTHS[POISONED_JOB], NQ)
    assert [o <= POISON_AT < o + n for o, n in zip(offs, lens)] == [False, True]
    jobs = list(clean)
    jobs[POISONED_JOB] = clean[POISONED_JOB].copy()
    jobs[POISONED_JOB][0, POISON_AT] = np.nan
    jobs[POISONED_JOB][1, POISON_AT + 3] = np.inf
    alone = [eng.separate_queue([x], levels=True, loudness=True, true_peak=pkg.TRUE_PEAK_MEASURE) for x in clean]
    for j, x in enumerate(clean):
        _bits_equal(alone[j][0][0], eng.separate(x), ("a queue of one job is separate()", j))
        assert all(np.isfinite(s).all() and np.abs(s).max() > 0 for s in alone[j][0][0])
    return clean, jobs, alone


def _engine3(lab, monkeypatch):
    for var in ("UMX_LSTM8_PAIRED", "UMX_LSTM8_MIN_LANES", "UMX_WIENER"):
        monkeypatch.delenv(var, raising=False)
    return lab.engine(128, NQ, 3)


def _record_bytes(rec):
    """Every field of a ctypes record as bytes (the padding between fields is not part of the record)."""
    out = []
    for field, _ in type(rec)._fields_:
        v = getattr(rec, field)
        out.append((field, bytes(v) if isinstance(v, C.Array) else repr(v).encode()))
    return out


def _poisoned_counts(pkg, stems, levels):
    """The poisoned job's own record: nothing but that its nonfinite counts are those of the outputs it returned."""
    for t in range(4):
        acc = pkg.levels_host(stems[t], buffer=t)
        assert int(levels.nonfinite[t]) == int(acc.nonfinite[t]), (t, int(levels.nonfinite[t]), int(acc.nonfinite[t]))


def test_separate_many_with_the_middle_track_poisoned(pkg, lab, monkeypatch, tracks):
    clean, jobs, alone = tracks
    eng = _engine3(lab, monkeypatch)
    for run in range(2):  # the second run meets what the poisoned track of the first left in lane 1
        got = eng.separate_many(jobs[:3])
        for j in (0, 2):
            _bits_equal(got[j], alone[j][0][0], ("separate_many", run, j))
    got = eng.separate_many([clean[3], clean[4], clean[5]])  # clean tracks in all three lanes behind it
    for lane, j in enumerate((3, 4, 5)):
        _bits_equal(got[lane], alone[j][0][0], ("separate_many behind the poisoned run", j))
    got, levels = eng.separate_many_levels(jobs[:3])
    for j in (0, 2):
        _bits_equal(got[j], alone[j][0][0], ("separate_many_levels", j))
        assert _record_bytes(levels[j]) == _record_bytes(alone[j][1][0]), j
    _poisoned_counts(pkg, got[1], levels[1])


def test_queue_refills_the_poisoned_lane_beside_two_running_tracks(pkg, lab, monkeypatch, tracks):
    clean, jobs, alone = tracks
    eng = _engine3(lab, monkeypatch)
    counts = [len(pkg.segment_plan(L, NQ)[0]) for L in JOB_LENGTHS]
    lane, first, calls = pkg.queue_plan(3, counts)
    assert lane[:4] == [0, 1, 2, 1] and first[3] == counts[1] == 2  # job 3 takes lane 1 ...
    assert first[3] + 1 < min(counts[0], counts[2])  # ... while jobs 0 and 2 are mid-track in lanes 0 and 2
    for run in range(2):
        got = eng.separate_queue(jobs)
        assert eng.queue_calls() == calls
        for j in range(len(jobs)):
            if j != POISONED_JOB:
                _bits_equal(got[j], alone[j][0][0], ("queue", run, j))
    got = eng.separate_queue(clean)  # and the clean job in the same place behind them
    for j in range(len(jobs)):
        _bits_equal(got[j], alone[j][0][0], ("clean queue behind the poisoned ones", j))


def test_queue_records_of_every_clean_job_are_those_of_the_job_alone(pkg, lab, monkeypatch, tracks):
    clean, jobs, alone = tracks
    eng = _engine3(lab, monkeypatch)
    got, levels, loud, env, tps = eng.separate_queue(jobs, levels=True, loudness=True, true_peak=pkg.TRUE_PEAK_MEASURE)
    for j in range(len(jobs)):
        if j == POISONED_JOB:
            continue
        a_out, a_levels, a_loud, a_env, a_tps = alone[j]
        _bits_equal(got[j], a_out[0], ("queue with records", j))
        assert _record_bytes(levels[j]) == _record_bytes(a_levels[0]), ("levels", j)
        assert _record_bytes(loud[j]) == _record_bytes(a_loud[0]), ("loudness", j)
        assert _record_bytes(tps[j]) == _record_bytes(a_tps[0]), ("true peak", j)
        assert env[j].shape == a_env[0].shape and env[j].tobytes() == a_env[0].tobytes(), ("hop energies", j)
        assert list(levels[j].nonfinite) == [0, 0, 0, 0]
    _poisoned_counts(pkg, got[POISONED_JOB], levels[POISONED_JOB])


def test_queue_with_the_poisoned_job_at_48_khz(pkg, lab, monkeypatch, tracks):
    clean, jobs, alone = tracks
    eng = _engine3(lab, monkeypatch)
    rates = [pkg.MODEL_RATE] * len(jobs)
    rates[POISONED_JOB] = 48000  # (the same samples read at 48 kHz: the resampler spreads the two poisoned samples over its taps)
    got, levels = eng.separate_queue(jobs, rates=rates, levels=True)
    fwd, back = eng.resample_launches()
    assert fwd >= 1 and back >= 1
    for j in range(len(jobs)):
        if j != POISONED_JOB:
            _bits_equal(got[j], alone[j][0][0], ("queue with a 48 kHz job", j))
            assert _record_bytes(levels[j]) == _record_bytes(alone[j][1][0]), j
    _poisoned_counts(pkg, got[POISONED_JOB], levels[POISONED_JOB])
    got = eng.separate_queue(clean, rates=rates)  # the resampled lane behind it: the clean job at 48 kHz is what it is alone
    _bits_equal(got[POISONED_JOB], eng.separate_queue([clean[POISONED_JOB]], rates=[48000])[0], "the 48 kHz job, clean")
    for j in range(len(jobs)):
        if j != POISONED_JOB:
            _bits_equal(got[j], alone[j][0][0], ("clean queue with a 48 kHz job", j))
