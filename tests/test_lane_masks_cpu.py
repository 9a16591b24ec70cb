"""tests/lane_masks.py on hand-worked cases: the launches of one LSTM layer for sparse sets of active lanes (csrc/engine_lstm.h,
csrc/lstm_batch8.h), the plane GEMMs' runs and tile kinds (csrc/engine_stages.h), and the segment bookkeeping of a schedule.  Each
expected value below was worked out from those files by hand, not taken from the model.  No GPU: the kernels themselves are held to
these launches in tests/test_gpu_sparse_lanes.py."""
import lane_masks as lm

R = lambda a, b: set(range(a, b + 1))  # noqa: E731  (lanes a .. b)


def test_second_octet_only_in_a_64_lane_context():
    # hidden 1024: Hl = 512, 8 column shards, 4 octets side by side, per = 32; top = 40 > 32: two octets per workgroup, span 64, one part
    p = lm.lstm_launch_plan(1024, R(32, 39))
    assert (p.kernel, p.top, p.per, p.octs, p.span, p.parts) == ("lstm_batch8_kernel", 40, 32, 2, 64, 1)
    assert len(p.launches) == 1
    base, octs, pairs = p.launches[0]
    assert (base, octs) == (0, 2)
    # lanes 32 .. 39 are octet 4 = the SECOND octet (o + 4) of workgroup-octet 0
    assert pairs == [(False, True), (False, False), (False, False), (False, False)]
    assert [lm.returns_early(x) for x in pairs] == [False, True, True, True]


def test_first_only_and_second_only_workgroups():
    p = lm.lstm_launch_plan(1024, {3, 63})
    assert (p.top, p.octs, p.parts) == (64, 2, 1) and len(p.launches) == 1
    pairs = p.launches[0][2]
    # lane 3: octet 0 (first of workgroup-octet 0); lane 63: octet 7 = second of workgroup-octet 3
    assert pairs == [(True, False), (False, False), (False, False), (False, True)]
    assert [lm.returns_early(x) for x in pairs] == [False, True, True, False]


def test_one_octet_per_workgroup_inside_a_64_lane_context():
    p = lm.lstm_launch_plan(1024, R(0, 7) | R(16, 20))
    assert (p.top, p.octs, p.span, p.parts) == (21, 1, 32, 1)  # top <= per: the NO = 1 instantiation
    assert p.launches == [(0, 1, [(True, False), (False, False), (True, False), (False, False)])]
    assert lm.returns_early(p.launches[0][2][1])
    # ... and the dense call beside it is NO = 2
    assert lm.lstm_launch_plan(1024, range(64)).octs == 2
    assert lm.lstm_launch_plan(1024, range(64)).launches == [(0, 2, [(True, True)] * 4)]


def test_unpaired_context_skips_a_part():
    p = lm.lstm_launch_plan(1024, R(40, 47), paired=False)
    assert (p.top, p.octs, p.span, p.parts) == (48, 1, 32, 2)
    assert p.launches == [(32, 1, [(False, False), (True, False), (False, False), (False, False)])]  # part 0 is not launched
    p = lm.lstm_launch_plan(1024, {3, 63}, paired=False)
    assert [(b, o) for b, o, _ in p.launches] == [(0, 1), (32, 1)]
    assert p.launches[0][2][0] == (True, False) and p.launches[1][2][3] == (True, False)


def test_hidden_512_has_its_eight_octets_side_by_side():
    p = lm.lstm_launch_plan(512, {9, 63})
    assert (p.kernel, p.per, p.top, p.octs, p.parts) == ("lstm_batch8_kernel", 64, 64, 1, 1)  # top is never above per
    assert len(p.launches) == 1 and p.launches[0][:2] == (0, 1)
    assert [i for i, x in enumerate(p.launches[0][2]) if x[0]] == [1, 7]
    assert all(not x[1] for x in p.launches[0][2])


def test_group_kernel_launches_only_the_groups_with_a_lane():
    p = lm.lstm_launch_plan(256, {20})  # hidden 256 has no octet kernel
    assert (p.kernel, p.top, p.per, p.parts, p.groups) == ("lstm_batch_kernel", 21, 16, 2, [1])
    assert (p.lanes_arg, p.nbp) == (16, 16)  # min(top, span): the launch of group 1 is sized for a full group
    p = lm.lstm_launch_plan(256, {2, 47})
    assert (p.parts, p.groups, p.nbp) == (3, [0, 2], 16)
    assert lm.lstm_launch_plan(256, {2}).nbp == 4 and lm.lstm_launch_plan(256, {0}).nbp == 1  # alone, the LDS layout shrinks
    # hidden 1024 kept off the octet kernel (UMX_LSTM8_MIN_LANES=99)
    p = lm.lstm_launch_plan(1024, {35}, lstm8=False)
    assert (p.kernel, p.groups) == ("lstm_batch_kernel", [2])
    assert lm.lstm_launch_plan(1024, {1, 39}, lstm8=False).groups == [0, 2]


def test_gemm_runs_and_kinds():
    assert lm.gemm_runs({5, 12} | R(40, 47) | {50}) == [(5, 1), (12, 1), (40, 8), (50, 1)]
    assert lm.gemm_runs(range(64)) == [(0, 64)]
    assert lm.gemm_runs({63, 3}) == [(3, 1), (63, 1)]
    # hidden 1024, W_ih (N = 4096, K = 1024), Tp = 256, four targets, 256 CUs: one lane = 16 x 1 x 4 = 64 big tiles < 224: 128 x 128
    assert lm.gemm_kind(lm.G_IH, 1024, 1, 256, 4, 256) == "gemm_planes_kernel"
    # four lanes: 256 tiles >= 224 but not more than the 256 persistent workgroups: ping-pong; eight lanes: 512: persistent
    assert lm.gemm_kind(lm.G_IH, 1024, 4, 256, 4, 256) == "gemm_planes_pp_kernel"
    assert lm.gemm_kind(lm.G_IH, 1024, 8, 256, 4, 256) == "gemm_planes_ps_kernel"
    # fc1 (N = 1024): 4 x 64 x 4 = 1024 tiles at 64 lanes; one target: 256, not above 256 workgroups
    assert lm.gemm_kind(lm.G_FC1, 1024, 64, 256, 4, 256) == "gemm_planes_ps_kernel"
    assert lm.gemm_kind(lm.G_FC1, 1024, 64, 256, 1, 256) == "gemm_planes_pp_kernel"
    # fc2 at hidden 128: N = 128 is no multiple of 256
    assert lm.gemm_kind(lm.G_FC2, 128, 64, 256, 4, 256) == "gemm_planes_kernel"
    # fc1 at hidden 256, K = 2976: 93 k-steps; fc3 at hidden 128: K / 32 = 4 < 6 never runs persistent
    assert lm.gemm_kind(lm.G_FC3, 128, 64, 256, 4, 256) == "gemm_planes_pp_kernel"


def test_schedule_gives_every_lane_its_own_segment_count():
    s = lm.Schedule([range(4), {1, 3}, {0, 3}])
    assert s.counts == {0: 2, 1: 2, 2: 1, 3: 3}
    assert [s.segment(1, ln) for ln in range(4)] == [None, 1, None, 1]
    assert [s.segment(2, ln) for ln in range(4)] == [1, None, None, 2]  # lane 0 sat call 1 out: its SECOND segment, not its third
    assert [s.consumed_before(2, ln) for ln in range(4)] == [1, 2, 1, 2]
    assert s.per_lane() == {0: [(0, 0), (2, 1)], 1: [(0, 0), (1, 1)], 2: [(0, 0)], 3: [(0, 0), (1, 1), (2, 2)]}
    assert s.lanes() == [0, 1, 2, 3]
