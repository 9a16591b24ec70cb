"""tests/lane_masks.py -- what a call's set of active track lanes decides on the host, restated in plain Python: the launches of one
LSTM layer (csrc/engine_lstm.h run_lstm_layer_batched: top, per, octs, span, parts, part_on; per workgroup of lstm_batch8_kernel the
octets it finds present, csrc/lstm_batch8.h lstm8_workgroup / lstm8_body `on[o]`), the runs of consecutive active lanes the plane GEMMs
are launched over (csrc/engine_stages.h launch_gemm_lanes) and the tile kind each run takes (launch_gemm_planes: big / pp / ps), and
the bookkeeping of a schedule of calls in which lanes leave and return.  Test infrastructure for tests/test_lane_masks_cpu.py (hand-worked
cases, no GPU) and tests/test_gpu_sparse_lanes.py, where every schedule asserts through this model that it contains the condition it is
named for.  Nothing here needs a GPU.
"""
from collections import namedtuple

MAX_TRACKS = 64         # lstm_batch.h LSTMB_MAX_TRACKS
GROUP_TRACKS = 16       # lstm_batch.h LSTMB_GROUP_TRACKS: lanes per launch of lstm_batch_kernel
LSTM8_TRACKS = 8        # lstm_batch8.h: lanes per octet
LSTM8_UNITS = 64        # lstm_batch8.h: hidden units per workgroup
LSTM8_HL = (256, 512)   # engine.hip kLstmKernels: the LSTM hidden sizes lstm_batch8_kernel is built for (model hidden 512 / 1024)
KX, NOUT_PAD, GP_BK = 2976, 4352, 32  # common.h, gemm_planes.h
G_FC1, G_IH, G_FC2, G_FC3 = range(4)  # GemmMode = the `mode` of Engine.gemm_kernel_name


def lstm8_octets(Hl):
    """lstm_batch8.h: octets side by side in one launch (hidden 1024: 4 = 32 lanes, hidden 512: 8 = 64 lanes)."""
    return 32 // (Hl // LSTM8_UNITS)


def lstmb_lanes(lanes):
    """lstm_batch.h lstmb_lanes: (nbp, bulk) of the LDS layout of lstm_batch_kernel for a launch of `lanes` lanes."""
    nbp = 16 if lanes > 8 else 8 if lanes > 4 else 4 if lanes > 2 else 2 if lanes > 1 else 1
    return nbp, 8 if nbp > 8 else 16


def mask_bits(lanes):
    m = 0
    for ln in lanes:
        assert 0 <= ln < MAX_TRACKS, ln
        m |= 1 << ln
    return m


LstmPlan = namedtuple("LstmPlan", "kernel top per octs span parts launches groups lanes_arg nbp")
LstmPlan.__doc__ = """One LSTM layer of a call.  kernel: "lstm_batch8_kernel" or "lstm_batch_kernel"; launches (lstm_batch8_kernel):
[(lane_base, octs, [(on0, on1) per workgroup-octet])] -- a workgroup-octet whose pair is (False, False) returns early, after the census;
groups (lstm_batch_kernel): the 16-lane groups launched, lanes_arg / nbp: the argument and the result of lstmb_lanes."""


def lstm_launch_plan(hidden, mask, paired=True, lstm8=True):
    """engine_lstm.h run_lstm_layer_batched for the active lanes `mask` (any iterable of lane numbers).  paired: UMX_LSTM8_PAIRED;
    lstm8: the context runs lstm_batch8_kernel where it exists for this width (False: UMX_LSTM8_MIN_LANES=99)."""
    lanes = sorted(set(mask))
    assert lanes, "a call without an active lane launches no layer"
    bits, Hl = mask_bits(lanes), hidden // 2
    top = lanes[-1] + 1
    octets = bool(lstm8) and Hl in LSTM8_HL
    per = LSTM8_TRACKS * lstm8_octets(Hl) if octets else GROUP_TRACKS
    octs = 2 if (octets and paired and top > per) else 1
    span = per * octs
    parts = (top + span - 1) // span

    def part_on(p):
        return (bits >> (span * p)) & ((1 << span) - 1) != 0

    if not octets:
        lanes_arg = min(top, span)
        return LstmPlan("lstm_batch_kernel", top, per, 1, span, parts, [], [p for p in range(parts) if part_on(p)], lanes_arg,
                        lstmb_lanes(lanes_arg)[0])
    OCT = lstm8_octets(Hl)

    def octet_on(base, o):
        return (bits >> (base + LSTM8_TRACKS * o)) & 0xff != 0

    launches = []
    for p in range(parts):
        if not part_on(p):
            continue
        base = span * p
        launches.append((base, octs, [(octet_on(base, o), octs == 2 and octet_on(base, o + OCT)) for o in range(OCT)]))
    return LstmPlan("lstm_batch8_kernel", top, per, octs, span, parts, launches, [], GROUP_TRACKS, lstmb_lanes(GROUP_TRACKS)[0])


def returns_early(pair):
    """lstm8_workgroup: a workgroup none of whose octets has an active lane returns, its census ticket already taken."""
    return not (pair[0] or pair[1])


def workgroup_pairs(plan):
    """Every (on0, on1) of every launch of a lstm_batch8_kernel plan."""
    return [pair for _, _, pairs in plan.launches for pair in pairs]


def gemm_runs(mask):
    """engine_stages.h launch_gemm_lanes: the runs (l0, nl) of consecutive active lanes, one plane-GEMM launch each."""
    runs = []
    for ln in sorted(set(mask)):
        if runs and runs[-1][0] + runs[-1][1] == ln:
            runs[-1][1] += 1
        else:
            runs.append([ln, 1])
    return [tuple(r) for r in runs]


def gemm_kind(mode, hidden, nl, Tp, nact, n_cus, nbp=2):
    """engine_stages.h launch_gemm_planes (UMX_GEMM_PP / UMX_GEMM_PS unset): the kernel a launch over `nl` lanes of Tp rows takes for
    stage `mode` with `nact` active targets on a device of n_cus CUs.  nbp: planes of B (1 or 2: the same selection, another
    instantiation)."""
    assert nbp in (1, 2) and (nbp == 2 or mode in (G_FC1, G_IH))
    H = hidden
    N, K = {G_FC1: (H, KX), G_IH: (4 * H, H), G_FC2: (H, 2 * H), G_FC3: (NOUT_PAD, H)}[mode]
    M = (nl * Tp + 255) // 256 * 256
    blocks_big = (N // 256) * (M // 256) * nact
    big = N % 256 == 0 and blocks_big >= 224
    pp = big
    ps_wgs = n_cus // 8 * 8
    ps = pp and K // GP_BK >= 6 and ps_wgs >= 8 and blocks_big > ps_wgs and Tp >= 256
    return "gemm_planes_ps_kernel" if ps else "gemm_planes_pp_kernel" if pp else "gemm_planes_kernel"


class Schedule:
    """A list of calls, each the set of lanes active in it.  A lane's k-th active call consumes that lane's k-th segment."""

    def __init__(self, calls):
        self.calls = [frozenset(c) for c in calls]
        assert all(self.calls), "every call has an active lane"
        self._seg = []
        seen = {}
        for c in self.calls:
            self._seg.append({ln: seen.get(ln, 0) for ln in c})
            for ln in c:
                seen[ln] = seen.get(ln, 0) + 1
        self.counts = seen  # lane -> segments it consumes in all

    def lanes(self):
        return sorted(self.counts)

    def segment(self, call, lane):
        """The segment lane `lane` consumes in call `call` (None: idle there)."""
        return self._seg[call].get(lane)

    def consumed_before(self, call, lane):
        """Segments the lane has consumed when call `call` begins = the index of the reference state it must then hold."""
        return sum(1 for c in self.calls[:call] if lane in c)

    def per_lane(self):
        """lane -> [(call, segment)] in call order."""
        return {ln: [(i, s[ln]) for i, s in enumerate(self._seg) if ln in s] for ln in self.lanes()}
