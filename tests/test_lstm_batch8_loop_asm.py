"""The instruction stream of lstm_batch8_kernel's step loop ("the loop's instruction stream").

The source describes a turn as: polls' check, the previous row's stores and the next row's request, an LDS barrier, a matrix phase that
is ONE basic block, an LDS barrier, the gate phase.  What the compiler made of it was far from that: scalar-register spills restored
with v_readlane_b32 all over the loop (21 of them between the two barriers), kernel arguments reloaded every step, 64-bit vector
address arithmetic and multiplications per turn.  These tests read the gfx950 assembly (cross-compiled with the Makefile's flags, no
GPU needed) and hold the loop to what the source says.
"""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
# the four 512-unit instantiations (UMX-L's width): <512, PRECISE, NO>, the bench's is <512, false, 2>
CASES = [(0, 1), (0, 2), (1, 1), (1, 2)]
KERNELS = {(pr, no): f"_ZN3umx18lstm_batch8_kernelILi512ELb{pr}ELi{no}EEEvNS_9LstmBArgsE" for pr, no in CASES}
# scalar-register spills of the PROLOGUE (kernel arguments the epilogue needs again, pieces of the address arithmetic in front of the
# loop): written and restored outside the step loops, which test_step_loops_reload_and_multiply_nothing holds to zero restores.
# DESIGN 4.6 documents the figures; before the loop diet <512, false, 2> had 125, restored all over the loops.
PROLOGUE_SGPR_SPILLS = {(0, 1): 0, (0, 2): 26, (1, 1): 0, (1, 2): 34}


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    """The gfx950 assembly of the engine, compiled once with the Makefile's flags (hipcc cross-compiles without a GPU)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    mk = (ROOT / "umx.cpp_amd" / "Makefile").read_text()
    assert "-fno-slp-vectorize" in mk
    out = tmp_path_factory.mktemp("asm") / "engine.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           f"-I{ROOT / 'include'}", "-S", "--cuda-device-only", "-o", str(out), str(ROOT / "umx.cpp_amd" / "csrc" / "engine.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def function_lines(asm, name):
    """[(mnemonic, whole line, loop)] of one function's instructions in layout order; loop = the label of the OUTERMOST loop header
    the instruction's block belongs to (None outside loops), from the compiler's block comments."""
    body = asm[asm.index(name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    out, parent, cur = [], {}, None

    def outermost(label):
        while label in parent:
            label = parent[label]
        return label

    for raw in body.splitlines()[1:]:
        line = raw.split(";")[0].strip()
        block = re.match(r"\.L(BB\w+):", line) or re.match(r"\s*; %bb\.\d+:", raw)
        if block:
            own = block.group(1) if block.re.groups else None
            m = re.search(r"Parent Loop (BB\w+) Depth=1\b", raw)
            if m and own:  # the header of an inner loop
                parent[own] = m.group(1)
                cur = m.group(1)
            elif re.search(r"=>This (Inner )?Loop Header: Depth=1\b", raw):
                cur = own
            else:
                m = re.search(r"in Loop: Header=(BB\w+) Depth=", raw)
                cur = outermost(m.group(1)) if m else None
        elif line and not line.startswith("."):
            out.append((line.split()[0], line, cur))
    return out


def is_branch(op):
    return op.startswith("s_cbranch") or op in ("s_branch", "s_setpc_b64", "s_endpgm")


def matrix_phases(lines):
    """(first, last) indices of every run of v_mfma with no s_barrier between them."""
    phases, first, last = [], None, None
    for i, (op, _, _) in enumerate(lines):
        if op.startswith("v_mfma"):
            if first is None:
                first = i
            last = i
        elif op == "s_barrier" and first is not None:
            phases.append((first, last))
            first = None
    if first is not None:
        phases.append((first, last))
    return phases


def step_loops(lines):
    """Per outermost loop that holds matrix instructions: its instructions from the first v_mfma on, in layout order -- through the
    loop's backward branch and whatever blocks of the loop the compiler laid out behind it."""
    loops = {}
    for op, text, loop in lines:
        if loop is None:
            continue
        if op.startswith("v_mfma"):
            loops.setdefault(loop, [])
        if loop in loops:
            loops[loop].append((op, text))
    return list(loops.values())


def count(lines, pred):
    return [line[1] for line in lines if pred(line[0])]


@pytest.mark.parametrize("pr,no", CASES)
def test_matrix_phases_are_one_basic_block(device_asm, pr, no):
    """From the first to the last matrix instruction of a phase: no spill restore, no scalar load, no scratch access, no branch."""
    lines = function_lines(device_asm, KERNELS[pr, no])
    phases = matrix_phases(lines)
    # two bodies (intra-XCD and sc1 protocol) x NO turns, 2 + 2 x 16 matrix instructions each
    assert len(phases) == 2 * no, (pr, no, len(phases))
    for lo, hi in phases:
        n_mfma = len(count(lines[lo:hi + 1], lambda op: op.startswith("v_mfma")))
        assert n_mfma == 34, (pr, no, n_mfma)
        for what, pred in (("v_readlane / v_writelane", lambda op: op in ("v_readlane_b32", "v_writelane_b32")),
                           ("scalar loads", lambda op: op.startswith("s_load_")),
                           ("scratch accesses", lambda op: op.startswith("scratch_")),
                           ("branches", is_branch)):
            hits = count(lines[lo:hi + 1], pred)
            assert not hits, f"lstm_batch8_kernel<512, {pr}, {no}>: {what} inside a matrix phase: {hits[:4]}"


@pytest.mark.parametrize("pr,no", CASES)
def test_step_loops_reload_and_multiply_nothing(device_asm, pr, no):
    """From the first matrix instruction of a body's step loop to the loop's backward branch: no kernel-argument load, no
    multiplication for an address, no scalar-spill restore.  Spill traffic: nowhere in the loop, the polls' check included."""
    lines = function_lines(device_asm, KERNELS[pr, no])
    headers = {loop for op, _, loop in lines if loop and op.startswith("v_mfma")}
    spills = [text for op, text, loop in lines if loop in headers and op in ("v_readlane_b32", "v_writelane_b32")]
    assert not spills, f"lstm_batch8_kernel<512, {pr}, {no}>: {len(spills)} spill moves in the step loops: {spills[:4]}"
    loops = step_loops(lines)
    assert len(loops) == 2, (pr, no, len(loops))
    for loop in loops:
        assert any(is_branch(op) for op, _ in loop)
        for what, pred in (("scalar loads", lambda op: op.startswith("s_load_")),
                           ("multiplications", lambda op: op.split("_e")[0] in ("v_mad_u64_u32", "v_mul_lo_u32", "v_mul_hi_u32")),
                           ("v_readlane_b32", lambda op: op == "v_readlane_b32")):
            hits = count(loop, pred)
            assert not hits, f"lstm_batch8_kernel<512, {pr}, {no}>: {len(hits)} {what} in the step loop: {hits[:4]}"


@pytest.mark.parametrize("pr,no", CASES)
def test_no_scalar_register_spills(device_asm, pr, no):
    m = re.search(r"\.name:\s+" + KERNELS[pr, no] + r"\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)", device_asm)
    assert m, KERNELS[pr, no]
    assert int(m.group(1)) <= PROLOGUE_SGPR_SPILLS[pr, no], (pr, no, int(m.group(1)))
