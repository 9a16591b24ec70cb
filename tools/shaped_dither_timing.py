"""Times of the noise-shaped 16-bit encode (UMX_DITHER_SHAPED; csrc/pcm16_shaped.h) beside the TPDF encode and fp32.

    python tools/shaped_dither_timing.py --kernel [--out FILE]   the shaped encode launch against the TPDF encode launch on a 600 s track
                                                 with four outputs, stream events in one process
    python tools/shaped_dither_timing.py [--reps 5] [--rounds 2] [--parent-root <built checkout of the parent commit>] [--out FILE]
        one 600 s track at shift offset 4033 on a one-lane context, host buffers in and out (umx_hip_separate_tracks_io): fp32, and
        UMX_SAMPLE_S16 out with dither 0, 1 and 2 (a tree without the mode -- the parent commit -- runs the first three: the rows this
        tree's fp32 and mode-1 rows are held against).  Every form: one warm-up run, then `reps` runs, the forms alternating; one fresh
        process per tree and round, the trees alternating (UMX_TIMING_ROOT tells a child which tree to load); a row is the median of a
        tree's rounds x reps runs with min .. max."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(os.environ.get("UMX_TIMING_ROOT") or Path(__file__).resolve().parent.parent).resolve()
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

SHIFT = 4033
FORMS = ("f32", "s16 dither 0", "s16 dither 1", "s16 dither 2")


def med(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"


def child_main(a):
    pkg = ge.load_package()
    forms = [f for f in FORMS if f != "s16 dither 2" or hasattr(pkg, "DITHER_SHAPED")]
    n = int(a.seconds * 44100)
    audio = np.clip(np.random.default_rng(5).standard_normal(2 * n) * 0.4, -1, 1).astype(np.float32)
    io = {f: pkg.SampleIO(pkg.SAMPLE_F32, pkg.SAMPLE_F32 if f == "f32" else pkg.SAMPLE_S16, 0 if f == "f32" else int(f[-1]), 7) for f in forms}
    outs = [np.zeros(8 * n, np.uint8) for _ in range(4)]
    res = {}
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(a.hidden, seed=7), a.hidden)
        e = pkg.Engine.from_file(path, segment_samples=pkg.SEGMENT_SAMPLES)

        def run(f):
            au, out = (C.c_void_p * 1)(audio.ctypes.data), (C.c_void_p * 4)(*[b.ctypes.data for b in outs])
            t0 = time.perf_counter()
            rc = e.lib.umx_hip_separate_tracks_io(e.h, 1, au, (C.c_int * 1)(n), None, (C.c_int * 1)(SHIFT), 4, None, out, 0, C.byref(io[f]), None, None)
            dt = time.perf_counter() - t0
            assert rc == 0, e.last_error()
            return dt * 1e3

        runs = {f: [] for f in forms}
        for f in forms:
            run(f)  # warm-up: buffers grow, pages are touched
        for _ in range(a.reps):  # the forms alternate, so that drift shows in all of them alike
            for f in forms:
                runs[f].append(run(f))
        res.update(runs)
        e.close()
    print(json.dumps(res))


def kernel_main(a):
    pkg = ge.load_package()
    import torch
    torch.zeros(1).cuda()
    n = int(a.seconds * 44100)
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(128, seed=7), 128)
        eng = pkg.Engine.from_file(path)
    src = [(torch.randn(2 * n, device="cuda") * 0.4) for _ in range(4)]
    dst = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4)]
    acc = torch.zeros(28, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    s, d, hs = [b.data_ptr() for b in src], [b.data_ptr() for b in dst], st.cuda_stream
    eng.levels_device(s, n, acc.data_ptr(), hip_stream=hs)  # the peaks the rescaled encodes form their divisor from
    cases = [("encode_kernel<SampleS16> x 4, TPDF", lambda: eng.pcm16_encode_device(s, n, d, 0, 7, hip_stream=hs)),
             ("pcm16_shaped_encode_kernel<false, Plain> x 4", lambda: eng.pcm16_encode_device(s, n, d, 0, 7, hip_stream=hs, shaped=True)),
             ("encode_rescaled_kernel<SampleS16> x 4, TPDF", lambda: eng.pcm16_encode_rescaled_device(s, n, d, acc.data_ptr(), 0, 7, hip_stream=hs)),
             ("pcm16_shaped_encode_kernel<true, Rescaled> x 4", lambda: eng.pcm16_encode_rescaled_device(s, n, d, acc.data_ptr(), 0, 7, hip_stream=hs, shaped=True))]
    blocks = -(-n // 4096)
    lines = [f"# {torch.cuda.get_device_name(0)}; {n} frames ({a.seconds:.0f} s), four buffers, stream events, 1 warm-up launch, median of {a.reps} (min .. max)",
             f"# the shaped launch: {blocks} blocks of 4096 frames a buffer, {-(-blocks // 32) * 4} workgroups of one wave"]
    for what, call in cases:
        ms = []
        for _ in range(a.reps + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            call()
            t1.record(st)
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        v = ms[1:]
        lines.append(f"{what:<50} {statistics.median(v) * 1e3:9.1f} us ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})")
    eng.close()
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="processes per tree, the trees alternating")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--child", action="store_true", help="(the fresh processes) run the forms of the tree UMX_TIMING_ROOT names, one JSON line")
    ap.add_argument("--out", default=None, help="also write the table here")
    a = ap.parse_args()
    if a.kernel:
        return kernel_main(a)
    if a.child:
        return child_main(a)

    def child(root):
        env = dict(os.environ)
        env.pop("UMX_HIP_LIB", None)
        env.pop("UMX_TIMING_ROOT", None)
        if root:
            env["UMX_TIMING_ROOT"] = str(Path(root).resolve())
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--hidden", str(a.hidden), "--seconds", str(a.seconds), "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    par, tree = {}, {}
    for _ in range(a.rounds):  # parent, tree, parent, tree, ...
        for into, root in ((par, a.parent_root), (tree, None)):
            if into is tree or root:
                for k, v in child(root).items():
                    into.setdefault(k, []).extend(v)
    import torch
    lines = [f"# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); torch {torch.__version__}, HIP {torch.version.hip}",
             f"# one {a.seconds:.0f} s track, one-lane context, hidden {a.hidden}, synthetic weights, shift offset {SHIFT}, fp32 in, pageable host buffers",
             f"# wall ms of the bare C call: per process 1 warm-up run and {a.reps} runs, the forms alternating; {a.rounds} fresh processes per tree, the "
             f"trees alternating; median of a tree's {a.rounds * a.reps} runs (min .. max)"]
    base = statistics.median(tree["f32"])
    for f in FORMS:
        if f in par:
            lines.append(f"{f:<14} parent commit  {med(par[f]):>26} ms")
        lines.append(f"{f:<14} this tree      {med(tree[f]):>26} ms   / fp32 of this tree = {statistics.median(tree[f]) / base:.3f}")
    for f in FORMS:
        if f in par:
            old, m = par[f], statistics.median(tree[f])
            verdict = "inside" if min(old) <= m <= max(old) else ("BELOW (faster than)" if m < min(old) else "ABOVE (SLOWER than)")
            lines.append(f"# {f}: this tree's median {m:.2f} ms is {verdict} the parent's min .. max {min(old):.2f} .. {max(old):.2f} ms")
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
