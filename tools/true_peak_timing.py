"""Times of the true peak in the whole-track drivers (umx_hip_separate_tracks_true_peak / umx_hip_separate_queue_true_peak;
csrc/true_peak.h), host buffers in and out, int16 both ways, hidden 1024, 60 s segments.

    python tools/true_peak_timing.py [--lanes 64] [--jobs 160] [--reps 5] [--procs 3] [--parent-root <built checkout of the parent commit>] [--out FILE]
    python tools/true_peak_timing.py --kernel    true_peak_kernel alone on a 600 s track's four outputs, timed with stream events, beside
                                                 stem_levels_kernel on the same buffers (the HBM rate the byte floor is taken from)

    one lane    one 600 s track at shift offset 4033 on a one-lane context
    reset       the same track in reset mode (UMX_FLAG_RESET_SEGMENTS) on a 14-lane context
    catalogue   the seeded catalogue of tools/levels_timing.py through the queue
Each in three forms: base = the _loudness call, clamp with levels and no loudness (the queue: the _loudness queue), which the parent
commit has too; off = the same request through the new rung with UMX_TRUE_PEAK_OFF and no record; on = UMX_TRUE_PEAK_MEASURE with the
record.  Every form: one warm-up run, then the median of `reps` with min .. max, the forms alternating; `procs` fresh processes per
tree, the trees alternating (UMX_TIMING_ROOT tells a child which tree to load)."""
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

FP = C.POINTER(C.c_float)
SHIFT = 4033
RESET_LANES = 14  # a 600 s track is 14 segments: one call in reset mode
FLAG_RESET = 0x4000
FORMS = ("base", "off", "on")
CASES = {"one": "one lane   one {single:.0f} s track, one-lane context", "reset": "reset      one {single:.0f} s track, reset mode, 14 lanes",
         "catalogue": "catalogue  the queue, {jobs} jobs on {lanes} lanes"}


def med(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"


def job_lengths(jobs, lo, hi, seed=18):
    rng = np.random.default_rng(seed)
    return [int(s * 44100) for s in rng.uniform(lo, hi, jobs)]


def child_main(a):
    pkg = ge.load_package()
    has_true_peak = hasattr(pkg, "TruePeak")
    N = pkg.SEGMENT_SAMPLES
    lens = job_lengths(a.jobs, a.min_seconds, a.max_seconds)
    single_len = int(a.single_seconds * 44100)
    longest = max(max(lens, default=0), single_len)
    track16 = np.clip(np.random.default_rng(5).standard_normal(2 * longest) * 0.4 * 32767, -32768, 32767).astype(np.int16)
    n_sets = a.lanes + 2
    pool = [[np.zeros(longest if k == 0 else max(lens, default=1), np.int32) for _ in range(4)] for k in range(n_sets)]  # int16 stereo frames
    io16 = pkg.sample_io(pkg.SAMPLE_S16, pkg.SAMPLE_S16)
    res = {"true_peak": has_true_peak, "lengths_s": [round(x / 44100, 1) for x in lens]}
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(a.hidden, seed=7), a.hidden)

        def tracks(e, length, form, flags):
            au = (C.c_void_p * 1)(track16.ctypes.data)
            out = (C.c_void_p * 4)(*[b.ctypes.data for b in pool[0]])
            ln, sh = (C.c_int * 1)(length), (C.c_int * 1)(SHIFT)
            lv = (pkg.Levels * 1)()
            t0 = time.perf_counter()
            if form == "base":
                rc = e.lib.umx_hip_separate_tracks_loudness(e.h, 1, au, ln, None, sh, 4, None, out, flags, C.byref(io16), pkg.CLIP_CLAMP, lv, None, None,
                                                            None, None)
            else:
                tp = (pkg.TruePeak * 1)() if form == "on" else None
                rc = e.lib.umx_hip_separate_tracks_true_peak(e.h, 1, au, ln, None, sh, 4, None, out, flags, C.byref(io16), pkg.CLIP_CLAMP, lv, None, None,
                                                             pkg.TRUE_PEAK_MEASURE if form == "on" else pkg.TRUE_PEAK_OFF, tp, None, None)
            dt = time.perf_counter() - t0
            assert rc == 0, e.last_error()
            return dt

        def queued(e, form):
            free_sets, it = list(range(n_sets)), iter(range(len(lens)))

            def nxt(_u, job):
                j = next(it, None)
                if j is None:
                    return 0
                k = free_sets.pop()
                job[0].audio, job[0].length, job[0].shift_offset, job[0].tag = C.cast(track16.ctypes.data, FP), lens[j], SHIFT, k + 1
                for t in range(4):
                    job[0].out[t] = C.cast(pool[k][t].ctypes.data, FP)
                return 1

            def done(_u, job, *_records):
                free_sets.append(int(job[0].tag) - 1)

            t0 = time.perf_counter()
            if form == "base":
                rc = e.lib.umx_hip_separate_queue_loudness(e.h, pkg.QUEUE_NEXT_FN(nxt), pkg.QUEUE_LOUDNESS_FN(done), None, 4, None, 0, C.byref(io16),
                                                           pkg.CLIP_CLAMP)
            else:
                rc = e.lib.umx_hip_separate_queue_true_peak(e.h, pkg.QUEUE_NEXT_FN(nxt), pkg.QUEUE_TRUE_PEAK_FN(done), None, 4, None, 0, C.byref(io16),
                                                            pkg.CLIP_CLAMP, pkg.TRUE_PEAK_MEASURE if form == "on" else pkg.TRUE_PEAK_OFF)
            dt = time.perf_counter() - t0
            assert rc == 0, e.last_error()
            return dt

        def timed(name, fn):
            runs = {f: [] for f in FORMS if f == "base" or has_true_peak}
            for f in runs:
                fn(f)  # warm-up: buffers grow, pages are touched
            for _ in range(a.reps):  # the forms alternate, so that drift shows in all of them alike
                for f in runs:
                    runs[f].append(fn(f) * 1e3)
            for f, v in runs.items():
                res[f"{name}_{f}"] = v
            print(f"({name} is done)", file=sys.stderr, flush=True)

        one = pkg.Engine.from_file(path, segment_samples=N)
        timed("one", lambda f: tracks(one, single_len, f, 0))
        one.close()
        rst = pkg.Engine.from_file(path, segment_samples=N, tracks=RESET_LANES)
        timed("reset", lambda f: tracks(rst, single_len, f, FLAG_RESET))
        rst.close()
        if a.jobs > 0:
            eng = pkg.Engine.from_file(path, segment_samples=N, tracks=a.lanes)
            timed("catalogue", lambda f: queued(eng, f))
            eng.close()
    print(json.dumps(res))


def kernel_main(a):
    pkg = ge.load_package()
    import torch
    torch.zeros(1).cuda()
    n = int(a.single_seconds * 44100)
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(128, seed=7), 128)
        eng = pkg.Engine.from_file(path)
    bufs = [(torch.randn(2 * n, device="cuda") * 0.4) for _ in range(4)]
    ptrs = [b.data_ptr() for b in bufs]
    bits = torch.zeros(4, dtype=torch.int32, device="cuda")
    acc = torch.zeros(C.sizeof(pkg.LevelsAcc) // 4, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    lines = []

    def timed(what, launch):
        ms = []
        for _ in range(a.reps + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            launch()
            t1.record(st)
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        v = [x * 1e3 for x in ms[1:]]
        lines.append(f"{what:<70} {statistics.median(v):9.1f} us ({min(v):.1f} .. {max(v):.1f}), stream events, {a.reps} launches")
        return statistics.median(v)

    nbytes = 8 * n * 4
    lev = timed(f"stem_levels_kernel    {n} frames x 4 outputs, one launch", lambda: eng.levels_device(ptrs, n, acc.data_ptr(), hip_stream=st.cuda_stream))
    lines.append(f"#   {nbytes / 1e6:.1f} MB read: {nbytes / lev / 1e6:.2f} TB/s -- the rate the byte floor of the next rows is taken from: {lev:.1f} us")
    for rate in (44100, 96000, 192000):
        t = timed(f"true_peak_kernel<{ref_factor(rate)}>   {n} frames x 4 outputs at {rate} Hz, one launch",
                  lambda: eng.true_peak_device(ptrs, n, rate, bits.data_ptr(), hip_stream=st.cuda_stream))
        lines.append(f"#   {t / lev:.2f} x the byte floor")
    region = 45 * 44100
    timed(f"true_peak_kernel<4>   {region} frames x 4 outputs (one 45 s region)", lambda: eng.true_peak_device(ptrs, n, 44100, bits.data_ptr(), region, region,
                                                                                                                hip_stream=st.cuda_stream))
    eng.close()
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


def ref_factor(rate):
    return 4 if rate < 96000 else 2 if rate < 192000 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--jobs", type=int, default=160, help="0: no catalogue")
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--single-seconds", type=float, default=600.0)
    ap.add_argument("--min-seconds", type=float, default=90.0 * 0.578, help="catalogue: the shortest job (profiles/pcm16_timing.txt ran 53 .. 277 s)")
    ap.add_argument("--max-seconds", type=float, default=480.0 * 0.578, help="catalogue: the longest job")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3, help="fresh processes per tree")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--child", action="store_true", help="(the fresh processes) run the cases of the tree UMX_TIMING_ROOT names, one JSON line")
    ap.add_argument("--out", default=None, help="also write the table here")
    a = ap.parse_args()
    if a.kernel:
        return kernel_main(a)
    if a.child:
        return child_main(a)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def child(root):
        env = dict(os.environ)
        env.pop("UMX_HIP_LIB", None)
        env.pop("UMX_TIMING_ROOT", None)
        if root:
            env["UMX_TIMING_ROOT"] = str(Path(root).resolve())
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--lanes", str(a.lanes), "--jobs", str(a.jobs), "--hidden", str(a.hidden),
               "--single-seconds", str(a.single_seconds), "--min-seconds", str(a.min_seconds), "--max-seconds", str(a.max_seconds), "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=1100)  # (its progress lines go to this process's stderr)
        assert r.returncode == 0, r.stdout[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    pars, trees = [], []
    for _ in range(a.procs):  # the trees alternate
        if a.parent_root:
            pars.append(child(a.parent_root))
        trees.append(child(None))
    import torch
    say(f"# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); torch {torch.__version__}, HIP {torch.version.hip}")
    say(f"# hidden {a.hidden}, segment_samples 2646000 (stride 1984500), synthetic weights, shift offset {SHIFT}, int16 both ways, pageable host buffers")
    say(f"# wall ms of the bare C calls: 1 warm-up run, median of {a.reps} (min .. max), the forms alternating; {a.procs} fresh processes per tree, "
        "the trees alternating: one column per process")
    L = trees[0]["lengths_s"]
    if a.jobs > 0:
        say(f"# catalogue: {a.jobs} jobs of {min(L):.0f} .. {max(L):.0f} s (seeded), {sum(L):.0f} s of audio")
    for name, label in CASES.items():
        if f"{name}_base" not in trees[0]:
            continue
        label = label.format(lanes=a.lanes, single=a.single_seconds, jobs=a.jobs)
        if pars:
            say(f"{label:<52} _loudness, parent commit  " + "   ".join(f"{med(p[f'{name}_base']):>26}" for p in pars) + " ms")
        for f, what in (("base", "_loudness, this tree"), ("off", "true peak off"), ("on", "true peak on")):
            say(f"{label:<52} {what:<25} " + "   ".join(f"{med(t[f'{name}_{f}']):>26}" for t in trees) + " ms")
        on = statistics.median([statistics.median(t[f"{name}_on"]) for t in trees])
        off = statistics.median([statistics.median(t[f"{name}_off"]) for t in trees])
        say(f"# {name}: true peak on costs {on - off:+.2f} ms, {on / off:.3f} x the off form (medians of the process medians)")
        if pars:
            lo, hi = min(min(p[f"{name}_base"]) for p in pars), max(max(p[f"{name}_base"]) for p in pars)
            ms = [statistics.median(t[f"{name}_off"]) for t in trees]
            verdict = "inside" if all(lo <= m <= hi for m in ms) else "NOT all inside"
            say(f"# {name}: true peak off, process medians {', '.join(f'{m:.2f}' for m in ms)} ms, are {verdict} the parent's own min .. max "
                f"{lo:.2f} .. {hi:.2f} ms of the _loudness call")
    print(json.dumps({"trees": trees, "parents": pars}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
