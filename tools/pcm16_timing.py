"""Times of 16-bit PCM in and out of the whole-track drivers (umx_hip_separate_tracks_io / umx_hip_separate_queue_io; csrc/pcm16.h,
DESIGN 19), host buffers in and out, hidden 1024, 60 s segments.

    python tools/pcm16_timing.py [--lanes 64] [--jobs 160] [--reps 5] [--parent-root <built checkout of the parent commit>] [--out FILE]

    equal       `lanes` equal 600 s tracks through umx_hip_separate_tracks (the equal case of tools/queue_timing.py), fp32, and the
                same tracks as int16 both ways through umx_hip_separate_tracks_io
    catalogue   the seeded catalogue of tools/queue_timing.py (`jobs` jobs of 90 .. 480 s) through the queue, fp32 and int16 both ways
    one lane    one 600 s track at shift offset 4033 on a one-lane context: umx_hip_separate_tracks with one track (the call behind
                umx_hip_shift_inference), fp32, and umx_hip_separate_tracks_io with int16 both ways
    reset       the same track in reset mode (UMX_FLAG_RESET_SEGMENTS) on a 14-lane context, fp32 and int16 both ways
Every case: one warm-up run, then the median of `reps` with min .. max.  One fresh process per tree (this one; with --parent-root also
a built checkout of the parent commit, which runs the fp32 rows: each fp32 row of this tree is held against the parent's own
min .. max of that row).  UMX_TIMING_ROOT tells a child which tree to load.  A first process reports the HBM the context leaves free;
if the accumulators of the longest lengths would not fit, the lengths are scaled and the table says so: one factor for the cases that
hold lanes + 2 accumulator sets (equal, catalogue), one of their own for the two that hold a single set (one lane, reset).  The int16
tracks are the fp32 ones encoded; the jobs read slices of ONE track and the outputs come from a pool of lanes + 2 buffer sets."""
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
FP32_ROWS = ("equal_f32", "catalogue_f32", "one_f32", "reset_f32")
ROW_NAMES = {"equal": "equal      {lanes} x {sec:.0f} s, umx_hip_separate_tracks", "catalogue": "catalogue  the queue, {jobs} jobs",
             "one": "one lane   one {single:.0f} s track, one-lane context", "reset": "reset      one {single:.0f} s track, reset mode, 14 lanes"}


def med(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def job_lengths(jobs, lo=90.0, hi=480.0, seed=18):
    rng = np.random.default_rng(seed)
    return [int(s * 44100) for s in rng.uniform(lo, hi, jobs)]


def child_main(a):
    pkg = ge.load_package()
    has_io = hasattr(pkg, "SampleIO")
    N = pkg.SEGMENT_SAMPLES
    lens = job_lengths(a.jobs, a.min_seconds, a.max_seconds)
    equal_len, single_len = int(a.equal_seconds * 44100), int(a.single_seconds * 44100)
    longest = max(max(lens), equal_len)
    track16 = np.clip(np.random.default_rng(5).standard_normal(2 * max(longest, single_len)) * 0.1 * 32767, -32768, 32767).astype(np.int16)  # (2,longest) interleaved
    track = track16.astype(np.float32) / np.float32(32767.0)  # what the int16 upload decodes to
    n_sets = a.lanes + 2
    # (the warm-up run touches the pages; an int16 run fills the first half of each buffer)
    pool = [] if a.probe else [[np.zeros(2 * (max(longest, single_len) if k == 0 else longest), np.float32) for _ in range(4)] for k in range(n_sets)]
    res = {"io": has_io, "lanes": a.lanes, "jobs": a.jobs, "reps": a.reps, "lengths_s": [round(x / 44100, 1) for x in lens]}
    io16 = pkg.sample_io(pkg.SAMPLE_S16, pkg.SAMPLE_S16) if has_io else None
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(a.hidden, seed=7), a.hidden)
        eng = pkg.Engine.from_file(path, segment_samples=N, tracks=a.lanes)
        import torch
        free, total = torch.cuda.mem_get_info()
        res["hbm_free_gib"], res["hbm_total_gib"] = round(free / 2**30, 1), round(total / 2**30, 1)
        print(f"(HBM free behind the {a.lanes}-lane context: {free / 2**30:.1f} of {total / 2**30:.1f} GiB)", file=sys.stderr, flush=True)
        if a.probe:
            eng.close()
            print(json.dumps({"free": free, "total": total}))
            return

        def tracks(e, lengths, io, flags=0):  # umx_hip_separate_tracks(_io) on slices of the track, one per lane
            nt = len(lengths)
            src = track16 if io is not None else track
            t0 = time.perf_counter()
            if io is None:
                au = (FP * nt)(*[src.ctypes.data_as(FP)] * nt)
                out = (FP * (4 * nt))(*[b.ctypes.data_as(FP) for k in range(nt) for b in pool[k]])
                rc = e.lib.umx_hip_separate_tracks(e.h, nt, au, (C.c_int * nt)(*lengths), (C.c_int * nt)(*[SHIFT] * nt), out, flags, None, None)
            else:
                au = (C.c_void_p * nt)(*[src.ctypes.data] * nt)
                out = (C.c_void_p * (4 * nt))(*[b.ctypes.data for k in range(nt) for b in pool[k]])
                rc = e.lib.umx_hip_separate_tracks_io(e.h, nt, au, (C.c_int * nt)(*lengths), None, (C.c_int * nt)(*[SHIFT] * nt), 4, None, out, flags,
                                                      C.byref(io), None, None)
            dt = time.perf_counter() - t0
            assert rc == 0, e.last_error()
            return dt

        def queued(e, lengths, io):
            free_sets, it = list(range(n_sets)), iter(range(len(lengths)))
            src = track16 if io is not None else track

            def nxt(_u, job):
                j = next(it, None)
                if j is None:
                    return 0
                k = free_sets.pop()
                job[0].audio, job[0].length, job[0].shift_offset, job[0].tag = C.cast(src.ctypes.data, FP), lengths[j], SHIFT, k + 1
                for t in range(4):
                    job[0].out[t] = pool[k][t].ctypes.data_as(FP)
                return 1

            def done(_u, job):
                free_sets.append(int(job[0].tag) - 1)

            t0 = time.perf_counter()
            if io is None:
                rc = e.lib.umx_hip_separate_queue(e.h, pkg.QUEUE_NEXT_FN(nxt), pkg.QUEUE_DONE_FN(done), None, 4, None, 0)
            else:
                rc = e.lib.umx_hip_separate_queue_io(e.h, pkg.QUEUE_NEXT_FN(nxt), pkg.QUEUE_DONE_FN(done), None, 4, None, 0, C.byref(io))
            dt = time.perf_counter() - t0
            assert rc == 0, e.last_error()
            return dt

        def timed(name, fn):
            for fmt, io in (("f32", None), ("s16", io16)):
                if fmt == "s16" and not has_io:
                    continue
                res[f"{name}_{fmt}"] = [fn(io) * 1e3 for _ in range(a.reps + 1)][1:]  # run 0 warms up (buffers grow, pages are touched)
                print(f"({name} {fmt} is done)", file=sys.stderr, flush=True)

        timed("equal", lambda io: tracks(eng, [equal_len] * a.lanes, io))
        eng.close()  # a fresh context: the per-lane accumulators and the queue's pool need not fit together
        eng = pkg.Engine.from_file(path, segment_samples=N, tracks=a.lanes)
        timed("catalogue", lambda io: queued(eng, lens, io))
        eng.close()
        one = pkg.Engine.from_file(path, segment_samples=N)
        timed("one", lambda io: tracks(one, [single_len], io))
        one.close()
        rst = pkg.Engine.from_file(path, segment_samples=N, tracks=RESET_LANES)
        timed("reset", lambda io: tracks(rst, [single_len], io, FLAG_RESET))
        rst.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--jobs", type=int, default=160)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--equal-seconds", type=float, default=600.0)
    ap.add_argument("--single-seconds", type=float, default=None, help="the one-lane and reset-mode track (default: --equal-seconds)")
    ap.add_argument("--min-seconds", type=float, default=90.0, help="catalogue: the shortest job")
    ap.add_argument("--max-seconds", type=float, default=480.0, help="catalogue: the longest job")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--probe", action="store_true", help="(a fresh process) only report the HBM free behind the context")
    ap.add_argument("--child", action="store_true", help="(the fresh processes) run the cases of the tree UMX_TIMING_ROOT names, one JSON line")
    ap.add_argument("--out", default=None, help="also write the table here")
    a = ap.parse_args()
    if a.single_seconds is None:
        a.single_seconds = a.equal_seconds
    if a.child:
        return child_main(a)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def child(root, probe=False):
        env = dict(os.environ)
        env.pop("UMX_HIP_LIB", None)
        env.pop("UMX_TIMING_ROOT", None)
        if root:
            env["UMX_TIMING_ROOT"] = str(Path(root).resolve())
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--lanes", str(a.lanes), "--jobs", str(a.jobs), "--hidden", str(a.hidden),
               "--equal-seconds", str(a.equal_seconds), "--single-seconds", str(a.single_seconds), "--min-seconds", str(a.min_seconds), "--max-seconds", str(a.max_seconds), "--reps", str(a.reps)]
        if probe:
            cmd.append("--probe")
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=1100)  # (its progress lines go to this process's stderr)
        assert r.returncode == 0, r.stdout[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    # The accumulators must fit the HBM the context leaves free (a device may be shared or partitioned): 44 B per frame of a set, and
    # 20 B more with int16 both ways; if they do not, every length is scaled down by one factor, and the table says so.
    mem = child(None, probe=True)
    set_bytes = lambda secs: 64 * (int(secs * 44100) + 22050) * 9 // 8  # noqa: E731 - 1/8 slack
    need = (a.lanes + 2) * set_bytes(max(a.equal_seconds, a.max_seconds))
    scale = min(1.0, 0.8 * mem["free"] / need)
    asked = (a.equal_seconds, a.min_seconds, a.max_seconds)
    if scale < 1.0:
        a.equal_seconds, a.min_seconds, a.max_seconds = (round(v * scale, 1) for v in asked)
    single_asked = a.single_seconds  # one set at a time (the reset context's free HBM is at least the large context's)
    single_scale = min(1.0, 0.8 * mem["free"] / set_bytes(single_asked))
    a.single_seconds = round(single_asked * single_scale, 1)
    par = child(a.parent_root) if a.parent_root else None
    if par:
        print("(the process with the parent's library is done)", file=sys.stderr, flush=True)
    tree = child(None)
    import torch
    say(f"# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); torch {torch.__version__}, HIP {torch.version.hip}")
    say(f"# hidden {a.hidden}, segment_samples 2646000 (stride 1984500), synthetic weights, shift offset {SHIFT}, pageable host buffers in and out")
    say(f"# wall ms of the bare C calls: 1 warm-up run, median of {a.reps} (min .. max); one fresh process per tree")
    if scale < 1.0:
        say(f"# NOTE: {mem['free'] / 2**30:.1f} of {mem['total'] / 2**30:.1f} GiB of HBM were free behind the {a.lanes}-lane context and the accumulators of "
            f"{a.lanes + 2} x {max(asked[0], asked[2]):.0f} s with int16 both ways need {need / 2**30:.1f} GiB: every length below is scaled by {scale:.3f} "
            f"(equal: {a.equal_seconds:.1f} s; catalogue: {a.min_seconds:.1f} .. {a.max_seconds:.1f} s); one lane and reset hold one set: "
            f"{a.single_seconds:.1f} s" + ("" if single_scale == 1.0 else f" (scaled by {single_scale:.3f})"))
    L = tree["lengths_s"]
    say(f"# catalogue: {a.jobs} jobs of {min(L):.0f} .. {max(L):.0f} s (seeded), {sum(L):.0f} s of audio; bytes across PCIe per stereo frame: "
        f"fp32 8 up + 32 down, int16 4 up + 16 down")
    for name, label in ROW_NAMES.items():
        label = label.format(lanes=a.lanes, sec=a.equal_seconds, single=a.single_seconds, jobs=a.jobs)
        f32, s16 = tree[f"{name}_f32"], tree[f"{name}_s16"]
        say(f"{label:<58} fp32  {med(f32):>28} ms  (this tree)")
        if par:
            say(f"{label:<58} fp32  {med(par[f'{name}_f32']):>28} ms  (parent commit)")
        say(f"{label:<58} int16 {med(s16):>28} ms  (this tree)   int16 / fp32 = {statistics.median(s16) / statistics.median(f32):.3f}")
    if par:
        for name in ROW_NAMES:
            new, old = tree[f"{name}_f32"], par[f"{name}_f32"]
            m = statistics.median(new)
            inside = min(old) <= m <= max(old)
            verdict = "inside the parent's min .. max" if inside else ("BELOW the parent's min .. max (faster)" if m < min(old) else "ABOVE the parent's min .. max (SLOWER)")
            say(f"# {name}, fp32: this tree's median {m:.1f} ms against the parent's {min(old):.1f} .. {max(old):.1f} ms (median {statistics.median(old):.1f}): {verdict}")
    print(json.dumps({"tree": tree, "parent": par}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
