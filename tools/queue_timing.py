"""Times of the track queue (umx_hip_separate_queue; csrc/engine_queue.h), host buffers in and out, hidden 1024, 60 s segments.

    python tools/queue_timing.py [--lanes 64] [--jobs 160] [--reps 5] [--parent-root <built checkout of the parent commit>] [--out FILE]

    catalogue   a fixed list of `jobs` jobs, lengths from a seeded generator between 90 and 480 s, shift offset 4033:
                  the queue                       against
                  separate_many in groups of `lanes`, in list order (the path without the queue)
                both walls, both call counts and umx_hip_queue_plan's prediction; the queue's count must EQUAL the prediction
    equal       `lanes` equal 600 s jobs (the schedule of umx_hip_separate_tracks): the queue against umx_hip_separate_tracks
    plain       umx_hip_shift_inference of one 600 s track on a one-lane context (the figure of profiles/mix_timing.txt)
Every case runs in a fresh process per tree (this one; with --parent-root also a built checkout of the parent commit: each row of
this tree is compared with the parent's row, and the margin is the parent's own run-to-run spread, max - min over its runs; a parent
without a queue gives the margins of `equal` and `plain` only).  UMX_TIMING_ROOT tells a child which tree to load.  A first process reports the HBM the context leaves free; if the accumulators of the longest lengths would not fit, every
length is scaled by one factor and the table says so.  The jobs read slices of ONE synthetic track and the outputs come from a pool of lanes + 2 buffer sets: a job's stems are
not kept."""
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


def med(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def job_lengths(jobs, lo=90.0, hi=480.0, seed=18):
    rng = np.random.default_rng(seed)
    return [int(s * 44100) for s in rng.uniform(lo, hi, jobs)]


def child_main(a):
    pkg = ge.load_package()
    has_queue = hasattr(pkg.Engine, "separate_queue")
    N = pkg.SEGMENT_SAMPLES
    stride = int(0.75 * N)
    lens = job_lengths(a.jobs, a.min_seconds, a.max_seconds)
    equal_len = int(a.equal_seconds * 44100)
    longest = max(max(lens), equal_len)
    track = (np.random.default_rng(5).standard_normal(2 * longest).astype(np.float32) * np.float32(0.1))  # (2,longest) interleaved
    n_sets = a.lanes + 2
    pool = [] if a.probe else [[np.zeros(2 * longest, np.float32) for _ in range(4)] for _ in range(n_sets)]  # (the warm-up run touches the pages)
    res = {"queue": has_queue, "lanes": a.lanes, "jobs": a.jobs, "lengths_s": [round(x / 44100, 1) for x in lens], "reps": a.reps}
    segs = [-(-(L + max(22050 - SHIFT, SHIFT)) // stride) for L in lens]
    res["seg_counts"] = segs
    res["grouped_calls"] = sum(max(segs[i:i + a.lanes]) for i in range(0, a.jobs, a.lanes))
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(a.hidden, seed=7), a.hidden)
        eng = pkg.Engine.from_file(path, segment_samples=N, tracks=a.lanes)
        lib = eng.lib
        import torch
        free, total = torch.cuda.mem_get_info()
        res["hbm_free_gib"], res["hbm_total_gib"] = round(free / 2**30, 1), round(total / 2**30, 1)
        print(f"(HBM free behind the {a.lanes}-lane context: {free / 2**30:.1f} of {total / 2**30:.1f} GiB)", file=sys.stderr, flush=True)
        if a.probe:
            eng.close()
            print(json.dumps({"free": free, "total": total}))
            return

        def tracks(lengths):  # umx_hip_separate_tracks on up to `lanes` slices of the track
            nt = len(lengths)
            au = (FP * nt)(*[track.ctypes.data_as(FP)] * nt)
            out = (FP * (4 * nt))(*[b.ctypes.data_as(FP) for k in range(nt) for b in pool[k]])
            t0 = time.perf_counter()
            rc = lib.umx_hip_separate_tracks(eng.h, nt, au, (C.c_int * nt)(*lengths), (C.c_int * nt)(*[SHIFT] * nt), out, 0, None, None)
            dt = time.perf_counter() - t0
            assert rc == 0, eng.last_error()
            return dt

        def grouped(lengths):
            return sum(tracks(lengths[i:i + a.lanes]) for i in range(0, len(lengths), a.lanes))

        def queued(lengths):
            free, it = list(range(n_sets)), iter(range(len(lengths)))

            def nxt(_u, job):
                j = next(it, None)
                if j is None:
                    return 0
                k = free.pop()
                job[0].audio, job[0].length, job[0].shift_offset, job[0].tag = track.ctypes.data_as(FP), lengths[j], SHIFT, k + 1
                for t in range(4):
                    job[0].out[t] = pool[k][t].ctypes.data_as(FP)
                return 1

            def done(_u, job):
                free.append(int(job[0].tag) - 1)

            t0 = time.perf_counter()
            rc = lib.umx_hip_separate_queue(eng.h, pkg.QUEUE_NEXT_FN(nxt), pkg.QUEUE_DONE_FN(done), None, 4, None, 0)
            dt = time.perf_counter() - t0
            assert rc == 0, eng.last_error()
            return dt, eng.queue_calls()

        cases = {"equal_tracks": lambda: tracks([equal_len] * a.lanes), "catalogue_grouped": lambda: grouped(lens)}
        if has_queue:
            res["plan_calls"] = pkg.queue_plan(a.lanes, segs)[2]
            cases["equal_queue"] = lambda: queued([equal_len] * a.lanes)
            cases["catalogue_queue"] = lambda: queued(lens)
        first_queue = next((k for k in cases if k.endswith("_queue")), None)
        for name, fn in cases.items():
            if name == first_queue:  # a fresh context: the grouped path's per-lane accumulators and the queue's pool need not fit together
                eng.close()
                eng = pkg.Engine.from_file(path, segment_samples=N, tracks=a.lanes)
            walls = []
            for rep in range(a.reps + 1):  # run 0 warms up (buffers grow, pages are touched)
                r = fn()
                dt, calls = r if isinstance(r, tuple) else (r, None)
                if calls is not None:
                    res[name + "_calls"] = calls
                if rep:
                    walls.append(dt * 1e3)
            res[name] = walls
            print(f"({name} is done)", file=sys.stderr, flush=True)
        eng.close()
        one = pkg.Engine.from_file(path, segment_samples=N)
        outs = (FP * 4)(*[b.ctypes.data_as(FP) for b in pool[0]])
        walls = []
        for rep in range(2 * a.reps + 1):
            t0 = time.perf_counter()
            rc = one.lib.umx_hip_shift_inference(one.h, track.ctypes.data_as(FP), equal_len, SHIFT, outs, 0, None, None)
            dt = time.perf_counter() - t0
            assert rc == 0, one.last_error()
            if rep:
                walls.append(dt * 1e3)
        res["plain"] = walls
        one.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--jobs", type=int, default=160)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--equal-seconds", type=float, default=600.0)
    ap.add_argument("--min-seconds", type=float, default=90.0, help="catalogue: the shortest job")
    ap.add_argument("--max-seconds", type=float, default=480.0, help="catalogue: the longest job")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--probe", action="store_true", help="(a fresh process) only report the HBM free behind the context")
    ap.add_argument("--child", action="store_true", help="(the fresh processes) run the cases of the tree UMX_TIMING_ROOT names, one JSON line")
    ap.add_argument("--out", default=None, help="also write the table here")
    a = ap.parse_args()
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
               "--equal-seconds", str(a.equal_seconds), "--min-seconds", str(a.min_seconds), "--max-seconds", str(a.max_seconds), "--reps", str(a.reps)]
        if probe:
            cmd.append("--probe")
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=1100)  # (its progress lines go to this process's stderr)
        assert r.returncode == 0, r.stdout[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    # The accumulators of both cases must fit the HBM the context leaves free (a device may be shared or partitioned): if they do
    # not, every length is scaled down by one factor, and the table says so.
    mem = child(None, probe=True)
    set_bytes = lambda secs: 44 * (int(secs * 44100) + 22050) * 9 // 8  # noqa: E731 - in, 4 stems, weight sum; 1/8 slack
    need = (a.lanes + 2) * set_bytes(max(a.equal_seconds, a.max_seconds))
    scale = min(1.0, 0.8 * mem["free"] / need)
    asked = (a.equal_seconds, a.min_seconds, a.max_seconds)
    if scale < 1.0:
        a.equal_seconds, a.min_seconds, a.max_seconds = (round(v * scale, 1) for v in asked)
    par = child(a.parent_root) if a.parent_root else None
    if par:
        print("(the process with the parent's library is done)", file=sys.stderr, flush=True)
    tree = child(None)
    import torch
    say(f"# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); torch {torch.__version__}, HIP {torch.version.hip}")
    say(f"# hidden {a.hidden}, segment_samples 2646000 (stride 1984500), {a.lanes} track lanes, synthetic weights, shift offset {SHIFT}, pageable host buffers in and out")
    say(f"# wall ms of the bare C calls: 1 warm-up run, median of {a.reps} (min .. max); one fresh process per tree")
    if scale < 1.0:
        say(f"# NOTE: {mem['free'] / 2**30:.1f} of {mem['total'] / 2**30:.1f} GiB of HBM were free behind the {a.lanes}-lane context and the accumulators of "
            f"{a.lanes + 2} x {max(asked[0], asked[2]):.0f} s need {need / 2**30:.1f} GiB: every length below is scaled by {scale:.3f} "
            f"(equal: {a.equal_seconds:.1f} s; catalogue: {a.min_seconds:.1f} .. {a.max_seconds:.1f} s)")
    L = tree["lengths_s"]
    say(f"# catalogue: {a.jobs} jobs of {min(L):.0f} .. {max(L):.0f} s (seeded), {sum(L):.0f} s of audio, {sum(tree['seg_counts'])} segments")
    q, g = tree["catalogue_queue"], tree["catalogue_grouped"]
    qc, gc, pc = tree["catalogue_queue_calls"], tree["grouped_calls"], tree["plan_calls"]
    say(f"catalogue  queue                 {med(q):>28} ms  {qc} calls (umx_hip_queue_plan: {pc}: {'equal' if qc == pc else 'NOT EQUAL'})  {statistics.median(q) / qc:.1f} ms per call")
    say(f"catalogue  groups of {a.lanes:<3} in order {med(g):>28} ms  {gc} calls  {statistics.median(g) / gc:.1f} ms per call")
    say(f"# catalogue: queue / grouped wall = {statistics.median(q) / statistics.median(g):.3f}, calls {qc} / {gc} = {qc / gc:.3f}; "
        f"grouped run-to-run spread {max(g) - min(g):.1f} ms")
    assert qc == pc, (qc, pc)
    eq, et = tree["equal_queue"], tree["equal_tracks"]
    say(f"equal      queue, {a.lanes} x {a.equal_seconds:.0f} s      {med(eq):>28} ms  {tree['equal_queue_calls']} calls")
    say(f"equal      umx_hip_separate_tracks {med(et):>28} ms  (this tree)")
    say(f"plain      umx_hip_shift_inference, one {a.equal_seconds:.0f} s track, one-lane context {med(tree['plain']):>24} ms  (this tree)")
    if par:
        pt, pp = par["equal_tracks"], par["plain"]
        say(f"equal      umx_hip_separate_tracks {med(pt):>28} ms  (parent commit)")
        say(f"plain      umx_hip_shift_inference {med(pp):>28} ms  (parent commit)")
        rows = [("equal: this tree's umx_hip_separate_tracks - parent's", et, pt), ("plain: this tree - parent", tree["plain"], pp)]
        if par["queue"]:  # the parent has a queue of its own: each queue row against the parent's row
            pq, pe = par["catalogue_queue"], par["equal_queue"]
            say(f"catalogue  queue                 {med(pq):>28} ms  {par['catalogue_queue_calls']} calls  (parent commit)")
            say(f"equal      queue                 {med(pe):>28} ms  {par['equal_queue_calls']} calls  (parent commit)")
            rows = [("catalogue: queue - parent's queue", q, pq), ("equal: queue - parent's queue", eq, pe)] + rows
        else:
            rows.insert(0, ("equal: queue - parent's umx_hip_separate_tracks", eq, pt))
        for what, new, old in rows:
            d, spread = statistics.median(new) - statistics.median(old), max(old) - min(old)
            say(f"# {what} = {d:+.1f} ms; the parent's run-to-run spread (max - min of its {len(old)} runs) is {spread:.1f} ms: "
                f"{'no slower (within the spread)' if d <= spread else 'SLOWER than the spread'}")
    cap = lambda s: int(s * 44100 + 22050 - SHIFT) * 9 // 8  # noqa: E731 - a set's capacity in frames (grow-only, 1/8 slack)
    say(f"# HBM of the accumulator pool in the catalogue run: {a.lanes + 2} sets x 44 bytes x {cap(max(L))} frames (the longest job, {max(L):.0f} s, + 1/8) "
        f"= {(a.lanes + 2) * 44 * cap(max(L)) / 2**30:.1f} GiB at most (a set grows only when a job needs it); {tree['hbm_free_gib']} of {tree['hbm_total_gib']} GiB "
        f"were free behind the {a.lanes}-lane context")
    print(json.dumps({"tree": tree, "parent": par}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
