"""Times of the stem mix matrix (umx_hip_separate_tracks_mix; csrc/stem_mix.h) on a whole track, host buffers in and out.

    python tools/mix_timing.py [--seconds 600] [--hidden 1024] [--reps 10] [--rounds 3] [--parent-root <built checkout of the parent commit>] [--out FILE]

Per mode -- carry mode on a one-lane context, reset mode (UMX_FLAG_RESET_SEGMENTS) on a 14-lane context -- the wall time of
    plain     umx_hip_shift_inference, four stems downloaded
    identity  the mix entry point with the identity matrix (four outputs; no kernel is launched for it)
    n_out 2   vocals + accompaniment (bass + drums + other)
    n_out 1   karaoke (mixture - vocals)
the four alternated call by call on ONE context, so that drift hits them alike; one warm-up round, then `reps` timed rounds; medians
with min .. max.  The plain call's run-to-run spread is taken over `rounds` fresh processes of this tree (max - min of their medians);
with --parent-root the same processes alternate with ones that run THIS file on the package and library of a built checkout of the
parent commit (UMX_TIMING_ROOT tells the child which tree to load; --plain-only needs nothing of the mix), plain call only.
stem_mix_kernel's own milliseconds come from device events around one whole-track launch on device buffers, in place as the track
path runs it."""
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

ROOT = Path(os.environ.get("UMX_TIMING_ROOT") or Path(__file__).resolve().parent.parent).resolve()  # (the child processes: see --parent-root)
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

FP = C.POINTER(C.c_float)
IDENTITY = np.eye(4, 5, dtype=np.float32)
TWO = np.array([[0, 0, 0, 1, 0], [1, 1, 1, 0, 0]], np.float32)
ONE = np.array([[0, 0, 0, -1, 1]], np.float32)
RESET_LANES = 14  # a 600 s track is 14 segments: one call in reset mode


def med(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--segment", type=int, default=None, help="segment_samples (default: the production 60 s)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="fresh processes for the plain call's run-to-run spread")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--plain-only", action="store_true", help="(the child processes) plain calls only, one JSON line")
    ap.add_argument("--out", default=None, help="also write the table here")
    a = ap.parse_args()
    if a.rounds < 2 and not a.plain_only:
        ap.error("--rounds: a run-to-run spread needs at least 2 fresh processes")
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
        cmd = [sys.executable, str(Path(__file__).resolve()), "--plain-only", "--seconds", str(a.seconds), "--hidden", str(a.hidden), "--reps", str(a.reps)]
        if a.segment:
            cmd += ["--segment", str(a.segment)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    # the fresh processes first, before this one opens the GPU: parent, this tree, parent, this tree, ...
    rounds = {"parent": [], "tree": []}
    if not a.plain_only:
        for _ in range(a.rounds):
            if a.parent_root:
                rounds["parent"].append(child(a.parent_root))
                print("(a process with the parent's library is done)", file=sys.stderr, flush=True)
            rounds["tree"].append(child(None))
            print("(a process of this tree is done)", file=sys.stderr, flush=True)

    pkg = ge.load_package()
    import torch
    torch.zeros(1).cuda()
    N = a.segment or pkg.SEGMENT_SAMPLES
    L = int(a.seconds * 44100)
    xi = np.ascontiguousarray(pkg.ggml.synth_audio(L, 5).T).ravel()  # (2,L) interleaved
    bufs = [np.empty(2 * L, np.float32) for _ in range(4)]
    outs = (FP * 4)(*[b.ctypes.data_as(FP) for b in bufs])
    audio, length, shift = (FP * 1)(xi.ctypes.data_as(FP)), (C.c_int * 1)(L), (C.c_int * 1)(4033)

    def plain(eng, flags):
        t0 = time.perf_counter()
        rc = eng.lib.umx_hip_shift_inference(eng.h, xi.ctypes.data_as(FP), L, 4033, outs, flags, None, None)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, eng.last_error()
        return dt

    def mixed(eng, flags, gains):
        g = np.ascontiguousarray(gains).ravel()
        t0 = time.perf_counter()
        rc = eng.lib.umx_hip_separate_tracks_mix(eng.h, 1, audio, length, None, shift, gains.shape[0], g.ctypes.data_as(FP), outs, flags, None, None)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, eng.last_error()
        return dt

    result = {"seconds": a.seconds, "frames": L, "segment_samples": N, "hidden": a.hidden, "reps": a.reps}
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(a.hidden, seed=7), a.hidden)
        for mode, lanes, flags in (("carry", 1, 0), ("reset", RESET_LANES, pkg.FLAG_RESET_SEGMENTS)):
            eng = pkg.Engine.from_file(path, segment_samples=N, tracks=lanes)  # one context alive at a time
            calls = {"plain": lambda: plain(eng, flags)}
            if not a.plain_only:
                calls.update({"identity": lambda: mixed(eng, flags, IDENTITY), "n_out 2": lambda: mixed(eng, flags, TWO),
                              "n_out 1": lambda: mixed(eng, flags, ONE)})
            times = {k: [] for k in calls}
            for rep in range(a.reps + 1):  # round 0 warms up
                for k, f in calls.items():
                    dt = f()
                    if rep:
                        times[k].append(dt)
            eng.close()
            result[mode] = times
            print(f"({mode} mode is done)", file=sys.stderr, flush=True)
        if a.plain_only:
            print(json.dumps(result))
            return
        # the kernel alone: one launch over the whole track's frames on device buffers, in place, between device events
        eng = pkg.Engine.from_file(path, segment_samples=N)
        dev = [torch.randn(2 * L, device="cuda") for _ in range(5)]
        kernel = {}
        for name, G in (("n_out 2", TWO), ("n_out 1", ONE)):
            ms = []
            for rep in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.mix_stems_device(G, [d.data_ptr() for d in dev[:4]], dev[4].data_ptr(), L, [dev[m].data_ptr() for m in range(G.shape[0])],
                                     hip_stream=torch.cuda.current_stream().cuda_stream)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms.append(e0.elapsed_time(e1))
            cols = bin(pkg.mix_columns(G)).count("1")
            kernel[name] = (ms, (cols + G.shape[0]) * 8 * L / 1e9)
        eng.close()

    try:
        box = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
        names = sorted({ln.split(":", 1)[1].strip() for ln in box.splitlines() if "Marketing Name" in ln and "Instinct" in ln})
    except Exception:  # noqa: BLE001 - the identity line is a courtesy
        names = []
    say(f"# {', '.join(names) or torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); torch {torch.__version__}, HIP {torch.version.hip}")
    say(f"# track {a.seconds:.0f} s ({L} frames), segment_samples {N}, hidden {a.hidden}, synthetic weights, shift offset 4033, pageable host buffers in and out")
    say(f"# wall ms of the bare C calls: 1 warm-up round, median of {a.reps} (min .. max); the four calls of a mode alternate on one context")
    say("# carry: one-lane context; reset: UMX_FLAG_RESET_SEGMENTS on a 14-lane context")
    say(f"{'mode':>6} {'plain (4 stems)':>26} {'identity mix (4)':>26} {'n_out 2 (voc + acc)':>26} {'n_out 1 (karaoke)':>26}")
    for mode in ("carry", "reset"):
        t = result[mode]
        say(f"{mode:>6} {med(t['plain']):>26} {med(t['identity']):>26} {med(t['n_out 2']):>26} {med(t['n_out 1']):>26}")
    for mode in ("carry", "reset"):
        tree = [statistics.median(r[mode]["plain"]) for r in rounds["tree"]]
        spread = max(tree) - min(tree)
        say(f"# {mode}: plain call in {len(tree)} fresh processes of this tree: medians {', '.join(f'{v:.2f}' for v in tree)} ms -> run-to-run spread {spread:.2f} ms")
        if rounds["parent"]:
            par = [statistics.median(r[mode]["plain"]) for r in rounds["parent"]]
            d = statistics.median(tree) - statistics.median(par)
            say(f"# {mode}: plain call in fresh processes of the parent commit's tree, alternated with those: medians {', '.join(f'{v:.2f}' for v in par)} ms; "
                f"this tree - parent = {d:+.2f} ms: {'no slower (within the spread)' if d <= spread else 'SLOWER than the spread'}")
        t = result[mode]
        d = statistics.median(t["identity"]) - statistics.median(t["plain"])
        say(f"# {mode}: identity mix - plain (same context, alternated) = {d:+.2f} ms: {'no slower (within the spread)' if d <= spread else 'SLOWER than the spread'}; "
            f"n_out 2 saves {statistics.median(t['plain']) - statistics.median(t['n_out 2']):.2f} ms, n_out 1 saves {statistics.median(t['plain']) - statistics.median(t['n_out 1']):.2f} ms")
    for name, (ms, gb) in kernel.items():
        m = statistics.median(ms)
        say(f"# stem_mix_kernel, {name}, one launch over {L} frames in place (device events): {med(ms)} ms, {gb:.2f} GB moved, {gb / m:.2f} TB/s")
    say("# the identity matrix in place launches nothing (every row is its own stem)")
    result.update({"rounds": rounds, "kernel_ms": {k: v[0] for k, v in kernel.items()}})
    print(json.dumps(result))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
