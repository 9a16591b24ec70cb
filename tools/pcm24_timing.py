"""Times of packed 24-bit PCM in and out of the whole-track drivers (UMX_SAMPLE_S24; csrc/pcm24.h) beside fp32 and int16,
host buffers in and out, hidden 1024, 60 s segments.

    python tools/pcm24_timing.py [--lanes 64] [--jobs 160] [--reps 5] [--rounds 2] [--parent-root <built checkout of the parent commit>] [--out FILE]
    python tools/pcm24_timing.py --kernel    the three 24-bit kernels alone on a 600 s track with four outputs, beside the int16 kernels,
                                             timed with stream events in one process

    one lane    one 600 s track at shift offset 4033 on a one-lane context (umx_hip_separate_tracks_io)
    reset       the same track in reset mode (UMX_FLAG_RESET_SEGMENTS) on a 14-lane context
    catalogue   the seeded catalogue of tools/levels_timing.py through the queue (umx_hip_separate_queue_io)
Each with the same format on both sides: F32 / F32, S16 / S16 and S24 / S24 (a tree without UMX_SAMPLE_S24 -- the parent commit -- runs
the first two: the rows this tree's F32 and S16 rows are held against).  Every form: one warm-up run, then `reps` runs, the forms
alternating; one fresh process per tree and round, the trees alternating over `rounds` rounds (UMX_TIMING_ROOT tells a child which tree
to load); a row is the median of a tree's rounds x reps runs with min .. max."""
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
FORMS = ("f32", "s16", "s24")
FRAME_BYTES = {"f32": 8, "s16": 4, "s24": 6}
CASES = {"one": "one lane   one {single:.0f} s track, one-lane context", "reset": "reset      one {single:.0f} s track, reset mode, 14 lanes",
         "catalogue": "catalogue  the queue, {jobs} jobs on {lanes} lanes"}


def med(v):
    return f"{statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})"


def job_lengths(jobs, lo, hi, seed=18):
    rng = np.random.default_rng(seed)
    return [int(s * 44100) for s in rng.uniform(lo, hi, jobs)]


def child_main(a):
    pkg = ge.load_package()
    forms = [f for f in FORMS if f != "s24" or hasattr(pkg, "SAMPLE_S24")]
    N = pkg.SEGMENT_SAMPLES
    lens = job_lengths(a.jobs, a.min_seconds, a.max_seconds) if a.jobs > 0 else [0]
    single_len = int(a.single_seconds * 44100)
    longest = max(max(lens), single_len)
    noise = np.random.default_rng(5).standard_normal(2 * longest) * 0.4
    audio = {"f32": np.clip(noise, -1, 1).astype(np.float32), "s16": np.clip(noise * 32767, -32768, 32767).astype(np.int16)}
    io = {"f32": pkg.sample_io(), "s16": pkg.sample_io(pkg.SAMPLE_S16, pkg.SAMPLE_S16)}
    if "s24" in forms:
        q = np.clip(noise * 8388608, -8388608, 8388607).astype(np.int32).reshape(-1, 2).T
        audio["s24"], io["s24"] = pkg.pcm24_pack(q), pkg.sample_io(pkg.SAMPLE_S24, pkg.SAMPLE_S24)
    n_sets = a.lanes + 2
    # output buffers of 8 bytes a frame, so that every format fits; set 0 also takes the single track (pageable, touched by the warm-up)
    pool = [[np.zeros(8 * (longest if k == 0 else max(lens)), np.uint8) for _ in range(4)] for k in range(n_sets)]
    res = {"forms": forms, "lengths_s": [round(x / 44100, 1) for x in lens]}
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(a.hidden, seed=7), a.hidden)

        def tracks(e, length, form, flags):
            au = (C.c_void_p * 1)(audio[form].ctypes.data)
            out = (C.c_void_p * 4)(*[b.ctypes.data for b in pool[0]])
            ln, sh = (C.c_int * 1)(length), (C.c_int * 1)(SHIFT)
            t0 = time.perf_counter()
            rc = e.lib.umx_hip_separate_tracks_io(e.h, 1, au, ln, None, sh, 4, None, out, flags, C.byref(io[form]), None, None)
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
                job[0].audio, job[0].length, job[0].shift_offset, job[0].tag = C.cast(audio[form].ctypes.data, FP), lens[j], SHIFT, k + 1
                for t in range(4):
                    job[0].out[t] = C.cast(pool[k][t].ctypes.data, FP)
                return 1

            def done(_u, job):
                free_sets.append(int(job[0].tag) - 1)

            t0 = time.perf_counter()
            rc = e.lib.umx_hip_separate_queue_io(e.h, pkg.QUEUE_NEXT_FN(nxt), pkg.QUEUE_DONE_FN(done), None, 4, None, 0, C.byref(io[form]))
            dt = time.perf_counter() - t0
            assert rc == 0, e.last_error()
            return dt

        def timed(name, fn):
            runs = {f: [] for f in forms}
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
    packed = [torch.zeros(6 * n + 8, dtype=torch.uint8, device="cuda") for _ in range(4)]
    acc = torch.zeros(28, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    src, p16, p24, hs = [b.data_ptr() for b in bufs], [p.data_ptr() for p in packed], [p.data_ptr() for p in packed], st.cuda_stream
    p24odd = [p + 6 for p in p24]  # 2 mod 4: a head frame, as every region that starts at an odd frame of its track has
    eng.levels_device(src, n, acc.data_ptr(), hip_stream=hs)  # the peaks the rescaled encodes form their divisor from
    cases = [("pcm16_decode_kernel", 12, lambda: eng.pcm16_decode_device(p16[0], n, src[0], hip_stream=hs)),
             ("pcm24_decode_kernel", 14, lambda: eng.pcm24_decode_device(p24[0], n, src[0], hip_stream=hs)),
             ("pcm24_decode_kernel, address 2 mod 4", 14, lambda: eng.pcm24_decode_device(p24odd[0], n, src[0], hip_stream=hs)),
             ("encode_kernel<SampleS16> x 4, dither", 48, lambda: eng.pcm16_encode_device(src, n, p16, 0, 7, hip_stream=hs)),
             ("encode_kernel<SampleS24> x 4, dither", 56, lambda: eng.pcm24_encode_device(src, n, p24, 0, 7, hip_stream=hs)),
             ("encode_kernel<SampleS24> x 4, dither, 2 mod 4", 56, lambda: eng.pcm24_encode_device(src, n, p24odd, 1, 7, hip_stream=hs)),
             ("encode_kernel<SampleS24> x 4, no dither", 56, lambda: eng.pcm24_encode_device(src, n, p24, 0, None, hip_stream=hs)),
             ("encode_rescaled_kernel<SampleS16> x 4, dither", 48, lambda: eng.pcm16_encode_rescaled_device(src, n, p16, acc.data_ptr(), 0, 7, hip_stream=hs)),
             ("encode_rescaled_kernel<SampleS24> x 4, dither", 56, lambda: eng.pcm24_encode_rescaled_device(src, n, p24, acc.data_ptr(), 0, 7, hip_stream=hs))]
    lines = [f"# {torch.cuda.get_device_name(0)}; {n} frames ({a.single_seconds:.0f} s), stream events, 1 warm-up launch, median of {a.reps} (min .. max); "
             "GB/s: bytes read + written over the median"]
    order = [0, 1, 2, 3, 4, 5, 6, 7, 8]
    for i in order[3:] + order[:3]:  # (the decodes last: they write over the fp32 input of buffer 0)
        what, bytes_per_frame, call = cases[i]
        ms = []
        for _ in range(a.reps + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            call()
            t1.record(st)
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        v = ms[1:]
        m = statistics.median(v)
        lines.append(f"{what:<46} {m * 1e3:9.1f} us ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})  {bytes_per_frame * n / (m * 1e-3) / 1e9:7.0f} GB/s")
    eng.close()
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--jobs", type=int, default=160, help="0: no catalogue")
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--single-seconds", type=float, default=600.0)
    ap.add_argument("--min-seconds", type=float, default=90.0 * 0.578, help="catalogue: the shortest job (profiles/pcm16_timing.txt ran 53 .. 277 s)")
    ap.add_argument("--max-seconds", type=float, default=480.0 * 0.578, help="catalogue: the longest job")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="processes per tree, the trees alternating")
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

    def pooled(runs):
        out = dict(runs[0])
        for r in runs[1:]:
            for k, v in r.items():
                if k.split("_")[-1] in FORMS:
                    out[k] = out[k] + v
        return out

    par_runs, tree_runs = [], []
    for _ in range(a.rounds):  # parent, tree, parent, tree, ...
        if a.parent_root:
            par_runs.append(child(a.parent_root))
        tree_runs.append(child(None))
    par, tree = (pooled(par_runs) if par_runs else None), pooled(tree_runs)
    import torch
    say(f"# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); torch {torch.__version__}, HIP {torch.version.hip}")
    say(f"# hidden {a.hidden}, segment_samples 2646000 (stride 1984500), synthetic weights, shift offset {SHIFT}, pageable host buffers, the same format both ways")
    say(f"# wall ms of the bare C calls: per process 1 warm-up run and {a.reps} runs, the forms alternating; {a.rounds} fresh processes per tree, the trees "
        f"alternating; median of a tree's {a.rounds * a.reps} runs (min .. max)")
    say("# bytes across PCIe per stereo frame: fp32 8 up + 32 down, int16 4 up + 16 down, 24-bit 6 up + 24 down")
    L = tree["lengths_s"]
    if a.jobs > 0:
        say(f"# catalogue: {a.jobs} jobs of {min(L):.0f} .. {max(L):.0f} s (seeded), {sum(L):.0f} s of audio")
    for name, label in CASES.items():
        if f"{name}_f32" not in tree:
            continue
        label = label.format(lanes=a.lanes, single=a.single_seconds, jobs=a.jobs)
        base = statistics.median(tree[f"{name}_f32"])
        for f in FORMS:
            if par and f"{name}_{f}" in par:
                say(f"{label:<52} {f.upper()} / {f.upper()}, parent commit  {med(par[f'{name}_{f}']):>28} ms")
            v = tree[f"{name}_{f}"]
            say(f"{label:<52} {f.upper()} / {f.upper()}, this tree      {med(v):>28} ms   / F32 of this tree = {statistics.median(v) / base:.3f}")
        for f in FORMS:
            if par and f"{name}_{f}" in par:
                old, m = par[f"{name}_{f}"], statistics.median(tree[f"{name}_{f}"])
                verdict = "inside" if min(old) <= m <= max(old) else ("BELOW (faster than)" if m < min(old) else "ABOVE (SLOWER than)")
                say(f"# {name}, {f.upper()}: this tree's median {m:.1f} ms is {verdict} the parent's min .. max {min(old):.1f} .. {max(old):.1f} ms")
        m16, m24, m32 = (statistics.median(tree[f"{name}_{f}"]) for f in ("s16", "s24", "f32"))
        say(f"# {name}: S24 {m24:.1f} ms " + ("lies between" if min(m16, m32) <= m24 <= max(m16, m32) else "does NOT lie between") + f" S16 {m16:.1f} and F32 {m32:.1f} ms")
    print(json.dumps({"tree": tree_runs, "parent": par_runs}))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
