"""What the look-ahead peak limiter costs, with the inputs and method of tools/flac_in_timing.py: one 600 s stereo track at
44.1 kHz.

    python tools/limit_timing.py --kernel
        umx_hip_limit_gain_device and umx_hip_limit_apply_device alone on four outputs of 600 s (noise at 0.5 with a 4.0 spike every
        second), each between two events on one stream: ms as median [min .. max] of 9 calls after a warm-up, and the bytes a second
        of what the kernel has to move (gain: 32 B read and 4 B written a frame; apply: 4 B read a frame, plus 32 B read and written a
        limited frame).  Whether gains and report are the host call's.
    python tools/limit_timing.py --walls [--parent-root <built checkout of the parent commit>]
        hidden 1024, host buffers in and out, the bare C entry points (marshalled once, outside the timing), carry mode on one lane and
        reset mode on 14 lanes, on gspi_stereo.wav tiled to length and tripled (so that it passes full scale): the plain fp32 and int16
        calls, which the parent has too; in this tree also the fp32 call with UMX_CLIP_RESCALE and with the limiter at -1 dB.  ms: median
        [min .. max] of 7 calls after 2 warm-ups; four fresh processes in the order parent1, pr1, parent2, pr2 (UMX_TIMING_ROOT tells a
        child which tree to load)."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
ROOT = Path(os.environ.get("UMX_TIMING_ROOT") or HERE).resolve()
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

SECONDS, RATE = 600, 44100
SHIFT, RESET_LANES = 4033, 14  # a 600 s track is 14 segments: one call in reset mode
CEILING = np.float32(10 ** (-1 / 20))


def med(v):
    return f"{statistics.median(v):7.3f} [{min(v):7.3f} .. {max(v):7.3f}]"


def kernel_main():
    import torch
    torch.zeros(1).cuda()
    pkg = ge.load_package()
    n = SECONDS * RATE
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(128, seed=3), 128)
        eng = pkg.Engine.from_file(path, 16 * 1024, tracks=1)
    rng = np.random.default_rng(5)
    xs = [(0.5 * rng.uniform(-1, 1, (2, n))).astype(np.float32) for _ in range(4)]
    for b, x in enumerate(xs):
        x[b & 1, b * 1000 + RATE // 2::RATE] = 4.0
    g_ref, _, rep_ref = pkg.limit_host(xs, RATE, CEILING)
    src = [torch.from_numpy(np.ascontiguousarray(x.T)).cuda() for x in xs]
    work = [s.clone() for s in src]
    gain, rep = torch.zeros(n, dtype=torch.float32).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    times = {"gain": [], "apply": []}
    for it in range(10):
        rep.zero_()
        for w, s in zip(work, src):
            w.copy_(s)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        eng.limit_gain_device([s.data_ptr() for s in src], n, RATE, CEILING, gain.data_ptr(), rep.data_ptr(), hip_stream=stream)
        ev[1].record()
        eng.limit_apply_device([w.data_ptr() for w in work], n, gain.data_ptr(), hip_stream=stream)
        ev[2].record()
        torch.cuda.synchronize()
        if it:
            times["gain"].append(ev[0].elapsed_time(ev[1]))
            times["apply"].append(ev[1].elapsed_time(ev[2]))
    words = rep.cpu().numpy()
    same = np.array_equal(gain.cpu().numpy().view(np.uint32), g_ref.view(np.uint32)) and int(words[1]) == rep_ref[1]
    moved = {"gain": 36 * n, "apply": 4 * n + 64 * rep_ref[1]}
    for k, v in times.items():
        print(f"{k:<5} | 4 outputs x {SECONDS} s | {med(v)} ms | {moved[k] / (1e6 * statistics.median(v)):.1f} GB/s of {moved[k]} bytes", flush=True)
    print(f"limited frames {rep_ref[1]} of {n}, min gain {rep_ref[0]:.6f} | gains and count equal to the host's: {same}", flush=True)
    eng.close()


def walls_child(tag):
    import torch
    torch.zeros(1).cuda()
    pkg = ge.load_package()
    n = SECONDS * RATE
    q = pkg.wav_load_pcm16(HERE / "tests" / "golden" / "gspi_stereo.wav")[0].astype(np.float32) / 32768.0
    x = 3.0 * np.tile(q, (1, n // q.shape[1] + 1))[:, :n]
    has_limit = hasattr(pkg, "Limit")
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(1024, seed=7), 1024)
        engines = [("carry, 1 lane  ", pkg.Engine.from_file(path, segment_samples=pkg.SEGMENT_SAMPLES), 0),
                   ("reset, 14 lanes", pkg.Engine.from_file(path, segment_samples=pkg.SEGMENT_SAMPLES, tracks=RESET_LANES), pkg.FLAG_RESET_SEGMENTS)]
    top = "umx_hip_separate_tracks_limit" if has_limit else "umx_hip_separate_tracks_levels"
    cases = [("fp32", "umx_hip_separate_tracks_io", None, {}), ("int16 out", "umx_hip_separate_tracks_io", pkg.sample_io(pkg.SAMPLE_F32, pkg.SAMPLE_S16), {})]
    if has_limit:
        cases += [("fp32 rescale", top, None, {"clip": pkg.CLIP_RESCALE}), ("fp32 limit", top, None, {"ceiling": CEILING})]
    for mode, eng, flags in engines:
        for label, entry, io, more in cases:
            call = pkg._MeasuredCall(entry, eng.h, [x], io, flags, [SHIFT], None, None, **more)
            ms = []
            for it in range(9):
                t0 = time.perf_counter()
                rc = getattr(eng.lib, entry)(*call.args)
                dt = 1e3 * (time.perf_counter() - t0)
                assert rc == 0, eng.last_error()
                if it >= 2:
                    ms.append(dt)
            lr = getattr(call, "lr", None)
            note = "" if lr is None else f" | min gain {lr[0].min_gain:.4f}, {lr[0].limited_frames} frames limited"
            print(f"{tag:<7} | {mode} | {label:<12} {med(ms)} ms{note}", flush=True)
    for _, eng, _ in engines:
        eng.close()


def main():
    global SECONDS
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--walls", action="store_true")
    ap.add_argument("--seconds", type=int, default=SECONDS, help="the track's length (600: 14 segments, one call in reset mode)")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--child", default=None, help="(the fresh processes) the tag of the tree UMX_TIMING_ROOT names")
    a = ap.parse_args()
    SECONDS = a.seconds
    if a.child:
        return walls_child(a.child)
    if a.kernel:
        kernel_main()
    if a.walls:
        for tag, root in [("parent1", a.parent_root), ("pr1", None), ("parent2", a.parent_root), ("pr2", None)]:
            if tag.startswith("parent") and not root:
                continue
            env = {k: v for k, v in os.environ.items() if k not in ("UMX_HIP_LIB", "UMX_TIMING_ROOT")}
            if root:
                env["UMX_TIMING_ROOT"] = str(Path(root).resolve())
            subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", tag, "--seconds", str(SECONDS)], env=env, check=True, timeout=500)


if __name__ == "__main__":
    main()
