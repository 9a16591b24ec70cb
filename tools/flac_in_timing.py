"""What FLAC in costs and saves, with the inputs and method of profiles/flac_timing.txt: one 600 s stereo track at 44.1 kHz,
"music" = tests/golden/gspi_stereo.wav tiled to length, "noise" = white noise at 0.5.  The streams are this project's own, FIXED-only,
written by the device encoder (byte for byte the host encoder's, tests/test_gpu_flac.py).

    python tools/flac_in_timing.py --kernel
        umx_hip_flac_decode_device on the 600 s stream at both widths: the call's six launches between two events on one stream, ms as
        median [min .. max] of 5 calls after a warm-up; whether the floats are the host decoder's; the stream's bytes against PCM; the
        host restatement's time for the same stream (a reference, not an optimised decoder: nothing is claimed from it)
    python tools/flac_in_timing.py --walls [--parent-root <built checkout of the parent commit>]
        hidden 1024, host buffers in and out, the bare C entry point umx_hip_separate_tracks_io (marshalled once, outside the timing):
        carry mode on one lane and reset mode on 14 lanes.  The plain fp32 call and the int16-in call, which the parent has too; in this
        tree also packed 24-bit in and SAMPLE_FLAC in at both widths on the same codes.  ms: median [min .. max] of 7 calls after 2
        warm-ups; four fresh processes in the order parent1, pr1, parent2, pr2 (UMX_TIMING_ROOT tells a child which tree to load)."""
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


def inputs(pkg, n):
    q = pkg.wav_load_pcm16(HERE / "tests" / "golden" / "gspi_stereo.wav")[0].astype(np.float32) / 32768.0
    return {"music": np.tile(q, (1, n // q.shape[1] + 1))[:, :n],
            "noise": (0.5 * np.random.default_rng(5).uniform(-1, 1, (2, n))).astype(np.float32)}


def med(v):
    return f"{statistics.median(v):7.2f} [{min(v):7.2f} .. {max(v):7.2f}]"


def device_stream(pkg, torch, eng, x, bits):
    """the FLAC stream of x's codes at that width, from the device encoder"""
    n = x.shape[1]
    src = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    cap = pkg.flac_bound(n, bits)
    out, got = torch.empty(cap, dtype=torch.uint8).cuda(), torch.zeros(1, dtype=torch.int64).cuda()
    eng.flac_encode_device([src.data_ptr()], n, RATE, bits, [out.data_ptr()], [cap], got.data_ptr())
    torch.cuda.synchronize()
    return out[:int(got[0])].cpu().numpy().copy()


def small_engine(pkg):
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(128, seed=3), 128)
        return pkg.Engine.from_file(path, 16 * 1024, tracks=1)


def kernel_main():
    import torch
    torch.zeros(1).cuda()
    pkg = ge.load_package()
    n = SECONDS * RATE
    eng = small_engine(pkg)
    stream = torch.cuda.current_stream().cuda_stream
    for name, x in inputs(pkg, n).items():
        for bits in (16, 24):
            data = device_stream(pkg, torch, eng, x, bits)
            info = pkg.flac_probe(data)
            t0 = time.perf_counter()
            want = pkg.flac_decode_host(data)
            host_ms = 1e3 * (time.perf_counter() - t0)
            dev = torch.from_numpy(data).cuda()
            out = torch.zeros(n, 2, dtype=torch.float32).cuda()
            status = torch.zeros(1, dtype=torch.int32).cuda()
            ms = []
            for it in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.flac_decode_device(dev.data_ptr(), data.size, info, out.data_ptr(), status.data_ptr(), hip_stream=stream)
                e1.record()
                torch.cuda.synchronize()
                if it:
                    ms.append(e0.elapsed_time(e1))
            same = int(status[0]) == 0 and np.array_equal(out.cpu().numpy().T.view(np.uint32), want.view(np.uint32))
            print(f"{name} | {bits} bits | decode {med(ms)} ms | bits equal to the host: {same} | stream {data.size} bytes ="
                  f" {data.size / (n * 2 * bits // 8):.3f} of PCM | host restatement {host_ms:.0f} ms", flush=True)
    eng.close()


def walls_child(tag):
    import torch
    torch.zeros(1).cuda()
    pkg = ge.load_package()
    n = SECONDS * RATE
    has_flac_in = hasattr(pkg, "SAMPLE_FLAC")
    audio = inputs(pkg, n)
    streams = {}
    if has_flac_in:  # the streams first, from a context that is gone before the timed ones exist (a second context in the process slows carry mode)
        enc = small_engine(pkg)
        streams = {(name, bits): device_stream(pkg, torch, enc, x, bits) for name, x in audio.items() for bits in (16, 24)}
        enc.close()
        torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as td:
        path = str(Path(td) / "m.bin.gz")
        pkg.ggml.write_model(path, pkg.ggml.synth_weights(1024, seed=7), 1024)
        engines = [("carry, 1 lane  ", pkg.Engine.from_file(path, segment_samples=pkg.SEGMENT_SAMPLES), 0),
                   ("reset, 14 lanes", pkg.Engine.from_file(path, segment_samples=pkg.SEGMENT_SAMPLES, tracks=RESET_LANES), pkg.FLAG_RESET_SEGMENTS)]
    for name, x in audio.items():
        cases = [("fp32 in", x, None), ("S16 in", pkg.pcm16_encode_host(x), pkg.sample_io(pkg.SAMPLE_S16))]
        if has_flac_in:
            cases.append(("FLAC16 in", streams[name, 16], pkg.sample_io(pkg.SAMPLE_FLAC)))
            cases.append(("S24 in", pkg.pcm24_encode_host(x), pkg.sample_io(pkg.SAMPLE_S24)))
            cases.append(("FLAC24 in", streams[name, 24], pkg.sample_io(pkg.SAMPLE_FLAC)))
        for mode, eng, flags in engines:
            for label, wave, io in cases:
                call = pkg._MeasuredCall("umx_hip_separate_tracks_io", eng.h, [wave], io, flags, [SHIFT], None, None)
                ms = []
                for it in range(9):
                    t0 = time.perf_counter()
                    rc = eng.lib.umx_hip_separate_tracks_io(*call.args)
                    dt = 1e3 * (time.perf_counter() - t0)
                    assert rc == 0, eng.last_error()
                    if it >= 2:
                        ms.append(dt)
                print(f"{tag:<7} | {name} | {mode} | {label:<10} {med(ms)} ms | {call.m.ins[0].nbytes} bytes up", flush=True)
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
