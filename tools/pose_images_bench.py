"""Landmarks -> the pipelines' ``landmarks`` argument on the GPU, host path against device path: ``landmarks.pose_images`` for a
25-frame (config 3) and a 97-frame (config 5) clip at 576 x 1024, drawn at 320 x 320.
  host:   draw_landmarks + resize_linear per frame in Python / numpy, then the upload of fp32 [1,N,3,576,1024] (``.to("cuda")``);
  device: scaling + truncation of N * 68 * 2 coordinates on the host, their upload, mofa_pose_images_f32 (csrc/landmarks.hip).
Both are wall-clock times around a call that ends in a device synchronise (median of the repeats after warm-up; min .. max given);
the entry point alone is also timed between two HIP events and set against its bytes model: the output written once, 12 N H W
bytes (the int32 canvases, 4 N 320^2 bytes cleared, painted and read from cache, are about 2 % of that).  The two results are compared bit for bit.
    python tools/pose_images_bench.py [--log profiles/pose_images_bench.log] [--host-reps 3] [--reps 20]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

H, W, DRAW = 576, 1024, 320


def faces(n, seed=0):
    """a plausible face per frame, in clip pixels: one base shape, a few pixels of motion per frame"""
    rng = np.random.default_rng(seed)
    lm = rng.uniform(40, 280, (1, 68, 2)) + rng.normal(0, 3, (n, 68, 2))
    return lm * np.array([W / DRAW, H / DRAW])


def wall(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "pose_images_bench.log"))
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, nargs="+", default=[25, 97])
    args = ap.parse_args()
    from mofa_video_amd import landmarks as L, lib, ops
    assert torch.cuda.is_available(), "pose_images_bench.py measures on the GPU; there is none here"
    lib.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say(f"device: {torch.cuda.get_device_name(0)}; pose images {H} x {W} drawn at {DRAW} x {DRAW}; wall clock around a call that ends in a "
        f"device synchronise")
    say(f"host: 1 warm-up + {args.host_reps} repeats; device: 3 warm-ups + {args.reps} repeats; median (min .. max)")
    say(f"{'frames':>6} {'host draw+resize+upload':>34} {'device path':>34} {'host/device':>12} {'entry point':>12} {'GB/s':>7} {'equal':>6}")
    for n in args.frames:
        lm = faces(n)
        res = {}
        th = wall(lambda: res.__setitem__("host", L.pose_images(lm, H, W, DRAW).to("cuda")), 1, args.host_reps)
        td = wall(lambda: res.__setitem__("dev", L.pose_images(lm, H, W, DRAW, device="cuda")), 3, args.reps)
        equal = torch.equal(res["host"], res["dev"])
        pts = torch.from_numpy(np.trunc(lm / np.array([W, H]) * DRAW).astype(np.int32)).cuda()
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device="cuda")
        ws = torch.empty((n * DRAW * DRAW,), dtype=torch.int32, device="cuda")
        ev = []
        for i in range(3 + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.pose_images(pts, H, W, DRAW, out=out, workspace=ws)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ev.append(e0.elapsed_time(e1) * 1e-3)
        te = statistics.median(ev)
        say(f"{n:>6} {th[0]:>10.3f} s ({th[1]:.3f} .. {th[2]:.3f}) {'':>3} {td[0] * 1e3:>10.3f} ms ({td[1] * 1e3:.3f} .. {td[2] * 1e3:.3f}) "
            f"{th[0] / td[0]:>11.0f}x {te * 1e3:>9.3f} ms {12.0 * n * H * W / te / 1e9:>7.0f} {str(equal):>6}")
        say(f"       host per frame: {th[0] / n:.3f} s")
        if th[0] / td[0] < 10:
            say("       the gain is under 10x: see which of the upload, the synchronise or the kernels bounds the device path above")
        del res, out, ws
        torch.cuda.empty_cache()
    say("entry point = one mofa_pose_images_f32 call (canvas clear, rasterise, resize: 3 stream operations) between two HIP events;")
    say("GB/s = 12 N H W output bytes over that time (MI355X HBM copy ~6.3 TB/s measured, 8 TB/s spec)")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
