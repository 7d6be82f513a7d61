"""The warp's backward as adapter training calls it: one 'avg' softsplat per flow (svdxt_..._norefine.py:231), 24 flows at each
feature level of a 576 x 1024 clip, gradients for the first-frame feature and the flow.  HIP (mofa_video_amd.softsplat) against
torch autograd through oracle.softsplat on the same GPU; per call: forward + backward, and the backward alone (median of
repeats, HIP events).  Bytes model of the gather kernel (mofa_softsplat_grad_f32) with dI and dF requested: grad read once,
I read, dI written = 12 C H W bytes; the whole backward adds the prologue's grad + out reads (8 C H W).
    python tools/softsplat_grad_bench.py [--reps 20]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LEVELS = [(320, 72, 128), (320, 36, 64), (640, 18, 32), (1280, 9, 16)]
NFLOWS = 24


def _time(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from mofa_video_amd import lib as L, ops
    from mofa_video_amd.softsplat import softsplat
    from oracle.softsplat import softsplat as softsplat_ref
    L.load()
    dev = "cuda"
    print(f"device: {torch.cuda.get_device_name(0)}; {NFLOWS} 'avg' warps per level, one call per flow, N = 1; times are per call (us)")
    print(f"{'level':>16} {'impl':>6} {'fwd+bwd':>9} {'bwd':>9} {'gather':>8} {'GB/s':>7}")
    for C, H, W in LEVELS:
        g = torch.Generator(device=dev).manual_seed(C + H)
        feat = torch.randn(1, C, H, W, generator=g, device=dev).half().float().requires_grad_()
        flows = [(torch.randn(1, 2, H, W, generator=g, device=dev) * 3.0).requires_grad_() for _ in range(NFLOWS)]
        gouts = [torch.randn(1, C, H, W, generator=g, device=dev) for _ in range(NFLOWS)]
        res = {}
        for name, fn in (("hip", softsplat), ("torch", softsplat_ref)):
            def fwd_bwd():
                for f, go in zip(flows, gouts):
                    torch.autograd.grad(fn(feat, f, None, "avg"), [feat, f], go)
            outs = [fn(feat, f, None, "avg") for f in flows]

            def bwd():
                for o, f, go in zip(outs, flows, gouts):
                    torch.autograd.grad(o, [feat, f], go, retain_graph=True)
            res[name] = (_time(fwd_bwd, args.reps) / NFLOWS, _time(bwd, args.reps) / NFLOWS)
        ops.TIMER = ops.LaunchTimer()
        outs = [softsplat(feat, f, None, "avg") for f in flows]
        for o, f, go in zip(outs, flows, gouts):
            torch.autograd.grad(o, [feat, f], go)
        s = ops.TIMER.summary()["softsplat_grad"]
        ops.TIMER = None
        t_gather = s["seconds"] / s["launches"] * 1e6
        gbs = 12.0 * C * H * W / (t_gather * 1e-6) / 1e9
        lvl = f"{C} @ {H}x{W}"
        print(f"{lvl:>16} {'hip':>6} {res['hip'][0]:9.1f} {res['hip'][1]:9.1f} {t_gather:8.1f} {gbs:7.0f}")
        print(f"{'':>16} {'torch':>6} {res['torch'][0]:9.1f} {res['torch'][1]:9.1f}")
        print(f"{'':>16} factor  fwd+bwd {res['torch'][0] / res['hip'][0]:.1f}x, bwd {res['torch'][1] / res['hip'][1]:.1f}x")
    print("reference points: MI355X HBM copy ~6.3 TB/s measured (8 TB/s spec)")


if __name__ == "__main__":
    main()
