"""The warp's backward as adapter training calls it: one 'avg' softsplat per flow (svdxt_..._norefine.py:231), 24 flows at each
feature level of a 576 x 1024 clip, gradients for the first-frame feature and the flow.  HIP (mofa_video_amd.softsplat) against
torch autograd through oracle.softsplat on the same GPU; per call: forward + backward, and the backward alone (median of
repeats, HIP events).  Bytes model of the gather kernel (mofa_softsplat_grad_f32) with dI and dF requested: grad read once,
I read, dI written = 12 C H W bytes; the whole backward adds the prologue's grad + out reads (8 C H W).
    python tools/softsplat_grad_bench.py [--reps 20]
--gather: today's path against the fp32 gather forward (mofa_video_amd.softsplat.GATHER_F32) on fp32 features, the two alternating
repeat by repeat in one process: forward, backward, forward + backward per call, and the mofa_softsplat_gather_f32 entry point (CSR
build + gather) against its bytes model, 8 C H W for the feature read and the output written + the flow + 4 H W CSR entries.
    python tools/softsplat_grad_bench.py --gather [--reps 20]"""
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


def _time_alternating(fns, reps, warmup=3):
    """medians of `reps` timings of each function, one of each per round (so drift and neighbours hit both alike)"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
    return [statistics.median(t) for t in ts]


def gather_rows(reps):
    from mofa_video_amd import lib as L, ops
    from mofa_video_amd import softsplat as S
    L.load()
    dev = "cuda"
    print(f"device: {torch.cuda.get_device_name(0)}; {NFLOWS} 'avg' warps per level on fp32 features, one call per flow, N = 1; per call "
          f"(us), medians of {reps}, the two paths alternating")
    print(f"{'level':>16} {'path':>8} {'fwd':>9} {'bwd':>9} {'fwd+bwd':>9} {'entry':>8} {'GB/s':>7}")
    for C, H, W in LEVELS:
        g = torch.Generator(device=dev).manual_seed(C + H)
        feat = torch.randn(1, C, H, W, generator=g, device=dev).requires_grad_()
        flows = [(torch.randn(1, 2, H, W, generator=g, device=dev) * 3.0).requires_grad_() for _ in range(NFLOWS)]
        gouts = [torch.randn(1, C, H, W, generator=g, device=dev) for _ in range(NFLOWS)]

        def with_switch(on, fn):
            def run():
                S.GATHER_F32 = on
                try:
                    fn()
                finally:
                    S.GATHER_F32 = False
            return run

        def fwd():
            with torch.no_grad():
                for f in flows:
                    S.softsplat(feat, f, None, "avg")

        def fwd_bwd():
            for f, go in zip(flows, gouts):
                torch.autograd.grad(S.softsplat(feat, f, None, "avg"), [feat, f], go)
        outs = {}
        for on in (False, True):
            with_switch(on, lambda: outs.__setitem__(on, [S.softsplat(feat, f, None, "avg") for f in flows]))()

        def bwd_of(on):
            def bwd():
                for o, f, go in zip(outs[on], flows, gouts):
                    torch.autograd.grad(o, [feat, f], go, retain_graph=True)
            return bwd
        t_f = _time_alternating([with_switch(False, fwd), with_switch(True, fwd)], reps)
        t_b = _time_alternating([bwd_of(False), bwd_of(True)], reps)
        t_fb = _time_alternating([with_switch(False, fwd_bwd), with_switch(True, fwd_bwd)], reps)
        ops.TIMER = ops.LaunchTimer()
        with_switch(True, fwd)()
        s = ops.TIMER.summary()["softsplat_gather_f32"]
        ops.TIMER = None
        t_entry = s["seconds"] / s["launches"] * 1e6
        gbs = H * W * (8.0 * C + 8.0 + 32.0) / (t_entry * 1e-6) / 1e9
        lvl = f"{C} @ {H}x{W}"
        print(f"{lvl:>16} {'today':>8} {t_f[0] / NFLOWS:9.1f} {t_b[0] / NFLOWS:9.1f} {t_fb[0] / NFLOWS:9.1f}")
        print(f"{'':>16} {'gather':>8} {t_f[1] / NFLOWS:9.1f} {t_b[1] / NFLOWS:9.1f} {t_fb[1] / NFLOWS:9.1f} {t_entry:8.1f} {gbs:7.0f}")
        print(f"{'':>16} today / gather: fwd {t_f[0] / t_f[1]:.2f}x, bwd {t_b[0] / t_b[1]:.2f}x, fwd+bwd {t_fb[0] / t_fb[1]:.2f}x")
    print("entry = one mofa_softsplat_gather_f32 call (memset, count, scan, fill, sort, gather: 6 launches) between two events")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gather", action="store_true", help="today's path against the fp32 gather forward, alternating")
    args = ap.parse_args()
    if args.gather:
        return gather_rows(args.reps)
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
