"""Tracks / landmarks -> controlnet_flow, host path against device path, around the CMP run (which is the same in both and is
timed on its own):
  Traj:     12 tracks of 4 points, T = 25, 576 x 1024, working size 384;
  Keypoint: 97 frames of 68 landmarks, 576 x 1024, working size 384.
  front = from the Python inputs to the synchronised sparse flow + mask on the device that CMP takes
          host:   tracking_points_to_drags + permute / float / repeat + upload   |  sample_inputs_face + float + upload
          device: track_points + upload + mofa_sparse_points_f32 per group       |  landmark_points + upload + mofa_sparse_points_f32
  tail  = from CMP's output [n,2,384,384] per group to controlnet_flow [1,n,2,576,1024]
          host:   get_flow's brush multiply, nearest resize, two scalings, then merge_inmask_outmask (torch launches)
          device: mofa_flow_finish_f32
Wall-clock medians around calls that end in a device synchronise; the two entry points are also timed alone between HIP events
and set against their bytes: the clear writes 16 n 384^2 bytes per group, flow_finish writes 8 n H W bytes once.  Results of
the two arms are compared bit for bit.
    python tools/control_bench.py [--log profiles/control_bench.log] [--reps 10] [--no-cmp]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

H, W, WORK = 576, 1024, 384


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


def events(fn, warmup, reps):
    ts = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(ts)


def fmt(t):
    return f"{t[0] * 1e3:9.3f} ms ({t[1] * 1e3:.3f} .. {t[2] * 1e3:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "control_bench.log"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-cmp", action="store_true", help="skip timing CMP itself")
    args = ap.parse_args()
    from mofa_video_amd import cmp as cmpmod, control, lib, ops, schema
    assert torch.cuda.is_available(), "control_bench.py measures on the GPU; there is none here"
    lib.load()
    dev = "cuda"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say(f"device: {torch.cuda.get_device_name(0)}; clip {H} x {W}, CMP working size {WORK}; wall clock around calls that end in a device "
        f"synchronise, median (min .. max); host arm 1 warm-up + {args.host_reps} repeats, device arm 3 + {args.reps}")

    # ---- Traj ------------------------------------------------------------------------------------------------------------
    T = 25
    n = T - 1
    rng = np.random.RandomState(0)
    tracks = [[(float(x), float(y)) for x, y in np.cumsum(np.concatenate([rng.uniform(100, 400, (1, 2)), rng.uniform(-40, 60, (3, 2))]), axis=0)]
              for _ in range(12)]
    brush = np.zeros((WORK, WORK), dtype=np.uint8)
    brush[:200, :150] = 255
    res = {}

    def host_front():
        d = control.tracking_points_to_drags(tracks, W, H, T, brush, work=WORK)
        out = {}
        for name in ("in", "out"):
            if d[name + "_flag"]:
                sp = d["drag_" + name].permute(0, 1, 4, 2, 3).float()
                m = d["mask_" + name].unsqueeze(2).repeat(1, 1, 2, 1, 1).float()
                out[name] = torch.cat([sp[0], m[0]], dim=1).to(dev)
        res["host_front"] = out

    def dev_front():
        start, disp, inside = control.track_points(tracks, W, H, T, brush, work=WORK)
        out = {}
        for name, sel in (("in", inside), ("out", ~inside)):
            if sel.any():
                val = torch.from_numpy(np.ascontiguousarray(disp[sel].transpose(1, 0, 2)).astype(np.float32)).to(dev)
                out[name] = ops.sparse_points(torch.from_numpy(start[sel]), val, WORK, WORK, lib.SPARSE_ADD)
        res["dev_front"] = out
    th, td = wall(host_front, 1, args.host_reps), wall(dev_front, 3, args.reps)
    groups = sorted(res["host_front"])
    equal = groups == sorted(res["dev_front"]) and all(torch.equal(res["host_front"][g], res["dev_front"][g]) for g in groups)
    say(f"Traj, 12 tracks x 4 points, T = {T} ({len(groups)} groups):")
    say(f"  front  host {fmt(th)}   device {fmt(td)}   host/device {th[0] / td[0]:8.1f}x   equal {equal}")

    g = torch.Generator().manual_seed(1)
    fin, fout = (torch.randn(n, 2, WORK, WORK, generator=g) * 5).to(dev), (torch.randn(n, 2, WORK, WORK, generator=g) * 5).to(dev)
    fin[:, :, 100:, :] = 0                                   # the in-brush flow vanishes outside the brush, as after the multiply
    bm_dev = torch.from_numpy(brush).to(dev)

    def host_tail():
        flows = []
        for flow, b in ((fin, brush), (fout, None)):
            f = flow
            if b is not None:
                f = f * (torch.as_tensor(b) / 255.).to(f.device, dtype=f.dtype).unsqueeze(0).unsqueeze(0)
            f = ops.resize_nearest_f32(f.reshape(n * 2, WORK, WORK).float().contiguous(), H, W).reshape(1, n, 2, H, W)
            f[:, :, 0] *= W / WORK
            f[:, :, 1] *= H / WORK
            flows.append(f)
        res["host_tail"] = control.merge_inmask_outmask(*flows)

    def dev_tail():
        res["dev_tail"] = ops.flow_finish(fin, fout, torch.from_numpy(brush).to(dev), H, W).unsqueeze(0)
    th2, td2 = wall(host_tail, 2, args.reps), wall(dev_tail, 3, args.reps)
    equal = torch.equal(res["host_tail"], res["dev_tail"])
    say(f"  tail   host {fmt(th2)}   device {fmt(td2)}   host/device {th2[0] / td2[0]:8.1f}x   equal {equal}")
    say(f"  both   host {(th[0] + th2[0]) * 1e3:9.3f} ms   device {(td[0] + td2[0]) * 1e3:9.3f} ms   host/device "
        f"{(th[0] + th2[0]) / (td[0] + td2[0]):8.1f}x")
    out_f = torch.empty(n, 2, H, W, device=dev)
    te = events(lambda: ops.flow_finish(fin, fout, bm_dev, H, W, out=out_f), 3, 20)
    say(f"  mofa_flow_finish_f32 alone: {te * 1e3:.3f} ms, {8.0 * n * H * W / 1e6:.0f} MB written = {8.0 * n * H * W / te / 1e9:.0f} GB/s "
        f"(reads {2 * 8.0 * n * WORK * WORK / 1e6:.0f} MB of sources, mostly from cache)")
    pos = torch.from_numpy(control.track_points(tracks, W, H, T, brush, work=WORK)[0]).to(dev)
    val = torch.zeros(n, pos.shape[0], 2, device=dev)
    out_s = torch.empty(n, 4, WORK, WORK, device=dev)
    lib_ = lib.load()

    def sparse_alone():
        lib.check(lib_.mofa_sparse_points_f32(pos.data_ptr(), val.data_ptr(), pos.shape[0], n, WORK, WORK, lib.SPARSE_ADD, out_s.data_ptr(),
                                              lib.stream_ptr()), "mofa_sparse_points_f32")
    te = events(sparse_alone, 3, 20)
    say(f"  mofa_sparse_points_f32 alone (12 points, n = {n}): {te * 1e3:.3f} ms, {16.0 * n * WORK * WORK / 1e6:.0f} MB cleared = "
        f"{16.0 * n * WORK * WORK / te / 1e9:.0f} GB/s")
    del res["host_tail"], res["dev_tail"], out_f, fin, fout
    torch.cuda.empty_cache()

    # ---- Keypoint --------------------------------------------------------------------------------------------------------
    N = 97
    g = torch.Generator().manual_seed(2)
    first = torch.rand(3, H, W, generator=g)
    lm = torch.rand(1, 68, 2, generator=g) * torch.tensor([W * 0.6, H * 0.6]) + torch.tensor([W * 0.2, H * 0.2]) + torch.randn(N, 68, 2, generator=g) * 6

    def host_front_kp():
        _, _, _, _, sp, m = control.sample_inputs_face(first, lm)
        res["host_kp"] = torch.cat([sp[0].float(), m[0].float()], dim=1).to(dev)

    def dev_front_kp():
        lw = torch.zeros(1, N, 68, 2)
        lw[0, :, :, 0] = lm[:, :, 0] / W * WORK
        lw[0, :, :, 1] = lm[:, :, 1] / H * WORK
        p, v = control.landmark_points(lw)
        res["dev_kp"] = ops.sparse_points(p, v.to(dev), WORK, WORK, lib.SPARSE_LAST)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                 # index_put_ is last-writer-wins only when it runs serially
    th = wall(host_front_kp, 1, args.host_reps)
    torch.set_num_threads(threads)
    td = wall(dev_front_kp, 3, args.reps)
    equal = torch.equal(res["host_kp"], res["dev_kp"])
    say(f"Keypoint, {N} frames of 68 landmarks (host: sample_inputs_face, which also builds the unused {H} x {W} pair, on one thread):")
    say(f"  front  host {fmt(th)}   device {fmt(td)}   host/device {th[0] / td[0]:8.1f}x   equal {equal}")
    flow = (torch.randn(N - 1, 2, WORK, WORK, generator=g) * 5).to(dev)

    def host_tail_kp():
        f = ops.resize_nearest_f32(flow.reshape((N - 1) * 2, WORK, WORK).contiguous(), H, W).reshape(1, N - 1, 2, H, W)
        f[:, :, 0] *= W / WORK
        f[:, :, 1] *= H / WORK
        res["host_tail"] = f

    def dev_tail_kp():
        res["dev_tail"] = ops.flow_finish(None, flow, None, H, W).unsqueeze(0)
    th2, td2 = wall(host_tail_kp, 2, args.reps), wall(dev_tail_kp, 3, args.reps)
    equal = torch.equal(res["host_tail"], res["dev_tail"])
    say(f"  tail   host {fmt(th2)}   device {fmt(td2)}   host/device {th2[0] / td2[0]:8.1f}x   equal {equal}")
    say(f"  both   host {(th[0] + th2[0]) * 1e3:9.3f} ms   device {(td[0] + td2[0]) * 1e3:9.3f} ms   host/device "
        f"{(th[0] + th2[0]) / (td[0] + td2[0]):8.1f}x")
    out_f = torch.empty(N - 1, 2, H, W, device=dev)
    te = events(lambda: ops.flow_finish(None, flow, None, H, W, out=out_f), 3, 20)
    say(f"  mofa_flow_finish_f32 alone: {te * 1e3:.3f} ms, {8.0 * (N - 1) * H * W / 1e6:.0f} MB written = "
        f"{8.0 * (N - 1) * H * W / te / 1e9:.0f} GB/s")
    res.clear()
    del out_f, flow
    torch.cuda.empty_cache()

    # ---- CMP itself (identical in both arms) -------------------------------------------------------------------------------
    if not args.no_cmp:
        model = cmpmod.CMP_demo(schema.synthetic_state_dict(schema.cmp_schema(), seed=21, gain=2.0), dev)
        for frames in (n, N - 1):
            img = torch.rand(frames, 3, WORK, WORK, device=dev)
            sp = torch.zeros(frames, 4, WORK, WORK, device=dev)
            sp[:, :, 100, 100] = 1.0
            t = wall(lambda: model.run(img, sp[:, :2], sp[:, 2:]), 1, 3)
            say(f"CMP_demo.run, {frames} frames at {WORK} x {WORK} (random weights; per group): {fmt(t)}")
            del img, sp
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
