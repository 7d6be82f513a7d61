"""Local temporal attention (mofa_attn_temporal_long_local_f16, ops.attn_temporal_local(..., local=(radius, anchor))) beside the dense
kernel (mofa_attn_temporal_long_f16) at the same shape: the three UNet levels (HW = 9216 / 2304 / 576 with the level's heads, 2
clips = both CFG halves) and the ControlNet's head_dim-128 level, T = 49 / 97 / 128, (radius, anchor) = (12, 1), (24, 1) -- the
window loop's context: frame 0 plus 12 / 24 neighbours on either side -- and (T - 1, 0), a rule that hides nothing.  Both kernels
stage the same bytes (q, k, v read + out written), so GB/s is on the same footing.  The kernels alternate inside every round
(dense, then the three rules), ROUNDS rounds of REPS launches each, events; a row gives the median over the rounds, the ratio
local / dense of the medians, and for the dense row the run-to-run spread (max - min) / median over its rounds -- a ratio inside
that spread says nothing.
usage: python tools/attn_temporal_local_bench.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from mofa_video_amd import lib, ops

L = lib.load()
ROUNDS, REPS = 7, 10
GEOMS = [(2, 9216, 5, 64, "L0"), (2, 2304, 10, 64, "L1"), (2, 576, 20, 64, "L2"), (2, 576, 10, 128, "CN L2 d128")]


def dense(q, k, v, B, T, HW, heads, hd, out):
    lib.check(L.mofa_attn_temporal_long_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, T, HW, heads, hd, q.stride(0),
                                            k.stride(0), out.stride(0), hd ** -0.5, lib.stream_ptr()), "mofa_attn_temporal_long_f16")


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e-3


def median(ts):
    return sorted(ts)[len(ts) // 2]


worst_spread, ratios = 0.0, []
for (B, HW, heads, hd, tag) in GEOMS:
    for T in (49, 97, 128):
        Cc = heads * hd
        qkv = torch.randn(B * T * HW, 3 * Cc, device="cuda").half()
        q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
        out = torch.empty((B * T * HW, Cc), dtype=torch.float16, device="cuda")
        rules = [(12, 1), (24, 1), (T - 1, 0)]
        runs = [lambda: dense(q, k, v, B, T, HW, heads, hd, out)] + \
               [lambda loc=loc: ops.attn_temporal_local(q, k, v, B, T, HW, heads, head_dim=hd, out=out, local=loc) for loc in rules]
        for run in runs:
            run()
        torch.cuda.synchronize()
        ts = [[] for _ in runs]
        for _ in range(ROUNDS):
            for i, run in enumerate(runs):
                ts[i].append(timed(run))
        nbytes = 4 * B * T * HW * Cc * 2
        shape = f"attn temporal {tag:10s} {B}x{T}x{HW} {heads}h d{hd}"
        td = median(ts[0])
        spread = (max(ts[0]) - min(ts[0])) / td
        worst_spread = max(worst_spread, spread)
        print(f"{shape} dense          : {td * 1e6:8.1f} us  {nbytes / td / 1e9:6.0f} GB/s  spread {100 * spread:4.1f} %", flush=True)
        for (r, a), tl in zip(rules, ts[1:]):
            t = median(tl)
            ratios.append((t / td, spread, f"{tag} T{T} ({r}, {a})"))
            print(f"{shape} local ({r:3d}, {a}): {t * 1e6:8.1f} us  {nbytes / t / 1e9:6.0f} GB/s  local / dense {t / td:5.3f}", flush=True)
        del qkv, q, k, v, out
lo, hi = min(ratios), max(ratios)
slower = [r for r in ratios if r[0] > 1.0 + r[1]]
print(f"# local / dense: {lo[0]:.3f} ({lo[2]}) .. {hi[0]:.3f} ({hi[2]}); largest dense spread {100 * worst_spread:.1f} %")
print(f"# slower than dense by more than the dense spread of its shape: {len(slower)} of {len(ratios)} rows" + (":" if slower else ""))
for x, s, what in slower:
    print(f"#   {what}: {x:.3f} (dense spread {100 * s:.1f} %)")
