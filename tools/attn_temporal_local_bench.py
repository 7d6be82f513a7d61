"""Local temporal attention (mofa_attn_temporal_long_local_f16, ops.attn_temporal_local(..., local=(radius, anchor))) beside the dense
kernel (mofa_attn_temporal_long_f16) at the same shape: the three UNet levels (HW = 9216 / 2304 / 576 with the level's heads, 2
clips = both CFG halves) and the ControlNet's head_dim-128 level, T = 49 / 97 / 128, (radius, anchor) = (12, 1), (24, 1) -- the
window loop's context: frame 0 plus 12 / 24 neighbours on either side -- and (T - 1, 0), a rule that hides nothing.  Both kernels
stage the same bytes (q, k, v read + out written), so GB/s is on the same footing.  The kernels alternate inside every round
(dense, then the three rules), ROUNDS rounds of REPS launches each, events; a row gives the median over the rounds, the ratio
local / dense of the medians, and for the dense row the run-to-run spread (max - min) / median over its rounds -- a ratio inside
that spread says nothing.
A second part times the streaming entry (mofa_attn_temporal_stream_local_f16, ops.attn_temporal_local_stream) on the same four
shapes, in one process and on one set of buffers (allocated for 256 frames; a shorter clip uses their first rows): the local kernel
at T = 128 under (12, 1) and (32, 1), the streaming entry at T = 128 on the same rows, and the streaming entry at T = 160 and 256.
A row gives microseconds per launch, microseconds per frame and GB/s against the same 8 T HW C bytes per clip; the T = 128 rows
also the ratio stream / local with the local row's spread.
usage: python tools/attn_temporal_local_bench.py [--stream-only]"""
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
for (B, HW, heads, hd, tag) in ([] if "--stream-only" in sys.argv else GEOMS):
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
if not ratios:
    ratios = [(1.0, 0.0, "skipped")]
lo, hi = min(ratios), max(ratios)
slower = [r for r in ratios if r[0] > 1.0 + r[1]]
print(f"# local / dense: {lo[0]:.3f} ({lo[2]}) .. {hi[0]:.3f} ({hi[2]}); largest dense spread {100 * worst_spread:.1f} %")
print(f"# slower than dense by more than the dense spread of its shape: {len(slower)} of {len(ratios)} rows" + (":" if slower else ""))
for x, s, what in slower:
    print(f"#   {what}: {x:.3f} (dense spread {100 * s:.1f} %)")

# ---- the streaming entry: T = 128 beside the local kernel, then T = 160 and 256 ----
TMAX = 256
for (B, HW, heads, hd, tag) in GEOMS:
    Cc = heads * hd
    qkv = torch.randn(B * TMAX * HW, 3 * Cc, dtype=torch.float16, device="cuda")
    out = torch.empty((B * TMAX * HW, Cc), dtype=torch.float16, device="cuda")
    for loc in ((12, 1), (32, 1)):
        def op(fn, T):
            n = B * T * HW
            return lambda: fn(qkv[:n, :Cc], qkv[:n, Cc:2 * Cc], qkv[:n, 2 * Cc:], B, T, HW, heads, head_dim=hd, out=out[:n], local=loc)
        rows = [("local ", 128, op(ops.attn_temporal_local, 128))] + [("stream", T, op(ops.attn_temporal_local_stream, T)) for T in (128, 160, 256)]
        for _, _, run in rows:
            run()
        torch.cuda.synchronize()
        ts = [[] for _ in rows]
        for _ in range(ROUNDS):
            for i, (_, _, run) in enumerate(rows):
                ts[i].append(timed(run))
        t_local = median(ts[0])
        for (name, T, _), tl in zip(rows, ts):
            t, nbytes = median(tl), 4 * B * T * HW * Cc * 2
            note = f"  spread {100 * (max(tl) - min(tl)) / t:4.1f} %" if name == "local " else \
                f"  stream / local {t / t_local:5.3f}" if T == 128 else ""
            print(f"attn temporal {tag:10s} {B}x{T}x{HW} {heads}h d{hd} {name} ({loc[0]:2d}, {loc[1]}): {t * 1e6:8.1f} us  "
                  f"{t * 1e6 / T:7.2f} us/frame  {nbytes / t / 1e9:6.0f} GB/s{note}", flush=True)
    del qkv, out
