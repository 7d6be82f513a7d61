"""The streaming temporal attention under any window (mofa_attn_temporal_stream_f16, ops.attn_temporal_stream) beside the kernels it
overlaps with, at level-0 geometry (HW = 9216, 5 heads x 64, 2 clips = both CFG halves) and at the 1280-channel level (HW = 576, 20
heads x 64).  One process and one set of buffers per geometry (allocated for 256 frames; a shorter clip uses their first rows):

  T = 128  dense: mofa_attn_temporal_long_f16 (``long``) and the new entry (``stream``) on the same rows;
  T = 161 / 256 under (12, 1): the ring kernel, mofa_attn_temporal_stream_local_f16 (``ring``), and the new entry;
  T = 161 / 256 dense and under (48, 1): the new entry alone -- nothing else runs these.

The launches of a geometry alternate inside every round, ROUNDS rounds of REPS launches each, device events; a row gives the
median over the rounds, the run-to-run spread (max - min) / median over its rounds, TF/s over the VISIBLE (query, key) pairs
(4 pairs head_dim flops per sequence: Q K^T and P V), and ``x128``: its time over the T = 128 dense time of the same entry kind
scaled by visible pairs (pairs / 128^2) -- 1.0 means the pairs cost what they cost at 128 frames.  Where two kernels run the same
rule a line gives stream / other; a ratio inside the two spreads says nothing.
usage: python tools/attn_temporal_stream_bench.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from mofa_video_amd import lib, ops

L = lib.load()
ROUNDS, REPS, TMAX = 7, 10, 256
GEOMS = [(2, 9216, 5, 64, "L0"), (2, 576, 20, 64, "L2 1280ch")]


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


for (B, HW, heads, hd, tag) in GEOMS:
    Cc = heads * hd
    qkv = torch.randn(B * TMAX * HW, 3 * Cc, dtype=torch.float16, device="cuda")
    out = torch.empty((B * TMAX * HW, Cc), dtype=torch.float16, device="cuda")

    def op(fn, T, **kw):
        n = B * T * HW
        return lambda: fn(qkv[:n, :Cc], qkv[:n, Cc:2 * Cc], qkv[:n, 2 * Cc:], B, T, HW, heads, head_dim=hd, out=out[:n], **kw)
    # (kernel, T, rule as printed, (radius, anchor) for the pair count, launch)
    rows = [("long  ", 128, "dense  ", (127, 0), op(ops.attn_temporal, 128)),
            ("stream", 128, "dense  ", (127, 0), op(ops.attn_temporal_stream, 128))]
    for T in (161, 256):
        rows += [("ring  ", T, "(12, 1)", (12, 1), op(ops.attn_temporal_local_stream, T, local=(12, 1))),
                 ("stream", T, "(12, 1)", (12, 1), op(ops.attn_temporal_stream, T, local=(12, 1))),
                 ("stream", T, "(48, 1)", (48, 1), op(ops.attn_temporal_stream, T, local=(48, 1))),
                 ("stream", T, "dense  ", (T - 1, 0), op(ops.attn_temporal_stream, T))]
    for row in rows:
        row[-1]()
    torch.cuda.synchronize()
    ts = [[] for _ in rows]
    for _ in range(ROUNDS):
        for i, row in enumerate(rows):
            ts[i].append(timed(row[-1]))
    med = [median(t) for t in ts]
    spread = [(max(t) - min(t)) / m for t, m in zip(ts, med)]
    base = {"long  ": med[0], "stream": med[1], "ring  ": med[0]}     # the T = 128 dense time a row is scaled against
    for i, (name, T, rule, (r, a), _) in enumerate(rows):
        pairs = ops.stream_visible_pairs(T, r, a)
        flops = 4.0 * pairs * hd * B * HW * heads
        x128 = med[i] / (base[name] * pairs / 128.0 ** 2)
        print(f"attn temporal {tag:10s} {B}x{T}x{HW} {heads}h d{hd} {name} {rule}: {med[i] * 1e6:9.1f} us  spread {100 * spread[i]:4.1f} %  "
              f"{flops / med[i] / 1e12:6.1f} TF/s visible  x128 {x128:5.2f}" + (" (of long)" if name == "ring  " else ""), flush=True)
    for i, j, what in [(1, 0, "T128 dense stream / long")] + [(3 + 4 * n, 2 + 4 * n, f"T{T} (12, 1) stream / ring") for n, T in enumerate((161, 256))]:
        print(f"# {tag} {what}: {med[i] / med[j]:5.3f} (spreads {100 * spread[i]:.1f} % / {100 * spread[j]:.1f} %)", flush=True)
    del qkv, out
