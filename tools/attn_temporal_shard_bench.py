"""The streaming temporal attention of a frame shard (mofa_attn_temporal_stream_shard_f16, ops.attn_temporal_stream_shard) on ONE GPU
at the level-0 geometry of one rank: HW = 9216, 5 heads x 64, one clip (a rank of the product layout holds one CFG half).  The
clip has 256 frames; a rank of 4 / 8 frame shards holds Tq = 64 / 32 of them:

  dense    S = 256 key slots (the gathered buffer, every slot live), Tq = 64 and 32;
  window   (48, 1) on a middle shard of 4: S = 1 + 64 + 2 x 48 = 161 slots.  (Over 8 shards the radius exceeds the 32-frame shard
           and ``FrameParallel.window_plan`` refuses the layout, so there is no such call to time.)

Beside each row: the whole-clip call of the same rule on the same box (``ops.attn_temporal_stream``, 256 frames, the first rows of
the same buffers) and ``share`` = Tq / T of it -- what the rank's call would cost if its queries cost what the whole clip's do;
``x share`` = the rank's time over that.  Dense, a rank reads all 256 key frames for Tq / 32 query blocks as the whole clip does
for its 8, so x share near 1 is the expectation; nothing here measures the exchange that fills the buffer.

All launches alternate inside every round, ROUNDS rounds of REPS launches each after one warm-up launch of every shape, device
events; a row gives the median over the rounds, the run-to-run spread (max - min) / median over its rounds, and TF/s over the
VISIBLE (query, slot) pairs (4 pairs head_dim flops per sequence: Q K^T and P V).  No threshold: the log is the record.
usage: python tools/attn_temporal_shard_bench.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from mofa_video_amd import lib, ops

L = lib.load()
ROUNDS, REPS, T = 7, 10, 256
HW, HEADS, HD = 9216, 5, 64
WINDOW = (48, 1)


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


Cc = HEADS * HD
qkv = torch.randn(T * HW, 3 * Cc, dtype=torch.float16, device="cuda")
out = torch.empty((T * HW, Cc), dtype=torch.float16, device="cuda")
q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]


def whole(local):
    return lambda: ops.attn_temporal_stream(q, k, v, 1, T, HW, HEADS, head_dim=HD, out=out, local=local)


def shard(S, Tq, **kw):
    return lambda: ops.attn_temporal_stream_shard(q[:Tq * HW], k[:S * HW], v[:S * HW], 1, S, HW, HEADS, head_dim=HD, out=out[:Tq * HW],
                                                  Tq=Tq, **kw)


r, a = WINDOW
Sw, f0 = a + 64 + 2 * r, 64                                           # shard 1 of 4: frames 64 .. 127, band 16 .. 175
# (name, rule as printed, Tq, S, visible pairs, launch, index of the whole-clip row it is compared with)
rows = [("whole", "dense  ", T, T, T * T, whole(None), None),
        ("whole", "(48, 1)", T, T, ops.stream_visible_pairs(T, r, a), whole(WINDOW), None),
        ("shard", "dense  ", 64, T, 64 * T, shard(T, 64), 0),
        ("shard", "dense  ", 32, T, 32 * T, shard(T, 32), 0),
        ("shard", "(48, 1)", 64, Sw, ops.window_visible_keys(Sw, 64, r, a, f0, f0 - r),
         shard(Sw, 64, local=WINDOW, q_frame0=f0, band_frame0=f0 - r), 1)]
for row in rows:
    row[5]()
torch.cuda.synchronize()
ts = [[] for _ in rows]
for _ in range(ROUNDS):
    for i, row in enumerate(rows):
        ts[i].append(timed(row[5]))
med = [median(t) for t in ts]
spread = [(max(t) - min(t)) / m for t, m in zip(ts, med)]
for i, (name, rule, Tq, S, pairs, _, ref) in enumerate(rows):
    flops = 4.0 * pairs * HD * HW * HEADS
    line = (f"attn temporal L0 1x{HW} {HEADS}h d{HD} {name} {rule} Tq {Tq:3d} S {S:3d}: {med[i] * 1e6:9.1f} us  spread {100 * spread[i]:4.1f} %  "
            f"{flops / med[i] / 1e12:6.1f} TF/s visible")
    if ref is not None:
        share = med[ref] * Tq / T
        line += (f"  | whole clip {rows[ref][1].strip()} {med[ref] * 1e6:9.1f} us (spread {100 * spread[ref]:.1f} %), share Tq/T {share * 1e6:8.1f} us, "
                 f"x share {med[i] / share:5.2f}")
    print(line, flush=True)
