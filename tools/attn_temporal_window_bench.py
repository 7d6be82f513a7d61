"""Windowed temporal attention of a frame shard (mofa_attn_temporal_long_window_f16, ops.attn_temporal_window) beside the gathered
path (mofa_attn_temporal_long_masked_f16 at 128 key slots), on ONE GPU at the level-0 geometry of one rank: HW = 9216, C = 320
(5 heads x 64), 128 frames on 4 frame shards -> Tq = 32 query frames, one clip (a rank holds one CFG half).  No exchange is
timed: nothing here has run on more than one GPU, the wire time of either path is unmeasured.

Part 1, what a rank computes per temporal layer after its keys have arrived: the K|V projection over the key slots plus the
attention -- window path: S = anchor + 32 + 2 radius slots (a middle shard) under (radius, anchor) = (8, 1) and (31, 1); gathered
path: 128 slots, every one live.
Part 2, the kernels alone at equal (Tq, S): window and masked on the same buffers, and in the same run the local kernel beside
the dense one at T = S (the window kernel is expected to cost over the masked kernel what the local one costs over the dense
one: the same per-score test on the same body).
The candidates alternate inside every round, ROUNDS rounds of REPS launches each, events; a row gives the median over the rounds
and the spread (max - min) / median of its rounds -- a ratio inside the spread says nothing.
usage: python tools/attn_temporal_window_bench.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from mofa_video_amd import lib, ops

L = lib.load()
ROUNDS, REPS = 7, 10
HW, HEADS, HD, TQ, T_FULL = 9216, 5, 64, 32, 128
C = HEADS * HD


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e-3


def measure(rows):
    """rows: [(name, run)] -> [(name, median seconds, spread)]; the candidates alternate inside every round"""
    for _, run in rows:
        run()
    torch.cuda.synchronize()
    ts = [[] for _ in rows]
    for _ in range(ROUNDS):
        for i, (_, run) in enumerate(rows):
            ts[i].append(timed(run))
    out = []
    for (name, _), tl in zip(rows, ts):
        t = sorted(tl)[len(tl) // 2]
        out.append((name, t, (max(tl) - min(tl)) / t))
    return out


def masked(q, k, v, Tq, T, out):
    lib.check(L.mofa_attn_temporal_long_masked_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 1, Tq, T, HW, HEADS, HD,
                                                   q.stride(0), k.stride(0), out.stride(0), HD ** -0.5, None, lib.stream_ptr()),
              "mofa_attn_temporal_long_masked_f16")


def dense(q, k, v, T, out):
    lib.check(L.mofa_attn_temporal_long_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 1, T, HW, HEADS, HD, q.stride(0),
                                            k.stride(0), out.stride(0), HD ** -0.5, lib.stream_ptr()), "mofa_attn_temporal_long_f16")


g = torch.Generator(device="cuda").manual_seed(1)
hid = torch.randn(T_FULL * HW, C, device="cuda", generator=g).half()          # normed hidden tokens of up to 128 key slots
wkv = (torch.randn(2 * C, C, device="cuda", generator=g) * C ** -0.5).half()
q = torch.randn(T_FULL * HW, C, device="cuda", generator=g).half()
out = torch.empty((T_FULL * HW, C), dtype=torch.float16, device="cuda")
kv_all = ops.igemm(hid, wkv)

# ---- part 1: K|V projection + attention of one temporal layer of a middle shard (frames 32 .. 63) ----
print(f"# part 1: K|V projection + attention per temporal layer, one rank of 4 frame shards of {T_FULL} frames, HW {HW}, C {C}, Tq {TQ}")


def gathered_pair():
    kv = ops.igemm(hid, wkv)
    masked(q, kv[:, :C], kv[:, C:], TQ, T_FULL, out)


pairs = [("gathered  128 slots (masked kernel)", gathered_pair)]
for radius, anchor in ((8, 1), (31, 1)):
    S = anchor + TQ + 2 * radius

    def window_pair(S=S, radius=radius, anchor=anchor):
        kv = ops.igemm(hid[:S * HW], wkv)
        ops.attn_temporal_window(q, kv[:, :C], kv[:, C:], 1, S, HW, HEADS, head_dim=HD, out=out[:TQ * HW], Tq=TQ, local=(radius, anchor),
                                 q_frame0=TQ, band_frame0=TQ - radius)
    pairs.append((f"window ({radius:2d}, {anchor}) {S:3d} slots", window_pair))
res = measure(pairs)
t_g = res[0][1]
for name, t, spread in res:
    print(f"pair  {name:38s}: {t * 1e6:8.1f} us  spread {100 * spread:4.1f} %  / gathered {t / t_g:5.3f}", flush=True)

# ---- part 2: the kernels alone at equal (Tq, S), and local beside dense at T = S in the same run ----
print("# part 2: kernels alone; window / masked at equal (Tq, S) beside local / dense at T = S")
for Tq, S, radius, anchor in ((32, 49, 8, 1), (32, 95, 31, 1), (32, 128, 31, 1), (96, 128, 15, 2), (128, 128, 31, 0)):
    k, v = kv_all[:S * HW, :C], kv_all[:S * HW, C:]
    b0 = 40
    f0 = b0 + ((S - anchor) - Tq) // 2                                         # the queries in the middle of the band
    rows = [("masked", lambda: masked(q, k, v, Tq, S, out)),
            ("window", lambda: ops.attn_temporal_window(q, k, v, 1, S, HW, HEADS, head_dim=HD, out=out[:Tq * HW], Tq=Tq, local=(radius, anchor),
                                                        q_frame0=f0, band_frame0=b0)),
            ("dense ", lambda: dense(q, k, v, S, out)),
            ("local ", lambda: ops.attn_temporal_local(q[:S * HW], k, v, 1, S, HW, HEADS, head_dim=HD, out=out[:S * HW], local=(radius, anchor)))]
    res = {name: (t, spread) for name, t, spread in measure(rows)}
    for name in ("masked", "window", "dense ", "local "):
        t, spread = res[name]
        print(f"alone Tq {Tq:3d} S {S:3d} ({radius:2d}, {anchor}) {name}: {t * 1e6:8.1f} us  spread {100 * spread:4.1f} %", flush=True)
    print(f"alone Tq {Tq:3d} S {S:3d} ({radius:2d}, {anchor}) window / masked {res['window'][0] / res['masked'][0]:5.3f}   "
          f"local / dense (T = {S}) {res['local '][0] / res['dense '][0]:5.3f}", flush=True)
