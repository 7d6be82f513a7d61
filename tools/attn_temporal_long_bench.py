"""GB/s of the temporal attention kernels (q, k, v read + out written) around and beyond the 32-frame limit of the shipped
kernel: T = 25 / 32 through mofa_attn_temporal_f16, T = 33 ... 128 through mofa_attn_temporal_long_f16 (what ops.attn_temporal
dispatches to), and the long entry point called directly at T = 32 for a like-for-like figure; then the masked entry of
frame-sharded clips, mofa_attn_temporal_long_masked_f16 through ops.attn_temporal_sharded, at 64 and 128 key slots: every slot
live with Tq = T (the self-attention rows of the same run say what the mask costs), Tq = T / 2 and T / 4, and one rank's call of
a padded layout (4 uneven frame shards: Tq = T / 4 queries, T - 3 live slots).  Bytes = the rows the kernel touches: q read and
out written for Tq frames, k and v read for the live slots.  Events, median of 3 x 5 launches.
usage: python tools/attn_temporal_long_bench.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from mofa_video_amd import lib, ops

L = lib.load()


def long_direct(q, k, v, B, T, HW, heads, hd):
    out = torch.empty((B * T * HW, heads * hd), dtype=torch.float16, device=q.device)
    lib.check(L.mofa_attn_temporal_long_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, T, HW, heads, hd, q.stride(0),
                                            k.stride(0), out.stride(0), hd ** -0.5, lib.stream_ptr()), "mofa_attn_temporal_long_f16")
    return out


def median_time(run):
    run(); torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5): run()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 5 * 1e-3)
    return sorted(ts)[1]


GEOMS = [(2, 9216, 5, 64, "L0"), (2, 576, 10, 128, "CN L2 d128")]
for (B, HW, heads, hd, tag) in GEOMS:
    for T, direct in [(25, False), (32, False), (32, True), (33, False), (48, False), (64, False), (96, False), (128, False)]:
        Cc = heads * hd
        qkv = torch.randn(B * T * HW, 3 * Cc, device="cuda").half()
        q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
        run = (lambda: long_direct(q, k, v, B, T, HW, heads, hd)) if direct else \
              (lambda: ops.attn_temporal(q, k, v, B, T, HW, heads, head_dim=hd))
        t = median_time(run)
        kern = "long" if direct or T > 32 else "shipped"
        print(f"attn temporal {tag:12s} {B}x{T}x{HW} {heads}h d{hd} {kern:8s}: {t*1e6:8.1f} us  {4 * B * T * HW * Cc * 2 / t / 1e9:7.0f} GB/s "
              "(q, k, v read + out written)", flush=True)
        del qkv, q, k, v

# the masked entry: one CFG half per rank (1 clip), Tq query frames against T key slots
for (_, HW, heads, hd, tag) in GEOMS:
    for T in (64, 128):
        Cc = heads * hd
        kv = torch.randn(T * HW, 2 * Cc, device="cuda").half()
        k, v = kv[:, :Cc], kv[:, Cc:]
        padded = sum(((1 << (T // 4 - (s > 0))) - 1) << (s * (T // 4)) for s in range(4))      # shards of T/4, T/4-1, T/4-1, T/4-1 frames
        for Tq, mask, what in [(T, None, "full"), (T // 2, None, "full"), (T // 4, None, "full"), (T // 4, padded, "padded")]:
            q = torch.randn(Tq * HW, Cc, device="cuda").half()
            live = T if mask is None else bin(mask).count("1")
            t = median_time(lambda: ops.attn_temporal_sharded(q, k, v, 1, T, HW, heads, head_dim=hd, Tq=Tq, key_mask=mask))
            print(f"attn temporal {tag:12s} 1x{Tq}/{T}x{HW} {heads}h d{hd} masked {what:6s} ({live:3d} live): {t*1e6:8.1f} us  "
                  f"{2 * (Tq + live) * HW * Cc * 2 / t / 1e9:7.0f} GB/s (q, live k, v read + out written)", flush=True)
            del q
        del kv, k, v
