"""Two builds of libmofa_hip.so in ONE process on the same buffers: the three long temporal attention entry points (dense, local
(12, 1), masked with Tq = T and every slot live, masked with Tq = T / 4 and three dead slots) at the UNet's three levels and the
ControlNet's head_dim-128 level, T = 33 ... 128.  The loader, the alternating rounds and what a row prints: tools/attn_ab.py.
usage: python tools/attn_temporal_long_ab.py PARENT_LIB [NEW_LIB]     (NEW_LIB defaults to the in-tree build; a parent build:
       python -m mofa_video_amd._build --variant parent in a checkout of the parent commit)"""
import ctypes as C

import torch

from attn_ab import ab, ok, st


GEOMS = [(2, 9216, 5, 64, "L0"), (2, 2304, 10, 64, "L1"), (2, 576, 20, 64, "L2"), (2, 576, 10, 128, "CN L2 d128")]
slower = total = 0
for (B, HW, heads, hd, tag) in GEOMS:
    for T in (33, 49, 64, 97, 128):
        Cc = heads * hd
        qkv = torch.randn(B * T * HW, 3 * Cc, device="cuda").half()
        q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
        out = torch.empty((B * T * HW, Cc), dtype=torch.float16, device="cuda")
        a = (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr())
        ld = (q.stride(0), k.stride(0), out.stride(0), hd ** -0.5)
        shape = f"{tag:10s} {B}x{T}x{HW} {heads}h d{hd}"
        slower += ab(f"{shape} dense", lambda l: ok(l.mofa_attn_temporal_long_f16(*a, B, T, HW, heads, hd, *ld, st)))
        slower += ab(f"{shape} local (12, 1)", lambda l: ok(l.mofa_attn_temporal_long_local_f16(*a, B, T, HW, heads, hd, *ld, 12, 1, st)))
        total += 2
        # masked: one clip, the first Tq frames of q as the queries
        for Tq, dead, what in ((T, (), "full"), (T // 4, (T // 4 - 1, T // 2 - 1, T - 1), "padded")):
            mask = ((1 << T) - 1) & ~sum(1 << j for j in dead)
            words = (C.c_uint32 * 4)(*[(mask >> (32 * w)) & 0xffffffff for w in range(4)])
            slower += ab(f"{shape} masked 1x{Tq}/{T} {what}",
                         lambda l: ok(l.mofa_attn_temporal_long_masked_f16(*a, 1, Tq, T, HW, heads, hd, *ld, words, st)))
            total += 1
        del qkv, q, k, v, out
print(f"# rows slower than the parent by more than the parent's spread: {slower} of {total}")
