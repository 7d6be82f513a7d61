"""Two builds of libmofa_hip.so in ONE process on the same buffers: the three long temporal attention entry points (dense, local
(12, 1), masked with Tq = T and every slot live, masked with Tq = T / 4 and three dead slots) at the UNet's three levels and the
ControlNet's head_dim-128 level, T = 33 ... 128.  The two libraries alternate inside every round (the order flips from round to
round), ROUNDS rounds of REPS launches each, events.  Per row: the medians, the parent's run-to-run spread (max - min) / median
over its rounds, and new / parent -- a ratio inside that spread says nothing.  A process's buffer placement moves these kernels by
1-3 %, which a comparison of two processes cannot tell from the code; this one can.
usage: python tools/attn_temporal_long_ab.py PARENT_LIB [NEW_LIB]     (NEW_LIB defaults to the in-tree build; a parent build:
       python -m mofa_video_amd._build --variant parent in a checkout of the parent commit)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from mofa_video_amd import lib

ROUNDS, REPS = 11, 10


def load(path):
    l = C.CDLL(path)
    for name, argtypes in lib.PROTOTYPES.items():
        fn = getattr(l, name)
        fn.argtypes = argtypes
        fn.restype = lib._RESTYPE.get(name, C.c_int)
    return l


LIBS = {"parent": load(sys.argv[1]), "new": load(sys.argv[2] if len(sys.argv) > 2 else lib.LIB_PATH)}
torch.zeros(1, device="cuda")
st = lib.stream_ptr()


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


def ab(label, call):
    """call(library) launches once"""
    runs = {w: (lambda l=l: call(l)) for w, l in LIBS.items()}
    for r in runs.values():
        r()
    torch.cuda.synchronize()
    ts = {"parent": [], "new": []}
    for i in range(ROUNDS):
        for w in (("parent", "new") if i % 2 == 0 else ("new", "parent")):
            ts[w].append(timed(runs[w]))
    p, n = median(ts["parent"]), median(ts["new"])
    spread = (max(ts["parent"]) - min(ts["parent"])) / p
    ratio = n / p
    flag = "" if abs(ratio - 1) <= spread else ("  SLOWER than the spread" if ratio > 1 else "  faster than the spread")
    print(f"{label:58s} parent {p * 1e6:8.1f} us  new {n * 1e6:8.1f} us  parent spread {100 * spread:4.1f} %  new / parent {ratio:5.3f}{flag}", flush=True)
    return ratio > 1 + spread


def ok(rc):
    assert rc == 0, rc


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
