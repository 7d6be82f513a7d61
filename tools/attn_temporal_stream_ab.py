"""Two builds of libmofa_hip.so in ONE process on the same buffers: the three streaming temporal attention entry points
(mofa_attn_temporal_stream_f16, ..._stream_shard_f16, ..._stream_local_f16), whose kernels share attn_temporal_stream_body.inc.
Bits (always): torch.equal between the two builds on small shapes where a slip in the shared text shows -- HW = 3, 2 heads,
2 clips (12 sequences: the last workgroup at head_dim 64 has waves without one), head_dim 64 and 128, operands from the
generators of the case tables under tests/:
  stream  T = 1, 33, 65, 129, 161 dense and under (12, 1), (33, 0) (a visited tile hidden as a whole) and (48, 33) (two anchor tiles)
  shard   dense, (Tq, S) = (33, 161), (32, 257): every slot; the middle of a tile dead; a whole tile dead; NaN in the dead slots' rows
          window, the first and the middle shard of the layouts (256 frames over 4, (48, 1)) and (200 over 2, (33, 0))
  ring    T = 33, 97, 129, 161 under (12, 1), (32, 32), (0, 0)
Times (``--times stream shard ring``, only what is named; needed only for a kernel whose instructions differ from the parent's):
rows of profiles/attn_temporal_stream_bench.log and profiles/attn_temporal_shard_bench.log, measured as tools/attn_ab.py says.
usage: python tools/attn_temporal_stream_ab.py PARENT_LIB [NEW_LIB] [--times KERNEL ...]   (NEW_LIB defaults to the in-tree build; a
       parent build: python -m mofa_video_amd._build --variant parent in a checkout of the parent commit)"""
import ctypes as C
import os
import sys

_i = sys.argv.index("--times") if "--times" in sys.argv else len(sys.argv)
TIMES, sys.argv = sys.argv[_i + 1:], sys.argv[:_i]                      # (tools/attn_ab.py reads the two libraries off argv)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch

from attn_ab import LIBS, ab, ok, st

import attn_cases as ac
import attn_window_cases as wc

HW, HEADS, CLIPS = 3, 2, 2
NAN = float("nan")


def packed(t):
    return ac._pack_temporal(t).cuda()


def both(label, entry, q, k, v, rows, D, head, tail):
    """entry(q, k, v, out, *head, HW, HEADS, D, the leading dimensions, scale, *tail, stream) on both builds -> whether the bits differ"""
    outs = {}
    for w, l in LIBS.items():
        out = torch.full((rows, HEADS * D), NAN, dtype=torch.float16, device="cuda")
        ok(getattr(l, entry)(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), *head, HW, HEADS, D,
                             q.stride(0), k.stride(0), out.stride(0), D ** -0.5, *tail, st))
        outs[w] = out
    torch.cuda.synchronize()
    same = torch.equal(outs["parent"].view(torch.int16), outs["new"].view(torch.int16)) and bool(torch.isfinite(outs["new"]).all())
    print(f"{'equal' if same else 'DIFFERENT':9s} {label}", flush=True)
    return not same


def words_of(mask, S):
    nw = (S + 31) // 32
    return (C.c_uint32 * nw)(*[(mask >> (32 * w)) & 0xffffffff for w in range(nw)])


def bits():
    bad = n = 0
    for D in (64, 128):
        for T in (1, 33, 65, 129, 161):
            q, k, v = (packed(t) for t in ac._family_A((CLIPS, HW, HEADS), T, T, D, 100 * D + T))
            for local in (None, (12, 1), (33, 0), (48, 33)):
                r, a = (T - 1, 0) if local is None else (local[0], min(local[1], T))
                bad += both(f"stream d{D} T{T} {local or 'dense'}", "mofa_attn_temporal_stream_f16", q, k, v, CLIPS * T * HW, D,
                            (CLIPS, T), (r, a))
                n += 1
        for T in (33, 97, 129, 161):
            q, k, v = (packed(t) for t in ac._family_A((CLIPS, HW, HEADS), T, T, D, 300 * D + T))
            for (r, a) in ((12, 1), (32, 32), (0, 0)):
                bad += both(f"ring d{D} T{T} ({r}, {a})", "mofa_attn_temporal_stream_local_f16", q, k, v, CLIPS * T * HW, D,
                            (CLIPS, T), (r, a))
                n += 1
        for (Tq, S) in ((33, 161), (32, 257)):
            q, k, v = ac._family_A((CLIPS, HW, HEADS), Tq, S, D, 500 * D + S)
            full = (1 << S) - 1
            masks = {"every slot": full, "middle of a tile dead": full & ~(((1 << 9) - 1) << 43), "a whole tile dead": full & ~(((1 << 32) - 1) << 64)}
            for what, mask in list(masks.items()) + [("a whole tile dead, NaN in the dead rows", masks["a whole tile dead"])]:
                kk, vv = k.clone(), v.clone()
                if "NaN" in what:
                    dead = [j for j in range(S) if not (mask >> j) & 1]
                    kk[..., dead, :] = NAN
                    vv[..., dead, :] = NAN
                bad += both(f"shard dense d{D} Tq{Tq} S{S} {what}", "mofa_attn_temporal_stream_shard_f16", packed(q), packed(kk), packed(vv),
                            CLIPS * Tq * HW, D, (CLIPS, Tq, S), (-1, 0, 0, 0, None if mask == full else words_of(mask, S)))
                n += 1
    for (D, T, shards, r, a) in ((64, 256, 4, 48, 1), (128, 200, 2, 33, 0)):
        q, k, v = ac._family_A((CLIPS, HW, HEADS), T, T, D, 700 * D + T)
        for s in sorted({0, shards // 2}):
            g = wc.geometry(T, shards, r, a, s)
            bad += both(f"shard window d{D} T{T} over {shards} ({r}, {a}) shard {s}", "mofa_attn_temporal_stream_shard_f16",
                        packed(q[..., g.f0:g.f1, :]), packed(wc.slot_rows(k, g, a)), packed(wc.slot_rows(v, g, a)), CLIPS * g.Tq * HW, D,
                        (CLIPS, g.Tq, g.S), (r, a, g.f0, g.b0, None))
            n += 1
    print(f"# cases whose bits differ between the two builds: {bad} of {n}")
    return bad


def time_rows(kernels):
    """the rows of the two bench logs that run the named kernels"""
    slower = total = 0
    for (HW_, heads, hd, tag) in ((9216, 5, 64, "L0"), (576, 10, 128, "L2 1280ch")):
        Cc = heads * hd
        rows = []
        if "stream" in kernels:
            rows += [(f"T{T} {what}", "mofa_attn_temporal_stream_f16", T, T, (1, T), (r, a))
                     for T in (128, 161, 256) for what, r, a in (("dense", T - 1, 0), ("(12, 1)", 12, 1), ("(48, 1)", 48, 1))]
        if "ring" in kernels:
            rows += [(f"T{T} ring (12, 1)", "mofa_attn_temporal_stream_local_f16", T, T, (1, T), (12, 1)) for T in (161, 256)]
        if "shard" in kernels:
            rows += [("whole dense Tq 256 S 256", "mofa_attn_temporal_stream_shard_f16", 256, 256, (1, 256, 256), (-1, 0, 0, 0, None)),
                     ("whole (48, 1) Tq 256 S 256", "mofa_attn_temporal_stream_shard_f16", 256, 256, (1, 256, 256), (48, 1, 0, 0, None)),
                     ("shard dense Tq 64 S 256", "mofa_attn_temporal_stream_shard_f16", 64, 256, (1, 64, 256), (-1, 0, 0, 0, None)),
                     ("shard dense Tq 32 S 256", "mofa_attn_temporal_stream_shard_f16", 32, 256, (1, 32, 256), (-1, 0, 0, 0, None)),
                     ("shard (48, 1) Tq 64 S 161", "mofa_attn_temporal_stream_shard_f16", 64, 161, (1, 64, 161), (48, 1, 64, 16, None))]
        for (what, entry, Tq, S, head, tail) in rows:
            q = torch.randn(Tq * HW_, Cc, device="cuda").half()
            kv = torch.randn(S * HW_, 2 * Cc, device="cuda").half()
            k, v = kv[:, :Cc], kv[:, Cc:]
            out = torch.empty((Tq * HW_, Cc), dtype=torch.float16, device="cuda")
            slower += ab(f"{tag:10s} {heads}h d{hd} {what}",
                         lambda l: ok(getattr(l, entry)(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), *head, HW_, heads, hd,
                                                        q.stride(0), k.stride(0), out.stride(0), hd ** -0.5, *tail, st)))
            total += 1
    print(f"# rows slower than the parent by more than the parent's spread: {slower} of {total}")
    return slower


if __name__ == "__main__":
    sys.exit(1 if bits() + (time_rows(TIMES) if TIMES else 0) else 0)
