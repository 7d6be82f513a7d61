"""TEST INFRASTRUCTURE ONLY: the cases of the windowed temporal attention of frame-sharded clips (csrc/attention.hip
attn_temporal_long_window_kernel, mofa_attn_temporal_long_window_f16, ``ops.attn_temporal_window``).  A rank that holds the frames
[f0, f1) of a clip of T_full frames attends, under the rule of tests/attn_local_cases.py on GLOBAL frame numbers

    query frame g sees key frame j  iff  j < anchor  or  |g - j| <= radius,

against a key buffer of S = anchor + (b1 - b0) SLOTS: the frames 0 .. anchor - 1, then the band b0 = max(f0 - radius, 0) ..
b1 = min(f1 + radius, T_full).  ``LAYOUTS`` lists (T_full, frame shards, radius, anchor); every shard of a layout is a case
(``CASES``), head dim 64 everywhere and head dim 128 on ``HD128``.  Together: S from 11 to 128 and all four key-tile counts, first
shards (their band repeats the anchor frames: those slots must count zero times), last shards (a truncated band), an anchor that
crosses a 32-slot tile edge (33), radius 0, an empty band below the anchor, clips of 250 and 256 frames.  The geometry is that of
attn_local_cases: HW = 5, heads 2 (head dim 64) / 1 (head dim 128), 1 or 2 clips.

The expectation of a case is rows f0 .. f1 of ``attn_local_cases.attention64`` on the WHOLE clip under ``visible(T_full, radius,
anchor)`` -- nothing of the slot layout enters it.  ``slot_visible`` is the rule in slot space, the table the kernel's words must
reproduce; ``MUTANTS`` are wrong slot-space rules."""
import functools
import types

import torch

import attn_cases as ac
import attn_local_cases as lc
from op_cases import TOL, close_errors  # noqa: F401  (re-exported)

LAYOUTS = ((24, 4, 4, 1), (25, 4, 6, 1), (40, 4, 8, 1), (37, 4, 9, 2), (33, 2, 0, 0), (64, 2, 16, 0), (128, 4, 31, 1), (128, 3, 16, 33),
           (130, 2, 12, 2), (256, 4, 31, 1), (250, 4, 32, 0), (96, 3, 32, 32), (66, 2, 31, 33))
HD128 = ((25, 4, 6, 1), (128, 4, 31, 1), (66, 2, 31, 33), (130, 2, 12, 2))
HW = lc.HW
HEADS = lc.HEADS
BOUND = TOL["attn_temporal"]


def bounds(T, n):
    """contiguous shards, larger ones first (parallel.split_frames, restated: the table does not import the package)"""
    base, extra = divmod(T, n)
    out, f = [], 0
    for i in range(n):
        k = base + (1 if i < extra else 0)
        out.append((f, f + k))
        f += k
    return out


def geometry(T, shards, radius, anchor, shard):
    """-> namespace f0, f1, Tq, b0, b1, L, S, own (slot of the rank's first frame)"""
    f0, f1 = bounds(T, shards)[shard]
    b0, b1 = max(f0 - radius, 0), min(f1 + radius, T)
    return types.SimpleNamespace(f0=f0, f1=f1, Tq=f1 - f0, b0=b0, b1=b1, L=b1 - b0, S=anchor + b1 - b0, own=anchor + f0 - b0)


CASES = tuple((D, T, n, r, a, s) for (T, n, r, a) in LAYOUTS for s in range(n) for D in ((64, 128) if (T, n, r, a) in HD128 else (64,)))


def slot_frames(g, anchor):
    """global frame of every slot: the anchors, then the band"""
    return list(range(anchor)) + list(range(g.b0, g.b1))


def slot_visible(g, radius, anchor):
    """THE rule in slot space -> bool [Tq, S]: slot s < anchor always; a band slot iff its frame is no anchor frame and within
    ``radius`` of the query's"""
    i = torch.arange(g.f0, g.f1)[:, None]
    f = torch.tensor(slot_frames(g, anchor))[None, :]
    s = torch.arange(g.S)[None, :]
    return (s < anchor) | ((s >= anchor) & (f >= anchor) & ((i - f).abs() <= radius))


def formula_visible(g, radius, anchor):
    """the words the kernel builds (the header's lo / hi1), as a table: ml = below(anchor) | (below(hi1) & ~below(lo))"""
    vis = torch.zeros(g.Tq, g.S, dtype=torch.bool)
    for i in range(g.Tq):
        fr = g.f0 + i
        lo = anchor + max(fr - radius, anchor, g.b0) - g.b0
        hi1 = anchor + min(fr + radius, g.b0 + g.L - 1) - g.b0 + 1
        vis[i, :anchor] = True
        if hi1 > lo:
            vis[i, lo:hi1] = True
    return vis


MUTANTS = ("duplicates", "slot-distance", "no-anchor", "strict")


def mutant_slot_visible(defect, g, radius, anchor):
    """duplicates: a band slot that repeats an anchor frame is counted too; slot-distance: the band taken on |query row - band
    slot| (the offset between the first query frame and the first band frame forgotten); no-anchor: the anchor slots ignored
    (the band alone, anchor frames inside it included); strict: ``<`` for ``<=``"""
    i = torch.arange(g.f0, g.f1)[:, None]
    f = torch.tensor(slot_frames(g, anchor))[None, :]
    s = torch.arange(g.S)[None, :]
    if defect == "duplicates":
        return (s < anchor) | ((s >= anchor) & ((i - f).abs() <= radius))
    if defect == "slot-distance":
        return (s < anchor) | ((s >= anchor) & (f >= anchor) & (((i - g.f0) - (s - anchor)).abs() <= radius))
    if defect == "no-anchor":
        return (s >= anchor) & ((i - f).abs() <= radius)
    if defect == "strict":
        return (s < anchor) | ((s >= anchor) & (f >= anchor) & ((i - f).abs() < radius))
    raise KeyError(defect)


def clips_of(D, T, n, r, a, s):
    return 1 + (T + r + a + s) % 2


@functools.lru_cache(maxsize=None)
def operands(D, T, clips):
    """q, k, v ~ N(0, 1) in fp16 for the WHOLE clip, [clips, HW, heads, T, D]; one draw per (head dim, T_full, clips)"""
    return ac._family_A((clips, HW, HEADS[D]), T, T, D, 7000 * D + 10 * T + clips)


@functools.lru_cache(maxsize=None)
def expectation(D, T, r, a, clips):
    """fp64 local attention of the whole clip [clips, HW, heads, T, D]; shared by the shards of a layout"""
    q, k, v = operands(D, T, clips)
    return lc.attention64(q, k, v, D ** -0.5, lc.visible(T, r, a))


def slot_rows(t, g, anchor):
    """[clips, HW, heads, T, D] of the whole clip -> the key buffer's slots [clips, HW, heads, S, D]"""
    return torch.cat([t[..., :anchor, :], t[..., g.b0:g.b1, :]], -2)


@functools.lru_cache(maxsize=None)
def window_data(D, T, n, r, a, s):
    """-> what ``ops.attn_temporal_window`` takes for shard s, packed (rows (clip, frame or slot, pixel), columns (head, d)), and
    expect fp64 = rows f0 .. f1 of the whole clip's local attention"""
    g = geometry(T, n, r, a, s)
    clips = clips_of(D, T, n, r, a, s)
    q, k, v = operands(D, T, clips)
    P = ac._pack_temporal
    return types.SimpleNamespace(g=g, clips=clips, heads=HEADS[D], HW=HW, q=P(q[..., g.f0:g.f1, :]), k=P(slot_rows(k, g, a)),
                                 v=P(slot_rows(v, g, a)), expect=P(expectation(D, T, r, a, clips)[..., g.f0:g.f1, :]),
                                 kw=dict(Tq=g.Tq, local=(r, a), q_frame0=g.f0, band_frame0=g.b0))


def split(t, clips, n, D):
    """packed rows -> [clips, HW, heads, n, D]"""
    return t.reshape(clips, n, HW, HEADS[D], D).permute(0, 2, 3, 1, 4)


def stand_in(q, k, v, nclips, S, HW, heads, head_dim=64, scale=None, out=None, Tq=None, local=None, q_frame0=0, band_frame0=0,
             _visible=None):
    """``ops.attn_temporal_window`` in torch fp32 on the CPU: the kernel's arithmetic in outline (fp32 scores, invisible scores
    replaced before the maximum, fp16 output), packed rows in and out.  ``_visible(g, radius, anchor)``: a mutant's table"""
    assert local is not None
    radius, anchor = local
    Tq = S if Tq is None else Tq
    L = S - anchor
    assert 0 <= anchor <= S and radius >= 0 and 0 <= band_frame0 <= q_frame0 and q_frame0 + Tq <= band_frame0 + L
    g = types.SimpleNamespace(f0=q_frame0, f1=q_frame0 + Tq, Tq=Tq, b0=band_frame0, b1=band_frame0 + L, L=L, S=S)
    vis = (_visible or slot_visible)(g, radius, anchor)
    Q = q.float().reshape(nclips, Tq, HW, heads, head_dim).permute(0, 2, 3, 1, 4)
    K, V = (t.float().reshape(nclips, S, HW, heads, head_dim).permute(0, 2, 3, 1, 4) for t in (k, v))
    lg = (Q @ K.transpose(-1, -2) * (head_dim ** -0.5 if scale is None else scale)).masked_fill(~vis, -1e30)
    res = ac._pack_temporal(torch.softmax(lg, -1) @ V).half()
    if out is None:
        return res
    out[:] = res
    return out


def release():
    operands.cache_clear()
    expectation.cache_clear()
    window_data.cache_clear()
