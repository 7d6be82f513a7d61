"""TEST INFRASTRUCTURE ONLY: the cases of the streaming temporal attention under any window, dense included (csrc/attention.hip
attn_temporal_stream_kernel, mofa_attn_temporal_stream_f16, ``ops.attn_temporal_stream(..., local=(radius, anchor) or None)``).
The rule is the local one, ``attn_local_cases.visible``:

    query frame i sees key frame j  iff  j < anchor  or  |i - j| <= radius      (1 <= T <= 1024, radius >= 0, 0 <= anchor <= T)

and the float64 reference, the bound, the operands and the geometry (HW = 5, heads 2 at head_dim 64 / 1 at 128, 1 or 2 clips) are
those of tests/attn_local_cases.py.  ``CASES`` is the list of (head_dim, T, radius, anchor) the CPU test
(tests/test_attn_stream_dense_cases_cpu.py) and the GPU test (tests/test_attn_temporal_stream_dense_gpu.py) share; radius None
(with anchor None) is the dense call, ``local=None``:

  T        past 128: 129, 159 / 160 / 161, 255 / 256 / 257, 1024 (the entry point's limit); up to 128: 1, 33, 97, 128;
  windows  dense; (T - 1, 0) and (0, T), which hide nothing either; what the ring kernel refuses -- (33, 0), (40, 0), (48, 1),
           (100, 2), (12, 33), (33, 33), (4, 128) -- those whose anchor is <= T;
  hazard   anchor 0 with radius 1, 15, 16, 31: the first band tile of a query block then hides every key from the block's last
           queries while their running maximum is still the initial value.

head_dim 64 takes every (T, window); head_dim 128 a subset.

``stand_in`` walks a sequence as the kernel does -- per 32-query block the anchor tiles and the band tiles only, ascending, with a
running maximum, a running sum and rescaled accumulators -- and takes a ``defect`` that makes the walk wrong in one of the ways
of ``MUTANTS``."""
import functools
import types

import torch

import attn_cases as ac
import attn_local_cases as lc
from attn_local_cases import BOUND, HEADS, HW, attention64, close_errors, operands, split_rows, visible  # noqa: F401

STREAM_T = (129, 159, 160, 161, 255, 256, 257, 1024)
SHORT_T = (1, 33, 97, 128)
ALL_T = SHORT_T + STREAM_T
D128_T = (33, 129, 161, 257, 1024)
HAZARD = ((1, 0), (15, 0), (16, 0), (31, 0))


def windows(T):
    """(radius, anchor) of every listed window that is valid at T; (None, None) is the dense call"""
    w = [(None, None), (T - 1, 0), (0, T), (33, 0), (40, 0), (48, 1), (100, 2), (12, 33), (33, 33), (4, 128)] + list(HAZARD)
    return [x for x in dict.fromkeys(w) if x[1] is None or x[1] <= T]


def _cases():
    cases = [(64, T, r, a) for T in ALL_T for r, a in windows(T)]
    sub = ((None, None), "all-anchor", (40, 0), (48, 1), (12, 33), (4, 128), (15, 0), (31, 0))
    for T in D128_T:
        cases += [(128, T, r, a) for r, a in dict.fromkeys((0, T) if w == "all-anchor" else w for w in sub) if a is None or a <= T]
    return tuple(cases)


CASES = _cases()


def rule(T, radius, anchor):
    """(radius, anchor) of a case as integers: dense is (T - 1, 0)"""
    return (T - 1, 0) if radius is None else (radius, anchor)


def local_of(radius, anchor):
    """the ``local=`` argument of a case"""
    return None if radius is None else (radius, anchor)


def clips_of(D, T, radius, anchor):
    return lc.clips_of(D, T, *rule(T, radius, anchor))


@functools.lru_cache(maxsize=None)
def expect64(D, T, clips, radius, anchor):
    """float64 attention under the rule, packed; one per (operands, clamped rule): the windows that hide nothing share it"""
    q, k, v = operands(D, T, clips)
    return ac._pack_temporal(attention64(q, k, v, D ** -0.5, visible(T, radius, anchor)))


def dense_data(D, T, radius, anchor):
    """-> q, k, v fp16 and expect fp64, packed as the op takes them: rows (clip, frame, pixel), columns (head, d)"""
    clips = clips_of(D, T, radius, anchor)
    q, k, v = operands(D, T, clips)
    r, a = rule(T, radius, anchor)
    r, a = (T - 1, 0) if lc.all_visible(T, r, a) else (min(r, T - 1), a)
    P = ac._pack_temporal
    return types.SimpleNamespace(clips=clips, heads=HEADS[D], HW=HW, q=P(q), k=P(k), v=P(v), expect=expect64(D, T, clips, r, a))


def visited_tiles(T, q0, radius, anchor, defect=None):
    """the key tiles the kernel visits for the 32-query block at q0, ascending, each once"""
    nA = (anchor + 31) // 32
    if defect == "anchor-tile0":
        nA = min(nA, 1)
    hi = min(q0 + 31 + radius, T - 1)
    if defect == "band-last":
        hi = min(q0 + 30 + radius, T - 1)                               # the tile whose first key is q0 + 31 + radius is lost
    band = range(max(q0 - radius, 0) // 32, hi // 32 + 1)
    return sorted(set(range(nA)) | set(band))


MUTANTS = ("stale-max", "no-rescale", "anchor-tile0", "band-last", "clamp-127")


def stand_in(q, k, v, nclips, T, HW, heads, head_dim=64, scale=None, out=None, Tq=None, key_mask=None, local=None, defect=None):
    """``ops.attn_temporal_stream`` in torch fp32 on the CPU, computed the way the kernel walks a sequence; packed rows in and out.
    defect: stale-max -- a hidden key's probability left to exp(s - m) with s = -1e30, which is 1 while the running maximum is
    still -1e30, in a walk that does not rescale a row that has met no visible key yet ("nothing accumulated": a = 1); the
    hidden keys of an all-hidden first tile then stay counted.  (With a = exp(-1e30 - m') = 0 at the first visible key the
    count would be wiped: the select is what makes the kernel independent of that.)  no-rescale -- the sum and the
    accumulators not rescaled when the maximum moves; anchor-tile0 -- anchor tiles past tile 0 not visited; band-last -- the last
    band tile dropped when q0 + 31 + radius is its first key; clamp-127 -- a key index above 127 reads key 127"""
    assert Tq is None and key_mask is None and 1 <= T <= 1024
    radius, anchor = (T - 1, 0) if local is None else local
    assert radius >= 0 and 0 <= anchor <= T
    radius = min(radius, T - 1)
    vis = visible(T, radius, anchor)
    Q, K, V = (t.float().reshape(nclips, T, HW, heads, head_dim).permute(0, 2, 3, 1, 4) for t in (q, k, v))
    factor = head_dim ** -0.5 if scale is None else scale
    res = torch.empty_like(Q)
    for q0 in range(0, T, 32):
        rows = slice(q0, min(q0 + 32, T))
        n = rows.stop - rows.start
        m = torch.full((*Q.shape[:3], n, 1), -1e30)
        l = torch.zeros_like(m)
        o = torch.zeros(*Q.shape[:3], n, head_dim)
        for kt in visited_tiles(T, q0, radius, anchor, defect):
            keys = torch.arange(32 * kt, min(32 * kt + 32, T))
            seen = vis[rows][:, keys]
            if defect == "clamp-127":
                keys = keys.clamp(max=127)
            s = (Q[..., rows, :] @ K[..., keys, :].transpose(-1, -2) * factor).masked_fill(~seen, -1e30)
            mn = torch.maximum(m, s.amax(-1, keepdim=True))
            p = torch.exp(s - mn)
            if defect != "stale-max":
                p = torch.where(seen, p, torch.zeros(()))
            a = torch.ones_like(m) if defect == "no-rescale" else torch.exp(m - mn)
            if defect == "stale-max":
                a = torch.where(m == -1e30, torch.ones(()), a)
            l = l * a + p.sum(-1, keepdim=True)
            o = o * a + p.half().float() @ V[..., keys, :]
            m = mn
        res[..., rows, :] = o / l
    res = ac._pack_temporal(res).half()
    if out is None:
        return res
    out[:] = res
    return out


def release():
    expect64.cache_clear()
    lc.release()
