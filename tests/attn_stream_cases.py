"""TEST INFRASTRUCTURE ONLY: the cases of the streaming local temporal attention (csrc/attention.hip
attn_temporal_stream_local_kernel, mofa_attn_temporal_stream_local_f16, ``ops.attn_temporal_local_stream(..., local=(radius,
anchor))``).  The rule is the local one, ``attn_local_cases.visible``:

    query frame i sees key frame j  iff  j < anchor  or  |i - j| <= radius      (1 <= T <= 1024, radius <= 32, anchor <= min(T, 32))

and the float64 reference, the bound, the operands and the geometry (HW = 5, heads 2 at head_dim 64 / 1 at 128, 1 or 2 clips) are
those of tests/attn_local_cases.py.  ``CASES`` is the list of (head_dim, T, radius, anchor) the CPU test
(tests/test_attn_stream_cases_cpu.py) and the GPU test (tests/test_attn_temporal_stream_gpu.py) share:

  T       past 128: 129 (one frame into the fifth tile), 159 / 160 / 161 and 192 / 193 (a tile edge from both sides), 255 / 256 /
          257, 1024 (the entry point's limit: 32 query blocks, the ring turned ten times); up to 128, where the kernel must give
          the local kernel's bits: 1, 31 / 32 / 33, 64 / 65, 96 / 97, 127 / 128;
  radius  0, 1, 15 / 16, 31 / 32 (the limit: a band that ends one past a tile edge seen from a tile's first query);
  anchor  0, 1, 2, 31 / 32 (the limit), those that are <= T.

Per T at head_dim 64 every radius appears, with a rotating anchor, so that every anchor appears too; head_dim 128 takes a subset.

``MUTANTS`` are wrong ways to run the ring.  Several of them count a key twice or read one key in place of another, which no
bool table expresses, so a mutant is a table of MULTIPLICITIES: weights[i, j] = how many times query i counts key j (the rule
itself: 0 or 1).  Two tables mean the same attention iff their rows are proportional."""
import torch

import attn_cases as ac
import attn_local_cases as lc
from attn_local_cases import BOUND, HEADS, HW, attention64, clips_of, close_errors, local_data, operands, split_rows, visible  # noqa: F401

STREAM_T = (129, 159, 160, 161, 192, 193, 255, 256, 257, 1024)
SHORT_T = (1, 31, 32, 33, 64, 65, 96, 97, 127, 128)
ALL_T = SHORT_T + STREAM_T
RADII = (0, 1, 15, 16, 31, 32)
ANCHORS = (0, 1, 2, 31, 32)
D128_T = (1, 33, 129, 161, 257, 1024)


def anchors(T):
    return [a for a in ANCHORS if a <= T]


def _cases():
    cases = []
    for ti, T in enumerate(ALL_T):
        A = anchors(T)
        cases += [(64, T, r, A[(ri + ti) % len(A)]) for ri, r in enumerate(RADII)]        # six consecutive indices: every anchor
    for ti, T in enumerate(D128_T):
        A = anchors(T)
        pairs = [(0, A[ti % len(A)]), (16, A[(ti + 1) % len(A)]), (32, A[(ti + 2) % len(A)]), (1, A[-1])]
        cases += [(128, T, r, a) for r, a in dict.fromkeys(pairs)]
    return tuple(cases)


CASES = _cases()

MUTANTS = ("ring-stale", "anchor-twice", "anchor-first-blocks", "two-tile-band", "clamp-128")


def mutant_weights(defect, T, radius, anchor):
    """-> int64 [T (query i), T (key j)]: how often query i counts key j.
    ring-stale: the slot of band tile tq + 1 still holds tile tq - 2 -- the band keys of tile tq + 1 are read 96 frames back (not
    at all where tile tq - 2 does not exist); anchor-twice: the band copy of tile 0 is not hidden for the anchors, which the
    queries of blocks 0 and 1 then count twice; anchor-first-blocks: the anchors are visible to queries < 96 only (tile 0 left to
    the ring); two-tile-band: band tile tq + 1 dropped; clamp-128: a key index above 127 reads key 127"""
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    anch, band = (j < anchor) & (i >= 0), ((i - j).abs() <= radius) & (j >= anchor)      # disjoint, their union is the rule
    ahead = band & (j // 32 == i // 32 + 1)                                              # the band's keys in tile tq + 1
    if defect == "ring-stale":
        w = (anch | (band & ~ahead)).long()
        qi, kj = torch.nonzero(ahead & (j >= 96), as_tuple=True)
        w.index_put_((qi, kj - 96), torch.ones_like(qi), accumulate=True)
        return w
    if defect == "anchor-twice":
        return anch.long() * (1 + (i < 64).long()) + band.long()
    if defect == "anchor-first-blocks":
        return ((anch & (i < 96)) | ((i - j).abs() <= radius)).long()
    if defect == "two-tile-band":
        return (anch | (band & ~ahead)).long()
    if defect == "clamp-128":
        w = (anch | band).long()
        if T > 128:
            w[:, 127] += w[:, 128:].sum(1)
            w[:, 128:] = 0
        return w
    raise KeyError(defect)


def same_attention(w, T, radius, anchor):
    """do the multiplicities ``w`` mean the rule's attention: no empty row, every row proportional to the rule's row"""
    vis = visible(T, radius, anchor).long()
    return bool((w.sum(1) > 0).all()) and torch.equal(w * vis.sum(1, keepdim=True), vis * w.sum(1, keepdim=True))


def attention64_weighted(q, k, v, factor, w):
    """``attention64`` with key j counted w[i, j] times by query i (w > 0 somewhere in every row)"""
    lg = q.double() @ k.double().transpose(-1, -2) * factor + w.double().log()
    return torch.softmax(lg, -1) @ v.double()


def stand_in(q, k, v, nclips, T, HW, heads, head_dim=64, scale=None, out=None, Tq=None, key_mask=None, local=None):
    """``ops.attn_temporal_local_stream(..., local=(radius, anchor))`` in torch fp32 on the CPU, computed the way the kernel walks a
    sequence: per 32-query block the score tiles [tile 0, tq - 1, tq, tq + 1] only, a band tile that is out of range or tile 0
    hidden as a whole (-1e30 before the maximum), fp16 output; packed rows in and out"""
    assert local is not None and Tq is None and key_mask is None
    radius, anchor = local
    assert 1 <= T <= 1024 and 0 <= radius <= 32 and 0 <= anchor <= min(T, 32)
    vis = visible(T, radius, anchor)
    Q, K, V = (t.float().reshape(nclips, T, HW, heads, head_dim).permute(0, 2, 3, 1, 4) for t in (q, k, v))
    factor = head_dim ** -0.5 if scale is None else scale
    ntiles, res = (T + 31) // 32, torch.empty_like(Q)
    for tq in range(ntiles):
        rows = slice(32 * tq, min(32 * tq + 32, T))
        tiles = [0] + [t for t in (tq - 1, tq, tq + 1) if 0 < t < ntiles]
        keys = torch.cat([torch.arange(32 * t, min(32 * t + 32, T)) for t in tiles])
        lg = (Q[..., rows, :] @ K[..., keys, :].transpose(-1, -2) * factor).masked_fill(~vis[rows][:, keys], -1e30)
        res[..., rows, :] = torch.softmax(lg, -1) @ V[..., keys, :]
    res = ac._pack_temporal(res).half()
    if out is None:
        return res
    out[:] = res
    return out


def release():
    lc.release()
