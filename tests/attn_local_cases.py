"""TEST INFRASTRUCTURE ONLY: the cases of the local temporal attention (csrc/attention.hip attn_temporal_long_local_kernel,
mofa_attn_temporal_long_local_f16, ``ops.attn_temporal_local(..., local=(radius, anchor))``).  ONE rule, the one the header states:

    query frame i sees key frame j  iff  j < anchor  or  |i - j| <= radius          (1 <= T <= 128, radius >= 0, 0 <= anchor <= T)

``visible`` is that rule as a [T, T] table, ``attention64`` the float64 masked softmax built from it, ``CASES`` the list of
(head_dim, T, radius, anchor) that the CPU test (tests/test_attn_local_cases_cpu.py) and the GPU test
(tests/test_attn_temporal_local_gpu.py) share:

  T       every length at which the kernel changes its number of key tiles or query blocks, and both ends: 1, 2, 31 / 32 / 33,
          63 / 64 / 65, 96 / 97, 127 / 128;
  radius  0, 1, 15 / 16, 31 / 32 (a band that ends at, or one past, a 32-key tile edge seen from a tile's first query),
          T - 2 (the largest band that still hides a key), T - 1 and 127 (all visible; 127 > T - 1 is accepted);
  anchor  0, 1, 2, 33 (one key into the second tile), T (all visible);

only the valid combinations (radius >= 0, anchor <= T).  Per T every radius appears with a rotating anchor and every anchor with
a rotating radius, head_dim 64; head_dim 128 takes a subset.  The geometry is tiny: HW = 5, heads 2 (head_dim 64) / 1 (head_dim
128), 1 or 2 clips -- 5, 10 or 20 sequences per launch, which leaves the last workgroup partly empty at 4 waves per workgroup (10
sequences) and at 2 (head_dim 128: 5 sequences).

``MUTANTS`` are wrong rules; each differs from the true table on at least one listed case (the CPU test asserts it)."""
import functools
import types

import torch

import attn_cases as ac
from op_cases import TOL, close_errors  # noqa: F401  (re-exported for the two test files)

LOCAL_T = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128)
HW = 5
HEADS = {64: 2, 128: 1}
BOUND = TOL["attn_temporal"]             # the bound tests/test_attn_temporal_long_gpu.py applies to the dense kernel against fp64


def radii(T):
    return sorted({r for r in (0, 1, 15, 16, 31, 32, T - 2, T - 1, 127) if r >= 0})


def anchors(T):
    return sorted({a for a in (0, 1, 2, 33, T) if 0 <= a <= T})


def _cases():
    cases = []
    for ti, T in enumerate(LOCAL_T):
        R, A = radii(T), anchors(T)
        pairs = [(r, A[(ri + ti) % len(A)]) for ri, r in enumerate(R)] + [(R[(ai + ti) % len(R)], a) for ai, a in enumerate(A)]
        cases += [(64, T, r, a) for r, a in dict.fromkeys(pairs)]
    for T in (1, 33, 65, 128):
        pairs = [(0, 0), (1, 1), (16, 2), (31, 33), (32, 1), (T - 2, 0), (T - 1, 0), (127, T), (0, T)]
        cases += [(128, T, r, a) for r, a in dict.fromkeys(pairs) if r >= 0 and a <= T]
    return tuple(cases)


CASES = _cases()


def visible(T, radius, anchor):
    """THE rule -> bool [T (query i), T (key j)]"""
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    return (j < anchor) | ((i - j).abs() <= radius)


def all_visible(T, radius, anchor):
    return radius >= T - 1 or anchor == T


MUTANTS = ("strict", "no-anchor", "one-sided", "tile-local")


def mutant_visible(defect, T, radius, anchor):
    """strict: ``<`` for ``<=``; no-anchor: the anchor ignored; one-sided: the band reaches back only (j <= i); tile-local:
    |i - j| taken on the indices inside their 32-frame tiles"""
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    if defect == "strict":
        return (j < anchor) | ((i - j).abs() < radius)
    if defect == "no-anchor":
        return (i - j).abs() <= radius
    if defect == "one-sided":
        return (j < anchor) | ((i - j >= 0) & (i - j <= radius))
    if defect == "tile-local":
        return (j < anchor) | ((i % 32 - j % 32).abs() <= radius)
    raise KeyError(defect)


def attention64(q, k, v, factor, vis):
    """float64 softmax(q k^T * factor, invisible keys at -inf) v per group; q / k / v [..., T, hd], vis bool [T, T]"""
    lg = q.double() @ k.double().transpose(-1, -2) * factor
    return torch.softmax(lg.masked_fill(~vis, float("-inf")), -1) @ v.double()


def clips_of(D, T, radius, anchor):
    return 1 + (T + radius + anchor) % 2


@functools.lru_cache(maxsize=None)
def operands(D, T, clips):
    """q, k, v ~ N(0, 1) in fp16, [clips, HW, heads, T, D]; one draw per (head_dim, T, clips), shared by every (radius, anchor)"""
    return ac._family_A((clips, HW, HEADS[D]), T, T, D, 1000 * D + 10 * T + clips)


@functools.lru_cache(maxsize=None)
def local_data(D, T, radius, anchor):
    """-> q, k, v fp16 and expect fp64, packed as ``ops.attn_temporal`` takes them: rows (clip, frame, pixel), columns (head, d)"""
    clips = clips_of(D, T, radius, anchor)
    q, k, v = operands(D, T, clips)
    P = ac._pack_temporal
    return types.SimpleNamespace(clips=clips, heads=HEADS[D], HW=HW, q=P(q), k=P(k), v=P(v),
                                 expect=P(attention64(q, k, v, D ** -0.5, visible(T, radius, anchor))))


def split_rows(t, clips, T, D):
    """packed rows -> [clips, HW, heads, T, D]"""
    return t.reshape(clips, T, HW, HEADS[D], D).permute(0, 2, 3, 1, 4)


def stand_in(q, k, v, nclips, T, HW, heads, head_dim=64, scale=None, out=None, Tq=None, key_mask=None, local=None):
    """``ops.attn_temporal_local(..., local=(radius, anchor))`` in torch fp32 on the CPU: the kernel's arithmetic in outline (fp32
    scores, invisible scores replaced before the maximum, fp16 output), packed rows in and out"""
    assert local is not None and Tq is None and key_mask is None
    vis = visible(T, *local)
    Q, K, V = (t.float().reshape(nclips, T, HW, heads, head_dim).permute(0, 2, 3, 1, 4) for t in (q, k, v))
    lg = (Q @ K.transpose(-1, -2) * (head_dim ** -0.5 if scale is None else scale)).masked_fill(~vis, -1e30)
    res = ac._pack_temporal(torch.softmax(lg, -1) @ V).half()
    if out is None:
        return res
    out[:] = res
    return out


def release():
    operands.cache_clear()
    local_data.cache_clear()
