"""TEST INFRASTRUCTURE ONLY: the cases of the streaming temporal attention of a frame shard (csrc/attention.hip
attn_temporal_stream_shard_kernel, mofa_attn_temporal_stream_shard_f16, ``ops.attn_temporal_stream_shard``): Tq query frames against
1 <= S <= 1024 key slots, in the two modes of the entry point.  A case is an ``op_cases.Case`` whose tensor arguments are guarded
views (NaN guard rows and columns, three leading dimensions), so ``op_cases.run`` takes the identical case through ``stand_in`` on
the CPU (tests/test_attn_stream_shard_cases_cpu.py) and through ``mofa_video_amd.ops`` on the GPU
(tests/test_attn_temporal_stream_shard_gpu.py).  Geometry as in tests/attn_local_cases.py: HW = 5, heads 2 at head dim 64 and 1 at
128, 1 or 2 clips.  Every expectation is float64 on the WHOLE clip (``attn_cases.attention64`` with the dead slots removed;
``attn_local_cases.attention64`` under the rule on global frames, through tests/attn_window_cases.py), so nothing of the slot
layout or of the tile walk enters it; the bound is ``TOL["attn_temporal"]`` of tests/op_cases.py.

Dense mode (``local=None``, a key mask), ``DENSE_CASES`` = (head dim, S, Tq, mask kind, fill, family):
  S        129, 160, 161, 256, 257, 1024 (Tq = 33 and one clip only), and 132, 252, 264 = the gathered buffers of 130 frames over
           3 shards (44 + 43 + 43), 250 over 4 and 259 over 8 with the mask ``FrameParallel.kv_mask`` gives for them;
  Tq       1, 31, 32, 33, 65, S;
  kinds    ``mask_kinds``: every slot; uneven 3 / 4 / 8 frame shards; padding bits on slots 31 / 32 / 63 / 64; only slot 0; only
           slot S - 1; the first, the last or a middle 32-slot tile wholly dead; every other slot;
  fills    of the K / V rows of dead slots, as in tests/attn_long_masked_cases.py: "nan", "decoy" (the query x 8 with value 1000),
           "decoy-nan", "plain";
  families "gauss" (fp64, the bound), "select" (the output equals one live v row element for element), "count-one" (1 / L to one
           fp16 ulp), "count-c" (exact) -- those of tests/attn_long_masked_cases.py on more slots.
Per S every kind and every Tq occurs in a gauss case (the other coordinate and the fill cycle); the exact families take three
kinds each; head dim 128 runs at S = 129 and 257.

Window mode (``local=(radius, anchor)``), ``WINDOW_CASES`` = (head dim, T_full, shards, radius, anchor, shard): every shard of
every layout of ``LAYOUTS``, the data and the fp64 expectation those of ``attn_window_cases.window_data``.

``stand_in`` has the op's signature and walks a sequence as the kernel does: per 32-query block the tiles that hold a slot some
query of the block sees, ascending, with a running maximum, a running sum and rescaled accumulators.  ``kernel_tiles`` restates
the kernel's own tile arithmetic; ``assert_table`` proves the two agree and that the table holds what it claims."""
import functools
import types

import torch

import attn_cases as ac
import attn_local_cases as lc
import attn_long_masked_cases as mc
import attn_window_cases as wc
from attn_long_cases import COUNT_C, ulp16  # noqa: F401  (re-exported)
from op_cases import NAN, TOL, Case, close_errors, guard, run  # noqa: F401

OP = "attn_temporal_stream_shard"
HW = lc.HW
HEADS = lc.HEADS
BOUND = TOL["attn_temporal"]
check = mc.check_masked                  # guards, the returned buffer, finiteness, then the family's comparison

# ---- dense mode --------------------------------------------------------------------------------------------------------------------
DENSE_S = (129, 160, 161, 256, 257)
BIG_S = 1024
LAYOUT_CLIPS = ((130, 3), (250, 4), (259, 8))          # (frames, frame shards) -> S = shards x largest shard = 132, 252, 264
DENSE_TQ = (1, 31, 32, 33, 65, "S")
FORMS = ("gauss", "select", "count-one", "count-c")
FILLS = ("nan", "decoy", "decoy-nan", "plain")
PAD_EDGES = (31, 32, 63, 64)


def tqs(S):
    return [S if t == "S" else t for t in DENSE_TQ]


def _kv_mask(frames, shards):
    """(slots, mask) of the gathered buffer of ``frames`` over ``shards`` -- from the Layout / FrameParallel code itself"""
    from mofa_video_amd.parallel import FrameParallel, Layout
    par = FrameParallel(Layout(shards, 0, frames, cfg_ranks=1), None)
    assert bin(par.kv_mask).count("1") == frames
    return par.kv_slots, par.kv_mask


def layout_mask(S, shards):
    """the key mask of the largest clip of uneven shards whose gathered buffer has at most S slots (only the first shard is
    full); slots beyond shards x T_max are dead like padding"""
    t_max = S // shards
    slots, m = _kv_mask(shards * t_max - (shards - 1), shards)
    assert slots == shards * t_max <= S
    return m


LAYOUT_S = {_kv_mask(f, n)[0]: (f, n) for f, n in LAYOUT_CLIPS}


@functools.lru_cache(maxsize=None)
def mask_kinds(S):
    """{kind: (key_mask or None, [live slots])}"""
    word = lambda live: sum(1 << j for j in live)
    live_of = lambda m: [j for j in range(S) if (m >> j) & 1]
    nt = (S + 31) // 32
    kinds = {"full": None, "first": 1, "last": 1 << (S - 1), "alt": word(range(0, S, 2)),
             "pad-edges": word(j for j in range(S) if j not in PAD_EDGES),
             "tile-first-dead": word(range(32, S)), "tile-last-dead": word(range(32 * (nt - 1))),
             "tile-mid-dead": word(j for j in range(S) if j // 32 != nt // 2)}
    for n in (3, 4, 8):
        kinds[f"lay{n}"] = layout_mask(S, n)
    if S in LAYOUT_S:
        kinds["lay"] = _kv_mask(*LAYOUT_S[S])[1]
    return {k: (m, list(range(S)) if m is None else live_of(m)) for k, m in kinds.items()}


def _dense_cases():
    cases = []
    for si, S in enumerate(DENSE_S):
        kinds, tq = list(mask_kinds(S)), tqs(S)
        for i, kind in enumerate(kinds):                               # every kind per S, Tq and fill cycling
            cases.append((64, S, tq[(i + si) % len(tq)], kind, FILLS[(i + si) % 4], "gauss"))
        for i, t in enumerate(tq):                                     # every Tq per S, kind and fill cycling
            cases.append((64, S, t, kinds[(3 * i + 1 + si) % len(kinds)], FILLS[(i + si + 2) % 4], "gauss"))
        for fi, form in enumerate(FORMS[1:]):
            for j in range(3):
                cases.append((64, S, tq[(2 * j + fi + si) % len(tq)], kinds[(4 * j + 3 * fi + si) % len(kinds)],
                              FILLS[(j + fi + si) % 4], form))
    for S in sorted(LAYOUT_S):                                          # the gathered buffers of uneven shards: shard 0's queries
        tq = -(-LAYOUT_S[S][0] // LAYOUT_S[S][1])
        cases += [(64, S, tq, "lay", "nan", "gauss"), (64, S, tq, "lay", "decoy", "count-one"), (64, S, tq, "lay", "decoy-nan", "select"),
                  (64, S, S, "full", "plain", "gauss")]
    cases += [(64, BIG_S, 33, kind, fill, form) for kind, fill, form in
              (("full", "plain", "gauss"), ("alt", "nan", "gauss"), ("tile-mid-dead", "decoy", "gauss"), ("lay8", "decoy-nan", "gauss"),
               ("lay3", "nan", "count-one"), ("tile-first-dead", "nan", "select"))]
    for S in (129, 257):
        cases += [(128, S, 33, "full", "plain", "gauss"), (128, S, S, "lay3", "nan", "gauss"), (128, S, 65, "tile-mid-dead", "decoy", "gauss"),
                  (128, S, 1, "alt", "decoy-nan", "gauss"), (128, S, 32, "last", "nan", "select"), (128, S, 31, "pad-edges", "nan", "count-c")]
    return tuple(dict.fromkeys(cases))


DENSE_CASES = _dense_cases()


def dense_clips(D, S, Tq, kind, fill, form):
    return 1 if S == BIG_S else 1 + (S + Tq + len(kind)) % 2


@functools.lru_cache(maxsize=64)
def dense_data(D, S, Tq, kind, fill, form, seed=23):
    """what the op takes, packed (rows (clip, frame or slot, pixel), columns (head, d)), the expectation and the live slots"""
    key_mask, live = mask_kinds(S)[kind]
    L, clips = len(live), dense_clips(D, S, Tq, kind, fill, form)
    dead = torch.tensor([j not in set(live) for j in range(S)]) if L < S else None
    G, factor = (clips, HW, HEADS[D]), D ** -0.5
    pi = None
    if form == "gauss":
        q, k, v = ac._family_A(G, Tq, S, D, seed + S)
        expect = ac.attention64(q, k, v, factor, dead)
    elif form == "select":
        q, k, v, expect, pi, st = ac._make("C", G, Tq, S, D, seed, dead, None, "cpu")
        assert st["others"] < ac.C_OTHERS_MAX and st["match"] <= ac.C_MATCH_LOGIT_MAX, st
        assert set(pi.flatten().tolist()) <= set(live)
    elif form in ("count-one", "count-c"):
        q = torch.randn(*G, Tq, D, generator=torch.Generator().manual_seed(seed)).half()
        k = torch.zeros(*G, S, D).half()
        if form == "count-one":
            v = torch.zeros(*G, S, D).half()
            v[..., live[-1], :] = 1.0
            expect = torch.full((*G, Tq, D), 1.0 / L, dtype=torch.float64)
        else:
            v = torch.full((*G, S, D), COUNT_C).half()
            expect = torch.full((*G, Tq, D), COUNT_C).half()
    else:
        raise KeyError(form)
    if dead is not None:
        g = torch.Generator().manual_seed(seed + 1)
        for j in torch.nonzero(dead).flatten().tolist():
            if fill == "nan":
                k[..., j, :], v[..., j, :] = NAN, NAN
            elif fill in ("decoy", "decoy-nan"):
                k[..., j, :], v[..., j, :] = (8 * q[..., j % Tq, :].float()).half(), (1000.0 if fill == "decoy" else NAN)
            elif fill == "plain":
                k[..., j, :], v[..., j, :] = (torch.randn(*G, D, generator=g).half() for _ in range(2))
            else:
                raise KeyError(fill)
    P = ac._pack_temporal
    return types.SimpleNamespace(
        clips=clips, heads=HEADS[D], HW=HW, q=P(q), k=P(k), v=P(v), expect=P(expect), pi=pi, tol=BOUND, key_mask=key_mask, live=live,
        kw=dict(Tq=Tq, **({} if key_mask is None else dict(key_mask=key_mask))),
        where=lambda row, col: f"clip {row // (Tq * HW)} query frame {row // HW % Tq} pixel {row % HW} head {col // D} d {col % D}")


# ---- window mode -------------------------------------------------------------------------------------------------------------------
LAYOUTS = ((256, 4, 48, 1), (256, 2, 31, 33), (250, 4, 62, 2), (300, 4, 40, 0), (258, 2, 0, 0), (1024, 8, 64, 1), (200, 2, 33, 0))
HD128 = ((256, 4, 48, 1), (258, 2, 0, 0), (200, 2, 33, 0))
WINDOW_CASES = tuple((D, T, n, r, a, s) for (T, n, r, a) in LAYOUTS for s in range(n)
                     for D in ((64, 128) if (T, n, r, a) in HD128 else (64,)))


def window_data(D, T, n, r, a, s):
    """``attn_window_cases.window_data`` (the whole clip's operands, its fp64 local attention, this shard's rows and slots) with
    what ``check`` reads"""
    d = wc.window_data(D, T, n, r, a, s)
    Tq = d.g.Tq
    return types.SimpleNamespace(
        g=d.g, clips=d.clips, heads=d.heads, HW=HW, q=d.q, k=d.k, v=d.v, expect=d.expect, tol=BOUND, kw=d.kw, live=None, pi=None,
        where=lambda row, col: f"clip {row // (Tq * HW)} query frame {d.g.f0 + row // HW % Tq} pixel {row % HW} head {col // D} d {col % D}")


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def _case(id_, form, data, S, D):
    def build():
        d, Cc = data(), HEADS[D] * D
        return dict(q=guard(d.q, ld=Cc + 24), k=guard(d.k, ld=Cc + 40), v=guard(d.v, ld=Cc + 40), nclips=d.clips, S=S, HW=HW,
                    heads=d.heads, head_dim=D, out=guard(shape=tuple(d.expect.shape), ld=Cc + 56), **d.kw)
    case = Case(id_, OP, build, form)
    case.data, case.form, case.S, case.hd = data, form, S, D
    return case


def dense_case(D, S, Tq, kind, fill, form):
    case = _case(f"temporal-stream-shard/dense-hd{D}-S{S}-Tq{Tq}-{kind}-{fill}-{form}", form,
                 lambda: dense_data(D, S, Tq, kind, fill, form), S, D)
    case.key = (D, S, Tq, kind, fill, form)
    return case


def window_case(D, T, n, r, a, s):
    S = wc.geometry(T, n, r, a, s).S
    case = _case(f"temporal-stream-shard/window-hd{D}-T{T}-over{n}-r{r}-a{a}-shard{s}", "gauss", lambda: window_data(D, T, n, r, a, s), S, D)
    case.key = (D, T, n, r, a, s)
    return case


def dense_cases():
    return [dense_case(*c) for c in DENSE_CASES]


def window_cases():
    return [window_case(*c) for c in WINDOW_CASES]


# ---- the rule in slot space, the kernel's tiles, the stand-in ------------------------------------------------------------------------
def slot_visible(S, Tq, local, q_frame0, band_frame0, key_mask, _visible=None):
    """THE rule -> bool [Tq, S].  dense: the live slots for every query; window: ``attn_window_cases.slot_visible``"""
    if local is None:
        m = (1 << S) - 1 if key_mask is None else int(key_mask) & ((1 << S) - 1)
        return torch.tensor([bool((m >> j) & 1) for j in range(S)])[None, :].expand(Tq, S)
    radius, anchor = local
    L = S - anchor
    g = types.SimpleNamespace(f0=q_frame0, f1=q_frame0 + Tq, Tq=Tq, b0=band_frame0, b1=band_frame0 + L, L=L, S=S)
    return (_visible or wc.slot_visible)(g, radius, anchor)


def kernel_tiles(S, Tq, local, q_frame0, band_frame0, key_mask, q0):
    """the tiles the kernel visits for the 32-query block at q0, restated from its text: the anchor tiles and the band tiles of
    slots [lo of the block's first query, hi1 of its last), those whose mask word is non-zero"""
    m = (1 << S) - 1 if key_mask is None else int(key_mask) & ((1 << S) - 1)
    radius, anchor = (1 << 30, 0) if local is None else (min(local[0], S - 1), local[1])
    g0, g1 = q_frame0 + q0, q_frame0 + min(q0 + 31, Tq - 1)
    hi_f = band_frame0 + (S - anchor) - 1
    lo = anchor + max(g0 - radius, anchor, band_frame0) - band_frame0
    hi1 = anchor + min(g1 + radius, hi_f) - band_frame0 + 1
    tiles = set(range((anchor + 31) // 32))
    if lo < hi1:
        tiles |= set(range(lo // 32, (hi1 - 1) // 32 + 1))
    return sorted(t for t in tiles if (m >> (32 * t)) & 0xffffffff)


def needed_tiles(vis, q0):
    """the tiles that hold a slot some query of the block at q0 sees"""
    return sorted({int(j) // 32 for j in torch.nonzero(vis[q0:q0 + 32].any(0)).flatten()})


def stand_in(q, k, v, nclips, S, HW, heads, head_dim=64, scale=None, out=None, Tq=None, local=None, q_frame0=0, band_frame0=0,
             key_mask=None, _visible=None):
    """``ops.attn_temporal_stream_shard`` in torch fp32 on the CPU, computed the way the kernel walks a sequence (tile by tile with
    a running maximum; an unseen slot's probability set to 0; the K / V rows of slots that do not exist taken as zeros, never
    read); packed rows in and out.  ``_visible(g, radius, anchor)``: a mutant's slot-space rule (window mode)"""
    Tq = S if Tq is None else Tq
    assert 1 <= S <= 1024 and Tq >= 1
    if local is None:
        assert q_frame0 == 0 and band_frame0 == 0
    else:
        radius, anchor = local
        assert key_mask is None and radius >= 0 and 0 <= anchor <= S
        assert 0 <= band_frame0 <= q_frame0 and q_frame0 + Tq <= band_frame0 + (S - anchor)
    vis = slot_visible(S, Tq, local, q_frame0, band_frame0, key_mask, _visible)
    assert bool(vis.any(1).all()), "a query that sees no slot"
    exists = vis.any(0) if local is None else torch.ones(S, dtype=torch.bool)
    Q = q.float().reshape(nclips, Tq, HW, heads, head_dim).permute(0, 2, 3, 1, 4)
    K, V = (t.float().reshape(nclips, S, HW, heads, head_dim).permute(0, 2, 3, 1, 4).masked_fill(~exists[:, None], 0.0) for t in (k, v))
    factor = head_dim ** -0.5 if scale is None else scale
    res = torch.empty_like(Q)
    for q0 in range(0, Tq, 32):
        rows = slice(q0, min(q0 + 32, Tq))
        n = rows.stop - rows.start
        m = torch.full((*Q.shape[:3], n, 1), -1e30)
        l = torch.zeros_like(m)
        o = torch.zeros(*Q.shape[:3], n, head_dim)
        for kt in needed_tiles(vis, q0):
            keys = torch.arange(32 * kt, min(32 * kt + 32, S))
            seen = vis[rows][:, keys]
            s = (Q[..., rows, :] @ K[..., keys, :].transpose(-1, -2) * factor).masked_fill(~seen, -1e30)
            mn = torch.maximum(m, s.amax(-1, keepdim=True))
            p = torch.where(seen, torch.exp(s - mn), torch.zeros(()))
            a = torch.exp(m - mn)
            l = l * a + p.sum(-1, keepdim=True)
            o = o * a + p.half().float() @ V[..., keys, :]
            m = mn
        res[..., rows, :] = o / l
    res = ac._pack_temporal(res).half()
    if out is None:
        return res
    out[:] = res
    return out


MUTANTS = wc.MUTANTS                     # duplicates, slot-distance, no-anchor, strict: wrong slot-space rules of the window


def mutant(defect):
    """a module with the op under one of ``attn_window_cases.mutant_slot_visible``'s wrong rules"""
    def op(*a, **kw):
        return stand_in(*a, _visible=lambda g, radius, anchor: wc.mutant_slot_visible(defect, g, radius, anchor), **kw)
    return types.SimpleNamespace(**{OP: op})


def assert_table():
    """the table holds what it is there for, and the kernel's tile arithmetic visits exactly the tiles that hold a visible slot"""
    keys = set(DENSE_CASES)
    assert len(DENSE_CASES) == len(keys) and len(WINDOW_CASES) == len(set(WINDOW_CASES))
    assert sorted(LAYOUT_S) == [132, 252, 264] and _kv_mask(130, 3)[1] == ((1 << 44) - 1) | (((1 << 43) - 1) << 44) | (((1 << 43) - 1) << 88)
    for S in DENSE_S + (BIG_S,) + tuple(LAYOUT_S):
        kinds, nt = mask_kinds(S), (S + 31) // 32
        for kind, (m, live) in kinds.items():
            assert live and all(0 <= j < S for j in live) and (m is None) == (kind == "full"), (S, kind)
            words = [(((1 << S) - 1 if m is None else m) >> (32 * t)) & 0xffffffff for t in range(nt)]
            dead_tiles = [t for t in range(nt) if not words[t]]
            want = {"tile-first-dead": [0], "tile-last-dead": [nt - 1], "tile-mid-dead": [nt // 2], "first": list(range(1, nt)),
                    "last": list(range(nt - 1))}.get(kind)
            assert want is None or dead_tiles == want, (S, kind, dead_tiles)
        assert 0 < nt // 2 < nt - 1
        assert kinds["first"][1] == [0] and kinds["last"][1] == [S - 1] and len(kinds["alt"][1]) == (S + 1) // 2
        assert set(range(S)) - set(kinds["pad-edges"][1]) == set(PAD_EDGES)
        for n in (3, 4, 8):
            live = kinds[f"lay{n}"][1]
            dead = sorted(set(range(S)) - set(live))
            assert len(dead) >= n - 1 and any(d < max(live) for d in dead), (S, n)          # padding between live slots
    for S in DENSE_S:                                                  # per S: every kind and every Tq in a gauss case, every family
        mine = [c for c in DENSE_CASES if c[0] == 64 and c[1] == S]
        assert {c[3] for c in mine if c[5] == "gauss"} == set(mask_kinds(S)), S
        assert {c[2] for c in mine if c[5] == "gauss"} == set(tqs(S)), S
        assert {c[5] for c in mine} == set(FORMS) and {c[4] for c in mine} == set(FILLS), S
    big = [c for c in DENSE_CASES if c[1] == BIG_S]
    assert big and all(c[2] == 33 and dense_clips(*c) == 1 for c in big)
    assert {c[1] for c in DENSE_CASES if c[0] == 128} == {129, 257}
    assert {dense_clips(*c) for c in DENSE_CASES} == {1, 2}
    for S, (f, n) in LAYOUT_S.items():
        assert any(c[1] == S and c[3] == "lay" for c in DENSE_CASES) and len(mask_kinds(S)["lay"][1]) == f
    # window layouts
    assert LAYOUTS == ((256, 4, 48, 1), (256, 2, 31, 33), (250, 4, 62, 2), (300, 4, 40, 0), (258, 2, 0, 0), (1024, 8, 64, 1), (200, 2, 33, 0))
    assert set(HD128) <= set(LAYOUTS) and len(HD128) == 3
    geoms = {(T, n, r, a, s): wc.geometry(T, n, r, a, s) for T, n, r, a in LAYOUTS for s in range(n)}
    for T, n, r, a in LAYOUTS:
        gs = [geoms[T, n, r, a, s] for s in range(n)]
        assert max(g.S for g in gs) > 128, (T, n, r, a)
        assert all(g.S <= 1024 and g.b0 <= g.f0 and g.f1 <= g.b1 for g in gs)
        assert gs[0].b0 == 0 and gs[-1].b1 == T and gs[-1].b1 - gs[-1].f1 < r + 1                 # first / last shard (truncated band)
    assert any(a > 0 and geoms[T, n, r, a, 0].b0 < a for T, n, r, a in LAYOUTS)                      # a band that repeats the anchor frames
    assert any(a % 32 and a > 32 for _, _, _, a in LAYOUTS)                                           # an anchor across a tile edge
    assert any(g.S == 129 for g in geoms.values())
    assert any(a == 0 and r % 32 for _, _, r, a in LAYOUTS)                                           # the -1e30 row
    hazard = False
    for (T, n, r, a, s), g in geoms.items():
        local = (r, a)
        vis = slot_visible(g.S, g.Tq, local, g.f0, g.b0, None)
        assert torch.equal(vis, wc.formula_visible(g, r, a)) and bool(vis.any(1).all()), (T, n, r, a, s)
        for q0 in range(0, g.Tq, 32):
            tiles = kernel_tiles(g.S, g.Tq, local, g.f0, g.b0, None, q0)
            assert tiles == needed_tiles(vis, q0), (T, n, r, a, s, q0, tiles)
            last_q = min(q0 + 31, g.Tq - 1)
            hazard |= a == 0 and not bool(vis[last_q, 32 * tiles[0]:32 * tiles[0] + 32].any())
    assert hazard, "no block whose first visited tile hides every slot from its last query"
    for D, S, Tq, kind, fill, form in DENSE_CASES:
        m = mask_kinds(S)[kind][0]
        vis = slot_visible(S, Tq, None, 0, 0, m)
        for q0 in range(0, Tq, 32):
            assert kernel_tiles(S, Tq, None, 0, 0, m, q0) == needed_tiles(vis, q0), (S, kind, q0)


def release():
    dense_data.cache_clear()
    mask_kinds.cache_clear()
    wc.release()
