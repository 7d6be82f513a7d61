"""TEST INFRASTRUCTURE ONLY: the cases of the masked / rectangular long temporal attention (csrc/attention.hip
attn_temporal_long_masked_kernel through ``ops.attn_temporal_sharded``): Tq query frames against T in 33 .. 128 key slots under a
key mask of up to 128 bits.  Built like tests/attn_long_cases.py: a case is an ``op_cases.Case`` whose arguments are guarded views
(NaN guard rows and columns, three leading dimensions), so ``op_cases.run`` takes the identical case through the stand-in of
tests/emu_sharded.py on the CPU and through ``mofa_video_amd.ops`` on the GPU.

Families, each restricted to the L live slots of the mask:

  "gauss"     q, k, v ~ N(0, 1) against float64 (attn_cases.attention64 with the dead slots removed), TOL["attn_temporal"].
  "select"    attn_cases' family C: k = +-a sign vectors, every query equals one live key (a seeded permutation of the live
              keys walked round), v = integers / 64: the match has probability 1, the rest sums below 2^-40 of it (asserted in
              fp64, a draw that misses is re-seeded), so out[i] == v[pi(i)] element for element.
  "count-one" k = 0 on the live slots, v = 0 but for the LAST live slot, which holds 1.0: every output is 1 / L to one fp16 ulp
              (L = 1: exactly 1).  One live slot too many or too few is >= 15 ulps away for L >= 16 and more below.
  "count-c"   k = 0, v = c on the live slots, c a multiple of 2^-7 below 4: the fp32 sum c L is exact and the output equals c.

The K / V rows of dead slots hold what ``fill`` says: "nan" (never-written memory), "decoy" (the query times 8 -- it would win
any softmax it entered -- with a value of 1000), "decoy-nan" (that key with NaN values) or "plain" (ordinary N(0, 1) rows).

Mask kinds of a T-slot buffer (``mask_kinds``): every slot; what ``parallel.FrameParallel.kv_mask`` gives for 2 / 3 / 4 frame
shards of uneven length that fill at most T slots (slots beyond frame_ranks x T_max, where that does not divide T, are dead
like padding); only slot 0; only slot T-1; one whole 32-slot tile dead; every other slot."""
import functools
import types

import torch

import attn_cases as ac
from attn_long_cases import COUNT_C, LONG_GEOM, LONG_HD, ulp16  # noqa: F401  (re-exported)
from op_cases import NAN, TOL, Case, close_errors, guard, run  # noqa: F401

MASKED_T = (33, 64, 65, 97, 128)
MASKED_TQ = (1, 20, 33, "T")
KINDS = ("full", "lay2", "lay3", "lay4", "first", "last", "tile-dead", "alt")
FORMS = ("gauss", "select", "count-one", "count-c")
FILLS = ("nan", "decoy", "decoy-nan", "plain")
OP = "attn_temporal_sharded"


def tqs(T):
    return sorted({T if tq == "T" else tq for tq in MASKED_TQ if tq == "T" or tq <= T})


def layout_mask(T, shards):
    """the key mask of the largest clip of uneven shards whose gathered buffer has at most T slots: T_max = T // shards, only
    the first shard is full -- from the Layout / FrameParallel code itself"""
    from mofa_video_amd.parallel import FrameParallel, Layout
    t_max = T // shards
    frames = shards * t_max - (shards - 1)
    par = FrameParallel(Layout(shards, 0, frames, cfg_ranks=1), None)
    assert par.kv_slots == shards * t_max <= T and bin(par.kv_mask).count("1") == frames
    return par.kv_mask


@functools.lru_cache(maxsize=None)
def mask_kinds(T):
    """{kind: (key_mask or None, [live slots])}"""
    word = lambda live: sum(1 << j for j in live)
    live_of = lambda m: [j for j in range(T) if (m >> j) & 1]
    dead_tile = 0 if T < 64 else 1
    kinds = {"full": None, "first": 1, "last": 1 << (T - 1), "alt": word(range(0, T, 2)),
             "tile-dead": word(j for j in range(T) if j // 32 != dead_tile)}
    for n in (2, 3, 4):
        kinds[f"lay{n}"] = layout_mask(T, n)
    return {k: (m, list(range(T)) if m is None else live_of(m)) for k, m in kinds.items()}


def assert_mask_table():
    """what the kinds are for: dead slots in every tile position (first, last, inside, a whole tile), masks that differ between
    their 32-bit words, and layout masks with padding slots inside the buffer as well as behind it"""
    assert set(KINDS) == set(mask_kinds(33)) and MASKED_T == (33, 64, 65, 97, 128)
    for T in MASKED_T:
        kinds = mask_kinds(T)
        for kind, (m, live) in kinds.items():
            assert live and all(0 <= j < T for j in live), (T, kind)
            assert (m is None) == (kind == "full") and (m is None or (m >> T) == 0), (T, kind)
        assert kinds["first"][1] == [0] and kinds["last"][1] == [T - 1]
        t = 0 if T < 64 else 1
        assert not any(j // 32 == t for j in kinds["tile-dead"][1]) and len(kinds["tile-dead"][1]) == T - min(32, T - 32 * t)
        for n in (2, 3, 4):
            live = kinds[f"lay{n}"][1]
            dead = sorted(set(range(T)) - set(live))
            assert len(dead) >= n - 1 and (n == 2 or any(d < max(live) for d in dead)), (T, n, dead)     # padding between live slots
        assert any(j >= 32 for j in kinds["alt"][1]) and 1 not in kinds["alt"][1] and len(kinds["alt"][1]) == (T + 1) // 2
    w = lambda m, i: (m >> (32 * i)) & 0xffffffff
    m = mask_kinds(97)["lay4"][0]
    assert w(m, 1) != w(m, 2) and w(m, 0) != w(m, 1)                      # (the mutant that exchanges words 1 and 2 needs this)
    assert any(T > 96 for T in MASKED_T) and any(32 < T <= 64 for T in MASKED_T)


@functools.lru_cache(maxsize=96)
def masked_data(form, T, Tq, kind, hd, HW, heads, clips, fill="nan", seed=17):
    key_mask, live = mask_kinds(T)[kind]
    L = len(live)
    dead = torch.tensor([j not in live for j in range(T)]) if L < T else None
    G, factor = (clips, HW, heads), hd ** -0.5
    pi = tol = None
    if form == "gauss":
        q, k, v = ac._family_A(G, Tq, T, hd, seed)
        expect, tol = ac.attention64(q, k, v, factor, dead), TOL["attn_temporal"]
    elif form == "select":
        q, k, v, expect, pi, st = ac._make("C", G, Tq, T, hd, seed, dead, None, "cpu")
        assert st["others"] < ac.C_OTHERS_MAX and st["match"] <= ac.C_MATCH_LOGIT_MAX, st
        assert set(pi.flatten().tolist()) <= set(live)
    elif form in ("count-one", "count-c"):
        q = torch.randn(*G, Tq, hd, generator=torch.Generator().manual_seed(seed)).half()
        k = torch.zeros(*G, T, hd).half()
        if form == "count-one":
            v = torch.zeros(*G, T, hd).half()
            v[..., live[-1], :] = 1.0
            expect = torch.full((*G, Tq, hd), 1.0 / L, dtype=torch.float64)
        else:
            v = torch.full((*G, T, hd), COUNT_C).half()
            expect = torch.full((*G, Tq, hd), COUNT_C).half()
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
                k[..., j, :], v[..., j, :] = (torch.randn(*G, hd, generator=g).half() for _ in range(2))
            else:
                raise KeyError(fill)
    P = ac._pack_temporal
    return types.SimpleNamespace(
        q=P(q), k=P(k), v=P(v), expect=P(expect), pi=pi, tol=tol, key_mask=key_mask, live=live,
        where=lambda row, col: f"clip {row // (Tq * HW)} query frame {row // HW % Tq} pixel {row % HW} head {col // hd} d {col % hd}")


def masked_case(form, T, Tq, kind, hd, HW, heads, clips, fill="nan"):
    def data():
        return masked_data(form, T, Tq, kind, hd, HW, heads, clips, fill)

    def build():
        d, Cc = data(), heads * hd
        kw = dict(q=guard(d.q, ld=Cc + 24), k=guard(d.k, ld=Cc + 40), v=guard(d.v, ld=Cc + 40), nclips=clips, T=T, HW=HW, heads=heads,
                  head_dim=hd, out=guard(shape=(clips * Tq * HW, Cc), ld=Cc + 56), Tq=Tq)
        if d.key_mask is not None:
            kw["key_mask"] = d.key_mask
        return kw
    case = Case(f"temporal-long-masked/hd{hd}-T{T}-Tq{Tq}-{kind}-{fill}-hw{HW}-h{heads}-c{clips}-{form}", OP, build, form)
    case.data, case.form, case.T, case.Tq, case.kind, case.hd, case.HW = data, form, T, Tq, kind, hd, HW
    return case


def cases_of(T, hd, forms=FORMS, geoms=LONG_GEOM):
    """every (Tq, mask kind, geometry, family) of one (T, head_dim)"""
    return [masked_case(form, T, Tq, kind, hd, HW, heads, clips)
            for Tq in tqs(T) for kind in KINDS for HW, heads, clips in geoms for form in forms]


def check_masked(case, r):
    """guards intact and inputs unchanged, the result is the ``out`` buffer, no non-finite output, then the family's check
    -> (worst err / bound, [messages])"""
    d, errs = case.data(), list(r.guard_errors())
    if r.ret is not r.placed["out"].t:
        errs.append(f"{case.id}: the call does not return its out buffer")
    out = r.placed["out"].t.detach().cpu()
    if out.shape != d.expect.shape:
        return float("inf"), errs + [f"{case.id}: shape {tuple(out.shape)} != {tuple(d.expect.shape)}"]
    nonfinite = ~torch.isfinite(out.float())
    if nonfinite.any():
        rr, cc = torch.nonzero(nonfinite)[0].tolist()
        return float("inf"), errs + [f"{case.id}: {int(nonfinite.sum())} non-finite outputs, first at [{rr}, {cc}] = {d.where(rr, cc)}"]
    if case.form in ("select", "count-c"):
        bad = ~(out == d.expect)
        if bad.any():
            rr, cc = torch.nonzero(bad)[0].tolist()
            errs.append(f"{case.id}: {int(bad.sum())} / {bad.numel()} elements differ ({int(bad.any(1).sum())} rows), first at [{rr}, {cc}] = "
                        f"{d.where(rr, cc)}: got {out[rr, cc].item()!r}, expected {d.expect[rr, cc].item()!r}")
        return (float("inf") if bad.any() else 0.0), errs
    if case.form == "count-one":
        L = len(d.live)
        err = (out.double() - 1.0 / L).abs().max().item() / ulp16(1.0 / L)
        if err > 1.0:
            errs.append(f"{case.id}: output {err:.2f} fp16 ulps away from 1 / {L}")
        return err, errs
    worst, msg = close_errors(out, d.expect, d.tol, case.id)
    return worst, errs + ([msg] if msg is not None else [])


# ---------------------------------------------------------------------------------------------------------------------------
# mutants: fp64 attention over the live slots with one defect of the mask handling each
# ---------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("mask-shift", "swap-words", "low-only", "dead-v")


def wrong_sharded(defect):
    """``defect`` None: the plain fp64 truth.  mask-shift: the mask read one slot off; swap-words: mask words 1 and 2 exchanged;
    low-only: the mask honoured below slot 32 only (every slot from 32 to T-1 taken as live); dead-v: the scores are masked
    correctly, but the V rows of dead slots enter the sum with weight 0 (0 * NaN)"""
    def attn_temporal_sharded(q, k, v, nclips, T, HW, heads, head_dim=64, scale=None, out=None, Tq=None, key_mask=None):
        Tq, full = (T if Tq is None else Tq), (1 << T) - 1
        m = full if key_mask is None else key_mask & full
        if defect == "mask-shift":
            m = (m << 1) & full
        elif defect == "swap-words":
            w = [(m >> (32 * i)) & 0xffffffff for i in range(4)]
            w[1], w[2] = w[2], w[1]
            m = sum(x << (32 * i) for i, x in enumerate(w)) & full
        elif defect == "low-only":
            m |= full & ~0xffffffff
        dead = torch.tensor([not (m >> j) & 1 for j in range(T)])
        Q = q.double().reshape(nclips, Tq, HW, heads, head_dim).permute(0, 2, 3, 1, 4)
        K, V = (t.double().reshape(nclips, T, HW, heads, head_dim).permute(0, 2, 3, 1, 4) for t in (k, v))
        lg = Q @ K.masked_fill(dead[:, None], 0.0).transpose(-1, -2) * (head_dim ** -0.5 if scale is None else scale)
        p = torch.softmax(lg.masked_fill(dead, float("-inf")), -1)
        o = p @ (V if defect == "dead-v" else V.masked_fill(dead[:, None], 0.0))
        out[:] = ac._pack_temporal(o).half()
        return out
    return types.SimpleNamespace(attn_temporal_sharded=attn_temporal_sharded)


def release():
    masked_data.cache_clear()
