"""TEST INFRASTRUCTURE ONLY: the cases of the long temporal attention (csrc/attention.hip attn_temporal_long_kernel, 33 ... 128
frames per clip), built on tests/op_cases.py and tests/attn_cases.py in the same way as the T <= 32 tables: a case is an
``op_cases.Case`` of ``attn_temporal`` whose arguments are guarded views (NaN guard rows before and after, 8 guard columns on the
left, q / k,v / out with three different leading dimensions), so ``op_cases.run`` takes the identical case through
tests/emu_ops.py on the CPU (tests/test_temporal_long_cpu.py) and through ``mofa_video_amd.ops`` on the GPU
(tests/test_attn_temporal_long_gpu.py).

Families, each a function of (T, head_dim, HW, heads, clips):

  "gauss"     q, k, v ~ N(0, 1) against float64 (attn_cases.attention64), tolerance TOL["attn_temporal"].
  "select"    k = random +-a sign vectors, q[i] = k[pi(i)] for ONE fixed permutation pi of 0 .. T-1 (``selection_perm``), v =
              integers / 64: the matched key has probability 1, every other probability is below 2^-40 of it (asserted in fp64,
              a draw that misses is re-seeded) and rounds to fp16 zero, so out[i] == v[pi(i)] element for element.  pi walks
              the keys with a stride near 32, so the queries of every 32-query block land in every 32-key tile: the key-slot <->
              tile <-> frame mapping and the query-block stores are pinned by equality.
  "count-one" k = 0 (every probability 1 / T), v = 0 but for frame T-1, which holds 1.0: every output is 1 / T to one fp16 ulp
              (1 / (T +- 1) is T / (T +- 1) ulps of 2^-11 relative, i.e. >= 15 ulps, away).
  "count-c"   k = 0, v = c everywhere with c a multiple of 2^-7 below 4: the fp32 sum c T is exact and the output equals c.
  "phantom"   two clips; clip 1's K / V rows hold either ordinary values or keys with huge logits (8 q) and NaN values.  Clip
              0's output must not depend on which: a last key tile that read rows >= T of clip 0 would read clip 1's rows."""
import functools
import math
import types

import torch

import attn_cases as ac
from op_cases import TOL, Case, close_errors, guard, run  # noqa: F401  (re-exported for the two test files)

LONG_T = (33, 40, 63, 64, 65, 95, 96, 97, 125, 127, 128)
LONG_HD = (64, 128)
LONG_GEOM = ((1, 1, 1), (5, 2, 2), (7, 1, 2))            # (HW, heads, clips): 1 / 20 / 14 sequences
COUNT_C = 511.0 / 128.0                                    # 3.9921875


def _perm(T, a):
    return [(a * i + T - 1) % T for i in range(T)]


def _perm_spreads(T, pi):
    """the queries of every FULL 32-query block land in every key tile that holds at least as many keys as there are query
    blocks (a last tile of one key can be matched by one query only), a partial last block of n queries in min(n, number of
    such tiles) different tiles"""
    kt = -(-T // 32)
    big = {t for t in range(kt) if min(32, T - 32 * t) >= kt}
    for q0 in range(0, T, 32):
        n = min(q0 + 32, T) - q0
        tiles = {pi[i] // 32 for i in range(q0, q0 + n)}
        if not (big <= tiles if n == 32 else len(tiles) >= min(n, len(big))):
            return False
    return True


@functools.lru_cache(maxsize=None)
def selection_perm(T):
    """pi(i) = (a i + T - 1) mod T with a the smallest integer >= 29 coprime to T for which ``_perm_spreads`` holds: ONE fixed
    permutation of 0 .. T-1 per T whose consecutive images are about one key tile apart"""
    a = next(a for a in range(29, 29 + 2 * T) if math.gcd(a, T) == 1 and _perm_spreads(T, _perm(T, a)))
    return tuple(_perm(T, a))


def assert_selection_perm(T):
    """pi is a permutation of all T keys -- keys 0, 31, 32, 63, 64 (those below T) and T-1 are all matched -- that spreads every
    query block over the key tiles (``_perm_spreads``)"""
    pi = selection_perm(T)
    assert sorted(pi) == list(range(T)), T
    assert _perm_spreads(T, pi), T
    assert {j for j in (0, 31, 32, 63, 64, T - 1) if j < T} <= set(pi)


def ulp16(x):
    """the spacing of fp16 at |x| (normal range)"""
    return 2.0 ** (math.floor(math.log2(abs(x))) - 10)


@functools.lru_cache(maxsize=128)
def long_data(form, T, hd, HW, heads, clips, seed=11):
    G, Cc = (clips, HW, heads), heads * hd
    factor = hd ** -0.5
    pi = tol = None
    if form == "gauss":
        q, k, v = ac._family_A(G, T, T, hd, seed)
        expect, tol = ac.attention64(q, k, v, factor), TOL["attn_temporal"]
    elif form == "select":
        pi = torch.tensor(selection_perm(T)).expand(*G, T)
        for attempt in range(8):
            g = torch.Generator().manual_seed(seed + 7919 * attempt)
            k = ((torch.randint(0, 2, (*G, T, hd), generator=g) * 2 - 1) * ac.C_AMPLITUDE[hd]).half()
            v = (torch.randint(-512, 513, (*G, T, hd), generator=g).float() / 64).half()
            q = torch.gather(k, -2, pi[..., None].expand(*G, T, hd))
            st = ac.logit_stats(q, k, factor, None, pi)
            if st["others"] < ac.C_OTHERS_MAX and st["match"] <= ac.C_MATCH_LOGIT_MAX:
                break
        else:
            raise AssertionError(f"selection precondition not met in 8 draws: {st}")
        expect = torch.gather(v, -2, pi[..., None].expand(*G, T, hd))
    elif form in ("count-one", "count-c"):
        g = torch.Generator().manual_seed(seed)
        q = torch.randn(*G, T, hd, generator=g).half()
        k = torch.zeros(*G, T, hd).half()
        if form == "count-one":
            v = torch.zeros(*G, T, hd).half()
            v[..., T - 1, :] = 1.0
            expect = torch.full((*G, T, hd), 1.0 / T, dtype=torch.float64)
        else:
            v = torch.full((*G, T, hd), COUNT_C).half()
            expect = v.clone()
    elif form in ("phantom-plain", "phantom-decoy"):
        assert clips == 2
        q, k, v = ac._family_A(G, T, T, hd, seed)
        if form == "phantom-decoy":                      # clip 1: every key would win any softmax it entered, every value is NaN
            k[1], v[1] = (8 * q[1].float()).half(), ac.NAN
        expect = ac.attention64(q[:1], k[:1], v[:1], factor)            # of clip 0 alone
        tol = TOL["attn_temporal"]
    else:
        raise KeyError(form)
    P = ac._pack_temporal
    return types.SimpleNamespace(q=P(q), k=P(k), v=P(v), expect=P(expect), pi=pi, tol=tol,
                                 where=lambda row, col: f"clip {row // (T * HW)} frame {row // HW % T} pixel {row % HW} head {col // hd} d {col % hd}")


def long_case(form, T, hd, HW, heads, clips):
    def data():
        return long_data(form, T, hd, HW, heads, clips)

    def build():
        d, Cc = data(), heads * hd
        return dict(q=guard(d.q, ld=Cc + 24), k=guard(d.k, ld=Cc + 40), v=guard(d.v, ld=Cc + 40), nclips=clips, T=T, HW=HW, heads=heads,
                    head_dim=hd, out=guard(shape=(clips * T * HW, Cc), ld=Cc + 56))
    case = Case(f"temporal-long/hd{hd}-T{T}-hw{HW}-h{heads}-c{clips}-{form}", "attn_temporal", build, form)
    case.data, case.form, case.T, case.hd, case.HW = data, form, T, hd, HW
    return case


def check_long(case, r):
    """guards intact and inputs unchanged, the result is the ``out`` buffer, then the family's check -> (worst err / bound, [messages])"""
    d, errs = case.data(), list(r.guard_errors())
    if r.ret is not r.placed["out"].t:
        errs.append(f"{case.id}: the call does not return its out buffer")
    out = r.placed["out"].t.detach().cpu()
    if case.form.startswith("phantom"):                  # clip 1's rows are NaN by construction in the decoy run: clip 0 only
        out = out[:case.T * case.HW]
    nonfinite = ~torch.isfinite(out.float())
    if nonfinite.any():
        rr, cc = torch.nonzero(nonfinite)[0].tolist()
        return float("inf"), errs + [f"{case.id}: {int(nonfinite.sum())} non-finite outputs, first at [{rr}, {cc}] = {d.where(rr, cc)}"]
    if case.form in ("select", "count-c"):
        bad = ~(out == d.expect)
        if bad.any():
            rr, cc = torch.nonzero(bad)[0].tolist()
            errs.append(f"{case.id}: {int(bad.sum())} / {bad.numel()} elements differ ({int(bad.any(1).sum())} rows), first at [{rr}, {cc}] = "
                        f"{d.where(rr, cc)}" + (f" (matches key {selection_perm(case.T)[rr // case.HW % case.T]})" if d.pi is not None else "")
                        + f": got {out[rr, cc].item()!r}, expected {d.expect[rr, cc].item()!r}")
        return (float("inf") if bad.any() else 0.0), errs
    if case.form == "count-one":
        err = (out.double() - 1.0 / case.T).abs().max().item() / ulp16(1.0 / case.T)
        if err > 1.0:
            errs.append(f"{case.id}: output {err:.2f} fp16 ulps away from 1 / {case.T}")
        return err, errs
    worst, msg = close_errors(out, d.expect, d.tol, case.id)
    return worst, errs + ([msg] if msg is not None else [])


def release():
    long_data.cache_clear()
