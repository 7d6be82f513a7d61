"""TEST INFRASTRUCTURE ONLY: the sequence-edge case tables of the attention kernels (csrc/attention.hip), their fp64 reference, the
preconditions of the exact family and the "wrong attention" mutants that prove the checks can fail.

Built on tests/op_cases.py: a case is an ``op_cases.Case`` whose ``build()`` gives the keyword arguments of ``attn_spatial`` /
``attn_temporal`` as guarded views (NaN guard rows before and after, 8 guard columns on the left, a different leading dimension
for every argument of a call -- temporal k and v share one, ops.attn_temporal asserts it), so ``op_cases.run`` takes the
identical case through tests/emu_ops.py on the CPU (tests/test_attn_cases_cpu.py) and through ``mofa_video_amd.ops`` on the GPU
(tests/test_attn_edges_gpu.py).  The expectation is float64 softmax attention on the fp16 inputs exactly as the kernel receives
them.

Three input families, each a function of (S or T, head_dim, heads, frames / clips, seed):

  A "gauss"    q, k, v ~ N(0, 1): what the older attention tests use.  Sees gross errors; blind to a wrong key COUNT (one extra
               zero key moves every output by 1 / (S + 1) of itself, inside the tolerance from S ~ 100 on).
  B "sink"     m = sqrt(12 / sqrt(head_dim)), q = m + n / 4, k = -m + n / 4, v = n: every real logit lies near -12, so a phantom
               key of score 0 (a zero-filled LDS row beyond S or T whose mask is off by one) takes almost all of the weight and
               the output collapses towards 0: > 100 x the bound.  Precondition (asserted): all logits within b_logit_range().
  C "one-hot"  k = random +-a sign vectors, q[i] = k[pi(i)], v = integers in [-512, 512] / 64 (exact in fp16, <= 10 significant
               bits).  The matched key is the row maximum (probability exp2(0) = 1), every other probability is far below 2^-24
               and rounds to fp16 zero in the PV product, the fp32 row sum stays 1 (or 1 + O(1e-5) in the temporal kernel, which
               rounds a 10-bit value back to itself): the output is v[pi(i)] EQUAL BY VALUE, element for element -- the index
               algebra (source swizzle, transpose read, k-slot permutation shared by P and V^T) is checked exactly.
               Precondition (asserted, a condition and not a measurement): per row the fp64 sum of the non-matching weights
               relative to the match, computed with the match masked out, is below 2^-40, and the match logit is <= 128.  A
               draw that fails it is re-seeded, never skipped."""
import functools
import math
import types

import torch

import op_cases as oc
from op_cases import F16, NAN, TOL, Case, close_errors, guard, run  # noqa: F401  (re-exported for the two test files)

LN2 = 0.6931471805599453
C_AMPLITUDE = {64: 3.75, 128: 2.5}
C_OTHERS_MAX = 2.0 ** -40
C_MATCH_LOGIT_MAX = 128.0
# family B: logit = sum_d (m + a_d / 4)(-m + b_d / 4) * head_dim^-0.5 = -12 + noise of standard deviation 0.44 (head_dim 64:
# per-term variance m^2 / 8 + 1 / 256 with m^2 = 1.5, times 64 terms, times the squared scale 1 / 64) or 0.37 (head_dim 128);
# the product of the two positive row sums skews the tail towards MORE negative logits.  The range follows the number of
# logits of a case.  Every matrix shape has at most 300 * 300 * 21 = 1.9e6 < 2^21 of them: 5.2 sigma = 2.3 for a Gaussian,
# 2.5 with the skew.  The auto-dispatch pair has 6e7 (5.6 sigma, and the skewed tail reaches -15): it alone gets the wide
# range.  What the family is for holds in both: with every real logit <= -9 a phantom key of logit 0 holds
# >= 1 / (1 + 1000 e^-9) = 0.89 of the weight at S <= 1000, and with a spread of <= 7 nats no real key's weight falls below
# e^-7 of another's, so a dropped or exchanged real key still moves the output.
B_LOGIT_RANGE = (-14.5, -9.5)
B_LOGIT_RANGE_WIDE = (-16.0, -9.0)
B_LOGITS_MAX = 2 ** 21                 # cases with more logits than this are held to the wide range


def b_logit_range(nlogits):
    return B_LOGIT_RANGE if nlogits <= B_LOGITS_MAX else B_LOGIT_RANGE_WIDE

SPATIAL_INST = ((64, 1), (64, 2), (128, 1))                       # (head_dim, query_blocks): the three instantiations
SPATIAL_S = (1, 7, 31, 33, 63, 64, 65, 127, 129, 255, 257, 300, 1000)
HEADS_FRAMES = ((1, 1), (3, 1), (2, 3), (5, 1), (1, 8), (3, 7))   # cycled over SPATIAL_S
SPATIAL_FORMS = ("A", "B", "C", "C-prescaled")
AUTO_S, AUTO_HEADS, AUTO_FRAMES = (240, 241), 1, 1024            # query_blocks=0: the rule takes 128- / 256-row workgroups
AUTO_FORMS = ("B", "C", "C-prescaled")

TEMPORAL_T = (1, 2, 15, 16, 17, 24, 25, 31, 32)
TEMPORAL_HD = (64, 128)
TEMPORAL_GEOM = ((5, 1, 1), (5, 3, 1), (3, 1, 3), (1, 3, 5))      # (HW, heads, clips): 5 / 15 / 9 / 15 sequences, all odd
TEMPORAL_FORMS = ("A", "B", "C", "C-scale")
FILLS = ("nan", "decoy")


# ---------------------------------------------------------------------------------------------------------------------------
# the three families on [groups..., n, head_dim] tensors (one group = one softmax problem)
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _family_A(G, nq, nk, hd, seed):
    g = _gen(seed)
    return tuple(torch.randn(*G, n, hd, generator=g).half() for n in (nq, nk, nk))


def _family_B(G, nq, nk, hd, seed):
    g = _gen(seed)
    m = math.sqrt(12.0 / math.sqrt(hd))
    q = (m + 0.25 * torch.randn(*G, nq, hd, generator=g)).half()
    k = (-m + 0.25 * torch.randn(*G, nk, hd, generator=g)).half()
    return q, k, torch.randn(*G, nk, hd, generator=g).half()


def _family_C(G, nq, nk, hd, seed, live):
    """-> q, k, v, pi [groups..., nq]: the key every query matches; a permutation of the keys when all of them are live and
    nq == nk, else a seeded permutation of the live keys walked round"""
    g = _gen(seed)
    a = C_AMPLITUDE[hd]
    k = ((torch.randint(0, 2, (*G, nk, hd), generator=g) * 2 - 1) * a).half()
    v = (torch.randint(-512, 513, (*G, nk, hd), generator=g).float() / 64).half()
    order = torch.rand(*G, len(live), generator=g).argsort(-1)                 # a permutation of the live keys per group
    pi = torch.tensor(live)[order][..., torch.arange(nq) % len(live)]
    q = torch.gather(k, -2, pi[..., None].expand(*G, nq, hd))
    return q, k, v, pi


def attention64(q, k, v, factor, dead=None, device="cpu", chunk=32, keep=False):
    """float64 softmax(q k^T * factor) v per group; ``dead`` [nk] bool: keys that do not exist (their rows may hold anything);
    computed on ``device`` in chunks of groups and, unless ``keep``, brought back to the CPU"""
    G, nq, nk, hd = q.shape[:-2], q.shape[-2], k.shape[-2], q.shape[-1]
    q, k, v = (t.reshape(-1, t.shape[-2], hd).to(device) for t in (q, k, v))
    if dead is not None:
        dead = dead.to(device)
        k, v = k.masked_fill(dead[:, None], 0.0), v.masked_fill(dead[:, None], 0.0)
    out = torch.empty(q.shape[0], nq, hd, dtype=torch.float64, device=device)
    for i in range(0, q.shape[0], chunk):
        lg = q[i:i + chunk].double() @ k[i:i + chunk].double().transpose(-1, -2) * factor
        if dead is not None:
            lg = lg.masked_fill(dead, float("-inf"))
        out[i:i + chunk] = torch.softmax(lg, -1) @ v[i:i + chunk].double()
    out = out.reshape(*G, nq, hd)
    return out if keep else out.cpu()


def logit_stats(q, k, factor, dead=None, pi=None, device="cpu", chunk=32):
    """fp64 logits of the live keys -> dict(lo, hi) and, with ``pi``, others = the largest per-row sum of the NON-matching
    weights relative to the match (the match masked out of the sum: ``sum - 1`` would only report the fp64 epsilon), match = the
    largest match logit, gap = the smallest distance from the match to the next logit"""
    nq, nk, hd = q.shape[-2], k.shape[-2], q.shape[-1]
    q, k = q.reshape(-1, nq, hd).to(device), k.reshape(-1, nk, hd).to(device)
    pi = None if pi is None else pi.reshape(-1, nq).to(device)
    if dead is not None:
        dead = dead.to(device)
        k = k.masked_fill(dead[:, None], 0.0)
    st = dict(lo=float("inf"), hi=float("-inf"), others=0.0, match=float("-inf"), gap=float("inf"))
    for i in range(0, q.shape[0], chunk):
        lg = q[i:i + chunk].double() @ k[i:i + chunk].double().transpose(-1, -2) * factor
        if dead is not None:
            lg = lg.masked_fill(dead, float("nan"))
        live = lg[~torch.isnan(lg)]
        st["lo"], st["hi"] = min(st["lo"], live.min().item()), max(st["hi"], live.max().item())
        if pi is not None:
            lg = torch.nan_to_num(lg, nan=float("-inf"))
            match = torch.gather(lg, -1, pi[i:i + chunk, :, None])
            rest = lg.scatter(-1, pi[i:i + chunk, :, None], float("-inf"))
            st["others"] = max(st["others"], torch.exp(rest - match).sum(-1).max().item())
            st["match"] = max(st["match"], match.max().item())
            if nk > 1 and torch.isfinite(rest).any():
                st["gap"] = min(st["gap"], (match - rest.max(-1, keepdim=True).values).min().item())
    return st


def _make(form, G, nq, nk, hd, seed, dead, scale, device):
    """-> q, k, v (fp16, as the kernel receives them: q rounded after the fold for the prescaled form), expect, pi, stats"""
    from mofa_video_amd.ops import Q_FOLD_LOG2E
    factor = hd ** -0.5 if scale is None else scale
    live = [j for j in range(nk) if dead is None or not bool(dead[j])]
    if form in ("A", "B"):
        q, k, v = (_family_A if form == "A" else _family_B)(G, nq, nk, hd, seed)
        st = logit_stats(q, k, factor, dead, device=device)
        if form == "B":
            st["range"] = b_logit_range(math.prod(G) * nq * len(live))
            assert st["range"][0] <= st["lo"] and st["hi"] <= st["range"][1], ("family B logits out of range", st)
        return q, k, v, attention64(q, k, v, factor, dead, device=device), None, st
    for attempt in range(8):                                         # a draw that misses the precondition is re-seeded
        q, k, v, pi = _family_C(G, nq, nk, hd, seed + 7919 * attempt, live)
        if form == "C-prescaled":                                    # the caller's fold, one fp16 rounding; logits = q' . k * ln 2
            q, factor = (q.float() * (hd ** -0.5 * Q_FOLD_LOG2E)).half(), LN2
        st = logit_stats(q, k, factor, dead, pi, device=device)
        if st["others"] < C_OTHERS_MAX and st["match"] <= C_MATCH_LOGIT_MAX:
            expect = torch.gather(v, -2, pi[..., None].expand(*G, nq, hd))
            return q, k, v, expect, pi, st
    raise AssertionError(f"family C precondition not met in 8 draws: {st}")


# ---------------------------------------------------------------------------------------------------------------------------
# spatial
# ---------------------------------------------------------------------------------------------------------------------------
def _pack_spatial(t):                     # [frames, heads, S, hd] -> [frames * S, heads * hd]
    F_, H, S, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(F_ * S, H * hd).contiguous()


def _spatial_data(form, S, hd, heads, frames, seed=3, device="cpu"):
    q, k, v, expect, pi, st = _make(form, (frames, heads), S, S, hd, seed, None, None, device)
    return types.SimpleNamespace(q=_pack_spatial(q), k=_pack_spatial(k), v=_pack_spatial(v), expect=_pack_spatial(expect), pi=pi,
                                 stats=st, where=lambda row, col: f"frame {row // S} query {row % S} head {col // hd} d {col % hd}"
                                 + (f" (matches key {int(pi[row // S, col // hd, row % S])})" if pi is not None else ""))


# matrix shapes: built once, shared by the instantiations.  13 lengths x 2 head_dims x 4 forms = 104 entries hold the whole table
spatial_data = functools.lru_cache(maxsize=128)(_spatial_data)


def spatial_case(hd, qb, S, heads, frames, form, big=False, device="cpu"):
    """``big``: the data (tens of MB) is built per use, its reference on ``device``, and not kept"""
    def data():
        return _spatial_data(form, S, hd, heads, frames, device=device) if big else spatial_data(form, S, hd, heads, frames)

    def build():
        d, Cc = case.data(), heads * hd
        kw = dict(q=guard(d.q, ld=Cc + 24), k=guard(d.k, ld=Cc + 40), v=guard(d.v, ld=Cc + 56), nframes=frames, heads=heads, S=S,
                  head_dim=hd, out=guard(shape=(frames * S, Cc), ld=Cc + 72))
        if qb:
            kw["query_blocks"] = qb
        if form == "C-prescaled":
            kw["prescaled"] = True
        return kw
    case = Case(f"spatial/hd{hd}-qb{qb}-S{S}-h{heads}-f{frames}-{form}", "attn_spatial", build,
                "exact" if form.startswith("C") else "attn_spatial")
    case.data, case.form, case.S, case.hd, case.big = (functools.lru_cache(maxsize=1)(data) if big else data), form, S, hd, big
    return case


def spatial_shapes():
    """[(S, heads, frames)]: (heads, frames) cycled over the sequence lengths"""
    return [(S,) + HEADS_FRAMES[i % len(HEADS_FRAMES)] for i, S in enumerate(SPATIAL_S)]


def spatial_work_counts(qb):
    """workgroup count nqb * heads * frames of every table shape for 128 * qb query rows per workgroup (launch_attn_spatial)"""
    return [-(-S // (128 * qb)) * heads * frames for S, heads, frames in spatial_shapes()]


def assert_spatial_table():
    """the table holds what it is there for.  Per instantiation: S < 32, 64 +- 1, the workgroup height +- 1 and a ragged
    multi-tile S; work counts below 8, equal to 8, a larger multiple of 8, and above 8 with a remainder.  The remainders
    1 ... 7 of the deal over the 8 XCDs are all met only over the table as a whole, not by every instantiation: with the
    issue's thirteen lengths and six (heads, frames) pairs <64,2> reaches 0 ... 6 and never 7"""
    rems = set()
    for hd, qb in SPATIAL_INST:
        wg, S = 128 * qb, set(SPATIAL_S)
        assert min(S) == 1 and any(1 < s < 32 for s in S) and {63, 64, 65, wg - 1, wg + 1} <= S, (hd, qb)
        assert any(s > wg and s % 64 and s % 2 for s in S) and any(s > 2 * wg and s % 64 for s in S), (hd, qb)
        tot = spatial_work_counts(qb)
        assert any(t < 8 for t in tot) and 8 in tot and any(t > 8 and t % 8 == 0 for t in tot), (hd, qb, tot)
        assert any(t > 8 and t % 8 for t in tot), (hd, qb, tot)
        assert len({t % 8 for t in tot}) >= 6, (hd, qb, tot)          # ... and most of them per instantiation
        rems |= {t % 8 for t in tot}
    assert rems >= set(range(8)), rems
    # the auto-dispatch pair straddles the launcher's rule cdiv(S, 256) * 256 * 16 <= 17 * S at >= 1024 workgroups
    for S, two in zip(AUTO_S, (False, True)):
        nqb2 = -(-S // 256)
        assert (nqb2 * 256 * 16 <= 17 * S and nqb2 * AUTO_HEADS * AUTO_FRAMES >= 1024) == two, S


# ---------------------------------------------------------------------------------------------------------------------------
# temporal
# ---------------------------------------------------------------------------------------------------------------------------
def _pack_temporal(t):                    # [clips, HW, heads, n, hd] -> rows (clip, frame, pixel), columns (head, d)
    c, HW, H, n, hd = t.shape
    return t.permute(0, 3, 1, 2, 4).reshape(c * n * HW, H * hd).contiguous()


def temporal_masks(T):
    """{kind: (key_mask or None, live keys)}: every key; bit 0 clear; exactly one key; every other key; and for T < 32 the last
    two again with every bit >= T set, which the launcher must clear"""
    allk, high = list(range(T)), (0xffffffff << T) & 0xffffffff
    word = lambda live: sum(1 << j for j in live)
    m = {"full": (None, allk), "one": (word([2 * T // 3]), [2 * T // 3])}
    if T >= 2:
        m["no0"] = (word(allk[1:]), allk[1:])
        m["alt"] = (word(allk[1::2]), allk[1::2])
    if T < 32:
        m["one-high"] = (m["one"][0] | high, m["one"][1])
        if T >= 2:
            m["alt-high"] = (m["alt"][0] | high, m["alt"][1])
    return m


def temporal_tqs(T):
    return sorted({tq for tq in (T, 1, T - 1) if tq >= 1}, reverse=True)


def temporal_geom(T, hd):
    return TEMPORAL_GEOM[(TEMPORAL_T.index(T) + TEMPORAL_HD.index(hd)) % len(TEMPORAL_GEOM)]


@functools.lru_cache(maxsize=256)          # one (head_dim, T) has at most 3 Tq x (1 + 5 masks x 2 fills) x 4 forms = 132 entries
def temporal_data(form, T, Tq, hd, HW, heads, clips, mask, fill, seed=3):
    key_mask, live = temporal_masks(T)[mask]
    dead = torch.tensor([j not in live for j in range(T)]) if len(live) < T else None
    scale = 1.125 * hd ** -0.5 if form == "C-scale" else None
    q, k, v, expect, pi, st = _make("C" if form == "C-scale" else form, (clips, HW, heads), Tq, T, hd, seed, dead, scale, "cpu")
    if dead is not None:                  # the rows of key frames that do not exist: never-written memory, or finite decoys
        if fill == "nan":
            k[..., dead, :], v[..., dead, :] = NAN, NAN
        else:                             # the same pixel's query times 8 (it would win the softmax) with a value of 1000
            for j in torch.nonzero(dead).flatten().tolist():
                k[..., j, :], v[..., j, :] = 8 * q[..., j % Tq, :], 1000.0
    return types.SimpleNamespace(
        q=_pack_temporal(q), k=_pack_temporal(k), v=_pack_temporal(v), expect=_pack_temporal(expect), pi=pi, stats=st,
        key_mask=key_mask, scale=scale, live=live,
        where=lambda row, col: f"clip {row // (Tq * HW)} query frame {row // HW % Tq} pixel {row % HW} head {col // hd} d {col % hd}"
        + (f" (matches key {int(pi[row // (Tq * HW), row % HW, col // hd, row // HW % Tq])})" if pi is not None else ""))


def temporal_case(hd, T, Tq, form, mask="full", fill="nan"):
    HW, heads, clips = temporal_geom(T, hd)

    def data():
        return temporal_data(form, T, Tq, hd, HW, heads, clips, mask, fill if mask != "full" else "nan")

    def build():
        d, Cc = data(), heads * hd
        kw = dict(q=guard(d.q, ld=Cc + 24), k=guard(d.k, ld=Cc + 40), v=guard(d.v, ld=Cc + 40), nclips=clips, T=T, HW=HW, heads=heads,
                  head_dim=hd, out=guard(shape=(clips * Tq * HW, Cc), ld=Cc + 56))
        if Tq != T:
            kw["Tq"] = Tq
        if d.key_mask is not None:
            kw["key_mask"] = d.key_mask
        if d.scale is not None:
            kw["scale"] = d.scale
        return kw
    case = Case(f"temporal/hd{hd}-T{T}-Tq{Tq}-{mask}-{fill if mask != 'full' else 'nofill'}-{form}", "attn_temporal", build,
                "exact" if form.startswith("C") else ("attn_temporal" if mask == "full" else "attn_temporal_masked"))
    case.data, case.form, case.T, case.hd, case.mask, case.big = data, form, T, hd, mask, False
    return case


def temporal_cases(hd, T, forms=TEMPORAL_FORMS):
    """every (Tq, mask, fill, form) of one (head_dim, T)"""
    out = []
    for Tq in temporal_tqs(T):
        for mask in temporal_masks(T):
            for fill in (FILLS if mask != "full" else FILLS[:1]):
                out += [temporal_case(hd, T, Tq, form, mask, fill) for form in forms]
    return out


def assert_temporal_table():
    assert {1, 15, 16, 17, 31, 32} <= set(TEMPORAL_T)
    for hd, wpb in ((64, 4), (128, 2)):   # waves (= sequences) per workgroup of attn_temporal_kernel
        for T in TEMPORAL_T:
            HW, heads, clips = temporal_geom(T, hd)
            assert (clips * HW * heads) % wpb, (hd, T)                # a partial last workgroup
            assert {"full", "one"} <= set(temporal_masks(T)) and (T < 2 or {"no0", "alt"} <= set(temporal_masks(T)))
            assert T == 32 or any(k.endswith("-high") for k in temporal_masks(T))
            assert T < 3 or any(tq < T for tq in temporal_tqs(T))
        assert any(temporal_geom(T, hd)[2] > 1 and T > 2 for T in TEMPORAL_T), hd      # Tq < T with more than one clip


def release():
    """drop the cached data and references; the two test files call it when their last test is done"""
    spatial_data.cache_clear()
    temporal_data.cache_clear()


# ---------------------------------------------------------------------------------------------------------------------------
# the checks, the same for the stand-in, the kernels and the mutants
# ---------------------------------------------------------------------------------------------------------------------------
def check_output(case, out):
    """-> (worst err / bound; inf for a failed equality, [messages])"""
    d = case.data()
    out, errs = out.detach().cpu(), []
    if out.shape != d.expect.shape:
        return float("inf"), [f"{case.id}: shape {tuple(out.shape)} != {tuple(d.expect.shape)}"]
    nonfinite = ~torch.isfinite(out.float())
    if nonfinite.any():
        r, c = torch.nonzero(nonfinite)[0].tolist()
        errs.append(f"{case.id}: {int(nonfinite.sum())} non-finite outputs, first at [{r}, {c}] = {d.where(r, c)}")
    if case.tol == "exact":
        bad = ~(out == d.expect)                                     # by value (-0 == 0); a NaN is unequal to everything
        if bad.any():
            r, c = torch.nonzero(bad)[0].tolist()
            errs.append(f"{case.id}: {int(bad.sum())} / {bad.numel()} elements differ from v[pi] ({int(bad.any(1).sum())} rows), first at "
                        f"[{r}, {c}] = {d.where(r, c)}: got {out[r, c].item()!r}, expected {d.expect[r, c].item()!r}")
        return (float("inf") if errs else 0.0), errs
    if errs:
        return float("inf"), errs
    worst, msg = close_errors(out, d.expect, TOL[case.tol], case.id)
    if msg is not None:
        bound = TOL[case.tol] * (d.expect.abs().max() + d.expect.abs())
        r, c = divmod(int(((out.double() - d.expect).abs() / bound).argmax()), out.shape[1])
        errs.append(f"{msg}; worst err / bound {worst:.2f} at [{r}, {c}] = {d.where(r, c)}")
    return worst, errs


def check_run(case, r):
    """guards intact and read-only arguments unchanged, the result is the ``out`` buffer, no non-finite output, then the
    family's comparison"""
    errs = list(r.guard_errors())
    if r.ret is not r.placed["out"].t:
        errs.append(f"{case.id}: the call does not return its out buffer")
    worst, e = check_output(case, r.placed["out"].t)
    return worst, errs + e


# ---------------------------------------------------------------------------------------------------------------------------
# mutants: fp64 attention with one defect each, in the signature of the op, so they go through op_cases.run like the real thing
# ---------------------------------------------------------------------------------------------------------------------------
SPATIAL_MUTANTS = ("phantom", "drop-last", "mask-late", "swap-v")
TEMPORAL_MUTANTS = SPATIAL_MUTANTS + ("mask-shift",)


def _softmax_pv(lg, V, defect, n, tile, swap):
    """logits [..., nq, n], values [..., n, hd] of the n real keys in order; the kernel's key tile holds ``tile`` rows"""
    if defect == "phantom" or (defect == "mask-late" and n % tile):  # key n: a zero-filled LDS row, score 0, value 0
        lg = torch.cat([lg, torch.zeros_like(lg[..., :1])], -1)
        V = torch.cat([V, torch.zeros_like(V[..., :1, :])], -2)
    elif defect == "drop-last":
        lg, V = lg[..., :-1], V[..., :-1, :]
    elif defect == "swap-v" and swap[0] != swap[1]:                  # two keys of one tile, on the V side only
        V = V.clone()
        V[..., list(swap), :] = V[..., list(swap[::-1]), :]
    return torch.softmax(lg, -1) @ V


def mutant_differs(defect, n, tile=64):
    """does the defect change the mathematics at n real keys?  Where it does not the mutant is asserted EQUAL to the truth"""
    return {None: False, "phantom": True, "drop-last": n > 1, "mask-late": n % tile != 0, "swap-v": n > 1}[defect]


def spatial_swap(S):
    return (0, min(S - 1, 37))           # both inside key tile 0


def wrong_spatial(defect):
    """``defect`` None: the plain fp64 truth"""
    def attn_spatial(q, k, v, nframes, heads, S, head_dim=64, scale=None, out=None, prescaled=False, query_blocks=0):
        factor = LN2 if prescaled else (head_dim ** -0.5 if scale is None else scale)
        Q, K, V = (t.double().reshape(nframes, S, heads, head_dim).permute(0, 2, 1, 3) for t in (q, k, v))
        o = _softmax_pv(Q @ K.transpose(-1, -2) * factor, V, defect, S, 64, spatial_swap(S))
        out[:] = _pack_spatial(o).half()
        return out
    return types.SimpleNamespace(attn_spatial=attn_spatial)


def shifted_mask(key_mask, T):
    return ((0xffffffff if key_mask is None else key_mask) << 1) & ((1 << T) - 1)


def wrong_temporal(defect):
    """the first four act on the live keys in order (the kernel's 32-row tile holds all T frames, masked ones included, so
    "one position late" unmasks row T); mask-shift reads the mask one bit off and with it rows it must not read"""
    def attn_temporal(q, k, v, nclips, T, HW, heads, head_dim=64, scale=None, out=None, Tq=None, key_mask=None):
        Tq = T if Tq is None else Tq
        mask = (0xffffffff if key_mask is None else key_mask) & ((1 << T) - 1)
        if defect == "mask-shift":
            mask = shifted_mask(key_mask, T)
        live = [j for j in range(T) if (mask >> j) & 1]
        Q = q.double().reshape(nclips, Tq, HW, heads, head_dim).permute(0, 2, 3, 1, 4)
        K, V = (t.double().reshape(nclips, T, HW, heads, head_dim).permute(0, 2, 3, 1, 4)[..., live, :] for t in (k, v))
        late = "phantom" if (defect == "mask-late" and T < 32) else None
        o = _softmax_pv(Q @ K.transpose(-1, -2) * (head_dim ** -0.5 if scale is None else scale), V,
                        late or (defect if defect not in ("mask-late", "mask-shift") else None), len(live), 32,
                        (0, min(len(live) - 1, 9)))
        out[:] = _pack_temporal(o).half()
        return out
    return types.SimpleNamespace(attn_temporal=attn_temporal)
