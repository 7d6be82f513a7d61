"""TEST INFRASTRUCTURE ONLY: the case table of the VAE mid-block attention -- ``softmax_rows_``, ``transpose_v`` and the composed
``vae.mid_attention_core`` (per frame: ``igemm`` with s_acc = 1 / sqrt(C) -> ``softmax_rows_`` -> ``igemm`` on the frame's slice of
``transpose_v``) -- with the fp64 references, the per-element bounds and the "wrong kernel" mutants that prove the checks can fail.

Built like tests/aux_cases.py on tests/op_cases.py (guarded views, ``op_cases.run`` through ``mofa_video_amd.ops`` on the GPU --
tests/test_vae_attn_gpu.py -- and through ``impl(defect)`` on the CPU -- tests/test_vae_attn_cases_cpu.py --, ``check_run`` against
``case.ref`` computed from the call's own arguments).  u16 = 2^-11, u32 = 2^-24; the bounds are derived, never measured.

softmax_rows_ (csrc/attention.hip: 256 threads per row, passes of 2048 columns -- a thread takes 8 adjacent columns per pass --,
fp32 maximum, exp(x - max) summed per thread, 6-level wave sum, the four wave sums added, one reciprocal, exp(x - max) * inv
rounded once to fp16):
  constant rows    at 0, +65504, -65504: every exponential is exactly 1, the fp32 sum is the integer cols, every output is
                   round16(fl32(1 / cols)): bit-equal
  one-hot rows     one entry 0, the rest -inf: exactly 1 and exactly 0: bit-equal.  The hot column at 0, at the last column, at
                   column 2048 (the first of the second pass) and inside the ragged last pass
  bounded          Gaussian logits x 3 and x 12; "tail" rows -- one maximum, the rest at max - d, d on a grid over [8, 20] row
                   by row: the outputs run through the fp16 subnormal range down to the exact-zero threshold 2^-25, and
                   subnormal results must be right, not flushed.  With d_i = max - x_i, dbar = sum p_j d_j:
                       |out - p_i| <= u16 p_i + 2^-25 + [(1.5 d_i + 4) + (1.5 dbar + 4) + cols / 256 + 12] u32 p_i
                   u16 p + 2^-25: the output rounding, normal and subnormal.  (1.5 d_i + 4) u32: the term exp(-d_i) -- the
                   rounding of d * log2(e) in front of the hardware exp2 and that exp2, the ``flow_expectation`` argument of
                   tests/aux_cases.py.  (1.5 dbar + 4) u32: the same errors in the sum, weighted by the terms' shares.
                   cols / 256: the serial sum of a thread (cols / 256 terms).  12: the wave tree (6), the three adds over the
                   waves, the reciprocal, the product, one for the second-order terms
  OFF_ROUNDING     (``aux_cases.OFF_ROUNDING``) the share of elements that are not the fp64 softmax rounded once

transpose_v: family P of tests/step_cases.py (exact in fp16, pairwise distinct inside a 64 x 64 window, other values in the next
frame, column block and key block): bit-equal.  ``v`` is a column block at column 72 of a wider guarded buffer.

mid_attention_core (3 frames; q, k, v guarded views of distinct leading dimensions):
  uniform          Q = 0, V integers in [-8, 8], S a power of two: every probability is 2^-log2(S), the fp32 products and sums
                   are exact, row i of frame f is the mean of frame f's V rows, |sum| <= 8 S <= 1024 < 2048: representable,
                   bit-equal.  Catches a frame that reads another frame's V
  one-hot          S == C, k_j = 16 e_sig_f(j), q_i = 16 e_sig_f(pi_f(i)) with other permutations per frame: scores 256 / sqrt(C) >= 22.6 at
                   the match and 0 elsewhere; off the match p = e^-22.6 / (1 + ..) = 1.5e-10 < 2^-25 rounds to exactly 0, at
                   the match 1 - 127 * 1.5e-10 rounds to exactly 1: o_i = v_pi_f(i) bit for bit.  Catches wrong K slices, a
                   wrong scale, a wrong transpose
  Gaussian         q, k ~ N(0, 1) * sqrt(2) (|s| reaches about 8), v ~ N(0, 1); against fp64 attention on the fp16 inputs with
                   exact scores:  |o - ref| <= u16 |o| + 2^-25 + sum_j [1.05 p_ij (delta_ij + dbar_i) + u16 p_ij + 2^-25] |v_jc|,
                   delta_ij = 0.51 ulp16(s_ij) -- the fp16 storage of the scores, a rounding tipped by the fp32 accumulation
                   included --, dbar_i = sum_j p_ij delta_ij (its effect on the normaliser); 1.05: e^delta - 1 <= 1.002 delta
                   for delta <= 2^-8 and the softmax's own fp32 errors; u16 p_ij + 2^-25: the fp16 storage of the probability

Mutants (``mutant_differs``: where each computes something else; elsewhere it must EQUAL the truth).  A softmax does not change
when all logits of a row are shifted, so a wrong or missing shift shows only where fp32 overflows or underflows:
  no-max-sub         no maximum subtracted                            rows of +-65504: exp overflows / every term underflows
  max-first-pass     maximum over the first pass only                 one-hot rows with the hot column >= 2048: the running
                                                                      maximum stays at its start value, the hot term overflows
  ragged-pass-drop   ragged last pass left out of the sum             cols % 2048 != 0
  one-wave-sum       normalised by wave 0's partial sum               cols > 512 (wave 0 holds columns [0, 512) of every pass)
  flush-subnormal    subnormal outputs flushed to zero                some output is a non-zero fp16 subnormal (from the reference)
  frame-stride       frame f of v sought at row f (S - 8)             nframes > 1
  cb-stride          column block cb sought at column 32 cb           ncb > 1
  ragged-key-drop    ragged last key block not written                S % 64 != 0
  dk-swapped         (d, key) exchanged inside a 64 x 64 block        every transpose_v case
  k-frame0           every frame scores against frame 0's K           Gaussian and one-hot families (uniform: Q = 0)
  vt-frame0          every frame multiplies frame 0's V^T             every family
  no-s-acc           scores not scaled                                Gaussian (one-hot stays one-hot, uniform stays 0)
  scale-1/C          scores scaled by 1 / C                           Gaussian and one-hot"""
import math
import types

import torch

import aux_cases as ac
import step_cases as sc
from aux_cases import U16, U32, Want, round16, ulp16
from op_cases import F16, F32, NAN, _h, _ints, guard

F64 = torch.float64
INF = float("inf")
PASS = 2048
SOFTMAX_COLS = (8, 520, 2040, 2048, 2056, 4104, 9216)
SOFTMAX_ROWS = (1, 33)
TV_S, TV_NCB, TV_FRAMES = (8, 56, 64, 72, 200), (1, 3, 8), (1, 3)
CORE_SHAPES = ((64, 64), (128, 128), (192, 64))
CORE_FRAMES = 3
SOFTMAX_MUTANTS = ("no-max-sub", "max-first-pass", "ragged-pass-drop", "one-wave-sum", "flush-subnormal")
TV_MUTANTS = ("frame-stride", "cb-stride", "ragged-key-drop", "dk-swapped")
CORE_MUTANTS = ("k-frame0", "vt-frame0", "no-s-acc", "scale-1/C")
MUTANTS = SOFTMAX_MUTANTS + TV_MUTANTS + CORE_MUTANTS
MUTANT_OPS = dict([(m, ("softmax_rows_",)) for m in SOFTMAX_MUTANTS] + [(m, ("transpose_v",)) for m in TV_MUTANTS]
                  + [(m, ("mid_attention_core",)) for m in CORE_MUTANTS])
EXP_OVER, EXP_UNDER = 88.72, -103.97                 # fp32: exp overflows above / is zero below


# ---------------------------------------------------------------------------------------------------------------------------
# softmax_rows_
# ---------------------------------------------------------------------------------------------------------------------------
def hot_columns(rows, cols):
    """the hot / maximum column of every row: 0, the last, 2048, inside the ragged last pass -- in turn; a single row takes the
    ragged last pass (the last column where there is none)"""
    ragged = cols - 4 if cols % PASS else cols - 1                # (of the last pass's 8-column vectors the last: thread (cols % 2048) / 8 - 1)
    turn = [0, cols - 1, min(PASS, cols - 1), ragged]
    return [ragged] if rows == 1 else [turn[r % 4] for r in range(rows)]


def softmax_ref(x64, defect=None):
    """fp64 [rows, cols] -> (p, d = max - x)"""
    mx = x64.max(1, keepdim=True).values
    d = mx - x64
    p = torch.softmax(x64, 1)
    rows, cols = x64.shape
    col = torch.arange(cols)
    if defect == "no-max-sub":
        bad = (mx[:, 0] > EXP_OVER) | (mx[:, 0] < EXP_UNDER)         # inf / inf, or 0 * (1 / 0)
        p = torch.where(bad[:, None], torch.full_like(p, NAN), p)
    elif defect == "max-first-pass":
        mx1 = x64[:, :PASS].max(1, keepdim=True).values.clamp(min=-1e30)
        bad = ((x64 - mx1) > EXP_OVER).any(1)
        p = torch.where(bad[:, None], torch.full_like(p, NAN), p)
    elif defect in ("ragged-pass-drop", "one-wave-sum"):
        keep = col < cols // PASS * PASS if defect == "ragged-pass-drop" else (col % PASS) < 512
        if defect == "ragged-pass-drop" and cols % PASS == 0:
            keep = torch.ones(cols, dtype=torch.bool)
        e = torch.exp(-d)
        with_nan = e / (e * keep[None, :]).sum(1, keepdim=True)      # a zero sum: inf at the non-zero terms, NaN at the zeros
        p = torch.where(keep.all(), p, with_nan)
    elif defect == "flush-subnormal":
        p = torch.where(round16(p).double().abs() < 2.0 ** -14, torch.zeros_like(p), p)
    return p, d


def softmax_bound(p, d, cols):
    dbar = (p * torch.where(p > 0, d, torch.zeros_like(d))).sum(1, keepdim=True)
    return U16 * p + 2.0 ** -25 + ((1.5 * d + 4) + (1.5 * dbar + 4) + cols / 256 + 12) * U32 * p


def _softmax_data(family, rows, cols, seed):
    hot = hot_columns(rows, cols)
    if family == "const":
        x = torch.tensor([0.0, 65504.0, -65504.0])[torch.arange(rows) % 3][:, None].expand(rows, cols).half().contiguous()
        one = torch.ones(cols, dtype=F32)
        assert float(one.sum()) == cols and float(torch.tensor(float(cols), dtype=F32)) == cols       # the sum is exact
        return x
    if family == "onehot":
        x = torch.full((rows, cols), -INF, dtype=F16)
        x[torch.arange(rows), hot] = 0.0
        return x
    if family.startswith("gauss"):
        x = _h(rows, cols, seed=seed, scale=float(family[5:]))
        top = x.float().amax(1) + 1.0                               # the row maximum where the table wants it
        x[torch.arange(rows), hot] = top.half()
        return x
    assert family == "tail"
    dgrid = 8.0 + 12.0 * torch.arange(rows) / max(rows - 1, 1) if rows > 1 else torch.tensor([14.0])
    x = (4.0 - dgrid)[:, None].expand(rows, cols).half().contiguous()
    x[torch.arange(rows), hot] = 4.0
    return x


SOFTMAX_FAMILIES = ("const", "onehot", "gauss3", "gauss12", "tail")


def _softmax_case(family, rows, cols, padded, seed):
    def build():
        x = _softmax_data(family, rows, cols, seed)
        return dict(x=guard(x, ld=cols + 8 + 24) if padded else guard(x, ld=cols, col=0))

    def ref(kw):
        x64 = kw["x"].double()
        if family == "const":
            inv = (torch.tensor(1.0, dtype=F32) / torch.tensor(float(cols), dtype=F32)).half()
            return [Want(bits=inv.expand(rows, cols).contiguous())]
        p, d = softmax_ref(x64)
        if family == "onehot":
            return [Want(bits=p.half())]
        return [Want(ref=p, bound=softmax_bound(p, d, cols))]
    tag = f"softmax_rows_/{family}-{rows}x{cols}-" + ("ld+32" if padded else "ld=cols")
    return ac.AuxCase(tag, "softmax_rows_", build, ref, family=family, rows=rows, cols=cols, padded=padded)


def _softmax_cases():
    cases = []
    for i, cols in enumerate(SOFTMAX_COLS):
        for j, rows in enumerate(SOFTMAX_ROWS):
            for k, fam in enumerate(SOFTMAX_FAMILIES):
                cases.append(_softmax_case(fam, rows, cols, bool((i + j + k) % 2), 700 + 10 * i + j))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------
# transpose_v
# ---------------------------------------------------------------------------------------------------------------------------
def tv_ref(v, nframes, ncb, S, defect=None):
    """v [nframes*S, ncb*64] -> [nframes*ncb*64, S] (pure data movement; a mutant's unwritten elements are NaN)"""
    C = ncb * 64
    if defect == "frame-stride" and nframes > 1:
        v = torch.stack([v[f * (S - 8):f * (S - 8) + S] for f in range(nframes)]).reshape(nframes * S, C)
    if defect == "cb-stride" and ncb > 1:
        v = torch.cat([v[:, 32 * cb:32 * cb + 64] for cb in range(ncb)], 1)
    v3 = v.reshape(nframes, S, C)
    if defect == "dk-swapped":
        out = torch.zeros((nframes, C, S), dtype=v.dtype)
        for k0 in range(0, S, 64):
            for cb in range(ncb):
                kn = min(64, S - k0)
                blk = v3[:, k0:k0 + kn, cb * 64:cb * 64 + 64]         # [f, key, d]: written as if it were [f, d, key]
                out[:, cb * 64:cb * 64 + kn, k0:k0 + kn] = blk[:, :, :kn]
        return out.reshape(nframes * C, S)
    out = v3.permute(0, 2, 1).contiguous()
    if defect == "ragged-key-drop" and S % 64:
        out[:, :, S // 64 * 64:] = NAN
    return out.reshape(nframes * C, S)


def _tv_case(S, ncb, frames):
    C = ncb * 64

    def build():
        data = sc.placement(frames, C, S).permute(0, 2, 1).reshape(frames * S, C).half()
        return dict(v=guard(data, ld=72 + C + 24, col=72), nframes=frames, ncb=ncb, S=S)

    def ref(kw):
        return [Want(bits=tv_ref(kw["v"], frames, ncb, S))]
    return ac.AuxCase(f"transpose_v/S{S}-ncb{ncb}-f{frames}", "transpose_v", build, ref, S=S, ncb=ncb, frames=frames)


# ---------------------------------------------------------------------------------------------------------------------------
# mid_attention_core
# ---------------------------------------------------------------------------------------------------------------------------
def core_ref(q, k, v, nframes, S, defect=None):
    """fp16 q, k, v [nframes*S, C] -> (fp64 o, fp64 bound): exact scores, fp64 softmax, fp64 P V"""
    C = q.shape[1]
    scale = {"no-s-acc": 1.0, "scale-1/C": 1.0 / C}.get(defect, 1.0 / math.sqrt(C))
    o, bound = [], []
    for f in range(nframes):
        rows = slice(f * S, (f + 1) * S)
        kf = k[:S] if defect == "k-frame0" else k[rows]
        vf = (v[:S] if defect == "vt-frame0" else v[rows]).double()
        s = q[rows].double() @ kf.double().T * scale
        p = torch.softmax(s, 1)
        delta = 0.51 * ulp16(round16(s))
        dbar = (p * delta).sum(1, keepdim=True)
        of = p @ vf
        o.append(of)
        bound.append(U16 * of.abs() + 2.0 ** -25 + (1.05 * p * (delta + dbar) + U16 * p + 2.0 ** -25) @ vf.abs())
    return torch.cat(o), torch.cat(bound)


def perms(S, frames, seed=900):
    return [torch.randperm(S, generator=torch.Generator().manual_seed(seed + f)) for f in range(frames)]


def _core_case(family, S, C):
    n = CORE_FRAMES
    M = n * S

    def build():
        if family == "uniform":
            assert S & (S - 1) == 0 and 8 * S < 2048                  # the mean is representable (module docstring)
            q, k, v = torch.zeros(M, C, dtype=F16), _h(M, C, seed=910), _ints(-8, 8, M, C, seed=911).half()
        elif family == "onehot":
            assert S == C and math.exp(-256 / math.sqrt(C)) < 2.0 ** -25 and (S - 1) * math.exp(-256 / math.sqrt(C)) < 2.0 ** -12
            eye = 16.0 * torch.eye(S, dtype=F16)
            sig = perms(S, n, 950)                                    # k_j = 16 e_sig_f(j), q_i = 16 e_sig_f(pi_f(i)): the match is j = pi_f(i)
            k = torch.cat([eye[sg] for sg in sig])
            q = torch.cat([eye[sg[pi]] for sg, pi in zip(sig, perms(S, n))])
            v = _h(M, C, seed=912)
        else:
            q, k, v = _h(M, C, seed=913, scale=2 ** 0.5), _h(M, C, seed=914, scale=2 ** 0.5), _h(M, C, seed=915)
        return dict(q=guard(q, ld=C + 24), k=guard(k, ld=C + 40), v=guard(v, ld=C + 56), nframes=n, S=S)

    def ref(kw):
        if family == "uniform":
            mean = kw["v"].double().reshape(n, S, C).mean(1, keepdim=True).expand(n, S, C).reshape(M, C)
            return [Want(bits=round16(mean))]
        if family == "onehot":
            return [Want(bits=torch.cat([kw["v"][f * S:(f + 1) * S][pi] for f, pi in enumerate(perms(S, n))]))]
        o, bound = core_ref(kw["q"], kw["k"], kw["v"], n, S)
        return [Want(ref=o, bound=bound)]
    return ac.AuxCase(f"mid_attention_core/{family}-S{S}-C{C}", "mid_attention_core", build, ref, family=family, S=S, C=C, frames=n)


def _core_cases():
    cases = []
    for S, C in CORE_SHAPES:
        cases.append(_core_case("gauss", S, C))
        if S & (S - 1) == 0:
            cases.append(_core_case("uniform", S, C))
        if S == C:
            cases.append(_core_case("onehot", S, C))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------
# the references behind the signatures of mofa_video_amd.ops / vae.mid_attention_core
# ---------------------------------------------------------------------------------------------------------------------------
def impl(defect=None):
    def softmax_rows_(x):
        x.copy_(round16(softmax_ref(x.double(), defect)[0]))
        return x

    def transpose_v(v, nframes, ncb, S):
        return tv_ref(v, nframes, ncb, S, defect).clone()

    def mid_attention_core(q, k, v, nframes, S):
        return round16(core_ref(q, k, v, nframes, S, defect)[0])
    return types.SimpleNamespace(**{k: v for k, v in locals().items() if callable(v) and not k.startswith("_")})


def core_module():
    """``mid_attention_core`` of mofa_video_amd.vae as an attribute, so that ``op_cases.run`` can call it by name"""
    from mofa_video_amd import vae
    return types.SimpleNamespace(mid_attention_core=vae.mid_attention_core)


CASES = (_softmax_cases() + [_tv_case(S, ncb, fr) for S in TV_S for ncb in TV_NCB for fr in TV_FRAMES] + _core_cases())
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
OPS = tuple(dict.fromkeys(c.op for c in CASES))


def has_subnormal_output(case):
    x = case.build()["x"]
    p = round16(softmax_ref(x.cut(x.base).double())[0]).double()
    return bool(((p > 0) & (p < 2.0 ** -14)).any())


def mutant_differs(defect, case):
    m = case.meta
    if case.op not in MUTANT_OPS[defect]:
        return False
    if defect == "no-max-sub":
        return m["family"] == "const" and m["rows"] > 1               # (a single row is the row of zeros)
    if defect == "max-first-pass":
        return m["family"] == "onehot" and m["cols"] > PASS
    if defect == "ragged-pass-drop":
        return m["cols"] % PASS != 0
    if defect == "one-wave-sum":           # (a one-hot row whose hot column wave 0 holds is normalised by the right sum)
        return m["cols"] > 512 and (m["family"] != "onehot" or any(h % PASS >= 512 for h in hot_columns(m["rows"], m["cols"])))
    if defect == "flush-subnormal":
        return has_subnormal_output(case)
    if defect == "frame-stride":
        return m["frames"] > 1
    if defect == "cb-stride":
        return m["ncb"] > 1
    if defect == "ragged-key-drop":
        return m["S"] % 64 != 0
    if defect in ("dk-swapped", "vt-frame0"):
        return True
    if defect == "k-frame0":
        return m["family"] != "uniform"
    if defect == "no-s-acc":
        return m["family"] == "gauss"
    if defect == "scale-1/C":
        return m["family"] in ("gauss", "onehot")
    raise KeyError(defect)


def assert_table():
    sm = [c for c in CASES if c.op == "softmax_rows_"]
    for fam in SOFTMAX_FAMILIES:
        sel = [c for c in sm if c.meta["family"] == fam]
        assert {(c.meta["rows"], c.meta["cols"]) for c in sel} == {(r, c) for r in SOFTMAX_ROWS for c in SOFTMAX_COLS}, fam
        assert {c.meta["padded"] for c in sel} == {False, True}, fam
        assert {c.meta["padded"] for c in sel if c.meta["cols"] > PASS} == {False, True}, fam
    assert all(c % 8 == 0 for c in SOFTMAX_COLS) and 9216 / PASS == 4.5
    for cols in SOFTMAX_COLS:                                         # the maximum at every position the issue names
        hot = set(hot_columns(33, cols))
        assert {0, cols - 1} <= hot and (cols <= PASS or PASS in hot)
        if cols % PASS and cols > PASS:
            assert any(cols // PASS * PASS <= h < cols - 1 for h in hot), cols
        one = hot_columns(1, cols)[0]
        assert one >= min(PASS, cols - 1) or cols < PASS
    tv = [c for c in CASES if c.op == "transpose_v"]
    assert {(c.meta["S"], c.meta["ncb"], c.meta["frames"]) for c in tv} == {(S, n, f) for S in TV_S for n in TV_NCB for f in TV_FRAMES}
    assert all(S % 8 == 0 for S in TV_S) and any(S % 64 and S > 64 for S in TV_S) and any(S < 64 for S in TV_S)
    core = [c for c in CASES if c.op == "mid_attention_core"]
    assert {(c.meta["S"], c.meta["C"]) for c in core if c.meta["family"] == "gauss"} == set(CORE_SHAPES)
    assert {(c.meta["S"], c.meta["C"]) for c in core if c.meta["family"] == "uniform"} == {(64, 64), (128, 128)}
    assert {(c.meta["S"], c.meta["C"]) for c in core if c.meta["family"] == "onehot"} == {(64, 64), (128, 128)}
    assert all(c.meta["frames"] == 3 for c in core)
