"""TEST INFRASTRUCTURE ONLY: the case table of the normalisation kernels of csrc/norm.hip -- ``layer_norm`` (the four instantiations
of ``layernorm_kernel``, plain and with a row vector) and ``group_norm`` (``gn_partial`` + ``gn_apply`` and, past
``ops.GN_FUSED_MAX_ENTRIES``, ``gn_finalize`` + ``affine_act``) -- with their fp64 references, per-element bounds and the "wrong
kernel" mutants that prove the checks can fail.

Built on tests/op_cases.py and tests/aux_cases.py: a case is an ``aux_cases.AuxCase``; every fp16 argument is a guarded view (NaN
rows before and after, 8 NaN columns on the left, a leading dimension of its own), the row vector lies between NaN rows of an fp32
buffer, ``out=`` starts as NaN.  ``op_cases.run`` takes a case through ``mofa_video_amd.ops`` on the GPU
(tests/test_norm_matrix_gpu.py) and through ``impl(defect)`` on the CPU (tests/test_norm_cases_cpu.py); ``check_run`` compares
with the fp64 reference computed from the very tensors the call received (``aux_cases.check_want`` per output; the ``big`` cases
in row chunks).

The bounds are derived from the kernels' arithmetic, never measured (u16 = 2^-11, u32 = 2^-24: half an ulp of fp16 / fp32, first
order in u32 unless said otherwise).  Every output is ONE conversion of an fp32 value y32 to fp16, so

    |out - ref| <= u16 |ref| + 2^-25 + B32,      B32 >= |y32 - ref|,

and wherever no fp16 rounding tie lies within B32 of ref, out == round16(ref) bit for bit (``Want.exact``, asserted too).

LayerNorm, instantiation <MAXIT, LPR> (``ln_inst``), v = x (+ row vector), m = mean, n = (v - m) rstd, ref = n gamma + beta:
  sum      8 MAXIT sequential adds per lane (the first onto 0 is exact), log2 LPR shuffle levels: Ds = 8 MAXIT - 1 + log2 LPR
           roundings at most on the way of any term; mean = fl(fl(1 / C) sum): 2 more.  |dm| <= (Ds + 2) u32 mean|v|
  variance d = fl(v - m^): d^ - d = -dm + u32 |d|.  Two passes: sum d dm = 0, so dm enters sum d^2 only as C dm^2 (kept, second
           order); the roundings of d: 2 u32 relative; the fma chain: Dq = 8 MAXIT + log2 LPR; times fl(1 / C): 2; plus eps: 1.
           E = Dq + 5 + dm^2 / ((var + eps) u32) relative error of the argument of rsqrtf, in u32
  rstd     rsqrtf: 1 ulp = 2 u32 relative assumed -- the maximum error the HIP math API documentation states for rsqrtf, and the
           accuracy the CDNA ISA guide gives V_RSQ_F32.  e_r = E / 2 + 2
  output   fl(d^ rstd^) and the fma: t - n = -dm rstd + n (e_r + 2 u32), plus u32 |ref| <= u32 (|ref - beta| + |beta|)
  B32 = u32 (a |ref - beta| + b |gamma| rstd mean|v| + c |beta|),   a = E / 2 + 5,  b = Ds + 2,  c = 1
  row vector: v^ = fl(x + r) is off by u32 |v| <= u32 (|d| + mean|v|): a + 1 and b + 1 directly, b + 1 through the mean, and
           2 u32 sum |d||v| / sum d^2 <= 2 kappa u32 in the variance, kappa = sqrt((var + m^2) / (var + eps)): E + 2 kappa

GroupNorm: the partial sums are fp32, everything between them and scale / shift is fp64 (taken as exact):
  depth    D = rows per thread (rows per chunk / row lanes, rounded up) + row lanes (the LDS tree, sequential) + channels per
           group + passes over the columns (``gn_depth``): |dS| <= D u32 sum|x|, |dQ| <= D u32 sum x^2
  variance var = Q / cnt - mean^2: |dvar| <= D u32 (E[x^2] + 2 |m| mean|x|); K = (E[x^2] + 2 |m| mean|x|) / (var + eps)
           <= 3 (1 + m^2 / var) is the conditioning the one-pass form brings; rho = K D u32, rstd off by rho / (2 (1 - rho))
           (never by more than eps^-1/2 in all: the kernel clamps var^ at 0) and by its rounding to fp32: e_r
  scale    s^ = fl(rstd^ gamma): e_r + u32.  m^ = fl32(mean): D u32 mean|x| + u32 |m|.  shift = fl(beta - fl(m^ s^)):
           u32 |m s| + u32 (|beta| + |m s|).  y32 = fma(x, s^, shift^): u32 |y|
  B32y = u32 (a |y - beta| + |gamma| rstd (D mean|x| + 3 |m|) + 2 |beta|),   a = e_r / u32 + 3  (+ 1: products of the above)
  SiLU     z = y rcp(1 + exp2(-log2e y)): the product in front of the exponential and the constant's rounding 2 u32 |y| relative,
           the hardware exp2 and rcp one ulp = 2 u32 each (as aux_cases takes the hardware exp), the sum and the product one
           each; |silu'| <= 1.1:   B32 = 1.1 B32y + (2 |y| + 6) u32 |z|

Launch geometry that the cases are built around (written out again in ``ln_inst`` / ``ln_launch`` / ``gn_nchunks`` /
``gn_rows_per_wg``; tests/test_norm_cases_cpu.py asserts which class every case reaches): at most SLOTS_MAX = 256 CUs x 8
workgroups of 256 threads are resident, so M = 2 * 2048 * GROUPS + GROUPS + 5 rows make ``nrr`` >= 2 whatever the occupancy,
2304 frames make one gn_apply workgroup per frame, and 64 frames of 1000 rows make rows_per_wg >= 32 with a ragged last chunk."""
import math
import types

import numpy as np
import torch

import aux_cases as ac
import op_cases as oc
from aux_cases import F64, U16, U32, AuxCase, Want, round16
from op_cases import F16, F32, NAN, View, guard

SLOTS_MAX = 2048                 # 256 CUs x 8 workgroups of 256 threads: the most a 256-thread kernel can have resident
RSQRT_ULP = 1                    # assumed maximum error of rsqrtf (module docstring)
LN_WIDTHS = (8, 72, 320, 376, 384, 392, 640, 648, 1280)
LN_BIG_WIDTHS = (64, 8, 392, 648)
GN_WIDTHS = (32, 96, 160, 224, 960, 1920, 2048, 2080, 2560, 4096)
GN_HW = (1, 15, 16, 17, 145)
GN_FUSED_MAX_ENTRIES = 512       # ops.GN_FUSED_MAX_ENTRIES (asserted equal on the CPU)

MUTANTS = ("ln-mean-drops-tail-vector", "ln-var-counts-padding", "ln-one-pass-var", "ln-unbiased", "ln-rv-rounded", "ln-rv-no-mod",
           "ln-rv-div-after-mod", "ln-skip-last-pass", "gn-straddle-dropped", "gn-count-per-frame", "gn-set-of-frame",
           "gn-walk-no-carry", "gn-last-chunk", "gn-silu-first")


# ---------------------------------------------------------------------------------------------------------------------------
# the dispatch rules of csrc/norm.hip, written out
# ---------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def ln_inst(C):
    """(MAXIT, LPR) of the layernorm_kernel instantiation that mofa_layernorm_f16 launches for C channels"""
    CV = C // 8
    if CV <= 40 and CV % 8 == 0:
        return 5, 8
    if CV <= 48:
        return 3, 16
    if CV <= 80:
        return 5, 16
    return 10, 16


def ln_groups(C):
    return 256 // ln_inst(C)[1]


def ln_launch(M, C, slots=SLOTS_MAX):
    """(nrr, grid) of launch_layernorm with ``slots`` resident workgroups"""
    passes = cdiv(M, ln_groups(C))
    nrr = cdiv(passes, slots)
    return nrr, cdiv(passes, nrr)


def ln_big_rows(C):
    return 2 * SLOTS_MAX * ln_groups(C) + ln_groups(C) + 5


def gn_nchunks(HW):
    n = cdiv(HW, 576) if HW >= 9216 else cdiv(HW, 144)
    return max(1, min(n, 128 if HW >= 9216 else 16))


def gn_partial_geom(HW, C):
    """gn_partial_kernel: (column threads, row lanes, passes over the columns, rows per chunk, chunks)"""
    CV = C // 8
    cols = min(CV, 256)
    nch = gn_nchunks(HW)
    return cols, 256 // cols, cdiv(CV, 256), cdiv(HW, nch), nch


def gn_depth(HW, C):
    cols, rl, passes, rpc, _ = gn_partial_geom(HW, C)
    return cdiv(rpc, rl) + rl + C // 32 + passes


def gn_walk(C):
    """(drow, dcv) of gn_apply_kernel's division-free row walk"""
    CV = C // 8
    return 256 // CV, 256 - (256 // CV) * CV


def gn_rows_per_wg(HW, C, nframes, n_cu=256, wg_per_cu=8):
    """gn_apply_rows_per_wg for a device of ``n_cu`` CUs holding ``wg_per_cu`` workgroups of the kernel each"""
    slots = n_cu * wg_per_cu
    by_lds = 163840 // (C * 8 + 8704)
    chunks = (n_cu * max(by_lds, 1) if by_lds < wg_per_cu else slots) // nframes
    return max(16, cdiv(HW, max(chunks, 1)))


def gn_straddles(C):
    """a group holds channels on both sides of the 2048-channel pass boundary of gn_partial"""
    return C > 2048 and 2048 % (C // 32) != 0


def gn_walk_written(nrows, CV, carry=True):
    """mask [nrows, CV] of the vectors the row walk of one workgroup reaches; ``carry`` False: without the ++row on column wrap, every
    thread taking as many steps as the right walk does (vector tid + 256 k < nrows * CV) -- left to end by ``row < nrows`` the broken
    walk is only late where 256 / CV >= 1 (the lanes that fell a row behind pick up the rest) and never ends beyond 256 vectors a row"""
    tid = np.arange(256)
    row, drow = tid // CV, 256 // CV
    cv, dcv = tid - row * CV, 256 - drow * CV
    written = np.zeros((nrows, CV), dtype=bool)
    for k in range(cdiv(nrows * CV, 256)):
        act = (row < nrows) & (tid + 256 * k < nrows * CV)
        written[row[act], cv[act]] = True
        cv, row = cv + dcv, row + drow
        wrap = cv >= CV
        cv[wrap] -= CV
        if carry:
            row[wrap] += 1
    return torch.from_numpy(written)


def gn_written(nframes, HW, C, carry):
    """mask [HW, C] of what the workgroups of gn_apply write of ONE frame when the call has ``nframes`` (SLOTS_MAX device)"""
    rpw, CV = gn_rows_per_wg(HW, C, nframes), C // 8
    return torch.cat([gn_walk_written(min(rpw, HW - r0), CV, carry) for r0 in range(0, HW, rpw)]).repeat_interleave(8, dim=1)


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references (``defect``: one of MUTANTS) and bounds
# ---------------------------------------------------------------------------------------------------------------------------
def rv_index(rows, rv_div, rv_mod, defect=None):
    if defect == "ln-rv-no-mod":
        return rows // rv_div
    if defect == "ln-rv-div-after-mod":
        return (rows % rv_mod) // rv_div
    return (rows // rv_div) % rv_mod


def ln_ref(x, gamma, beta, eps, rowvec=None, rv_div=1, rv_mod=1, r0=0, defect=None):
    """rows r0 .. of the call: x fp16 [m, C] -> (ref fp64 [m, C], statistics of the rows for ``ln_bound``)"""
    v = x.double()
    m_, C = v.shape
    MAXIT, LPR = ln_inst(C)
    CV = C // 8
    if rowvec is not None:
        idx = rv_index(torch.arange(r0, r0 + m_), rv_div, rv_mod, defect)
        table = torch.cat([rowvec.double(), torch.full((1, C), NAN, dtype=F64)])    # beyond the rv_mod rows lies the NaN guard
        v = v + table[idx.clamp(max=rv_mod)]
        if defect == "ln-rv-rounded":
            v = round16(v).double()
    mean = v.mean(1, keepdim=True)
    if defect == "ln-mean-drops-tail-vector" and CV % LPR:
        mean = v[:, :CV // LPR * LPR * 8].sum(1, keepdim=True) / C
    d = v - mean
    var = (d * d).mean(1, keepdim=True)
    if defect == "ln-var-counts-padding":
        var = var + (MAXIT * LPR - CV) * 8 * mean * mean / C
    elif defect == "ln-unbiased":
        var = (d * d).sum(1, keepdim=True) / (C - 1)
    elif defect == "ln-one-pass-var":
        v32 = v.float()
        m32 = v32.sum(1, keepdim=True) * torch.tensor(1.0 / C)
        var = ((v32 * v32).sum(1, keepdim=True) * torch.tensor(1.0 / C) - m32 * m32).clamp(min=0).double()
    rstd = 1.0 / torch.sqrt(var + eps)
    ref = d * rstd * gamma.double() + beta.double()
    return ref, dict(mean=mean, var=var, rstd=rstd, mav=v.abs().mean(1, keepdim=True))


def ln_bound32(ref, st, gamma, beta, eps, rv):
    """B32 of the module docstring"""
    C = ref.shape[1]
    MAXIT, LPR = ln_inst(C)
    lg = int(math.log2(LPR))
    Ds, Dq = 8 * MAXIT - 1 + lg, 8 * MAXIT + lg
    dm = (Ds + 2 + (1 if rv else 0)) * U32 * st["mav"]
    E = Dq + 5 + dm * dm / ((st["var"] + eps) * U32)
    if rv:
        E = E + 2 * torch.sqrt((st["var"] + st["mean"] ** 2) / (st["var"] + eps))
    a = E / 2 + 2 * RSQRT_ULP + 3 + (1 if rv else 0)
    b = Ds + 2 + (2 if rv else 0)
    g, bt = gamma.double().abs(), beta.double().abs()
    return U32 * (a * (ref - beta.double()).abs() + b * g * st["rstd"] * st["mav"] + bt)


def tie_free(ref, b32):
    """mask: no fp16 rounding tie within ``b32`` of ``ref``, so every y32 within b32 of ref converts to round16(ref)"""
    h, a = round16(ref).double().abs(), ref.abs()
    m, e = torch.frexp(h)                                            # h = m 2^e, 1/2 <= m < 1: the spacing above h is 2^(e - 11)
    ulp = torch.where(h < 2.0 ** -14, torch.full_like(h, 2.0 ** -24), torch.ldexp(torch.ones_like(h), e - 11))
    below = torch.where((m == 0.5) & (h > 2.0 ** -14), ulp / 2, ulp)  # ... and half of that below a power of two
    dist = torch.minimum((h + ulp / 2 - a).abs(), (a - (h - below / 2)).abs())
    return torch.isfinite(ref) & (dist > b32 + 1e-12)


def want16(ref, b32):
    return Want(ref=ref, bound=U16 * ref.abs() + 2.0 ** -25 + b32, exact=tie_free(ref, b32))


def gn_stats(v, nframes, HW, fps, eps, defect=None):
    """v fp64 [nframes * HW, C] -> per (frame, group) mean / var / E[x^2] / mean|x| of the frame's statistics set, each [nframes, 32]"""
    C = v.shape[1]
    cpg, nsets = C // 32, nframes // fps
    s5 = v.reshape(nsets, fps, HW, 32, cpg)
    w = torch.ones(1, 1, HW, 32, cpg, dtype=F64)
    if defect == "gn-straddle-dropped" and gn_straddles(C):
        g = 2048 // cpg
        w[:, :, :, g, 2048 - g * cpg:] = 0
    if defect == "gn-last-chunk":
        rpc = gn_partial_geom(HW, C)[3]
        w[:, :, HW // rpc * rpc:] = 0
    cnt = float((HW if defect == "gn-count-per-frame" else fps * HW) * cpg)
    if defect in ("gn-straddle-dropped", "gn-last-chunk", "gn-count-per-frame"):
        mean = (s5 * w).sum((1, 2, 4)) / cnt
        var = ((s5 * s5 * w).sum((1, 2, 4)) / cnt - mean * mean).clamp(min=0)
    else:
        mean = s5.mean((1, 2, 4))
        var = ((s5 - mean[:, None, None, :, None]) ** 2).mean((1, 2, 4))
    ex2, mav = (s5 * s5).mean((1, 2, 4)), s5.abs().mean((1, 2, 4))
    frames = torch.arange(nframes)
    of = frames % nsets if defect == "gn-set-of-frame" else frames // fps
    return {k: t[of] for k, t in dict(mean=mean, var=var, ex2=ex2, mav=mav).items()}


def silu64(y):
    return y * torch.sigmoid(y)


def gn_ref(x, gamma, beta, nframes, HW, eps, fps=1, silu=False, defect=None):
    """x fp16 [nframes * HW, C] -> (ref fp64, (y before the activation, statistics per element) for ``gn_bound32``)"""
    v = x.double()
    C = v.shape[1]
    cpg = C // 32
    st = gn_stats(v, nframes, HW, fps, eps, defect)
    el = {k: t.repeat_interleave(cpg, dim=1).repeat_interleave(HW, dim=0) for k, t in st.items()}      # [nframes * HW, C]
    rstd = 1.0 / torch.sqrt(el["var"] + eps)
    src = silu64(v) if (silu and defect == "gn-silu-first") else v
    y = (src - el["mean"]) * rstd * gamma.double() + beta.double()
    el["rstd"] = rstd
    return (silu64(y) if silu and defect != "gn-silu-first" else y), (y, el)


def gn_bound32(y, el, gamma, beta, HW, eps, silu):
    D = gn_depth(HW, y.shape[1])
    m = el["mean"].abs()
    rho = (el["ex2"] + 2 * m * el["mav"]) / (el["var"] + eps) * D * U32
    cap = 1.0 / (math.sqrt(eps) * el["rstd"])                        # var^ >= 0 is clamped: rstd^ lies in (0, eps^-1/2] whatever rho
    e_r = torch.where(rho < 1, torch.minimum(rho / (2 * (1 - rho).clamp(min=1e-300)), cap), cap) / U32 + 1
    g, bt = gamma.double().abs(), beta.double().abs()
    by = U32 * ((e_r + 4) * (y - beta.double()).abs() + g * el["rstd"] * (D * el["mav"] + 3 * m) + 2 * bt)
    return 1.1 * by + (2 * y.abs() + 6) * U32 * silu64(y).abs() if silu else by


# ---------------------------------------------------------------------------------------------------------------------------
# the references behind the signatures of mofa_video_amd.ops: impl(None) is a correct implementation, impl(defect) a wrong one
# ---------------------------------------------------------------------------------------------------------------------------
def impl(defect=None):
    def _put(out, y, written=None):
        if out is None:
            out = torch.full(tuple(y.shape), NAN, dtype=F16)                # (a fresh output: what is left unwritten shows)
        dst = out[:, :y.shape[1]]
        if written is None:
            dst.copy_(y)
        else:
            dst[written] = y[written]
        return out

    def layer_norm(x, gamma, beta, eps=1e-5, rowvec=None, rv_div=1, rv_mod=1, out=None):
        M, C = x.shape
        y = torch.cat([round16(ln_ref(x[r0:r0 + 8192], gamma, beta, eps, rowvec, rv_div, rv_mod, r0, defect)[0]) for r0 in range(0, M, 8192)])
        written = None
        nrr = ln_launch(M, C)[0]
        if defect == "ln-skip-last-pass" and nrr >= 2:
            written = ((torch.arange(M) // ln_groups(C)) % nrr != nrr - 1)[:, None].expand(M, C)
        return _put(out, y, written)

    def group_norm(x, gamma, beta, nframes, HW, eps, frames_per_stat=1, silu=False, out=None, C_=None):
        C = C_ if C_ is not None else x.shape[1]
        y = round16(gn_ref(x[:, :C], gamma, beta, nframes, HW, eps, frames_per_stat, silu, defect)[0])
        fused = frames_per_stat * gn_nchunks(HW) <= GN_FUSED_MAX_ENTRIES
        return _put(out, y, gn_written(nframes, HW, C, False).repeat(nframes, 1) if defect == "gn-walk-no-carry" and fused else None)
    return types.SimpleNamespace(layer_norm=layer_norm, group_norm=group_norm)


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _channel_affine(C, seed):
    """(mean, scale) per channel: a value read from the wrong channel is off by far more than any bound"""
    g = _gen(seed)
    return torch.randn(C, generator=g) * 0.5, 0.5 + 1.5 * torch.rand(C, generator=g)


def _ln_data(family, M, C, seed, big=False):
    g = _gen(seed)
    if family == "gauss":
        cm, cs = _channel_affine(C, seed + 1)
        if big:                                                      # a random block tiled, the per-row shift makes every row its own
            blk = torch.randn(257, C, generator=g) * cs + cm
            return (blk.repeat(cdiv(M, 257), 1)[:M] + ((torch.arange(M) % 89).float() / 16 - 2.75)[:, None]).half()
        return (torch.randn(M, C, generator=g) * cs + cm + torch.randn(M, 1, generator=g)).half()
    if family == "offset":                                           # mean 40, std 1
        return (torch.randn(M, C, generator=g) + 40.0).half()
    if family == "const":                                            # variance 0; every row another constant on the 1 / 8 grid
        return (torch.randint(-24, 25, (M, 1), generator=g).float() / 8).expand(M, C).half().contiguous()
    assert family == "exact"                                         # rows of m +- d: m on the 1 / 4 grid, d a power of two, C / 2 of each sign
    m = torch.randint(-16, 17, (M, 1), generator=g).float() / 4
    d = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (M, 1), generator=g)]
    sign = torch.stack([torch.cat([torch.ones(C // 2), -torch.ones(C // 2)])[torch.randperm(C, generator=g)] for _ in range(M)])
    return (m + sign * d).half()


def _rowvec_view(rv_mod, C, seed):
    """fp32 [rv_mod, C] between NaN rows; values that fp16 cannot hold"""
    base = torch.full((2 + rv_mod + 1, C), NAN, dtype=F32)
    base[2:2 + rv_mod] = torch.randn(rv_mod, C, generator=_gen(seed)) * 0.5 + 2.0 ** -13
    return View(base, lambda b: b[2:2 + rv_mod])


def _eps_tag(eps):
    return "" if eps == 1e-5 else f"-eps{eps:g}"


def _ln_case(C, M, family="gauss", rv=None, eps=1e-5, seed=0, big=False):
    """rv: None or (rv_div, rv_mod)"""
    rows = (1, 1) if big else (3, 2)

    def build():
        kw = dict(x=guard(_ln_data(family, M, C, seed, big), ld=C + 24, rows=rows), gamma=oc._f(C, seed=seed + 2), beta=oc._f(C, seed=seed + 3),
                  eps=eps, out=guard(shape=(M, C), ld=C + 40, rows=rows))
        if rv is not None:
            kw.update(rowvec=_rowvec_view(rv[1], C, seed + 4), rv_div=rv[0], rv_mod=rv[1])
        return kw

    def ref_rows(kw, r0, r1):
        args = (kw["gamma"], kw["beta"], eps, kw.get("rowvec"), kw.get("rv_div", 1), kw.get("rv_mod", 1))
        ref, st = ln_ref(kw["x"][r0:r1], *args, r0=r0)
        b32 = ln_bound32(ref, st, kw["gamma"], kw["beta"], eps, rv is not None)
        w = want16(ref, b32)
        if family == "const" and rv is None and C & (C - 1) == 0:     # sum, 1 / C and so d = 0 are exact: the result IS fl16(beta)
            w.exact = torch.ones_like(w.exact)
        return w
    tag = f"layer_norm/C{C}-M{M}-{family}" + (f"-rv{rv[0]}x{rv[1]}" if rv else "") + _eps_tag(eps)
    c = AuxCase(tag, "layer_norm", build, lambda kw: [ref_rows(kw, 0, M)], big=big, C=C, M=M, family=family, rv=rv, eps=eps)
    c.ref_rows = ref_rows
    return c


def _gn_data(family, nframes, HW, C, seed):
    g = _gen(seed)
    if family == "gauss":
        cm, cs = _channel_affine(C, seed + 1)
        fs = torch.randn(nframes, 1, 1, generator=g)
        return ((torch.randn(nframes, HW, C, generator=g) * cs + cm + fs).reshape(nframes * HW, C)).half()
    assert family == "exact"                                         # per (frame, group) m +- d: m on the 1 / 4 grid, d a power of two
    cpg = C // 32
    m = torch.randint(-16, 17, (nframes, 1, 32, 1), generator=g).float() / 4
    d = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (nframes, 1, 32, 1), generator=g)]
    sign = torch.randint(0, 2, (nframes, HW, 32, cpg), generator=g).float() * 2 - 1
    return (m + sign * d).reshape(nframes * HW, C).half()


def _gn_case(C, HW, frames, fps=1, silu=False, family="gauss", xw=None, out_extra=0, eps=1e-5, seed=0, tag=None):
    M = frames * HW

    def build():
        x = _gn_data(family, frames, HW, C, seed)
        if xw:                                                       # columns beyond C_ belong to x but not to the call: other numbers
            x = torch.cat([x, oc._h(M, xw - C, seed=seed + 5, scale=3.0)], 1)
        kw = dict(x=guard(x, ld=(xw or C) + 24), gamma=oc._f(C, seed=seed + 2), beta=oc._f(C, seed=seed + 3), nframes=frames, HW=HW, eps=eps,
                  frames_per_stat=fps, silu=silu, out=guard(shape=(M, C + out_extra), ld=C + out_extra + 48))
        if xw:
            kw["C_"] = C
        return kw

    def ref(kw):
        r, (y, el) = gn_ref(kw["x"][:, :C], kw["gamma"], kw["beta"], frames, HW, eps, fps, silu)
        w = want16(r, gn_bound32(y, el, kw["gamma"], kw["beta"], HW, eps, silu))
        return [w]
    name = tag or (f"C{C}-HW{HW}-f{frames}-fps{fps}" + ("-silu" if silu else "") + ("" if family == "gauss" else f"-{family}")
                   + (f"-xw{xw}-out+{out_extra}" if xw else "") + _eps_tag(eps))
    return AuxCase("group_norm/" + name, "group_norm", build, ref, C=C, HW=HW, frames=frames, fps=fps, silu=silu, family=family, xw=xw,
                   out_extra=out_extra)


ROWS_PER_CHECK = 8192


def check_run(case, r):
    """as ``aux_cases.check_run``: guards, then the one output against the reference -- ``ROWS_PER_CHECK`` rows at a time (the
    ``big`` cases), and the columns of a wider ``out`` beyond C bit-unchanged"""
    errs, worst = list(r.guard_errors()), 0.0
    kw, ((label, g, before),) = ac.inputs_of(r), r.outputs()
    what, C, M = f"{case.id} {label}", case.meta["C"], g.shape[0]
    if g.shape[1] > C:
        if before is None or not oc.same_bits(g[:, C:], before[:, C:]):
            errs.append(f"{what}: columns beyond the result's {C} were written")
        g = g[:, :C]
    rows = getattr(case, "ref_rows", None)
    ac.OFF_ROUNDING.pop(what, None)
    for r0 in range(0, M, ROWS_PER_CHECK) if rows else (0,):
        r1 = min(r0 + ROWS_PER_CHECK, M) if rows else M
        wo, e = ac.check_want(what, g[r0:r1], rows(kw, r0, r1) if rows else case.ref(kw)[0], accumulate=True)
        worst, errs = max(worst, wo), errs + (e if len(errs) < 8 else [])
    return worst, errs


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
def _rv_of(kind, M):
    return {"1x1": (1, 1), "7x5": (7, 5), "M+3x2": (M + 3, 2)}[kind]


def _ln_cases():
    out = []
    for i, C in enumerate(LN_WIDTHS):
        G = ln_groups(C)
        for j, M in enumerate((1, G - 1, G, G + 1, 101)):
            eps, kind = (1e-5, 1e-6)[(i + j) % 2], ("1x1", "7x5", "M+3x2")[(i + j) % 3]
            out += [_ln_case(C, M, eps=eps, seed=1000 + 10 * (5 * i + j)), _ln_case(C, M, rv=_rv_of(kind, M), eps=eps, seed=1000 + 10 * (5 * i + j))]
        out += [_ln_case(C, G + 1, "exact", seed=2000 + 10 * i), _ln_case(C, G + 1, "exact", rv=(7, 5), eps=1e-6, seed=2000 + 10 * i)]
    for k, C in enumerate((72, 320)):                                # (HW, T) = (37, 25) on two clips: the index wraps
        out += [_ln_case(C, 37 * 25 * 2, seed=2200 + 10 * k), _ln_case(C, 37 * 25 * 2, rv=(37, 25), seed=2200 + 10 * k)]
    for k, C in enumerate((8, 320)):
        out += [_ln_case(C, ln_groups(C) + 1, "const", eps=(1e-5, 1e-6)[k], seed=2300 + 10 * k),
                _ln_case(C, ln_groups(C) + 1, "const", rv=(1, 1), eps=(1e-5, 1e-6)[k], seed=2300 + 10 * k)]
    for k, C in enumerate((640, 1280)):
        out += [_ln_case(C, 101, "offset", seed=2400 + 10 * k), _ln_case(C, 101, "offset", rv=(7, 5), seed=2400 + 10 * k)]
    for k, C in enumerate(LN_BIG_WIDTHS):
        M = ln_big_rows(C)
        out += [_ln_case(C, M, seed=2500 + 10 * k, big=True), _ln_case(C, M, rv=(7, 5), eps=1e-6, seed=2500 + 10 * k, big=True)]
    return out


def _gn_cases():
    out = []
    for i, C in enumerate(GN_WIDTHS):
        three = 0
        for j, HW in enumerate(GN_HW):
            frames = (1, 3)[(i + j) % 2]
            fps = 1
            if frames == 3:
                fps, three = (3, 1)[three % 2], three + 1
            out.append(_gn_case(C, HW, frames, fps, silu=(j + i // 2) % 2 == 0, eps=(1e-5, 1e-6)[j % 2], seed=3000 + 10 * (5 * i + j)))
    out += [
        _gn_case(32, 24, 2304, tag="one-workgroup-per-frame-f2304-HW24-C32", seed=3600),
        _gn_case(32, 1000, 64, silu=True, tag="ragged-last-chunk-f64-HW1000-C32", seed=3610),
        _gn_case(160, 17, 6, fps=3, silu=True, seed=3620),           # two statistics sets of three frames
        _gn_case(32, 2304, 33, fps=33, tag="split-path-f33-fps33-HW2304-C32", seed=3630),      # 33 * 16 entries > 512
        _gn_case(960, 17, 3, fps=3, xw=992, out_extra=16, seed=3640),
        _gn_case(2080, 17, 3, fps=1, silu=True, xw=2112, out_extra=16, seed=3650),
        _gn_case(96, 17, 3, fps=3, family="exact", seed=3660),
        _gn_case(2080, 145, 1, silu=True, family="exact", seed=3670),
    ]
    return out


CASES = _ln_cases() + _gn_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
OPS = ("layer_norm", "group_norm")


def mutant_differs(defect, case):
    """from the geometry alone: True = the wrong kernel ``defect`` must fail on ``case``, False = it computes the same there,
    None = it differs by roundings only and may or may not show"""
    m = case.meta
    if case.op != ("layer_norm" if defect.startswith("ln-") else "group_norm"):
        return False
    if case.op == "layer_norm":
        C, M, rv = m["C"], m["M"], m["rv"]
        MAXIT, LPR = ln_inst(C)
        CV = C // 8
        if defect == "ln-mean-drops-tail-vector":
            return CV % LPR != 0
        if m["family"] == "const" and rv is None:                    # d = 0 whatever the variance: only a wrong mean shows
            return CV % LPR != 0 if defect == "ln-mean-drops-tail-vector" else False if defect != "ln-one-pass-var" else None
        if defect == "ln-var-counts-padding":
            return MAXIT * LPR != CV
        if defect == "ln-one-pass-var":
            return True if m["family"] == "offset" else None
        if defect == "ln-unbiased":
            return True
        if defect == "ln-rv-rounded":                                # moves every v by up to 2^-11 |v|: a quarter of the elements cross a tie
            return False if rv is None else True if M * C >= 2048 else None
        if defect == "ln-rv-no-mod":
            return rv is not None and (M - 1) // rv[0] >= rv[1]
        if defect == "ln-rv-div-after-mod":
            return rv is not None and bool((rv_index(torch.arange(M), *rv) != rv_index(torch.arange(M), *rv, defect)).any())
        if defect == "ln-skip-last-pass":
            return ln_launch(M, C)[0] >= 2
    else:
        C, HW, frames, fps = m["C"], m["HW"], m["frames"], m["fps"]
        if defect == "gn-straddle-dropped":
            return gn_straddles(C)
        if defect == "gn-count-per-frame":
            return fps > 1
        if defect == "gn-set-of-frame":
            return fps > 1 and frames // fps > 1
        if defect == "gn-walk-no-carry":
            return fps * gn_nchunks(HW) <= GN_FUSED_MAX_ENTRIES and not bool(gn_written(frames, HW, C, False).all())
        if defect == "gn-last-chunk":
            return HW % gn_partial_geom(HW, C)[3] != 0
        if defect == "gn-silu-first":
            return m["silu"]
    raise KeyError(defect)


# ---------------------------------------------------------------------------------------------------------------------------
# argument lists that every norm entry point of the C ABI must reject without a launch (tests/test_norm_cases_cpu.py on host
# buffers, tests/test_norm_matrix_gpu.py on device buffers)
# ---------------------------------------------------------------------------------------------------------------------------
MOFA_EINVAL = -22


def edge_buffers(device):
    """(x, y, part, gamma, beta, scale, shift, rowvec, sums): NaN-filled"""
    # sized for the largest reading of any argument list below, so that nothing could write out of bounds even where a check were
    # missing: 2 frames of 16 rows (32 LayerNorm rows) of up to 4128 channels at ld 4160, 4097 partial entries, 2 x 4128 scales
    x = torch.full((40, 4160), NAN, dtype=F16, device=device)
    y = torch.full((40, 4160), NAN, dtype=F16, device=device)
    part = torch.full((4200 * 64,), NAN, dtype=F32, device=device)
    g = torch.full((4160,), NAN, dtype=F32, device=device)
    b = torch.full((4160,), NAN, dtype=F32, device=device)
    sc = torch.full((2 * 4160,), NAN, dtype=F32, device=device)
    sh = torch.full((2 * 4160,), NAN, dtype=F32, device=device)
    rv = torch.full((8, 4160), NAN, dtype=F32, device=device)
    sums = torch.full((2 * 64,), NAN, dtype=torch.float64, device=device)
    return x, y, part, g, b, sc, sh, rv, sums


def edge_calls(lib, ptrs, st):
    """{name: call -> return code}; ``ptrs``: the data pointers of ``edge_buffers``"""
    X, Y, P, G, B, SC, SH, RV, SU = ptrs

    def ln(C=320, ldx=4160, ldy=4160, rowvec=0, rv_div=1, rv_mod=1):
        return lib.mofa_layernorm_f16(X, G, B, Y, 32, C, ldx, ldy, 1e-5, rowvec, rv_div, rv_mod, st)

    def partial(C=64, HW=16, ldx=4160):
        return lib.mofa_gn_partial_f16(X, P, 2, HW, C, ldx, st)

    def finalize(C=64, HW=16, nframes=2, fps=1):
        return lib.mofa_gn_finalize(P, G, B, SC, SH, nframes, HW, C, fps, 1e-5, st)

    def reduce(C=64, HW=16, nframes=2, fps=1):
        return lib.mofa_gn_reduce(P, SU, nframes, HW, C, fps, st)

    def finalize_sums(C=64, nframes=2, fps=1, count=32.0):
        return lib.mofa_gn_finalize_sums(SU, G, B, SC, SH, nframes, C, fps, count, 1e-5, st)

    def apply(C=64, HW=16, nframes=2, fps=1, ldx=4160, ldy=4160):
        return lib.mofa_gn_apply_f16(X, P, G, B, Y, nframes, HW, C, ldx, ldy, fps, 1e-5, 0, st)

    def gathered(C=64, HW=16, nentries=2, count=64.0, ldx=4160, ldy=4160):
        return lib.mofa_gn_apply_gathered_f16(X, P, nentries, count, G, B, Y, 2, HW, C, ldx, ldy, 1e-5, 0, st)

    def affine(C=64, HW=16, ldx=4160, ldy=4160):
        return lib.mofa_affine_act_f16(X, SC, SH, Y, 2, HW, C, ldx, ldy, 0, st)

    def from_stats(C=64, HW=64):
        return lib.mofa_gn_partial_from_stats(SC, P, 2, HW, C, st)
    calls = {
        "layernorm C % 8": lambda: ln(C=12), "layernorm C 1288": lambda: ln(C=1288), "layernorm C 0": lambda: ln(C=0),
        "layernorm C -8": lambda: ln(C=-8), "layernorm ldx % 8": lambda: ln(ldx=4156), "layernorm ldy % 8": lambda: ln(ldy=4156),
        "layernorm rv_div 0": lambda: ln(rowvec=RV, rv_div=0, rv_mod=3), "layernorm rv_mod 0": lambda: ln(rowvec=RV, rv_div=3, rv_mod=0),
        "layernorm rv_div -1": lambda: ln(rowvec=RV, rv_div=-1, rv_mod=3),
    }
    gn = dict(partial=partial, finalize=finalize, reduce=reduce, finalize_sums=finalize_sums, apply=apply, gathered=gathered, affine=affine,
              from_stats=from_stats)
    for name, fn in gn.items():
        for C in (0, -32) + ((40,) if name != "affine" else (-8, 12)):               # (affine_act takes any C % 8 == 0)
            calls[f"gn {name} C {C}"] = lambda fn=fn, C=C: fn(C=C)
    for name in ("partial", "apply", "gathered", "from_stats"):                     # the entry points that stage C channels in LDS
        calls[f"gn {name} C 4128"] = lambda fn=gn[name]: fn(C=4128)
    for name in ("finalize", "reduce", "finalize_sums", "apply"):
        calls[f"gn {name} nframes % frames_per_stat"] = lambda fn=gn[name]: fn(nframes=2, fps=3)
        calls[f"gn {name} frames_per_stat 0"] = lambda fn=gn[name]: fn(nframes=2, fps=0)
    for name in ("partial", "finalize", "reduce", "apply", "gathered", "affine", "from_stats"):
        calls[f"gn {name} HW 0"] = lambda fn=gn[name]: fn(HW=0)
    calls.update({
        "gn gathered nentries 0": lambda: gathered(nentries=0), "gn gathered nentries 4097": lambda: gathered(nentries=4097),
        "gn gathered count_per_group 0": lambda: gathered(count=0.0), "gn finalize_sums count_per_group 0": lambda: finalize_sums(count=0.0),
        "gn partial ldx % 8": lambda: partial(ldx=4156), "gn apply ldy % 8": lambda: apply(ldy=4156), "gn affine ldx % 8": lambda: affine(ldx=4156),
        "gn from_stats HW % 64": lambda: from_stats(HW=32),
    })
    return calls
