"""TEST INFRASTRUCTURE ONLY: the case table of the two hand-scheduled level-0 kernels, ``lin320`` (csrc/lin320.hip) and ``ff320``
(csrc/ff320.hip) -- exact sums, row edges, ring phases, row isolation -- with their fp64 references and the "wrong kernel"
mutants that prove the checks can fail.

Built on tests/op_cases.py: a case is an ``op_cases.Case`` whose ``build()`` gives the keyword arguments of the op, every fp16
2-D argument a guarded view (NaN rows before and after, 8 NaN columns on the left, a leading dimension larger than the width and
different for every argument of a call), every ``out=`` and ``ln_out`` buffer NaN-filled and guarded.  ``op_cases.run`` takes a
case through ``mofa_video_amd.ops`` on the GPU (tests/test_l0_matrix_gpu.py) and through tests/emu_ops.py and ``model(defect)``
on the CPU (tests/test_l0_cases_cpu.py).  ``check_run`` compares a run with the fp64 reference computed from the very tensors
the call received (the packed weights are unpacked by the layout include/mofa_hip.h documents).

The matrices (``case.matrix``):
  a  lin320 exact sums     bit-equal: N x M x the eight instances (NORM, RV, R1), thinned so that every (instance, N) and every
                           (instance, M) pair occurs
  b  lin320 ring phases    a block of P = 333 rows repeated until some workgroup processes four tiles: rows [0, P) against the
                           reference, every later repeat bit-equal to the first
  c  ff320 ring phases     the same with three tiles per workgroup
  d  ff320 row edges       M around the wave and the tile height
  e  row isolation         poisoned rows (NaN row 0, NaN row M - 1, one +inf at a wave boundary) against the clean run

Why the exact cases are exact (derived, not measured).  x = integers in [-64, 64] / 16, W = integers in [-32, 32] / 64, bias and
row vector = integers in [-8192, 8192] / 1024, r1 = integers in [-512, 512] / 64, s_acc and s1 powers of two.  Every product
x W is a multiple of 2^-10, and so is every bias and row-vector entry; |acc| <= 320 * 4 * 0.5 + 16 = 656 < 2^14, so any partial
sum is one of fewer than 2^24 multiples of 2^-10: the fp32 accumulator holds the exact value whatever the summation order, and
s_acc * acc is exact as well.  The result is therefore the literal ``round16(round16(s_acc * acc) + s1 * r1)``, each round16
one rounding of an exact value to fp16 (s1 * r1 and its sum with an fp16 value are exact in fp32).

Exact LayerNorm rows (the NORM instances): a row holds +a in 160 places and -a in the other 160, a one of {0.25, 0.5, 1, 2, 8,
64, 1024, 16384}.  Sums of at most 320 multiples of a and of a^2 are exact in fp32: mean = 0, variance = a^2, and
(x - mean) * rstd = +-1 / sqrt(1 + eps / a^2), which is within 1.6e-4 (eps <= 1e-5, a >= 0.25) of +-1 -- less than a quarter of
an fp16 ulp below 1 (2^-11): it rounds to exactly +-1.  Gains in {0.5, 1, 2} and norm biases on the 1/16 grid fold into W / bias
(weights.pack_lin320) without rounding: W' = W * gain is a multiple of 2^-7 of magnitude <= 1, W . beta a sum of multiples of
2^-10.

ff320 admits no exact grid (GELU): Gaussian data as ``op_cases._ff320_params``, the project's stated tolerances --
``oc.TOL["ff320"]`` for ``out``, ``oc.TOL["ff320_ln"]`` for ``out_ln`` against the reference, and half of ``oc.TOL["ff320"]``
(the 1.5e-3 of tests/test_ff320_gpu.py) for ``out_ln`` against the LayerNorm of the kernel's own ``out``.  One ff320 case is
exact all the same, ``ff320/d-lnround-M33``: with s_acc = 2^-30 the term f16(s_acc * FF) is zero, x = 512 + k / 2 and r2 on the
1/64 grid make s1 x + s2 r2 exact in fp32, so ``out`` is round16(x + r2) whatever the GEMMs give, with an fp16 spacing of 0.5
against a row deviation of about 1.4: a second output that normalised the UNROUNDED row is off by up to 0.25 / 1.4, far beyond
the bound, where on Gaussian rows the rounding (2^-11 relative) hides inside it."""
import types

import torch
import torch.nn.functional as F

import op_cases as oc
from aux_cases import gelu64, round16
from op_cases import F16, NAN, View, _f, _h, _ints

F64 = torch.float64
INF = float("inf")
P_ROWS = 333                                         # the period of matrices b and c: gcd(333, 256) = gcd(333, 128) = 1
LN_OWN_TOL = oc.TOL["ff320"] / 2                     # out_ln against LayerNorm(the kernel's own out): tests/test_ff320_gpu.py's figure
LIN_N = (64, 128, 192, 256, 320, 384, 960)
LIN_M = (1, 7, 8, 9, 25, 31, 32, 33, 255, 256, 257, 481, 505)
FF_M = (1, 31, 32, 33, 127, 128, 129, 225)
INSTANCES = tuple((n, v, r) for r in (0, 1) for v in (0, 1) for n in (0, 1))      # (NORM, RV, R1) in the launcher's order
LN_AMPS = (0.25, 0.5, 1.0, 2.0, 8.0, 64.0, 1024.0, 16384.0)
SCALES = ((0.5, 1.0), (1.0, 0.5), (0.25, 2.0))       # (s_acc, s1)
RV_QUIRK = (7, 3, 4, 5)
RV_ROWS = 37                                         # rows of the per-row mapping idx = m % RV_ROWS in matrix a
NO_CUS = 1 << 20                                     # "more compute units than tiles": every workgroup runs one tile

MUTANTS = ("drop-kstep", "stale-chunk-third-tile", "bias-wrong-chunk", "single-rounding", "r1-row0-straddle", "rv-row0-of-wave",
           "store-row-M", "pos-mod-T", "ln-unrounded")
MUTANT_OPS = {"drop-kstep": ("lin320",), "stale-chunk-third-tile": ("lin320", "ff320"), "bias-wrong-chunk": ("lin320",),
              "single-rounding": ("lin320",), "r1-row0-straddle": ("lin320",), "rv-row0-of-wave": ("lin320",),
              "store-row-M": ("lin320", "ff320"), "pos-mod-T": ("ff320",), "ln-unrounded": ("ff320",)}


class L0Case(oc.Case):
    """``matrix``: a .. e; ``meta``: what the mutant rules, the table invariants and the failure messages read (M, N, inst,
    data, rvmap, bias, kind, reps, cus, poison)"""

    def __init__(self, id, op, build, tol, matrix, **meta):
        super().__init__(id, op, build, tol)
        self.matrix, self.meta = matrix, meta


def guard_rep(block, reps, ld, device="cpu", rows=(3, 2), col=8):
    """``op_cases.guard`` of ``block`` repeated ``reps`` times along the rows, assembled on ``device``"""
    P, C = block.shape
    assert ld % 8 == 0 and ld >= col + C
    base = torch.full((rows[0] + reps * P + rows[1], ld), NAN, dtype=block.dtype, device=device)
    base[rows[0]:rows[0] + reps * P, col:col + C] = block.to(device).repeat(reps, 1)
    r0, r1 = rows[0], rows[0] + reps * P
    return View(base, lambda b: b[r0:r1, col:col + C])


def guard_out(M, C, ld, device="cpu", rows=(3, 2), col=8):
    base = torch.full((rows[0] + M + rows[1], ld), NAN, dtype=F16, device=device)
    r0, r1 = rows[0], rows[0] + M
    return View(base, lambda b: b[r0:r1, col:col + C])


# ---------------------------------------------------------------------------------------------------------------------------
# packed operands back to matrices, from the layouts include/mofa_hip.h documents (pure reshapes)
# ---------------------------------------------------------------------------------------------------------------------------
def unpack_lin320(wp):
    """wp [N / 64 c][2 t][20 s][64 l][8 e] -> W' [N, 320]: W'[64 c + 32 t + (l & 31)][16 s + 8 (l >> 5) + e]"""
    nch = wp.shape[0]
    return wp.reshape(nch, 2, 20, 2, 32, 8).permute(0, 1, 4, 2, 3, 5).reshape(nch * 64, 320)


def unpack_ff320(w1p, w2p):
    """w1p [40 c][2 t][20 s][64 l][8 e] -> W1g [2560, 320]: W1g[1280 t + 32 c + (l & 31)][16 s + 8 (l >> 5) + e];
    w2p [40 c][10 j][2 u][64 l][8 jj] -> W2 [320, 1280]: W2[32 j + (l & 31)][32 c + 16 u + 4 (l >> 5) + (jj & 3) + 8 (jj >> 2)]"""
    w1 = w1p.reshape(40, 2, 20, 2, 32, 8).permute(1, 0, 4, 2, 3, 5).reshape(2560, 320)
    w2 = w2p.reshape(40, 10, 2, 2, 32, 2, 4).permute(1, 4, 0, 2, 5, 3, 6).reshape(320, 1280)
    return w1, w2


# ---------------------------------------------------------------------------------------------------------------------------
# the fp64 references, straight from the formulas of include/mofa_hip.h
# ---------------------------------------------------------------------------------------------------------------------------
def layer_norm64(x64, eps):
    mean = x64.mean(1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(1, keepdim=True)
    return (x64 - mean) / torch.sqrt(var + eps)


def rv_index(M, rv):
    m = torch.arange(M)
    return ((m // rv[0]) * rv[1] + (m % rv[2])) % rv[3]


def lin320_ref(kw, rows=None):
    """-> fp64 [rows, N]: round16(s_acc * acc) + s1 * r1 BEFORE its final rounding to fp16 (``rows``: the first rows only)"""
    M = kw["x"].shape[0] if rows is None else rows
    w = unpack_lin320(kw["wp"].cpu()).double()
    N = w.shape[0]
    xh = kw["x"][:M, :320].cpu().double()
    if kw.get("norm"):
        xh = round16(layer_norm64(xh, kw.get("eps", 1e-5))).double()
    acc = xh @ w.T
    if kw.get("bias") is not None:
        acc = acc + kw["bias"].cpu().double()
    if kw.get("rowvec") is not None:
        acc = acc + kw["rowvec"].cpu().double()[rv_index(M, kw["rv"])]
    y = round16(kw.get("s_acc", 1.0) * acc).double()
    if kw.get("r1") is not None:
        y = y + kw.get("s1", 1.0) * kw["r1"][:M, :N].cpu().double()
    return y


_FF_UNPACKED = []                                    # [(w1p, w2p, W1g fp64, W2 fp64)]: the few parameter sets of the table, unpacked once


def _ff_weights(w1p, w2p):
    w1p, w2p = w1p.cpu(), w2p.cpu()
    for a, b, w1, w2 in _FF_UNPACKED:
        if torch.equal(a, w1p) and torch.equal(b, w2p):
            return w1, w2
    w1, w2 = (t.double() for t in unpack_ff320(w1p, w2p))
    _FF_UNPACKED.append((w1p, w2p, w1, w2))
    return w1, w2


def ff320_ref(kw, rows=None):
    """-> (fp64 out before its final rounding, fp64 LayerNorm(round16(out)) * gamma + beta or None)"""
    M = kw["x"].shape[0] if rows is None else rows
    w1, w2 = _ff_weights(kw["w1p"], kw["w2p"])
    xf = kw["x"][:M, :320].cpu().double()
    if kw.get("pos") is not None:
        xf = xf + kw["pos"].cpu().double()[(torch.arange(M) // kw.get("HW", 1)) % kw.get("T", 1)]
    xn = round16(layer_norm64(xf, kw.get("eps", 1e-5))).double()
    p = xn @ w1.T + kw["b1"].cpu().double()
    h = round16(p[:, :1280] * gelu64(p[:, 1280:])).double()
    y = round16(kw.get("s_acc", 1.0) * (h @ w2.T + kw["b2"].cpu().double())).double() + kw.get("s1", 1.0) * xf
    if kw.get("r2") is not None:
        y = y + kw.get("s2", 0.0) * kw["r2"][:M, :320].cpu().double()
    ln = kw.get("ln_out")
    if ln is None:
        return y, None
    return y, own_layer_norm(round16(y), ln, kw.get("ln_eps", 1e-5))


def own_layer_norm(out16, ln, ln_eps):
    """fp64 LayerNorm of an fp16 row as it stands"""
    return layer_norm64(out16.cpu().double(), ln_eps) * ln[0].cpu().double() + ln[1].cpu().double()


# ---------------------------------------------------------------------------------------------------------------------------
# where an element lives in the kernels (csrc/lin320.hip: 256-row tiles, 8 waves of 32 rows, chunks of 64 columns = two 32-column
# MFMA tiles, stores in row groups of 8; csrc/ff320.hip: 128-row tiles, 4 waves, ten 32-column output tiles)
# ---------------------------------------------------------------------------------------------------------------------------
def where(op, row, col, N=320, cus=None):
    th = 256 if op == "lin320" else 128
    tile, wave, l31 = row // th, (row % th) // 32, row % 32
    s = f"row {row} col {col}: tile {tile}"
    if cus:
        s += f" (tile {tile // cus} of workgroup {tile % cus})"
    s += f", wave {wave}, row {l31} of the wave (row group {l31 // 8}, store lane {8 * (l31 % 8) + (col % 64) // 8})"
    if op == "lin320":
        s += f", chunk {col // 64} MFMA tile {(col % 64) // 32}"
        if cus:
            s += f", ring slot g % 3 = {((tile // cus) * (N // 64) + col // 64) % 3}"
    else:
        s += f", output tile {col // 32} piece {col // 16}"
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# checking a run
# ---------------------------------------------------------------------------------------------------------------------------
def _args_of(r, rows):
    """the call's arguments as they were BEFORE the call (their first ``rows`` rows where they are token matrices), CPU"""
    def before(name):
        t = r.placed[name].before()
        return (t[:rows] if t.dim() == 2 and t.dtype == F16 and name not in ("wp", "w1p", "w2p") else t).cpu()
    kw = {}
    for k, v in r.kwargs.items():
        if k in r.placed:
            kw[k] = before(k)
        elif isinstance(v, tuple) and f"{k}[0]" in r.placed:
            kw[k] = tuple(before(f"{k}[{i}]") for i in range(len(v)))
        else:
            kw[k] = v
    return kw


def _first_bad(mask):
    return torch.nonzero(mask)[0].tolist()


def _bits_errors(case, what, got, want, cus):
    bad = oc.bits(got) != oc.bits(want)
    if not bool(bad.any()):
        return []
    i, j = _first_bad(bad)
    return [f"{case.id} {what}: {int(bad.sum())} / {bad.numel()} elements are not bit-equal, first {got[i, j].item()!r} for "
            f"{want[i, j].item()!r} at {where(case.op, i, j, case.meta.get('N', 320), cus)}"]


def _close_errors(case, what, got, ref, tol, cus):
    """the form of ``oc.close_errors``: |err| <= tol * max|ref| + tol * |ref| -> (worst err / bound, [message])"""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        i, j = _first_bad(~torch.isfinite(got))
        return INF, [f"{case.id} {what}: non-finite output, first at {where(case.op, i, j, case.meta.get('N', 320), cus)}"]
    scale = ref.abs().max().item() + 1e-12
    ratio = (got - ref).abs() / (tol * scale + tol * ref.abs())
    worst = ratio.max().item()
    if worst <= 1.0:
        return worst, []
    i, j = _first_bad(ratio > 1.0)
    return worst, [f"{case.id} {what}: {int((ratio > 1).sum())} / {ratio.numel()} elements out of tolerance {tol:g}, worst {worst:.3f} x its "
                   f"bound; first {got[i, j].item()!r} for {ref[i, j].item()!r} at {where(case.op, i, j, case.meta.get('N', 320), cus)}"]


def check_run(case, r, cus=None):
    """-> (worst err / bound: 0.0 for a bit-equal case, [messages]): guards, the returned buffers, the columns of ``out`` beyond
    the result's, rows [0, P) against the reference and, in the periodic matrices, every later repeat against the first"""
    errs = list(r.guard_errors())
    m, op = case.meta, case.op
    N, reps = m.get("N", 320), m.get("reps", 1)
    P = m["M"] // reps
    kw = _args_of(r, P)
    rets = list(r.ret) if isinstance(r.ret, (tuple, list)) else [r.ret]
    names = ["out"] + (["ln_out[2]"] if "ln_out[2]" in r.placed else [])
    if len(rets) != len(names) or any(rets[i] is not r.placed[n].t for i, n in enumerate(names)):
        return INF, errs + [f"{case.id}: the call does not return its out / ln_out buffers"]
    if op == "lin320":
        refs = [lin320_ref(kw, P)]
    else:
        refs = [x for x in ff320_ref(kw, P) if x is not None]
    worst = 0.0
    own_out = r.placed["out"].t[:P, :N].cpu()
    for name, ref in zip(names, refs):
        p = r.placed[name]
        full = p.t
        if full.shape[1] > N and not oc.same_bits(full[:, N:], p.before()[:, N:]):
            errs.append(f"{case.id} {name}: columns beyond the result's {N} were written")
        got = full[:P, :N].cpu()
        if m.get("poison"):                                          # the poisoned row: non-finite throughout, and out of the comparison
            row = m["poison"][0]
            if bool(torch.isfinite(got[row].float()).any()):
                errs.append(f"{case.id} {name}: finite values in the poisoned row {row}")
            got, ref, own_out = got.clone(), ref.clone(), own_out.clone()
            got[row], ref[row], own_out[row] = 0.0, 0.0, torch.arange(320, dtype=F16)[:own_out.shape[1]]
        if case.tol == "exact":
            e = _bits_errors(case, name, got, round16(ref), cus)
            worst = INF if e else worst
            errs += e
        else:
            tol = oc.TOL["ff320_ln" if name == "ln_out[2]" else case.tol]
            w, e = _close_errors(case, name + " against the reference", got, ref, tol, cus)
            worst, errs = max(worst, w), errs + e
            if name == "ln_out[2]" and not e:
                own = own_layer_norm(own_out, kw["ln_out"], kw.get("ln_eps", 1e-5))
                if m.get("poison"):
                    own[m["poison"][0]] = 0.0
                w, e = _close_errors(case, name + " against LayerNorm(out)", got, own, LN_OWN_TOL, cus)
                worst, errs = max(worst, w), errs + e
        if reps > 1:
            v = full[:, :N].unflatten(0, (reps, P))
            if not torch.equal(v, v[:1].expand_as(v)):
                bad = (v != v[:1]) | (torch.isnan(v) != torch.isnan(v[:1]))
                k, i, j = _first_bad(bad)
                worst = INF
                errs.append(f"{case.id} {name}: repeat {k} differs from the first in {int(bad.sum())} elements, first {v[k, i, j].item()!r} "
                            f"for {v[0, i, j].item()!r} at {where(op, k * P + i, j, N, cus)}")
    return worst, errs


def isolation_errors(case, r, clean):
    """matrix e: the run ``r`` of a poisoned case against the run ``clean`` of the same case without the poison -- every buffer
    element outside the poisoned row bit-equal (guard rows and columns included), the poisoned row non-finite throughout"""
    errs = list(r.guard_errors())
    row, N = case.meta["poison"][0], case.meta.get("N", 320)
    for name in ("out", "ln_out[2]"):
        if name not in r.placed:
            continue
        p = r.placed[name]
        r0 = int(torch.nonzero(p.inside)[0][0])
        diff = oc.bits(p.buf) != oc.bits(clean.placed[name].buf)
        diff[r0 + row] = False
        if bool(diff.any()):
            i, j = _first_bad(diff)
            errs.append(f"{case.id} {name}: {int(diff.sum())} elements outside the poisoned row {row} differ from the clean run, first at "
                        f"{where(case.op, i - r0, j - 8, N)}")
        if bool(torch.isfinite(p.t[row, :N].float()).any()):
            errs.append(f"{case.id} {name}: finite values in the poisoned row {row}")
    return errs


# ---------------------------------------------------------------------------------------------------------------------------
# the stand-ins with one defect each: model(None) IS tests/emu_ops.py (asserted bit for bit on every case)
# ---------------------------------------------------------------------------------------------------------------------------
def _store_row_m(out, width):
    """what a store that ignored M would do: the row behind the last one (a guard row of the buffer) gets numbers"""
    torch.as_strided(out, (1, width), (out.stride(0), 1), out.storage_offset() + out.shape[0] * out.stride(0))[...] = 1.0


def model(defect=None, cus=NO_CUS):
    """the CPU stand-ins of emu_ops with the structure of the kernels (tiles handed to ``cus`` workgroups round-robin, chunks,
    k-steps, waves) and one ``defect`` of MUTANTS"""
    def lin320(x, wp, bias=None, norm=False, eps=1e-5, rowvec=None, rv=(1, 1, 1, 1 << 30), r1=None, s1=1.0, s_acc=1.0, out=None):
        w = unpack_lin320(wp).float()
        N, M = w.shape[0], x.shape[0]
        nchunk = N // 64
        xf = x[:, :320].float()
        if norm:
            xf = F.layer_norm(xf, (320,), None, None, eps).to(F16).float()
        y = xf @ w.T
        m = torch.arange(M)
        if defect == "drop-kstep":                                   # k-step 7 of chunk 1 (of the only chunk at N = 64)
            c, xz = min(1, nchunk - 1), xf.clone()
            xz[:, 16 * 7:16 * 8] = 0
            y[:, 64 * c:64 * c + 64] = xz @ w[64 * c:64 * c + 64].T
        if defect == "stale-chunk-third-tile" and nchunk > 1:       # chunk 1 computed on the ring slot chunk 0 left behind
            third = (m // 256) // cus == 2
            y[third, 64:128] = xf[third] @ w[0:64].T
        if bias is not None:
            y = y + (bias.float().roll(-64) if defect == "bias-wrong-chunk" else bias.float())
        if rowvec is not None:
            mi = m // 32 * 32 if defect == "rv-row0-of-wave" else m
            idx = ((mi // rv[0]) * rv[1] + (mi % rv[2])) % rv[3]
            rows = torch.as_strided(rowvec, (int(idx.max()) + 1, N), (N, 1))
            y = y + rows.float()[idx]
        y = s_acc * y
        if defect != "single-rounding":
            y = y.to(F16).float()
        if r1 is not None:
            rr = r1[:, :N].float()
            if defect == "r1-row0-straddle":                         # the wave that straddles M: rows + 8, + 16, + 24 of a lane from row 0
                wrong = (m // 32 == (M - 1) // 32) & (m % 32 >= 8) & (M % 32 != 0)
                rr = torch.where(wrong[:, None], rr[:1], rr)
            y = y + s1 * rr
        y = y.to(F16)
        if out is None:
            return y
        out[:, :N].copy_(y)
        if defect == "store-row-M":
            _store_row_m(out, N)
        return out

    def ff320(x, w1p, b1, w2p, b2, eps=1e-5, pos=None, HW=1, T=1, r2=None, s_acc=1.0, s1=1.0, s2=0.0, out=None, ln_out=None,
              ln_eps=1e-5):
        w1, w2 = (t.float() for t in unpack_ff320(w1p, w2p))
        m = torch.arange(x.shape[0])
        xf = x[:, :320].float()
        if pos is not None:
            xf = xf + pos.float()[m % T if defect == "pos-mod-T" else (m // HW) % T]
        xn = F.layer_norm(xf, (320,), None, None, eps).to(F16).float()
        p = xn @ w1.T + b1.float()
        if defect == "stale-chunk-third-tile":                       # W1 chunk 1 (value and gate tile) on the slot chunk 0 left behind
            third = (m // 128) // cus == 2
            for t in (0, 1280):
                p[third, t + 32:t + 64] = xn[third] @ w1[t:t + 32].T + b1.float()[t + 32:t + 64]
        h = (p[:, :1280] * F.gelu(p[:, 1280:])).to(F16).float()
        y = (s_acc * (h @ w2.T + b2.float())).to(F16).float() + s1 * xf
        if r2 is not None:
            y = y + s2 * r2[:, :320].float()
        unrounded, y = y, y.to(F16)
        if out is not None:
            out[:, :320].copy_(y)
            y = out
            if defect == "store-row-M":
                _store_row_m(out, 320)
        if ln_out is None:
            return y
        src = unrounded if defect == "ln-unrounded" else y[:, :320].float()
        yl = F.layer_norm(src, (320,), ln_out[0], ln_out[1], ln_eps).to(F16)
        if len(ln_out) > 2 and ln_out[2] is not None:
            ln_out[2][:, :320].copy_(yl)
            yl = ln_out[2]
        return y, yl
    return types.SimpleNamespace(lin320=lin320, ff320=ff320)


def mutant_effect(defect, case, cus=NO_CUS):
    """from the geometry alone, what the wrong kernel ``defect`` does on ``case``: "caught" (the check must fail), "within" (it
    computes something else that the case's stated tolerance cannot tell) or "same" (it computes the same bits)"""
    m = case.meta
    if case.op not in MUTANT_OPS[defect]:
        return "same"
    M, N, reps = m["M"], m.get("N", 320), m.get("reps", 1)
    norm, rv, r1 = m.get("inst", (0, 0, 0))
    kind = m.get("kind", ())
    third_tile = -(-M // (256 if case.op == "lin320" else 128)) > 2 * cus
    if defect in ("drop-kstep", "store-row-M"):
        return "caught"
    if defect == "stale-chunk-third-tile":
        return "caught" if third_tile and (N > 64 or case.op == "ff320") else "same"
    if defect == "bias-wrong-chunk":
        return "caught" if m["bias"] and N > 64 else "same"
    if defect == "single-rounding":                                  # one rounding against two: an fp16 ulp at the most, 2^-10 relative
        return "same" if not r1 else ("caught" if case.tol == "exact" else "within")
    if defect == "r1-row0-straddle":
        return "caught" if r1 and M % 32 > 8 else "same"
    if defect == "rv-row0-of-wave":
        return "caught" if rv and M > 1 else "same"
    if defect == "pos-mod-T":
        return "caught" if "pos" in kind and m["HW"] > 1 and M > 1 else "same"
    if defect == "ln-unrounded":                                     # 2^-11 relative on Gaussian rows; 0.25 of 1.4 on the lnround case
        return "same" if "ln" not in kind else ("caught" if "lnround" in kind else "within")
    raise KeyError(defect)


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ln_exact_rows(P, seed):
    """fp16 [P, 320]: every row +a in 160 places and -a in the other 160, a of LN_AMPS per row"""
    g = _gen(seed)
    sign = torch.where(torch.rand(P, 320, generator=g).argsort(1) < 160, 1.0, -1.0)
    amp = torch.tensor(LN_AMPS)[torch.randint(0, len(LN_AMPS), (P,), generator=g)]
    amp[:min(P, len(LN_AMPS))] = torch.tensor(LN_AMPS)[:min(P, len(LN_AMPS))]      # every amplitude where there are rows for it
    return (sign * amp[:, None]).half()


def _lin_period(inst, N, P, data, rvmap, bias, seed):
    """one period of lin320 operands on the CPU: (x [P, 320], wp, bias or None, rowvec or None, rv, r1 [P, N] or None)"""
    from mofa_video_amd.weights import pack_lin320
    norm, rv_on, r1_on = inst
    g = _gen(seed)
    gamma = beta = None
    if data == "exact":
        w = _ints(-32, 32, N, 320, seed=seed + 1) / 64
        b = _ints(-8192, 8192, N, seed=seed + 2) / 1024 if bias else None
        if norm:
            x = ln_exact_rows(P, seed + 3)
            gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (320,), generator=g)]
            beta = _ints(-16, 16, 320, seed=seed + 4) / 16 if bias else None
        else:
            x = (_ints(-64, 64, P, 320, seed=seed + 3) / 16).half()
        nrv = RV_ROWS if rvmap == "row" else (P if rvmap == "period" else 5)
        rowvec = _ints(-8192, 8192, nrv, N, seed=seed + 5) / 1024 if rv_on else None
        r1 = (_ints(-512, 512, P, N, seed=seed + 6) / 64).half() if r1_on else None
    else:
        w = (torch.randn(N, 320, generator=g) * 320 ** -0.5).half()
        b = torch.randn(N, generator=g) * 0.3 if bias else None
        if norm:
            gamma, beta = 1 + 0.2 * torch.randn(320, generator=g), 0.2 * torch.randn(320, generator=g)
        x = _h(P, 320, seed=seed + 3, scale=1.2, shift=0.3)
        nrv = RV_ROWS if rvmap == "row" else (P if rvmap == "period" else 5)
        rowvec = _f(nrv, N, seed=seed + 5, scale=0.5) if rv_on else None
        r1 = _h(P, N, seed=seed + 6) if r1_on else None
    wp, bp = pack_lin320(w, b, gamma, beta)
    rv = {"row": (1 << 30, 0, RV_ROWS, 1 << 30), "period": (1 << 30, 0, P, 1 << 30), "quirk": RV_QUIRK, None: None}[rvmap]
    return x, wp, bp, rowvec, rv, r1


def _poison(x, poison):
    """poison = (row, column or None, value): a whole row (column None) or one element of x"""
    if poison is not None:
        row, colm, val = poison
        x = x.clone()
        if colm is None:
            x[row] = val
        else:
            x[row, colm] = val
    return x


def lin_case(matrix, inst, N, M, data, rvmap=None, bias=True, seed=0, scales=SCALES[0], extra=0, reps=1, cus=NO_CUS, device="cpu",
             poison=None, tag=None):
    norm, rv_on, r1_on = inst
    rvmap = rvmap if rv_on else None
    P = M // reps
    assert P * reps == M

    def build():
        x, wp, bp, rowvec, rv, r1 = _lin_period(inst, N, P, data, rvmap, bias, seed)
        kw = dict(x=guard_rep(_poison(x, poison), reps, 344, device), wp=wp, s_acc=scales[0], out=guard_out(M, N + extra, N + extra + 56, device))
        if bp is not None:
            kw["bias"] = bp
        if norm:
            kw.update(norm=True, eps=1e-6 if seed % 2 else 1e-5)
        if rv_on:
            kw.update(rowvec=rowvec, rv=rv)
        if r1_on:
            kw.update(r1=guard_rep(r1, reps, N + 40, device), s1=scales[1])
        return kw
    id = f"lin320/{matrix}-{data}-n{norm}v{rv_on}r{r1_on}-N{N}-M{M}" + (f"-{tag}" if tag else "")
    return L0Case(id, "lin320", build, "exact" if data == "exact" else "lin320", matrix, M=M, N=N, inst=inst, data=data, rvmap=rvmap,
                  bias=bias, reps=reps, cus=cus, poison=poison)


_FF_PARAMS = {}


def ff_params(seed=3):
    """(w1p, b1 folded, w2p, b2) of ``op_cases._ff320_params(seed)``, packed once"""
    if seed not in _FF_PARAMS:
        from mofa_video_amd.weights import pack_ff320
        w1, b1, w2, b2, gamma, beta = oc._ff320_params(seed)
        _FF_PARAMS[seed] = pack_ff320(w1, b1, w2, gamma, beta) + (b2,)
    w1p, b1f, w2p, b2 = _FF_PARAMS[seed]
    return w1p, b1f, w2p, b2


def ff_case(matrix, kind, M, HW=7, T=5, reps=1, cus=NO_CUS, device="cpu", poison=None, tag=None):
    """kind: "+"-joined subset of pos, r2, ln (``plain``: none), or ``lnround`` (module docstring)"""
    kinds = tuple(k for k in kind.split("+") if k != "plain")
    if "lnround" in kinds:
        kinds = ("r2", "ln", "lnround")
    P = M // reps
    assert P * reps == M

    def build():
        w1p, b1f, w2p, b2 = ff_params()
        if "lnround" in kinds:
            x = (512 + _ints(-4, 4, P, 320, seed=P) / 2).half()
        else:
            x = _h(P, 320, seed=P, scale=1.3, shift=0.2)
        kw = dict(x=guard_rep(_poison(x, poison), reps, 352, device), w1p=w1p, b1=b1f, w2p=w2p, b2=b2, out=guard_out(M, 328, 384, device))
        if "pos" in kinds:
            kw.update(pos=_f(T, 320, seed=60, scale=0.5), HW=HW, T=T)
        if "lnround" in kinds:
            kw.update(r2=guard_rep((_ints(-64, 64, P, 320, seed=61) / 64).half(), reps, 368, device), s_acc=2.0 ** -30, s1=1.0, s2=1.0)
        elif "r2" in kinds:
            kw.update(r2=guard_rep(_h(P, 320, seed=61), reps, 368, device), s_acc=0.6, s1=0.6, s2=0.4)
        if "ln" in kinds:
            kw["ln_out"] = (1 + 0.1 * _f(320, seed=62), 0.1 * _f(320, seed=63), guard_out(M, 328, 400, device))
            kw["ln_eps"] = 3e-5
        return kw
    id = f"ff320/{matrix}-{kind}-M{M}" + (f"-{tag}" if tag else "")
    return L0Case(id, "ff320", build, "ff320", matrix, M=M, kind=kinds, HW=HW if "pos" in kinds else 1, T=T, reps=reps, cus=cus,
                  poison=poison)


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
def _matrix_a():
    """per instance every M once, N cycling through its seven values from an instance-dependent start: 13 cases per instance hold
    every (instance, M) and every (instance, N) pair; the row-vector mapping, the bias, the scales and the width of ``out``
    alternate along the way"""
    cases = []
    for k, inst in enumerate(INSTANCES):
        for i, M in enumerate(LIN_M):
            N = LIN_N[(i + k) % len(LIN_N)]
            cases.append(lin_case("a", inst, N, M, "exact", rvmap=("quirk", "row")[(i + k) % 2], bias=(i + k) % 4 != 3,
                                  seed=1000 + 100 * k + i, scales=SCALES[(i + k) % 3], extra=8 * ((i + k) % 2)))
    return cases


FF_KINDS = ("plain", "pos", "r2", "ln", "pos+r2+ln")
ISO_POISON = {"row0-nan": lambda M: (0, None, NAN), "last-row-nan": lambda M: (M - 1, None, NAN), "inf-at-wave-boundary": lambda M: (32, 17, INF)}
ISO_LIN = (((0, 1, 1), 300, "gauss"), ((1, 0, 0), 300, "exact"))
ISO_FF = (("pos+r2+ln", 200),)


def _matrix_e():
    cases = []
    for inst, M, data in ISO_LIN:
        for tag in (None,) + tuple(ISO_POISON):
            cases.append(lin_case("e", inst, 320, M, data, rvmap="quirk", seed=3000, scales=SCALES[0], extra=8,
                                  poison=ISO_POISON[tag](M) if tag else None, tag=tag or "clean"))
    for kind, M in ISO_FF:
        for tag in (None,) + tuple(ISO_POISON):
            cases.append(ff_case("e", kind, M, poison=ISO_POISON[tag](M) if tag else None, tag=tag or "clean"))
    return cases


CASES = (_matrix_a()
         + [ff_case("d", kind, M) for kind in FF_KINDS for M in FF_M] + [ff_case("d", "lnround", 33)]
         + _matrix_e())

# matrices b and c: (instance, N, data) / kind; the cases are built for a compute-unit count and a device
PERIODIC_LIN = ([(inst, N, data) for inst in ((0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1)) for N in (64, 128, 320) for data in ("exact", "gauss")]
                + [((0, 0, 0), 960, "gauss"), ((1, 0, 0), 960, "exact"), ((0, 1, 1), 960, "exact"), ((1, 1, 1), 960, "gauss")])
PERIODIC_FF = ("plain", "pos+r2+ln", "r2")


def periodic_reps(tile, tiles_per_cu, cus):
    """the fewest repeats of P_ROWS rows that give ``tiles_per_cu * cus + 1`` tiles of ``tile`` rows: some workgroup of a grid of
    ``cus`` then processes ``tiles_per_cu + 1`` tiles"""
    return -(-(tiles_per_cu * cus * tile + 1) // P_ROWS)


def periodic_lin(inst, N, data, cus, device="cpu"):
    """N < 960: 3 cus + 1 tiles, the fourth tile of a workgroup (every ring phase once and the first again); N = 960 (15 chunks, a
    multiple of 3: every tile starts in phase 0): 2 cus + 1 tiles, at least two tiles for every workgroup"""
    reps = periodic_reps(256, 2 if N == 960 else 3, cus)
    return lin_case("b", inst, N, reps * P_ROWS, data, rvmap="period", seed=2000 + N + 7 * sum(inst), scales=SCALES[N % 3],
                    reps=reps, cus=cus, device=device)


def periodic_ff(kind, cus, device="cpu"):
    reps = periodic_reps(128, 2, cus)
    return ff_case("c", kind, reps * P_ROWS, HW=1, T=P_ROWS, reps=reps, cus=cus, device=device)


CPU_CUS = 2                                          # the grid tests/test_l0_cases_cpu.py scales matrices b and c down to
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
