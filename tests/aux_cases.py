"""TEST INFRASTRUCTURE ONLY: the case table of the kernels between the stages that have no stand-in in tests/emu_ops.py --
csrc/cmp_ops.hip (``pool2d``, ``resize_bilinear_ac``, ``resize_bilinear_ac_f32``, ``flow_expectation``) and the blends and
movers of csrc/elementwise.hip (``mask_blend``, ``matting_blend``, ``geglu``, ``subsample_tokens``, ``flow_downscale``) -- with
their fp64 references, the per-element bounds and the "wrong kernel" mutants that prove the checks can fail.

Built on tests/op_cases.py: a case is an ``op_cases.Case`` whose ``build()`` gives the keyword arguments of the op as seeded CPU
tensors, every fp16 2-D argument a guarded view (NaN rows before and after, 8 NaN columns on the left, a leading dimension
larger than the width and different for every argument of a call), every fp32 NCHW input a ``View`` into a longer 1-D NaN
buffer, every ``out=`` a NaN-filled guarded view.  ``op_cases.run`` takes the case through ``mofa_video_amd.ops`` on the GPU
(tests/test_aux_ops_gpu.py) and through ``impl(defect)`` -- the references of this file behind the signatures of ``ops`` -- on
the CPU (tests/test_aux_cases_cpu.py).  ``check_run`` compares a run with ``case.ref``, computed in fp64 from the very tensors
the call received: per output either exact bits or ``|out - ref| <= bound`` per element, plus the elements that must be exact
and the ones that must be a same-signed infinity.

The bounds are derived from the arithmetic (u16 = 2^-11, u32 = 2^-24: half an ulp of fp16 / fp32), never measured:

  pool2d max          bit-equal: a maximum of fp16 values is one of them
  pool2d avg          data on the 2^-6 grid, |v| <= 8: the fp32 sum of k*k = 4 values and its product with 1/4 are exact, so the
                      result is the fp64 mean rounded once: bit-equal.  Gaussian data: within one fp16 ulp of that
  resize (fp16)       the source coordinate the documented ATen way in fp32 -- scale = fl((in-1)/(out-1)), s = fl(scale*d),
                      i0 = int(s), f = s - i0 (exact) -- the blend in fp64; u16 |ref| + 2^-25 (the output rounding, normal and
                      subnormal) + 6 u32 max|v00..v11| (1 - f, two products, three sums, taken per axis pair)
  resize (fp32)       6 u32 max|v|
  flow_expectation    64 u32 fmax: each weight's relative error is <= (1.5 |d_i| + 4) u32 (the rounding of d * log2e in front
                      of the hardware exp, and that exp), the softmax-weighted mean of |d_i| is <= ln(nbins) <= 4.9, and the two
                      7-level wave sums add less than 16 u32 fmax
  mask_blend          u16 |ref| + 2^-25 + 3 u32 (|a| + |b|); exact where w is 0.0 or 1.0
  matting_blend       out as mask_blend with the fp64 sigmoid; mask: (1.5 |l| + 4) u32 m, exactly 0 / 1 at l = -+65504
  geglu               u16 |ref| + 2^-25 + 2^-21 |v| max(1, |g|); saturated gates (+-30) exact; a product beyond the fp16 range is
                      the same-signed infinity on both sides
  subsample_tokens,
  flow_downscale      bit-equal (data movement; the division by s is one correctly rounded fp32 division)

Second pass of the grid-stride loops (csrc/elementwise.hip ``ew_blocks`` caps the grid at 16384 blocks of 256 items,
``op_cases.EW_GRID_ITEMS``).  The largest item counts of the BASELINE.md configurations (25 frames of 576 x 1024, flow maps of
72 x 128 = 9216 tokens and 320 channels = 40 vectors at the finest scale):
  mask_blend        25 * 9216 * 40 = 9.2 M  > 4.19 M   second-pass case
  matting_blend     24 * 9216 * 40 = 8.8 M  > 4.19 M   second-pass case (adapter.py: one call per scale over all warped frames)
  subsample_tokens  25 * 36 * 64 * 40 = 2.3 M (the landmark pyramid's half level) -- a second-pass case all the same
  geglu             not called by the package (the implicit GEMM's GEGLU epilogue is); a second-pass case all the same.  The
                    shape needs M * Ch / 8 > 4.19 M items: 32800 x (2 * 1032) (16400 rows give 2.1 M and stay in the first pass)
  flow_downscale    25 * 2 * 72 * 128 = 0.46 M: never reaches the second pass, no such case
  pool2d, the resizes, flow_expectation: one item per thread, no grid-stride loop."""
import types

import numpy as np
import torch

import op_cases as oc
from op_cases import F16, F32, NAN, View, _f, _h, _ints, guard

U16, U32 = 2.0 ** -11, 2.0 ** -24
F64 = torch.float64
INF = float("inf")
FMAX = 50.0
NBINS = (1, 63, 64, 65, 99, 128)
FLOW_IMG, FLOW_H, FLOW_W = 3, 7, 9                   # 189 tokens: the last block of 4 is ragged, image boundaries fall inside blocks
MUTANTS = ("pool-pad-zero", "avg-valid-count", "ac-false", "i1-unclamped", "no-half-step", "swap-xy", "drop-high-half", "w-div",
           "sub-round", "sigmoid-col1")
MUTANT_OPS = {"pool-pad-zero": ("pool2d",), "avg-valid-count": ("pool2d",), "ac-false": ("resize_bilinear_ac", "resize_bilinear_ac_f32"),
              "i1-unclamped": ("resize_bilinear_ac", "resize_bilinear_ac_f32"), "no-half-step": ("flow_expectation",),
              "swap-xy": ("flow_expectation",), "drop-high-half": ("flow_expectation",), "w-div": ("mask_blend",),
              "sub-round": ("subsample_tokens",), "sigmoid-col1": ("matting_blend",)}


def round16(x64):
    """fp64 -> fp16 in ONE rounding (numpy converts directly; a conversion through fp32 would round twice)"""
    with np.errstate(over="ignore"):                                  # beyond 65520: the infinity, as the kernels' conversion gives
        return torch.from_numpy(x64.numpy().astype(np.float16))


def ulp16(h):
    """one unit in the last place of the fp16 values ``h`` (2^-24 in the subnormal range), fp64"""
    a = h.double().abs().clamp(min=2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


OFF_ROUNDING = {}     # "case label" -> (elements that are not the fp64 reference rounded once, elements): filled by check_run


class Want:
    """what one output must be: ``bits`` (a tensor: bit-equal), or ``ref`` (fp64) with ``bound`` per element, ``exact`` (mask: the
    output equals round16(ref) there) and ``inf`` (mask: ``ref`` holds +-inf there and the output is that infinity)"""

    def __init__(self, bits=None, ref=None, bound=None, exact=None, inf=None):
        self.bits, self.ref, self.bound, self.exact, self.inf = bits, ref, bound, exact, inf


class AuxCase(oc.Case):
    """``ref(kw)`` -> [Want or int or None per entry of ``Run.outputs()``] from the call's own arguments (CPU copies taken before
    the call); ``meta``: the geometry the mutant rules and the table invariants read; ``big``: a second-pass case"""

    def __init__(self, id, op, build, ref, big=False, **meta):
        super().__init__(id, op, build, None)
        self.ref, self.big, self.meta = ref, big, meta


def inputs_of(r):
    """the keyword arguments of a run with every tensor as it was BEFORE the call, on the CPU"""
    return {k: (r.placed[k].before().cpu() if k in r.placed else v) for k, v in r.kwargs.items()}


def check_want(what, g, w, accumulate=False):
    """one output ``g`` against its ``Want`` (or the int / None / object it must be) -> (worst err / bound, [messages]);
    ``accumulate``: add to the OFF_ROUNDING entry of ``what`` (an output checked in row chunks), not replace it"""
    errs, worst = [], 0.0
    if not isinstance(w, Want):
        if not (g is w or (not torch.is_tensor(g) and g == w)):
            errs.append(f"{what}: {g!r} returned, {w!r} expected")
        return worst, errs
    want = w.bits if w.bits is not None else w.ref
    if not torch.is_tensor(g) or g.shape != want.shape or (w.bits is not None and g.dtype != want.dtype):
        errs.append(f"{what}: {getattr(g, 'shape', g)} / {getattr(g, 'dtype', None)} returned, {tuple(want.shape)} expected")
        return worst, errs
    if w.bits is not None:
        n = int((oc.bits(g) != oc.bits(want)).sum())
        if n:
            worst = INF
            first = torch.nonzero(oc.bits(g) != oc.bits(want))[0].tolist()
            errs.append(f"{what}: {n} / {g.numel()} elements are not bit-equal, first at {first}: {g[tuple(first)].item()!r} "
                        f"for {want[tuple(first)].item()!r}")
        return worst, errs
    gd = g.double()
    if w.inf is None:                                                # (no mask to apply: a 40 M element output is not gathered four times)
        inf, sel = torch.zeros((), dtype=torch.bool), (lambda t: t.reshape(-1))
    else:
        inf, sel = w.inf, (lambda t: t[~w.inf])
        if bool((gd[inf] != w.ref[inf]).any()):
            errs.append(f"{what}: {int((gd[inf] != w.ref[inf]).sum())} of the {int(inf.sum())} overflowing elements are not the same-signed inf")
    if not bool(torch.isfinite(sel(gd)).all()):
        bad = ~torch.isfinite(gd) & ~inf
        errs.append(f"{what}: {int(bad.sum())} non-finite elements, first at {torch.nonzero(bad)[0].tolist()}")
        return INF, errs
    err = sel((gd - w.ref).abs())
    bound = sel((w.bound if torch.is_tensor(w.bound) else torch.full(gd.shape, float(w.bound), dtype=F64)).expand(gd.shape))
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, INF), torch.zeros_like(err)))
    if ratio.numel():
        worst = max(worst, ratio.max().item())
        if ratio.max().item() > 1.0:
            i = int(ratio.argmax())
            errs.append(f"{what}: {int((ratio > 1).sum())} / {ratio.numel()} elements out of bound, worst err {err[i].item():.4e} "
                        f"= {ratio[i].item():.3f} x its bound {bound[i].item():.4e}")
    once = (round16(w.ref) if g.dtype == F16 else w.ref.float()).double()
    n0, m0 = OFF_ROUNDING.get(what, (0, 0)) if accumulate else (0, 0)
    OFF_ROUNDING[what] = (n0 + int(sel(gd != once).sum()), m0 + sel(gd).numel())
    if w.exact is not None and bool(w.exact.any()):
        n = int((gd[w.exact] != once[w.exact]).sum())
        if n:
            errs.append(f"{what}: {n} of the {int(w.exact.sum())} elements that must be exact are not")
    return worst, errs


def check_run(case, r):
    """-> (worst err / bound over the bounded outputs, [messages]): guards, then every output against ``case.ref``"""
    errs = list(r.guard_errors())
    wants, outs = case.ref(inputs_of(r)), r.outputs()
    worst = 0.0
    if len(wants) != len(outs):
        return INF, errs + [f"{case.id}: {len(outs)} outputs {[o[0] for o in outs]}, {len(wants)} expected"]
    for (label, g, _), w in zip(outs, wants):
        wo, e = check_want(f"{case.id} {label}", g, w)
        worst, errs = max(worst, wo), errs + e
    return worst, errs


# ---------------------------------------------------------------------------------------------------------------------------
# the fp64 references, straight from the definitions in include/mofa_hip.h (``defect``: one of MUTANTS, a wrong kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def pool_size(n_in, k, stride, pad):
    return (n_in + 2 * pad - k) // stride + 1


def pool_ref(x64, n, H, W, k, stride, pad, mode, defect=None):
    """x64 [n*H*W, C] -> [n*Ho*Wo, C]: the window maximum with the padding ignored (mode "max") / the window mean ("avg")"""
    C = x64.shape[1]
    Ho, Wo = pool_size(H, k, stride, pad), pool_size(W, k, stride, pad)
    fill = -INF if mode == "max" and defect != "pool-pad-zero" else 0.0
    vp = torch.full((n, H + 2 * pad, W + 2 * pad, C), fill, dtype=F64)
    vp[:, pad:pad + H, pad:pad + W] = x64.reshape(n, H, W, C)
    inside = torch.zeros((1, H + 2 * pad, W + 2 * pad, 1), dtype=F64)
    inside[:, pad:pad + H, pad:pad + W] = 1.0
    acc, cnt = None, 0.0
    for ky in range(k):
        for kx in range(k):
            ys, xs = slice(ky, ky + (Ho - 1) * stride + 1, stride), slice(kx, kx + (Wo - 1) * stride + 1, stride)
            win = vp[:, ys, xs]
            acc = win if acc is None else (torch.maximum(acc, win) if mode == "max" else acc + win)
            cnt = cnt + inside[:, ys, xs]
    if mode == "avg":
        acc = acc / (cnt if defect == "avg-valid-count" else float(k * k))
    return acc.reshape(n * Ho * Wo, C)


def border_windows(H, W, k, stride, pad):
    """mask [Ho, Wo] of the windows that reach into the padding"""
    Ho, Wo = pool_size(H, k, stride, pad), pool_size(W, k, stride, pad)
    oy, ox = torch.arange(Ho)[:, None] * stride - pad, torch.arange(Wo)[None, :] * stride - pad
    return (oy < 0) | (oy + k > H) | (ox < 0) | (ox + k > W)


def ac_coords(n_in, n_out, defect=None):
    """-> (i0 int64 [n_out], f fp64 [n_out]): the align_corners=True source coordinate as ATen takes it, IN fp32"""
    d = torch.arange(n_out, dtype=F32)
    if defect == "ac-false":
        s = ((d + 0.5) * (float(n_in) / float(n_out)) - 0.5).clamp(min=0.0)
    else:
        scale = torch.tensor(float(n_in - 1), dtype=F32) / torch.tensor(float(n_out - 1), dtype=F32) if n_out > 1 else torch.tensor(0.0)
        s = scale * d                                                 # one fp32 product, rounded
    i0 = s.to(torch.int64)
    f = s - i0.to(F32)                                                # exact (Sterbenz / same binade)
    return i0, f.double()


def bilinear_ref(v64, P, Hin, Win, Hout, Wout, defect=None):
    """v64 [P*Hin*Win, C] (P images of Hin x Win pixels) -> (blend [P*Hout*Wout, C] in fp64, max |v00..v11| per element)"""
    y0, fy = ac_coords(Hin, Hout, defect)
    x0, fx = ac_coords(Win, Wout, defect)
    if defect == "i1-unclamped":           # reads the next pixel / row of the flat buffer; behind the last image lies the NaN guard
        y1, x1 = y0 + 1, x0 + 1
        v64 = torch.cat([v64, torch.full((Win + 2, v64.shape[1]), NAN, dtype=F64)])
    else:
        y1, x1 = y0 + (y0 < Hin - 1).long(), x0 + (x0 < Win - 1).long()
    img = torch.arange(P)[:, None, None] * (Hin * Win)

    def at(yy, xx):
        return v64[(img + yy[None, :, None] * Win + xx[None, None, :]).reshape(-1)]
    v00, v01, v10, v11 = at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1)
    fxe = fx[None, None, :].expand(P, Hout, Wout).reshape(-1, 1)
    fye = fy[None, :, None].expand(P, Hout, Wout).reshape(-1, 1)
    out = (1 - fye) * ((1 - fxe) * v00 + fxe * v01) + fye * ((1 - fxe) * v10 + fxe * v11)
    vmax = torch.stack([v00.abs(), v01.abs(), v10.abs(), v11.abs()]).amax(0)
    return out, vmax


def bilinear_fp32_is_exact(v64, P, Hin, Win, Hout, Wout):
    """the kernel's own fp32 operation order gives the fp64 blend exactly (the precondition of the exact sub-family)"""
    y0, fy = ac_coords(Hin, Hout)
    x0, fx = ac_coords(Win, Wout)
    y1, x1 = y0 + (y0 < Hin - 1).long(), x0 + (x0 < Win - 1).long()
    img = torch.arange(P)[:, None, None] * (Hin * Win)
    v = v64.float()

    def at(yy, xx):
        return v[(img + yy[None, :, None] * Win + xx[None, None, :]).reshape(-1)]
    fxe = fx.float()[None, None, :].expand(P, Hout, Wout).reshape(-1, 1)
    fye = fy.float()[None, :, None].expand(P, Hout, Wout).reshape(-1, 1)
    top = (1 - fxe) * at(y0, x0) + fxe * at(y0, x1)
    bot = (1 - fxe) * at(y1, x0) + fxe * at(y1, x1)
    out = (1 - fye) * top + fye * bot
    return bool((out.double() == bilinear_ref(v64, P, Hin, Win, Hout, Wout)[0]).all())


def flow_centres(nbins, fmax, defect=None):
    return (torch.arange(nbins, dtype=F64) + (0.0 if defect == "no-half-step" else 0.5)) * (2.0 * fmax / nbins) - fmax


def flowexp_ref(l64, nimg, HW, nbins, fmax, defect=None):
    """l64 [nimg*HW, >= 2*nbins] -> [nimg, 2, HW]: per axis the softmax expectation over the bin centres"""
    c = flow_centres(nbins, fmax, defect)
    halves = [l64[:, :nbins], l64[:, nbins:2 * nbins]]
    if defect == "swap-xy":
        halves.reverse()
    keep = 64 if defect == "drop-high-half" else nbins
    e = torch.stack([(torch.softmax(h[:, :keep], dim=1) * c[:keep]).sum(1) for h in halves], 1)      # [ntok, 2]
    return e.reshape(nimg, HW, 2).permute(0, 2, 1).contiguous()


def blend_bound(ref, a, b):
    return U16 * ref.abs() + 2.0 ** -25 + 3 * U32 * (a.abs() + b.abs())


def gelu64(g):
    return g * (0.5 * torch.special.erfc(g * -(0.5 ** 0.5)))


def subsample_ref(x, n, H, W, s, defect=None):
    off = s // 2 if defect == "sub-round" else 0
    return x.reshape(n, H, W, -1)[:, off::s, off::s].reshape(n * (H // s) * (W // s), -1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# the references behind the signatures of mofa_video_amd.ops: impl(None) is a correct implementation, impl(defect) a wrong one
# ---------------------------------------------------------------------------------------------------------------------------
def _into(out, y):
    if out is None:
        return y
    out[:, :y.shape[1]] = y
    return out


def impl(defect=None):
    def pool2d(x, nimg, H, W, C, k, stride, pad=0, mode="max", out=None):
        y = round16(pool_ref(x[:, :C].double(), nimg, H, W, k, stride, pad, mode, defect))
        return _into(out, y), pool_size(H, k, stride, pad), pool_size(W, k, stride, pad)

    def resize_bilinear_ac(x, nimg, H, W, C, Ho, Wo, out=None):
        return _into(out, round16(bilinear_ref(x[:, :C].double(), nimg, H, W, Ho, Wo, defect)[0]))

    def resize_bilinear_ac_f32(x, Ho, Wo):
        H, W = x.shape[-2:]
        P = x.numel() // (H * W)
        y = bilinear_ref(x.double().reshape(P * H * W, 1), P, H, W, Ho, Wo, defect)[0]
        return y.float().reshape(tuple(x.shape[:-2]) + (Ho, Wo))

    def flow_expectation(logits, nimg, H, W, nbins, fmax):
        return flowexp_ref(logits.double(), nimg, H * W, nbins, fmax, defect).float().reshape(nimg, 2, H, W)

    def _w_rows(w, M, HW):
        rows = torch.arange(M)
        return w.double()[(rows // HW) % HW if defect == "w-div" else rows % HW][:, None]

    def mask_blend(a, b, w, HW, out=None):
        m = _w_rows(w, a.shape[0], HW)
        return _into(out, round16(a.double() * m + b.double() * (1 - m)))

    def matting_blend(warped, matting, logit, want_mask=True):
        m = torch.sigmoid(logit[:, 1 if defect == "sigmoid-col1" else 0].double())
        out = round16(warped.double() * m[:, None] + matting.double() * (1 - m[:, None]))
        return out, (m.float() if want_mask else None)

    def geglu(x, out=None):
        Ch = x.shape[1] // 2
        return _into(out, round16(x[:, :Ch].double() * gelu64(x[:, Ch:].double())))

    def subsample_tokens(x, n, H, W, s):
        return subsample_ref(x, n, H, W, s, defect).clone()

    def flow_downscale(flow, s):
        return (flow[:, :, ::s, ::s].double() / s).float().contiguous()
    return types.SimpleNamespace(**{k: v for k, v in locals().items() if callable(v) and not k.startswith("_")})


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
def _grid(*shape, seed=0):
    """fp16 values on the 2^-6 grid, |v| <= 8"""
    return (_ints(-512, 512, *shape, seed=seed) / 64).half()


def _nchw_view(data, pre=5, post=37):
    """fp32 [..] data as a View into a longer 1-D NaN buffer"""
    n, shape = data.numel(), tuple(data.shape)
    base = torch.full((pre + n + post,), NAN, dtype=F32)
    base[pre:pre + n] = data.reshape(-1)
    return View(base, lambda b: b[pre:pre + n].view(shape))


def _pool_data(n, H, W, C, seed):
    """max pooling: Gaussian shifted by -3 and capped below zero, so a window that counted its padding as 0 would show; +65504
    at the centre pixel of image 0 (which no window that reaches into the padding holds, asserted on the CPU) and -65504"""
    x = torch.minimum(_f(n, H, W, C, seed=seed, shift=-3.0), torch.tensor(-0.0625)).half()
    x[0, H // 2, W // 2, 0] = 65504.0
    x[n - 1, H // 2, W // 2, C - 1] = 65504.0
    x[0, 0, 0, 1] = x[n - 1, H - 1, W - 1, 0] = x[0, H // 2, W // 2, 2] = -65504.0
    return x.reshape(n * H * W, C)


def _pool_case(mode, k, s, p, H, W, C, data, seed, production=False):
    n = 2

    def build():
        x = {"neg": _pool_data, "grid": lambda *a: _grid(n * H * W, C, seed=seed), "gauss": lambda *a: _h(n * H * W, C, seed=seed)}[data](n, H, W, C, seed)
        kw = dict(nimg=n, H=H, W=W, C=C, k=k, stride=s, pad=p, mode=mode)
        if production:                                               # cmp.py's decoder pools: the 320-wide concat buffer itself, ld == C
            return dict(x=x.contiguous(), **kw)
        M = n * pool_size(H, k, s, p) * pool_size(W, k, s, p)
        return dict(x=guard(x, ld=88), out=guard(shape=(M, C), ld=104), **kw)

    def ref(kw):
        y = pool_ref(kw["x"][:, :C].double(), n, H, W, k, s, p, mode)
        if mode == "avg" and data == "gauss":
            once = round16(y)
            want = Want(ref=once.double(), bound=ulp16(once))
        else:
            want = Want(bits=round16(y))
        return [want, pool_size(H, k, s, p), pool_size(W, k, s, p)]
    tag = f"pool2d/{mode}-k{k}s{s}p{p}-{H}x{W}-C{C}" + ("-ld320" if production else "") + (f"-{data}" if mode == "avg" else "")
    return AuxCase(tag, "pool2d", build, ref, mode=mode, k=k, s=s, p=p, H=H, W=W, C=C, data=data, n=n)


RESIZE_PAIRS = [((1, 1), (4, 6)), ((3, 5), (1, 1)), ((2, 3), (16, 24)), ((6, 10), (12, 20)), ((12, 20), (6, 10)), ((5, 7), (5, 7)),
                ((3, 5), (9, 9))]
RESIZE_EXACT = [((5, 7), (5, 7)), ((3, 5), (9, 9))]              # identity; every f a multiple of 1/4 on both axes


def _resize_tok_case(pair, C, exact, seed):
    (Hin, Win), (Hout, Wout) = pair
    n = 2

    def build():
        x = _grid(n * Hin * Win, C, seed=seed) if exact else _h(n * Hin * Win, C, seed=seed)
        M = n * Hout * Wout
        base = torch.full((3 + M + 2, 8 + 512 + 16), NAN, dtype=F16)          # a 512-wide concat buffer, guarded; block 1 is written
        return dict(x=guard(x, ld=C + 24), nimg=n, H=Hin, W=Win, C=C, Ho=Hout, Wo=Wout,
                    out=View(base, lambda b: b[3:3 + M, 8 + 128:8 + 128 + C]))

    def ref(kw):
        y, vmax = bilinear_ref(kw["x"][:, :C].double(), n, Hin, Win, Hout, Wout)
        if exact:
            return [Want(bits=round16(y))]
        return [Want(ref=y, bound=U16 * y.abs() + 2.0 ** -25 + 6 * U32 * vmax)]
    tag = f"resize_bilinear_ac/{Hin}x{Win}-to-{Hout}x{Wout}-C{C}" + ("-exact" if exact else "")
    return AuxCase(tag, "resize_bilinear_ac", build, ref, pair=pair, C=C, exact=exact, n=n)


def _resize_f32_case(pair, lead, seed):
    (Hin, Win), (Hout, Wout) = pair
    P = lead[0] * lead[1]

    def build():
        return dict(x=_nchw_view(_f(*lead, Hin, Win, seed=seed, scale=20.0)), Ho=Hout, Wo=Wout)

    def ref(kw):
        y, vmax = bilinear_ref(kw["x"].double().reshape(P * Hin * Win, 1), P, Hin, Win, Hout, Wout)
        shape = tuple(lead) + (Hout, Wout)
        return [Want(ref=y.reshape(shape), bound=(6 * U32 * vmax).reshape(shape))]
    return AuxCase(f"resize_bilinear_ac_f32/{lead[0]}x{lead[1]}x{Hin}x{Win}-to-{Hout}x{Wout}", "resize_bilinear_ac_f32", build, ref,
                   pair=pair, n=P)


FLOW_HOT = (0, 63, 64, -1)                                          # one-hot bins (the last one for -1), clipped to the bin count
FLOW_ROWS = dict(equal=(10, 20), hot=(30, 38), huge=(50, 58))        # token rows of the non-Gaussian logit patterns


def _flow_logits(nbins, seed):
    """189 tokens: Gaussian x 3; rows of all-equal logits (0.75, and -65504 throughout); one-hot +40 at bin 0 / 63 / 64 / last,
    another of them for the y half than for the x half; rows holding +65504 (that bin takes all the weight) and -65504"""
    ntok = FLOW_IMG * FLOW_H * FLOW_W
    l = _h(ntok, 2 * nbins, seed=seed, scale=3.0)
    e0, e1 = FLOW_ROWS["equal"]
    l[e0:(e0 + e1) // 2] = 0.75
    l[(e0 + e1) // 2:e1] = -65504.0
    hot = [nbins - 1 if b < 0 else min(b, nbins - 1) for b in FLOW_HOT]
    h0, h1 = FLOW_ROWS["hot"]
    for r in range(h0, h1):
        i = r - h0
        l[r] *= 0.25
        l[r, hot[i % 4]] = 40.0
        l[r, nbins + hot[(i + 1 + i // 4) % 4]] = 40.0
    g0, g1 = FLOW_ROWS["huge"]
    for r in range(g0, g1):
        l[r, (7 * r) % nbins] = 65504.0 if r % 2 else -65504.0
        l[r, nbins + (5 * r + 3) % nbins] = -65504.0 if r % 2 else 65504.0
    return l


def _flow_case(nbins):
    nimg, H, W = FLOW_IMG, FLOW_H, FLOW_W

    def build():                                                     # the columns beyond 2 * nbins are guard: NaN
        return dict(logits=guard(_flow_logits(nbins, seed=200 + nbins), ld=(2 * nbins + 7) // 8 * 8 + 16), nimg=nimg, H=H, W=W, nbins=nbins,
                    fmax=FMAX)

    def ref(kw):
        y = flowexp_ref(kw["logits"].double(), nimg, H * W, nbins, FMAX)
        return [Want(ref=y.reshape(nimg, 2, H, W), bound=64 * U32 * FMAX)]
    return AuxCase(f"flow_expectation/nbins{nbins}", "flow_expectation", build, ref, nbins=nbins, ntok=nimg * H * W)


def _blend_w(HW, seed):
    w = torch.rand(HW, generator=torch.Generator().manual_seed(seed))
    w[0] = w[HW // 2] = 0.0
    w[5] = w[HW - 1] = 1.0
    return w


def _mask_blend_case(big):
    M, C, HW = (oc.BIG_ROWS, oc.BIG_COLS, 41) if big else (6 * 35, 64, 35)

    def build():
        if big:
            return dict(a=guard(oc._big16(210), ld=2072, rows=(1, 1)), b=guard(oc._big16(211), ld=2080, rows=(1, 1)), w=_blend_w(HW, 212),
                        HW=HW, out=guard(shape=(M, C), ld=2088, rows=(1, 1)))
        return dict(a=guard(_h(M, C, seed=210), ld=88), b=guard(_h(M, C, seed=211), ld=104), w=_blend_w(HW, 212), HW=HW,
                    out=guard(shape=(M, C), ld=120))

    def ref(kw):
        a, b = kw["a"].double(), kw["b"].double()
        m = kw["w"].double()[torch.arange(M) % HW][:, None]
        y = a * m + b * (1 - m)
        return [Want(ref=y, bound=blend_bound(y, a, b), exact=((m == 0) | (m == 1)).expand(M, C))]
    return AuxCase("mask_blend/" + ("second-pass" if big else "small"), "mask_blend", build, ref, big=big, M=M, C=C, HW=HW, items=M * (C // 8))


MATTING_LOGITS = (0.0, 12.0, -12.0, 65504.0, -65504.0)


def _matting_case(big, want_mask):
    M, C = (oc.BIG_ROWS, oc.BIG_COLS) if big else (210, 64)

    def build():
        lg = _h(M, 8, seed=222, scale=3.0)                          # column 0 = the logit, the other seven are other numbers
        for i, v in enumerate(MATTING_LOGITS):
            lg[i, 0] = lg[M - 1 - i, 0] = v
            lg[i, 1] = lg[M - 1 - i, 1] = 1.5 - i
        if big:
            return dict(warped=guard(oc._big16(220), ld=2072, rows=(1, 1)), matting=guard(oc._big16(221), ld=2080, rows=(1, 1)),
                        logit=guard(lg, ld=24), want_mask=want_mask)
        return dict(warped=guard(_h(M, C, seed=220), ld=88), matting=guard(_h(M, C, seed=221), ld=104), logit=guard(lg, ld=24),
                    want_mask=want_mask)

    def ref(kw):
        a, b, l = kw["warped"].double(), kw["matting"].double(), kw["logit"][:, 0].double()
        m = torch.sigmoid(l)
        y = a * m[:, None] + b * (1 - m[:, None])
        sat = l.abs() == 65504.0
        out = Want(ref=y, bound=blend_bound(y, a, b), exact=sat[:, None].expand(M, C))
        return [out, Want(ref=m, bound=(1.5 * l.abs() + 4) * U32 * m, exact=sat) if want_mask else None]
    tag = "matting_blend/" + ("second-pass" if big else "small") + ("" if want_mask else "-no-mask")
    return AuxCase(tag, "matting_blend", build, ref, big=big, M=M, C=C, items=M * (C // 8))


GEGLU_GATES = (0.0, -0.0, 30.0, -30.0, 6.0, -6.0)
GEGLU_BIG = (32800, 1032)                                            # 32800 * 129 vectors = 4 231 200 > 4 194 304


def _geglu_case(kind):
    M, Ch = GEGLU_BIG if kind == "second-pass" else (50, 128)

    def build():
        if kind == "second-pass":
            blk = torch.cat([_h(257, Ch, seed=230), _h(257, Ch, seed=231, scale=2.0)], 1)
            return dict(x=guard(blk.repeat(-(-M // 257), 1)[:M].contiguous(), ld=2 * Ch + 24, rows=(1, 1)),
                        out=guard(shape=(M, Ch), ld=Ch + 16, rows=(1, 1)))
        x = torch.cat([_h(M, Ch, seed=230), _h(M, Ch, seed=231, scale=2.0)], 1)
        for j, g in enumerate(GEGLU_GATES):
            x[0, Ch + j] = x[M - 1, Ch + 64 + j] = g
            x[0, j], x[M - 1, 64 + j] = 1.25 + j, -0.75 - j
        if kind == "overflow":                                       # 300 * gelu(300) = 90000: beyond fp16, +inf; and its negative
            x[3, 7], x[3, Ch + 7], x[4, 9], x[4, Ch + 9] = 300.0, 300.0, -300.0, 300.0
            return dict(x=guard(x, ld=280))
        return dict(x=guard(x, ld=280), out=guard(shape=(M, Ch), ld=152))

    def ref(kw):
        v, g = kw["x"][:, :Ch].double(), kw["x"][:, Ch:].double()
        y = v * gelu64(g)
        over = y.abs() >= 65520.0                                    # rounds to the fp16 infinity
        y = torch.where(over, torch.sign(y) * INF, y)
        return [Want(ref=y, bound=U16 * y.abs() + 2.0 ** -25 + 2.0 ** -21 * v.abs() * g.abs().clamp(min=1.0), exact=g.abs() == 30.0, inf=over)]
    return AuxCase(f"geglu/{kind}", "geglu", build, ref, big=kind == "second-pass", M=M, Ch=Ch, items=M * (Ch // 8), kind=kind)


def _subsample_case(n, H, W, s, C=64, big=False):
    def build():
        if big:
            blk = _h(257, C, seed=240)
            rows = n * H * W
            x = blk.repeat(-(-rows // 257), 1)[:rows] * (1.0 + (torch.arange(rows) % 89).float() / 128)[:, None].half()
            return dict(x=guard(x, ld=C + 16, rows=(1, 1)), n=n, H=H, W=W, s=s)
        return dict(x=guard(_h(n * H * W, C, seed=240 + s), ld=88), n=n, H=H, W=W, s=s)

    def ref(kw):
        return [Want(bits=subsample_ref(kw["x"], n, H, W, s))]
    return AuxCase(f"subsample_tokens/n{n}-{H}x{W}-s{s}" + ("-second-pass" if big else ""), "subsample_tokens", build, ref, big=big, s=s,
                   items=n * (H // s) * (W // s) * (C // 8))


def _flow_downscale_case(n, H, W, s):
    def build():
        return dict(flow=_nchw_view(_f(n, 2, H, W, seed=250 + s, scale=20.0)), s=s)

    def ref(kw):
        return [Want(bits=(kw["flow"][:, :, ::s, ::s].double() / s).float().contiguous())]
    return AuxCase(f"flow_downscale/n{n}-{H}x{W}-s{s}", "flow_downscale", build, ref, s=s, n=n, H=H, W=W)


POOL_MAX = [(3, 2, 1), (2, 2, 0), (4, 4, 0)]
POOL_MAPS = [(7, 9), (8, 10), (9, 17)]
CASES = (
    [_pool_case("max", k, s, p, H, W, (8, 64)[(i + j) % 2], "neg", 300 + 10 * i + j)
     for i, (k, s, p) in enumerate(POOL_MAX) for j, (H, W) in enumerate(POOL_MAPS)]
    + [_pool_case("max", 8, 8, 0, H, W, C, "neg", 340 + i) for i, (H, W, C) in enumerate(((8, 10, 8), (9, 17, 64), (8, 16, 64)))]
    + [_pool_case("max", 8, 8, 0, 8, 16, 320, "neg", 345, production=True)]
    + [_pool_case("avg", 2, 2, 0, H, W, C, data, 350 + i)
       for i, (H, W, C, data) in enumerate(((6, 10, 8, "grid"), (7, 9, 64, "grid"), (6, 10, 64, "gauss"), (7, 9, 8, "gauss")))]
    + [_resize_tok_case(pair, C, False, 400 + 2 * i + j) for i, pair in enumerate(RESIZE_PAIRS) for j, C in enumerate((8, 128))]
    + [_resize_tok_case(pair, (128, 8)[i], True, 420 + i) for i, pair in enumerate(RESIZE_EXACT)]
    + [_resize_f32_case(pair, (2, 2), 430 + i) for i, pair in enumerate(RESIZE_PAIRS)]
    + [_resize_f32_case(((4, 6), (8, 12)), (3, 2), 440)]
    + [_flow_case(nb) for nb in NBINS]
    + [_mask_blend_case(False), _mask_blend_case(True)]
    + [_matting_case(False, True), _matting_case(False, False), _matting_case(True, True)]
    + [_geglu_case("small"), _geglu_case("overflow"), _geglu_case("second-pass")]
    + [_subsample_case(3, 8, 12, 2), _subsample_case(2, 6, 6, 3), _subsample_case(2, 4, 4, 4), _subsample_case(2, 5, 7, 1),
       _subsample_case(1, 200, 328, 2, C=2056, big=True)]
    + [_flow_downscale_case(3, 8, 12, 1), _flow_downscale_case(2, 8, 24, 8), _flow_downscale_case(1, 16, 32, 4),
       _flow_downscale_case(3, 16, 32, 2)]
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
OPS = tuple(dict.fromkeys(c.op for c in CASES))


def mutant_differs(defect, case):
    """from the geometry alone: does the wrong kernel ``defect`` compute something else than the right one on ``case``"""
    m = case.meta
    if case.op not in MUTANT_OPS[defect]:
        return False
    if defect == "pool-pad-zero":          # some window reaches into the padding (its true maximum is negative, asserted)
        return m["mode"] == "max" and bool(border_windows(m["H"], m["W"], m["k"], m["s"], m["p"]).any())
    if defect == "avg-valid-count":        # the average takes pad == 0 only and the output size is floored: every window lies
        return False                       # wholly inside the map and holds k * k valid pixels -- the two divisors never differ
    if defect in ("ac-false", "i1-unclamped"):
        (Hin, Win), (Hout, Wout) = m["pair"]
        if defect == "ac-false":           # the two coordinate rules agree only for an identity or a one-pixel source axis
            return any(i > 1 and i != o for i, o in ((Hin, Hout), (Win, Wout)))
        # some output pixel sits ON the last source row / column: i1 = i0 + 1 leaves the image, and behind the last image
        # lies the NaN guard (one-pixel axes: always; else when fl(fl((in-1)/(out-1)) * (out-1)) reaches in - 1)
        return any(bool((ac_coords(i, o)[0] == i - 1).any()) for i, o in ((Hin, Hout), (Win, Wout)))
    if defect == "no-half-step":
        return True
    if defect == "swap-xy":                # one bin: both expectations are the one centre
        return m["nbins"] > 1
    if defect == "drop-high-half":
        return m["nbins"] > 64
    if defect == "w-div":
        return m["M"] > m["HW"]
    if defect == "sub-round":
        return m["s"] >= 2
    if defect == "sigmoid-col1":
        return True
    raise KeyError(defect)
