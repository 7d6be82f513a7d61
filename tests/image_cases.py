"""TEST INFRASTRUCTURE ONLY: the case table of the kernels that bracket the denoising loop -- csrc/frontend.hip
(``filter1d_reflect``, ``resize_bicubic_ac``, ``patchify``), ``resize_nearest_f32`` of csrc/elementwise.hip and csrc/output.hip
(``frames_postprocess``, ``flow_maxrad`` + ``flow_to_image``) -- with their references, the per-element bounds and the "wrong
kernel" mutants that prove the checks can fail.

Built on tests/op_cases.py and tests/aux_cases.py.  A case is an ``op_cases.Case`` whose ``build()`` gives the keyword arguments
of one call: every input a ``View`` into a longer NaN buffer, ``out`` a ``View`` into a buffer of NaN (0xA5 bytes for uint8), the
flow workspace a view of exactly ``WS_BYTES`` bytes inside a longer 0xA5 buffer.  The ``ops`` wrappers allocate their own outputs,
so a case is called through a backend with ``out=`` / ``ws=`` parameters: ``impl(defect)`` of this file on the CPU
(tests/test_image_cases_cpu.py), the C ABI on the GPU (tests/test_image_ops_gpu.py).  ``check_run`` compares a run with
``case.ref``, computed from the very tensors the call received, and checks that everything outside the views and every
read-only argument kept its bits.

The bounds are derived from the arithmetic (u32 = 2^-24, half an ulp of fp32 at 1), never measured:

  filter1d_reflect    acc_j = fma(tap_j, x_j, acc_(j-1)): k roundings, each at most u32 times a partial sum that is at most
                      S = sum_j |tap_j x_j|: k u32 S.  k = 1 with tap 1.0 is a copy: bit-equal.  Exact family: dyadic taps on
                      2^-6 grid data, |v| <= 8: every product is a multiple of 2^-9 and every partial sum at most 8, 13 bits
                      -- the fp32 chain IS the fp64 sum (asserted on the CPU): bit-equal
  resize_bicubic_ac   the coordinate in fp32 as ATen takes it: s = fl(fl((in-1)/(out-1)) * o), t = s - floor(s) (exact) clamped
                      to [0, 1]; weights and blend in fp64.  The kernel evaluates the Keys polynomials (A = -0.75) in fp32 by
                      Horner's rule.  End taps, x = 1 + t or 2 - t in [1, 2] (rounded: error u32, times |dw/dx| <= 0.75):
                        p1 = A x (|p1| <= 1.5), p2 = p1 - 5A (<= 3), p3 = p2 x (<= 4.5), p4 = p3 + 8A (<= 3), p5 = p4 x (<= 3),
                        w = p5 - 4A (<= 0.15); the error doubles at most at each product with x and grows by u32 |p_i| at each
                        step: ((1.5 + 3) 2 + 4.5 + 3) 2 + 3 + 0.15 < 37, with the argument's 0.75: eps_end = 38 u32 ABSOLUTE
                        (the polynomial's terms reach 6 and cancel to |w| <= 0.15: relative to w this is unbounded)
                      Inner taps, x = t or 1 - t in [0, 1] (1 - t rounded: u32 / 2 times |dw/dx| <= 1.35):
                        q1 = (A + 2) x - (A + 3) (two roundings, |.| <= 2.25: 3.5 u32), q2 = q1 x (<= 2.25), q3 = q2 x (<= 2.25),
                        w = q3 + 1 (<= 1): 3.5 + 2.25 + 2.25 + 1 + 0.7 < 10: eps_in = 10 u32
                      Carried through both axes, with the 9 roundings of the blend itself (4 products and 3 sums per row, the
                      product with wy, the sum over rows; fewer when fused), each relative to the running sum of magnitudes:
                        bound = sum |v| [(|wy| + eps_y)(|wx| + eps_x) - |wy||wx|] + 10 u32 sum (|wy| + eps_y)(|wx| + eps_x) |v|
                      Identity: t = 0, weights exactly (0, 1, 0, 0): bit-equal.  Exact family (3,5) -> (9,17): every t a multiple
                      of 1/4, weights multiples of 2^-8 evaluated exactly; data on the 2^-2 grid, |v| <= 8: v wx is a multiple
                      of 2^-10, times wy of 2^-18, sums below 2^4: 22 bits (the kernel's own fp32 order asserted exact on the
                      CPU; the 2^-6 grid would need 26)
  patchify            data movement and ONE rounding fp32 -> fp16: bit-equal to round16 of F.unfold; columns >= C p p are +0
  resize_nearest_f32  src = min(floor(fl(o * fl(in / out))), in - 1) in fp32, ATen's rule: bit-equal to F.interpolate
  frames_postprocess  x / 2 is exact, so fma(x, 0.5, 0.5) = fl(x / 2 + 0.5); clamp; fl(v * 255) and round-half-even: bit-equal
                      to the torch spelling.  NaN stays NaN in the float modes (compared as "NaN at the same places"), is 0 in
                      the uint8 mode; +-inf clamp
  flow_to_image       every step but one is a correctly rounded fp32 / fp64 operation in the order numpy takes it
                      (``flow_ref`` is bit-equal to oracle.output.flow_to_image, asserted on the CPU).  The one exception is the
                      angle: the device atan2f is taken as 2 ulp (HIP math documentation, not verified here), numpy's own and
                      the division by pi add up to 4 ulp of a = atan2 / pi, taken as delta = 2^-22 absolute for |a| <= 1.  A
                      byte passes between the smallest and the largest reference byte over a - delta, a, a + delta and the
                      integer fk between them where there is one (the colour is piecewise linear in fk with kinks at the
                      integers).  Small cases: seeds chosen so that no byte moves under +-delta (asserted on the CPU) -- the
                      output is bit-equal.  513 x 512: at most 1e-4 of the bytes differ from the unperturbed reference, whose
                      own +-delta share is asserted <= 5e-5.  The axes family (u or v = +-0.0) is bit-equal without that
                      assertion: atan2 of an exact axis is 0, +-pi/2 or +-pi, which a 2-ulp atan2f may miss -- a finding then
                      NaN pixels: black, excluded from the maximum, everything else as if they held zero flow (the contract
                      of include/mofa_hip.h; the reference's own max(-1, nan) accident is not copied)

Mutants (``MUTANTS``; ``mutant_differs`` states from the geometry alone where each computes something else).
``s-not-rounded`` (t from the exact product scale * o: what a fused ``scale * o - floor(s)`` gives) moves t by up to half an
ulp of s, 2^e u32 for s in [2^e, 2^(e+1)), and the result by that times sum |dw/dt| |v| <= 4.2 |v| (0.75 + 1.35 + 1.35 + 0.75);
the derived bound is about 250 u32 |v| (16 taps, eps_end on half of them, both axes).  Up to in = 24 (e <= 4) the mutant moves
the result by at most 68 u32 |v|: the check cannot see it.  At in = 256 (e = 7: up to 540 u32 |v|) it can, at in = 4097 (e = 11)
it does so sixteen times over: the table holds that axis next to the issue's 256, the rule is in - 1 >= 128."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

import aux_cases as ac
import op_cases as oc
from aux_cases import U32, Want, _nchw_view, check_want, round16
from op_cases import F16, F32, NAN, View, _f, _ints, bits

F64, U8 = torch.float64, torch.uint8
INF = float("inf")
CANARY = 0xA5
WS_BYTES = 1025 * 4                                                  # mofa_flow_to_image_ws_bytes (asserted on the GPU)
MAXRAD_BLOCKS = 1024                                                 # csrc/output.hip: the first pass covers 1024 * 256 pixels
FIRST_PASS = MAXRAD_BLOCKS * 256
DELTA = 2.0 ** -22
BIG_FRAC, BIG_OWN_FRAC = 1e-4, 5e-5
EPS_W = torch.tensor([38.0, 10.0, 10.0, 38.0], dtype=F64) * U32

MUTANTS = ("reflect-symmetric", "front-rear-swapped", "axis-swapped", "cubic-A-0.5", "bicubic-ac-false", "taps-unclamped",
           "s-not-rounded", "patch-px-py-swapped", "patch-channel-last", "nearest-exact-ratio", "nearest-round", "maxrad-first-pass",
           "maxrad-whole-blocks", "no-k1-wrap", "unknown-counts-in-max", "nan-not-black", "post-nan-to-zero")
MUTANT_OPS = {"reflect-symmetric": ("filter1d_reflect",), "front-rear-swapped": ("filter1d_reflect",), "axis-swapped": ("filter1d_reflect",),
              "cubic-A-0.5": ("resize_bicubic_ac",), "bicubic-ac-false": ("resize_bicubic_ac",), "taps-unclamped": ("resize_bicubic_ac",),
              "s-not-rounded": ("resize_bicubic_ac",), "patch-px-py-swapped": ("patchify",), "patch-channel-last": ("patchify",),
              "nearest-exact-ratio": ("resize_nearest_f32",), "nearest-round": ("resize_nearest_f32",),
              "maxrad-first-pass": ("flow_to_image",), "maxrad-whole-blocks": ("flow_to_image",), "no-k1-wrap": ("flow_to_image",),
              "unknown-counts-in-max": ("flow_to_image",), "nan-not-black": ("flow_to_image",), "post-nan-to-zero": ("frames_postprocess",)}


class ByteWant:
    """a uint8 output: every byte within [lo, hi], at most ``frac`` of them different from ``ref``"""

    def __init__(self, ref, lo=None, hi=None, frac=0.0):
        self.ref, self.lo, self.hi, self.frac = ref, (ref if lo is None else lo), (ref if hi is None else hi), frac


class ImgCase(oc.Case):
    """``ref(kw)`` -> the Want / ByteWant of ``out`` from the call's own arguments (CPU copies taken before the call); ``meta``:
    the geometry the mutant rules and the table invariants read; ``big``: a 513 x 512 flow"""

    def __init__(self, id, op, build, ref, big=False, **meta):
        super().__init__(id, op, build, None)
        self.ref, self.big, self.meta = ref, big, meta


def run_case(module, case, device="cpu"):
    r = oc.run(module, case, device)
    r.writes = tuple(n for n in ("out", "ws") if n in r.placed)
    return r


def _raw(t):
    return t if t.dtype == U8 else bits(t)


def guard_errors(r):
    """``op_cases.Run.guard_errors`` for buffers that may hold bytes: what the call changed that it must not"""
    bad = []
    for name, p in r.placed.items():
        diff = _raw(p.buf) != _raw(p.snap)
        if name in r.writes:
            diff = diff & ~p.inside
        n = int(diff.sum())
        if n:
            kind = "the guard of " if name in r.writes else "read-only "
            bad.append(f"{r.case.id}: {n} elements of {kind}{name} changed, first at {torch.nonzero(diff)[0].tolist()}")
    return bad


def check_out(what, g, w):
    """one output against its Want / ByteWant -> (worst err / bound, [messages])"""
    if isinstance(w, ByteWant):
        if g.dtype != U8 or g.shape != w.ref.shape:
            return INF, [f"{what}: {tuple(g.shape)} / {g.dtype} returned, uint8 {tuple(w.ref.shape)} expected"]
        errs = []
        out = (g < w.lo) | (g > w.hi)
        if bool(out.any()):
            i = torch.nonzero(out)[0].tolist()
            errs.append(f"{what}: {int(out.sum())} / {g.numel()} bytes outside their range, first at {i}: {int(g[tuple(i)])} for "
                        f"[{int(w.lo[tuple(i)])}, {int(w.hi[tuple(i)])}]")
        share = float((g != w.ref).double().mean()) if g.numel() else 0.0
        if share > w.frac:
            errs.append(f"{what}: {share:.3e} of the bytes differ from the reference, {w.frac:g} allowed")
        return (share / w.frac if w.frac else (INF if share else 0.0)), errs
    if w.bits is not None and w.bits.dtype == U8:
        if g.dtype != U8 or g.shape != w.bits.shape:
            return INF, [f"{what}: {tuple(g.shape)} / {g.dtype} returned, uint8 {tuple(w.bits.shape)} expected"]
        diff = g != w.bits
        if bool(diff.any()):
            i = torch.nonzero(diff)[0].tolist()
            return INF, [f"{what}: {int(diff.sum())} / {g.numel()} bytes differ, first at {i}: {int(g[tuple(i)])} for {int(w.bits[tuple(i)])}"]
        return 0.0, []
    if w.bits is not None and bool(torch.isnan(w.bits).any()):       # NaN at the same places, the rest bit-equal
        if g.shape != w.bits.shape or g.dtype != w.bits.dtype:
            return INF, [f"{what}: {tuple(g.shape)} / {g.dtype} returned, {tuple(w.bits.shape)} expected"]
        gn, wn = torch.isnan(g), torch.isnan(w.bits)
        if bool((gn != wn).any()):
            i = torch.nonzero(gn != wn)[0].tolist()
            return INF, [f"{what}: {int((gn != wn).sum())} elements are NaN on one side only, first at {i}: {g[tuple(i)].item()!r} for "
                         f"{w.bits[tuple(i)].item()!r}"]
        return check_want(what, torch.where(gn, torch.zeros_like(g), g), Want(bits=torch.where(wn, torch.zeros_like(w.bits), w.bits)))
    return check_want(what, g, w)


def check_run(case, r):
    """-> (worst err / bound, [messages]): guards, then ``out`` against ``case.ref``"""
    errs = guard_errors(r)
    worst, e = check_out(case.id, r.placed["out"].t.detach().cpu(), case.ref(ac.inputs_of(r)))
    return worst, errs + e


def _out_view(shape, dtype=F32, pre=8, post=40):
    n = int(np.prod(shape))
    base = torch.full((pre + n + post,), CANARY if dtype == U8 else NAN, dtype=dtype)
    return View(base, lambda b: b[pre:pre + n].view(shape))


def _vec_view(data, pre=3, post=11):
    """a 1-D fp32 argument (the filter taps) inside a NaN buffer"""
    return _nchw_view(data, pre=pre, post=post)


def _grid(*shape, seed=0, step=64):
    """fp32 values on the 1 / step grid, |v| <= 8"""
    return _ints(-8 * step, 8 * step, *shape, seed=seed) / step


# ---------------------------------------------------------------------------------------------------------------------------
# filter1d_reflect
# ---------------------------------------------------------------------------------------------------------------------------
def reflect_index(i, n, defect=None):
    if defect == "reflect-symmetric":                                # index -1 -> 0: the edge pixel repeated
        j = torch.where(i < 0, -i - 1, torch.where(i >= n, 2 * n - 1 - i, i))
    else:
        j = torch.where(i < 0, -i, torch.where(i >= n, 2 * (n - 1) - i, i))
    return j.clamp(0, n - 1)                                         # (only a mutant leaves the range)


def filter_ref(x64, taps64, axis, defect=None):
    """x64 [P, H, W] -> (sum_j tap_j x[reflect(o + j - front)], sum_j |tap_j x_j|) along W (axis 1) or H (axis 0)"""
    if defect == "axis-swapped":
        axis = 1 - axis
    k = taps64.numel()
    front = (k - 1) // 2
    if defect == "front-rear-swapped":
        front = k - 1 - front
    n = x64.shape[1 + axis]
    o = torch.arange(n)
    out, mag = torch.zeros_like(x64), torch.zeros_like(x64)
    for j in range(k):
        g = x64.index_select(1 + axis, reflect_index(o + j - front, n, defect)) * taps64[j]
        out, mag = out + g, mag + g.abs()
    return out, mag


def filter_fp32_is_exact(x, taps, axis):
    """the kernel's fp32 chain acc = tap_j * x_j + acc gives the fp64 sum exactly (every product then is exact, so the fused
    and the unfused chain are the same)"""
    P = x.numel() // (x.shape[-2] * x.shape[-1])
    x3 = x.reshape(P, *x.shape[-2:])
    k, n = taps.numel(), x3.shape[1 + axis]
    front, o = (k - 1) // 2, torch.arange(n)
    acc = torch.zeros_like(x3)
    for j in range(k):
        prod = taps[j] * x3.index_select(1 + axis, reflect_index(o + j - front, n))
        if not bool((prod.double() == taps[j].double() * x3.index_select(1 + axis, reflect_index(o + j - front, n)).double()).all()):
            return False
        acc = prod + acc
    return bool((acc.double() == filter_ref(x3.double(), taps.double(), axis)[0]).all())


def production_taps():
    """the two tap sets of the 576 x 1024 -> 224 x 224 conditioning resize"""
    from mofa_video_amd.frontend import _gaussian_taps, blur_geometry
    (ky, kx), (sy, sx) = blur_geometry(576, 1024, (224, 224))
    return {ky: _gaussian_taps(ky, sy, "cpu"), kx: _gaussian_taps(kx, sx, "cpu")}


def _rand_taps(k, seed):
    t = torch.rand(k, generator=torch.Generator().manual_seed(seed)) + 0.1
    return t / t.sum()


DYADIC_TAPS = {3: (0.25, 0.5, 0.25), 4: (0.125, 0.375, 0.375, 0.125)}


def _filter_case(tag, H, W, k, axis, kind="gauss", seed=0):
    """kind: gauss (random taps) | copy (k = 1, tap 1.0) | exact (dyadic taps, grid data) | production (the Gaussian taps)"""
    lead = (2, 3)

    def build():
        if kind == "exact":
            x, taps = _grid(*lead, H, W, seed=seed), torch.tensor(DYADIC_TAPS[k])
        else:
            x = _f(*lead, H, W, seed=seed, scale=2.0)
            taps = torch.ones(1) if kind == "copy" else (production_taps()[k] if kind == "production" else _rand_taps(k, seed + 1))
        return dict(x=_nchw_view(x), taps=_vec_view(taps), axis=axis, out=_out_view((*lead, H, W)))

    def ref(kw):
        x = kw["x"]
        y, mag = filter_ref(x.double().reshape(-1, H, W), kw["taps"].double(), axis)
        y, mag = y.reshape(x.shape), mag.reshape(x.shape)
        if kind == "copy":
            return Want(bits=x.clone())
        if kind == "exact":
            return Want(bits=y.float())
        return Want(ref=y, bound=k * U32 * mag)
    size = W if axis == 1 else H
    return ImgCase(f"filter1d_reflect/{tag}-{H}x{W}-k{k}-axis{axis}", "filter1d_reflect", build, ref, H=H, W=W, k=k, axis=axis, kind=kind,
                   size=size, rear=k - 1 - (k - 1) // 2, items=6 * H * W)


# ---------------------------------------------------------------------------------------------------------------------------
# resize_bicubic_ac
# ---------------------------------------------------------------------------------------------------------------------------
def cubic_coords(n_in, n_out, defect=None):
    """-> (i0 int64 [n_out], t fp64 [n_out]): floor and fraction of the align_corners=True source coordinate, taken IN fp32"""
    d = torch.arange(n_out, dtype=F32)
    if defect == "bicubic-ac-false":
        s = (d + 0.5) * torch.tensor(float(n_in) / float(n_out), dtype=F32) - 0.5
    else:
        scale = torch.tensor(float(n_in - 1), dtype=F32) / torch.tensor(float(n_out - 1), dtype=F32) if n_out > 1 else torch.tensor(0.0)
        s = scale.double() * d.double() if defect == "s-not-rounded" else scale * d
    f = torch.floor(s)
    return f.to(torch.int64), (s - f).clamp(0.0, 1.0).double()


def cubic_weights(t, A=-0.75):
    """Keys' cubic convolution weights of the taps at floor(s) - 1 .. floor(s) + 2 -> [n, 4], in the dtype of ``t``"""
    x0, x1, x2, x3 = t + 1, t, 1 - t, 2 - t
    return torch.stack([((A * x0 - 5 * A) * x0 + 8 * A) * x0 - 4 * A, ((A + 2) * x1 - (A + 3)) * x1 * x1 + 1,
                        ((A + 2) * x2 - (A + 3)) * x2 * x2 + 1, ((A * x3 - 5 * A) * x3 + 8 * A) * x3 - 4 * A], 1)


def _gather16(v, Hin, Win, iy, ix, clamp=True):
    """v [P, Hin, Win] -> [P, Hout, 4, Wout, 4]; unclamped: through the flat buffer, a NaN guard on either side"""
    P = v.shape[0]
    if clamp:
        return v[:, iy.clamp(0, Hin - 1)[:, :, None, None], ix.clamp(0, Win - 1)[None, None, :, :]]
    pad = 2 * Win + 3                                                # rows -1 .. Hin + 1, columns -1 .. Win + 1
    flat = torch.cat([torch.full((pad,), NAN, dtype=v.dtype), v.reshape(-1), torch.full((pad,), NAN, dtype=v.dtype)])
    idx = (torch.arange(P) * Hin * Win)[:, None, None, None, None] + (iy * Win)[None, :, :, None, None] + ix[None, None, None, :, :] + pad
    return flat[idx]


def bicubic_ref(v64, Hout, Wout, defect=None):
    """v64 [P, Hin, Win] -> (fp64 blend [P, Hout, Wout], its derived bound)"""
    P, Hin, Win = v64.shape
    A = -0.5 if defect == "cubic-A-0.5" else -0.75
    (y0, ty), (x0, tx) = cubic_coords(Hin, Hout, defect), cubic_coords(Win, Wout, defect)
    wy, wx = cubic_weights(ty, A), cubic_weights(tx, A)
    iy, ix = y0[:, None] - 1 + torch.arange(4)[None], x0[:, None] - 1 + torch.arange(4)[None]
    g = _gather16(v64, Hin, Win, iy, ix, clamp=defect != "taps-unclamped")
    out = (g * wy[None, :, :, None, None] * wx[None, None, None, :, :]).sum((2, 4))

    def mag(a, b):
        return (g.abs() * a[None, :, :, None, None] * b[None, None, None, :, :]).sum((2, 4))
    bound = mag(wy.abs() + EPS_W, wx.abs() + EPS_W) * (1 + 10 * U32) - mag(wy.abs(), wx.abs())
    return out, bound


def bicubic_fp32_is_exact(v, Hout, Wout):
    """the kernel's own fp32 order -- Horner weights, the row's dot product left to right, times wy, summed over the rows -- gives
    the fp64 blend exactly (every intermediate then is exact, fused or not)"""
    P, Hin, Win = v.shape
    (y0, ty), (x0, tx) = cubic_coords(Hin, Hout), cubic_coords(Win, Wout)
    wy, wx = cubic_weights(ty.float()), cubic_weights(tx.float())
    if not (bool((wy.double() == cubic_weights(ty)).all()) and bool((wx.double() == cubic_weights(tx)).all())):
        return False
    iy, ix = y0[:, None] - 1 + torch.arange(4)[None], x0[:, None] - 1 + torch.arange(4)[None]
    g = _gather16(v, Hin, Win, iy, ix)
    acc = torch.zeros(P, Hout, Wout)
    for a in range(4):
        row = torch.zeros(P, Hout, Wout)
        for j in range(4):
            row = row + g[:, :, a, :, j] * wx[None, None, :, j]
        acc = acc + row * wy[None, :, a, None]
    return bool((acc.double() == bicubic_ref(v.double(), Hout, Wout)[0]).all())


BICUBIC_PAIRS = [((1, 1), (4, 6)), ((3, 5), (1, 1)), ((5, 7), (5, 7)), ((3, 5), (9, 17)), ((2, 3), (16, 24)), ((16, 24), (4, 6)),
                 ((11, 13), (7, 19)), ((256, 4), (100, 9)), ((3, 4097), (2, 1500))]
BICUBIC_EXACT = ((3, 5), (9, 17))


def _bicubic_case(pair, seed, exact=False):
    (Hin, Win), (Hout, Wout) = pair
    lead = (2, 3)
    identity = (Hin, Win) == (Hout, Wout)

    def build():
        x = _grid(*lead, Hin, Win, seed=seed, step=4) if exact else _f(*lead, Hin, Win, seed=seed, scale=2.0)
        return dict(x=_nchw_view(x), out=_out_view((*lead, Hout, Wout)))

    def ref(kw):
        x = kw["x"]
        if identity:
            return Want(bits=x.clone())
        y, bound = bicubic_ref(x.double().reshape(-1, Hin, Win), Hout, Wout)
        shape = (*lead, Hout, Wout)
        return Want(bits=y.float().reshape(shape)) if exact else Want(ref=y.reshape(shape), bound=bound.reshape(shape))
    tag = f"resize_bicubic_ac/{Hin}x{Win}-to-{Hout}x{Wout}" + ("-exact" if exact else "")
    return ImgCase(tag, "resize_bicubic_ac", build, ref, pair=pair, exact=exact, items=6 * Hout * Wout)


# ---------------------------------------------------------------------------------------------------------------------------
# patchify
# ---------------------------------------------------------------------------------------------------------------------------
PATCH_SHAPES = [(2, 3, 28, 42, 14, 640), (2, 3, 28, 42, 14, 588), (1, 3, 14, 14, 14, 592), (2, 5, 6, 9, 1, 8), (2, 3, 8, 12, 2, 16)]
PATCH_PLANTS = (70000.0, -70000.0, 65520.0, 65519.0, 1e-8, 3e-6, -0.0)   # inf, -inf, inf (the tie), 65504, 0, a subnormal, -0


def patch_ref(x, p, ld, defect=None):
    """fp32 [n, C, H, W] -> fp16 [n (H/p) (W/p), ld]: column c p p + py p + px, zero beyond"""
    n, C, H, W = x.shape
    cols = F.unfold(x.double(), kernel_size=p, stride=p).transpose(1, 2).reshape(-1, C, p, p)
    if defect == "patch-px-py-swapped":
        cols = cols.transpose(2, 3)
    elif defect == "patch-channel-last":
        cols = cols.permute(0, 2, 3, 1)
    out = torch.zeros(cols.shape[0], ld, dtype=F16)
    out[:, :C * p * p] = round16(cols.reshape(-1, C * p * p).contiguous())
    return out


def _patch_case(shape, seed):
    n, C, H, W, p, ld = shape

    def build():
        x = _f(n, C, H, W, seed=seed, scale=3.0)
        flat = x.view(-1)
        for i, val in enumerate(PATCH_PLANTS):                       # spread over the images, channels and patch positions
            flat[(i * 37 + 5) % flat.numel()] = val
        rows = n * (H // p) * (W // p)
        return dict(x=_nchw_view(x), p=p, out=_out_view((rows, ld), dtype=F16))

    def ref(kw):
        return Want(bits=patch_ref(kw["x"], p, ld))
    return ImgCase(f"patchify/n{n}-C{C}-{H}x{W}-p{p}-ld{ld}", "patchify", build, ref, shape=shape, items=n * (H // p) * (W // p) * ld)


# ---------------------------------------------------------------------------------------------------------------------------
# resize_nearest_f32
# ---------------------------------------------------------------------------------------------------------------------------
def nearest_index(n_in, n_out, defect=None):
    o = torch.arange(n_out)
    if defect == "nearest-exact-ratio":
        return (o * n_in) // n_out
    if defect == "nearest-round":
        return torch.floor(o.double() * n_in / n_out + 0.5).long().clamp(max=n_in - 1)
    scale = torch.tensor(float(n_in), dtype=F32) / torch.tensor(float(n_out), dtype=F32)
    return torch.floor(o.to(F32) * scale).long().clamp(max=n_in - 1)


def nearest_ref(x, h, w, defect=None):
    return x[:, nearest_index(x.shape[1], h, defect)][:, :, nearest_index(x.shape[2], w, defect)].contiguous()


SWEEP_SIZES = range(1, 25)
_PAIRS = [(i, o) for i in SWEEP_SIZES for o in SWEEP_SIZES]
# every (in, out) pair of 1..24 once: launch j takes pair 2 j along H and pair 2 j + 1 along W -> (H, W, h, w)
NEAREST_SWEEP = [(_PAIRS[2 * j][0], _PAIRS[2 * j + 1][0], _PAIRS[2 * j][1], _PAIRS[2 * j + 1][1]) for j in range(len(_PAIRS) // 2)]
NEAREST_TABLE = [(48, 80, 7, 11), (48, 80, 6, 10), (48, 80, 12, 20), (48, 80, 24, 40),      # production-like downscales
                 (5, 7, 5, 7), (3, 5, 7, 16), (1, 1, 4, 6), (7, 24, 1, 23), (24, 17, 23, 3),
                 (2, 5, 82, 3)]    # 2 -> 82: fl(fl(2 / 82) * 41) < 1, the one place up to here where the fp32 rule is not the integer one


def nearest_data(n, H, W, seed):
    """distinct values, so a wrong source index is a wrong value"""
    return (torch.randperm(n * H * W, generator=torch.Generator().manual_seed(seed)).float() + 0.5).reshape(n, H, W)


def _nearest_case(H, W, h, w, seed):
    n = 2

    def build():
        return dict(x=_nchw_view(nearest_data(n, H, W, seed)), out=_out_view((n, h, w)))

    def ref(kw):
        return Want(bits=nearest_ref(kw["x"], h, w))
    return ImgCase(f"resize_nearest_f32/{H}x{W}-to-{h}x{w}", "resize_nearest_f32", build, ref, sizes=(H, W, h, w), items=n * h * w)


# ---------------------------------------------------------------------------------------------------------------------------
# frames_postprocess
# ---------------------------------------------------------------------------------------------------------------------------
POST_PLANTS = (INF, -INF, -0.0, 0.0, 1.0, -1.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, -1.0 + 2.0 ** -24, -1.0 - 2.0 ** -23, 5.0, -5.0)


def post_data(n, H, W, seed):
    """Gaussian x 1.3; one pixel column of specials; the (k + 0.5) / 255 ties; NaN in every channel and frame"""
    x = _f(n, 3, H, W, seed=seed, scale=1.3)
    flat = x.view(-1)
    ties = [2 * (k + 0.5) / 255 - 1 for k in range(0, 255, 2 if flat.numel() > 600 else 13)]
    vals = list(POST_PLANTS) + ties
    stride = max(1, (flat.numel() - 7) // len(vals))
    for i, val in enumerate(vals):
        flat[(3 + i * stride) % flat.numel()] = val
    for f in range(n):
        for c in range(3):
            x[f, c, (f + c) % H, (2 * c + f) % W] = NAN
    return x


def post_ref(x, mode, defect=None):
    v = (x / 2 + 0.5).clamp(0, 1)                                    # torch's clamp propagates NaN
    if defect == "post-nan-to-zero":
        v = torch.nan_to_num(v, nan=0.0)
    if mode == 0:
        return v
    v = v.permute(0, 2, 3, 1).contiguous()
    if mode == 1:
        return v
    return torch.nan_to_num(v * 255, nan=0.0).round().to(U8)         # round-half-even, as numpy's


def _post_case(n, H, W, mode, seed):
    def build():
        shape, dtype = ((n, 3, H, W), F32) if mode == 0 else ((n, H, W, 3), F32 if mode == 1 else U8)
        return dict(frames=_nchw_view(post_data(n, H, W, seed)), mode=mode, out=_out_view(shape, dtype=dtype))

    def ref(kw):
        return Want(bits=post_ref(kw["frames"], mode))
    return ImgCase(f"frames_postprocess/mode{mode}-n{n}-{H}x{W}", "frames_postprocess", build, ref, mode=mode, items=n * H * W)


# ---------------------------------------------------------------------------------------------------------------------------
# flow_to_image
# ---------------------------------------------------------------------------------------------------------------------------
NCOLS = 55


def _sqrt32(t):
    """the correctly rounded fp32 root, as oracle.output takes it: numpy's, whatever vector library torch.sqrt uses on this host"""
    return torch.from_numpy(np.sqrt(t.contiguous().numpy()))


@functools.lru_cache(None)
def _wheel():
    """the Middlebury colour wheel [55, 3] (make_color_wheel), with a NaN row behind it for the mutant that does not wrap"""
    seg = (15, 6, 4, 11, 13, 6)                                      # RY YG GC CB BM MR
    cw, col = np.zeros((NCOLS + 1, 3)), 0
    for s, n in enumerate(seg):
        ramp = np.floor(255 * np.arange(n) / n)
        a, b = (s // 2) % 3, (s // 2 + 1) % 3                        # the full channel / the next one of the segment pair
        if s % 2 == 0:
            cw[col:col + n, a], cw[col:col + n, b] = 255, ramp
        else:
            cw[col:col + n, a], cw[col:col + n, b] = 255 - ramp, 255
        col += n
    cw[NCOLS] = np.nan
    return cw


def _fk(a):
    return (a + 1) / 2 * (NCOLS - 1) + 1                             # fp32 throughout, as numpy keeps it


def _bytes(k0, f, rad, wrap=True):
    cw = _wheel()
    k1 = k0 + 1
    if wrap:
        k1 = np.where(k1 == NCOLS + 1, 1, k1)
    out = np.zeros(k0.shape + (3,), np.uint8)
    with np.errstate(invalid="ignore"):
        for i in range(3):
            col0, col1 = cw[k0 - 1, i] / 255, cw[k1 - 1, i] / 255
            col = (1 - f) * col0 + f * col1
            col = np.where(rad <= 1, 1 - rad * (1 - col), col * 0.75)
            val = np.floor(255 * col)
            out[..., i] = np.where(np.isnan(val), 0, val).astype(np.uint8)
    return out


def flow_normalised(flow, defect=None):
    """-> (u / den, v / den as fp32 numpy [H, W], mask of the black pixels): flow_to_image up to the call of compute_color"""
    fl = flow.clone()
    u, v = fl[..., 0], fl[..., 1]
    nanpix = torch.isnan(u) | torch.isnan(v)
    unknown = (u.abs() > 1e7) | (v.abs() > 1e7)
    gone = unknown | nanpix
    rad_raw = _sqrt32(u ** 2 + v ** 2)
    u[gone] = 0
    v[gone] = 0
    rad = _sqrt32(u ** 2 + v ** 2).reshape(-1)
    n = rad.numel()
    if defect == "unknown-counts-in-max":
        rad = torch.where(nanpix, torch.zeros(()), rad_raw).reshape(-1)
    elif defect == "maxrad-first-pass":
        rad = rad[:FIRST_PASS]
    elif defect == "maxrad-whole-blocks":
        rad = rad[:n // 256 * 256]
    maxrad = np.float32(max(-1.0, float(rad.max()) if rad.numel() else -1.0))
    den = float(np.float32(np.float64(maxrad) + np.finfo(float).eps))
    return (u / den).numpy(), (v / den).numpy(), (unknown if defect == "nan-not-black" else gone).numpy()


def flow_ref(flow, defect=None, ranges=False):
    """flow fp32 [H, W, 2] -> uint8 [H, W, 3] as numpy computes flow_viz.py's flow_to_image, NaN pixels as include/mofa_hip.h
    states; ``ranges``: -> (ref, lo, hi), the smallest and largest byte over the angle moved by -+DELTA"""
    un, vn, black = flow_normalised(flow, defect)
    radn = np.sqrt(un ** 2 + vn ** 2)
    a = (np.arctan2(-vn, -un) / np.pi).astype(np.float32)

    def image(fk, k0=None):
        snap = k0 is not None
        k0 = np.floor(fk).astype(np.int64) if k0 is None else k0
        f = np.zeros(fk.shape) if snap else fk - k0
        img = _bytes(k0, f, radn, wrap=defect != "no-k1-wrap")
        img[black] = 0
        return img
    ref = image(_fk(a))
    if not ranges:
        return torch.from_numpy(ref)
    fks = [_fk(np.clip(a + np.float32(d), -1, 1).astype(np.float32)) for d in (-DELTA, DELTA)]
    imgs = [ref] + [image(fk) for fk in fks]
    k_lo, k_hi = np.floor(fks[0]).astype(np.int64), np.floor(fks[1]).astype(np.int64)
    kink = image(fks[1], k0=k_hi)                                     # fk = the integer between a - delta and a + delta, f = 0
    cross = (k_hi > k_lo)[..., None]
    lo = np.minimum.reduce(imgs + [np.where(cross, kink, ref)])
    hi = np.maximum.reduce(imgs + [np.where(cross, kink, ref)])
    return torch.from_numpy(ref), torch.from_numpy(lo), torch.from_numpy(hi)


def radius(flow):
    """fp32 radius per pixel [H * W] with unknown and NaN pixels at 0, as the maximum takes it"""
    u, v = flow[..., 0].clone(), flow[..., 1].clone()
    gone = (u.abs() > 1e7) | (v.abs() > 1e7) | torch.isnan(u) | torch.isnan(v)
    u[gone] = 0
    v[gone] = 0
    return _sqrt32(u ** 2 + v ** 2).reshape(-1)


def _plant_max(flow, pos):
    """the pixel at flat index ``pos`` becomes the only largest: its own direction, 1.5 times the largest radius"""
    flat = flow.view(-1, 2)
    r = radius(flow)
    flat[pos] = flat[pos] / r[pos] * (1.5 * r.max())
    return flow


@functools.lru_cache(None)
def radgt1_direction():
    """a flow vector p whose own normalisation p / fl(|p| + eps) has an fp32 radius ABOVE 1 (rounding alone; about 0.75 % of the
    directions): the first of a seeded draw.  As the maximum pixel of a flow it takes compute_color's ``col *= 0.75`` branch"""
    p = torch.randn(4096, 2, generator=torch.Generator().manual_seed(7)) * 5
    r = _sqrt32(p[:, 0] ** 2 + p[:, 1] ** 2)
    den = (r.double() + np.finfo(float).eps).float()
    a, b = p[:, 0] / den, p[:, 1] / den
    hit = torch.nonzero(_sqrt32(a ** 2 + b ** 2) > 1)
    return p[int(hit[0])].clone()


def flow_data(kind, H, W, seed, maxpos=None):
    g = torch.Generator().manual_seed(seed)
    n = H * W
    if kind == "axes":       # u or v = +-0.0 with graded radii: fk = 1 (a = -1), 14.5, 28, 41.5 and 55 (a = +1: the wrap)
        flow = torch.zeros(n, 2)
        combos = [(1.0, 0.0), (1.0, -0.0), (-1.0, 0.0), (-1.0, -0.0), (0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0)]
        for i in range(min(n, 56)):
            cu, cv = combos[i % 8]
            flow[i, 0], flow[i, 1] = cu * (i // 8 + 1) / 8, cv * (i // 8 + 1) / 8
        return flow.reshape(H, W, 2)
    if kind == "zero":
        flow = torch.zeros(n, 2)
        flow[::3] = -0.0
        return flow.reshape(H, W, 2)
    if kind == "tiny":
        return torch.randn(H, W, 2, generator=g) * 1e-20
    if kind == "all-unknown":
        flow = torch.full((n, 2), 2e7)
        flow[::2, 0], flow[1::3, 1], flow[::5, 1] = 1.0, -INF, INF
        flow[::2, 1] = -3e7
        return flow.reshape(H, W, 2)
    flow = torch.randn(H, W, 2, generator=g) * 4
    flat = flow.view(-1, 2)
    if kind == "radgt1":
        flow *= 0.05
        flat[maxpos] = radgt1_direction()
        return flow
    if kind == "unknown":    # the largest pixels are unknown and must not set the maximum; +-inf; a component of 1e7 is too large
        flat[3 % n] = torch.tensor([2e7, 1.0])                       # for the maximum but not unknown
        flat[10 % n] = torch.tensor([1.0, -2e7])
        flat[11 % n] = torch.tensor([INF, 0.0])
        flat[12 % n] = torch.tensor([0.0, -INF])
        flat[17 % n] = torch.tensor([-INF, INF])
        flat[n - 1] = torch.tensor([1.0000001e7, -1.0000001e7])
    elif kind == "exact-1e7":   # |u| == 1e7 exactly is NOT unknown: these pixels are the largest and are coloured
        flow *= 5e5
        flat[5 % n] = torch.tensor([1e7, -6e6])                      # (not 45 degrees: fk = 48.25 sits on a byte boundary)
        flat[6 % n] = torch.tensor([3e6, -1e7])
        flat[n - 2] = torch.tensor([-1e7, 2.5e6])
        flat[n // 2] = torch.tensor([1e7, 3e7])                       # ... and this one is unknown
    elif kind == "nan":      # NaN in u, in v, in both; the finite component of a NaN pixel is far larger than every radius
        flat[4 % n] = torch.tensor([NAN, 1e3])
        flat[n // 2] = torch.tensor([-1e3, NAN])
        flat[n - 1] = torch.tensor([NAN, NAN])
    if maxpos is not None:
        _plant_max(flow, maxpos)
    return flow


def _flow_case(kind, H, W, seed, maxpos=None, exact=None):
    big = H * W > FIRST_PASS
    n = H * W

    def build():
        ws = torch.full((64 + WS_BYTES + 256,), CANARY, dtype=U8)
        return dict(flow=_nchw_view(flow_data(kind, H, W, seed, maxpos)), out=_out_view((H, W, 3), dtype=U8),
                    ws=View(ws, lambda b: b[64:64 + WS_BYTES]))

    def ref(kw):
        if big:
            r, lo, hi = flow_ref(kw["flow"], ranges=True)
            return ByteWant(r, lo, hi, BIG_FRAC)
        return ByteWant(flow_ref(kw["flow"]))
    tag = f"flow_to_image/{kind}-{H}x{W}" + (f"-max@{maxpos}" if maxpos is not None else "") + f"-s{seed}"
    r = radius(flow_data(kind, H, W, seed, maxpos)) if not big else None
    where = (maxpos,) if big else tuple(torch.nonzero(r == r.max()).reshape(-1).tolist())
    return ImgCase(tag, "flow_to_image", build, ref, big=big, kind=kind, H=H, W=W, n=n, maxpos=where,
                   nonzero=True if big else bool(r.max() > 0), items=n)


# ---------------------------------------------------------------------------------------------------------------------------
# the references behind one calling convention: impl(None) is a correct implementation, impl(defect) a wrong one
# ---------------------------------------------------------------------------------------------------------------------------
def impl(defect=None):
    def filter1d_reflect(x, taps, axis, out):
        H, W = x.shape[-2:]
        out[...] = filter_ref(x.double().reshape(-1, H, W), taps.double(), axis, defect)[0].float().reshape(x.shape)

    def resize_bicubic_ac(x, out):
        H, W = x.shape[-2:]
        out[...] = bicubic_ref(x.double().reshape(-1, H, W), out.shape[-2], out.shape[-1], defect)[0].float().reshape(out.shape)

    def patchify(x, p, out):
        out[...] = patch_ref(x, p, out.shape[1], defect)

    def resize_nearest_f32(x, out):
        out[...] = nearest_ref(x, out.shape[1], out.shape[2], defect)

    def frames_postprocess(frames, mode, out):
        out[...] = post_ref(frames, mode, defect)

    def flow_to_image(flow, out, ws):
        out[...] = flow_ref(flow, defect)
    return types.SimpleNamespace(**{k: v for k, v in locals().items() if callable(v)})


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
BIG_HW = (513, 512)                                                  # 262656 pixels = 1026 blocks: 512 pixels in the second pass
FLOW_MAX_POSITIONS = {                                               # pixel 0, the last of a full block, the first of the ragged
    (1, 257): (0, 255, 256),                                         # tail, the last pixel; beyond the first pass
    (48, 64): (0, 255, 1500, 3071),
    (23, 31): (0, 511, 512, 712),
    BIG_HW: (0, 255, FIRST_PASS - 1, FIRST_PASS, 513 * 512 - 1),
}
# seeds: the first from 0 at which no byte of the reference moves when the angle moves by -+DELTA (tools: none -- the CPU test
# asserts the property, a seed that loses it fails there)
FLOW_SEEDS = {}


def _seed(key, default=0):
    return FLOW_SEEDS.get(key, default)


def _flow_cases():
    out = [_flow_case("gauss", 1, 1, _seed(("gauss", 1, 1, None))), _flow_case("gauss", 7, 9, _seed(("gauss", 7, 9, None))),
           _flow_case("gauss", 7, 9, _seed(("gauss", 7, 9, 62)), maxpos=62)]
    for (H, W), positions in FLOW_MAX_POSITIONS.items():
        out += [_flow_case("gauss", H, W, _seed(("gauss", H, W, p)), maxpos=p) for p in positions]
    out.append(_flow_case("axes", 7, 9, 0))
    for kind in ("radgt1", "unknown", "exact-1e7", "nan"):
        for H, W in ((7, 9), (23, 31)):
            mp = {"radgt1": H * W // 2, "nan": H * W - 3}.get(kind)
            out.append(_flow_case(kind, H, W, _seed((kind, H, W, mp)), maxpos=mp))
    out += [_flow_case(kind, 7, 9, 0) for kind in ("all-unknown", "zero", "tiny")]
    return out


CASES = (
    [_filter_case("copy", 5, 9, 1, ax, "copy", 500 + ax) for ax in (0, 1)]
    + [_filter_case("gauss", 5, 9, k, ax, seed=510 + 2 * k + ax) for k in (3, 7, 4) for ax in (0, 1)]
    + [_filter_case("largest", 3, 4, 7, 1, seed=530), _filter_case("largest", 3, 4, 5, 0, seed=531),
       _filter_case("largest", 3, 4, 6, 1, seed=532), _filter_case("largest", 4, 3, 6, 0, seed=533)]
    + [_filter_case("one-pixel", 1, 9, 3, 1, seed=540), _filter_case("one-pixel", 9, 1, 3, 0, seed=541),
       _filter_case("one-pixel", 1, 4, 6, 1, seed=542)]
    + [_filter_case("ragged", 11, 13, 5, 1, seed=550), _filter_case("ragged", 11, 13, 4, 0, seed=551)]
    + [_filter_case("exact", 5, 9, k, ax, "exact", 560 + 2 * k + ax) for k in (3, 4) for ax in (0, 1)]
    + [_filter_case("production", 3, 5, 7, 1, "production", 570), _filter_case("production", 3, 5, 3, 0, "production", 571),
       _filter_case("production", 11, 13, 7, 1, "production", 572)]
    + [_bicubic_case(pair, 600 + i) for i, pair in enumerate(BICUBIC_PAIRS)]
    + [_bicubic_case(BICUBIC_EXACT, 620, exact=True)]
    + [_patch_case(shape, 700 + i) for i, shape in enumerate(PATCH_SHAPES)]
    + [_nearest_case(*s, 800 + i) for i, s in enumerate(NEAREST_TABLE)]
    + [_post_case(n, H, W, mode, 900 + mode) for (n, H, W) in ((2, 5, 7), (3, 16, 24)) for mode in (0, 1, 2)]
    + _flow_cases()
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
OPS = tuple(dict.fromkeys(c.op for c in CASES))


def mutant_differs(defect, case):
    """from the geometry alone: does the wrong kernel ``defect`` compute something else than the right one on ``case``"""
    m = case.meta
    if case.op not in MUTANT_OPS[defect]:
        return False
    if defect in ("reflect-symmetric", "axis-swapped"):              # any tap beside the centre one reaches the padding of an
        return m["k"] > 1                                            # edge pixel / lies along the other axis
    if defect == "front-rear-swapped":
        return m["k"] % 2 == 0
    if defect in ("cubic-A-0.5", "bicubic-ac-false", "s-not-rounded"):
        (Hin, Win), (Hout, Wout) = m["pair"]
        axes = ((Hin, Hout), (Win, Wout))
        if defect == "cubic-A-0.5":        # the weights depend on A wherever t != 0
            return any(bool((cubic_coords(i, o)[1] != 0).any()) for i, o in axes)
        if defect == "bicubic-ac-false":   # the two coordinate rules agree only for an identity or a one-pixel source axis
            return any(i > 1 and i != o for i, o in axes)
        return any(i - 1 >= 128 and o > 1 for i, o in axes)          # (docstring: below the bound up to in = 24)
    if defect == "taps-unclamped":         # output pixel 0 of plane 0 reads row / column -1: the NaN guard, even at weight 0
        return True
    if defect == "patch-px-py-swapped":
        return m["shape"][4] > 1
    if defect == "patch-channel-last":
        return m["shape"][4] > 1 and m["shape"][1] > 1
    if defect in ("nearest-exact-ratio", "nearest-round"):
        H, W, h, w = m["sizes"]
        return any(bool((nearest_index(i, o, defect) != nearest_index(i, o)).any()) for i, o in ((H, h), (W, w)))
    if defect == "post-nan-to-zero":       # every case holds NaN; the uint8 mode writes 0 for it anyway
        return m["mode"] in (0, 1)
    if defect == "maxrad-first-pass":
        return m["nonzero"] and all(p >= FIRST_PASS for p in m["maxpos"])
    if defect == "maxrad-whole-blocks":
        return m["nonzero"] and all(p >= m["n"] // 256 * 256 for p in m["maxpos"])
    if defect == "no-k1-wrap":             # a pixel at the angle +pi exactly (v = -0.0, u > 0) with a radius: fk = 55, k1 = 56
        return m["kind"] == "axes"
    if defect == "unknown-counts-in-max":  # an unknown pixel is the largest, and there is a known one to rescale
        return m["kind"] in ("unknown", "exact-1e7")
    if defect == "nan-not-black":
        return m["kind"] == "nan"
    raise KeyError(defect)
