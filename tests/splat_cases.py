"""TEST INFRASTRUCTURE ONLY: the case table of the adapter's warp, ``mofa_softsplat_avg_f16`` (csrc/softsplat.hip: the five CSR
kernels count / scan / fill / sort / gather), with its own fp64 reference, the per-element bound, the exact families and the
"wrong kernel" mutants that prove the checks can fail.  The table is run on the CPU against ``standin(defect)``
(tests/test_splat_cases_cpu.py) and on the GPU against the kernels (tests/test_splat_matrix_gpu.py); a backend is a function
``splat(feat, flow, out, H, W)`` that fills ``out`` and returns a list of complaints of its own (the GPU one: the workspace).

Every run takes ``feat`` as a guarded view (``op_cases.guard``: NaN rows before and after, 8 NaN columns on the left, a leading
dimension larger than C) and a NaN-filled guarded ``out`` with another, larger leading dimension; the guards are compared as bits.

Reference (``entries`` + ``splat_sums``).  fx = fl32(x + flow_x), fy = fl32(y + flow_y): ONE IEEE addition, the same on both
sides.  A source with a non-finite fx or fy is skipped.  Everything after that in fp64: x0 = floor(fx), the corner weights
(x0 + 1 - fx)(y0 + 1 - fy), (fx - x0)(y0 + 1 - fy), (x0 + 1 - fx)(fy - y0), (fx - x0)(fy - y0) for NW, NE, SW, SE, each corner
tested against the plane on its own (a coordinate beyond the int range is not inside any plane), and per target
S = sum w v, A = sum w |v|, Nw = sum w, n = number of entries (zero-weight corners that lie in the plane ARE entries);
ref = S / (Nw + 1e-7).  ``oracle.softsplat`` is not used here; the CPU test ties the two together on the Gaussian cases.

Bound, with u16 = 2^-11, u32 = 2^-24, derived by counting the roundings of the kernel, never measured:
  * x0 + 1 - fx and fx - x0 are exact in fp32 for |fx| < 2^23 (x0 <= fx < x0 + 1 share a binade or Sterbenz applies), so every
    weight is ONE rounded product: w (1 + d), |d| <= u32;
  * the accumulator takes per entry one rounded product and one rounded sum, or one FMA (at most two roundings either way, in
    any order of the entries); the first addition, to 0, is exact.  With the weight's own rounding the numerator carries at most
    n + 1 roundings on every term: |S' - S| <= (n + 1) u32 A;
  * the norm is a sum of n rounded weights with n - 1 rounded additions: |N' - Nw| <= n u32 Nw (all weights are >= 0);
  * d = fl(N' + fl32(1e-7)): fl32(1e-7) is off by at most u32 1e-7, the sum rounds once -- 2 u32 relative to Nw + 1e-7;
  * the reciprocal (correctly rounded) and the product with it: 2 u32;
  * the fp16 rounding: u16 |result| for a normal, 2^-25 for a subnormal result.
  First order: (n + 1) + n + 2 + 2 = 2n + 5 roundings of fp32, each relative to A / (Nw + 1e-7) at most.  The bound is
      |out - ref| <= u16 |ref| + 2^-25 + (2n + 6) u32 A / (Nw + 1e-7),
  the constant 6 of the issue: the one unit above the count pays for the second-order terms, (2n + 5) u32 (u16 + (2n + 5) u32)
  <= u32, which holds for n <= ``N_MAX`` = 500 (1005 (2^-11 + 1005 * 2^-24) = 0.55); ``want`` asserts n <= N_MAX.  It holds
  for any summation order and with or without contraction.  A target with Nw = 0 (no entry, or zero-weight entries only) must be
  the VALUE 0: 0 * (1 / 1e-7).

Exact family (``exact=True``): flows on the 1/4 grid, features on the 2^-4 grid with |v| <= 4, at most ``N_EXACT`` = 64 entries
on a target.  Every weight is a multiple of 2^-4, every product of 2^-8 and at most 4, every partial sum at most 256 -- 17 bits
of the 24 of fp32: S and Nw are exact in fp32 in any order.  (16 entries would do for most of the table; the border frames that
send EVERY source of 7 x 9 to x = -1 or x = W - 1 put 18 on a target: the 9 sources of its row and the zero-weight south corners
of the 9 of the row above.  The argument needs 4 n 2^8 <= 2^24 only.)  What is left is d = fl(Nw + fl32(1e-7)), 1 / d, the
product and the fp16 rounding: the fp32 quotient lies within 4 u32 |ref| (first order) of ref, so wherever round16 is constant
on [ref (1 - 6 u32), ref (1 + 6 u32)] the output must EQUAL round16(ref).  Elements nearer than that to a rounding boundary are left out and counted per case (``LEFT_OUT``);
they may be at most 1 % (asserted on the reference alone by the CPU test).  The tiny-normaliser case is exact by the same
argument with one entry per target: v * 2^-k is exact.

Summation order (``norm_emulation``): ``mofa_softsplat_norm_f32`` shares the CSR and the sort and adds the fp32 weights with plain
fp32 additions, so on the segment-length cases it must be bit-equal to the sequential fp32 sum in key order
corner * HW + source.  The CPU test shows that the source-major order gives other bits on the same inputs.
"""
import numpy as np
import torch

import op_cases as oc
from aux_cases import round16
from op_cases import F16, F32, NAN, _h, _ints, guard

U16, U32 = 2.0 ** -11, 2.0 ** -24
F64 = torch.float64
EPS = 1e-7
INF = float("inf")
N_MAX, N_EXACT = 500, 64
PASS_CH = 512                                          # ss_gather_kernel: 64 lanes x 8 channels per pass of the channel loop
SCAN_THREADS = 1024                                    # ss_scan_kernel
SS_INSERTION_MAX = 48                                  # csrc/softsplat.hip: longer segments are heap-sorted

MUTANTS = ("eps-dropped", "eps-1e-6", "trunc-not-floor", "oob-clamped-to-border", "nonfinite-as-zero-flow", "swap-xy", "ne-sw-swapped",
           "last-channel-pass-stale", "second-pass-only-full", "flow0-csr-for-all", "segment-cut-at-48", "sum-not-avg",
           "scan-last-segment-dropped")


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
class Entries:
    """the CSR of one flow frame: per entry target, source, key = corner * HW + source, the fp64 weight and the weight as the
    kernel forms it in fp32; sorted by (target, key)"""

    def __init__(self, tgt, src, key, w64, w32, HW):
        self.tgt, self.src, self.key, self.w64, self.w32, self.HW = tgt, src, key, w64, w32, HW

    def take(self, idx):
        return Entries(self.tgt[idx], self.src[idx], self.key[idx], self.w64[idx], self.w32[idx], self.HW)

    def rank(self):
        """position of every entry in its target's segment"""
        return np.arange(len(self.tgt)) - np.searchsorted(self.tgt, self.tgt, "left")


def entries(flow, H, W, defect=None):
    """flow fp32 [2, H, W] -> Entries (``defect``: one of MUTANTS, a wrong kernel)"""
    HW = H * W
    f = flow.detach().cpu().numpy().astype(np.float32).reshape(2, H, W)
    if defect == "swap-xy":
        f = f[::-1]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    with np.errstate(all="ignore"):
        fx, fy = xs + f[0], ys + f[1]                                 # fp32: one rounded addition each
        assert fx.dtype == np.float32 and fy.dtype == np.float32
        live = np.isfinite(fx) & np.isfinite(fy)
        if defect == "nonfinite-as-zero-flow":
            fx, fy = np.where(np.isfinite(fx), fx, xs), np.where(np.isfinite(fy), fy, ys)
            live = np.ones_like(live)
        fx, fy = np.where(live, fx, np.float32(0)), np.where(live, fy, np.float32(0))
        X, Y = fx.astype(np.float64), fy.astype(np.float64)
        fl = np.trunc if defect == "trunc-not-floor" else np.floor
        x0, y0 = fl(X), fl(Y)
        wx, wy = (x0 + 1 - X, X - x0), (y0 + 1 - Y, Y - y0)
        x0f, y0f, x1f, y1f = (a.astype(np.float32) for a in (x0, y0, x0 + 1, y0 + 1))
        wx32, wy32 = (x1f - fx, fx - x0f), (y1f - fy, fy - y0f)
        src = np.arange(HW, dtype=np.int64).reshape(H, W)
        cols = []
        for k in range(4):
            ix, iy = k & 1, k >> 1
            kw = 3 - k if defect == "ne-sw-swapped" and k in (1, 2) else k
            w64 = wx[kw & 1] * wy[kw >> 1]
            w32 = wx32[kw & 1] * wy32[kw >> 1]                        # fp32: one rounded product of two exact factors
            cx, cy = x0 + ix, y0 + iy
            if defect == "oob-clamped-to-border":
                cx, cy, ok = np.clip(cx, 0, W - 1), np.clip(cy, 0, H - 1), live
            else:
                ok = live & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
            t = (np.where(ok, cy, 0) * W + np.where(ok, cx, 0)).astype(np.int64)
            cols.append((t[ok], src[ok], k * HW + src[ok], w64[ok], w32[ok].astype(np.float32)))
    tgt, s, key, w64, w32 = (np.concatenate([c[i] for c in cols]) for i in range(5))
    e = Entries(tgt, s, key, w64, w32, HW).take(np.lexsort((key, tgt)))
    if defect == "scan-last-segment-dropped":                         # the targets of the last, partly filled run of 1024 get nothing
        cut = SCAN_THREADS * (HW // SCAN_THREADS)
        if SCAN_THREADS <= cut < HW:
            e = e.take(e.tgt < cut)
    if defect == "segment-cut-at-48":
        e = e.take(e.rank() < SS_INSERTION_MAX)
    return e


def splat_sums(feat64, e):
    """feat64 [HW, C] -> S [HW, C], A [HW, C], Nw [HW], n [HW] (fp64 / int64)"""
    HW, C = e.HW, feat64.shape[1]
    t, w = torch.from_numpy(e.tgt), torch.from_numpy(e.w64)
    v = feat64[torch.from_numpy(e.src)] * w[:, None]
    S = torch.zeros(HW, C, dtype=F64).index_add_(0, t, v)
    A = torch.zeros(HW, C, dtype=F64).index_add_(0, t, v.abs())
    Nw = torch.zeros(HW, dtype=F64).index_add_(0, t, w)
    n = torch.bincount(t, minlength=HW)
    return S, A, Nw, n


def stable16(ref):
    """mask: round16 is constant on [ref (1 - 6 u32), ref (1 + 6 u32)] -- no fp16 rounding boundary within 6 u32 |ref| of ref"""
    lo, hi = round16(ref * (1 - 6 * U32)).double(), round16(ref * (1 + 6 * U32)).double()
    return lo == hi


class Want:
    """what one flow frame of a case must give: ``ref`` / ``bound`` fp64 [HW, C], ``zero`` [HW] (Nw == 0: the value 0), ``stable``
    (exact cases: where the output must equal round16(ref)), ``n`` [HW]"""

    def __init__(self, ref, bound, zero, stable, n):
        self.ref, self.bound, self.zero, self.stable, self.n = ref, bound, zero, stable, n


LEFT_OUT = {}      # case id -> (elements of the exact check left out as too near a rounding boundary, elements): filled by want()


def standin(defect=None):
    """the reference behind the backend signature: standin(None) is a correct warp, standin(defect) a wrong one"""
    def splat(feat, flow, out, H, W):
        HW, C = H * W, feat.shape[1]
        f64 = feat.double()
        hi = C
        if defect == "last-channel-pass-stale":                       # channels of the second and later passes left as they were
            hi = min(C, PASS_CH)
        if defect == "second-pass-only-full" and C > PASS_CH:         # the ragged last pass dropped
            hi = PASS_CH * (C // PASS_CH)
        for i in range(flow.shape[0]):
            S, _, Nw, _ = splat_sums(f64, entries(flow[0 if defect == "flow0-csr-for-all" else i], H, W, defect))
            if defect == "sum-not-avg":
                y = S
            elif defect == "eps-dropped":
                y = torch.where(Nw[:, None] > 0, S / Nw.clamp(min=1e-300)[:, None], torch.zeros_like(S))
            else:
                y = S / (Nw + (1e-6 if defect == "eps-1e-6" else EPS))[:, None]
            out[i * HW:(i + 1) * HW, :hi] = round16(y)[:, :hi]
        return []
    return splat


def norm_emulation(flow, H, W, order="key"):
    """flow [N, 2, H, W] -> fp32 [N, H, W]: per target the fp32 weights added one after the other in fp32, in key order
    corner * HW + source (``order="key"``: the kernels' order) or source-major, (source, corner) (``order="source"``)"""
    HW = H * W
    out = np.zeros((flow.shape[0], HW), dtype=np.float32)
    for i in range(flow.shape[0]):
        e = entries(flow[i], H, W)
        if order == "source":
            e = e.take(np.lexsort((e.key // HW, e.src, e.tgt)))
        rank = e.rank()
        for j in range(int(rank.max()) + 1 if len(rank) else 0):
            m = rank == j
            out[i, e.tgt[m]] = out[i, e.tgt[m]] + e.w32[m]            # fp32 + fp32: one rounded addition
    return torch.from_numpy(out).reshape(flow.shape[0], H, W)


# ---------------------------------------------------------------------------------------------------------------------------
# cases and runs
# ---------------------------------------------------------------------------------------------------------------------------
class SplatCase:
    """``build()`` -> (feat fp16 [HW, C], flow fp32 [nflows, 2, H, W]); ``cls``: the class the worst ratio is recorded under;
    ``exact``: dyadic data (module docstring); ``singles``: every flow frame is also run alone and must give the same bits;
    ``counts``: {(flow frame, target): number of entries} the construction promises"""

    def __init__(self, id, cls, H, W, C, build, exact=False, singles=False, counts=None):
        self.id, self.cls, self.H, self.W, self.C, self.build = id, cls, H, W, C, build
        self.exact, self.singles, self.counts = exact, singles, counts or {}
        self._inputs = self._want = None

    def __repr__(self):
        return self.id

    def inputs(self):
        if self._inputs is None:
            feat, flow = self.build()
            assert feat.dtype == F16 and tuple(feat.shape) == (self.H * self.W, self.C) and flow.dtype == F32
            assert tuple(flow.shape[1:]) == (2, self.H, self.W)
            self._inputs = (feat, flow.contiguous())
        return self._inputs

    def want(self):
        """[Want per flow frame], computed once from the case's own inputs"""
        if self._want is None:
            feat, flow = self.inputs()
            f64, wants, left = feat.double(), [], 0
            for i in range(flow.shape[0]):
                S, A, Nw, n = splat_sums(f64, entries(flow[i], self.H, self.W))
                assert int(n.max()) <= (N_EXACT if self.exact else N_MAX), (self.id, i, int(n.max()))
                ref = S / (Nw + EPS)[:, None]
                bound = U16 * ref.abs() + 2.0 ** -25 + ((2 * n + 6) * U32 / (Nw + EPS))[:, None] * A
                stable = stable16(ref) if self.exact else None
                left += 0 if stable is None else int((~stable).sum())
                wants.append(Want(ref, bound, Nw == 0, stable, n))
            LEFT_OUT[self.id] = (left, flow.shape[0] * ref.numel())
            self._want = wants
        return self._want


class Run:
    """one call of a backend on a case (or on the flow frames ``frames`` of it alone)"""

    def __init__(self, case, splat, device="cpu", frames=None):
        feat, flow = case.inputs()
        flow = flow if frames is None else flow[frames].contiguous()
        HW, C = case.H * case.W, case.C
        self.case = case
        self.feat = oc.Placed(guard(feat, ld=C + 24), device)
        self.out = oc.Placed(guard(shape=(flow.shape[0] * HW, C), ld=C + 40), device)
        self.flow = oc.Placed(flow, device)
        self.complaints = list(splat(self.feat.t, self.flow.t, self.out.t, case.H, case.W) or [])
        if str(device).startswith("cuda"):
            torch.cuda.synchronize()

    def guard_errors(self):
        bad = list(self.complaints)
        for name, p, written in (("feat", self.feat, False), ("flow", self.flow, False), ("out", self.out, True)):
            diff = oc.bits(p.buf) != oc.bits(p.snap)
            if written:
                diff = diff & ~p.inside
            if int(diff.sum()):
                bad.append(f"{self.case.id}: {int(diff.sum())} elements of {'the guard of ' if written else 'read-only '}{name} changed, "
                           f"first at {torch.nonzero(diff)[0].tolist()}")
        return bad

    def result(self):
        return self.out.t.detach().cpu()


def check_frame(what, g, w):
    """one flow frame's output ``g`` fp16 [HW, C] against its Want -> (worst err / bound, [messages])"""
    gd = g.double()
    if not bool(torch.isfinite(gd).all()):
        bad = ~torch.isfinite(gd)
        return INF, [f"{what}: {int(bad.sum())} non-finite elements, first at {torch.nonzero(bad)[0].tolist()}"]
    errs = []
    err = (gd - w.ref).abs()
    ratio = err / w.bound
    worst = ratio.max().item()
    if worst > 1.0:
        i = torch.nonzero(ratio == ratio.max())[0].tolist()
        errs.append(f"{what}: {int((ratio > 1).sum())} / {ratio.numel()} elements out of bound, worst at {i} (n = {int(w.n[i[0]])}): "
                    f"err {err[tuple(i)].item():.4e} = {worst:.3f} x its bound {w.bound[tuple(i)].item():.4e}")
    if bool((gd[w.zero] != 0).any()):
        errs.append(f"{what}: {int((gd[w.zero] != 0).sum())} elements of targets without weight are not 0")
    if w.stable is not None:
        off = (gd != round16(w.ref).double()) & w.stable
        if bool(off.any()):
            i = torch.nonzero(off)[0].tolist()
            errs.append(f"{what}: {int(off.sum())} of the {int(w.stable.sum())} elements that must be the reference rounded once are "
                        f"not, first at {i}: {gd[tuple(i)].item()!r} for {w.ref[tuple(i)].item()!r}")
    return worst, errs


def check_run(case, r, splat=None, device="cpu"):
    """-> (worst err / bound, [messages]): guards, every flow frame against the reference, and (``singles``, with ``splat``)
    every flow frame run alone bit-equal to its rows of the joint run"""
    errs, worst = r.guard_errors(), 0.0
    out, HW = r.result(), case.H * case.W
    wants = case.want()
    for i, w in enumerate(wants):
        wo, e = check_frame(f"{case.id} flow {i}", out[i * HW:(i + 1) * HW], w)
        worst, errs = max(worst, wo), errs + e
    if case.singles and splat is not None:
        for i in range(len(wants)):
            one = Run(case, splat, device, frames=[i])
            errs += one.guard_errors()
            if not oc.same_bits(one.result(), out[i * HW:(i + 1) * HW]):
                errs.append(f"{case.id}: flow {i} run alone gives other bits than in the joint run")
    return worst, errs


def column_subset_errors(splat, device="cpu"):
    """channel independence: the C = 8 run on the column view [:, :8] of the C = 1280 feature buffer must equal columns 0..7 of
    the C = 1280 output bit for bit"""
    case = BY_ID["gauss/7x9-C1280-mag1.5-n1"]
    wide = Run(case, splat, device)
    errs = wide.guard_errors()
    HW = case.H * case.W
    out8 = oc.Placed(guard(shape=(HW, 8), ld=56), device)
    feat8 = wide.feat.t[:, :8]
    errs += list(splat(feat8, wide.flow.t, out8.t, case.H, case.W) or [])
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    if int((oc.bits(out8.buf) != oc.bits(out8.snap))[~out8.inside].sum()):
        errs.append("column subset: the guard of out changed")
    if not oc.same_bits(out8.t.cpu(), wide.result()[:, :8].contiguous()):
        errs.append("column subset: the C = 8 run on feat[:, :8] gives other bits than columns 0..7 of the C = 1280 run")
    return errs


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
PLANES = [(1, 1), (1, 9), (7, 1), (5, 5), (6, 7), (7, 9), (31, 33), (32, 32), (25, 41), (33, 63)]
FULL = [(7, 9), (25, 41)]                              # every width, and several flow frames
WIDTHS = (8, 512, 520, 1280)
OUT = 1000.0                                           # a flow that sends its source far outside every plane of the table


def _grid16(HW, C, seed):
    """fp16 features on the 2^-4 grid, |v| <= 4"""
    return (_ints(-64, 64, HW, C, seed=seed) / 16).half()


def _gauss_flow(nf, H, W, seed, mag):
    return torch.randn(nf, 2, H, W, generator=torch.Generator().manual_seed(seed)) * mag


def _grid_xy(H, W):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F32), torch.arange(W, dtype=F32), indexing="ij")
    return xs, ys


def _gauss_case(H, W, C, mag, nf, seed):
    def build():
        return _h(H * W, C, seed=seed), _gauss_flow(nf, H, W, seed + 1, mag)
    return SplatCase(f"gauss/{H}x{W}-C{C}-mag{mag:g}-n{nf}", "gauss", H, W, C, build, singles=nf > 1)


def _dyadic_case(H, W, C, seed):
    def build():
        return _grid16(H * W, C, seed), _ints(-8, 8, 1, 2, H, W, seed=seed + 1) / 4
    return SplatCase(f"dyadic/{H}x{W}-C{C}", "dyadic", H, W, C, build, exact=True)


def border_values(n):
    """target coordinates along an axis of n pixels: west / north of the plane, on its first and last pixel, east / south of it"""
    return [-1.25, -1.0, -0.75, -0.25, -0.0, 0.0, n - 1.25, n - 1.0, n - 0.75, n - 0.25, float(n)]


def _border_axis_case(H, W, axis, seed):
    """one flow frame per value of border_values: EVERY source is sent to that coordinate on ``axis``, the other axis stays"""
    vals = border_values(W if axis == "x" else H)

    def build():
        xs, ys = _grid_xy(H, W)
        flow = torch.zeros(len(vals), 2, H, W)
        for i, v in enumerate(vals):
            flow[i, 0 if axis == "x" else 1] = torch.tensor(v, dtype=F32) - (xs if axis == "x" else ys)
        return _grid16(H * W, 8, seed), flow
    return SplatCase(f"border/{H}x{W}-{axis}", "border", H, W, 8, build, exact=True)


def _border_corner_case(H, W, seed):
    """the four corner combinations: the first 16 sources (at most) are sent just outside a corner of the plane, where one of the
    four corners of the splat lands inside; everyone else far outside"""
    def build():
        xs, ys = _grid_xy(H, W)
        flow = torch.full((4, 2, H, W), OUT)
        first = (torch.arange(H * W) < 16).reshape(H, W)
        for i, (fx, fy) in enumerate(((-0.25, -0.25), (W - 0.75, -0.25), (-0.25, H - 0.75), (W - 0.75, H - 0.75))):
            flow[i, 0][first] = (fx - xs)[first]
            flow[i, 1][first] = (fy - ys)[first]
        return _grid16(H * W, 8, seed), flow
    return SplatCase(f"border/{H}x{W}-corners", "border", H, W, 8, build, exact=True)


def _border_step_case(H, W, kind, seed):
    """integer flows (three zero-weight corners, which stay entries) / half-pixel flows"""
    def build():
        flow = _ints(-2, 2, 1, 2, H, W, seed=seed + 1) if kind == "integer" else _ints(-3, 3, 1, 2, H, W, seed=seed + 1) / 2
        return _grid16(H * W, 8, seed), flow
    return SplatCase(f"border/{H}x{W}-{kind}", "border", H, W, 8, build, exact=True)


SPECIAL_AT = (3, 4)                                                   # (y, x) of the special source on the 7 x 9 plane
SPECIAL_VALUES = (NAN, INF, -INF, 3e9, -3e9, 3e38, -3e38, 16777217.0)


def _special_case():
    """one flow frame per (value, axis): the zero flow with that value at one source.  That source contributes nowhere, so its
    own pixel keeps only the zero-weight corners of its neighbours (the value 0) and every other pixel is feat / (1 + 1e-7)"""
    H, W = 7, 9

    def build():
        flow = torch.zeros(2 * len(SPECIAL_VALUES), 2, H, W)
        for i, v in enumerate(SPECIAL_VALUES):
            flow[2 * i, 0, SPECIAL_AT[0], SPECIAL_AT[1]] = v
            flow[2 * i + 1, 1, SPECIAL_AT[0], SPECIAL_AT[1]] = v
        return _grid16(H * W, 8, 700), flow
    return SplatCase("special/7x9", "special", H, W, 8, build, exact=True)


TINY = ((10, 0), (12, 8), (15, 54))                                   # (k, target): a total weight of 2^-2k on that target of 7 x 9


def _tiny_case():
    """three targets that receive 2^-20, 2^-24, 2^-30 from ONE source each: the source is sent 2^-k inside the ring of width 1
    around the plane at a corner of it, so only one corner of its splat is in bounds, with weight 2^-k * 2^-k; w / (w + 1e-7) is
    0.905, 0.37, 0.009.  Everyone else is sent far outside"""
    H, W = 7, 9

    def build():
        flow = torch.full((1, 2, H, W), OUT)
        for j, ((k, _), (fx, fy)) in enumerate(zip(TINY, ((-1 + 2.0 ** -10, -1 + 2.0 ** -10), (W - 2.0 ** -12, -1 + 2.0 ** -12),
                                                         (-1 + 2.0 ** -15, H - 2.0 ** -15)))):
            y, x = 2 + j, 3 + j                                       # the source
            flow[0, 0, y, x], flow[0, 1, y, x] = fx - x, fy - y       # exact in fp32: at most 4 + 15 bits
        feat = _grid16(H * W, 8, 710)
        feat[feat == 0] = 0.5                                         # (a zero feature would hide the epsilon)
        return feat, flow
    return SplatCase("tiny/7x9", "tiny", H, W, 8, build, exact=True, counts={(0, t): 1 for _, t in TINY})


SEG_H, SEG_W = 12, 20
SEG_BLOCKS = {0: ((200, 3, 3),), 1: ((49, 1, 2), (48, 7, 2), (47, 13, 2))}      # flow frame -> (sources, tx, ty) per block


def _segments_case():
    """exact segment lengths around SS_INSERTION_MAX.  A block of K sources is sent to x in (tx, tx + 2), y in (ty, ty + 1) with
    non-dyadic fractions: pixel (tx + 1, ty) receives the NE corner of those with floor tx and the NW corner of the others -- K
    entries of two corner classes, so the key order is not the source order -- and so does (tx + 1, ty + 1).  One more source
    per frame is sent just outside a corner of the plane: a segment of exactly 1"""
    H, W = SEG_H, SEG_W

    def build():
        flow = torch.full((2, 2, H, W), OUT)
        xs, ys = _grid_xy(H, W)
        for i, blocks in SEG_BLOCKS.items():
            s0 = 0
            for K, tx, ty in blocks:
                j = torch.arange(K)
                px = tx + 0.153 + ((j * 37) % 100).float() / 100 * 1.7
                py = ty + 0.21 + ((j * 53) % 97).float() / 97 * 0.58
                idx = s0 + j
                flow[i, 0].view(-1)[idx] = px - xs.reshape(-1)[idx]
                flow[i, 1].view(-1)[idx] = py - ys.reshape(-1)[idx]
                s0 += K
            lone = H * W - 1 - i
            fx, fy = ((-0.37, -0.41), (W - 1 + 0.3, H - 1 + 0.4))[i]
            flow[i, 0].view(-1)[lone] = fx - xs.reshape(-1)[lone]
            flow[i, 1].view(-1)[lone] = fy - ys.reshape(-1)[lone]
        return _h(H * W, 8, seed=720), flow
    counts = {(i, (ty + dy) * W + tx + 1): K for i, blocks in SEG_BLOCKS.items() for K, tx, ty in blocks for dy in (0, 1)}
    counts[(0, 0)] = counts[(1, H * W - 1)] = 1
    return SplatCase(f"segments/{H}x{W}", "segments", H, W, 8, build, counts=counts)


CONVERGE_AT = (7.3, 5.6)


def _converge_case():
    """flow = c - position: every source lands on c, all 4 HW entries on the four pixels around it (the heap-sort path)"""
    H, W = SEG_H, SEG_W

    def build():
        xs, ys = _grid_xy(H, W)
        return _h(H * W, 8, seed=730), torch.stack([CONVERGE_AT[0] - xs, CONVERGE_AT[1] - ys])[None]
    t0 = 5 * W + 7
    return SplatCase(f"converge/{H}x{W}", "segments", H, W, 8, build, counts={(0, t): H * W for t in (t0, t0 + 1, t0 + W, t0 + W + 1)})


def _first_flow_convergent_case():
    """three flow frames in one workspace: the first convergent (long segments), the others sparse (most sources leave the plane)"""
    H, W = 7, 9

    def build():
        xs, ys = _grid_xy(H, W)
        flow = torch.full((3, 2, H, W), OUT)
        flow[0] = torch.stack([4.3 - xs, 3.6 - ys])
        g = _gauss_flow(3, H, W, 741, 1.5)
        keep = torch.rand(3, H, W, generator=torch.Generator().manual_seed(742)) < 0.2
        keep[0] = False
        flow[:, 0][keep], flow[:, 1][keep] = g[:, 0][keep], g[:, 1][keep]
        return _h(H * W, 8, seed=740), flow
    return SplatCase("flows/7x9-convergent-first", "flows", H, W, 8, build, singles=True)


def _range_case(kind):
    H, W = 7, 9

    def build():
        if kind == "max":                                             # +-65504: a weighted mean never leaves the range
            feat = torch.where(_ints(0, 1, H * W, 8, seed=750) > 0, 65504.0, -65504.0).half()
        else:                                                         # fp16 subnormals
            feat = (_ints(-1023, 1023, H * W, 8, seed=751) * 2.0 ** -24).half()
        return feat, _gauss_flow(1, H, W, 752, 1.5)
    return SplatCase(f"range/{kind}", "range", H, W, 8, build)


def _widths(plane):
    return WIDTHS if plane in FULL else (8, 520)


CASES = (
    [_gauss_case(H, W, C, 1.5, 3 if (H, W) in FULL and C == 8 else 1, 500 + 10 * i + j)
     for i, (H, W) in enumerate(PLANES) for j, C in enumerate(_widths((H, W)))]
    + [_gauss_case(H, W, 8, 4.0, 1, 600 + i) for i, (H, W) in enumerate(PLANES)]
    + [_dyadic_case(H, W, C, 620 + 10 * i + j) for i, (H, W) in enumerate(PLANES) for j, C in enumerate(_widths((H, W)))]
    + [c for i, (H, W) in enumerate(((7, 9), (1, 9), (7, 1)))
       for c in (_border_axis_case(H, W, "x", 660 + i), _border_axis_case(H, W, "y", 670 + i), _border_corner_case(H, W, 680 + i),
                 _border_step_case(H, W, "integer", 690 + 2 * i), _border_step_case(H, W, "half", 696 + 2 * i))]
    + [_special_case(), _tiny_case(), _segments_case(), _converge_case(), _first_flow_convergent_case(), _range_case("max"),
       _range_case("subnormal")]
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
CLASSES = tuple(dict.fromkeys(c.cls for c in CASES))
ORDER_CASES = ("segments/12x20", "converge/12x20")                    # the norm's summation order is checked on these

# mutant -> cases it must fail (tests/test_splat_cases_cpu.py)
MUTANT_CASES = {
    "eps-dropped": ("tiny/7x9",),
    "eps-1e-6": ("tiny/7x9",),
    "trunc-not-floor": ("border/7x9-x", "border/7x9-y", "border/1x9-x", "border/7x1-y"),
    "oob-clamped-to-border": ("border/7x9-x", "border/7x9-y", "border/7x9-corners"),
    "nonfinite-as-zero-flow": ("special/7x9",),
    "swap-xy": ("gauss/7x9-C8-mag1.5-n3", "border/7x9-x"),
    "ne-sw-swapped": ("dyadic/7x9-C8", "gauss/6x7-C8-mag1.5-n1"),
    "last-channel-pass-stale": ("gauss/7x9-C520-mag1.5-n1", "gauss/7x9-C1280-mag1.5-n1", "dyadic/5x5-C520"),
    "second-pass-only-full": ("gauss/7x9-C520-mag1.5-n1", "gauss/25x41-C1280-mag1.5-n1", "dyadic/33x63-C520"),
    "flow0-csr-for-all": ("gauss/7x9-C8-mag1.5-n3", "gauss/25x41-C8-mag1.5-n3", "flows/7x9-convergent-first", "segments/12x20"),
    "segment-cut-at-48": ("segments/12x20", "converge/12x20"),
    "sum-not-avg": ("gauss/7x9-C8-mag1.5-n3", "dyadic/7x9-C8"),
    "scan-last-segment-dropped": ("gauss/25x41-C8-mag1.5-n3", "gauss/33x63-C8-mag1.5-n1", "dyadic/25x41-C8"),
}
assert set(MUTANT_CASES) == set(MUTANTS) and all(i in BY_ID for ids in MUTANT_CASES.values() for i in ids)
