"""TEST INFRASTRUCTURE ONLY: the case table of the layout movers (``nchw_to_tokens`` / ``tokens_to_nchw``: the 32 x 32 LDS tile
transpose of csrc/elementwise.hip) and of the scheduler step kernels (``prepare_model_input(_dev)``, ``cfg_euler_step(_dev)_``),
with their references, the per-element expectations and the "wrong kernel" mutants that prove the checks can fail.

Built like tests/aux_cases.py on tests/op_cases.py: a case builds the keyword arguments of the op as seeded CPU tensors -- every
fp16 2-D argument a view into a NaN buffer (guard rows before and after, guard columns, a leading dimension larger than the width
and different for the arguments of one call), every fp32 NCHW tensor a ``View`` into a longer 1-D NaN buffer --, ``op_cases.run``
takes it through ``mofa_video_amd.ops`` on the GPU (tests/test_step_matrix_gpu.py) and through ``impl(defect)`` on the CPU
(tests/test_step_cases_cpu.py), ``check_run`` compares the run with ``case.ref`` computed from the call's own arguments.

Expectations (u16 = 2^-11, u32 = 2^-24: half an ulp), derived, never measured:

  nchw_to_tokens       bit-equal to (x * fl32(scale)).half(): ONE fp32 product, ONE rounding to fp16 (beyond 65519.99 the
                       infinity, the tie 65520 included; subnormal results kept; -0.0 kept; a NaN stays a NaN, whatever its
                       payload).  Fresh output with ld > C: columns >= C are zero.  ``out=`` a column slice: the columns of the
                       slice beyond C, everything of the buffer outside the slice and the guard rows keep their bits
  tokens_to_nchw       bit-equal to x[:, :Cc].float() (every fp16 value is an fp32 value); the columns >= Cc of the input rows
                       hold NaN and must never reach the result
  family P             placement: values k - 2048, k = 64 (c % 64) + p % 64, times 2^-e with e = n % 2 + 2 (c / 64 % 2) +
                       4 (p / 64 % 2): exact in fp16, pairwise distinct inside any 64 x 64 (channel, pixel) window (but the one
                       zero), other values in the next image, the next channel block and the next pixel block.  scale = 1
  family R             rounding: Gaussian x 3 with +-70000, 65520, 65519, 1e-8, 3e-6, -0.0 and a NaN planted, scale in
                       {1, 0.18215, 1 / 0.18215, 2^-5}

  prepare_model_input_dev   columns 0..3 bit-equal to (lat * tab[row, 4]).half() (one fp32 product), columns 4..7 bit-equal to
                       img[half].half(), both CFG halves the same latents, columns >= 8 of the view and every guard unchanged
  prepare_model_input  (host scalars) the launcher forms inv = 1 / sqrt(sigma^2 + 1) in fp32: sigma^2, + 1, sqrt, 1 / (four
                       roundings, fewer when contracted; the square root halves what it inherits) -- at most 3 u32 on inv, one
                       more for the product: |out - ref64| <= u16 |ref| + 2^-25 + 4 u32 |ref|.  Columns 4..7 as above.  Within
                       one fp16 ulp of the device-scalar form (checked by the test files on the pair of cases)
  cfg_euler_step(_dev)_     against the fp64 evaluation of
                           g = gmin + (gmax - gmin) t / (T - 1)   (T == 1: gmin),   v = v_u + g (v_c - v_u),
                           x0 = -sigma / sqrt(sigma^2 + 1) v + x / (sigma^2 + 1),   out = x + (x - x0) / sigma (sigma_next - sigma)
                       from the fp32 / fp16 inputs as the kernel receives them.  With A = |x|, B = |v_u| + |g| |v_c - v_u| >= |v|,
                       |c_out| <= 1, c_skip <= 1, |dt / sigma| <= 1 (0 <= sigma_next <= sigma, asserted) and 0 <= gmin <= gmax
                       (asserted: every intermediate of g is <= g), counting one u32 per fp32 operation relative to a quantity
                       that is <= A + B (division and square root are correctly rounded; a contraction to FMA only removes
                       roundings):
                           g: 4 (difference, product, quotient, sum)    v_c - v_u: 1    g (..): 1    v_u + ..: 1      -> 7 on v
                           c_out: 4 (square, + 1, sqrt, quotient)       v c_out: 1                                  -> 12 on v c_out
                           c_skip: 3 (square, + 1, reciprocal)          x c_skip: 1                                 -> 4 on x c_skip
                           x0 = sum: 1    x - x0: 1    / sigma: 1    dt: 1    d dt: 1    x + ..: 1                  -> + 6 on both
                       = 18 u32 B + 10 u32 A; one more of each for the second-order terms:
                           |out - ref64| <= u32 (11 |x| + 19 (|v_u| + |g| |v_c - v_u|))
                       (below the 24 u32 (|x| + |v_u| + |g| |v_c - v_u|) the kernels were specified with).  The prediction buffer
                       keeps its bits.  sigma_next == sigma: d * 0 = 0 and the latents keep their bits; gmin == gmax: g = gmin for
                       every frame.  Host- and device-scalar forms: bit-equal latents (the test files, on the pair of cases)

Second pass of the grid-stride loops (``op_cases.EW_GRID_ITEMS`` = 16384 blocks x 256 items): clips reach 1024 frames of 9216
latent pixels, 9.4 M items for cfg_euler and twice that for prepare_model_input.  ``BIG_T`` x ``BIG_HW`` is the smallest product
above the cap with T = 129 > 128 frames and HW % 256 != 0: 67 MB of latents, 134 MB of prediction (ldn = 8), one case per kernel.

Mutants (``mutant_differs`` says from the geometry where each computes something else; elsewhere it must EQUAL the truth):
  tile-transposed     (c, p) exchanged inside a 32 x 32 tile              movers with C > 1 or HW > 1
  drop-c0             the channel tile offset dropped: c -> c % 32        movers with C > 32
  image-stride-ld     image stride of x taken as ld * HW, not C * HW      nchw_to_tokens with n > 1 and ld != C
  scale-after-round   (x.half() * scale).half()                           nchw_to_tokens with scale != 1 (family R)
  pad-cols-written    zeros into the columns of ``out=`` beyond C         ``out=`` wider than C
  ragged-clamp        the ragged last pixel tile loads as if aligned to the end of the image (clamped), stores unshifted
                                                                          movers with HW % 32 > 1
  cfg-swap            CFG halves exchanged                                cfg_euler with sigma_next != sigma (g > 1/2, asserted)
  ramp-div-T          ramp divided by T                                   cfg_euler with T > 1, gmin != gmax, sigma_next != sigma
  ramp-pixel          ramp indexed by the pixel                           cfg_euler with T > 1, gmin != gmax, sigma_next != sigma
  eps-pred            x0 = x - sigma v                                    cfg_euler with sigma_next != sigma
  no-c-skip           x0 = c_out v + x                                    cfg_euler with sigma_next != sigma
  ldn-ignored         prediction rows at stride 4                         every cfg_euler case (the guard's NaN is read)
  img-half0           image latents of half 0 for both halves             every prepare_model_input case"""
import types

import torch

import aux_cases as ac
import op_cases as oc
from aux_cases import U16, U32, Want, round16
from op_cases import F16, F32, NAN, View, _f, _h, guard

F64 = torch.float64
INF = float("inf")

MOVER_C = (1, 3, 4, 31, 32, 33, 64, 65, 320)
MOVER_HW = (1, 31, 32, 33, 63, 64, 65, 1000)
FORMS = ("ldC", "ldpad", "out", "out-wide")
SCALES = (1.0, 0.18215, 1.0 / 0.18215, 2.0 ** -5)
R_PLANTS = (70000.0, -70000.0, 65520.0, 65519.0, 1e-8, 3e-6, -0.0, NAN)      # image_cases.PATCH_PLANTS and a NaN
T2N_PLANTS = (65504.0, -65504.0, 2.0 ** -24, 3e-6, -0.0)
MOVER_MUTANTS = ("tile-transposed", "drop-c0", "image-stride-ld", "scale-after-round", "pad-cols-written", "ragged-clamp")
STEP_MUTANTS = ("cfg-swap", "ramp-div-T", "ramp-pixel", "eps-pred", "no-c-skip", "ldn-ignored", "img-half0")
MUTANTS = MOVER_MUTANTS + STEP_MUTANTS
_MOVERS, _N2T = ("nchw_to_tokens", "tokens_to_nchw"), ("nchw_to_tokens",)
_EULER, _PREP = ("cfg_euler_step_", "cfg_euler_step_dev_"), ("prepare_model_input", "prepare_model_input_dev")
MUTANT_OPS = {"tile-transposed": _MOVERS, "drop-c0": _MOVERS, "image-stride-ld": _N2T, "scale-after-round": _N2T,
              "pad-cols-written": _N2T, "ragged-clamp": _MOVERS, "cfg-swap": _EULER, "ramp-div-T": _EULER, "ramp-pixel": _EULER,
              "eps-pred": _EULER, "no-c-skip": _EULER, "ldn-ignored": _EULER, "img-half0": _PREP}

STEP_T, STEP_HW = (1, 2, 25), {1: (1, 1), 48: (6, 8), 257: (1, 257)}
STEP_ROWS = (0, 3, 12, 24)
BIG_T, BIG_HW, BIG_H, BIG_W = 129, 32514, 6, 5419
assert BIG_H * BIG_W == BIG_HW and BIG_HW % 256 and BIG_T * BIG_HW > oc.EW_GRID_ITEMS >= BIG_T * (BIG_HW - 1)


class Part:
    """one output checked in pieces: [(tag, cut, Want)]"""

    def __init__(self, *pieces):
        self.pieces = pieces


def check_run(case, r):
    """-> (worst err / bound, [messages]): guards, then every output against ``case.ref`` (``aux_cases.check_want`` per piece; a
    ``Want`` with a ``nan`` mask: those elements must be NaN, of any payload)"""
    errs = list(r.guard_errors())
    wants, outs = case.ref(ac.inputs_of(r)), r.outputs()
    worst = 0.0
    if len(wants) != len(outs):
        return INF, errs + [f"{case.id}: {len(outs)} outputs {[o[0] for o in outs]}, {len(wants)} expected"]
    for (label, g, _), w in zip(outs, wants):
        for tag, cut, want in (w.pieces if isinstance(w, Part) else [("", lambda t: t, w)]):
            gg = cut(g)
            nan = getattr(want, "nan", None)
            if nan is not None and bool(nan.any()):
                if gg.shape != nan.shape or not bool(torch.isnan(gg[nan]).all()):
                    errs.append(f"{case.id} {label}{tag}: a NaN input did not stay NaN")
                    continue
                gg = gg.clone()
                gg[nan] = want.bits[nan]
            wo, e = ac.check_want(f"{case.id} {label}{tag}", gg, want)
            worst, errs = max(worst, wo), errs + e
    return worst, errs


# ---------------------------------------------------------------------------------------------------------------------------
# the layout movers
# ---------------------------------------------------------------------------------------------------------------------------
def placement(n, C, HW):
    """family P -> fp32 [n, C, HW] (module docstring)"""
    c, p, i = torch.arange(C), torch.arange(HW), torch.arange(n)
    k = (c % 64)[:, None] * 64 + (p % 64)[None, :]
    e = (i % 2)[:, None, None] + 2 * ((c // 64) % 2)[None, :, None] + 4 * ((p // 64) % 2)[None, None, :]
    return ((k - 2048).float()[None] * torch.exp2(-e.float())).contiguous()


def _src_maps(C, HW, defect):
    """for the token element (p, c): the source channel and pixel it is taken from, and whether it is taken at all"""
    c, p = torch.arange(C), torch.arange(HW)
    cc, pp = c[None, :].expand(HW, C), p[:, None].expand(HW, C)
    valid = torch.ones(HW, C, dtype=torch.bool)
    if defect == "tile-transposed":
        c0, p0 = c // 32 * 32, p // 32 * 32
        cc, pp = c0[None, :] + (p - p0)[:, None], p0[:, None] + (c - c0)[None, :]
        valid = (cc < C) & (pp < HW)
    elif defect == "drop-c0":
        cc = cc % 32
    elif defect == "ragged-clamp" and HW % 32:
        shifted = torch.where(p >= HW // 32 * 32, (p + 32 - HW % 32).clamp(max=HW - 1), p)
        pp = shifted[:, None].expand(HW, C)
    return cc.clamp(max=C - 1), pp.clamp(max=HW - 1), valid


def move_ref(x3, defect=None):
    """x3 [n, C, HW] -> [n, HW, C], pure data movement (any dtype)"""
    n, C, HW = x3.shape
    if defect not in ("tile-transposed", "drop-c0", "ragged-clamp"):
        return x3.permute(0, 2, 1).contiguous()
    cc, pp, valid = _src_maps(C, HW, defect)
    return torch.where(valid[None], x3[:, cc, pp], torch.zeros((), dtype=x3.dtype))


def n2t_value(x, scale, defect=None):
    """the fp16 value of fp32 ``x``: one fp32 product, one rounding"""
    s = torch.tensor(scale, dtype=F32)
    if defect == "scale-after-round":
        return (x.half().float() * s).half()
    return (x * s).half()


def n2t_ref(x, scale, ldo, defect=None):
    """fp32 [n, C, H, W] -> fp16 tokens [n*H*W, C]"""
    n, C, H, W = x.shape
    HW = H * W
    if defect == "image-stride-ld":      # image i of x sought at i * ldo * HW; what lies behind the tensor is the NaN guard
        flat = torch.cat([x.reshape(-1), torch.full((n * max(ldo, C) * HW,), NAN)])
        x = torch.stack([flat[i * ldo * HW:i * ldo * HW + C * HW] for i in range(n)]).reshape(n, C, H, W)
    return n2t_value(move_ref(x.reshape(n, C, HW), defect), scale, defect).reshape(n * HW, C)


def t2n_ref(x, n, Cc, H, W, defect=None):
    """fp16 tokens [n*H*W, >= Cc] -> fp32 [n, Cc, H, W]"""
    tok = x[:, :Cc].float().reshape(n, H * W, Cc)
    y = move_ref(tok.permute(0, 2, 1), defect)                      # [n, HW, Cc] as the (mis)placed tokens
    return y.permute(0, 2, 1).reshape(n, Cc, H, W).contiguous()


def _hw(HW):
    return (1, HW) if HW < 8 or HW % 8 else (8, HW // 8)


def _mover_data(family, n, C, HW, seed, plants):
    if family == "P":
        return placement(n, C, HW)
    x = _f(n, C, HW, seed=seed, scale=3.0)
    flat = x.reshape(-1)
    for i, val in enumerate(plants):
        flat[(i * 37 + 5) % flat.numel()] = val
    return x


def _n2t_case(family, n, C, HW, form, scale=1.0, seed=0):
    H, W = _hw(HW)
    M = n * HW
    ldpad = (C + 8) // 8 * 8 + 8
    wide = C + 2 if form == "out-wide" else C
    ldo = {"ldC": C, "ldpad": ldpad, "out": 24 + C + 13, "out-wide": 24 + wide + 13}[form]

    def build():
        x = _mover_data(family, n, C, HW, seed, R_PLANTS).reshape(n, C, H, W)
        kw = dict(x=ac._nchw_view(x), scale=scale)
        if form == "ldC":
            kw["ld"] = C
        elif form == "ldpad":
            kw["ld"] = ldpad
        else:                                                       # a column slice at column 24 of a wider NaN buffer
            base = torch.full((3 + M + 2, ldo), NAN, dtype=F16)
            kw["out"] = View(base, lambda b: b[3:3 + M, 24:24 + wide])
        return kw

    def ref(kw):
        tok = n2t_ref(kw["x"], scale, ldo)
        if "out" in kw:
            want = kw["out"].clone()                                # the slice as it was: columns beyond C keep their bits
            want[:, :C] = tok
        else:
            want = torch.zeros((M, kw["ld"]), dtype=F16)
            want[:, :C] = tok
        w = Want(bits=want)
        w.nan = torch.isnan(want) & (torch.arange(want.shape[1]) < C)[None, :]
        return [w]
    tag = f"nchw_to_tokens/{family}-n{n}-C{C}-HW{HW}-{form}" + (f"-s{scale:.5g}" if family == "R" else "")
    return ac.AuxCase(tag, "nchw_to_tokens", build, ref, family=family, n=n, C=C, HW=HW, form=form, scale=scale, ldo=ldo, wide=wide)


def _t2n_case(family, n, C, HW, seed=0):
    H, W = _hw(HW)
    width = (C + 8) // 8 * 8 + 8                                      # the view is wider than Cc: its columns >= Cc hold NaN

    def build():
        x3 = _mover_data(family, n, C, HW, seed, T2N_PLANTS)
        tok = torch.full((n * HW, width), NAN, dtype=F16)
        tok[:, :C] = x3.permute(0, 2, 1).reshape(n * HW, C).half()
        return dict(x=guard(tok, ld=width + 24), n=n, Cc=C, H=H, W=W)

    def ref(kw):
        return [Want(bits=t2n_ref(kw["x"], n, C, H, W))]
    return ac.AuxCase(f"tokens_to_nchw/{family}-n{n}-C{C}-HW{HW}", "tokens_to_nchw", build, ref, family=family, n=n, C=C, HW=HW)


def _mover_cases():
    cases = []
    for i, C in enumerate(MOVER_C):
        for j, HW in enumerate(MOVER_HW):
            n = (1, 3, 3)[(i + 2 * j) % 3]
            cases.append(_n2t_case("P", n, C, HW, FORMS[(i + j) % 4]))
            cases.append(_t2n_case("P", n, C, HW))
    shapes = [(3, 33, 65), (1, 4, 1000), (3, 320, 33), (3, 65, 63)]
    for a, scale in enumerate(SCALES):
        for b, (n, C, HW) in enumerate(shapes):
            cases.append(_n2t_case("R", n, C, HW, FORMS[(a + b) % 4], scale=scale, seed=500 + 4 * a + b))
    for b, (n, C, HW) in enumerate(shapes):
        cases.append(_t2n_case("R", n, C, HW, seed=520 + b))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------
# the scheduler step kernels
# ---------------------------------------------------------------------------------------------------------------------------
_TABLE = []


def step_table():
    """scheduler.EulerDiscreteScheduler().step_table() for 25 steps, fp32 [25, 8]"""
    if not _TABLE:
        from mofa_video_amd.scheduler import EulerDiscreteScheduler
        sch = EulerDiscreteScheduler()
        sch.set_timesteps(25)
        _TABLE.append(torch.from_numpy(sch.step_table().copy()))
    return _TABLE[0]


def prepare_ref(lat, img, inv, T, HW, defect=None):
    """-> (fp64 [2*T*HW, 4] = lat * inv in both halves, fp32 [2*T*HW, 4] image latents of the row's half)"""
    l = lat.reshape(T, 4, HW).permute(0, 2, 1).reshape(T * HW, 4)
    i = img.reshape(2, 4, HW).permute(0, 2, 1)                      # [2, HW, 4]
    if defect == "img-half0":
        i = i[:1].expand(2, HW, 4)
    return torch.cat([l, l]).double() * inv, i[:, None].expand(2, T, HW, 4).reshape(2 * T * HW, 4)


def ramp(T, HW, gmin, gmax, defect=None):
    """fp64 [T, 1, HW or 1]: the guidance of every (frame, pixel)"""
    if T == 1:
        return torch.full((1, 1, 1), float(gmin), dtype=F64)
    if defect == "ramp-pixel":
        return (gmin + (gmax - gmin) * torch.arange(HW, dtype=F64) / (T - 1)).reshape(1, 1, HW).expand(T, 1, HW)
    t = torch.arange(T, dtype=F64)
    return (gmin + (gmax - gmin) * t / (T if defect == "ramp-div-T" else T - 1)).reshape(T, 1, 1)


def euler_ref(x, npred, sigma, sigma_next, gmin, gmax, defect=None):
    """x fp32 [T, 4, h, w], npred fp16 [2*T*HW, 4] -> (fp64 result [T, 4, h, w], its bound)"""
    T = x.shape[0]
    HW = x.shape[2] * x.shape[3]
    x64 = x.double().reshape(T, 4, HW)
    v2 = npred.double().reshape(2, T, HW, 4).permute(0, 1, 3, 2)    # [2, T, 4, HW]
    vu, vc = (v2[1], v2[0]) if defect == "cfg-swap" else (v2[0], v2[1])
    g = ramp(T, HW, gmin, gmax, defect)
    gw = g * (vc - vu)
    v = vu + gw
    s2 = float(sigma) ** 2 + 1.0
    if defect == "eps-pred":
        x0 = x64 - sigma * v
    else:
        x0 = v * (-sigma / s2 ** 0.5) + (x64 if defect == "no-c-skip" else x64 / s2)
    out = x64 + (x64 - x0) / sigma * (float(sigma_next) - float(sigma))
    bound = U32 * (11 * x64.abs() + 19 * (vu.abs() + gw.abs()))
    return out.reshape(x.shape), bound.reshape(x.shape)


def _step_data(T, HW, family, seed):
    """latents, image latents, prediction [2*T*HW, 4]: as tests/test_kernels_gpu.py draws them; family V: |v| ~ 30 dominates"""
    h, w = STEP_HW[HW]
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(T, 4, h, w, generator=g) * (1.0 if family == "V" else 50.0)
    img = torch.randn(2, 4, h, w, generator=g)
    npred = (torch.randn(2 * T * HW, 4, generator=g) * (30.0 if family == "V" else 1.0)).half()
    return lat, img, npred


def _scalars(row, same_sigma=False):
    """(the fp32 [8] row, sigma, sigma_next as Python floats holding the fp32 values)"""
    scal = step_table()[row].clone()
    if same_sigma:
        scal[1] = scal[0]
    sigma, sigma_next = scal[0].item(), scal[1].item()
    assert 0.0 <= sigma_next <= sigma and sigma > 0.0               # |dt / sigma| <= 1 (module docstring)
    return scal, sigma, sigma_next


def _big_lat():
    blk = _f(4, BIG_HW, seed=601, scale=50.0)
    fr = (1.0 + (torch.arange(BIG_T) % 89).float() / 128)[:, None, None]
    return (blk[None] * fr).reshape(BIG_T, 4, BIG_H, BIG_W).contiguous()


def _prepare_case(dev, T, HW, row, big=False, seed=44):
    T_, HW_ = (BIG_T, BIG_HW) if big else (T, HW)
    M = 2 * T_ * HW_
    op = "prepare_model_input_dev" if dev else "prepare_model_input"

    def build():
        scal, sigma, _ = _scalars(row)
        if big:                                                     # ldo = 16: the whole row is the view, no guard columns
            lat, img = _big_lat(), _f(2, 4, BIG_H, BIG_W, seed=602)
            base = torch.full((1 + M + 1, 16), NAN, dtype=F16)
            out = View(base, lambda b: b[1:1 + M])
        else:
            lat, img, _ = _step_data(T, HW, "N", seed + T)
            base = torch.full((2 + M + 2, 24), NAN, dtype=F16)
            out = View(base, lambda b: b[2:2 + M, 8:24])
        kw = dict(latents=ac._nchw_view(lat), image_latents=ac._nchw_view(img), out=out)
        kw.update(scal=scal) if dev else kw.update(sigma=sigma)
        return kw

    def ref(kw):
        if dev:
            inv = kw["scal"][4]
            l64, im = prepare_ref(kw["latents"], kw["image_latents"], 1.0, T_, HW_)
            want = kw["out"].clone()
            want[:, :4] = (l64.float() * inv).half()                # one fp32 product, one rounding
            want[:, 4:8] = im.half()
            return [Want(bits=want)]
        l64, im = prepare_ref(kw["latents"], kw["image_latents"], 1.0 / (float(kw["sigma"]) ** 2 + 1.0) ** 0.5, T_, HW_)
        rest = kw["out"].clone()
        rest[:, 4:8] = im.half()
        return [Part((" latents", lambda t: t[:, :4], Want(ref=l64, bound=U16 * l64.abs() + 2.0 ** -25 + 4 * U32 * l64.abs())),
                     (" image / rest", lambda t: t[:, 4:], Want(bits=rest[:, 4:])))]
    tag = f"{op}/" + ("second-pass" if big else f"T{T}-HW{HW}-row{row}")
    return ac.AuxCase(tag, op, build, ref, big=big, T=T_, HW=HW_, row=row, items=2 * T_ * HW_, pair=("prepare", T_, HW_, row, big))


def _euler_case(dev, T, HW, row, family="N", gmin=1.0, gmax=3.0, same_sigma=False, big=False, seed=44):
    T_, HW_ = (BIG_T, BIG_HW) if big else (T, HW)
    M = 2 * T_ * HW_
    op = "cfg_euler_step_dev_" if dev else "cfg_euler_step_"
    assert 0.0 <= gmin <= gmax and gmin > 0.5                       # the ramp's intermediates are <= g; cfg-swap differs

    def build():
        scal, sigma, sigma_next = _scalars(row, same_sigma)
        if big:                                                     # ldn = 8, the four columns at column 4
            lat = _big_lat()
            blk = _h(257 * 1031, 4, seed=603)
            npred = blk.repeat(-(-M // blk.shape[0]), 1)[:M]
            base = torch.full((1 + M + 1, 8), NAN, dtype=F16)
            base[1:1 + M, 4:8] = npred
            np_view = View(base, lambda b: b[1:1 + M, 4:8])
        else:
            lat, _, npred = _step_data(T, HW, family, seed + T)
            base = torch.full((2 + M + 2, 16), NAN, dtype=F16)
            base[2:2 + M, 4:8] = npred
            np_view = View(base, lambda b: b[2:2 + M, 4:8])
        kw = dict(latents=ac._nchw_view(lat), noise_pred=np_view)
        kw.update(scal=scal) if dev else kw.update(sigma=sigma, sigma_next=sigma_next)
        kw.update(gmin=gmin, gmax=gmax)
        return kw

    def ref(kw):
        sigma, sigma_next = (kw["scal"][0].item(), kw["scal"][1].item()) if dev else (kw["sigma"], kw["sigma_next"])
        if same_sigma:
            return [Want(bits=kw["latents"].clone())]
        y, bound = euler_ref(kw["latents"], kw["noise_pred"], sigma, sigma_next, gmin, gmax)
        return [Want(ref=y, bound=bound)]
    tag = f"{op}/" + ("second-pass" if big else f"T{T}-HW{HW}-row{row}-{family}" + ("" if (gmin, gmax) == (1.0, 3.0) else f"-g{gmin:g}-{gmax:g}")
                      + ("-same-sigma" if same_sigma else ""))
    return ac.AuxCase(tag, op, build, ref, big=big, T=T_, HW=HW_, row=row, family=family, gmin=gmin, gmax=gmax, same_sigma=same_sigma,
                      items=T_ * HW_, pair=("euler", T_, HW_, row, family, gmin, gmax, same_sigma, big))


def _step_cases():
    cases = []
    shapes = [(T, HW) for T in STEP_T for HW in STEP_HW]
    picks = [(T, HW, STEP_ROWS[k % 4]) for k, (T, HW) in enumerate(shapes)] + [(25, 257, r) for r in STEP_ROWS] + [(1, 48, 24), (2, 257, 0)]
    for T, HW, row in dict.fromkeys(picks):
        for dev in (False, True):
            cases.append(_prepare_case(dev, T, HW, row))
            cases.append(_euler_case(dev, T, HW, row))
    for dev in (False, True):
        for T, HW, row in ((25, 257, 3), (2, 48, 24), (1, 257, 12)):
            cases.append(_euler_case(dev, T, HW, row, family="V"))
        cases.append(_euler_case(dev, 25, 257, 3, same_sigma=True))
        cases.append(_euler_case(dev, 25, 48, 12, gmin=2.5, gmax=2.5))
        cases.append(_euler_case(dev, 2, 257, 24, family="V", gmin=2.5, gmax=2.5))
    cases.append(_prepare_case(True, 0, 0, 3, big=True))
    cases.append(_euler_case(True, 0, 0, 3, big=True))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------
# the references behind the signatures of mofa_video_amd.ops: impl(None) is a correct implementation, impl(defect) a wrong one
# ---------------------------------------------------------------------------------------------------------------------------
def impl(defect=None):
    def nchw_to_tokens(x, ld=None, scale=1.0, out=None):
        n, C, H, W = x.shape
        if out is not None:
            out[:, :C] = n2t_ref(x, scale, out.stride(0), defect)
            if defect == "pad-cols-written":
                out[:, C:] = 0
            return out
        ld = ld or C
        y = torch.zeros((n * H * W, ld), dtype=F16)
        y[:, :C] = n2t_ref(x, scale, ld, defect)
        return y

    def tokens_to_nchw(x, n, Cc, H, W):
        return t2n_ref(x, n, Cc, H, W, defect)

    def _prepare(latents, image_latents, out, inv, once):
        T, _, h, w = latents.shape
        l64, im = prepare_ref(latents, image_latents, 1.0 if once else inv, T, h * w, defect)
        out[:, :4] = (l64.float() * inv).half() if once else round16(l64)
        out[:, 4:8] = im.half()
        return out

    def prepare_model_input(latents, image_latents, out, sigma):
        return _prepare(latents, image_latents, out, 1.0 / (float(sigma) ** 2 + 1.0) ** 0.5, False)

    def prepare_model_input_dev(latents, image_latents, out, scal):
        return _prepare(latents, image_latents, out, scal[4], True)

    def cfg_euler_step_(latents, noise_pred, sigma, sigma_next, gmin, gmax):
        M = 2 * latents.shape[0] * latents.shape[2] * latents.shape[3]
        if defect == "ldn-ignored":
            noise_pred = torch.as_strided(noise_pred, (M, 4), (4, 1), noise_pred.storage_offset())
        if sigma_next == sigma and defect is None:
            return latents
        latents.copy_(euler_ref(latents, noise_pred, sigma, sigma_next, gmin, gmax, defect)[0].float())
        return latents

    def cfg_euler_step_dev_(latents, noise_pred, scal, gmin, gmax):
        return cfg_euler_step_(latents, noise_pred, scal[0].item(), scal[1].item(), gmin, gmax)
    return types.SimpleNamespace(**{k: v for k, v in locals().items() if callable(v) and not k.startswith("_")})


CASES = _mover_cases() + _step_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
OPS = tuple(dict.fromkeys(c.op for c in CASES))


def pairs():
    """[(host-scalar case, device-scalar case)] over the same data and table row"""
    by = {}
    for c in CASES:
        if "pair" in c.meta:
            by.setdefault(c.meta["pair"], {})[c.op.endswith("dev") or c.op.endswith("dev_")] = c
    return [(v[False], v[True]) for v in by.values() if len(v) == 2]


def mutant_differs(defect, case):
    """from the geometry alone: does the wrong kernel ``defect`` compute something else than the right one on ``case``"""
    m = case.meta
    if case.op not in MUTANT_OPS[defect]:
        return False
    if defect == "tile-transposed":
        return m["C"] > 1 or m["HW"] > 1
    if defect == "drop-c0":
        return m["C"] > 32
    if defect == "image-stride-ld":
        return m["n"] > 1 and m["ldo"] != m["C"]
    if defect == "scale-after-round":      # the planted 65520 becomes inf before it is scaled down; scale > 1: 3e-6 rounds twice
        return m["scale"] != 1.0
    if defect == "pad-cols-written":
        return m["wide"] > m["C"]
    if defect == "ragged-clamp":
        return m["HW"] % 32 > 1           # (a ragged tile of ONE pixel: the clamp meets the pixel itself)
    if defect in ("ldn-ignored", "img-half0"):
        return True
    if defect == "cfg-swap":               # (sigma_next == sigma: the step moves nothing, whatever v is)
        return not m["same_sigma"]
    if defect in ("ramp-div-T", "ramp-pixel"):
        return m["T"] > 1 and m["gmin"] != m["gmax"] and not m["same_sigma"]
    if defect in ("eps-pred", "no-c-skip"):
        return not m["same_sigma"]
    raise KeyError(defect)


def assert_table():
    """the table holds what it is there for"""
    mv = [c for c in CASES if c.op in _MOVERS]
    for op in _MOVERS:                                              # every channel class meets every pixel class, family P
        assert {(c.meta["C"], c.meta["HW"]) for c in mv if c.op == op and c.meta["family"] == "P"} == {(C, HW) for C in MOVER_C for HW in MOVER_HW}
        assert {c.meta["n"] for c in mv if c.op == op} == {1, 3}
        assert any(c.meta["n"] == 3 and c.meta["C"] > 32 and c.meta["HW"] % 32 for c in mv if c.op == op)
    n2t = [c for c in mv if c.op == "nchw_to_tokens"]
    for form in FORMS:                                              # every form with a second channel tile, a ragged pixel tile, n = 3
        sel = [c for c in n2t if c.meta["form"] == form]
        assert any(c.meta["C"] > 32 and c.meta["n"] == 3 for c in sel) and any(c.meta["HW"] % 32 and c.meta["HW"] > 32 for c in sel), form
        assert {c.meta["family"] for c in sel} == {"P", "R"}, form
        assert any(c.meta["C"] == 320 for c in sel), form
    assert all((c.meta["ldo"] > c.meta["C"]) == (c.meta["form"] != "ldC") for c in n2t)
    assert all((c.meta["wide"] == c.meta["C"] + 2) == (c.meta["form"] == "out-wide") for c in n2t)
    assert {c.meta["scale"] for c in n2t if c.meta["family"] == "R"} == set(SCALES)
    assert all(c.meta["scale"] == 1.0 for c in n2t if c.meta["family"] == "P")
    st = [c for c in CASES if c.op in _EULER + _PREP]
    for op in _EULER + _PREP:
        small = [c for c in st if c.op == op and not c.big]
        assert {(c.meta["T"], c.meta["HW"]) for c in small} == {(T, HW) for T in STEP_T for HW in STEP_HW}, op
        assert {c.meta["row"] for c in small} == set(STEP_ROWS), op
        assert {c.meta["row"] for c in small if (c.meta["T"], c.meta["HW"]) == (25, 257)} == set(STEP_ROWS), op
    assert step_table().shape == (25, 8) and step_table()[24, 1].item() == 0.0
    for op in _EULER:
        sel = [c for c in st if c.op == op]
        assert any(c.meta["same_sigma"] for c in sel) and any(c.meta["gmin"] == c.meta["gmax"] for c in sel)
        assert {c.meta["family"] for c in sel} == {"N", "V"}
    big = [c for c in st if c.big]
    assert {c.op for c in big} == {"prepare_model_input_dev", "cfg_euler_step_dev_"}
    for c in st:
        assert (c.meta["items"] > oc.EW_GRID_ITEMS) == c.big, c.id
    assert 257 % 256 and 25 * 257 > 256 * 25                        # a ragged last block, frame boundaries inside blocks
    assert len(pairs()) == len([c for c in st if not c.big]) // 2
