"""TEST INFRASTRUCTURE ONLY: one table of cases for every function tests/emu_ops.py stands in for, runnable through either side.

``tests/emu_ops.py`` holds the torch-CPU stand-ins the ``-m "not gpu"`` suite monkeypatches over ``mofa_video_amd.ops``; whatever
those tests say about the host code holds only as far as a stand-in means what its HIP entry point means.  A ``Case`` names the
op and builds its keyword arguments as seeded CPU tensors; ``run(module, case, device)`` moves them to ``device`` and calls
``getattr(module, case.op)(**kwargs)``, so the identical case goes through ``emu_ops`` on the CPU
(tests/test_op_contract_cpu.py) and through ``mofa_video_amd.ops`` on the GPU (tests/test_op_contract_gpu.py).

Guard layout: every 2-D token matrix is a ``View`` into a larger NaN-filled base buffer -- guard rows before and after it, guard
columns left (8 elements: the 16-byte alignment include/mofa_hip.h asks for) and right of it, a leading dimension that is a
multiple of 8 and DIFFERENT for the different arguments of one call.  After the call everything outside the view of a written
argument, and all of a read-only argument, must be bit-unchanged (``Run.guard_errors``: compared through an integer view, so a
NaN that was overwritten by another NaN pattern or by a number shows); a stray read that reaches the result shows as a
non-finite output.  Pure outputs start as NaN as well: an element the op leaves unwritten stays non-finite.

Every argument is passed by keyword, so the table itself says which parameters it exercises (``nondefault_params``)."""
import inspect

import torch

from mofa_video_amd import lib as L

F16, F32 = torch.float16, torch.float32
NAN = float("nan")

# tolerance classes: |err| <= tol * max|ref| + tol * |ref| per element (the _close form of tests/test_kernels_gpu.py, whose
# stated figures these are; ff320 / lin320 take the figures of tests/test_ff320_gpu.py / tests/test_lin320_gpu.py)
TOL = {
    "exact": 0.0,                # ops that only move or re-type data, and the exactly representable igemm sums: torch.equal
    "gemm": 2e-3,                # igemm, group_norm, layer_norm, gn_apply_gathered, softmax_rows_
    "lin320": 2e-3,
    "ff320": 3e-3,               # two chained fp16 GEMMs with an fp16 hidden state
    "ff320_ln": 6e-3,            # ... its second output: the LayerNorm of a row that already differs by an fp16 rounding
    "attn_spatial": 4e-3,
    "attn_temporal": 2e-3,
    "attn_temporal_masked": 1e-3,
    "ew16": 1e-3,                # fp16 element-wise
    "temb": 2e-5,                # timestep_embedding
    "ew32": 1e-6,                # fp32 element-wise
    "gn_partial": None,          # fp32 partial sums: bound derived from the entry's row count (test_op_contract_gpu.py)
    "int": None,                 # host query returning an int: equality
}

# arguments an op writes whatever the case (an ``out`` / ``ln_out`` buffer is added where a case passes one)
WRITES = {"axpby_": ("y",), "axpby_f32_": ("y",), "copy2d": ("dst",), "softmax_rows_": ("x",), "gn_partial_into": ("part_rows",),
          "cfg_euler_step_": ("latents",), "cfg_euler_step_dev_": ("latents",)}
EW_GRID_ITEMS = 16384 * 256      # csrc/elementwise.hip ew_blocks: more items than this and the grid-stride loop runs a second pass


def _h(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).half()


def _f(*shape, seed=0, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def _ints(lo, hi, *shape, seed=0):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


class View:
    """an argument that is a view ``cut(base)`` into a larger base buffer; everything of ``base`` outside the view is guard"""

    def __init__(self, base, cut):
        self.base, self.cut = base, cut


def guard(data=None, shape=None, ld=None, dtype=F16, rows=(3, 2), col=8, trim=(0, 0)):
    """``data`` (or a NaN-filled ``shape``: a pure output) as a view into a NaN buffer of leading dimension ``ld`` with
    ``rows`` guard rows before / after and ``col`` guard columns to the left; ``trim`` = (a, b): the view leaves out the first a
    and the last b rows of ``data``, which then are real rows in front of and behind it (halo frames)"""
    if data is not None:
        shape, dtype = tuple(data.shape), data.dtype
    M, C = shape
    ld = ld if ld is not None else (col + C + 15) // 8 * 8
    assert ld % 8 == 0 and col % 8 == 0 and ld >= col + C, (ld, col, C)
    base = torch.full((rows[0] + M + rows[1], ld), NAN, dtype=dtype)
    if data is not None:
        base[rows[0]:rows[0] + M, col:col + C] = data
    r0, r1 = rows[0] + trim[0], rows[0] + M - trim[1]
    return View(base, lambda b: b[r0:r1, col:col + C])


class Case:
    def __init__(self, id, op, build, tol):
        self.id, self.op, self.build, self.tol = id, op, build, tol

    def __repr__(self):
        return self.id


class Placed:
    """one tensor argument on the device: ``t`` = what the op receives, ``buf`` = its whole base buffer, ``snap`` = the buffer
    before the call, ``inside`` = mask of the buffer's elements that belong to ``t``"""

    def __init__(self, spec, device):
        if isinstance(spec, View):
            self.buf = spec.base.to(device).clone()
            self.t = spec.cut(self.buf)
            self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=device)
            spec.cut(self.inside)[...] = True
            self.cut = spec.cut
        else:
            assert spec.is_contiguous(), "a strided argument goes into the table as a View of its base"
            self.buf = spec.to(device).clone()
            self.t = self.buf
            self.inside = torch.ones(self.buf.shape, dtype=torch.bool, device=device)
            self.cut = lambda b: b
        self.snap = self.buf.clone()

    def before(self):
        """the argument as it was before the call"""
        return self.cut(self.snap)


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


class Run:
    def __init__(self, case, kwargs, placed, ret):
        self.case, self.kwargs, self.placed, self.ret = case, kwargs, placed, ret
        self.writes = tuple(n for n in placed if n in WRITES.get(case.op, ()) or n in ("out", "ln_out[2]"))

    def guard_errors(self):
        """what the call changed that it must not: guards of written arguments, anything of read-only ones"""
        bad = []
        for name, p in self.placed.items():
            diff = bits(p.buf) != bits(p.snap)
            if name in self.writes:
                diff = diff & ~p.inside
            n = int(diff.sum())
            if n:
                where = torch.nonzero(diff)[0].tolist()
                bad.append(f"{self.case.id}: {n} elements of {'the guard of ' if name in self.writes else 'read-only '}{name} changed, first at {where}")
        return bad

    def outputs(self):
        """[(label, result tensor on the CPU, the same memory before the call or None for a fresh tensor)]: the returned
        tensor(s), then every written argument that was not returned"""
        rets = [] if self.ret is None else (list(self.ret) if isinstance(self.ret, (tuple, list)) else [self.ret])
        out, seen = [], []
        for i, r in enumerate(rets):
            if not torch.is_tensor(r):
                out.append((f"ret{i}", r, None))
                continue
            src = [p for p in self.placed.values() if p.t is r]
            seen += src
            out.append((f"ret{i}", r.detach().cpu(), src[0].before().cpu() if src else None))
        for name in self.writes:
            p = self.placed[name]
            if not any(p is s for s in seen):
                out.append((name, p.t.detach().cpu(), p.before().cpu()))
        return out


def run(module, case, device="cpu", drop=()):
    """call ``case`` through ``module`` (tests/emu_ops.py or mofa_video_amd.ops) with its tensors on ``device``.  ``drop``: leave
    out the ``out`` argument or the buffer of ``ln_out`` (``"ln_out[2]"``), for the fresh-output form of the same call"""
    kw = dict(case.build())
    for d in drop:
        if d == "ln_out[2]":
            kw["ln_out"] = tuple(kw["ln_out"][:2])
        else:
            del kw[d]
    placed = {}

    def place(name, v):
        if isinstance(v, View) or torch.is_tensor(v):
            placed[name] = Placed(v, device)
            return placed[name].t
        if isinstance(v, tuple) and any(isinstance(e, View) or torch.is_tensor(e) for e in v):
            return tuple(place(f"{name}[{i}]", e) for i, e in enumerate(v))
        return v
    call = {k: place(k, v) for k, v in kw.items()}
    ret = getattr(module, case.op)(**call)
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    return Run(case, call, placed, ret)


def _fresh_pairs(r):
    """[(argument to drop for the fresh-output form, index of the matching return value)] of a run"""
    from mofa_video_amd import ops
    pairs = []
    if "out" in r.placed and "out" in defaults(getattr(ops, r.case.op)):
        pairs.append(("out", 0))
    if "ln_out[2]" in r.placed:
        pairs.append(("ln_out[2]", 1))
    return pairs


def check_out_is_honoured(module, case, device, r):
    """wherever ``out=`` (or the buffer of ``ln_out``) is given: the returned tensor IS that buffer, holds bit for bit what
    the call without it returns, and columns of a wider buffer beyond the result's stay as they were"""
    for drop, i in _fresh_pairs(r):
        rets = r.ret if isinstance(r.ret, (tuple, list)) else [r.ret]
        p = r.placed[drop]
        assert rets[i] is p.t, f"{case.id}: the call with {drop} does not return that buffer"
        fresh = run(module, case, device, drop=(drop,))
        assert not fresh.guard_errors(), fresh.guard_errors()
        f = (fresh.ret if isinstance(fresh.ret, (tuple, list)) else [fresh.ret])[i]
        assert torch.isfinite(f.float()).all(), f"{case.id}: non-finite fresh output"
        if p.t.shape == f.shape:
            assert same_bits(p.t, f), f"{case.id}: {drop} holds other bits than the fresh output"
        else:
            n = f.shape[1]
            assert p.t.dim() == 2 and p.t.shape[0] == f.shape[0] and p.t.shape[1] > n, (case.id, p.t.shape, f.shape)
            assert same_bits(p.t[:, :n], f), f"{case.id}: {drop} holds other bits than the fresh output"
            assert same_bits(p.t[:, n:], p.before()[:, n:]), f"{case.id}: columns of {drop} beyond the result's {n} were written"


def close_errors(out, ref, tol, what):
    """|err| <= tol * max|ref| + tol * |ref| per element -> (worst err / bound, message or None)"""
    out, ref = out.double(), ref.double()
    if out.shape != ref.shape:
        return float("inf"), f"{what}: shape {tuple(out.shape)} != {tuple(ref.shape)}"
    if not torch.isfinite(out).all():
        return float("inf"), f"{what}: non-finite output"
    scale = ref.abs().max().item() + 1e-12
    err = (out - ref).abs()
    bound = tol * scale + tol * ref.abs()
    worst = (err / bound).max().item() if out.numel() else 0.0
    bad = err > bound
    if bad.any():
        return worst, (f"{what}: {int(bad.sum())} / {bad.numel()} elements out of tolerance {tol:g}; max err {err.max().item():.4e} "
                       f"(scale {scale:.4e}) at {int(err.argmax())}")
    return worst, None


def defaults(fn):
    """{parameter: default} of the parameters that have one"""
    return {n: p.default for n, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def is_default(value, default):
    from mofa_video_amd import ops
    if isinstance(default, ops.ConvGeom) or default is None:
        return value is None or (isinstance(value, ops.ConvGeom) and value.mode == L.MODE_PLAIN)
    if isinstance(value, (View, torch.Tensor, tuple)) and not isinstance(default, tuple):
        return False
    return value == default


def nondefault_params(cases, fn):
    """names of the parameters of ``fn`` that take a non-default value in at least one of ``cases`` (read off the table)"""
    dflt = defaults(fn)
    hit = set()
    for c in cases:
        for k, v in c.build().items():
            if k not in dflt or not is_default(v, dflt[k]):
                hit.add(k)
    return hit


# ---------------------------------------------------------------------------------------------------------------------------
# implicit GEMM
# ---------------------------------------------------------------------------------------------------------------------------
def _igemm_plain_all():
    """M tiles by no tile height (128 / 192 / 256), bias, a row vector taken as rows of a 3 x wider fp32 matrix (rv_mul carries
    the stride), two residuals, all three scale factors != 1, out wider than N, tile forced"""
    M, N, K = 333, 192, 128
    wide = _f(48, 3 * N, seed=4)                                   # row idx = (m // 7) * 3 in units of N = row m // 7 of `wide`
    return dict(x=guard(_h(M, K, seed=1), ld=152), w=_h(N, K, seed=2, scale=0.1), bias=_f(N, seed=3),
                rowvec=View(wide, lambda b: b[:, N:2 * N]), rv=(7, 3, 1, 1 << 30),
                r1=guard(_h(M, N, seed=5), ld=216), s1=0.5, r2=guard(_h(M, N, seed=6), ld=232), s2=-1.25, s_acc=0.75,
                out=guard(shape=(M, N + 16), ld=248), tile=L.TILE_128X128)


def _igemm_plain_rv():
    M, N, K = 77, 2560, 128
    return dict(x=guard(_h(M, K, seed=7)), w=_h(N, K, seed=8, scale=0.1), bias=_f(N, seed=9), rowvec=_f(5, N, seed=10),
                rv=(7, 3, 4, 5), r1=guard(_h(M, N, seed=11)), s1=0.5, s_acc=0.75)


def _igemm_act(act, with_r1=False):
    def build():
        M, N, K = 260, 96, 128
        kw = dict(x=guard(_h(M, K, seed=12), ld=168), w=_h(N, K, seed=13, scale=0.1), bias=_f(N, seed=14), act=act,
                  out=guard(shape=(M, N), ld=136))
        if with_r1:
            kw.update(r1=guard(_h(M, N, seed=15), ld=120), s1=0.5, s_acc=1.5)
        return kw
    return build


def _igemm_geglu():
    from mofa_video_amd.weights import interleave_geglu
    M, Cc = 200, 64
    wi, bi = interleave_geglu(_h(8 * Cc, Cc, seed=16, scale=0.2), _f(8 * Cc, seed=17))
    return dict(x=guard(_h(M, Cc, seed=18)), w=wi, bias=bi, act=L.ACT_GEGLU_PAIR, out=guard(shape=(M, 4 * Cc + 8), ld=288))


def _igemm_conv(H, W, stride=1, up=1, ksize=3, dil=1, pad=L.PAD_SAME, seed=20):
    def build():
        from mofa_video_amd import ops
        from mofa_video_amd.weights import pack_conv3x3
        n, Cin, Cout = 2, 64, 48
        x = _h(n, Cin, H, W, seed=seed)
        w = _h(Cout, Cin, ksize, ksize, seed=seed + 1, scale=0.15 / ksize)
        geom = ops.conv3x3_geom(H, W, stride=stride, up=up, ksize=ksize, dil=dil, pad=pad)
        M = n * geom.Hout * geom.Wout
        return dict(x=guard(x.permute(0, 2, 3, 1).reshape(n * H * W, Cin), ld=88), w=pack_conv3x3(w), bias=_f(Cout, seed=seed + 2),
                    geom=geom, r1=guard(_h(M, Cout, seed=seed + 3), ld=72), s1=0.5, out=guard(shape=(M, Cout), ld=64))
    return build


def _igemm_convt(T):
    """T > 0: clips of T frames, zero padding at the clip ends.  T == 0: unclipped with M=, the halo frames are real rows in
    front of and behind the view (then the NaN guard rows)"""
    def build():
        from mofa_video_amd import ops
        from mofa_video_amd.weights import pack_conv3d_t3
        HW, Cc, N = 33, 64, 96
        w = pack_conv3d_t3(_h(N, Cc, 3, 1, 1, seed=31, scale=0.1))
        if T > 0:
            M = 2 * T * HW
            return dict(x=guard(_h(M, Cc, seed=30)), w=w, bias=_f(N, seed=32), geom=ops.convt3_geom(T, HW),
                        r1=guard(_h(M, N, seed=33)), s1=1.0)
        M = 3 * HW                                                   # a rank that owns 3 frames, halo = one frame either side
        return dict(x=guard(_h(M + 2 * HW, Cc, seed=30), ld=80, trim=(HW, HW)), w=w, bias=_f(N, seed=32), geom=ops.convt3_geom(0, HW),
                    M=M, out=guard(shape=(M, N), ld=112))
    return build


def _igemm_exact_residual():
    """operands whose products and sums are EXACT in fp32 (small integers x multiples of 2^-6; bias on the 2^-6 grid up to 16;
    residuals on the 2^-6 grid, |r| <= 8): s_acc * (acc + bias) is a multiple of 3 * 2^-8 of magnitude up to ~15 -- exact in fp32,
    mostly NOT representable in fp16 above 4 -- so the documented rounding of that term to fp16 before the residuals are added
    (include/mofa_hip.h) changes the final fp16 value in a good share of the elements, and no summation order can: both sides
    must give the literal round16(round16(s_acc * acc) + s1 r1 + s2 r2), bit for bit"""
    M, N, K = 300, 64, 512
    return dict(x=guard(_ints(-3, 3, M, K, seed=40).half(), ld=536), w=(_ints(-2, 2, N, K, seed=41) / 64).half(),
                bias=_ints(-1024, 1024, N, seed=42) / 64, r1=guard((_ints(-512, 512, M, N, seed=43) / 64).half(), ld=88), s1=0.5,
                r2=guard((_ints(-512, 512, M, N, seed=44) / 64).half(), ld=104), s2=0.25, s_acc=0.75)


# ---------------------------------------------------------------------------------------------------------------------------
# lin320 / ff320 (kinds of tests/test_lin320_gpu.py / tests/test_ff320_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------
def _lin320(kind, M, N):
    def build():
        from mofa_video_amd.weights import pack_lin320
        g = torch.Generator().manual_seed(N + len(kind))
        w = (torch.randn(N, 320, generator=g) * 320 ** -0.5).half()
        every = kind == "all"
        b = torch.randn(N, generator=g) * 0.3 if ("bias" in kind or every) else None
        norm = "norm" in kind or every
        gamma, beta = (1 + 0.2 * torch.randn(320, generator=g), 0.2 * torch.randn(320, generator=g)) if norm else (None, None)
        wp, bp = pack_lin320(w, b, gamma, beta)
        kw = dict(x=guard(_h(M, 320, seed=M, scale=1.2, shift=0.3), ld=344), wp=wp)
        if bp is not None:
            kw["bias"] = bp
        if norm:
            kw["norm"] = True
        if every:
            kw.update(rowvec=_f(5, N, seed=50, scale=0.5), rv=(7, 3, 4, 5), s_acc=0.75, eps=1e-6)
        if "rvwide" in kind:
            wide = _f((M - 1) // 100 + 1, 2 * N, seed=51, scale=0.5)
            kw.update(rowvec=View(wide, lambda t: t[:, N:]), rv=(100, 2, 1, 1 << 30))
        if "r1" in kind or every:
            kw.update(r1=guard(_h(M, N, seed=52), ld=N + 40), s1=0.5 if every else 1.0)
        if "out" in kind or every:
            kw["out"] = guard(shape=(M, N + 8), ld=N + 56)
        return kw
    return build


def _ff320_params(seed, gain_spread=0.2):
    g = torch.Generator().manual_seed(seed)
    w1 = (torch.randn(2560, 320, generator=g) * 320 ** -0.5).half()
    b1 = torch.randn(2560, generator=g) * 0.1
    w2 = (torch.randn(320, 1280, generator=g) * 1280 ** -0.5).half()
    b2 = torch.randn(320, generator=g) * 0.1
    gamma, beta = 1 + gain_spread * torch.randn(320, generator=g), 0.2 * torch.randn(320, generator=g)
    return w1, b1, w2, b2, gamma, beta


def _ff320(kind, M):
    def build():
        from mofa_video_amd.weights import pack_ff320
        w1, b1, w2, b2, gamma, beta = _ff320_params(3)
        w1p, b1f, w2p = pack_ff320(w1, b1, w2, gamma, beta)
        kw = dict(x=guard(_h(M, 320, seed=M, scale=1.3, shift=0.2), ld=352), w1p=w1p, b1=b1f, w2p=w2p, b2=b2)
        if "pos" in kind:
            kw.update(pos=_f(5, 320, seed=60, scale=0.5), HW=7, T=5)
        if "r2" in kind:
            kw.update(r2=guard(_h(M, 320, seed=61), ld=368), s_acc=0.6, s1=0.6, s2=0.4)
        if "out" in kind:
            kw["out"] = guard(shape=(M, 328), ld=384)
        if "eps" in kind:
            kw.update(eps=2e-5, ln_eps=3e-5)
        if "ln" in kind:
            ln = (1 + 0.1 * _f(320, seed=62), 0.1 * _f(320, seed=63))
            kw["ln_out"] = ln + (guard(shape=(M, 328), ld=400),) if "lnbuf" in kind else ln
        return kw
    return build


# ---------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------
def _attn_spatial(S, heads, frames, hd, out=False, prescaled=False, scale=None, query_blocks=0, seed=70):
    def build():
        from mofa_video_amd.ops import Q_FOLD_LOG2E
        Cc, M = heads * hd, frames * S
        q = _h(M, Cc, seed=seed)
        kw = dict(k=guard(_h(M, Cc, seed=seed + 1), ld=Cc + 40), v=guard(_h(M, Cc, seed=seed + 2), ld=Cc + 56),
                  nframes=frames, heads=heads, S=S, head_dim=hd)
        if prescaled:                                                # the constant folded into Q before its single fp16 rounding
            q = (q.float() * (hd ** -0.5 * Q_FOLD_LOG2E)).half()
            kw["prescaled"] = True
        kw["q"] = guard(q, ld=Cc + 24)
        if scale is not None:
            kw["scale"] = scale
        if query_blocks:
            kw["query_blocks"] = query_blocks
        if out:
            kw["out"] = guard(shape=(M, Cc), ld=Cc + 72)
        return kw
    return build


def _attn_temporal(T, HW, heads, clips, hd, Tq=None, masked=(), out=False, scale=None, seed=80):
    """k / v in two buffers of one leading dimension (ops.attn_temporal asserts ld(k) == ld(v)), q and out of others; ``masked``:
    key frames without their mask bit, whose K / V rows hold NaN (never-written padding of the gathered buffer)"""
    def build():
        Cc = heads * hd
        k, v = _h(clips * T * HW, Cc, seed=seed + 1), _h(clips * T * HW, Cc, seed=seed + 2)
        kw = dict(nclips=clips, T=T, HW=HW, heads=heads, head_dim=hd)
        if masked:
            mask = (1 << T) - 1
            for j in masked:
                mask &= ~(1 << j)
                for c in range(clips):
                    k[(c * T + j) * HW:(c * T + j + 1) * HW] = NAN
                    v[(c * T + j) * HW:(c * T + j + 1) * HW] = NAN
            kw["key_mask"] = mask
        nq = T if Tq is None else Tq
        if Tq is not None:
            kw["Tq"] = Tq
        kw.update(q=guard(_h(clips * nq * HW, Cc, seed=seed), ld=Cc + 24), k=guard(k, ld=Cc + 40), v=guard(v, ld=Cc + 40))
        if scale is not None:
            kw["scale"] = scale
        if out:
            kw["out"] = guard(shape=(clips * nq * HW, Cc), ld=Cc + 56)
        return kw
    return build


# ---------------------------------------------------------------------------------------------------------------------------
# normalisation
# ---------------------------------------------------------------------------------------------------------------------------
def _group_norm(C, HW, frames, fps=1, silu=False, out_extra=None, xw=None, eps=1e-5, seed=90):
    def build():
        x = _h(frames * HW, xw or C, seed=seed, shift=0.5)
        kw = dict(x=guard(x), gamma=_f(C, seed=seed + 1), beta=_f(C, seed=seed + 2), nframes=frames, HW=HW, eps=eps)
        if fps != 1:
            kw["frames_per_stat"] = fps
        if silu:
            kw["silu"] = True
        if xw:
            kw["C_"] = C
        if out_extra is not None:
            kw["out"] = guard(shape=(frames * HW, C + out_extra), ld=C + out_extra + 24)
        return kw
    return build


GN_SHARD = dict(C=64, HW=150, frames=(3, 2, 2))      # 7 frames as 3 + 2 + 2: slots of 3 frames in the gathered buffer


def gn_shard_x(rank=None):
    """fp16 frames of the sharded GroupNorm cases: all 7, or those of one rank"""
    C, HW, fr = GN_SHARD["C"], GN_SHARD["HW"], GN_SHARD["frames"]
    x = _h(sum(fr) * HW, C, seed=100, shift=0.5)
    if rank is None:
        return x
    f0 = sum(fr[:rank])
    return x[f0 * HW:(f0 + fr[rank]) * HW]


def _gn_partial_into(rank):
    """the rank's partial entries into ITS rows of the gather buffer (the other ranks' rows are the guard)"""
    def build():
        import emu_ops
        C, HW, fr = GN_SHARD["C"], GN_SHARD["HW"], GN_SHARD["frames"]
        nparts, slot = emu_ops.gn_nparts(HW, C), max(fr)
        base = torch.full((len(fr) * slot * nparts, 64), NAN)
        r0 = rank * slot * nparts
        return dict(x=guard(gn_shard_x(rank), ld=96), part_rows=View(base, lambda b: b[r0:r0 + fr[rank] * nparts]),
                    nframes=fr[rank], HW=HW)
    return build


def gn_order_frames(HW, C, nparts):
    """two frames whose rows are constant over a chunk and distinct from chunk to chunk and frame to frame"""
    rpc = -(-HW // nparts)
    val = 0.25 * (1 + torch.arange(HW) // rpc).float()
    return torch.cat([val, val + 8.0])[:, None].expand(2 * HW, C).half().contiguous()


def _gn_partial_order():
    import emu_ops
    C, HW = 64, 600
    nparts = emu_ops.gn_nparts(HW, C)
    return dict(x=guard(gn_order_frames(HW, C, nparts)), part_rows=torch.full((2 * nparts, 64), NAN), nframes=2, HW=HW)


def _gn_apply_gathered(rank, silu, out_extra):
    """part_all: the gathered buffer of all three ranks, one entry per real frame holding its fp64 sums (the frame's other
    entries and the padding frames' entries are zero: the applying kernel only adds entries up)"""
    def build():
        import emu_ops
        C, HW, fr = GN_SHARD["C"], GN_SHARD["HW"], GN_SHARD["frames"]
        nparts, slot = emu_ops.gn_nparts(HW, C), max(fr)
        xd = gn_shard_x().double().reshape(sum(fr), HW, 32, C // 32)
        part = torch.zeros(len(fr) * slot * nparts, 64)
        f = 0
        for r, n in enumerate(fr):
            for i in range(n):
                part[(r * slot + i) * nparts] = torch.stack([xd[f].sum((0, 2)), (xd[f] ** 2).sum((0, 2))], -1).reshape(64).float()
                f += 1
        M = fr[rank] * HW
        kw = dict(x=guard(gn_shard_x(rank), ld=88), part_all=part, count_per_group=float(sum(fr) * HW * (C // 32)),
                  gamma=_f(C, seed=101), beta=_f(C, seed=102), eps=1e-5, out=guard(shape=(M, C + out_extra), ld=C + out_extra + 32),
                  nframes=fr[rank], HW=HW)
        if silu:
            kw["silu"] = True
        return kw
    return build


def _layer_norm(C, M, rowvec=False, out_extra=None, eps=1e-5, seed=110):
    def build():
        kw = dict(x=guard(_h(M, C, seed=seed, scale=2.0, shift=0.3)), gamma=_f(C, seed=seed + 1), beta=_f(C, seed=seed + 2))
        if eps != 1e-5:
            kw["eps"] = eps
        if rowvec:
            kw.update(rowvec=_f(3, C, seed=seed + 3), rv_div=10, rv_mod=3)
        if out_extra is not None:
            kw["out"] = guard(shape=(M, C + out_extra), ld=C + out_extra + 40)
        return kw
    return build


# ---------------------------------------------------------------------------------------------------------------------------
# element-wise (small, and > EW_GRID_ITEMS items: the second pass of the grid-stride loop)
# ---------------------------------------------------------------------------------------------------------------------------
BIG_ROWS, BIG_COLS = 16400, 2056                     # 16400 * 257 vectors of 8 halves = 4 214 800 > 4 194 304
BIG_N = EW_GRID_ITEMS + 20333
assert BIG_ROWS * (BIG_COLS // 8) > EW_GRID_ITEMS


def _big16(seed):
    """seeded fp16 [BIG_ROWS, BIG_COLS] without drawing 34 M normals: a small random block tiled with a per-row scale"""
    blk = _h(257, BIG_COLS, seed=seed)
    reps = -(-BIG_ROWS // 257)
    row = (1.0 + (torch.arange(reps * 257) % 89).float() / 128)[:, None].half()
    return (blk.repeat(reps, 1) * row)[:BIG_ROWS]


def _axpby_(big):
    def build():
        if big:
            return dict(x=guard(_big16(120), ld=2072, rows=(1, 1)), y=guard(_big16(121), ld=2080, rows=(1, 1)), a=0.5, b=2.0)
        return dict(x=guard(_h(50, 64, seed=120), ld=88), y=guard(_h(50, 64, seed=121), ld=104), a=0.5, b=2.0)
    return build


def _axpby_out(big):
    def build():
        if big:
            return dict(x=guard(_big16(122), ld=2072, rows=(1, 1)), y=guard(_big16(123), ld=2080, rows=(1, 1)), a=-0.75, b=1.5,
                        out=guard(shape=(BIG_ROWS, BIG_COLS), ld=2088, rows=(1, 1)))
        return dict(x=guard(_h(50, 64, seed=122), ld=88), y=guard(_h(50, 64, seed=123), ld=104), a=-0.75, b=1.5,
                    out=guard(shape=(50, 64), ld=120))
    return build


def _copy2d(big):
    def build():
        if big:
            return dict(src=guard(_big16(124), ld=2072, rows=(1, 1)), dst=guard(shape=(BIG_ROWS, BIG_COLS), ld=2088, rows=(1, 1)))
        return dict(src=guard(_h(40, 64, seed=124), ld=88), dst=guard(shape=(40, 64), ld=104))
    return build


def _axpby_f32_(n, overwrite):
    def build():
        x = _f(n, seed=125)
        if overwrite:                                                # b == 0 overwrites: y may hold anything, NaN included
            return dict(x=x, y=torch.full((n,), NAN), a=0.5, b=0.0)
        return dict(x=x, y=_f(n, seed=126), a=0.25, b=-1.5)
    return build


def _cast(to, n, out=False):
    def build():
        shape = (n // 8, 8) if n % 8 == 0 else (n,)
        if to == "f16":
            return dict(x=_f(*shape, seed=127, scale=30.0))
        kw = dict(x=_h(*shape, seed=128, scale=30.0))
        if out:
            kw["out"] = torch.full(shape, NAN)
        return kw
    return build


# ---------------------------------------------------------------------------------------------------------------------------
# the rest
# ---------------------------------------------------------------------------------------------------------------------------
def _transpose_v():
    frames, ncb, S = 2, 3, 200
    return dict(v=guard(_h(frames * S, ncb * 64, seed=130), ld=232), nframes=frames, ncb=ncb, S=S)


def _softmax_rows_():
    return dict(x=guard(_h(33, 520, seed=131, scale=3.0), ld=552))


def _nchw_to_tokens(kind):
    def build():
        n, C, H, W = 2, 3, 7, 9
        kw = dict(x=_f(n, C, H, W, seed=132))
        if kind == "ld":
            kw["ld"] = 64
        elif kind == "scale":
            kw.update(ld=8, scale=0.18215)
        else:       # out= a column slice of a wider buffer (the adapter's x[:, C:C + 2] form), scaled
            M = n * H * W
            base = torch.full((M + 4, 24), NAN, dtype=F16)
            kw.update(scale=0.5 if kind == "out-scale" else 1.0, out=View(base, lambda b: b[2:2 + M, 8:8 + C + 2]))
        return kw
    return build


def _tokens_to_nchw():
    n, Cc, H, W = 2, 3, 7, 9
    return dict(x=guard(_h(n * H * W, 8, seed=133), ld=24), n=n, Cc=Cc, H=H, W=W)


def _patchify():
    return dict(x=_f(2, 3, 8, 12, seed=134), p=2, ld=16)


def _filter1d(axis, k):
    def build():
        taps = torch.rand(k, generator=torch.Generator().manual_seed(135 + k))
        return dict(x=torch.rand(2, 3, 11, 13, generator=torch.Generator().manual_seed(136)), taps=taps / taps.sum(), axis=axis)
    return build


def _resize_bicubic():
    return dict(x=torch.rand(2, 3, 11, 13, generator=torch.Generator().manual_seed(137)), Ho=7, Wo=19)


def _resize_nearest():
    return dict(x=torch.rand(2, 48, 80, generator=torch.Generator().manual_seed(138)), h=7, w=11)      # ratios 6.86 / 7.27


def _timestep_embedding():
    return dict(t=torch.tensor([1.6378, 6.0, 128.0, 0.02, 24.0]), dim=320)


def _silu_f32():
    return dict(x=_f(300, seed=139, scale=3.0))


def _gn_nparts(HW, Cc):
    return lambda: dict(HW=HW, Cc=Cc)


CASES = [
    Case("igemm/plain-all", "igemm", _igemm_plain_all, "gemm"),
    Case("igemm/plain-rv", "igemm", _igemm_plain_rv, "gemm"),
    Case("igemm/silu", "igemm", _igemm_act(L.ACT_SILU), "gemm"),
    Case("igemm/relu", "igemm", _igemm_act(L.ACT_RELU), "gemm"),
    Case("igemm/gelu", "igemm", _igemm_act(L.ACT_GELU), "gemm"),
    Case("igemm/silu-r1", "igemm", _igemm_act(L.ACT_SILU, with_r1=True), "gemm"),
    Case("igemm/geglu-pair", "igemm", _igemm_geglu, "gemm"),
    Case("igemm/conv3-s2", "igemm", _igemm_conv(10, 14, stride=2), "gemm"),
    Case("igemm/conv3-up2", "igemm", _igemm_conv(5, 7, up=2), "gemm"),
    Case("igemm/conv1", "igemm", _igemm_conv(9, 13, ksize=1), "gemm"),
    Case("igemm/conv5", "igemm", _igemm_conv(9, 13, ksize=5), "gemm"),
    Case("igemm/conv7", "igemm", _igemm_conv(11, 9, ksize=7), "gemm"),
    Case("igemm/conv3-dil2", "igemm", _igemm_conv(9, 13, dil=2), "gemm"),
    Case("igemm/conv3-s2-trailing", "igemm", _igemm_conv(9, 13, stride=2, pad=L.PAD_TRAILING), "gemm"),
    Case("igemm/convt-T5", "igemm", _igemm_convt(5), "gemm"),
    Case("igemm/convt-halo", "igemm", _igemm_convt(0), "gemm"),
    Case("igemm/exact-residual", "igemm", _igemm_exact_residual, "exact"),
    Case("lin320/plain-N64-M33", "lin320", _lin320("plain", 33, 64), "lin320"),
    Case("lin320/norm-bias-out", "lin320", _lin320("norm+bias+out", 300, 320), "lin320"),
    Case("lin320/rvwide-r1", "lin320", _lin320("rvwide+r1", 300, 64), "lin320"),
    Case("lin320/all-N960", "lin320", _lin320("all", 256 + 77, 960), "lin320"),
    Case("ff320/plain-M300", "ff320", _ff320("plain", 300), "ff320"),
    Case("ff320/ln-M33", "ff320", _ff320("ln", 33), "ff320"),
    Case("ff320/pos-r2-out-lnbuf-eps", "ff320", _ff320("pos+r2+out+lnbuf+eps", 128 * 2 + 37), "ff320"),
    Case("attn_spatial/hd64-S200-out", "attn_spatial", _attn_spatial(200, 3, 2, 64, out=True), "attn_spatial"),
    Case("attn_spatial/hd128-S72-prescaled", "attn_spatial", _attn_spatial(72, 2, 2, 128, prescaled=True), "attn_spatial"),
    Case("attn_spatial/hd64-qb1-scale", "attn_spatial", _attn_spatial(136, 2, 1, 64, scale=0.2, query_blocks=1), "attn_spatial"),
    Case("attn_spatial/hd64-qb2-S256", "attn_spatial", _attn_spatial(256, 2, 1, 64, out=True, query_blocks=2), "attn_spatial"),
    Case("attn_temporal/T1", "attn_temporal", _attn_temporal(1, 9, 1, 1, 64), "attn_temporal"),
    Case("attn_temporal/T25-clips2-out-scale", "attn_temporal", _attn_temporal(25, 11, 2, 2, 64, out=True, scale=0.3), "attn_temporal"),
    Case("attn_temporal/T32-hd128", "attn_temporal", _attn_temporal(32, 5, 1, 1, 128), "attn_temporal"),
    Case("attn_temporal/T32-Tq5-masked-nan-out", "attn_temporal",
         _attn_temporal(32, 7, 2, 2, 64, Tq=5, masked=(7, 20, 31), out=True), "attn_temporal_masked"),
    Case("group_norm/fps1", "group_norm", _group_norm(64, 37, 3), "gemm"),
    Case("group_norm/fps3-silu-wide-out", "group_norm", _group_norm(64, 150, 6, fps=3, silu=True, out_extra=16, eps=1e-6), "gemm"),
    Case("group_norm/C_-narrower-than-x", "group_norm", _group_norm(64, 37, 2, xw=96), "gemm"),
    Case("group_norm/HW9215", "group_norm", _group_norm(32, 9215, 1), "gemm"),
    Case("group_norm/HW9216-fps2", "group_norm", _group_norm(32, 9216, 2, fps=2, out_extra=0), "gemm"),
    Case("gn_partial_into/rank0-of-3+2+2", "gn_partial_into", _gn_partial_into(0), "gn_partial"),
    Case("gn_partial_into/rank1-of-3+2+2", "gn_partial_into", _gn_partial_into(1), "gn_partial"),
    Case("gn_partial_into/order", "gn_partial_into", _gn_partial_order, "gn_partial"),
    Case("gn_apply_gathered/rank0", "gn_apply_gathered", _gn_apply_gathered(0, False, 0), "gemm"),
    Case("gn_apply_gathered/rank2-silu-wide-out", "gn_apply_gathered", _gn_apply_gathered(2, True, 16), "gemm"),
    Case("gn_nparts/small", "gn_nparts", _gn_nparts(150, 64), "int"),
    Case("gn_nparts/large", "gn_nparts", _gn_nparts(36864, 320), "int"),
    Case("layer_norm/plain", "layer_norm", _layer_norm(64, 33), "gemm"),
    Case("layer_norm/rowvec-out-view-eps", "layer_norm", _layer_norm(320, 101, rowvec=True, out_extra=0, eps=1e-6), "gemm"),
    Case("layer_norm/C1280-wide-out", "layer_norm", _layer_norm(1280, 50, out_extra=8), "gemm"),
    Case("axpby_/small", "axpby_", _axpby_(False), "ew16"),
    Case("axpby_/second-pass", "axpby_", _axpby_(True), "ew16"),
    Case("axpby_out/small", "axpby_out", _axpby_out(False), "ew16"),
    Case("axpby_out/second-pass", "axpby_out", _axpby_out(True), "ew16"),
    Case("copy2d/small", "copy2d", _copy2d(False), "exact"),
    Case("copy2d/second-pass", "copy2d", _copy2d(True), "exact"),
    Case("axpby_f32_/small", "axpby_f32_", _axpby_f32_(1000, False), "ew32"),
    Case("axpby_f32_/overwrite-nan", "axpby_f32_", _axpby_f32_(1000, True), "ew32"),
    Case("axpby_f32_/second-pass", "axpby_f32_", _axpby_f32_(BIG_N, False), "ew32"),
    Case("axpby_f32_/second-pass-overwrite-nan", "axpby_f32_", _axpby_f32_(BIG_N, True), "ew32"),
    Case("cast_f32_to_f16/small", "cast_f32_to_f16", _cast("f16", 301), "exact"),
    Case("cast_f32_to_f16/second-pass", "cast_f32_to_f16", _cast("f16", BIG_N), "exact"),
    Case("cast_f16_to_f32/small", "cast_f16_to_f32", _cast("f32", 301), "exact"),
    Case("cast_f16_to_f32/out", "cast_f16_to_f32", _cast("f32", 4 * 6 * 8, out=True), "exact"),
    Case("cast_f16_to_f32/second-pass-out", "cast_f16_to_f32", _cast("f32", BIG_N, out=True), "exact"),
    Case("transpose_v", "transpose_v", _transpose_v, "exact"),
    Case("softmax_rows_", "softmax_rows_", _softmax_rows_, "gemm"),
    Case("nchw_to_tokens/ld", "nchw_to_tokens", _nchw_to_tokens("ld"), "exact"),
    Case("nchw_to_tokens/scale", "nchw_to_tokens", _nchw_to_tokens("scale"), "ew16"),
    Case("nchw_to_tokens/out-column-slice", "nchw_to_tokens", _nchw_to_tokens("out"), "exact"),
    Case("nchw_to_tokens/out-column-slice-scale", "nchw_to_tokens", _nchw_to_tokens("out-scale"), "ew16"),
    Case("tokens_to_nchw", "tokens_to_nchw", _tokens_to_nchw, "exact"),
    Case("patchify", "patchify", _patchify, "exact"),
    Case("filter1d_reflect/axis1-k5", "filter1d_reflect", _filter1d(1, 5), "ew32"),
    Case("filter1d_reflect/axis0-k4", "filter1d_reflect", _filter1d(0, 4), "ew32"),
    Case("resize_bicubic_ac", "resize_bicubic_ac", _resize_bicubic, "ew32"),
    Case("resize_nearest_f32", "resize_nearest_f32", _resize_nearest, "exact"),
    Case("timestep_embedding", "timestep_embedding", _timestep_embedding, "temb"),
    Case("silu_f32", "silu_f32", _silu_f32, "ew32"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def cases_of(op):
    return [c for c in CASES if c.op == op]
