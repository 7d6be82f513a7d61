"""Backward of the warp: gradients through mofa_video_amd.softsplat.softsplat (the HIP backward kernels, include/mofa_hip.h
mofa_softsplat_norm_f32 / _grad_prologue_f32 / _grad_f32) against torch.autograd through oracle.softsplat.softsplat on the CPU
(written in differentiable torch ops, so autograd gives the reference's derivatives: softsplat_func.backward,
MOFA-Video-Traj/models/softsplat.py:349-524, through the wrapper's mode prep and normalisation :243-270).

Errors are max|gpu - cpu| / max|cpu| per gradient.  Measured worst values on MI355X: fp32 modes 1.6e-7 (dI), 2.4e-6 (dF), 1.3e-6
(dm).  'avg': dI 1.5e-7; dF 2.9e-2 (max) at 72 x 128 -- its forward output is the fp16 gather's, and the normaliser's gradient
-sum_c g_c out_c / nu carries that rounding amplified by 1 / nu at targets that receive little weight (the backward treats the
rounding as identity), so 'avg' dF is also bounded in relative L2 norm."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ["sum", "sum-addeps", "avg", "avg-zeroeps", "avg-clipeps", "linear", "linear-addeps", "linear-zeroeps", "linear-clipeps",
         "soft", "soft-addeps", "soft-zeroeps", "soft-clipeps"]


def _flows(N, H, W, seed, mag):
    """random flows plus the special sources (flat pixel index): 0 NaN, 1 inf (last image), 2 an integer shift, 3 far out of
    bounds, 4-8 convergent onto one point; with room, identity over the block [5:8, 10:14] (the targets there see only those
    sources' weights, so their normaliser can be exactly 0)"""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(N, 2, H, W, generator=g) * mag
    fl = f.view(N, 2, H * W)
    fl[0, :, 0] = float("nan")
    fl[-1, 0, 1] = float("inf")
    fl[0, :, 2] = torch.tensor([1.0, -2.0])
    fl[0, :, 3] = torch.tensor([1000.0, 5.0])
    s = torch.arange(4, 9)
    fl[:, 0, 4:9] = 6.3 - (s % W).float()
    fl[:, 1, 4:9] = 0.6 - (s // W).float()
    if H >= 8 and W >= 14:
        f[:, :, 5:8, 10:14] = 0.0
    return f


def _inputs(mode, N, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    base = mode.split("-")[0]
    if mode == "avg":
        x = x.half().float()                      # (the 'avg' forward works on fp16 features)
    if base == "avg" and mode != "avg":
        x = x.abs() + 0.1                         # (reference quirk: 'avg-<suffix>' normalises by the input's own last channel)
        x[:, -1, 5:8, 10:14] = 0.0                # zero normaliser on the identity block
    m = None
    if base in ("linear", "soft"):
        m = torch.randn(N, 1, H, W, generator=g)
        if base == "linear":
            m = m.abs() + 0.1
            m[:, :, 5:8, 10:14] = 0.0
        else:
            m[:, :, 5:8, 10:14] = -200.0          # e^m = 0 in fp32
    return x, _flows(N, H, W, seed + 1, 2.0), m


def _run(fn, x, f, m, mode, gout, dev, need=(True, True, True)):
    """forward + torch.autograd.grad of sum(out * gout) w.r.t. the inputs marked in `need` -> (out, [dI, dF, dm])"""
    ins = [x.to(dev).clone(), f.to(dev).clone(), m.to(dev).clone() if m is not None else None]
    for t, r in zip(ins, need):
        if t is not None and r:
            t.requires_grad_(True)
    out = fn(ins[0], ins[1], ins[2], mode)
    req = [t for t in ins if t is not None and t.requires_grad]
    grads = iter(torch.autograd.grad((out * gout.to(dev)).sum(), req))
    return out.detach(), [next(grads) if (t is not None and t.requires_grad) else None for t in ins]


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    assert a.shape == b.shape and torch.isfinite(a).all() and torch.isfinite(b).all()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _compare(mode, x, f, m, tol, what="", l2=2e-3):
    from mofa_video_amd.softsplat import softsplat
    from oracle.softsplat import softsplat as softsplat_ref
    C = x.shape[1] - (1 if mode.startswith("avg-") else 0)
    gout = torch.randn(x.shape[0], C, x.shape[2], x.shape[3], generator=torch.Generator().manual_seed(7))
    _, got = _run(softsplat, x, f, m, mode, gout, DEV)
    _, ref = _run(softsplat_ref, x, f, m, mode, gout, "cpu")
    errs = [_rel(a, b) if b is not None else 0.0 for a, b in zip(got, ref)]
    e2 = _rel_l2(got[1], ref[1])
    print(f"softsplat grad {mode} {what} {tuple(x.shape)}: rel err dI {errs[0]:.2e} dF {errs[1]:.2e} dm {errs[2]:.2e}; dF rel-L2 {e2:.2e}")
    if mode == "avg":                               # dI carries no fp16 term; dF: see the module docstring
        assert errs[0] <= 2e-5 and errs[1] <= tol and e2 <= l2, (mode, errs, e2)
    else:
        for e, name in zip(errs, ("dI", "dF", "dm")):
            assert e <= tol, (mode, name, e)
    return got


@pytest.mark.parametrize("mode", MODES)
def test_gradients_every_mode_vs_oracle(mode):
    x, f, m = _inputs(mode, 2, 5, 12, 20, 11)
    _compare(mode, x, f, m, 5e-3 if mode == "avg" else 2e-5)


@pytest.mark.parametrize("mode", ["avg", "linear-clipeps", "sum"])
def test_non_finite_and_out_of_bounds_sources_get_exact_zeros(mode):
    from mofa_video_amd.softsplat import softsplat
    N, C, H, W = 2, 4, 12, 20
    x, f, m = _inputs(mode, N, C, H, W, 21)
    f[1, :, 6, 6] = torch.tensor([-50.0, 0.5])                    # all four corners left of the image
    f[1, :, 7, 7] = torch.tensor([0.25, 40.0])                    # all four corners below it
    gout = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(22))
    _, (dI, dF, dm) = _run(softsplat, x, f, m, mode, gout, DEV)
    for n, y, xx in ((0, 0, 0), (1, 0, 1), (0, 0, 3), (1, 6, 6), (1, 7, 7)):
        assert torch.equal(dI[n, :, y, xx].cpu(), torch.zeros(C)), (n, y, xx)
        assert torch.equal(dF[n, :, y, xx].cpu(), torch.zeros(2)), (n, y, xx)
        if dm is not None:
            assert dm[n, 0, y, xx].item() == 0.0, (n, y, xx)


def _dyadic_inputs(mode, N, C, H, W, seed):
    """inputs whose splat sums are exact in fp32 (eighths, quarter-pixel flows, e^0 = 1), so the atomicAdd forward of the
    scatter-based modes gives the same bits in every run and separate forwards can be compared bit for bit"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-16, 17, (N, C, H, W), generator=g).float() / 8
    if mode.startswith("avg-"):
        x[:, -1] = torch.randint(1, 9, (N, H, W), generator=g).float() / 4
    f = torch.randint(-12, 13, (N, 2, H, W), generator=g).float() / 4
    f[0, :, 0, 0] = float("nan")
    m = None
    if mode.startswith("linear"):
        m = torch.randint(1, 9, (N, 1, H, W), generator=g).float() / 4
    elif mode.startswith("soft"):
        m = torch.zeros(N, 1, H, W)
    return x, f, m


@pytest.mark.parametrize("mode", ["avg", "soft-clipeps", "linear", "avg-zeroeps", "sum"])
def test_gradient_subsets_are_bit_identical_to_the_full_run(mode):
    from mofa_video_amd.softsplat import softsplat
    x, f, m = _dyadic_inputs(mode, 2, 70, 12, 20, 31)
    C = x.shape[1] - (1 if mode.startswith("avg-") else 0)
    gout = torch.randn(2, C, 12, 20, generator=torch.Generator().manual_seed(32))
    _, full = _run(softsplat, x, f, m, mode, gout, DEV)
    for i in range(3 if m is not None else 2):
        need = [j == i for j in range(3)]
        _, part = _run(softsplat, x, f, m, mode, gout, DEV, need=need)
        for j in range(3):
            if j == i:
                assert torch.equal(part[j], full[j]), (mode, i)
            else:
                assert part[j] is None, (mode, i, j)


@pytest.mark.parametrize("mode", MODES)
def test_backward_is_deterministic(mode):
    """every mode: two backward passes from one forward are bit-identical; 'avg' also across two forward + backward runs"""
    from mofa_video_amd.softsplat import softsplat
    x, f, m = _inputs(mode, 2, 40, 16, 24, 41)
    ins = [x.to(DEV).requires_grad_(), f.to(DEV).requires_grad_(), m.to(DEV).requires_grad_() if m is not None else None]
    req = [t for t in ins if t is not None]
    out = softsplat(ins[0], ins[1], ins[2], mode)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(42)).to(DEV)
    a = torch.autograd.grad(out, req, gout, retain_graph=True)
    b = torch.autograd.grad(out, req, gout)
    for u, v in zip(a, b):
        assert torch.equal(u, v), mode
    if mode == "avg":
        out2 = softsplat(ins[0], ins[1], None, mode)
        c = torch.autograd.grad(out2, req, gout)
        assert torch.equal(out, out2)
        for u, v in zip(a, c):
            assert torch.equal(u, v)


@pytest.mark.parametrize("mode", ["avg", "avg-clipeps", "soft"])
def test_forward_unchanged_by_grad_tracking(mode):
    from mofa_video_amd.softsplat import softsplat
    x, f, m = _inputs(mode, 2, 16, 12, 20, 51)
    x, f = x.to(DEV), f.to(DEV)
    m = m.to(DEV) if m is not None else None
    with torch.no_grad():
        ref = softsplat(x, f, m, mode)
    out = softsplat(x.clone().requires_grad_(), f, m, mode)
    assert out.grad_fn is not None
    if mode == "avg":                               # the deterministic gather: bit for bit
        assert torch.equal(out.detach(), ref)
    else:                                           # the atomicAdd scatter (the reference's own order class)
        assert _rel(out.detach(), ref) < 1e-6


@pytest.mark.parametrize("C", [1, 3, 320, 1280])
@pytest.mark.parametrize("mode", ["avg", "soft-zeroeps", "sum"])
def test_shapes_three_images_one_row(mode, C):
    x, f, m = _inputs(mode, 3, C, 1, 100, 61)
    f = f.clone()
    f[:, 1] = f[:, 1] * 0.2                         # (H = 1: keep some targets on the row)
    _compare(mode, x, f, m, 5e-3 if mode == "avg" else 2e-5, what="H=1")


@pytest.mark.parametrize("mode", ["avg", "linear-addeps"])
def test_non_contiguous_inputs(mode):
    from mofa_video_amd.softsplat import softsplat
    from oracle.softsplat import softsplat as softsplat_ref
    x, f, m = _inputs(mode, 2, 24, 12, 20, 71)
    gout = torch.randn(2, 24, 12, 20, generator=torch.Generator().manual_seed(72))

    def nc(t, dev):                                 # a channels-last copy, and a transposed view of it
        return t.to(dev).contiguous(memory_format=torch.channels_last).transpose(2, 3).contiguous().transpose(2, 3)
    got, ref = [], []
    for fn, dev, out in ((softsplat, DEV, got), (softsplat_ref, "cpu", ref)):
        ins = [nc(x, dev).requires_grad_(), nc(f, dev).requires_grad_(), nc(m, dev).requires_grad_() if m is not None else None]
        assert not ins[0].is_contiguous()
        o = fn(ins[0], ins[1], ins[2], mode)
        out.extend(torch.autograd.grad((o * gout.to(dev)).sum(), [t for t in ins if t is not None]))
    for a, b in zip(got, ref):
        assert _rel(a, b) <= (5e-3 if mode == "avg" else 2e-5)


@pytest.mark.parametrize("C,H,W", [(320, 72, 128), (320, 36, 64), (640, 18, 32), (1280, 9, 16)])
def test_adapter_level_sizes(C, H, W):
    """one 'avg' warp per pyramid level of a 576 x 1024 clip (the adapter's four feature levels), N = 1 as the training loop calls
    it.  Against the fp32 oracle the flow gradient carries the fp16 output's rounding (module docstring; measured max 2.9e-2,
    rel-L2 9.9e-3 at 72 x 128); against the spec with that output itself -- ghat_c = g_c / nu, ghat_last = -sum_c g_c out_c / nu
    from the forward's own fp16 result, back through the oracle's sum splat of [I | 1] -- it is fp32 summation noise"""
    from mofa_video_amd.softsplat import softsplat
    from oracle.softsplat import softsplat_sum
    x, f, _ = _inputs("avg", 1, C, H, W, 81)
    f = f * 2.0
    _, dF, _ = _compare("avg", x, f, None, 6e-2, l2=2e-2, what="level")
    with torch.no_grad():
        out = softsplat(x.to(DEV), f.to(DEV), None, "avg").cpu()
    gout = torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(7))
    xin = torch.cat([x, torch.ones(1, 1, H, W)], 1)
    fr = f.clone().requires_grad_()
    S = softsplat_sum(xin, fr)
    nu = S[:, -1:].detach() + 0.0000001
    ghat = torch.cat([gout / nu, -(gout * out).sum(1, keepdim=True) / nu], 1)
    dF_spec, = torch.autograd.grad(S, [fr], ghat)
    e = _rel(dF, dF_spec)
    print(f"softsplat grad avg level {(C, H, W)}: dF vs the spec on the fp16 output {e:.2e}")
    assert e < 1e-4, e


def test_training_chain_conv_grads_vs_oracle():
    """nn.Conv2d -> 24 per-flow 'avg' warps written as the reference's training model writes them (svdxt_..._norefine.py:231:
    .float() in, .to(torch.float16) out) -> a weighted loss: the conv weight and bias gradients against the same chain on the CPU"""
    from mofa_video_amd.softsplat import softsplat
    from oracle.softsplat import softsplat as softsplat_ref
    g = torch.Generator().manual_seed(91)
    H, W, C = 16, 24, 32
    img = torch.randn(1, 4, H, W, generator=g)
    flows = torch.randn(1, 24, 2, H, W, generator=g) * 3.0
    wts = torch.randn(24, 1, C, H, W, generator=g)
    conv = torch.nn.Conv2d(4, C, 3, padding=1)
    res = []
    for fn, dev in ((softsplat, DEV), (softsplat_ref, "cpu")):
        cv = torch.nn.Conv2d(4, C, 3, padding=1).to(dev)
        cv.load_state_dict(conv.state_dict())
        first_frame = cv(img.to(dev))
        fl = flows.to(dev)
        warped = [fn(first_frame.float(), fl[:, i].float(), None, "avg").to(torch.float16) for i in range(24)]
        loss = sum((wts[i].to(dev) * w.float()).sum() for i, w in enumerate(warped))
        loss.backward()
        res.append((cv.weight.grad, cv.bias.grad))
    e = [_rel(a, b) for a, b in zip(*res)]
    print(f"training chain: conv weight grad rel err {e[0]:.2e}, bias {e[1]:.2e}")
    assert max(e) < 2e-3, e


@pytest.mark.parametrize("mode", ["avg", "soft", "sum"])
def test_autocast_fp16_inputs(mode):
    from mofa_video_amd.softsplat import softsplat
    x, f, m = _inputs(mode, 2, 16, 12, 20, 101)
    x, f = x.half().float(), f.half().float()
    m = m.half().float() if m is not None else None
    gout = torch.randn(2, 16, 12, 20, generator=torch.Generator().manual_seed(102)).to(DEV)
    _, ref = _run(softsplat, x, f, m, mode, gout, DEV)
    ins = [x.half().to(DEV).requires_grad_(), f.half().to(DEV).requires_grad_(), m.half().to(DEV).requires_grad_() if m is not None else None]
    with torch.autocast("cuda", dtype=torch.float16):
        out = softsplat(ins[0], ins[1], ins[2], mode)
    assert out.dtype == torch.float32
    got = torch.autograd.grad((out * gout).sum(), [t for t in ins if t is not None])
    for a, b in zip(got, [r for r in ref if r is not None]):
        assert a.dtype == torch.float16
        assert _rel(a, b) < 2e-3
