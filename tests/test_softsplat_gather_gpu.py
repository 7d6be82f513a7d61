"""The fp32 gather forward of the warp (include/mofa_hip.h, mofa_softsplat_gather_f32; mofa_video_amd.softsplat.GATHER_F32) against
the CPU oracle: the raw sum bit for bit, every mode string within the 2e-5 the fp32 modes are held to, reproducible, and -- the
point of it -- 'avg' gradients on fp32 features that were never rounded to fp16 at fp32 accuracy.

Bounds: 2e-5 in the metric of test_kernels_gpu._close for forwards (what test_softsplat_modes_vs_oracle holds the fp32 modes to)
and 2e-5 in test_softsplat_grad_gpu._rel for gradients (what _compare grants every fp32 mode).  The training-accuracy bound is
measured in the test itself: 'linear' with m = 1 through the atomicAdd scatter forward and the same backward kernels.

Measured on MI355X (profiles/softsplat_gather_bench.log; every figure is printed before it is asserted): all 13 mode strings
bit-equal to the oracle except 'soft*' (expf against torch.exp, max err 4.8e-7); convergent flow 2 x 320 @ 72 x 128 bit-equal, 4.3 ms
against 2.6 ms ('sum', the atomicAdd scatter) and 46 ms ('avg', the fp16 gather and its serial sort); 'avg' gradients on fp32
features, worst level (320 @ 72 x 128): dI 1.2e-7, dF 2.7e-5 -- the same figures as 'linear' with m = 1 through the scatter forward
(the fp16 path: dF 2.9e-2)."""
import contextlib
import time

import pytest
import torch

from test_kernels_gpu import _close
from test_softsplat_grad_gpu import MODES, _flows, _inputs, _rel, _run

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEVELS = [(320, 72, 128), (320, 36, 64), (640, 18, 32), (1280, 9, 16)]


@contextlib.contextmanager
def _switch(on, deterministic=False):
    from mofa_video_amd import softsplat as S
    saved = (getattr(S, "GATHER_F32", False), torch.are_deterministic_algorithms_enabled())
    S.GATHER_F32 = on
    torch.use_deterministic_algorithms(deterministic)
    try:
        yield
    finally:
        S.GATHER_F32 = saved[0]
        torch.use_deterministic_algorithms(saved[1])


def _inputs32(mode, N, C, H, W, seed):
    """_inputs, with the 'avg' feature as drawn: fp32, not rounded to fp16"""
    x, f, m = _inputs(mode, N, C, H, W, seed)
    if mode == "avg":
        x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(seed))
        assert not torch.equal(x, x.half().float())
    return x, f, m


def _dev(t):
    return t.to(DEV) if t is not None else None


def _splat_on(x, f, m, mode):
    from mofa_video_amd.softsplat import softsplat
    with _switch(True), torch.no_grad():
        return softsplat(_dev(x), _dev(f), _dev(m), mode)


# ---- 5. exact against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(12, 20), (36, 64)])
@pytest.mark.parametrize("C", [1, 5, 70])
def test_raw_sum_is_bit_equal_to_the_oracle(C, H, W):
    from mofa_video_amd import ops
    from oracle.softsplat import softsplat_sum
    x = torch.randn(2, C, H, W, generator=torch.Generator().manual_seed(100 + C))
    f = _flows(2, H, W, 200 + C, 2.0)
    ref = softsplat_sum(x, f)
    for slices in sorted({None, 1, min(2, C), C}, key=str):
        out, norm = ops.softsplat_gather_f32(x.to(DEV), f.to(DEV), slices=slices)
        assert norm is None and out.dtype == torch.float32
        assert torch.equal(out.cpu(), ref), (C, H, W, slices, (out.cpu() - ref).abs().max().item())


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_vs_oracle_on_fp32_features(mode):
    from oracle.softsplat import softsplat as softsplat_ref
    for N, C, H, W, seed in ((2, 5, 12, 20, 11), (2, 40, 16, 24, 41)):
        x, f, m = _inputs32(mode, N, C, H, W, seed)
        out = _splat_on(x, f, m, mode).cpu()
        ref = softsplat_ref(x, f, m, mode)
        print(f"softsplat gather {mode} {tuple(x.shape)}: bit-equal to the oracle: {torch.equal(out, ref)}; "
              f"max err {(out - ref).abs().max().item():.2e} (scale {ref.abs().max().item():.2e})")
        _close(out, ref, tol=2e-5, what=f"softsplat gather {mode}")


# ---- 6. reproducible -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_two_forwards_and_batch_splits_give_the_same_bits(mode):
    x, f, m = _inputs32(mode, 3, 40, 16, 24, 141)
    a = _splat_on(x, f, m, mode)
    b = _splat_on(x, f, m, mode)
    assert torch.equal(a, b), mode
    for n in range(3):
        one = _splat_on(x[n:n + 1], f[n:n + 1], m[n:n + 1] if m is not None else None, mode)
        assert torch.equal(one, a[n:n + 1]), (mode, n)


@pytest.mark.parametrize("prep,normalize,eps", [(1, True, 0), (0, True, 1), (2, True, 2), (3, True, 0)])
def test_output_does_not_depend_on_norm_or_slices(prep, normalize, eps):
    from mofa_video_amd import ops
    mode = {1: "avg", 0: "avg-zeroeps", 2: "linear-clipeps", 3: "soft"}[prep]
    x, f, m = _inputs32(mode, 2, 70, 12, 20, 151)
    m = _dev(m.reshape(2, 12, 20)) if m is not None else None
    base, none = ops.softsplat_gather_f32(x.to(DEV), f.to(DEV), m, prep, normalize, eps)
    assert none is None
    norms = []
    for slices in (None, 1, 2, base.shape[1]):
        out, norm = ops.softsplat_gather_f32(x.to(DEV), f.to(DEV), m, prep, normalize, eps, want_norm=True, slices=slices)
        assert torch.equal(out, base), (mode, slices)
        assert tuple(norm.shape) == (2, 1, 12, 20)
        norms.append(norm)
    for nm in norms[1:]:
        assert torch.equal(nm, norms[0])


@pytest.mark.parametrize("mode", ["sum", "soft", "linear-clipeps"])
def test_deterministic_flag_moves_the_scatter_modes_onto_the_gather(mode):
    from mofa_video_amd.softsplat import softsplat
    x, f, m = _inputs32(mode, 2, 40, 16, 24, 161)
    on = _splat_on(x, f, m, mode)
    with _switch(False, deterministic=True), torch.no_grad():
        a = softsplat(_dev(x), _dev(f), _dev(m), mode)
        b = softsplat(_dev(x), _dev(f), _dev(m), mode)
    assert torch.equal(a, b) and torch.equal(a, on), mode


# ---- 7. special sources ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sum", "avg", "avg-addeps", "avg-zeroeps", "avg-clipeps", "avg-raw", "linear", "linear-zeroeps",
                                  "linear-clipeps", "linear-raw", "soft-zeroeps", "soft-raw"])
def test_special_sources_and_zero_normalisers(mode):
    """NaN / inf flow, all four corners outside, an integer shift, the identity block whose normaliser is exactly 0 under each eps
    mode ('-raw': an unknown suffix, the reference divides by the channel as it is): the oracle's values where they are finite
    (bit for bit; 'soft*' within 2e-5, expf against torch.exp), the oracle's non-finite pattern elsewhere"""
    from oracle.softsplat import softsplat as softsplat_ref
    N, C, H, W = 2, 6, 12, 20
    x, f, m = _inputs32(mode, N, C, H, W, 171)
    f[1, :, 6, 6] = torch.tensor([-50.0, 0.5])                    # all four corners left of the image
    f[1, :, 7, 7] = torch.tensor([0.25, 40.0])                    # all four corners below it
    f[1, :, 2, 5] = torch.tensor([3.0, 2.0])                      # integer shifts
    f[1, :, 2, 6] = torch.tensor([-6.0, -2.0])
    out = _splat_on(x, f, m, mode).cpu()
    ref = softsplat_ref(x, f, m, mode)
    fin = torch.isfinite(ref)
    print(f"softsplat gather {mode}: {(~fin).sum().item()} non-finite reference values; bit-equal on the finite ones: "
          f"{torch.equal(out[fin], ref[fin])}")
    assert torch.equal(torch.isnan(out), torch.isnan(ref)), mode
    assert torch.equal(torch.isinf(out), torch.isinf(ref)) and torch.equal(out[torch.isinf(ref)], ref[torch.isinf(ref)]), mode
    if mode.endswith("-raw"):
        assert not fin.all()                                     # (the case is there: 0 / 0 on the identity block)
    if mode.startswith("soft"):
        _close(torch.where(fin, out, 0.0), torch.where(fin, ref, 0.0), tol=2e-5, what=mode)
    else:
        assert torch.equal(out[fin], ref[fin]), (mode, (out[fin] - ref[fin]).abs().max().item())


# ---- 8. convergent flow --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["avg", "sum"])
def test_convergent_flow_value_bits_and_time(mode):
    """the two flows of test_softsplat_convergent_flow at 72 x 128, C = 320: up to 4 HW entries on one target.  The long segments
    are walked in the oracle's order by a whole workgroup, so the result stays bit-equal; the second, synchronised call may take
    at most twice the time of today's path on the same input (the fp16 gather for 'avg', the atomicAdd scatter for 'sum')"""
    from mofa_video_amd.softsplat import softsplat
    from oracle.softsplat import softsplat as softsplat_ref
    H, W, C = 72, 128, 320
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    flow = torch.stack([40.3 - xs, 30.6 - ys], 0)[None].repeat(2, 1, 1, 1)       # all sources -> (40.3, 30.6)
    flow[1] = flow[1] * 0.9                                                       # second flow: a tight cluster
    x = torch.randn(2, C, H, W, generator=torch.Generator().manual_seed(45))
    xd, fd = x.to(DEV), flow.to(DEV)
    times = {}
    outs = {}
    with torch.no_grad():
        for name, on in (("parent", False), ("gather", True), ("parent2", False), ("gather2", True)):
            with _switch(on):
                first = softsplat(xd, fd, None, mode)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                second = softsplat(xd, fd, None, mode)
                torch.cuda.synchronize()
                times[name] = time.perf_counter() - t0
                outs[name] = (first, second)
    t_parent, t_gather = min(times["parent"], times["parent2"]), min(times["gather"], times["gather2"])
    ref = softsplat_ref(x, flow, None, mode)
    out = outs["gather"][1].cpu()
    print(f"softsplat gather convergent {mode} 2 x {C} @ {H}x{W}: gather {t_gather * 1e3:.2f} ms, today's path {t_parent * 1e3:.2f} ms "
          f"(each the faster of two synchronised second calls: {[round(v * 1e3, 2) for v in times.values()]}); "
          f"bit-equal to the oracle: {torch.equal(out, ref)}; max err {(out - ref).abs().max().item():.2e}")
    assert torch.equal(outs["gather"][0], outs["gather"][1]) and torch.equal(outs["gather"][0], outs["gather2"][1])
    _close(out, ref, tol=2e-5, what=f"softsplat gather, convergent flow, {mode}")
    assert torch.equal(out, ref), mode
    assert t_gather <= 2.0 * t_parent, (mode, t_gather, t_parent)


# ---- 9. training accuracy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", LEVELS)
def test_adapter_levels_avg_gradients_on_fp32_features(C, H, W):
    """one 'avg' warp per pyramid level, fp32 features that were not rounded to fp16, switch on: dI and dF against autograd through
    the oracle.  The yardstick is measured on the same inputs: 'linear' with m = 1 -- mathematically 'avg', fp32 end to end through
    the atomicAdd scatter forward and the same backward kernels; the switch-on errors may be at most the larger of twice that
    run's (only the forward's summation order differs) and the 2e-5 every fp32 mode is granted."""
    from mofa_video_amd.softsplat import softsplat
    from oracle.softsplat import softsplat as softsplat_ref
    x, f, _ = _inputs32("avg", 1, C, H, W, 81)
    f = f * 2.0
    ones = torch.ones(1, 1, H, W)
    gout = torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(7))
    _, ref = _run(softsplat_ref, x, f, None, "avg", gout, "cpu")
    with _switch(True):
        out_on, got = _run(softsplat, x, f, None, "avg", gout, DEV)
    with _switch(False):
        _, base = _run(softsplat, x, f, ones, "linear", gout, DEV, need=(True, True, False))
    e_on = [_rel(got[i], ref[i]) for i in range(2)]
    e_base = [_rel(base[i], ref[i]) for i in range(2)]
    e_fwd = _rel(out_on, softsplat_ref(x, f, None, "avg"))
    print(f"softsplat gather avg level {(C, H, W)}: rel err dI {e_on[0]:.2e} dF {e_on[1]:.2e} (forward {e_fwd:.2e}); "
          f"'linear', m = 1 through the scatter: dI {e_base[0]:.2e} dF {e_base[1]:.2e}")
    for i, name in enumerate(("dI", "dF")):
        assert e_on[i] <= max(2.0 * e_base[i], 2e-5), (name, e_on[i], e_base[i])


# ---- 10. backward wiring -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_gradients_every_mode_vs_oracle_with_the_switch_on(mode):
    from mofa_video_amd.softsplat import softsplat
    from oracle.softsplat import softsplat as softsplat_ref
    x, f, m = _inputs32(mode, 2, 5, 12, 20, 11)
    C = x.shape[1] - (1 if mode.startswith("avg-") else 0)
    gout = torch.randn(2, C, 12, 20, generator=torch.Generator().manual_seed(7))
    with _switch(True):
        _, got = _run(softsplat, x, f, m, mode, gout, DEV)
    _, ref = _run(softsplat_ref, x, f, m, mode, gout, "cpu")
    errs = [_rel(a, b) if b is not None else 0.0 for a, b in zip(got, ref)]
    print(f"softsplat gather grad {mode}: rel err dI {errs[0]:.2e} dF {errs[1]:.2e} dm {errs[2]:.2e}")
    for e, name in zip(errs, ("dI", "dF", "dm")):
        assert e <= 2e-5, (mode, name, e)


def test_avg_backward_builds_no_second_csr():
    from mofa_video_amd import ops
    from mofa_video_amd.softsplat import softsplat
    x, f, _ = _inputs32("avg", 2, 16, 12, 20, 181)
    gout = torch.randn(2, 16, 12, 20, generator=torch.Generator().manual_seed(182))
    calls = []
    real = ops.softsplat_norm_f32

    def counted(flow):
        calls.append(1)
        return real(flow)
    ops.softsplat_norm_f32 = counted
    try:
        with _switch(True):
            _run(softsplat, x, f, None, "avg", gout, DEV)
        assert calls == []
        with _switch(False):
            _run(softsplat, x, f, None, "avg", gout, DEV)
        assert calls == [1]                         # (the wrapper counts: the fp16 path still rebuilds it)
    finally:
        ops.softsplat_norm_f32 = real


@pytest.mark.parametrize("mode", ["avg", "soft-clipeps", "linear", "avg-zeroeps", "sum"])
def test_gradient_subsets_are_bit_identical_on_non_dyadic_inputs(mode):
    from mofa_video_amd.softsplat import softsplat
    x, f, m = _inputs32(mode, 2, 70, 12, 20, 31)
    C = x.shape[1] - (1 if mode.startswith("avg-") else 0)
    gout = torch.randn(2, C, 12, 20, generator=torch.Generator().manual_seed(32))
    with _switch(True):
        out_full, full = _run(softsplat, x, f, m, mode, gout, DEV)
        with torch.no_grad():
            plain = softsplat(_dev(x), _dev(f), _dev(m), mode)
        assert torch.equal(plain, out_full), mode        # forward unchanged by grad tracking, bit for bit
        for i in range(3 if m is not None else 2):
            need = [j == i for j in range(3)]
            out_part, part = _run(softsplat, x, f, m, mode, gout, DEV, need=need)
            assert torch.equal(out_part, out_full), (mode, i)
            for j in range(3):
                if j == i:
                    assert torch.equal(part[j], full[j]), (mode, i)
                else:
                    assert part[j] is None, (mode, i, j)


@pytest.mark.parametrize("mode", ["avg", "soft", "sum"])
def test_autocast_fp16_inputs_with_the_switch_on(mode):
    from mofa_video_amd.softsplat import softsplat
    x, f, m = _inputs(mode, 2, 16, 12, 20, 101)
    x, f = x.half().float(), f.half().float()
    m = m.half().float() if m is not None else None
    gout = torch.randn(2, 16, 12, 20, generator=torch.Generator().manual_seed(102)).to(DEV)
    with _switch(True):
        _, ref = _run(softsplat, x, f, m, mode, gout, DEV)
        ins = [x.half().to(DEV).requires_grad_(), f.half().to(DEV).requires_grad_(),
               m.half().to(DEV).requires_grad_() if m is not None else None]
        with torch.autocast("cuda", dtype=torch.float16):
            out = softsplat(ins[0], ins[1], ins[2], mode)
        assert out.dtype == torch.float32
        got = torch.autograd.grad((out * gout).sum(), [t for t in ins if t is not None])
    for a, b in zip(got, [r for r in ref if r is not None]):
        assert a.dtype == torch.float16
        assert _rel(a, b) < 2e-3


@pytest.mark.parametrize("mode", ["avg", "linear-addeps"])
def test_non_contiguous_inputs_with_the_switch_on(mode):
    from mofa_video_amd.softsplat import softsplat
    from oracle.softsplat import softsplat as softsplat_ref
    x, f, m = _inputs32(mode, 2, 24, 12, 20, 71)
    gout = torch.randn(2, 24, 12, 20, generator=torch.Generator().manual_seed(72))

    def nc(t, dev):                                 # a channels-last copy, and a transposed view of it
        return t.to(dev).contiguous(memory_format=torch.channels_last).transpose(2, 3).contiguous().transpose(2, 3)
    got, ref, fwd = [], [], []
    for fn, dev, out in ((softsplat, DEV, got), (softsplat_ref, "cpu", ref)):
        ins = [nc(x, dev).requires_grad_(), nc(f, dev).requires_grad_(), nc(m, dev).requires_grad_() if m is not None else None]
        assert not ins[0].is_contiguous()
        with _switch(True):
            o = fn(ins[0], ins[1], ins[2], mode)
            out.extend(torch.autograd.grad((o * gout.to(dev)).sum(), [t for t in ins if t is not None]))
        fwd.append(o.detach().cpu())
    _close(fwd[0], fwd[1], tol=2e-5, what=f"non-contiguous {mode}")
    for a, b in zip(got, ref):
        assert _rel(a, b) <= 2e-5


# ---- 11. nothing else moved ----------------------------------------------------------------------------------------------------
def test_switch_off_avg_is_the_fp16_token_gather():
    from mofa_video_amd import ops
    from mofa_video_amd import softsplat as S
    N, C, H, W = 2, 24, 12, 20
    x, f, _ = _inputs32("avg", N, C, H, W, 191)
    xd, fd = x.to(DEV), f.to(DEV)
    with _switch(False), torch.no_grad():
        out = S.softsplat(xd, fd, None, "avg")
    for n in range(N):
        tok = ops.nchw_to_tokens(xd[n:n + 1].contiguous(), ld=C)
        ref = ops.tokens_to_nchw(ops.softsplat_avg_tokens(tok, fd[n:n + 1].contiguous(), H, W), 1, C, H, W)
        assert torch.equal(out[n:n + 1], ref), n
    assert not torch.equal(out, _splat_on(x, f, None, "avg"))      # (the fp16 rounding is there: the two paths differ)
