"""Every case of tests/op_cases.py through ``mofa_video_amd.ops`` on the GPU and through its torch-CPU stand-in
(tests/emu_ops.py) on the CPU: the two must mean the same by every argument, or what the ``-m "not gpu"`` suite verifies on the
stand-ins (the host graphs, the frame-sharded exchange at world 2 / 4 / 8) is verified against semantics the GPU does not have.

On the HIP side of every case: guards intact, read-only arguments bit-unchanged, outputs finite, ``out=`` bit-equal to the
fresh-output call.  Between the sides: torch.equal for the ops that only move or re-type data and for the exactly representable
igemm residual sums, the stated tolerance of the op's class otherwise (op_cases.TOL; |err| <= tol * max|ref| + tol * |ref| per
element, the figures of tests/test_kernels_gpu.py, tests/test_ff320_gpu.py and tests/test_lin320_gpu.py).  Each comparison prints
its worst err / bound ratio (pytest -s)."""
import pytest
import torch

import emu_ops
import op_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


def _gn_partial_yardstick(r):
    """fp64 sums of the same fp16 data per entry (frame f, chunk ch = rows [ch * rpc, (ch + 1) * rpc) of the frame, rpc =
    ceil(HW / nparts)) and the bound on an fp32 sum of them.  An entry adds n = rows * (C / 32) numbers per group; ANY order of
    n - 1 fp32 additions of exactly representable terms (fp16 values; their squares enter through one fused multiply-add each)
    is off by at most (n - 1) u sum|x_i| to first order, u = 2^-24 half an fp32 ulp -- i.e. n / 2 ulps of sum|x_i|: a few fp32
    ulps times the entry's row count.  Taken with n instead of n - 1 and 1 % on top for the higher-order terms."""
    x = r.placed["x"].t.detach().cpu().double()
    nframes, HW = r.kwargs["nframes"], r.kwargs["HW"]
    C = x.shape[1]
    nparts = r.placed["part_rows"].t.shape[0] // nframes
    rpc = -(-HW // nparts)
    x = x.reshape(nframes, HW, 32, C // 32)
    want = torch.zeros(nframes, nparts, 32, 2, dtype=torch.float64)
    bound = torch.zeros_like(want)
    for ch in range(nparts):
        blk = x[:, ch * rpc:(ch + 1) * rpc]
        n = blk.shape[1] * (C // 32)
        want[:, ch, :, 0], want[:, ch, :, 1] = blk.sum((1, 3)), (blk * blk).sum((1, 3))
        bound[:, ch, :, 0], bound[:, ch, :, 1] = blk.abs().sum((1, 3)), (blk * blk).sum((1, 3))
        bound[:, ch] *= 1.01 * n * 2.0 ** -24
    return want.reshape(-1, 64), bound.reshape(-1, 64)


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.id)
def test_hip_op_equals_stand_in(ops, case):
    ref = oc.run(emu_ops, case, "cpu")
    got = oc.run(ops, case, DEV)
    assert not got.guard_errors(), got.guard_errors()
    gouts, routs = got.outputs(), ref.outputs()
    assert [o[0] for o in gouts] == [o[0] for o in routs] and gouts, (case.id, [o[0] for o in gouts], [o[0] for o in routs])
    for (label, g, before), (_, r, _) in zip(gouts, routs):
        what = f"{case.id} {label}"
        if not torch.is_tensor(g):
            assert g == r, (what, g, r)
            continue
        assert g.shape == r.shape and g.dtype == r.dtype, (what, g.shape, r.shape, g.dtype, r.dtype)
        written = torch.isfinite(r.float())                       # (pure outputs start as NaN: what the stand-in left is unwritten)
        if before is None:
            assert written.all(), f"{what}: the stand-in's fresh output is not finite"
        else:
            assert bool((oc.bits(g)[~written] == oc.bits(before)[~written]).all()), f"{what}: written where the stand-in does not write"
        assert written.any() and torch.isfinite(g.float()[written]).all(), f"{what}: non-finite output"
        gw, rw = g[written], r[written]
        if case.tol == "exact":
            n = int((gw != rw).sum())
            assert n == 0, f"{what}: {n} / {gw.numel()} elements differ, max |diff| {(gw.float() - rw.float()).abs().max().item():.3e}"
            print(f"CONTRACT {what}: bit-equal ({gw.numel()} elements)")
        elif case.tol == "gn_partial":
            want, bound = _gn_partial_yardstick(got)
            eg, er = (g.double() - want).abs(), (r.double() - want).abs()
            print(f"CONTRACT {what}: worst |err| / bound vs fp64 sums: HIP {(eg / bound).max().item():.3f}, stand-in {(er / bound).max().item():.3f}")
            assert bool((eg <= bound).all()), f"{what}: HIP entries off the fp64 sums by up to {(eg / bound).max().item():.2f} x the bound"
            assert bool((er <= bound).all()), f"{what}: stand-in entries off the fp64 sums by up to {(er / bound).max().item():.2f} x the bound"
        else:
            tol = oc.TOL["ff320_ln" if (case.op == "ff320" and label == "ret1") else case.tol]
            worst, msg = oc.close_errors(gw, rw, tol, what)
            print(f"CONTRACT {what}: worst err / bound {worst:.3f} at tol {tol:g}, max |err| {(gw.double() - rw.double()).abs().max().item():.3e}")
            assert msg is None, msg
    oc.check_out_is_honoured(ops, case, DEV, got)


def test_gn_partial_entry_order(ops):
    """frames that are constant over a chunk, distinct from chunk to chunk and frame to frame: every sum is exact in fp32, so
    the kernel's entries equal the stand-in's bit for bit only if entry f * nparts + ch is chunk ch of frame f on both sides --
    an order error cannot hide in a sum"""
    case = oc.BY_ID["gn_partial_into/order"]
    g = oc.run(ops, case, DEV).placed["part_rows"].t.cpu()
    r = oc.run(emu_ops, case, "cpu").placed["part_rows"].t
    means = r.reshape(-1, 32, 2)[:, 0, 0]
    assert means.unique().numel() == means.numel()                # the case tells every entry from every other
    assert torch.equal(g, r), f"entries differ at {torch.nonzero((g != r).any(1)).flatten().tolist()}"

