"""Every case of tests/aux_cases.py through ``mofa_video_amd.ops`` on the GPU: the CMP pieces of csrc/cmp_ops.hip (``pool2d``, the
two ``resize_bilinear_ac``, ``flow_expectation``) and the blends and movers of csrc/elementwise.hip (``mask_blend``,
``matting_blend``, ``geglu``, ``subsample_tokens``, ``flow_downscale``), which have no stand-in in tests/emu_ops.py.

Per case: guards intact (NaN rows and columns around every view, compared as bits), read-only arguments bit-unchanged, outputs
finite except the one stated infinity, ``out=`` bit-equal to the fresh-output call, and the comparison the table states -- exact
bits, or |out - fp64 reference| <= the derived bound per element (aux_cases docstring; tests/test_aux_cases_cpu.py proves the
references, the exact families and that each check fails on a wrong kernel).  Each comparison prints its worst err / bound
(pytest -s), ``test_worst_ratio_per_op`` the worst per op.  fp16 outputs may sit near 1.0 by the final rounding alone: half an
fp16 ulp is u16 |ref| just above a power of two.

``test_argument_edges_rejected_without_launch`` goes through the C ABI: every call returns MOFA_EINVAL and leaves its NaN-filled
buffers bit-unchanged.  The pool2d calls with a window larger than the padded map are the ones the entry point used to accept
whenever the stride does not divide the (negative) numerator: it computed Hout = (Hin + 2 pad - k) / stride + 1 with C's
division, which truncates towards zero -- Hin = 4, k = 8, stride = 8: -4 / 8 = 0, Hout = 1; Hin = 7, k = 8, stride = 2:
-1 / 2 = 0, Hout = 1 -- and launched one row of output, where ``ops.pool2d`` floors to -1 + 1 = 0 rows and allocates nothing
(Hin = 4, k = 8, stride = 2 gave -2 + 1 = -1 and was rejected by luck of divisibility)."""
import collections

import pytest
import torch

import aux_cases as ac
import op_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = collections.defaultdict(float)


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.mark.parametrize("case", ac.CASES, ids=repr)
def test_hip_op_meets_its_reference(ops, case):
    r = oc.run(ops, case, DEV)
    worst, errs = ac.check_run(case, r)
    off = "; ".join(f"{k.split()[-1]} {n} / {m} elements off the reference rounded once" for k, (n, m) in ac.OFF_ROUNDING.items()
                    if k.startswith(case.id + " "))
    print(f"AUX {case.id}: worst err / bound {worst:.3f} ({off})" if worst else f"AUX {case.id}: bit-equal / exact")
    WORST[case.op] = max(WORST[case.op], worst)
    assert not errs, errs
    if not case.big:                                                 # (the small case of the op proves out= against fresh)
        oc.check_out_is_honoured(ops, case, DEV, r)


def test_worst_ratio_per_op():
    for op in ac.OPS:
        print(f"AUX-WORST {op}: {WORST[op]:.3f}")


def test_argument_edges_rejected_without_launch(ops):
    from mofa_video_amd import lib as L
    lib = L.load()
    st = L.stream_ptr()
    EINVAL = -22
    # sized for the largest output either reading of any argument list below could produce (2 images of at most 16 x 16
    # pixels, 64 channels, 264 logit columns): nothing here can write out of bounds even where a check is missing
    x = torch.full((4096, 64), ac.NAN, dtype=oc.F16, device=DEV)
    y = torch.full((4096, 64), ac.NAN, dtype=oc.F16, device=DEV)
    z = torch.full((4096, 64), ac.NAN, dtype=oc.F16, device=DEV)
    o = torch.full((4096, 64), ac.NAN, dtype=oc.F16, device=DEV)
    f = torch.full((65536,), ac.NAN, dtype=oc.F32, device=DEV)
    fo = torch.full((65536,), ac.NAN, dtype=oc.F32, device=DEV)
    bufs = (x, y, z, o, f, fo)
    snaps = [b.clone() for b in bufs]
    X, Y, Z, O, Fi, Fo = (L.ptr(b) for b in bufs)

    def pool(Hin=8, Win=16, C=8, ldx=64, ldo=64, k=2, stride=2, pad=0, mode=0):
        return lib.mofa_pool2d_f16(X, O, 2, Hin, Win, C, ldx, ldo, k, stride, pad, mode, st)
    calls = {
        "pool2d C % 8": lambda: pool(C=12), "pool2d ldx % 8": lambda: pool(ldx=60), "pool2d ldo % 8": lambda: pool(ldo=60),
        "pool2d mode 2": lambda: pool(mode=2), "pool2d avg with pad": lambda: pool(k=3, pad=1, mode=1),
        "pool2d k 0": lambda: pool(k=0), "pool2d stride 0": lambda: pool(stride=0),
        "pool2d k > Hin, stride 2": lambda: pool(Hin=4, k=8, stride=2), "pool2d k = Hin + 1, stride 2": lambda: pool(Hin=7, k=8, stride=2),
        "pool2d k > Hin, stride 8": lambda: pool(Hin=4, k=8, stride=8),
        "pool2d k > Win, stride 8": lambda: pool(Hin=16, Win=4, k=8, stride=8),
        "pool2d k > Hin + 2 pad": lambda: pool(Hin=2, Win=16, k=8, stride=8, pad=2),
        "pool2d 2 pad > k": lambda: pool(Hin=4, Win=4, k=2, stride=1, pad=2), "pool2d 2 pad > k, k 3": lambda: pool(k=3, stride=2, pad=2),
        "resize Hout 0": lambda: lib.mofa_resize_bilinear_ac_f16(X, O, 2, 4, 6, 0, 6, 8, 64, 64, st),
        "resize Wout 0": lambda: lib.mofa_resize_bilinear_ac_f16(X, O, 2, 4, 6, 4, 0, 8, 64, 64, st),
        "resize C % 8": lambda: lib.mofa_resize_bilinear_ac_f16(X, O, 2, 4, 6, 8, 12, 12, 64, 64, st),
        "resize ld % 8": lambda: lib.mofa_resize_bilinear_ac_f16(X, O, 2, 4, 6, 8, 12, 8, 60, 64, st),
        "resize f32 Hout 0": lambda: lib.mofa_resize_bilinear_ac_f32(Fi, Fo, 4, 4, 6, 0, 6, st),
        "resize f32 Wout 0": lambda: lib.mofa_resize_bilinear_ac_f32(Fi, Fo, 4, 4, 6, 4, 0, st),
        "flow_expectation nbins 0": lambda: lib.mofa_flow_expectation_f16(X, Fo, 3, 63, 64, 0, 50.0, st),
        "flow_expectation nbins 129": lambda: lib.mofa_flow_expectation_f16(X, Fo, 3, 63, 264, 129, 50.0, st),
        "flow_expectation ld < 2 nbins": lambda: lib.mofa_flow_expectation_f16(X, Fo, 3, 63, 64, 33, 50.0, st),
        "mask_blend C % 8": lambda: lib.mofa_mask_blend_f16(X, Y, Fi, O, 16, 12, 4, 64, 64, 64, st),
        "mask_blend lda % 8": lambda: lib.mofa_mask_blend_f16(X, Y, Fi, O, 16, 8, 4, 60, 64, 64, st),
        "mask_blend ldo % 8": lambda: lib.mofa_mask_blend_f16(X, Y, Fi, O, 16, 8, 4, 64, 64, 60, st),
        "matting_blend C % 8": lambda: lib.mofa_matting_blend_f16(X, Y, Z, O, Fo, 16, 12, 64, 64, 8, 64, st),
        "matting_blend ldm % 8": lambda: lib.mofa_matting_blend_f16(X, Y, Z, O, Fo, 16, 8, 64, 60, 8, 64, st),
        "geglu Ch % 8": lambda: lib.mofa_geglu_f16(X, O, 16, 12, 64, 64, st),
        "geglu ldx % 8": lambda: lib.mofa_geglu_f16(X, O, 16, 8, 60, 64, st),
        "subsample C % 8": lambda: lib.mofa_subsample_tokens_f16(X, O, 1, 8, 8, 2, 12, 64, 64, st),
        "subsample ldy % 8": lambda: lib.mofa_subsample_tokens_f16(X, O, 1, 8, 8, 2, 8, 64, 60, st),
        "subsample H % s": lambda: lib.mofa_subsample_tokens_f16(X, O, 1, 6, 8, 4, 8, 64, 64, st),
        "subsample W % s": lambda: lib.mofa_subsample_tokens_f16(X, O, 1, 8, 6, 4, 8, 64, 64, st),
    }
    wrong = {name: rc for name, rc in ((name, call()) for name, call in calls.items()) if rc != EINVAL}
    torch.cuda.synchronize()
    assert not wrong, f"accepted (return code): {wrong}"
    for b, s in zip(bufs, snaps):
        assert oc.same_bits(b, s), "a rejected call wrote to a buffer"
    # ... and the ops wrapper raises before it allocates, by the same rule
    for kw in (dict(H=4, W=16, k=8, stride=8), dict(H=4, W=16, k=8, stride=2), dict(H=16, W=4, k=8, stride=8),
               dict(H=4, W=4, k=2, stride=1, pad=2), dict(H=8, W=16, k=3, stride=2, pad=2)):
        with pytest.raises(ValueError):
            ops.pool2d(x[:2 * kw["H"] * kw["W"]], 2, C=64, **kw)
