"""Every case of tests/norm_cases.py through ``mofa_video_amd.ops`` on the GPU: ``layer_norm`` (the four instantiations of
csrc/norm.hip's layernorm_kernel, plain and with a row vector, at both edges of every dispatch branch, at the row edges of a pass
and with ``nrr`` >= 2 passes per workgroup) and ``group_norm`` (gn_partial + gn_apply at every class of the row walk and of the
partial sums' thread layout, one workgroup per frame, a ragged last chunk, and gn_finalize + affine_act past
``ops.GN_FUSED_MAX_ENTRIES``).

Per case: guards intact (NaN rows and columns around every view, compared as bits), read-only arguments bit-unchanged, outputs
finite, ``out=`` (NaN-filled before the call) bit-equal to the fresh-output call on the cases that are not ``big``, every element
within its derived bound of the fp64 reference, and equal to the reference rounded once wherever no rounding tie lies within the
fp32 part of the bound (norm_cases docstring; tests/test_norm_cases_cpu.py proves the references, the table's shape classes and
that each check fails on a wrong kernel).  Each case prints its worst err / bound and the share of elements that are not the
reference rounded once (pytest -s), ``test_worst_ratio_per_op`` the worst per op.  fp16 outputs may sit near 1.0 by the final
rounding alone: half an fp16 ulp is u16 |ref| just above a power of two.

``test_argument_edges_rejected_without_launch`` goes through the C ABI: every call returns MOFA_EINVAL and leaves its NaN-filled
buffers bit-unchanged.  C = 0 and C = -32 are the values six GroupNorm entry points used to accept (``C % 32 == 0`` holds for
both): gn_apply_kernel then divided by C / 8 = 0."""
import collections

import pytest
import torch

import aux_cases as ac
import norm_cases as nc
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


@pytest.mark.parametrize("case", nc.CASES, ids=repr)
def test_hip_norm_meets_its_reference(ops, case):
    r = oc.run(ops, case, DEV)
    worst, errs = nc.check_run(case, r)
    off = "; ".join(f"{n} / {m} elements off the reference rounded once" for k, (n, m) in ac.OFF_ROUNDING.items() if k.startswith(case.id + " "))
    print(f"NORM {case.id}: worst err / bound {worst:.3f} ({off})")
    WORST[case.op] = max(WORST[case.op], worst)
    assert not errs, errs
    if not case.big:                                                 # (the small cases of the width prove out= against fresh)
        oc.check_out_is_honoured(ops, case, DEV, r)


def test_worst_ratio_per_op():
    for op in nc.OPS:
        print(f"NORM-WORST {op}: {WORST[op]:.3f}")


def test_argument_edges_rejected_without_launch(ops):
    from mofa_video_amd import lib as L
    lib = L.load()
    st = L.stream_ptr()
    bufs = nc.edge_buffers(DEV)
    snaps = [t.clone() for t in bufs]
    calls = nc.edge_calls(lib, [L.ptr(t) for t in bufs], st)
    wrong = {name: rc for name, rc in ((name, call()) for name, call in calls.items()) if rc != nc.MOFA_EINVAL}
    torch.cuda.synchronize()
    assert not wrong, f"accepted (return code): {wrong}"
    for t, s in zip(bufs, snaps):
        assert oc.same_bits(t, s), "a rejected call wrote to a buffer"
