"""The torch-CPU stand-ins of tests/emu_ops.py against the contract of the entry points they stand in for, without a GPU:
same signatures as ``mofa_video_amd.ops``, a case table (tests/op_cases.py) that reaches every parameter, and the table run
through the stand-ins under the guard layout -- ``out=`` honoured, nothing outside a written view touched, read-only arguments
left alone.  tests/test_op_contract_gpu.py runs the same table through the HIP side and compares the two."""
import ctypes
import inspect

import pytest
import torch

import emu_ops
import op_cases as oc
from mofa_video_amd import lib as L
from mofa_video_amd import ops

# parameters the table need not vary: both are documented in ops.igemm as not changing what the result means (which launches
# produce it / whether the epilogue also emits GroupNorm pair sums) and have GPU tests of their own
# (test_igemm_tiles_gpu.py::test_split_k_*, test_gn_stats_gpu.py)
COVERAGE_EXEMPT = {"stats", "split_k"}


def _norm_default(d):
    if d is None or (isinstance(d, ops.ConvGeom) and d.mode == L.MODE_PLAIN):
        return "plain geometry or None"
    return d


@pytest.mark.parametrize("name", emu_ops.NAMES)
def test_signature_equals_entry_point(name):
    """parameter names, order and defaults; ``geom``'s default compares as plain geometry on both sides"""
    real = [(n, _norm_default(p.default)) for n, p in inspect.signature(getattr(ops, name)).parameters.items()]
    emu = [(n, _norm_default(p.default)) for n, p in inspect.signature(getattr(emu_ops, name)).parameters.items()]
    assert emu == real, f"{name}: ops {inspect.signature(getattr(ops, name))} != emu_ops {inspect.signature(getattr(emu_ops, name))}"


def test_table_covers_every_name_and_every_parameter():
    assert COVERAGE_EXEMPT <= {"stats", "split_k"}
    assert {c.op for c in oc.CASES} == set(emu_ops.NAMES)
    missing = []
    for name in emu_ops.NAMES:
        fn = getattr(ops, name)
        hit = oc.nondefault_params(oc.cases_of(name), fn)
        for p in inspect.signature(fn).parameters:
            if p not in hit and p not in COVERAGE_EXEMPT:
                missing.append(f"{name}({p}=)")
        for c in oc.cases_of(name):
            assert c.tol in oc.TOL, c
    assert not missing, f"no case passes a non-default value for: {missing}"


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.id)
def test_stand_in_semantics(case):
    r = oc.run(emu_ops, case, "cpu")
    assert not r.guard_errors(), r.guard_errors()
    outs = r.outputs()
    assert outs, case.id
    for label, t, before in outs:
        if not torch.is_tensor(t):
            continue
        if before is None:
            assert torch.isfinite(t.float()).all(), f"{case.id}: non-finite {label}"
        else:       # a written argument: finite wherever it was written, and written at all
            changed = oc.bits(t) != oc.bits(before)
            assert changed.any(), f"{case.id}: {label} was not written"
            assert torch.isfinite(t.float()[changed]).all(), f"{case.id}: non-finite values written to {label}"
    oc.check_out_is_honoured(emu_ops, case, "cpu", r)


def test_every_optional_out_is_exercised():
    """every op whose entry point takes an optional ``out`` has a case that passes one (so the check above is not vacuous)"""
    for name in emu_ops.NAMES:
        if "out" in oc.defaults(getattr(ops, name)):
            assert any("out" in c.build() for c in oc.cases_of(name)), name
    assert any(len(c.build().get("ln_out") or ()) == 3 for c in oc.cases_of("ff320"))
    assert any(len(c.build().get("ln_out") or ()) == 2 for c in oc.cases_of("ff320"))


def test_igemm_residual_rounding_is_the_documented_one():
    """include/mofa_hip.h: with a residual, s_acc * (acc + bias) is rounded to fp16, the residuals are added in fp32, the sum
    is rounded once more.  On the exactly representable case the stand-in must give the literal formula's bits, and the case
    must tell that formula from a single rounding in a good share of its elements."""
    case = oc.BY_ID["igemm/exact-residual"]
    kw = case.build()
    x, r1, r2 = [kw[n].cut(kw[n].base).float() for n in ("x", "r1", "r2")]
    acc = x.double() @ kw["w"].double().T + kw["bias"].double()
    assert torch.equal(acc.float().double(), acc)                                  # exact in fp32: no summation order matters
    t = (kw["s_acc"] * acc).float()
    assert torch.equal(t.double(), kw["s_acc"] * acc)
    twice = (t.half().float() + kw["s1"] * r1 + kw["s2"] * r2).half()
    once = (t + kw["s1"] * r1 + kw["s2"] * r2).half()
    share = (twice != once).float().mean().item()
    assert share > 0.05, share
    got = oc.run(emu_ops, case, "cpu").ret
    assert torch.equal(got, twice), f"{(got != twice).sum().item()} elements differ from round16(round16(s_acc * acc) + residuals)"


def test_gn_nparts_equals_the_library():
    """the frame-sharded GroupNorm exchange of the gloo suite is sized by emu_ops.gn_nparts: it must be the library's own
    chunking (a host function: libmofa_hip.so loads without a GPU)"""
    from mofa_video_amd import _build
    _build.build()
    dll = ctypes.CDLL(L.LIB_PATH)
    dll.mofa_gn_nparts.restype = ctypes.c_int
    dll.mofa_gn_nparts.argtypes = [ctypes.c_int, ctypes.c_int]
    hws = list(range(1, 20001)) + list(range(576, 200001, 576))
    for C in (32, 320, 1280):
        bad = [(HW, emu_ops.gn_nparts(HW, C), dll.mofa_gn_nparts(HW, C)) for HW in hws
               if emu_ops.gn_nparts(HW, C) != dll.mofa_gn_nparts(HW, C)]
        assert not bad, f"C={C}: {len(bad)} values of HW disagree, first (HW, emu, lib) = {bad[0]}"


def test_gn_partial_entries_follow_the_chunk_order():
    """entry f * nparts + ch holds the sums of rows [ch * rpc, (ch + 1) * rpc) of frame f, rpc = ceil(HW / nparts): on frames
    that are constant per chunk every entry is told from every other by its mean"""
    case = oc.BY_ID["gn_partial_into/order"]
    r = oc.run(emu_ops, case, "cpu")
    part = r.placed["part_rows"].t.reshape(2, -1, 32, 2)
    nparts, HW = part.shape[1], r.kwargs["HW"]
    rpc = -(-HW // nparts)
    for f in range(2):
        for ch in range(nparts):
            rows = min(rpc, HW - ch * rpc)
            val = 0.25 * (ch + 1) + 8.0 * f
            assert torch.equal(part[f, ch, :, 0], torch.full((32,), val * rows * 2)), (f, ch)          # 64 / 32 = 2 channels per group
            assert torch.equal(part[f, ch, :, 1], torch.full((32,), val * val * rows * 2)), (f, ch)
