"""Every case of tests/splat_cases.py through ``mofa_softsplat_avg_f16`` on the GPU (csrc/softsplat.hip: ss_count_kernel,
ss_scan_kernel, ss_fill_kernel, ss_sort_kernel, ss_gather_kernel).  The cases go through the C ABI, as ``out`` has a leading
dimension larger than C; ``test_ops_wrapper_gives_the_same_bits`` ties ``ops.softsplat_avg_tokens`` to it.

Per case: |out - fp64 reference| <= the derived bound per element (splat_cases docstring; tests/test_splat_cases_cpu.py proves
the reference, the exact families and that each check fails on a wrong kernel), targets without weight are the value 0, the exact
families equal the reference rounded once, the NaN guards around ``feat`` and ``out`` are intact bit for bit, the workspace --
exactly ``mofa_softsplat_ws_bytes`` bytes inside a longer buffer filled with 0xFF -- leaves the bytes behind it unchanged, a run
on a dirty workspace is bit-equal to one on a zeroed workspace, and every flow frame of a multi-frame case run alone gives the
bits of the joint run.  Each case prints its worst err / bound (pytest -s), ``test_worst_ratio_per_class`` the worst per class: a
record, the threshold is 1.0 by derivation.  fp16 outputs may sit near 1.0 by the final rounding alone.

``test_norm_sums_in_key_order``: ``ops.softsplat_norm_f32`` (the same CSR and sort, plain fp32 additions) is bit-equal to the
sequential fp32 sum in key order corner * HW + source on the segment-length cases."""
import collections

import pytest
import torch

import op_cases as oc
import splat_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = collections.defaultdict(float)
TAIL = 256                                                           # bytes behind the workspace that must stay as they were


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


def hip_splat(feat, flow, out, H, W):
    """the backend of splat_cases: mofa_softsplat_avg_f16 on views, twice -- on a workspace of 0xFF bytes and on a zeroed one"""
    from mofa_video_amd import lib as L
    lib = L.load()
    nfl, C = flow.shape[0], feat.shape[1]
    assert feat.stride(1) == 1 and out.stride(1) == 1 and flow.is_contiguous() and tuple(out.shape) == (nfl * H * W, C)
    nbytes = lib.mofa_softsplat_ws_bytes(nfl, H, W)
    assert nbytes == (11 * H * W + 1) * 4 * nfl + 64
    bad, first = [], None
    for fill in (0xFF, 0x00):
        ws = torch.full((nbytes + TAIL,), fill, dtype=torch.uint8, device=feat.device)
        ws[nbytes:] = 0xFF
        L.check(lib.mofa_softsplat_avg_f16(L.ptr(feat), L.ptr(flow), L.ptr(out), L.ptr(ws), nfl, H, W, C, feat.stride(0), out.stride(0),
                                           L.stream_ptr()), "mofa_softsplat_avg_f16")
        torch.cuda.synchronize()
        if not bool((ws[nbytes:] == 0xFF).all()):
            bad.append(f"bytes behind the workspace of {nbytes} bytes were written (workspace filled with {fill:#x})")
        if first is None:
            first = out.clone()
        elif not oc.same_bits(first, out):
            bad.append("the run on a dirty workspace gives other bits than the run on a zeroed one")
    return bad


@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_hip_warp_meets_its_reference(ops, case):
    r = sc.Run(case, hip_splat, DEV)
    worst, errs = sc.check_run(case, r, hip_splat, DEV)
    left = "; {} / {} elements left out of the exact check".format(*sc.LEFT_OUT[case.id]) if case.exact else ""
    print(f"SPLAT {case.id}: worst err / bound {worst:.3f}{left}")
    WORST[case.cls] = max(WORST[case.cls], worst)
    assert not errs, errs


def test_worst_ratio_per_class():
    for cls in sc.CLASSES:
        print(f"SPLAT-WORST {cls}: {WORST[cls]:.3f}")


def test_column_subset_is_bit_equal(ops):
    errs = sc.column_subset_errors(hip_splat, DEV)
    assert not errs, errs


@pytest.mark.parametrize("cid", ["gauss/7x9-C8-mag1.5-n3", "gauss/7x9-C512-mag1.5-n1", "gauss/7x9-C520-mag1.5-n1", "gauss/7x9-C1280-mag1.5-n1",
                                 "gauss/25x41-C1280-mag1.5-n1", "segments/12x20"])
def test_ops_wrapper_gives_the_same_bits(ops, cid):
    case = sc.BY_ID[cid]
    r = sc.Run(case, hip_splat, DEV)
    got = ops.softsplat_avg_tokens(r.feat.t, r.flow.t, case.H, case.W)
    torch.cuda.synchronize()
    assert not r.guard_errors()
    assert oc.same_bits(got.cpu(), r.result().contiguous())


@pytest.mark.parametrize("cid", sc.ORDER_CASES)
def test_norm_sums_in_key_order(ops, cid):
    case = sc.BY_ID[cid]
    flow = case.inputs()[1]
    got = ops.softsplat_norm_f32(flow.to(DEV)).cpu()
    want = sc.norm_emulation(flow, case.H, case.W)
    diff = oc.bits(got) != oc.bits(want)
    assert not bool(diff.any()), (cid, int(diff.sum()), torch.nonzero(diff)[0].tolist())
