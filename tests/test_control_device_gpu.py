"""Control signals on the device (csrc/control.hip through ``ops.sparse_points`` / ``ops.flow_finish`` and
``control.controlnet_flow_from_tracks`` / ``controlnet_flow_from_landmarks``).  Every comparison is by equality of the bytes
with the host functions the device path replaces (control_cases.py): integer-valued sums below 2^24, copies, and products
rounded one by one leave no tolerance to give.  Every device buffer is a view into a NaN-filled guard buffer that must be
intact afterwards; outputs start as NaN, so the launch has to clear or write every element."""
import functools

import numpy as np
import pytest
import torch

from mofa_video_amd import control

import control_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sparse(mode, pos, val, H, W, off=4):
    from mofa_video_amd import ops
    n = val.shape[0]
    p = CC.Guarded(tuple(pos.shape), torch.int32, DEV, pos, off=off)
    v = CC.Guarded(tuple(val.shape), torch.float32, DEV, val, off=off)
    o = CC.Guarded((n, 4, H, W), torch.float32, DEV, off=off)
    assert bool(torch.isnan(o.t).all())
    got = ops.sparse_points(p.t, v.t, H, W, mode, out=o.t)
    assert got is o.t
    torch.cuda.synchronize()
    assert p.intact() and v.intact() and o.intact()
    assert torch.equal(p.t.cpu(), pos) and CC.same_bits(v.t, val)             # inputs are only read
    return got


@pytest.mark.parametrize("name", list(CC.ADD_CASES))
def test_add_case(name):
    pos, val, H, W, want, largest = CC.add_case(name)
    assert largest < CC.EXACT
    got = _sparse(CC.ADD, pos, val, H, W)
    assert CC.same_bits(got, want)
    assert CC.same_bits(_sparse(CC.ADD, pos, val, H, W, off=1), want)        # a launch off 16-byte alignment


@pytest.mark.parametrize("name", list(CC.LAST_CASES))
def test_last_case(name):
    pos, val, H, W, want = CC.last_case(name)
    assert CC.same_bits(_sparse(CC.LAST, pos, val, H, W), want)


def test_last_case_in_fp16():
    pos, val, H, W, want = CC.last_case("40x56-n4", torch.float16)
    assert CC.same_bits(_sparse(CC.LAST, pos, val, H, W), want)


def test_add_position_off_the_canvas_raises():
    from mofa_video_amd import lib, ops
    pos, val, H, W, _want, _ = CC.add_case("corners-32x48-n3")
    for bad in ((-1, 0), (H, 0), (0, W)):
        p = pos.clone()
        p[1] = torch.tensor(bad, dtype=torch.int32)
        with pytest.raises(ValueError):
            ops.sparse_points(p.to(DEV), val.to(DEV), H, W, lib.SPARSE_ADD)


def _finish(name):
    from mofa_video_amd import ops
    fin, fout, brush, H, W, want, off = CC.finish_case(name)
    ref = fin if fin is not None else fout
    n = ref.shape[0]
    bufs = [None if t is None else CC.Guarded(tuple(t.shape), t.dtype, DEV, t, off=off) for t in (fin, fout, brush)]
    o = CC.Guarded((n, 2, H, W), torch.float32, DEV, off=off)
    got = ops.flow_finish(*[None if b is None else b.t for b in bufs], H, W, out=o.t)
    assert got is o.t
    torch.cuda.synchronize()
    assert o.intact() and all(b is None or b.intact() for b in bufs)
    for b, t in zip(bufs, (fin, fout, brush)):
        if b is not None:
            assert torch.equal(b.t.cpu(), t) if t.dtype == torch.uint8 else CC.same_bits(b.t, t)
    return got, want


@pytest.mark.parametrize("name", list(CC.FINISH_CASES))
def test_finish_case(name):
    got, want = _finish(name)
    assert CC.same_bits(got, want)


def test_repeat_launches_are_bit_identical():
    pos, val, H, W, want, _ = CC.add_case("k130-32x48-n3")
    a, b = _sparse(CC.ADD, pos, val, H, W), _sparse(CC.ADD, pos, val, H, W)
    assert CC.same_bits(a, b) and CC.same_bits(a, want)
    pos, val, H, W, want = CC.last_case("40x56-n4")
    a, b = _sparse(CC.LAST, pos, val, H, W), _sparse(CC.LAST, pos, val, H, W)
    assert CC.same_bits(a, b) and CC.same_bits(a, want)
    (a, want), (b, _) = _finish("ratio_384"), _finish("ratio_384")
    assert CC.same_bits(a, b) and CC.same_bits(a, want)


def test_launch_clears_a_used_output():
    """a dense launch, then -- same output -- one without points: zeros, not the first result"""
    from mofa_video_amd import lib, ops
    pos, val, H, W, want, _ = CC.add_case("k130-32x48-n3")
    out = torch.full((3, 4, H, W), CC.NAN, device=DEV)
    ops.sparse_points(pos, val.to(DEV), H, W, lib.SPARSE_ADD, out=out)
    assert CC.same_bits(out, want) and float(out.abs().max()) > 0
    ops.sparse_points(pos[:0], val[:, :0].to(DEV), H, W, lib.SPARSE_ADD, out=out)
    assert float(out.abs().max()) == 0.0


def test_launches_on_a_side_stream():
    pos, val, H, W, want, _ = CC.add_case("k130-32x48-n3")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = _sparse(CC.ADD, pos, val, H, W)
        b, bw = _finish("ratio_384")
    s.synchronize()
    assert CC.same_bits(a, want) and CC.same_bits(b, bw)


# ---- end to end: tracks / landmarks -> controlnet_flow, against the host compositions ------------------------------------------
WORK = 64


@pytest.fixture(scope="module")
def cmp_model():
    """CMP with random weights, as tests/test_cmp_gpu.py builds it"""
    from mofa_video_amd import schema
    from mofa_video_amd.cmp import CMP_demo
    return CMP_demo(schema.synthetic_state_dict(schema.cmp_schema(), seed=21, gain=2.0), DEV)


TRACKS = [[(10, 12), (40, 30), (70, 80)], [(80, 20), (60, 50)], [(10, 12), (30, 5)], [(50, 90), (20, 70), (25, 40)]]      # at 96 x 96


def _brush(kind):
    b = np.zeros((WORK, WORK), dtype=np.uint8)
    if kind == "in_only":
        b[:] = 255
    elif kind == "both":
        b[:30, :30] = 255                                     # tracks 0 and 2 (one start pixel) inside
    elif kind == "values":
        b[:] = np.random.RandomState(3).choice([0, 1, 128, 254], size=(WORK, WORK)).astype(np.uint8)
        b[:30, :30] = 255
    return b                                                  # "out_only": nothing inside


@functools.lru_cache(maxsize=None)
def _first(H, W):
    return torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(9))


@pytest.mark.parametrize("H,W", [(64, 64), (96, 160)])
@pytest.mark.parametrize("kind", ["in_only", "out_only", "both", "values"])
def test_from_tracks_equals_from_drags(cmp_model, kind, H, W):
    T = 4
    tracks = [[(x * W / 96, y * H / 96) for x, y in tr] for tr in TRACKS]
    brush = _brush(kind)
    first = _first(H, W).to(DEV)
    d = control.tracking_points_to_drags(tracks, W, H, T, brush, work=WORK)
    assert d["in_flag"] == (kind != "out_only") and d["out_flag"] == (kind != "in_only")
    want = control.controlnet_flow_from_drags(cmp_model, first, d, H, W, motion_brush_mask=brush, work=WORK)
    got = control.controlnet_flow_from_tracks(cmp_model, first, tracks, H, W, T, motion_brush_mask=brush, work=WORK)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (1, T - 1, 2, H, W)
    assert CC.same_bits(got, want)
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize("H,W", [(64, 64), (96, 160)])
def test_from_landmarks_equals_sparse_flow_plus_get_flow(cmp_model, H, W):
    from mofa_video_amd.cmp import get_flow
    N = 4
    g = torch.Generator().manual_seed(H + W)
    first = torch.rand(3, H, W, generator=g)
    lm = torch.rand(N, 68, 2, generator=g) * torch.tensor([W + 6.0, H + 6.0]) - 3.0
    lm[0, 7], lm[0, 40] = lm[0, 2], lm[0, 2] + 0.01           # one pixel, three landmarks
    lw, ff = lm.unsqueeze(0), first.unsqueeze(0)
    if (H, W) != (WORK, WORK):                                # sample_inputs_face's working-size branch, at WORK instead of 384
        ff = torch.nn.functional.interpolate(ff, (WORK, WORK))
        lw = torch.zeros_like(lw)
        lw[:, :, :, 0] = lm[None, :, :, 0] / W * WORK
        lw[:, :, :, 1] = lm[None, :, :, 1] / H * WORK
    with CC.one_thread():
        sparse, mask = control.get_sparse_flow(lw, WORK, WORK, N)
    want = get_flow(cmp_model, ff.unsqueeze(0).repeat(1, N - 1, 1, 1, 1).to(DEV), sparse, mask, H, W)
    got = control.controlnet_flow_from_landmarks(cmp_model, first, lm, work=WORK)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (1, N - 1, 2, H, W)
    assert CC.same_bits(got, want)
    assert float(want.abs().max()) > 0
