"""Pose images on the device (csrc/landmarks.hip through ``landmarks.pose_images(..., device=...)`` and ``ops.pose_images``):
every comparison is ``torch.equal`` against the host path of mofa_video_amd/landmarks.py -- integer rasterisation and a
resize that reproduces numpy's roundings leave no tolerance to give.  Rasteriser cases (pose_cases.py) run at
height = width = draw_size = 320, where the resize is the identity; resize cases on one or two frames of plausible faces;
then batch, repeat, workspace-reuse and stream cases."""
import functools

import numpy as np
import pytest
import torch

from mofa_video_amd import landmarks as L

import pose_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _to_image(drawn):
    """the host's drawn canvases [N, 320, 320, 3] -> what pose_images returns at the drawing size (the resize is the identity
    there: test_pose_images_cpu.py)"""
    return (torch.from_numpy(np.array(drawn)).permute(0, 3, 1, 2).float() / 255.0).unsqueeze(0)


@functools.lru_cache(maxsize=None)
def _host(n, height, width, draw_size, seed=0):
    """the host oracle for n frames of plausible faces in a height x width clip; computed once per shape"""
    lm = PC.faces(n, seed) * np.array([width / PC.SIZE, height / PC.SIZE])
    lm.setflags(write=False)
    return lm, L.pose_images(lm, height, width, draw_size)


@pytest.mark.parametrize("name", list(PC.RASTER_CASES))
def test_rasteriser_case_bit_equal(name):
    lm, drawn = PC.raster_case(name)
    got = L.pose_images(lm, PC.SIZE, PC.SIZE, PC.SIZE, device=DEV)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (1, lm.shape[0], 3, PC.SIZE, PC.SIZE)
    assert torch.equal(got.cpu(), _to_image(drawn))
    if name == "off_canvas":
        assert float(got.abs().max()) == 0.0


def test_coordinate_beyond_the_limit_raises():
    lm = np.array(PC.raster_case("far_ends")[0])
    lm[0, 1, 0] = 32768.0
    with pytest.raises(ValueError):
        L.pose_images(lm, PC.SIZE, PC.SIZE, PC.SIZE, device=DEV)
    lm[0, 1, 0] = np.nan
    with pytest.raises(ValueError):
        L.pose_images(lm, PC.SIZE, PC.SIZE, PC.SIZE, device=DEV)


@pytest.mark.parametrize("n,height,width,draw_size", [(2, 576, 1024, 320), (1, 1024, 576, 320), (2, 256, 384, 320), (2, 136, 200, 320),
                                                      (2, 321, 319, 320), (2, 1, 1, 320), (2, 96, 160, 64)])
def test_resize_bit_equal(n, height, width, draw_size):
    lm, ref = _host(n, height, width, draw_size)
    got = L.pose_images(lm, height, width, draw_size, device=DEV)
    assert torch.equal(got.cpu(), ref)
    if height > 1:
        assert float(got.max()) > 0.5


def test_device_result_looks_like_the_hosts():
    lm, ref = _host(2, 256, 384, 320)
    want = ref.to(DEV)
    got = L.pose_images(lm, 256, 384, device=DEV)
    assert got.shape == want.shape and got.dtype == want.dtype and got.device == want.device
    # the host's result is a permuted view of its [N, H, W, 3] images; the device's is [1, N, 3, H, W] in that order in memory,
    # which is what the host's .contiguous() gives
    assert got.is_contiguous() and got.stride() == want.contiguous().stride()
    assert torch.equal(got, want)


def test_batch_of_33_frames():
    lm, ref = _host(33, 64, 96, 320, seed=5)
    assert torch.equal(L.pose_images(lm, 64, 96, device=DEV).cpu(), ref)


def test_same_call_twice_is_bit_identical():
    lm, ref = _host(2, 136, 200, 320)
    a = L.pose_images(lm, 136, 200, device=DEV)
    b = L.pose_images(lm, 136, 200, device=DEV)
    assert torch.equal(a, b) and torch.equal(a.cpu(), ref)


def test_launch_clears_its_own_canvas():
    """a dense frame, then -- same workspace, same output -- a frame with nothing on the canvas: zeros, not the first frame"""
    from mofa_video_amd import ops
    lm, drawn = PC.raster_case("tiny_box_overdraw")
    dense = torch.from_numpy(np.trunc(lm[:1]).astype(np.int32)).to(DEV)
    empty = dense + 1000
    ws = torch.full((PC.SIZE * PC.SIZE,), 63, dtype=torch.int32, device=DEV)      # dirty to begin with
    out = torch.empty((1, 3, PC.SIZE, PC.SIZE), dtype=torch.float32, device=DEV)
    assert ops.pose_images(dense, PC.SIZE, PC.SIZE, PC.SIZE, out=out, workspace=ws) is out
    assert torch.equal(out.cpu(), _to_image(drawn[:1])[0]) and float(out.max()) > 0
    ops.pose_images(empty, PC.SIZE, PC.SIZE, PC.SIZE, out=out, workspace=ws)
    assert float(out.abs().max()) == 0.0 and int(ws.max()) == 0


def test_launch_on_a_side_stream():
    lm, ref = _host(2, 136, 200, 320)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = L.pose_images(lm, 136, 200, device=DEV)
    s.synchronize()
    assert torch.equal(got.cpu(), ref)
