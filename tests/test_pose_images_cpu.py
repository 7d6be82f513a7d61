"""Pose images on the device, the part that needs no GPU: the C-ABI symbol and its argument rules, the shared per-segment
rasteriser (csrc/landmarks_raster.h) executed ON THE HOST by a small stand-alone program over the case table of
pose_cases.py -- bit-equal to ``landmarks.draw_landmarks`` -- and the two facts the kernels rest on: a frame is the
per-pixel maximum of independently rasterised segments, and the resize at the drawing size is the identity."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from mofa_video_amd import landmarks as L

import pose_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_exported_and_validates_without_gpu():
    from mofa_video_amd import _build, lib
    _build.build()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mofa_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mofa_pose_images_f32\s*\(", hdr)
    assert "landmarks.hip" in _build.SOURCES
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "mofa_pose_images_f32")
    assert lib.PROTOTYPES["mofa_pose_images_f32"] == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    f = lib.load().mofa_pose_images_f32
    A = 0x10000                                              # 16-byte aligned, never touched: validation fails first
    assert f(A, A, A, 1, 8, 8, 4097, None) == -22            # draw_size > 4096
    assert f(A, A, A, 0, 8, 8, 320, None) == -22             # N = 0
    assert f(A, A, None, 1, 8, 8, 320, None) == -22          # NULL workspace
    for bad in ((None, A, A, 1, 8, 8, 320), (A, None, A, 1, 8, 8, 320), (A, A, A, -1, 8, 8, 320), (A, A, A, 1, 0, 8, 320),
                (A, A, A, 1, 8, 0, 320), (A, A, A, 1, 8, 8, 0), (A, A, A + 4, 1, 8, 8, 320)):
        assert f(*bad, None) == -22, bad


@pytest.fixture(scope="module")
def raster_program(tmp_path_factory):
    """tests/pose_raster_main.hip built with hipcc: the host side of the same header the kernel includes"""
    from mofa_video_amd import _build
    exe = str(tmp_path_factory.mktemp("pose_raster") / "pose_raster_main")
    subprocess.run([_build._hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "pose_raster_main.hip"),
                    "-o", exe], check=True)
    return exe


def _run_raster(exe, pts, tmp_path):
    n = pts.shape[0]
    src, dst = str(tmp_path / "pts.bin"), str(tmp_path / "canvas.bin")
    with open(src, "wb") as f:
        f.write(np.array([n, PC.SIZE, PC.SIZE], dtype="<i4").tobytes() + pts.astype("<i4").tobytes())
    subprocess.run([exe, src, dst], check=True)
    return np.fromfile(dst, dtype="<i4").reshape(n, PC.SIZE, PC.SIZE)


@pytest.mark.parametrize("name", list(PC.RASTER_CASES))
def test_shared_rasteriser_on_the_host_equals_draw_landmarks(name, raster_program, tmp_path):
    lm, drawn = PC.raster_case(name)
    pts = np.trunc(PC.scaled(lm, PC.SIZE, PC.SIZE, PC.SIZE))  # draw_landmarks' int(): toward zero
    canvas = _run_raster(raster_program, pts, tmp_path)
    assert canvas.min() >= 0 and canvas.max() <= len(PC.SEGMENTS)
    assert np.array_equal(PC.COLOURS[canvas], drawn)
    # (the radius-1 plus around (-1, -1) or (320, 320) has no pixel on the canvas)
    assert (canvas.max() == 0) == (name in ("off_canvas", "circles_only_off_canvas"))


@pytest.mark.parametrize("name", ["faces", "clipped_all_borders", "tiny_box_overdraw"])
def test_frame_is_the_maximum_of_independent_segments(name):
    """each segment rasterised alone on a blank canvas, combined by the highest segment number, then coloured = sequential
    painting: what lets the kernel give every segment its own lane"""
    lm, drawn = PC.raster_case(name)
    kp = PC.scaled(lm, PC.SIZE, PC.SIZE, PC.SIZE)[0]
    index = np.zeros((PC.SIZE, PC.SIZE), dtype=np.int64)
    for s, (a, b, _part) in enumerate(PC.SEGMENTS):
        one = L.line(np.zeros((PC.SIZE, PC.SIZE, 1)), (int(kp[a][0]), int(kp[a][1])), (int(kp[b][0]), int(kp[b][1])), (1,), 2)
        index = np.maximum(index, (s + 1) * (one[:, :, 0] != 0))
    assert np.array_equal(PC.COLOURS[index], drawn[0])


def test_resize_at_the_drawing_size_is_the_identity():
    _lm, drawn = PC.raster_case("faces")
    assert np.array_equal(L.resize_linear(drawn[0], PC.SIZE, PC.SIZE), drawn[0])


@pytest.mark.parametrize("height,width,draw_size", [(320, 320, 320), (48, 72, 64)])
def test_host_path_is_draw_plus_resize(height, width, draw_size):
    lm = PC.faces(2, seed=3) * np.array([width / 320, height / 320])
    got = L.pose_images(lm, height, width, draw_size)
    again = L.pose_images(lm, height, width, draw_size, device=None)
    kp = PC.scaled(lm, height, width, draw_size)
    imgs = np.stack([L.resize_linear(L.draw_landmarks(f, draw_size, draw_size), width, height) for f in kp])
    ref = (torch.from_numpy(imgs).permute(0, 3, 1, 2).float() / 255.0).unsqueeze(0)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 2, 3, height, width) and got.device.type == "cpu"
    assert got.numpy().tobytes() == ref.numpy().tobytes() == again.numpy().tobytes()
    assert float(got.max()) > 0.5


def test_device_path_rejects_what_the_rasteriser_does_not_take():
    """checked on the host before anything is uploaded"""
    lm = PC.faces(1)
    for bad in (np.nan, np.inf, 32768.0, -32768.0):
        x = lm.copy()
        x[0, 5, 1] = bad
        with pytest.raises(ValueError):
            L.pose_images(x, PC.SIZE, PC.SIZE, device="cuda")
    with pytest.raises(ValueError):
        x = lm.copy()
        x[0, 5, 1] = np.nan
        L.pose_images(x, PC.SIZE, PC.SIZE)
