"""The per-frame bounds of helpers.check_frames against the tensor-wide rel-L2 they sit next to: on a synthetic latent clip shaped like
the sharded runs' output ([1, 25, 4, 72, 128]), two defects a sharding bug leaves behind -- a small patch of large errors in one
frame, and one frame replaced by its neighbour (a wrong halo frame) -- pass the suite's tensor bar of 2e-2 and fail the per-frame
bounds, which name the planted frame."""
import re

import pytest
import torch

from helpers import check_frames, frame_errors, rel_l2

T, SHAPE = 25, (1, 25, 4, 72, 128)
TOL = 2e-2
ABS = 0.05                 # (above every per-frame max-abs bar of the GPU loop tests)


def _clip():
    """reference clip: a common image plus a linear drift over the frames (neighbouring frames differ by ~5 %, like the latents
    of a video), and a product with a small spread error of ~1e-4 relative"""
    g = torch.Generator().manual_seed(3)
    base = torch.randn(1, 1, 4, 72, 128, generator=g)
    drift = torch.randn(1, 1, 4, 72, 128, generator=g)
    f = torch.arange(T, dtype=torch.float32).view(1, T, 1, 1, 1) - T // 2
    ref = base + 0.05 * f * drift
    out = ref + 1e-4 * torch.randn(SHAPE, generator=g)
    return out, ref


def test_clean_clip_passes():
    out, ref = _clip()
    e = check_frames(out, ref, TOL, ABS, what="clean")
    assert max(e.rel) < 1e-3 and max(e.maxabs) < 1e-3 and abs(e.tensor - rel_l2(out, ref)) < 1e-6


def test_sparse_large_errors_in_one_frame():
    """0.1 x max|ref| on 0.1 % of the elements of frame 17: tensor rel-L2 ~3e-3"""
    out, ref = _clip()
    k = 17
    fr = out[0, k].reshape(-1)
    n = fr.numel() // 1000
    idx = torch.randperm(fr.numel(), generator=torch.Generator().manual_seed(5))[:n]
    fr[idx] += 0.1 * ref.abs().max()
    assert rel_l2(out, ref) < TOL
    e = frame_errors(out, ref)
    assert e.worst_abs == k and e.worst_elem[1] == k
    with pytest.raises(AssertionError, match=rf"frame {k} rel-L2") as info:
        check_frames(out, ref, TOL, ABS, what="sparse")
    assert re.findall(r"frame (\d+) rel-L2", str(info.value)) == [str(k)]


@pytest.mark.parametrize("k", [6, 7, 24])
def test_frame_replaced_by_its_neighbour(k):
    """frame k holds frame k - 1 (a halo frame taken from the wrong side of a shard boundary: 7 is the first frame of the second
    shard of 25 over 4, 6 the last of the first, 24 the last of the clip)"""
    out, ref = _clip()
    out[:, k] = out[:, k - 1]
    assert rel_l2(out, ref) < TOL
    with pytest.raises(AssertionError, match=rf"frame {k} rel-L2") as info:
        check_frames(out, ref, TOL, ABS, what="halo")
    assert re.findall(r"frame (\d+) rel-L2", str(info.value)) == [str(k)]


def test_shard_slice_frame_numbers_and_nan():
    """f0 numbers the frames of a shard slice as clip frames; a NaN fails its frame"""
    out, ref = _clip()
    out[0, 9, 1, 2, 3] = float("nan")
    e = frame_errors(out[:, 7:13], ref[:, 7:13], f0=7)
    assert e.worst_abs == 9 and e.worst_elem == (0, 9, 1, 2, 3)
    with pytest.raises(AssertionError, match=r"frame 9 rel-L2"):
        check_frames(out[:, 7:13], ref[:, 7:13], TOL, ABS, f0=7, what="nan")
