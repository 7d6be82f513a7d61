"""GPU parity of the output stage through the C ABI: frames post-processing is bit exact against the oracle
(pure fp32 arithmetic + round-half-even); the flow colour image is compared with the fixture produced by the reference's
own flow_viz.py -- exact except where the device atan2f differs from numpy's by a few ulp at a byte boundary (tolerance, the
rule of tests/image_cases.py: <= 1e-4 of the bytes may differ, each by one count -- moving the fp32 angle by +-4 ulp changes
2.2e-5 of the bytes of a Gaussian flow, each by one; it was 0.2 % and two counts while the radius was computed with a fused
multiply-add).  tests/test_image_ops_gpu.py holds the edge, guard and NaN cases."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("shape", [(1, 3, 3, 16, 24), (1, 3, 8, 72, 128), (1, 3, 2, 576, 1024)])
def test_tensor2vid_bit_exact(shape):
    from mofa_video_amd.output import tensor2vid
    from oracle.output import tensor2vid as otv
    g = torch.Generator().manual_seed(11)
    video = torch.randn(*shape, generator=g) * 1.3
    video[0, 0, 0, 0, :8] = torch.tensor([-1.0, 1.0, 0.0, -5.0, 5.0, 2 * 0.5 / 255 - 1, 2 * 1.5 / 255 - 1, 2 * 2.5 / 255 - 1])
    dev = video.cuda()
    assert torch.equal(tensor2vid(dev, output_type="pt")[0].cpu(), otv(video, "pt")[0])
    assert np.array_equal(tensor2vid(dev, output_type="np")[0], otv(video, "np")[0])
    got, ref = tensor2vid(dev, output_type="pil")[0], otv(video, "pil")[0]
    assert len(got) == len(ref) == shape[2]
    for a, b in zip(got, ref):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_flow_to_image_vs_reference_fixture():
    from mofa_video_amd.output import flow_to_image
    G = torch.load(os.path.join(GD, "reference_golden_output.pt"), weights_only=False)
    for name, case in G.items():
        img = flow_to_image(case["flow"])
        ref = case["image"].numpy()
        assert img.dtype == np.uint8 and img.shape == ref.shape
        diff = np.abs(img.astype(int) - ref.astype(int))
        frac = (diff > 0).mean()
        print(f"{name}: {100 * frac:.3f} % of bytes differ, max |diff| {diff.max()}")
        assert frac <= 1e-4 and diff.max() <= 1, (name, frac, diff.max())
