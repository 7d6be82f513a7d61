"""Golden vectors for the oracle softsplat: the reference's OWN ``softsplat_out`` kernel body, compiled for the
host by oracle/build_ref.py (oracle/_ref, never committed), run on seeded inputs with non-finite and far out-of-range
flows; stores inputs + kernel outputs, so that tests/test_oracle_structure.py pins the oracle without the host build.
    python tests/golden/make_golden_softsplat.py      (needs the reference source for build_ref; the fixture is committed)"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import build_ref, softsplat_ref  # noqa: E402

build_ref.build(verbose=True)
g = torch.Generator().manual_seed(3)
cases = []
for (N, C, H, W, mag) in [(2, 5, 12, 20, 3.0), (1, 33, 9, 16, 0.4), (3, 2, 18, 32, 12.0)]:
    x = torch.randn(N, C, H, W, generator=g)
    f = torch.randn(N, 2, H, W, generator=g) * mag
    f[0, :, 0, 0] = float("nan")
    f[-1, 0, 1, 1] = float("-inf")
    f[0, :, 2, 2] = torch.tensor([3.0, -2.0])
    f[0, :, 3, 3] = torch.tensor([-1000.0, 4.5])
    cases.append(dict(x=x, flow=f,
                      out=softsplat_ref.softsplat_out_ref(x, f),         # the kernel on the features
                      avg=softsplat_ref.softsplat_avg_ref(x, f)))        # the reference's 'avg' wrapper around it
out = os.path.join(HERE, "reference_golden_softsplat.pt")
torch.save(dict(cases=cases, source="reference softsplat_out kernel body, host build (oracle/build_ref.py)"), out)
print(out, os.path.getsize(out), "bytes")
