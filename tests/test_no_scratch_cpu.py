"""The hot kernels must not touch scratch memory: hipcc spills silently (hoisted division reciprocals, pointer-phi allocas,
accumulator tuples merged at a branch -- DESIGN.md section 3 lists the cases met), and a spill inside a K loop or an epilogue
costs more than most optimisations gain.  Cross-compiles the four hot sources for gfx950 with
-Rpass-analysis=kernel-resource-usage (no GPU needed) and checks every shipped kernel instantiation; the diagnostic K-loop
variants of tools/igemm8_probe.py (template parameter VAR != 0) are exempt."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SOURCES = ["attention.hip", "igemm.hip", "igemm8.hip", "igemm320.hip"]


def _usage(src):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(ROOT, "mofa_video_amd", "csrc", src), "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            rows[name] = {}
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            rows[name][m.group(1).split(" [")[0]] = int(m.group(2))
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_hot_kernels_use_no_scratch():
    with ThreadPoolExecutor(len(SOURCES)) as ex:
        results = list(ex.map(_usage, SOURCES))
    bad, seen = [], 0
    for src, rows in zip(SOURCES, results):
        assert rows, f"no kernel resource remarks for {src}"
        for name, r in rows.items():
            probe = re.search(r"igemm8_f16_kernelILi\d+ELi([1-9]\d*)E", name)     # VAR != 0: diagnostic build variants
            if probe:
                continue
            seen += 1
            if r.get("ScratchSize", 0) or r.get("VGPRs Spill", 0):
                bad.append((src, name, r))
    assert seen >= 37
    assert not bad, bad


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_long_temporal_attention_instantiations():
    """the three long temporal attention kernels include one body (csrc/attn_temporal_long_body.inc): each has exactly the eight instantiations
    (head dim, key tiles, waves per workgroup) the launcher dispatches to, none with scratch, a VGPR spill or an SGPR spill (the
    mask's 16 KT bit tests, hoisted out of the query loop, once took 42 SGPRs too many), and each at the occupancy [waves / SIMD]
    by (head dim, key tiles) that the three separate copies of the body had before they were merged"""
    occupancy = {(64, 1, 4): 4, (64, 2, 2): 3, (64, 3, 1): 2, (64, 4, 1): 2, (128, 1, 2): 2, (128, 2, 1): 2, (128, 3, 1): 1, (128, 4, 1): 1}
    usage = _usage("attention.hip")
    for kernel in ("attn_temporal_long_kernel", "attn_temporal_long_masked_kernel", "attn_temporal_long_local_kernel"):
        rows = {}
        for n, r in usage.items():
            m = re.match(r"_Z\d+" + kernel + r"ILi(\d+)ELi(\d+)ELi(\d+)EE", n)
            if m:
                inst = tuple(int(x) for x in m.groups())
                assert inst not in rows, (kernel, inst)
                rows[inst] = r
        assert set(rows) == set(occupancy), (kernel, sorted(rows))
        for inst, r in rows.items():
            assert r == {"ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0, "Occupancy": occupancy[inst]}, (kernel, inst, r)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_fused_level0_kernels_shipped_variants():
    """round 6: the fused feed-forward's three instantiations the transformer blocks launch (spatial ff; ff_in with the position vector
    and the LayerNorm output; temporal ff with the AlphaBlender residual) use no scratch at all; the transposed linear kernel's one
    shipped instantiation (LayerNorm + q | k | v) spills a few pointers at TILE boundaries (outside its chunk loop; <= 8 registers).
    The other instantiations exist for the C ABI's generality and the parity tests only."""
    with ThreadPoolExecutor(2) as ex:
        ff, ln = ex.map(_usage, ["ff320.hip", "lin320.hip"])
    shipped = {"ILb0ELb0ELb0E": 0, "ILb1ELb0ELb1E": 0, "ILb0ELb1ELb0E": 0}
    for tag, limit in shipped.items():
        rows = [r for n, r in ff.items() if "ff320_kernel" + tag in n]
        assert len(rows) == 1, (tag, list(ff))
        assert rows[0].get("VGPRs Spill", 0) <= limit and rows[0].get("ScratchSize", 0) == 0, (tag, rows[0])
    rows = [r for n, r in ln.items() if "lin320_kernelILb1ELb0ELb0E" in n]
    assert len(rows) == 1 and rows[0].get("VGPRs Spill", 0) <= 8, rows
