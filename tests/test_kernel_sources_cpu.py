"""The shipped HIP sources carry no build switches: experiment and timing-only variants are measured, logged under profiles/
and deleted, not left behind -D macros in the product kernels.  Two switches stay: MOFA_PROBE (the K-loop variants and the
cycle trace of tools/igemm8_probe.py, built only into tools/libmofa_hip_probe.so) and FF_DBG_VM0 (a correct-result ff320 build
with vmcnt(0) in place of the counted waits)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLOWED = {"MOFA_PROBE", "FF_DBG_VM0"}


def test_kernel_sources_have_no_build_switches():
    csrc = os.path.join(ROOT, "mofa_video_amd", "csrc")
    paths = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert len(paths) >= 15
    bad = []
    for path in paths:
        for no, line in enumerate(open(path), 1):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if not m:
                continue
            cond = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
            names = set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}
            if not names or names - ALLOWED:                      # (no name at all: `#if 0` / `#if 1`)
                bad.append(f"{os.path.basename(path)}:{no}: {line.strip()}")
    assert not bad, bad


def test_product_build_defines_no_macro():
    from mofa_video_amd import _build
    assert not [f for f in _build.FLAGS if f.startswith("-D")], _build.FLAGS
