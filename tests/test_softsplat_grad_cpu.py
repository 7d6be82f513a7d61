"""CPU checks of the warp's backward (include/mofa_hip.h, mofa_softsplat_norm_f32 / _grad_prologue_f32 / _grad_f32): the
autograd surface exists under the reference's name, the new entry points are exported and prototyped, bad arguments are refused
before any device call, and the new kernels cross-compile for gfx950 without scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ["mofa_softsplat_norm_f32", "mofa_softsplat_grad_prologue_f32", "mofa_softsplat_grad_f32"]
A = 0x10000                                  # a never-dereferenced address: validation fails first


def test_softsplat_func_is_an_autograd_function():
    from mofa_video_amd import softsplat as S
    assert issubclass(S.softsplat_func, torch.autograd.Function)
    assert issubclass(S._softsplat_normalized, torch.autograd.Function)


def test_new_symbols_are_declared_exported_and_prototyped():
    from mofa_video_amd import _build, lib
    _build.build()
    hdr = open(os.path.join(ROOT, "include", "mofa_hip.h")).read()
    dll = ctypes.CDLL(lib.LIB_PATH)
    for s in NEW:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert hasattr(dll, s) and s in lib.PROTOTYPES, s
    assert ctypes.sizeof(lib.SoftsplatGradArgs) == 120 and lib.SoftsplatGradArgs.N.offset == 80


def _grad_args(**kw):
    from mofa_video_amd import lib
    a = lib.SoftsplatGradArgs(grad=A, flow=A, inp=A, inv=A, glast=A, grad_in=A, grad_flow=A, partial=A, N=1, C=8, H=4, W=4,
                              prep=1, slices=2)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_bad_arguments_are_refused_without_gpu():
    from mofa_video_amd import lib
    l = lib.load()
    for eps in (-1, 4):
        assert l.mofa_softsplat_grad_prologue_f32(A, A, A, A, A, 1, 8, 4, 4, eps, None) == -22, eps
    for C in (0, -3):
        assert l.mofa_softsplat_grad_prologue_f32(A, A, A, A, A, 1, C, 4, 4, 0, None) == -22, C
    assert l.mofa_softsplat_grad_prologue_f32(A, A, A, A, A, 1, 8, 1 << 15, 1 << 14, 0, None) == -22   # H * W >= 2^29
    assert l.mofa_softsplat_norm_f32(A, A, A, 0, 4, 4, None) == -22
    assert l.mofa_softsplat_norm_f32(A, A, None, 1, 4, 4, None) == -22
    bad = [dict(C=0), dict(C=-1), dict(prep=4), dict(prep=-1), dict(slices=0), dict(slices=10), dict(N=0), dict(N=70000),
           dict(grad=None), dict(flow=None), dict(inv=None), dict(glast=None),                     # prep 1 needs the prologue
           dict(prep=2), dict(grad_metric=A), dict(partial=None), dict(inp=None),
           dict(grad_in=None, grad_flow=None), dict(H=1 << 15, W=1 << 14),
           dict(prep=0, C=1)]                                                                      # 'avg-<suffix>' with 1 channel
    for b in bad:
        assert l.mofa_softsplat_grad_f32(ctypes.byref(_grad_args(**b)), None) == -22, b
    for i in range(4):
        r = [0] * 4
        r[i] = 1
        assert l.mofa_softsplat_grad_f32(ctypes.byref(_grad_args(reserved=(ctypes.c_int32 * 4)(*r))), None) == -22, i


def test_channel_slices_depend_on_the_shape_only():
    from mofa_video_amd import ops
    for N, Cs, HW in ((1, 321, 9216), (1, 321, 2304), (1, 641, 576), (1, 1281, 144), (3, 2, 100), (2, 1, 1)):
        s = ops.softsplat_grad_slices(N, Cs, HW)
        assert 1 <= s <= Cs and s == ops.softsplat_grad_slices(N, Cs, HW)
    assert ops.softsplat_grad_slices(1, 321, 9216) > 1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_backward_kernels_use_no_scratch():
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           os.path.join(ROOT, "mofa_video_amd", "csrc", "softsplat.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            rows[name] = {}
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            rows[name][m.group(1).split(" [")[0]] = int(m.group(2))
    kernels = ["ss_norm_kernel", "ss_grad_prologue_kernel", "ss_grad_kernel", "ss_grad_reduce_kernel"]
    for k in kernels:
        hit = [r for n, r in rows.items() if re.search(r"\d" + k, n)]
        assert len(hit) == 1, (k, list(rows))
        assert hit[0].get("ScratchSize", -1) == 0 and hit[0].get("VGPRs Spill", -1) == 0, (k, hit[0])
