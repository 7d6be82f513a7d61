"""CPU checks of the fp32 gather forward of the warp (include/mofa_hip.h, mofa_softsplat_gather_f32): the entry point is declared,
exported and prototyped, every rule of its header is checked before any device call, `softsplat._splat` takes the path the switch
and torch's deterministic flag ask for (recording stubs in place of the ops, no device), and the new kernel cross-compiles for
gfx950 without scratch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from test_softsplat_grad_cpu import A, HIPCC, ROOT
from test_softsplat_grad_gpu import MODES

# strMode -> (prep, normalize, eps_mode) of the header's table
TABLE = {"sum": (0, False, 0), "sum-addeps": (0, False, 0), "avg": (1, True, 0), "avg-zeroeps": (0, True, 1), "avg-clipeps": (0, True, 2),
         "linear": (2, True, 0), "linear-addeps": (2, True, 0), "linear-zeroeps": (2, True, 1), "linear-clipeps": (2, True, 2),
         "soft": (3, True, 0), "soft-addeps": (3, True, 0), "soft-zeroeps": (3, True, 1), "soft-clipeps": (3, True, 2)}


def test_gather_symbol_is_declared_exported_and_prototyped():
    from mofa_video_amd import _build, lib
    _build.build()
    hdr = open(os.path.join(ROOT, "include", "mofa_hip.h")).read()
    dll = ctypes.CDLL(lib.LIB_PATH)
    s = "mofa_softsplat_gather_f32"
    assert re.search(r"\bint\s+" + s + r"\s*\(", hdr)
    assert hasattr(dll, s) and s in lib.PROTOTYPES
    stated = re.search(r"sizeof\(mofa_softsplat_gather_args\) = (\d+)", hdr)
    assert stated and ctypes.sizeof(lib.SoftsplatGatherArgs) == int(stated.group(1)) == 96
    assert lib.SoftsplatGatherArgs.N.offset == 48 and lib.SoftsplatGatherArgs.reserved.offset == 80


def _args(**kw):
    from mofa_video_amd import lib
    a = lib.SoftsplatGatherArgs(inp=A, flow=A, out=A, norm=A, ws=A, N=1, C=8, H=4, W=4, prep=1, normalize=1, eps_mode=0, slices=2)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_bad_arguments_are_refused_without_gpu():
    from mofa_video_amd import lib
    l = lib.load()
    assert l.mofa_softsplat_gather_f32(None, None) == -22
    bad = [dict(inp=None), dict(flow=None), dict(out=None), dict(ws=None),                        # each required pointer
           dict(prep=-1), dict(prep=4), dict(eps_mode=-1), dict(eps_mode=4), dict(slices=0), dict(slices=9), dict(slices=-2),
           dict(normalize=2), dict(normalize=-1),
           dict(metric=A), dict(prep=2), dict(prep=3),                                           # metric present xor prep >= 2
           dict(prep=0, normalize=0, metric=A),
           dict(normalize=0), dict(prep=2, metric=A, normalize=0), dict(prep=3, metric=A, normalize=0),   # prep >= 1 without normalize
           dict(prep=0, normalize=0),                                                            # (norm without a normaliser)
           dict(prep=0, C=1, slices=1),                                                          # 'avg-<suffix>' with one channel
           dict(prep=0, slices=8),                                                               # ... has C - 1 output channels
           dict(C=0), dict(C=-1), dict(N=0), dict(N=-1), dict(N=70000), dict(H=0), dict(W=-4), dict(H=1 << 15, W=1 << 14)]
    for b in bad:
        assert l.mofa_softsplat_gather_f32(ctypes.byref(_args(**b)), None) == -22, b
    for i in range(4):
        r = [0] * 4
        r[i] = 1
        assert l.mofa_softsplat_gather_f32(ctypes.byref(_args(reserved=(ctypes.c_int32 * 4)(*r))), None) == -22, i


def test_path_helper_over_every_mode_switch_and_flag():
    from mofa_video_amd.softsplat import _use_gather_f32
    assert len(MODES) == 13 and set(MODES) == set(TABLE)
    for mode in MODES:
        assert _use_gather_f32(mode, False, False) is False, mode
        assert _use_gather_f32(mode, True, False) is True, mode
        assert _use_gather_f32(mode, True, True) is True, mode
        assert _use_gather_f32(mode, False, True) is (mode != "avg"), mode


def test_slices_depend_on_the_shape_only():
    from mofa_video_amd import ops
    for N, Co, HW in ((1, 320, 9216), (1, 320, 2304), (1, 640, 576), (1, 1280, 144), (3, 2, 100), (2, 1, 1)):
        s = ops.softsplat_gather_slices(N, Co, HW)
        assert 1 <= s <= Co and s == ops.softsplat_gather_slices(N, Co, HW)


class _Recorder:
    """stands in for mofa_video_amd.ops: records (name, interesting arguments) and returns CPU tensors of the right shape"""

    def __init__(self):
        self.calls = []

    def softsplat_gather_f32(self, tenIn, tenFlow, tenMetric=None, prep=0, normalize=False, eps_mode=0, want_norm=False, slices=None):
        assert tenIn.dtype == tenFlow.dtype == torch.float32 and tenIn.is_contiguous() and tenFlow.is_contiguous()
        self.calls.append(("softsplat_gather_f32", prep, bool(normalize), eps_mode, tenMetric is not None, bool(want_norm), slices))
        N, C, H, W = tenIn.shape
        out = torch.zeros(N, C - (1 if normalize and prep == 0 else 0), H, W)
        return out, (torch.zeros(N, 1, H, W) if want_norm else None)

    def softsplat_scatter_f32(self, tenIn, tenFlow):
        self.calls.append(("softsplat_scatter_f32", tuple(tenIn.shape)))
        return torch.zeros_like(tenIn)

    def softsplat_weight_f32(self, tenIn, tenMetric, mode):
        self.calls.append(("softsplat_weight_f32", mode))
        N, C, H, W = tenIn.shape
        return torch.zeros(N, C + 1, H, W)

    def softsplat_normalize_f32(self, summed, eps_mode):
        self.calls.append(("softsplat_normalize_f32", eps_mode))
        return torch.zeros_like(summed[:, :-1])

    def nchw_to_tokens(self, x, ld=None, scale=1.0, out=None):
        self.calls.append(("nchw_to_tokens", tuple(x.shape), ld))
        return torch.zeros(x.shape[2] * x.shape[3], ld, dtype=torch.float16)

    def softsplat_avg_tokens(self, feat, flow, H, W):
        self.calls.append(("softsplat_avg_tokens", tuple(flow.shape)))
        return torch.zeros(flow.shape[0] * H * W, feat.shape[1], dtype=torch.float16)

    def tokens_to_nchw(self, x, n, Cc, H, W):
        self.calls.append(("tokens_to_nchw", n, Cc))
        return torch.zeros(n, Cc, H, W)


def _todays_calls(mode, N, C, H, W):
    """what `_splat` called before the fp32 gather existed"""
    base, Cp = mode.split("-")[0], (C + 7) // 8 * 8
    if base == "sum":
        return [("softsplat_scatter_f32", (N, C, H, W))]
    if mode == "avg":
        return [c for _ in range(N) for c in (("nchw_to_tokens", (1, C, H, W), Cp), ("softsplat_avg_tokens", (1, 2, H, W)),
                                               ("tokens_to_nchw", 1, C))]
    eps = TABLE[mode][2]
    if base == "avg":
        return [("softsplat_scatter_f32", (N, C, H, W)), ("softsplat_normalize_f32", eps)]
    return [("softsplat_weight_f32", 1 if base == "linear" else 2), ("softsplat_scatter_f32", (N, C + 1, H, W)),
            ("softsplat_normalize_f32", eps)]


def test_splat_dispatch_without_a_device():
    from mofa_video_amd import softsplat as S
    N, C, H, W = 2, 5, 6, 7
    x, f, m = torch.randn(N, C, H, W), torch.randn(N, 2, H, W), torch.rand(N, 1, H, W)
    saved = (S.ops, S.GATHER_F32, torch.are_deterministic_algorithms_enabled())
    try:
        for mode in MODES:
            metric = m if TABLE[mode][0] >= 2 else None
            for switch, flag in ((False, False), (True, False), (False, True), (True, True)):
                S.ops, S.GATHER_F32 = _Recorder(), switch
                torch.use_deterministic_algorithms(flag)
                for want_norm in (False, True):
                    S.ops.calls.clear()
                    out, norm = S._splat(x, f, metric, mode, want_norm=want_norm)
                    prep, normalize, eps = TABLE[mode]
                    if switch or (flag and mode != "avg"):        # exactly one call of the new op, nothing else
                        assert S.ops.calls == [("softsplat_gather_f32", prep, normalize, eps, prep >= 2, want_norm and normalize, None)], \
                            (mode, switch, flag, S.ops.calls)
                        assert (norm is not None) == (want_norm and normalize)
                    else:                                         # today's calls, the new op never reached
                        assert S.ops.calls == _todays_calls(mode, N, C, H, W), (mode, switch, flag, S.ops.calls)
                    assert tuple(out.shape) == (N, C - (1 if mode.startswith("avg-") else 0), H, W)
    finally:
        S.ops, S.GATHER_F32 = saved[0], saved[1]
        torch.use_deterministic_algorithms(saved[2])


def test_switch_is_off_by_default_and_follows_the_environment():
    code = "import mofa_video_amd.softsplat as S; print(S.GATHER_F32)"
    for val, want in ((None, "False"), ("1", "True"), ("0", "False")):
        env = {k: v for k, v in os.environ.items() if k != "MOFA_SOFTSPLAT_GATHER_F32"}
        if val is not None:
            env["MOFA_SOFTSPLAT_GATHER_F32"] = val
        import sys
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env)
        assert r.stdout.strip() == want, (val, r.stdout, r.stderr)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_gather_kernels_use_no_scratch():
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
    for k in ("ss_gather_f32_kernel", "ss_sort_wg_kernel"):
        hit = [r for n, r in rows.items() if re.search(r"\d" + k, n)]
        assert len(hit) == 1, (k, list(rows))
        assert hit[0].get("ScratchSize", -1) == 0 and hit[0].get("VGPRs Spill", -1) == 0, (k, hit[0])
