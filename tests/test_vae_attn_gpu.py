"""Every case of tests/vae_attn_cases.py on the GPU: ``softmax_rows_`` (one to 4.5 passes of 2048 columns, the exact constant and
one-hot rows, Gaussian and tail rows against the per-element bound, subnormal results included), ``transpose_v`` (every S, column
block and frame count, bit-equal) through ``mofa_video_amd.ops``, and the composed ``vae.mid_attention_core`` on its uniform,
one-hot and Gaussian families.

Per case: guards intact (compared as bits), read-only arguments bit-unchanged, and the comparison the table states -- exact bits, or
|out - fp64 reference| <= the derived bound per element (vae_attn_cases docstring; tests/test_vae_attn_cases_cpu.py proves the
references, the exact families and that each check fails on a wrong kernel).  Each comparison prints its worst err / bound and the
share of elements off the fp64 reference rounded once (pytest -s), ``test_worst_ratio_per_op`` the worst per op and family.

``test_argument_edges_rejected_without_launch`` goes through the C ABI: every call returns MOFA_EINVAL and leaves its NaN-filled
buffers bit-unchanged."""
import collections

import pytest
import torch

import aux_cases as ac
import op_cases as oc
import vae_attn_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = collections.defaultdict(float)
OFF = collections.defaultdict(lambda: [0, 0])


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.mark.parametrize("case", vc.CASES, ids=repr)
def test_hip_op_meets_its_reference(ops, case):
    r = oc.run(vc.core_module() if case.op == "mid_attention_core" else ops, case, DEV)
    worst, errs = ac.check_run(case, r)
    mine = [(n, m) for k, (n, m) in ac.OFF_ROUNDING.items() if k.startswith(case.id + " ")]
    off = "; ".join(f"{n} / {m} elements off the reference rounded once" for n, m in mine)
    print(f"VAE-ATTN {case.id}: worst err / bound {worst:.3f} ({off})" if worst else f"VAE-ATTN {case.id}: bit-equal / exact")
    key = f"{case.op}/{case.meta['family']}" if "family" in case.meta else case.op
    WORST[key] = max(WORST[key], worst)
    for n, m in mine:
        OFF[key][0] += n
        OFF[key][1] += m
    assert not errs, errs


def test_worst_ratio_per_op():
    for key in WORST:
        n, m = OFF[key]
        print(f"VAE-ATTN-WORST {key}: {WORST[key]:.3f}" + (f", OFF_ROUNDING {n} / {m} = {n / m:.4f}" if m else ""))


def test_argument_edges_rejected_without_launch(ops):
    from mofa_video_amd import lib as L
    lib = L.load()
    st = L.stream_ptr()
    EINVAL = -22
    # sized for the largest output either reading of any argument list below could produce: 65536 frames (or column blocks) of
    # 8 keys and 64 channels are 33.5 M halves on either side of transpose_v
    big = 65536 * 8 * 64
    x = torch.full((big,), ac.NAN, dtype=oc.F16, device=DEV)
    y = torch.full((big,), ac.NAN, dtype=oc.F16, device=DEV)
    snaps = [x.clone(), y.clone()]
    X, Y = L.ptr(x), L.ptr(y)

    def softmax(p=X, rows=4, cols=64, ld=72):
        return lib.mofa_softmax_rows_f16(p, rows, cols, ld, st)

    def tv(v=X, vt=Y, nframes=2, ncb=1, S=8, ldv=64):
        return lib.mofa_transpose_v_f16(v, vt, nframes, ncb, S, ldv, st)
    calls = {
        "softmax NULL": lambda: softmax(p=None), "softmax rows 0": lambda: softmax(rows=0), "softmax rows -1": lambda: softmax(rows=-1),
        "softmax cols 0": lambda: softmax(cols=0), "softmax cols % 8": lambda: softmax(cols=60), "softmax ld % 8": lambda: softmax(ld=68),
        "softmax ld < cols": lambda: softmax(ld=56),
        "transpose_v NULL v": lambda: tv(v=None), "transpose_v NULL vt": lambda: tv(vt=None), "transpose_v nframes 0": lambda: tv(nframes=0),
        "transpose_v ncb 0": lambda: tv(ncb=0), "transpose_v S 0": lambda: tv(S=0), "transpose_v S % 8": lambda: tv(S=12),
        "transpose_v S -8": lambda: tv(S=-8), "transpose_v ldv % 8": lambda: tv(ldv=68), "transpose_v ldv < ncb * 64": lambda: tv(ncb=2, ldv=64),
        "transpose_v nframes 65536": lambda: tv(nframes=65536), "transpose_v ncb 65536": lambda: tv(nframes=1, ncb=65536, ldv=65536 * 64),
    }
    wrong = {name: rc for name, rc in ((name, call()) for name, call in calls.items()) if rc != EINVAL}
    torch.cuda.synchronize()
    assert not wrong, f"accepted (return code): {wrong}"
    for b, s in zip((x, y), snaps):
        assert oc.same_bits(b, s), "a rejected call wrote to a buffer"
