"""Every case of tests/image_cases.py through the C ABI on the GPU: csrc/frontend.hip (``mofa_filter1d_reflect_f32``,
``mofa_resize_bicubic_ac_f32``, ``mofa_patchify_f16``), ``mofa_resize_nearest_f32`` of csrc/elementwise.hip and csrc/output.hip
(``mofa_frames_postprocess_f32``, ``mofa_flow_to_image_u8``).  The ``ops`` wrappers allocate their own outputs, so the cases call
the entry points themselves: inputs are views into longer NaN buffers, outputs views into buffers of NaN (0xA5 bytes for uint8),
the flow workspace exactly ``mofa_flow_to_image_ws_bytes`` bytes inside a longer 0xA5 buffer.

Per case: everything outside the views and every read-only argument bit-unchanged, and the comparison the table states -- exact
bits, |out - fp64 reference| <= the derived bound per element, or for the flow picture every byte inside its derived range
(image_cases docstring; tests/test_image_cases_cpu.py proves the references, the exact families, the fragile-byte conditions
and that each check fails on a wrong kernel).  Each comparison prints ``IMG <case>: worst err / bound`` (pytest -s),
``test_worst_ratio_per_op`` the worst per op; for a 513 x 512 flow the figure is (share of bytes off the reference) / 1e-4.

``test_nearest_sweep_every_size_pair``: every (in, out) pair of 1..24 against F.interpolate, two pairs per launch.
``test_ops_wrapper_gives_the_same_bits``: one small case per op ties the ``ops`` wrapper to the same bits.
``test_argument_edges_rejected_without_launch``: every call returns MOFA_EINVAL and leaves its NaN-filled buffers bit-unchanged."""
import collections
import types

import pytest
import torch
import torch.nn.functional as F

import image_cases as ic
import op_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = collections.defaultdict(float)


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


def abi():
    """the entry points behind the calling convention of image_cases.impl"""
    from mofa_video_amd import lib as L
    lib = L.load()

    def filter1d_reflect(x, taps, axis, out):
        H, W = x.shape[-2:]
        L.check(lib.mofa_filter1d_reflect_f32(L.ptr(x), L.ptr(out), L.ptr(taps), x.numel() // (H * W), H, W, taps.numel(), axis,
                                              L.stream_ptr()), "mofa_filter1d_reflect_f32")

    def resize_bicubic_ac(x, out):
        H, W = x.shape[-2:]
        L.check(lib.mofa_resize_bicubic_ac_f32(L.ptr(x), L.ptr(out), x.numel() // (H * W), H, W, out.shape[-2], out.shape[-1],
                                               L.stream_ptr()), "mofa_resize_bicubic_ac_f32")

    def patchify(x, p, out):
        n, C, H, W = x.shape
        assert out.shape[0] == n * (H // p) * (W // p)
        L.check(lib.mofa_patchify_f16(L.ptr(x), L.ptr(out), n, C, H, W, p, out.shape[1], L.stream_ptr()), "mofa_patchify_f16")

    def resize_nearest_f32(x, out):
        n, H, W = x.shape
        L.check(lib.mofa_resize_nearest_f32(L.ptr(x), L.ptr(out), n, H, W, out.shape[1], out.shape[2], L.stream_ptr()),
                "mofa_resize_nearest_f32")

    def frames_postprocess(frames, mode, out):
        n, _, H, W = frames.shape
        L.check(lib.mofa_frames_postprocess_f32(L.ptr(frames), L.ptr(out), n, H, W, mode, L.stream_ptr()), "mofa_frames_postprocess_f32")

    def flow_to_image(flow, out, ws):
        H, W = flow.shape[:2]
        assert lib.mofa_flow_to_image_ws_bytes(H, W) == ic.WS_BYTES == ws.numel()
        L.check(lib.mofa_flow_to_image_u8(L.ptr(flow), L.ptr(out), H, W, L.ptr(ws), L.stream_ptr()), "mofa_flow_to_image_u8")
    return types.SimpleNamespace(**{k: v for k, v in locals().items() if callable(v) and k in ic.OPS})


@pytest.mark.parametrize("case", ic.CASES, ids=repr)
def test_hip_op_meets_its_reference(ops, case):
    r = ic.run_case(abi(), case, DEV)
    for name, p in r.placed.items():
        assert p.t.is_contiguous(), (case.id, name)
    worst, errs = ic.check_run(case, r)
    print(f"IMG {case.id}: worst err / bound {worst:.3f}" if worst else f"IMG {case.id}: bit-equal / exact")
    WORST[case.op] = max(WORST[case.op], worst)
    assert not errs, errs


def test_worst_ratio_per_op():
    for op in ic.OPS:
        print(f"IMG-WORST {op}: {WORST[op]:.3f}")


def test_nearest_sweep_every_size_pair(ops):
    """in and out over 1..24, one pair along H and another along W per launch: identities, upscales, in = 1, out = 1"""
    from mofa_video_amd import lib as L
    lib = L.load()
    bad = []
    for j, (H, W, h, w) in enumerate(ic.NEAREST_SWEEP):
        x = ic.nearest_data(2, H, W, 1000 + j)
        want = F.interpolate(x[None], size=(h, w), mode="nearest")[0].contiguous()
        src = torch.full((5 + x.numel() + 37,), ic.NAN, device=DEV)
        src[5:5 + x.numel()] = x.reshape(-1).to(DEV)
        dst = torch.full((8 + want.numel() + 40,), ic.NAN, device=DEV)
        snap = src.clone()
        xs, ys = src[5:5 + x.numel()], dst[8:8 + want.numel()]
        L.check(lib.mofa_resize_nearest_f32(L.ptr(xs), L.ptr(ys), 2, H, W, h, w, L.stream_ptr()), "mofa_resize_nearest_f32")
        got = dst.cpu()
        if not (oc.same_bits(got[8:8 + want.numel()].view(want.shape), want) and bool(torch.isnan(got[:8]).all())
                and bool(torch.isnan(got[8 + want.numel():]).all()) and oc.same_bits(src, snap)):
            bad.append((H, W, h, w))
    assert not bad, bad


@pytest.mark.parametrize("cid", ["filter1d_reflect/ragged-11x13-k5-axis1", "resize_bicubic_ac/11x13-to-7x19", "patchify/n2-C3-8x12-p2-ld16",
                                 "resize_nearest_f32/3x5-to-7x16", "frames_postprocess/mode0-n2-5x7", "frames_postprocess/mode1-n2-5x7",
                                 "frames_postprocess/mode2-n2-5x7", "flow_to_image/nan-23x31-max@710-s0"])
def test_ops_wrapper_gives_the_same_bits(ops, cid):
    case = ic.BY_ID[cid]
    r = ic.run_case(abi(), case, DEV)
    a = {k: (r.placed[k].before().contiguous() if k in r.placed else v) for k, v in r.kwargs.items()}
    out = r.placed["out"].t
    got = {"filter1d_reflect": lambda: ops.filter1d_reflect(a["x"], a["taps"], a["axis"]),
           "resize_bicubic_ac": lambda: ops.resize_bicubic_ac(a["x"], out.shape[-2], out.shape[-1]),
           "patchify": lambda: ops.patchify(a["x"], a["p"], out.shape[1]),
           "resize_nearest_f32": lambda: ops.resize_nearest_f32(a["x"], out.shape[1], out.shape[2]),
           "frames_postprocess": lambda: ops.frames_postprocess(a["frames"], a["mode"]),
           "flow_to_image": lambda: ops.flow_to_image(a["flow"])}[case.op]()
    torch.cuda.synchronize()
    assert got.shape == out.shape and got.dtype == out.dtype
    assert bool((ic._raw(got) == ic._raw(out)).all()), cid


def test_argument_edges_rejected_without_launch(ops):
    from mofa_video_amd import lib as L
    lib = L.load()
    st = L.stream_ptr()
    EINVAL = -22
    # sized for the largest output any reading of an argument list below could produce: nothing here can write out of bounds
    # even where a check is missing
    f = torch.full((65536,), ic.NAN, dtype=oc.F32, device=DEV)
    fo = torch.full((65536,), ic.NAN, dtype=oc.F32, device=DEV)
    t = torch.full((64,), ic.NAN, dtype=oc.F32, device=DEV)
    h = torch.full((65536,), ic.NAN, dtype=oc.F16, device=DEV)
    b = torch.full((65536,), ic.CANARY, dtype=torch.uint8, device=DEV)
    ws = torch.full((8192,), ic.CANARY, dtype=torch.uint8, device=DEV)
    bufs = (f, fo, t, h, b, ws)
    snaps = [x.clone() for x in bufs]
    Fi, Fo, T, Hh, B, WS = (L.ptr(x) for x in bufs)
    Fi, Fo = L.ptr(f[8192:]), L.ptr(fo[8192:])                       # (room in front as well: a reflected index may be negative)

    def filt(x=Fi, out=Fo, planes=6, H=5, W=9, k=3, axis=1):
        return lib.mofa_filter1d_reflect_f32(x, out, T, planes, H, W, k, axis, st)

    def patch(C=3, H=8, W=12, p=2, ld=16):
        return lib.mofa_patchify_f16(Fi, Hh, 2, C, H, W, p, ld, st)
    calls = {
        "filter1d x == out": lambda: filt(out=Fi), "filter1d k 0": lambda: filt(k=0), "filter1d axis 2": lambda: filt(axis=2),
        "filter1d axis -1": lambda: filt(axis=-1), "filter1d rear >= W": lambda: filt(W=4, k=9, axis=1),
        "filter1d rear == W, even k": lambda: filt(W=4, k=8, axis=1), "filter1d rear >= H": lambda: filt(H=3, k=7, axis=0),
        "filter1d rear == H, even k": lambda: filt(H=3, k=6, axis=0), "filter1d zero planes": lambda: filt(planes=0),
        "bicubic planes 0": lambda: lib.mofa_resize_bicubic_ac_f32(Fi, Fo, 0, 4, 6, 4, 6, st),
        "bicubic Hin 0": lambda: lib.mofa_resize_bicubic_ac_f32(Fi, Fo, 2, 0, 6, 4, 6, st),
        "bicubic Win 0": lambda: lib.mofa_resize_bicubic_ac_f32(Fi, Fo, 2, 4, 0, 4, 6, st),
        "bicubic Hout 0": lambda: lib.mofa_resize_bicubic_ac_f32(Fi, Fo, 2, 4, 6, 0, 6, st),
        "bicubic Wout 0": lambda: lib.mofa_resize_bicubic_ac_f32(Fi, Fo, 2, 4, 6, 4, 0, st),
        "patchify H % p": lambda: patch(H=9), "patchify W % p": lambda: patch(W=13), "patchify ld < C p p": lambda: patch(ld=11),
        "patchify p 0": lambda: patch(p=0), "patchify C 0": lambda: patch(C=0),
        "nearest n 0": lambda: lib.mofa_resize_nearest_f32(Fi, Fo, 0, 4, 6, 4, 6, st),
        "nearest H 0": lambda: lib.mofa_resize_nearest_f32(Fi, Fo, 2, 0, 6, 4, 6, st),
        "nearest W 0": lambda: lib.mofa_resize_nearest_f32(Fi, Fo, 2, 4, 0, 4, 6, st),
        "nearest h 0": lambda: lib.mofa_resize_nearest_f32(Fi, Fo, 2, 4, 6, 0, 6, st),
        "nearest w 0": lambda: lib.mofa_resize_nearest_f32(Fi, Fo, 2, 4, 6, 4, 0, st),
        "postprocess mode 3": lambda: lib.mofa_frames_postprocess_f32(Fi, Fo, 2, 5, 7, 3, st),
        "postprocess mode -1": lambda: lib.mofa_frames_postprocess_f32(Fi, Fo, 2, 5, 7, -1, st),
        "postprocess frames 0": lambda: lib.mofa_frames_postprocess_f32(Fi, B, 0, 5, 7, 2, st),
        "flow null workspace": lambda: lib.mofa_flow_to_image_u8(Fi, B, 7, 9, None, st),
        "flow H 0": lambda: lib.mofa_flow_to_image_u8(Fi, B, 0, 9, WS, st),
        "flow W 0": lambda: lib.mofa_flow_to_image_u8(Fi, B, 7, 0, WS, st),
    }
    wrong = {name: rc for name, rc in ((name, call()) for name, call in calls.items()) if rc != EINVAL}
    torch.cuda.synchronize()
    assert not wrong, f"accepted (return code): {wrong}"
    for x, s in zip(bufs, snaps):
        assert bool((ic._raw(x) == ic._raw(s)).all()), "a rejected call wrote to a buffer"
