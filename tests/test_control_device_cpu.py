"""Control signals on the device, the part that needs no GPU: the two C-ABI symbols and their argument rules, the host halves
(``control.track_points`` against ``tracking_points_to_drags``, ``control.sample_inputs_face`` against a fixture produced by
the reference's own function), and the shared decision logic of the kernels (csrc/control_points.h) executed ON THE HOST by
tests/control_points_main.hip over every case of control_cases.py, equal to the host functions the device path replaces.
Two deliberately wrong variants of that program (first writer wins; rows and columns exchanged) are shown to fail."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from mofa_video_amd import control

import control_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I = ctypes.c_void_p, ctypes.c_int


def test_entry_points_declared_exported_and_validate_without_gpu():
    from mofa_video_amd import _build, lib
    _build.build()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mofa_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mofa_sparse_points_f32\s*\(", hdr) and re.search(r"\bint\s+mofa_flow_finish_f32\s*\(", hdr)
    assert re.search(r"MOFA_SPARSE_ADD\s*=\s*0\s*,\s*MOFA_SPARSE_LAST\s*=\s*1", hdr)
    assert (lib.SPARSE_ADD, lib.SPARSE_LAST) == (0, 1) == (CC.ADD, CC.LAST)
    assert "control.hip" in _build.SOURCES and any(h.endswith("control_points.h") for h in _build.HEADERS)
    dll = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(dll, "mofa_sparse_points_f32") and hasattr(dll, "mofa_flow_finish_f32")
    assert lib.PROTOTYPES["mofa_sparse_points_f32"] == [_P, _P, _I, _I, _I, _I, _I, _P, _P]
    assert lib.PROTOTYPES["mofa_flow_finish_f32"] == [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]
    sp, fin = lib.load().mofa_sparse_points_f32, lib.load().mofa_flow_finish_f32
    A = 0x10000                                              # never touched: validation fails first
    for bad in ((A, A, 4, 1, 8, 8, 0, None),                 # NULL out
                (A, A, -1, 1, 8, 8, 0, A), (A, A, 4, 0, 8, 8, 0, A), (A, A, 4, -1, 8, 8, 0, A), (A, A, 4, 1, 0, 8, 0, A),
                (A, A, 4, 1, 8, -8, 0, A),                   # negative / zero sizes
                (A, A, 4097, 1, 8, 8, 0, A), (A, A, 4097, 1, 8, 8, 1, A),      # K > 4096
                (A, A, 4, 1, 8, 8, 2, A), (A, A, 4, 1, 8, 8, -1, A),           # unknown mode
                (None, A, 4, 1, 8, 8, 0, A), (A, None, 4, 1, 8, 8, 1, A),      # K > 0 without points
                (A, A, 4, 65536, 8, 8, 0, A), (A, A, 4, 1, 65536, 65536, 0, A)):
        assert sp(*bad, None) == -22, bad
    for bad in ((A, A, A, 1, 8, 8, 8, 8, None), (A, A, A, 0, 8, 8, 8, 8, A), (A, A, A, -1, 8, 8, 8, 8, A), (A, A, A, 1, 0, 8, 8, 8, A),
                (A, A, A, 1, 8, -1, 8, 8, A), (A, A, A, 1, 8, 8, 0, 8, A), (A, A, A, 1, 8, 8, 8, 0, A), (A, A, A, 1, 8, 8, 65536, 65536, A)):
        assert fin(*bad, None) == -22, bad


def test_add_position_off_the_canvas_is_refused_on_the_host():
    """positions are device memory, which the launcher cannot inspect: ``ops.sparse_points`` checks them on the host, before the
    library is loaded or anything is uploaded (the host path wraps negative indices and raises IndexError beyond the canvas)"""
    from mofa_video_amd import lib, ops
    val = torch.zeros(1, 2, 2)
    for p in ([[0, 0], [-1, 3]], [[8, 0], [1, 1]], [[0, 0], [3, 12]], [[0, -1], [0, 0]]):
        with pytest.raises(ValueError):
            ops.sparse_points(torch.tensor(p, dtype=torch.int32), val, 8, 12, lib.SPARSE_ADD)
    with pytest.raises(ValueError):                           # K > 4096
        ops.sparse_points(torch.zeros(4097, 2, dtype=torch.int32), torch.zeros(1, 4097, 2), 8, 12, lib.SPARSE_LAST)


# ---- track_points -----------------------------------------------------------------------------------------------------------
GOLDEN_TRACKS = [[(30, 40), (80, 60), (150, 90), (170, 200)], [(300, 300), (280, 250)], [(10, 370), (60, 330), (200, 350)]]
SHARED_TRACKS = [[(30, 40), (80, 60)], [(30, 40), (10, 90), (50, 120)], [(200, 200), (210, 190)], [(30, 40), (33, 41)],
                 [(200, 200), (100, 100)], [(300, 20), (300, 20)]]


def _brush(work):
    b = np.zeros((work, work), dtype=np.uint8)
    b[work * 20 // 384:work * 120 // 384, work * 10 // 384:work * 200 // 384] = 255
    b[work // 2, work // 2] = 128                            # an intermediate value is not "inside"
    return b


def _scatter(start, disp, sel, n, work):
    flow, mask = np.zeros((n, work, work, 2)), np.zeros((n, work, work))
    for (r, c), d in zip(start[sel], disp[sel]):
        flow[:, r, c] += d
        mask[:, r, c] += 1
    return flow, mask


@pytest.mark.parametrize("tracks,work,size,T", [(GOLDEN_TRACKS, 384, (384, 384), 14), (SHARED_TRACKS, 384, (384, 384), 6),
                                                (SHARED_TRACKS, 96, (1024, 576), 5), ([GOLDEN_TRACKS[1]], 384, (384, 384), 4)])
def test_track_points_scatter_equals_tracking_points_to_drags(tracks, work, size, T):
    width, height = size
    tracks = [[(x * width / 384, y * height / 384) for x, y in tr] for tr in tracks]
    brush = _brush(work)
    d = control.tracking_points_to_drags(tracks, width, height, T, brush, work=work)
    start, disp, inside = control.track_points(tracks, width, height, T, brush, work=work)
    K = len(tracks)
    assert start.dtype == np.int32 and start.shape == (K, 2) and disp.dtype == np.int32 and disp.shape == (K, T - 1, 2)
    assert inside.dtype == np.bool_ and inside.shape == (K,)
    assert bool(inside.any()) == d["in_flag"] and bool((~inside).any()) == d["out_flag"]
    for name, sel in (("in", inside), ("out", ~inside)):
        flow, mask = _scatter(start, disp, sel, T - 1, work)
        assert np.array_equal(flow, d["drag_" + name][0].numpy()) and np.array_equal(mask, d["mask_" + name][0].numpy())
    if K == len(SHARED_TRACKS):
        assert len(np.unique(start, axis=0)) < K             # shared start pixels are in play


def test_track_points_refuses_an_off_size_brush():
    with pytest.raises(ValueError):
        control.track_points(GOLDEN_TRACKS, 384, 384, 5, np.zeros((96, 96), dtype=np.uint8))
    with pytest.raises(ValueError):
        control.tracking_points_to_drags(GOLDEN_TRACKS, 384, 384, 5, np.zeros((96, 96), dtype=np.uint8))


def test_from_tracks_raises_at_the_exactness_bound():
    """points on one start pixel x max |displacement| >= 2^24: refused on the host, before CMP or the device are touched"""
    class NoCMP:
        device = "cpu"
    work = 384
    far = (1 << 23) * 1.0
    tracks = [[(5, 5), (5 + far, 5)], [(5, 5), (5 + far, 5)]]             # 2 x 2^23 = 2^24
    first = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="exact"):
        control.controlnet_flow_from_tracks(NoCMP(), first, tracks, 8, 8, 2, np.zeros((work, work), dtype=np.uint8), work=work)
    start, disp, _ = control.track_points([[(5, 5), (5 + far - 1, 5)]] * 2, work, work, 2, np.zeros((work, work), dtype=np.uint8))
    assert 2 * int(np.abs(disp).max()) < control.SPARSE_EXACT == CC.EXACT  # one below the bound passes the check


# ---- sample_inputs_face -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["fp32", "fp16"])
def test_sample_inputs_face_equals_the_reference(tag):
    G = torch.load(os.path.join(ROOT, "tests", "golden", "reference_golden_control_face.pt"), weights_only=False)
    want = G[tag]
    got = control.sample_inputs_face(G["first_frame"], G["landmarks_" + tag].clone())
    names = ("controlnet_image", "sparse_optical_flow", "mask", "first_frame_384", "sparse_optical_flow_384", "mask_384")
    assert len(got) == 6
    for name, g in zip(names, got):
        w = G["fp32"]["first_frame_384_x16"].float() / 16 if name == "first_frame_384" else want[name]
        w = w.to_dense() if w.is_sparse else w
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g, w), name
    assert got[4].dtype == G["landmarks_" + tag].dtype and tuple(got[4].shape) == (1, 4, 2, 384, 384)
    if tag == "fp16":                                         # the fp16 positions are not the fp32 ones: the dtype matters
        assert not torch.equal(got[5], G["fp32"]["mask_384"].to_dense())


# ---- the shared header on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/control_points_main.hip built with hipcc: the host side of the same header the kernels include"""
    from mofa_video_amd import _build
    exe = str(tmp_path_factory.mktemp("control_points") / "control_points_main")
    subprocess.run([_build._hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "control_points_main.hip"),
                    "-o", exe], check=True)
    return exe


def _run(exe, tmp_path, words, arrays, shape, mutant=None):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array(words, dtype="<i4").tobytes())
        for a in arrays:
            f.write(a.contiguous().numpy().tobytes())
    r = subprocess.run([exe, src, dst] + ([mutant] if mutant else []))
    if r.returncode != 0:
        return r.returncode
    return torch.from_numpy(np.fromfile(dst, dtype="<f4").reshape(shape))


def _run_sparse(exe, tmp_path, mode, pos, val, H, W, mutant=None):
    n, K = val.shape[:2]
    return _run(exe, tmp_path, [0, mode, K, n, H, W], [pos, val], (n, 4, H, W), mutant)


@pytest.mark.parametrize("name", list(CC.ADD_CASES))
def test_add_case_on_the_host(name, program, tmp_path):
    pos, val, H, W, want, largest = CC.add_case(name)
    assert largest < CC.EXACT                                 # the precondition of exact fp32 sums
    got = _run_sparse(program, tmp_path, CC.ADD, pos, val, H, W)
    assert CC.same_bits(got, want)
    assert float(want[:, 2].sum()) == val.shape[0] * pos.shape[0] and torch.equal(want[:, 2], want[:, 3])


@pytest.mark.parametrize("name", list(CC.LAST_CASES))
def test_last_case_on_the_host(name, program, tmp_path):
    pos, val, H, W, want = CC.last_case(name)
    got = _run_sparse(program, tmp_path, CC.LAST, pos, val, H, W)
    assert CC.same_bits(got, want)
    assert int(torch.isnan(want).sum()) == 2 and float(want[:, 2].max()) == 1.0
    assert int(pos.min()) < 0 and int(pos[:, 0].max()) > H - 1 and int(pos[:, 1].max()) > W - 1          # clipping is in play
    keys = (pos[:, 0].clamp(0, H - 1) * W + pos[:, 1].clamp(0, W - 1)).tolist()
    assert keys[CC.LAST_DUP[0]] == keys[CC.LAST_DUP[-1]] and keys.count(keys[3]) >= 3


def test_last_case_in_fp16_on_the_host(program, tmp_path):
    """positions and displacements formed in fp16, as the reference forms them"""
    pos, val, H, W, want = CC.last_case("40x56-n4", torch.float16)
    assert CC.same_bits(_run_sparse(program, tmp_path, CC.LAST, pos, val, H, W), want)


def test_add_position_off_the_canvas_on_the_host(program, tmp_path):
    pos, val, H, W, _want, _ = CC.add_case("corners-8x8-n1")
    for bad in ((-1, 0), (0, -1), (H, 0), (0, W)):
        p = pos.clone()
        p[2] = torch.tensor(bad, dtype=torch.int32)
        assert _run_sparse(program, tmp_path, CC.ADD, p, val, H, W) == 22


def test_mutant_first_writer_fails(program, tmp_path):
    failed = []
    for name in CC.LAST_CASES:
        pos, val, H, W, want = CC.last_case(name)
        got = _run_sparse(program, tmp_path, CC.LAST, pos, val, H, W, mutant="first_writer")
        failed.append(not CC.same_bits(got, want))
    assert all(failed), failed                                # every LAST case has a duplicate whose first and last point differ


def test_mutant_rows_and_columns_exchanged_fails(program, tmp_path):
    for name in ("40x56-n4", "8x8-n1"):                       # even a square canvas tells: the points are not symmetric
        pos, val, H, W, want = CC.last_case(name)
        got = _run_sparse(program, tmp_path, CC.LAST, pos, val, H, W, mutant="swap_rc")
        assert not CC.same_bits(got, want), name
    for name in ("k1-32x48-n3", "shared-32x48-n3", "corners-32x48-n3", "k130-8x8-n1"):
        pos, val, H, W, want, _ = CC.add_case(name)
        got = _run_sparse(program, tmp_path, CC.ADD, pos, val, H, W, mutant="swap_rc")
        assert isinstance(got, int) or not CC.same_bits(got, want), name          # off the canvas (22) or the wrong pixels


@pytest.mark.parametrize("name", list(CC.FINISH_CASES))
def test_finish_case_on_the_host(name, program, tmp_path):
    fin, fout, brush, H, W, want, _off = CC.finish_case(name)
    ref = fin if fin is not None else fout
    n, _, hs, ws = ref.shape
    got = _run(program, tmp_path, [1, fin is not None, fout is not None, brush is not None, n, hs, ws, H, W],
               [t for t in (fin, fout, brush) if t is not None], (n, 2, H, W))
    assert CC.same_bits(got, want)


def test_finish_cases_cover_what_they_claim():
    # equal sizes: the scalings are skipped, and skipping them is invisible (a multiply by 1.0f changes nothing)
    fin, fout, brush, H, W, want, _ = CC.finish_case("equal_size")
    forced = CC.finish_expect(fin, fout, brush, H, W).clone()
    forced[:, 0] *= W / fin.shape[3]
    forced[:, 1] *= H / fin.shape[2]
    assert CC.same_bits(forced, want)
    # the fp32 product: sizes where floorf(o * fl(in / out)) is not floor(o * in / out)
    hs, ws, H, W = CC.FINISH_CASES["fp32_product_differs"][:4]
    for out, inp in ((H, hs), (W, ws)):
        exact = np.arange(out) * inp // out
        assert (CC.nearest_rows(out, inp) != exact).any(), (out, inp)
    # ... which cannot happen at 7 x 5 -> 23 x 13: with in and out coprime o * in / out is an integer only at o = 0, and the fp32
    # product is off by less than 1 / out; that case keeps its place for the odd sizes
    hs, ws, H, W = CC.FINISH_CASES["fp32_product"][:4]
    for out, inp in ((H, hs), (W, ws)):
        assert (CC.nearest_rows(out, inp) == np.arange(out) * inp // out).all()
    # the torch resize the expectation uses has the kernel's index rule
    x = torch.arange(14 * 26, dtype=torch.float32).reshape(1, 1, 14, 26)
    idx = torch.nn.functional.interpolate(x, (46, 22), mode="nearest")[0, 0].long()
    assert np.array_equal(idx.numpy(), CC.nearest_rows(46, 14)[:, None] * 26 + CC.nearest_rows(22, 26)[None, :])
    # pixels with exactly one zero component, -0.0 and NaN reach the merge; brush values 0 / 1 / 128 / 254 / 255 are all there
    for name in ("equal_size", "ratio_384", "fp32_product"):
        fin, fout, brush, H, W, want, _ = CC.finish_case(name)
        assert set(brush.unique().tolist()) == {0, 1, 128, 254, 255}, name
        one_zero = ((fin[:, 0] == 0) != (fin[:, 1] == 0))
        neg_zero = (fin == 0) & torch.signbit(fin)
        assert bool(one_zero.any()) and bool(neg_zero.any()) and bool(torch.isnan(fin).any()) and bool(torch.isnan(want).any())


def test_a_flow_without_partner_goes_in_as_flow_out():
    """alone as ``flow_out`` a flow is only resized and rescaled -- what the Keypoint path needs, which has no merge; alone as
    ``flow_in`` a pixel with one zero component gives way to the (zero) partner"""
    _fin, fout, _brush, H, W, want, _ = CC.finish_case("out_only")
    one_zero = (fout[:, 0] == 0) != (fout[:, 1] == 0)
    assert bool(one_zero.any())
    plain = torch.nn.functional.interpolate(fout, (H, W), mode="nearest")
    plain[:, 0] *= W / fout.shape[3]
    plain[:, 1] *= H / fout.shape[2]
    assert CC.same_bits(want, plain)
    assert not CC.same_bits(CC.finish_expect(fout, None, None, H, W), plain)
