"""The implicit GEMM's two address generators (make_geo / x_src of the 4-wave kernels; pack_geo / tap_src / tap_advance and the
split-K cur_setup of the 8-wave kernels) over the convolution-geometry tables of tests/conv_cases.py, every case forced onto
every output tile, by EQUALITY with a per-tap fp64 reference for the exact family and inside the GEMM class for the Gaussian one
(tests/test_conv_cases_cpu.py proves the same cases, the exactness bound and the checks' ability to fail on the CPU).

Every x, out and r1 is a guarded view (NaN rows before and after, NaN columns on the left, ld > width): the 8-wave kernels take
their zeros from the buffer descriptor's extent, which has to be right for ldx > Cin.  Kernel sizes 1 / 3 / 5 / 7, dilation 1 / 2 /
4, both strides, nearest-2x input, both pads, one and two K tiles per tap, 1 to 3 K tiles on the plain table (the ring prologue
and the peeled last K step of the 8-wave kernels), ragged last tiles of every height, tiles that straddle images and clips, the
last values of the packed row geometry (10-bit oy / ox and 2047 images on the 8-wave tiles, oy with bit 31 of the word set on the
4-wave tiles), and split-K slices that start inside a tap of a 5 x 5, 7 x 7 or dilated convolution."""
import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    cc.release()


def _einval():
    from mofa_video_amd.lib import MofaHipError
    return dict(expected_exception=MofaHipError, match=r"mofa_igemm_f16 failed with code -22$")


def _plan(s, epi="bias", tile=None):
    """what the launcher decides for this case on this device (mofa_igemm_plan)"""
    return cc.plan(s, epi, tile, n_cu=torch.cuda.get_device_properties(0).multi_processor_count)


WAVE4 = (cc.TILES["128x128"], cc.TILES["192x128"])


def _launch(ops, s, family, epi, tile, fresh=False, split_k=None):
    """one launch, checked -> (its messages, the result on the device)"""
    c = cc.case(s, family, epi, tile, split_k)
    r = cc.run(ops, c, DEV, drop=("out",) if fresh else ())
    worst, errs = cc.check_run(c, r, fresh=fresh)
    return worst, errs, (r.ret if fresh else r.placed["out"].t)


def _matrix(ops, s, tile, epis):
    """family E with every epilogue, through the guarded out= buffer and as a fresh tensor; family A with one.  All launches of
    the case run back to back; what failed is reported at the end"""
    bad, top = [], 0.0
    for epi in epis:
        for fresh in (False, True):
            bad += _launch(ops, s, "E", epi, tile, fresh)[1]
    worst, errs, _ = _launch(ops, s, "A", epis[len(s.id) % len(epis)], tile)
    return bad + errs, max(top, worst)


@pytest.mark.parametrize("tile", list(cc.TILES))
@pytest.mark.parametrize("s", cc.CONV_ROWS, ids=repr)
def test_conv_matrix(ops, s, tile):
    if s.id in cc.WAVE4_ONLY and tile in cc.PIPE:            # Hout > 1024 does not fit the 10-bit field: refused, not truncated
        with pytest.raises(**_einval()):
            cc.run(ops, cc.case(s, "E", "bias", tile), DEV)
        assert _plan(s, tile=tile).rc == -22
        return
    bad, worst = _matrix(ops, s, tile, cc.EPIS)
    print(f"CONV-EDGE {s.id} {tile}: family E {'equal' if not bad else 'DIFFERS'}, family A worst err / bound {worst:.3f}")
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("tile", list(cc.TILES))
@pytest.mark.parametrize("s", cc.CONVT_ROWS, ids=repr)
def test_convt3_matrix(ops, s, tile):
    bad, worst = _matrix(ops, s, tile, cc.EPIS)
    print(f"CONV-EDGE {s.id} {tile}: family E {'equal' if not bad else 'DIFFERS'}, family A worst err / bound {worst:.3f}")
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("tile", list(cc.TILES))
@pytest.mark.parametrize("K", cc.PLAIN_K)
def test_plain_shallow_k_matrix(ops, K, tile):
    """1, 2 and 3 K tiles x M in {1, 255, 256, 257, 513} x N in {8 ... 328}: fewer K tiles than the 8-wave ring has slots"""
    bad, top = [], 0.0
    for s in cc.plain_rows(K):
        errs, worst = _matrix(ops, s, tile, (cc.plain_epi(s),))
        bad, top = bad + errs, max(top, worst)
    print(f"CONV-EDGE plain K{K} {tile}: {len(cc.plain_rows(K))} shapes, family A worst err / bound {top:.3f}")
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("tile", list(cc.TILES))
def test_refused_forced_tiles(ops, tile):
    """what the launcher documents for a forced tile: N % 8 != 0 and an activation on a residual kind are MOFA_EINVAL on the
    8-wave tiles (no narrow-store path, only the plain kind carries activation code); the 4-wave tiles compute both exactly"""
    n68 = cc.Spec("plain-K64-M257-N68", "plain", 64, 68, M=257)
    n76 = cc.conv("k3-N76", 11, 13, N=76, M=286)
    jobs = [(n68, "bias"), (n76, "relu"), (cc.CONV_BY_ID["k5s2"], "r1-relu"), (cc.plain(128, 257, 72), "r1-relu")]
    bad = []
    for s, epi in jobs:
        if tile in cc.PIPE:
            with pytest.raises(**_einval()):
                cc.run(ops, cc.case(s, "E", epi, tile), DEV)
            assert _plan(s, epi, tile).rc == -22
        else:
            bad += _launch(ops, s, "E", epi, tile)[1]
    assert not bad, bad


@pytest.mark.parametrize("s", cc.PIPE_OVER_ROWS, ids=repr)
def test_packing_edges_of_the_8_wave_tiles(ops, s):
    """Wout = 1025 and 2048 images, one past the 10-bit ox field and the img << 20 field: the forced 8-wave tiles refuse, the
    launcher's own choice is exact and, by its plan, a 4-wave tile (at N = 72 the model's first choice; with the fall-back from an
    8-wave choice at N = 320: tests/test_igemm_plan_cpu.py)"""
    for tile in cc.PIPE:
        with pytest.raises(**_einval()):
            cc.run(ops, cc.case(s, "E", "bias", tile), DEV)
    bad, _ = _matrix(ops, s, None, cc.EPIS)
    assert not bad, (len(bad), bad[:6])
    assert all(_plan(s, epi).tile in WAVE4 for epi in cc.EPIS)


def test_wave4_oy_edge(ops):
    """Hout = 40000 through the launcher's own choice (the forced 4-wave tiles run it in test_conv_matrix): make_geo packs
    (oy << 16) | ox, and from oy = 32768 on bit 31 of the word is set, so the decode must shift logically.  This provokes no
    fault: a mis-decoded (negative) oy only makes x_src count every tap as out of the image and return the zero page, so the
    failure is a wrong VALUE (bias alone in rows 32768 ... 39999), which the equality names.  Hout = 65536 does not fit the
    16-bit field and is refused by every tile and by the default, before any launch"""
    s = cc.CONV_BY_ID["k3-H40000"]
    bad, _ = _matrix(ops, s, None, cc.EPIS)
    assert not bad, (len(bad), bad[:6])
    assert all(_plan(s, epi).tile in WAVE4 for epi in cc.EPIS)
    for tile in (None,) + tuple(cc.TILES):
        with pytest.raises(**_einval()):
            cc.run(ops, cc.case(cc.WAVE4_OVER_ROW, "E", "bias", tile), DEV)


@pytest.mark.parametrize("s", cc.SPLIT_ROWS, ids=repr)
def test_split_k_slice_starts_inside_a_tap(ops, s):
    """the 256x320 tile cuts the two remainder tiles of these launches into 6 / 6 / 6 / 8 / 4 K slices (conv_cases.SPLIT_SLICES,
    asserted against mofa_igemm_plan in the CPU file for 16 CUs and more): cur_setup rebuilds (ky, kx, K tile within the tap) from a slice start in the
    middle of a tap with ksize 5 / 7 (aux.ks_d) and with dilation.  Family E: split and whole launches equal each other and the
    reference.  Family A: both inside the tolerance, NOT equal (the proof that the split path ran: another fp32 summation
    order), and the split result bit-identical on a repeat launch"""
    bad = []
    for epi in cc.EPIS:
        _, e0, whole = _launch(ops, s, "E", epi, "256x320", split_k=False)
        _, e1, split = _launch(ops, s, "E", epi, "256x320", split_k=True)
        bad += e0 + e1
        if not torch.equal(whole, split):
            bad.append(f"{s.id} {epi}: family E differs between split and whole launches")
    w0, e0, whole = _launch(ops, s, "A", "bias", "256x320", split_k=False)
    w1, e1, split = _launch(ops, s, "A", "bias", "256x320", split_k=True)
    _, e2, again = _launch(ops, s, "A", "bias", "256x320", split_k=True)
    print(f"CONV-EDGE {s.id}: family A worst err / bound whole {w0:.3f}, split {w1:.3f}; "
          f"{int((whole != split).sum())} / {whole.numel()} elements differ between them")
    assert not bad + e0 + e1 + e2, bad + e0 + e1 + e2
    assert not torch.equal(whole, split), "split and whole launches agree bit for bit: did the split path run?"
    assert torch.equal(split, again)
