"""The folded up-sampler convolution (MOFA_MODE_CONV3X3_UP2F) without a GPU:

  1. ``weights.fold_up2`` is exact: four 2x2 convolutions with its weights equal nearest-2x + 3x3 on small-integer data;
  2. a torch model of the launch as the kernels address it (phase-padded tile rows, exported row map, per-tile weight base, tap
     origin per phase) reproduces the same references, and each of six mutants of it fails at least one case;
  3. the exported row map is a bijection of the valid tile rows onto the output rows, -1 on padding, one phase per 256-row tile;
  4. the plans of the mode through ``mofa_igemm_plan`` and the launcher's own verdict on what it refuses."""
import ctypes

import pytest
import torch

import up2_fold_cases as uc
from mofa_video_amd import lib as L
from mofa_video_amd import ops
from mofa_video_amd.weights import fold_up2

EINVAL = -22
T128, T192, T256, T320 = L.TILE_128X128, L.TILE_192X128, L.TILE_256X256, L.TILE_256X320
N_OUT = 8
CASES = [(g, c) for g in uc.GEOMS for c in uc.CINS]


@pytest.fixture(scope="module")
def refs():
    """(x, w, b, fp64 reference, folded fp16 weight) per case, computed once"""
    out = {}
    for (nimg, H, Wd), Cin in CASES:
        x, w, b = uc.int_data(nimg, H, Wd, Cin, N_OUT)
        out[(nimg, H, Wd), Cin] = (x, w, b, uc.reference(x, w, b), fold_up2(w))
    return out


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,Cin", CASES, ids=repr)
def test_fold_up2_is_exact_on_integers(refs, geom, Cin):
    x, w, b, ref, wf = refs[geom, Cin]
    assert wf.dtype is torch.float16 and tuple(wf.shape) == (4 * N_OUT, 4 * 64)
    assert torch.equal(wf.double(), wf.double().round()) and wf.abs().max() <= 4     # sums of 1, 2 or 4 taps of -1..1
    assert torch.equal(uc.folded_conv(x, wf, b), ref)


def test_fold_up2_sums_the_rounded_taps_in_fp32():
    """each folded weight = fp16(fp32 sum of the fp16-rounded taps): checked against the sums spelled out per phase and tap"""
    w = torch.randn(8, 70, 3, 3, generator=torch.Generator().manual_seed(3))
    wf = fold_up2(w).reshape(2, 2, 8, 2, 2, 128)
    wh = w.half().float()
    sets = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}                  # phase -> classic taps behind folded tap 0 / 1
    for a in range(2):
        for b in range(2):
            for ty in range(2):
                for tx in range(2):
                    s = sum(wh[:, :, ky, kx] for ky in sets[a][ty] for kx in sets[b][tx])
                    assert torch.equal(wf[a, b, :, ty, tx, :70], s.half()), (a, b, ty, tx)
    assert not wf[..., 70:].any()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
def _model(refs, geom, Cin, mutant=None):
    nimg, H, Wd = geom
    x, w, b, ref, wf = refs[geom, Cin]
    rows = uc.row_map(uc.make_args(nimg, H, Wd, 64, N_OUT))
    got = uc.launch_model(uc.tokens(uc.pad_channels(x, 64)), wf, b, nimg, H, Wd, rows, mutant)
    return got, uc.tokens(ref)


@pytest.mark.parametrize("geom,Cin", CASES, ids=repr)
def test_launch_model_reproduces_the_reference(refs, geom, Cin):
    got, ref = _model(refs, geom, Cin)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("mutant", uc.MUTANTS)
def test_every_mutant_of_the_model_fails_a_case(refs, mutant):
    failed = []
    for geom, Cin in CASES:
        got, ref = _model(refs, geom, Cin, mutant)
        if not torch.equal(got, ref):
            failed.append((geom, Cin))
    assert failed, f"mutant {mutant} passes every case"


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
ROWMAP_GEOMS = {1: (1, 1, 1), 255: (1, 15, 17), 256: (1, 16, 16), 257: (1, 1, 257), 7200: (50, 9, 16), 28800: (50, 18, 32)}


@pytest.mark.parametrize("Mq", sorted(ROWMAP_GEOMS))
def test_row_map_is_a_bijection_with_one_phase_per_tile(Mq):
    nimg, H, Wd = ROWMAP_GEOMS[Mq]
    assert nimg * H * Wd == Mq
    a = uc.make_args(nimg, H, Wd, 64, 8)
    rows = uc.row_map(a)
    tiles = 4 * ((Mq + 255) // 256)
    assert len(rows) == 256 * tiles
    valid = [r for r in rows if r >= 0]
    assert sorted(valid) == list(range(4 * Mq)) and all(r == -1 for r in rows if r < 0)
    for t in range(tiles):
        q0 = (t >> 2) * 256
        for i, r in enumerate(rows[256 * t:256 * t + 256]):
            q = q0 + i
            if q >= Mq:
                assert r == -1, (t, i)
                continue
            img, y, x = q // (H * Wd), q % (H * Wd) // Wd, q % Wd
            assert r == (img * 2 * H + 2 * y + (t & 3) // 2) * 2 * Wd + 2 * x + (t & 3) % 2, (t, i)
            assert ((r // (2 * Wd)) % 2, r % 2) == ((t & 3) >> 1, t & 1), (t, i)          # the tile's one phase
    fn = L.load().mofa_igemm_up2f_row
    assert fn(ctypes.byref(a), -1) == EINVAL and fn(ctypes.byref(a), 256 * tiles) == EINVAL and fn(None, 0) == EINVAL
    assert fn(ctypes.byref(uc.make_args(nimg, H, Wd, 64, 8, mode=L.MODE_CONV3X3)), 0) == EINVAL   # not this mode


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", (T256, T320))
def test_tiles_m_is_four_phases_of_padded_rows(tile):
    for Mq, (nimg, H, Wd) in ROWMAP_GEOMS.items():
        p = uc.plan(uc.make_args(nimg, H, Wd, 64, 320, tile=tile))
        assert (p.rc, p.tile, p.kind, p.tiles_m) == (0, tile, 0, 4 * ((Mq + 255) // 256)), Mq
        assert p.tiles_n == (320 + (255 if tile == T256 else 319)) // (256 if tile == T256 else 320)


def test_bench_shapes_run_on_the_8_wave_tiles():
    for nimg, H, Wd, Cin, N in uc.BENCH:
        p = uc.plan(uc.make_args(nimg, H, Wd, Cin, N))
        assert p.rc == 0 and p.tile == (T320 if N in (1280, 640) else p.tile) and p.tile in (T256, T320), (N, p.tile)
    p = uc.plan(uc.make_args(*uc.BENCH[1]))                      # 115 200 rows: 1808 tiles = 7 rounds + 16, cut along K
    assert (p.tiles_m * p.tiles_n, p.full_tiles, p.rem_tiles, p.split > 1, p.launches) == (1808, 1792, 16, True, 2)


def test_split_k_of_a_partial_last_round():
    """264 tiles on 256 CUs leave 8 remainder tiles.  igemm320_split cuts them only where 2 us x nk x (1 - 1 / S) is at least 50 us
    with S <= nk / 8: at Cin = 512 (nk = 32, S = 4: 48 us) the launch stays whole, at Cin = 576 (nk = 36, S = 4: 54 us) it splits --
    the shape test_igemm_up2_fold_gpu.py sends through the fix-up kernel"""
    whole, cut = uc.plan(uc.make_args(1, 128, 132, 512, 320)), uc.plan(uc.make_args(1, 128, 132, 576, 320))
    assert (whole.tile, whole.tiles_m * whole.tiles_n, whole.split) == (T320, 264, 1)
    assert (cut.tile, cut.split, cut.full_tiles, cut.rem_tiles, cut.launches) == (T320, 4, 256, 8, 2)
    assert uc.plan(uc.make_args(1, 128, 132, 576, 320, ws=False)).split == 1


REFUSED = [dict(tile=T128), dict(tile=T192), dict(stats=0x60000000), dict(act=L.ACT_SILU), dict(r1=0x70000000, ldr1=320),
           dict(r2=0x70000000, ldr2=320), dict(rowvec=0x70000000), dict(Hout=21), dict(Wout=27), dict(stride=2), dict(up=1),
           dict(ksize=5), dict(dil=2), dict(pad=L.PAD_TRAILING), dict(M=4 * 2 * 10 * 14 + 8), dict(geom=(1, 1025, 1)),
           dict(geom=(1, 1, 1025)), dict(geom=(2048, 1, 1)), dict(N=324, ldo=324), dict(x=uc.X + 8), dict(Cin=48, ldx=48)]


def test_refusals_are_the_launchers():
    """one violated rule at a time: the plan and mofa_igemm_f16 itself (NULL stream, nothing can launch) give MOFA_EINVAL"""
    l = L.load()
    assert uc.plan(uc.make_args(2, 10, 14, 64, 320)).rc == 0
    for last in (dict(geom=(1, 1024, 1)), dict(geom=(1, 1, 1024)), dict(geom=(2047, 1, 1))):
        assert uc.plan(uc.make_args(*last["geom"], 64, 320)).rc == 0, last
    for bad in REFUSED:
        kw = dict(bad)
        geom = kw.pop("geom", (2, 10, 14))
        a = uc.make_args(*geom, 64, 320)
        for k, v in kw.items():
            setattr(a, k, v)
        assert uc.plan(a).rc == l.mofa_igemm_f16(ctypes.byref(a), None) == EINVAL, bad


def test_auto_falls_back_from_256x320_to_256x256():
    """what 256x320 alone refuses (weight offsets beyond its bound) runs on 256x256, and is refused when 256x320 is forced"""
    big = (1, 16, 16, 12800, 10240)                               # (4 N + 320) x 4 Cin x 2 bytes >= 0x7ff00000
    assert uc.plan(uc.make_args(*big)).tile == T256 and uc.plan(uc.make_args(*big, tile=T320)).rc == EINVAL


def test_ops_geometry_and_switch():
    g = ops.conv3x3_up2f_geom(9, 16)
    assert (g.mode, g.Hin, g.Win, g.Hout, g.Wout, g.stride, g.up, g.ksize, g.dil, g.pad) == (3, 9, 16, 18, 32, 1, 2, 3, 1, L.PAD_SAME)
    assert ops.UP2_FOLD is True or ops.UP2_FOLD is False
