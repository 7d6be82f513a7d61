"""The folded up-sampler convolution (MOFA_MODE_CONV3X3_UP2F) on the GPU, on both 8-wave tiles:

  5. BIT equality with the classic launch (CONV3X3, up = 2) on small-integer data -- every fp32 sum is exact, so both forms round
     the same number -- written into a guarded, NaN-prefilled column view with ldo > N: every element of the view is written,
     every guard element stays.  The shapes are the issue's; (1, 128, 132, 512, 320) was meant to reach the split-K fix-up, but
     the planner's pinned rule (igemm320_split: 2 us x nk x (1 - 1 / S) >= 50 us, S <= nk / 8) leaves its 8 remainder tiles whole
     at nk = 32 (48 us), so it runs as a 264-tile two-round launch and (1, 128, 132, 576, 320) (nk = 36: split 4) is ADDED for the
     fix-up kernel, with ``plan.split > 1`` asserted first;
  6. accuracy on random fp16 data against the fp64 reference formed from the UNFOLDED weights on the up-sampled input, per element
     |got - ref| <= 2^-11 |ref| + 2^-11 S + 4 Cin 2^-24 S + 2^-25 with S = sum |x| |w_folded| (output rounding, one rounding per
     folded weight, fp32 accumulation);
  7. wiring: the tiny UNet's up blocks (which write into a column slice of the next concat buffer) and the tiny VAE decoder's up
     stages take the folded launch with ``ops.UP2_FOLD`` on (timer tags) and nothing else changes; with the switch off, or under a
     forced 4-wave tile, a ``Conv3x3(up=2)`` call is the classic ``ops.igemm`` launch bit for bit; a captured UNet step body and a
     captured VAE decode replay the eager result, folded and classic."""
import pytest
import torch

import up2_fold_cases as uc
from helpers import TINY, TINY_VAE
from mofa_video_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILES = {"256x256": L.TILE_256X256, "256x320": L.TILE_256X320}
SHAPES = [(1, 1, 1, 64, 8), (3, 2, 3, 64, 72), (2, 5, 7, 128, 320), (1, 16, 16, 64, 328), (1, 16, 17, 64, 640), (3, 40, 48, 64, 1280),
          (1, 128, 132, 512, 320), (1, 128, 132, 576, 320)]
ROUNDS, WHOLE, SPLIT = SHAPES[5], SHAPES[6], SHAPES[7]
GUARD, COL0, SENTINEL = 3, 8, 777.0


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import ops as o
    L.load()
    return o


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def classic(ops):
    """per shape, computed once: tokens, folded weight, bias, the classic launch's output (the launcher's own tile)"""
    from mofa_video_amd.weights import fold_up2, pack_conv3x3
    cache = {}

    def get(shape):
        if shape not in cache:
            nimg, H, Wd, Cin, N = shape
            g = torch.Generator(device=DEV).manual_seed(sum(shape))
            x = torch.randint(-2, 3, (nimg * H * Wd, Cin), generator=g, device=DEV).half()
            w = torch.randint(-1, 2, (N, Cin, 3, 3), generator=g, device=DEV).float()
            b = torch.randint(-3, 4, (N,), generator=g, device=DEV).float()
            ref = ops.igemm(x, pack_conv3x3(w), b, geom=ops.conv3x3_geom(H, Wd, up=2))
            cache[shape] = (x, fold_up2(w), b, ref)
        return cache[shape]
    return get


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_bit_equal_to_the_classic_launch(ops, classic, n_cu, shape, tile):
    nimg, H, Wd, Cin, N = shape
    p = uc.plan(uc.make_args(nimg, H, Wd, Cin, N, tile=TILES[tile]), n_cu)
    assert p.rc == 0 and p.tile == TILES[tile]
    if shape == ROUNDS and p.tiles_m * p.tiles_n <= p.grid:
        pytest.skip(f"{p.tiles_m * p.tiles_n} tiles fit one round of {p.grid} workgroups on {n_cu} CUs")
    if shape in (WHOLE, SPLIT) and tile == "256x320":
        assert p.tiles_m * p.tiles_n == 264
        if shape == SPLIT:
            if n_cu // 8 * 8 != 256:
                pytest.skip(f"264 tiles leave no 8-tile remainder on {n_cu} CUs")
            assert p.split > 1 and p.rem_tiles == 8 and p.launches == 2
    x, wf, b, ref = classic(shape)
    M, ldo = 4 * nimg * H * Wd, COL0 + N + 16
    buf = torch.full((M + 2 * GUARD, ldo), SENTINEL, dtype=torch.float16, device=DEV)
    view = buf[GUARD:GUARD + M, COL0:COL0 + N]
    view.fill_(float("nan"))
    out = ops.igemm(x, wf, b, geom=ops.conv3x3_up2f_geom(H, Wd), out=view, tile=TILES[tile])
    assert out.data_ptr() == view.data_ptr()
    assert not torch.isnan(view).any(), f"{int(torch.isnan(view).sum())} elements of the view not written"
    assert torch.equal(view, ref), f"{int((view != ref).sum())} of {ref.numel()} elements differ from the classic launch"
    guard = buf.clone()
    guard[GUARD:GUARD + M, COL0:COL0 + N] = SENTINEL
    assert bool((guard == SENTINEL).all()), "a guard element was overwritten"


def _shifted(xp, H, Wd, oy, ox):
    """tokens [n H W, C] of the padded fp64 image xp [n, C, H + 2, W + 2] shifted by (oy, ox) in -1..1"""
    return uc.tokens(xp[:, :, 1 + oy:1 + oy + H, 1 + ox:1 + ox + Wd])


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("shape", [(2, 5, 7, 128, 320), (1, 9, 16, 1280, 640)], ids=repr)
def test_accuracy_against_the_unfolded_fp64_reference(ops, shape, tile):
    from mofa_video_amd.weights import fold_up2
    nimg, H, Wd, Cin, N = shape
    g = torch.Generator(device=DEV).manual_seed(11 + Cin)
    x = torch.randn(nimg, Cin, H, Wd, generator=g, device=DEV).half()
    w = (torch.randn(N, Cin, 3, 3, generator=g, device=DEV) * (9 * Cin) ** -0.5).half()
    b = torch.randn(N, generator=g, device=DEV)
    wf = fold_up2(w)
    got = ops.igemm(uc.tokens(x).contiguous(), wf, b, geom=ops.conv3x3_up2f_geom(H, Wd), tile=TILES[tile]).double()
    # fp64 reference: the unfolded fp16 weights on the up-sampled input, as nine shifted matrix products
    xu = torch.nn.functional.pad(x.double().repeat_interleave(2, 2).repeat_interleave(2, 3), (1, 1, 1, 1))
    ref = b.double()[None, :].repeat(4 * nimg * H * Wd, 1)
    for ky in range(3):
        for kx in range(3):
            ref += _shifted(xu, 2 * H, 2 * Wd, ky - 1, kx - 1) @ w[:, :, ky, kx].double().T
    # S = sum |x| |w_folded| per output element: the four 2x2 convolutions of |x| with |wf|, scattered by phase
    xa = torch.nn.functional.pad(x.double().abs(), (1, 1, 1, 1))
    S = torch.zeros(nimg, 2 * H, 2 * Wd, N, dtype=torch.float64, device=DEV)
    wfa = wf.double().abs().reshape(4, N, 4, Cin)
    for p in range(4):
        a, bb = p >> 1, p & 1
        s = sum(_shifted(xa, H, Wd, a - 1 + ty, bb - 1 + tx) @ wfa[p, :, 2 * ty + tx].T for ty in range(2) for tx in range(2))
        S[:, a::2, bb::2] = s.reshape(nimg, H, Wd, N)
    S = S.reshape(-1, N)
    bound = 2.0 ** -11 * ref.abs() + 2.0 ** -11 * S + 4 * Cin * 2.0 ** -24 * S + 2.0 ** -25
    ratio = ((got - ref).abs() / bound).max().item()
    print(f"up2f {shape} {tile}: worst |err| / bound = {ratio:.3f}, rel-L2 {((got - ref).norm() / ref.norm()).item():.2e}")
    assert ratio <= 1.0, ratio


# ---- 7: wiring -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from mofa_video_amd import schema
    from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
    from mofa_video_amd.vae import AutoencoderKLTemporalDecoder
    hu = UNetSpatioTemporalConditionControlNetModel(schema.synthetic_state_dict(schema.unet_schema(TINY), seed=3), TINY, DEV)
    hv = AutoencoderKLTemporalDecoder(schema.synthetic_state_dict(schema.vae_decoder_schema(**TINY_VAE), seed=4), TINY_VAE, DEV)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(2, 2, 8, 16, 16, generator=g) * 0.5).to(DEV)
    emb = torch.randn(2, 1, TINY["cross_attention_dim"], generator=g).to(DEV)
    z = (torch.randn(2 * 8 * 8, 64, generator=g) * 0.5).half().to(DEV)
    z[:, 4:] = 0
    ids = torch.tensor([[6.0, 127.0, 0.02]] * 2, device=DEV)
    boc = TINY["block_out_channels"]
    shapes = [(boc[0], 16, 16)] * 3 + [(boc[0], 8, 8)] + [(boc[1], 8, 8)] * 2 + [(boc[1], 4, 4)] + [(boc[2], 4, 4)] * 2 + \
             [(boc[2], 2, 2)] + [(boc[3], 2, 2)] * 2
    res = [(torch.randn(4, *sh, generator=g) * 0.3).half().float().to(DEV) for sh in shapes]
    mid = (torch.randn(4, boc[3], 2, 2, generator=g) * 0.3).half().float().to(DEV)

    def unet():
        return hu(x, torch.tensor(0.8), emb, down_block_additional_residuals=res, mid_block_additional_residual=mid,
                  return_dict=False, added_time_ids=ids)[0]

    def vae():
        return hv.decoder(z[:, :hv.decoder.in_ld].contiguous(), 2, 8, 8)[0]

    # the body of a denoise step as the pipeline captures it: context and token inputs exist before, the networks run on tokens
    from mofa_video_amd import ops as o
    c = hu.make_ctx(torch.tensor(0.8), emb, ids, 2, 2)
    xt = o.nchw_to_tokens(x.reshape(4, 8, 16, 16).float(), ld=hu.in_ld)
    rt, mt = [o.nchw_to_tokens(r) for r in res], o.nchw_to_tokens(mid)

    def unet_step():
        return hu.forward_tokens(xt, c, 16, 16, rt, mt)
    return unet, vae, unet_step, hv


def _run(ops, fn, fold, force=L.TILE_AUTO):
    """(output, timer tags of the igemm launches) of fn() under the switch / forced tile"""
    old = ops.UP2_FOLD, ops.FORCE_TILE, ops.TIMER
    ops.UP2_FOLD, ops.FORCE_TILE, ops.TIMER = fold, force, ops.LaunchTimer()
    try:
        out = fn().clone()
        torch.cuda.synchronize()
        return out, [t for t, _ in ops.TIMER.tags]
    finally:
        ops.UP2_FOLD, ops.FORCE_TILE, ops.TIMER = old


@pytest.mark.parametrize("which", ("unet_up_blocks", "vae_up_stages"))
def test_up_samplers_take_the_folded_launch(ops, tiny, which):
    fn = tiny[0] if which == "unet_up_blocks" else tiny[1]
    off, tags_off = _run(ops, fn, False)
    on, tags_on = _run(ops, fn, True)
    ups = [i for i, t in enumerate(tags_off) if t[0] == L.MODE_CONV3X3 and t[2] == 2]
    assert len(ups) == 3 and not [t for t in tags_off if t[0] == L.MODE_CONV3X3_UP2F]
    assert len(tags_on) == len(tags_off)
    for i, (a, b) in enumerate(zip(tags_off, tags_on)):
        if i in ups:                                               # (mode, stride, up, M, N, Ktot, act): same rows, 4/9 of K
            assert b == (L.MODE_CONV3X3_UP2F, 1, 2, a[3], a[4], a[5] * 4 // 9, a[6]), (a, b)
        else:
            assert a == b, (i, a, b)
    assert torch.isfinite(on.float()).all() and ((on.float() - off.float()).norm() / off.float().norm()).item() < 5e-3
    # a forced 4-wave tile keeps the classic launch with the switch on
    forced_on, tags_f = _run(ops, fn, True, L.TILE_192X128)
    forced_off, tags_g = _run(ops, fn, False, L.TILE_192X128)
    assert tags_f == tags_g and not [t for t in tags_f if t[0] == L.MODE_CONV3X3_UP2F] and torch.equal(forced_on, forced_off)


def test_switched_off_call_is_the_classic_igemm_launch(ops, tiny):
    """``Conv3x3(up=2)`` with the switch off (or under a forced 4-wave tile) against the parent's line spelled out --
    ``ops.igemm(x, conv.w, conv.b, geom=conv3x3_geom(H, W, 1, 2))`` -- bit for bit, fresh output and column slice of a wider buffer;
    with the switch on the same calls are the folded launch, and the slice receives what the fresh output holds"""
    conv = tiny[3].decoder.up_blocks[0][1]
    N, Cin, H, Wd = conv.w.shape[0], conv.w.shape[1] // 9, 8, 8
    assert conv.up == 2 and conv.wf is not None and tuple(conv.wf.shape) == (4 * N, 4 * Cin)
    x = (torch.randn(2 * H * Wd, Cin, generator=torch.Generator().manual_seed(9)) * 0.5).half().to(DEV)
    direct = ops.igemm(x, conv.w, conv.b, geom=ops.conv3x3_geom(H, Wd, 1, 2))

    def sliced():
        buf = torch.full((8 * H * Wd, N + 64), SENTINEL, dtype=torch.float16, device=DEV)
        conv(x, H, Wd, out=buf[:, :N])
        assert bool((buf[:, N:] == SENTINEL).all())
        return buf[:, :N]
    for fold, force in ((False, L.TILE_AUTO), (False, L.TILE_256X320), (True, L.TILE_192X128)):
        fresh, tags = _run(ops, lambda: conv(x, H, Wd), fold, force)
        ref = direct if force == L.TILE_AUTO else ops.igemm(x, conv.w, conv.b, geom=ops.conv3x3_geom(H, Wd, 1, 2), tile=force)
        assert [t[0] for t in tags] == [L.MODE_CONV3X3] and torch.equal(fresh, ref), (fold, force)
        assert torch.equal(_run(ops, sliced, fold, force)[0], ref), (fold, force)
    fresh, tags = _run(ops, lambda: conv(x, H, Wd), True)
    assert [t[0] for t in tags] == [L.MODE_CONV3X3_UP2F]
    into, tags = _run(ops, sliced, True)
    assert [t[0] for t in tags] == [L.MODE_CONV3X3_UP2F] and torch.equal(into, fresh)
    assert ((fresh.float() - direct.float()).norm() / direct.float().norm()).item() < 2e-3


@pytest.mark.parametrize("which", ("unet_step", "vae_decode"))
def test_folded_launch_inside_a_captured_step(ops, tiny, which):
    """decisions are cached per layer and shape, so nothing is planned inside a capture: the captured UNet step body (up blocks
    writing into the next concat buffer's column slice) and the captured VAE decode replay the eager result, folded and classic"""
    fn = tiny[2] if which == "unet_step" else tiny[1]
    for fold in (True, False):
        old = ops.UP2_FOLD
        ops.UP2_FOLD = fold
        try:
            eager = fn().clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()                                               # warm-up on the capture stream (its split-K scratch exists)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                out = fn()
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager), fold
        finally:
            ops.UP2_FOLD = old
