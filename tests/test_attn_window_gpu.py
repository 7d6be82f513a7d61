"""mofa_attn_temporal_long_window_f16 (csrc/attention.hip attn_temporal_long_window_kernel) on the GPU, driven through
``ops.attn_temporal_window`` on the cases of tests/attn_window_cases.py (tests/test_attn_window_cpu.py proves the table on the
CPU): every shard of every layout against float64 of the WHOLE clip under the dense kernel's bound; the two bit equalities the
header states -- (a) the local kernel where the buffer is the clip, (b) row by row the key-mask kernel under that row's mask --;
repeat launches; large finite values in the duplicate band slots and in query rows >= Tq without influence; guard rows round
``out``; and the whole path on virtual ranks (``parallel.ThreadComm``: N ranks as N threads on one GPU) -- the temporal block and
the flow pipeline with ``window_keys=True`` against the single-rank windowed block / pipeline.  Nothing here runs on more than
one GPU.

Virtual ranks against the single rank: rel-L2 < 2e-3 tensor-wide and for every frame, max|delta| / max|ref| of every frame below
``ABS`` -- the bounds of tests/test_sharded_long_gpu.py, for its reason (the same arithmetic up to the summation order of the
temporal GroupNorm statistics and, here, of the attention's keys: slot s of a rank's buffer is not frame s of the clip).
Measured on one MI355X: the block, 128 frames over 4 shards under (31, 1): bit-identical on the middle ranks at both head dims, rel-L2
at most 2.3e-5 on rank 0 (head dim 128); 66 frames over 2 shards under (31, 33): at most 1.7e-5 tensor-wide, 5.9e-5 per frame,
max-abs / max|ref| 3.2e-4.  The pipeline on world 4 (identical on every rank): 40 frames under (8, 1) tensor-wide 8.6e-4, per frame at
most 1.02e-3, max-abs / max|ref| at most 1.26e-3 (frame 36); 130 frames under (12, 2) -- the single rank runs the streaming kernel --
8.9e-4, 1.09e-3 and 1.43e-3 (frame 128).  Every table case against fp64: worst err / bound below 0.2."""
import threading

import pytest
import torch

import attn_local_cases as lc
import attn_window_cases as wc
import sharded_long_checks as sc
import window_shard_checks as ws
from helpers import TINY, TINY_CN, check_frames, oracle_models, rel_l2, synthetic_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
HW = wc.HW
ABS = 3.5e-3               # per-frame max|delta| / max|ref| vs single rank: the bar of tests/test_sharded_long_gpu.py


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    wc.release()
    lc.release()


def _run(ops, d, D, **over):
    kw = dict(d.kw)
    kw.update(over)
    return ops.attn_temporal_window(d.q.to(DEV), d.k.to(DEV), d.v.to(DEV), d.clips, d.g.S, HW, d.heads, head_dim=D, **kw)


# ---- 1. every case against float64 of the whole clip ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", wc.LAYOUTS)
def test_table_cases_against_fp64(ops, layout):
    bad = []
    for case in [c for c in wc.CASES if c[1:5] == layout]:
        d = wc.window_data(*case)
        out = _run(ops, d, case[0])
        again = _run(ops, d, case[0])
        assert torch.equal(out, again), (case, "the repeat launch differs")
        worst, msg = wc.close_errors(out.cpu(), d.expect, wc.BOUND, f"hd{case[0]} {layout} shard {case[5]} S{d.g.S} Tq{d.g.Tq}")
        print(f"ATTN-WINDOW hd{case[0]} {layout} shard {case[5]} (S {d.g.S}, Tq {d.g.Tq}): worst err / bound {worst:.3f}")
        bad += [msg] if msg is not None else []
    assert not bad, (len(bad), bad[:4])


# ---- 2. equality (a): the buffer is the clip -> the local kernel's bits -------------------------------------------------------------
@pytest.mark.parametrize("D,T,r", [(64, 1, 0), (64, 31, 4), (64, 33, 0), (64, 64, 16), (64, 97, 31), (64, 128, 12), (64, 128, 127), (64, 128, 500),
                                   (128, 33, 4), (128, 65, 15), (128, 128, 24)])
def test_whole_clip_equals_the_local_kernel(ops, D, T, r):
    clips, heads = 2, lc.HEADS[D]
    q, k, v = (lc.ac._pack_temporal(t).to(DEV) for t in lc.operands(D, T, clips))
    ref = ops.attn_temporal_local(q, k, v, clips, T, HW, heads, head_dim=D, local=(r, 0))
    got = ops.attn_temporal_window(q, k, v, clips, T, HW, heads, head_dim=D, Tq=T, local=(r, 0), q_frame0=0, band_frame0=0)
    assert torch.equal(got, ref), (D, T, r)
    assert torch.equal(ops.attn_temporal_window(q, k, v, clips, T, HW, heads, head_dim=D, local=(r, 0)), ref)     # Tq=None: S


# ---- 3. equality (b): row i = row i of the key-mask kernel under the mask {s : i sees s} -------------------------------------------
ROW_CASES = [(64, 24, 4, 4, 1, 0), (64, 37, 4, 9, 2, 3), (64, 33, 2, 0, 0, 1), (64, 128, 3, 16, 33, 0), (64, 128, 3, 16, 33, 1), (64, 96, 3, 32, 32, 1),
             (64, 250, 4, 32, 0, 2), (128, 66, 2, 31, 33, 0), (128, 130, 2, 12, 2, 1)]


def _masked_long(q, k, v, clips, Tq, S, heads, D, mask):
    """mofa_attn_temporal_long_masked_f16 itself (``ops.attn_temporal_sharded`` sends up to 32 slots to the 32-key kernel)"""
    import ctypes
    from mofa_video_amd import lib as L
    out = torch.empty(clips * Tq * HW, heads * D, dtype=torch.float16, device=DEV)
    words = (ctypes.c_uint32 * 4)(*[(mask >> (32 * w)) & 0xffffffff for w in range(4)])
    L.check(L.load().mofa_attn_temporal_long_masked_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), clips, Tq, S, HW, heads, D,
                                                        q.stride(0), k.stride(0), out.stride(0), D ** -0.5, words, L.stream_ptr()),
            "mofa_attn_temporal_long_masked_f16")
    return out


@pytest.mark.parametrize("case", ROW_CASES)
def test_rows_equal_the_key_mask_kernel(ops, case):
    assert case in wc.CASES
    D, T, n, r, a, s = case
    d = wc.window_data(*case)
    g = d.g
    q, k, v = d.q.to(DEV), d.k.to(DEV), d.v.to(DEV)
    rows = lambda t: t.reshape(d.clips, g.Tq, -1)                        # noqa: E731
    win = rows(_run(ops, d, D))
    vis = wc.slot_visible(g, r, a)
    differ = []
    for i in range(g.Tq):
        mask = sum(1 << j for j in range(g.S) if vis[i, j])
        if not torch.equal(rows(_masked_long(q, k, v, d.clips, g.Tq, g.S, d.heads, D, mask))[:, i], win[:, i]):
            differ.append(i)
    assert not differ, f"{case}: rows {differ} differ from the key-mask kernel"


# ---- 4. what must have no influence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(64, 24, 4, 4, 1, 0), (64, 37, 4, 9, 2, 0), (64, 128, 3, 16, 33, 0), (64, 128, 3, 16, 33, 1), (64, 96, 3, 32, 32, 0),
                                  (128, 66, 2, 31, 33, 0)])
def test_duplicate_band_slots_have_no_influence(ops, case):
    """the band slots that repeat an anchor frame overwritten with +-6e4 (finite) in K and V: every output bit stays"""
    D, T, n, r, a, s = case
    d = wc.window_data(*case)
    g = d.g
    dup = [a + (f - g.b0) for f in range(g.b0, min(a, g.b1))]
    assert dup
    base = _run(ops, d, D)
    k2, v2 = d.k.clone(), d.v.clone()
    sign = torch.where(torch.arange(d.heads * D) % 2 == 0, 6e4, -6e4).half()
    for t in (k2, v2):
        t.reshape(d.clips, g.S, HW, -1)[:, dup] = sign
    pert = ops.attn_temporal_window(d.q.to(DEV), k2.to(DEV), v2.to(DEV), d.clips, g.S, HW, d.heads, head_dim=D, **d.kw)
    assert bool(torch.isfinite(pert.float()).all()) and torch.equal(pert, base), case
    # ... while an anchor slot itself matters
    k3 = d.k.clone()
    k3.reshape(d.clips, g.S, HW, -1)[:, 0] = sign * 1e-4
    moved = ops.attn_temporal_window(d.q.to(DEV), k3.to(DEV), d.v.to(DEV), d.clips, g.S, HW, d.heads, head_dim=D, **d.kw)
    assert not torch.equal(moved, base)


@pytest.mark.parametrize("case", [(64, 25, 4, 6, 1, 1), (64, 128, 4, 31, 1, 2), (64, 256, 4, 31, 1, 3), (128, 130, 2, 12, 2, 0)])
def test_query_rows_beyond_tq_and_guard_rows(ops, case):
    """one clip whose q and out buffers hold rows beyond Tq (and guard rows and columns round ``out``): q rows >= Tq hold +-6e4
    or NaN and are not read, nothing outside the Tq * HW output rows is written, and the output is the plain call's bit for bit"""
    D, T, n, r, a, s = case
    clips = 1
    g = wc.geometry(T, n, r, a, s)
    qa, ka, va = wc.operands(D, T, clips)
    P = lc.ac._pack_temporal
    q, k, v = P(qa[..., g.f0:g.f1, :]).to(DEV), P(wc.slot_rows(ka, g, a)).to(DEV), P(wc.slot_rows(va, g, a)).to(DEV)
    kw = dict(Tq=g.Tq, local=(r, a), q_frame0=g.f0, band_frame0=g.b0)
    Cc, rows = lc.HEADS[D] * D, g.Tq * HW
    base = ops.attn_temporal_window(q, k, v, clips, g.S, HW, lc.HEADS[D], head_dim=D, **kw)
    for fill in (6e4, float("nan")):
        qbig = torch.full((rows + 3 * HW, Cc), fill, dtype=torch.float16, device=DEV)
        qbig[:rows] = q
        buf = torch.full((rows + 3 * HW + 5, Cc + 24), float("nan"), dtype=torch.float16, device=DEV)
        inside = torch.zeros_like(buf, dtype=torch.bool)
        inside[3:3 + rows, 8:8 + Cc] = True
        out = buf[3:3 + rows, 8:8 + Cc]
        ret = ops.attn_temporal_window(qbig, k, v, clips, g.S, HW, lc.HEADS[D], head_dim=D, out=out, **kw)
        assert ret is out and torch.equal(out, base), (case, fill)
        assert bool(torch.isnan(buf[~inside]).all()), (case, fill, "wrote outside the Tq * HW rows of the out view")


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_rejections_through_lib_check(ops):
    from mofa_video_amd.lib import MofaHipError
    q = torch.randn(27 * 3, 64, device=DEV).half()
    good = dict(Tq=10, local=(8, 1), q_frame0=20, band_frame0=12)
    for bad in (dict(Tq=0), dict(Tq=27), dict(local=(-1, 1)), dict(local=(8, 28)), dict(local=(8, -1)), dict(band_frame0=-1), dict(q_frame0=11),
                dict(q_frame0=29), dict(head_dim=32)):
        with pytest.raises(MofaHipError, match=r"mofa_attn_temporal_long_window_f16 failed with code -22$"):
            ops.attn_temporal_window(q, q, q, 1, 27, 3, 1, **dict(good, **bad))
    with pytest.raises(ValueError, match="is required"):
        ops.attn_temporal_window(q, q, q, 1, 27, 3, 1, Tq=10, q_frame0=20, band_frame0=12)
    out = ops.attn_temporal_window(q[:30], q, q, 1, 27, 3, 1, **dict(good, local=(1000, 1)))              # radius above 127: clamped, "all"
    assert bool(torch.isfinite(out).all())


# ---- 6. virtual ranks -------------------------------------------------------------------------------------------------------------
def _threads(world, fn):
    """fn(rank, ThreadWorld) on ``world`` threads -> the results in rank order"""
    from mofa_video_amd.parallel import ThreadWorld
    tw = ThreadWorld(world)
    results, errors = [None] * world, []

    def worker(r):
        try:
            torch.cuda.set_device(0)
            results[r] = fn(r, tw)
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))
            for b in tw.barriers.values():
                b.abort()
    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors, errors
    return results


@pytest.mark.parametrize("T,world,radius,anchor", [(128, 4, 31, 1), (66, 2, 31, 33)])
@pytest.mark.parametrize("hd", (64, 128))
def test_windowed_sharded_temporal_block(hd, T, world, radius, anchor):
    """one TransformerSpatioTemporal block under the window on frames-only shards against the same windowed block on the whole
    clip; the p2p exchange and the conservative one give the same bits; one "window" exchange per layer, no token gather"""
    from mofa_video_amd import ops
    from mofa_video_amd.parallel import FrameParallel, Layout, ThreadComm
    blk = sc.make_block(hd, DEV)
    x, emb = sc.block_inputs(blk, T, DEV)
    HWb = sc.H * sc.W
    ref = ws.run_block(blk, x, emb, T, (radius, anchor)).reshape(T, HWb * blk.C)
    calls = []
    inner = ws.spy_on_window_attention(calls)
    try:
        def rank(r, tw):
            lay = Layout(world, r, T, cfg_ranks=1)
            par = FrameParallel(lay, ThreadComm(tw, r), window_keys=True)
            report = par.self_check(DEV)
            assert report["window"] == "batched p2p + anchor broadcast", report
            par.log = []
            mine = x[lay.f0 * HWb:lay.f1 * HWb]
            fast = ws.run_block(blk, mine, emb, lay.T_loc, (radius, anchor), par)
            par.window_p2p = False
            slow = ws.run_block(blk, mine, emb, lay.T_loc, (radius, anchor), par)
            assert par.log == [(0, "window")] * 2, par.log
            return lay, fast, slow
        outs = _threads(world, rank)
    finally:
        ops.attn_temporal_window = inner
    assert sorted(calls) == sorted([ws.expected_call(T, world, radius, anchor, r) for r in range(world)] * 2), calls
    for r, (lay, fast, slow) in enumerate(outs):
        assert torch.equal(fast, slow), (r, "the conservative exchange gives other bits")
        o, want = fast.reshape(lay.T_loc, HWb * blk.C), ref[lay.f0:lay.f1]
        e = rel_l2(o, want)
        print(f"ATTN-WINDOW block {T} frames over {world} shards, window ({radius}, {anchor}), head dim {hd}, rank {r}: rel-L2 {e:.3e}")
        assert e < 2e-3, (r, e)
        check_frames(o, want, 2e-3, ABS, dim=0, f0=lay.f0, what=f"ATTN-WINDOW block rank {r}")


H = W = 64
STEPS = 2


@pytest.fixture(scope="module")
def tiny():
    from mofa_video_amd.adapter import FlowControlNet
    from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
    _, _, _, sdu, sdc, _ = oracle_models(TINY, seed=0, cn_cfg=TINY_CN)
    return dict(unet=UNetSpatioTemporalConditionControlNetModel(sdu, TINY, DEV), controlnet=FlowControlNet(sdc, TINY_CN, DEV))


def _latents(mods, inp, T, window, limit, parallel=None):
    from mofa_video_amd.pipeline import FlowControlNetPipeline
    from mofa_video_amd.scheduler import EulerDiscreteScheduler
    pipe = FlowControlNetPipeline(**mods, scheduler=EulerDiscreteScheduler(), parallel=parallel, max_temporal_frames=limit,
                                  temporal_window=window)
    return pipe(None, controlnet_condition=inp["cond"], controlnet_flow=inp["flow"], height=H, width=W, num_frames=T,
                num_inference_steps=STEPS, latents=inp["latents"], output_type="latent", image_embeddings=inp["image_embeddings"],
                image_latents=inp["image_latents"]).frames


@pytest.mark.parametrize("T,world,window,limit", [(40, 4, (8, 1), 64), (130, 4, (12, 2), 256)])
def test_windowed_sharded_clip_equals_single_rank(tiny, T, world, window, limit):
    """the flow pipeline on tiny models, 2 CFG halves x 2 frame shards on virtual ranks, against the single-rank windowed
    pipeline: 40 frames under (8, 1) -- refused with "no per-query mask" without ``window_keys`` -- and 130 frames under (12, 2),
    more than every limit of the gathered path (128 key slots) allows"""
    from mofa_video_amd.parallel import FrameParallel, Layout, ThreadComm, ThreadWorld
    inp = synthetic_inputs(T, H, W, cross_dim=TINY["cross_attention_dim"], seed=52)
    with pytest.raises(ValueError, match="no per-query mask"):
        _latents(tiny, inp, T, window, limit, FrameParallel(Layout(world, 0, T), ThreadComm(ThreadWorld(world), 0), max_key_slots=128))
    ref = _latents(tiny, inp, T, window, limit)
    assert bool(torch.isfinite(ref).all())
    outs = _threads(world, lambda r, tw: _latents(tiny, inp, T, window, limit,
                                                  FrameParallel(Layout(world, r, T), ThreadComm(tw, r), window_keys=True)))
    for r, o in enumerate(outs):
        e = rel_l2(o, ref)
        print(f"ATTN-WINDOW world {world}, {T} frames, window {window}, rank {r}: latents rel-L2 vs single rank {e:.3e}")
        assert tuple(o.shape) == tuple(ref.shape)
        assert e < 2e-3, (world, r, e)
        check_frames(o, ref, 2e-3, ABS, what=f"ATTN-WINDOW world {world}, {T} frames, rank {r} vs single rank")
