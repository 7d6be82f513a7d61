"""Frame-sharded clips of 33 to 128 frames on the GPU: mofa_attn_temporal_long_masked_f16 (csrc/attention.hip
attn_temporal_long_masked_kernel) through ``ops.attn_temporal_sharded`` on the masked case table of
tests/attn_long_masked_cases.py (the same cases tests/test_sharded_long_cpu.py takes through the stand-in); dead slots are not
read; bit identity with the shipped long kernel; and the whole sharded path on virtual ranks (``parallel.ThreadComm``: N ranks as
N threads on one GPU, the layout, exchanges and kernels of the RCCL path) against the single-rank long path and the CPU oracle.

Virtual ranks against the single rank: rel-L2 <= 2e-3 tensor-wide and for every frame (tests/test_sharded_gpu.py's bound, for its
reason: identical arithmetic except the summation order of the temporal GroupNorm statistics), and max|delta| / max|ref| of every
frame below ``ABS``.  Measured on one MI355X (identical on every rank):
  40 frames on world 4 (slot j = frame j: the attention's bits are the single rank's): tensor-wide 2.4e-6, per-frame rel-L2 at most
     7.9e-6, max-abs / max|ref| at most 5.5e-5 (frame 26);
  37 frames on world 8 (10 + 9 + 9 + 9: the frames behind a padding slot sit one, two, three slots further on than in the unsharded
     clip, so the kernel sums their keys in another fp32 order and last fp16 bits flip, which two steps of the network then spread):
     tensor-wide 8.5e-4, per-frame rel-L2 at most 9.4e-4 (frame 33), max-abs / max|ref| at most 1.161e-3 (frame 35);
  one block, 128 frames over 3 shards (compaction: frame order restored): 0, bit-identical, at both head dims;
  one block, 37 frames over 4 shards in place: rel-L2 at most 2.1e-5 tensor-wide, 5.7e-5 per frame, max-abs at most 5.4e-4.
``ABS`` = 3 x the worst of these (1.161e-3).  Against the CPU oracle, 40 frames on world 4: latents 1.04e-3 / worst frame 1.13e-3,
decoded frames 2.60e-3 / 3.93e-3 -- the single-rank long path's figures (tests/test_long_clip_e2e_gpu.py)"""
import threading

import pytest
import torch

import attn_long_masked_cases as mc
import sharded_long_checks as sc
from helpers import TINY, TINY_CN, TINY_VAE, check_frames, frame_errors, oracle_models, rel_l2, synthetic_inputs
from op_cases import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = W = 128
STEPS, CHUNK = 2, 8
ABS = 3.5e-3               # per-frame max|delta| / max|ref| vs single rank (measured <= 1.161e-3)
BAR = 2e-2                 # against the CPU oracle: the project's stated bound (tests/test_model_gpu.py)


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    mc.release()


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", mc.MASKED_T)
@pytest.mark.parametrize("hd", mc.LONG_HD)
def test_masked_case_table(ops, hd, T):
    """every (Tq, mask kind, geometry) of the table: "gauss" against fp64 at TOL["attn_temporal"], the exact families by
    equality, "count-one" to one fp16 ulp of 1 / L; guards intact"""
    top, bad, n = {f: 0.0 for f in mc.FORMS}, [], 0
    for case in mc.cases_of(T, hd):
        worst, errs = mc.check_masked(case, mc.run(ops, case, DEV))
        top[case.form], bad, n = max(top[case.form], worst), bad + errs, n + 1
    print(f"ATTN-LONG-MASKED hd{hd} T{T}: {n} cases; gauss worst err / bound {top['gauss']:.3f}; count-one worst {top['count-one']:.3f} fp16 ulp; "
          + ("select and count-c equal by value" if not bad else "FAILURES"))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("T", (33, 65, 128))
@pytest.mark.parametrize("hd", mc.LONG_HD)
def test_dead_slots_are_not_read(ops, hd, T):
    """the K / V rows of dead slots hold winning keys (8 q) with NaN values, or ordinary data: the output is the same bit for
    bit, within tolerance of fp64, and every guard row and column is intact"""
    HW, heads, clips = mc.LONG_GEOM[1]
    for kind in ("lay3", "lay4", "tile-dead", "alt", "first"):
        for Tq in (20, T):
            outs = []
            for fill in ("decoy-nan", "plain"):
                case = mc.masked_case("gauss", T, Tq, kind, hd, HW, heads, clips, fill)
                r = mc.run(ops, case, DEV)
                worst, errs = mc.check_masked(case, r)
                assert not errs, errs
                outs.append(r.placed["out"].t.clone())
            assert same_bits(outs[0], outs[1]), f"hd{hd} T{T} Tq{Tq} {kind}: the output depends on the rows of dead slots"


def _randn16(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV).half()


@pytest.mark.parametrize("T", (33, 64, 97, 128))
@pytest.mark.parametrize("hd", mc.LONG_HD)
def test_bit_identical_with_the_long_kernel(ops, hd, T):
    """every slot live and Tq = T: the bits of mofa_attn_temporal_long_f16, with no mask and with a full one; q = the frames
    [a, b) of the clip: the rows [a, b) of that output (a query's arithmetic does not depend on its block-mates); a repeat
    launch gives the same bits"""
    HW, heads, clips = 37, 3, 2
    Cc = heads * hd
    q, k, v = (_randn16(clips * T * HW, Cc, seed=s) for s in (1, 2, 3))
    ref = ops.attn_temporal(q, k, v, clips, T, HW, heads, head_dim=hd)
    for mask in (None, (1 << T) - 1, (1 << 128) - 1):
        got = ops.attn_temporal_sharded(q, k, v, clips, T, HW, heads, head_dim=hd, Tq=T, key_mask=mask)
        assert torch.equal(got, ref), f"hd{hd} T{T} mask {mask}: differs from the long kernel"
    ref5 = ref.reshape(clips, T, HW, Cc)
    for a, b in ((0, 1), (0, T // 2), (T // 2, T), (T // 4, min(T // 4 + 33, T)), (T - 1, T), (T - 32, T)):
        qs = q.reshape(clips, T, HW, Cc)[:, a:b].reshape(-1, Cc).contiguous()
        first = ops.attn_temporal_sharded(qs, k, v, clips, T, HW, heads, head_dim=hd, Tq=b - a)
        assert torch.equal(first.reshape(clips, b - a, HW, Cc), ref5[:, a:b]), f"hd{hd} T{T}: frames [{a}, {b}) differ"
        again = ops.attn_temporal_sharded(qs, k, v, clips, T, HW, heads, head_dim=hd, Tq=b - a)
        assert torch.equal(again, first), f"hd{hd} T{T} frames [{a}, {b}): the repeat launch differs"


@pytest.mark.parametrize("hd", mc.LONG_HD)
def test_up_to_32_slots_are_attn_temporal(ops, hd):
    HW, heads, clips = 11, 2, 2
    for T, Tq, mask in ((32, 32, None), (32, 8, 0xfffffffe), (25, 7, 0x1555555), (24, 6, (1 << 24) - 1 - (1 << 5) - (1 << 23))):
        q = _randn16(clips * Tq * HW, heads * hd, seed=4)
        k, v = (_randn16(clips * T * HW, heads * hd, seed=s) for s in (5, 6))
        a = ops.attn_temporal(q, k, v, clips, T, HW, heads, head_dim=hd, Tq=Tq, key_mask=mask)
        b = ops.attn_temporal_sharded(q, k, v, clips, T, HW, heads, head_dim=hd, Tq=Tq, key_mask=mask)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (hd, T, Tq, mask)


def test_rejections_through_lib_check(ops):
    from mofa_video_amd.lib import MofaHipError
    q = _randn16(40 * 3, 64, seed=5)
    for kw in (dict(Tq=41), dict(Tq=0), dict(key_mask=0), dict(key_mask=1 << 40), dict(head_dim=32)):
        with pytest.raises(MofaHipError, match=r"mofa_attn_temporal_long_masked_f16 failed with code -22$"):
            ops.attn_temporal_sharded(q, q, q, 1, 40, 3, 1, **kw)
    with pytest.raises(ValueError, match="frame-sharded clips are limited to 32 key slots"):
        ops.attn_temporal(q, q, q, 1, 40, 3, 1, key_mask=1)


# ---- virtual ranks ----------------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def tiny():
    from mofa_video_amd.adapter import FlowControlNet
    from mofa_video_amd.scheduler import EulerDiscreteScheduler
    from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
    from mofa_video_amd.vae import AutoencoderKLTemporalDecoder
    ou, oc, ov, sdu, sdc, sdv = oracle_models(TINY, seed=0, vae_cfg=TINY_VAE, cn_cfg=TINY_CN)
    mods = dict(vae=AutoencoderKLTemporalDecoder(sdv, TINY_VAE, DEV), unet=UNetSpatioTemporalConditionControlNetModel(sdu, TINY, DEV),
                controlnet=FlowControlNet(sdc, TINY_CN, DEV))
    return mods, (ou, oc, ov)


def _latents(mods, inp, T, parallel=None):
    from mofa_video_amd.pipeline import FlowControlNetPipeline
    from mofa_video_amd.scheduler import EulerDiscreteScheduler
    pipe = FlowControlNetPipeline(**mods, scheduler=EulerDiscreteScheduler(), parallel=parallel, max_temporal_frames=64)
    return pipe(None, controlnet_condition=inp["cond"], controlnet_flow=inp["flow"], height=H, width=W, num_frames=T,
                num_inference_steps=STEPS, decode_chunk_size=CHUNK, latents=inp["latents"], output_type="latent",
                image_embeddings=inp["image_embeddings"], image_latents=inp["image_latents"]).frames


def _sharded_latents(mods, inp, T, world):
    from mofa_video_amd.parallel import FrameParallel, Layout, ThreadComm
    return _threads(world, lambda r, tw: _latents(mods, inp, T, FrameParallel(Layout(world, r, T), ThreadComm(tw, r), max_key_slots=64)))


@pytest.mark.parametrize("world,T", [(4, 40), (8, 37)])
def test_sharded_long_clip_equals_single_rank(tiny, world, T):
    """40 frames as 2 CFG halves x 2 shards of 20 (40 key slots, every one live); 37 frames as 2 x 4 shards of 10 + 9 + 9 + 9 (40
    slots, three of them padding the allocator left as they were): every rank's latents against the single-rank long path"""
    mods, _ = tiny
    inp = synthetic_inputs(T, H, W, cross_dim=TINY["cross_attention_dim"], seed=52)
    ref = _latents(mods, inp, T)
    for r, o in enumerate(_sharded_latents(mods, inp, T, world)):
        e = rel_l2(o, ref)
        print(f"SHARDED-LONG world {world}, {T} frames, rank {r}: latents rel-L2 vs single rank {e:.3e}")
        assert tuple(o.shape) == tuple(ref.shape)
        assert e < 2e-3, (world, r, e)
        check_frames(o, ref, 2e-3, ABS, what=f"SHARDED-LONG world {world}, {T} frames, rank {r} vs single rank")


def test_sharded_long_clip_refused_at_the_default_limits(tiny):
    from mofa_video_amd.parallel import FrameParallel, Layout, ThreadComm, ThreadWorld
    from mofa_video_amd.pipeline import FlowControlNetPipeline
    from mofa_video_amd.scheduler import EulerDiscreteScheduler
    mods, _ = tiny
    inp = synthetic_inputs(40, H, W, cross_dim=TINY["cross_attention_dim"], seed=52)
    par = FrameParallel(Layout(4, 0, 40), ThreadComm(ThreadWorld(4), 0))
    pipe = FlowControlNetPipeline(**mods, scheduler=EulerDiscreteScheduler(), parallel=par, max_temporal_frames=64)
    with pytest.raises(ValueError, match="sharded over ranks are limited to 32 frames"):
        pipe(None, controlnet_condition=inp["cond"], controlnet_flow=inp["flow"], height=H, width=W, num_frames=40,
             num_inference_steps=STEPS, latents=inp["latents"], output_type="latent", image_embeddings=inp["image_embeddings"],
             image_latents=inp["image_latents"])


@pytest.mark.parametrize("world,T,hd,slots", [(3, 128, 64, 128), (3, 128, 128, 128), (4, 37, 128, 64)])
def test_sharded_long_temporal_block(world, T, hd, slots):
    """one TransformerSpatioTemporal block on frames-only shards against the block on the whole clip: 128 frames as 43 + 43 + 42
    (129 padded slots: the block compacts to 128 frames, Tq = T_loc, no mask) at both head dims, and 10 + 9 + 9 + 9 in place"""
    from mofa_video_amd import ops
    from mofa_video_amd.parallel import FrameParallel, Layout, ThreadComm
    blk = sc.make_block(hd, DEV)
    x, emb = sc.block_inputs(blk, T, DEV)
    HW = sc.H * sc.W
    ref = sc.run_block(blk, x, emb, T).reshape(T, HW * blk.C)
    calls = []
    inner = sc.spy_on_sharded_attention(calls)
    try:
        def rank(r, tw):
            lay = Layout(world, r, T, cfg_ranks=1)
            par = FrameParallel(lay, ThreadComm(tw, r), max_key_slots=slots)
            return lay, sc.run_block(blk, x[lay.f0 * HW:lay.f1 * HW], emb, lay.T_loc, par)
        outs = _threads(world, rank)
    finally:
        ops.attn_temporal_sharded = inner
    assert sorted(calls, key=repr) == sorted((sc.expected_call(lay, slots) for lay, _ in outs), key=repr), calls
    for r, (lay, o) in enumerate(outs):
        o, want = o.reshape(lay.T_loc, HW * blk.C), ref[lay.f0:lay.f1]
        e = rel_l2(o, want)
        print(f"SHARDED-LONG block {T} frames over {world} shards, head dim {hd}, rank {r}: rel-L2 {e:.3e}")
        assert e < 2e-3, (r, e)
        check_frames(o, want, 2e-3, ABS, dim=0, f0=lay.f0, what=f"SHARDED-LONG block rank {r}")


def test_sharded_long_clip_vs_oracle(tiny):
    """40 frames on world 4 against the fp32 CPU oracle: latents and decoded frames, tensor-wide and worst single frame"""
    from mofa_video_amd.vae import decode_latents
    from oracle.pipeline import denoise
    from oracle.scheduler import EulerDiscreteScheduler as OSch
    from oracle.vae import decode_latents as odecode
    mods, (ou, oc, ov) = tiny
    T, world = 40, 4
    inp = synthetic_inputs(T, H, W, cross_dim=TINY["cross_attention_dim"], seed=52)
    with torch.no_grad():
        ref_lat = denoise(ou, oc, OSch(), inp["latents"], inp["image_latents"], inp["image_embeddings"], inp["cond"], inp["flow"],
                          num_inference_steps=STEPS)
        ref_frames = odecode(ov, ref_lat, T, decode_chunk_size=CHUNK)
    for r, lat in enumerate(_sharded_latents(mods, inp, T, world)):
        if r not in (0, world - 1):
            continue
        frames = decode_latents(mods["vae"], lat, T, CHUNK)
        el, ef = frame_errors(lat, ref_lat, dim=1), frame_errors(frames, ref_frames, dim=2)
        print(f"SHARDED-LONG world {world}, {T} frames, rank {r} vs oracle: latents rel-L2 {el.tensor:.3e}, worst frame {max(el.rel):.3e} "
              f"(frame {el.worst_rel}); decoded frames rel-L2 {ef.tensor:.3e}, worst frame {max(ef.rel):.3e} (frame {ef.worst_rel})")
        assert tuple(lat.shape) == tuple(ref_lat.shape) and tuple(frames.shape) == tuple(ref_frames.shape)
        assert el.tensor < BAR and max(el.rel) < BAR, el.summary()
        assert ef.tensor < BAR and max(ef.rel) < BAR, ef.summary()
