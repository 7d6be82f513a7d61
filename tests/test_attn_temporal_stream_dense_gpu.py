"""mofa_attn_temporal_stream_f16 (csrc/attention.hip attn_temporal_stream_kernel): temporal attention over up to 1024 frames under
any window of the local rule "query frame i sees key frame j iff j < anchor or |i - j| <= radius", dense included -- an
online-softmax walk over the key tiles the rule makes visible -- driven through ``ops.attn_temporal_stream`` on the cases of
tests/attn_stream_dense_cases.py (tests/test_attn_stream_dense_cases_cpu.py proves the table on the CPU).  Shapes are tiny on
purpose: HW = 5, heads 2 (head_dim 64) / 1 (head_dim 128), 1 or 2 clips, and ``attn_long_cases.LONG_GEOM`` for the exact families.

Against float64 under the dense kernel's bound; the exact families of the long kernel past 128 frames; the three spellings of
"nothing hidden" bit-equal and seven launches bit-identical; invisible frames without any influence (skipped tile, hidden part of
a visited tile, the all-hidden first tile, an anchor tile beyond tile 0); packed q|k|v with guarded output; the refusals; the
plumbing through the UNet, the ControlNet and the pipeline (eager and captured); and a dense 130-frame run against the fp32
oracle."""
import pytest
import torch

import attn_long_cases as lg
import attn_stream_dense_cases as dc
from helpers import TINY, TINY_CN, TINY_VAE, frame_errors, oracle_models, synthetic_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
HW = dc.HW
NAME = "mofa_attn_temporal_stream_f16"


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    dc.release()
    lg.release()


def _dev(d):
    return d.q.to(DEV), d.k.to(DEV), d.v.to(DEV)


# ---- (a) every table case against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T", sorted({(c[0], c[1]) for c in dc.CASES}))
def test_table_cases_against_fp64(ops, D, T):
    bad = []
    for _, _, r, a in [c for c in dc.CASES if c[:2] == (D, T)]:
        d = dc.dense_data(D, T, r, a)
        q, k, v = _dev(d)
        out = ops.attn_temporal_stream(q, k, v, d.clips, T, HW, d.heads, head_dim=D, local=dc.local_of(r, a)).cpu()
        assert bool(torch.isfinite(out.float()).all()), (D, T, r, a)
        worst, msg = dc.close_errors(out, d.expect, dc.BOUND, f"hd{D} T{T} radius {r} anchor {a} clips {d.clips}")
        print(f"ATTN-STREAM-DENSE hd{D} T{T} radius {r} anchor {a}: worst err / bound {worst:.3f}")
        bad += [msg] if msg is not None else []
    assert not bad, (len(bad), bad[:4])


# ---- (b) the exact families of the long kernel, past 128 frames -------------------------------------------------------------------
EXACT_T = (129, 161, 257, 1024)


@pytest.mark.parametrize("T", EXACT_T)
@pytest.mark.parametrize("hd", (64, 128))
def test_exact_families(ops, hd, T):
    for HWg, heads, clips in lg.LONG_GEOM:
        run = lambda d: ops.attn_temporal_stream(d.q.to(DEV), d.k.to(DEV), d.v.to(DEV), clips, T, HWg, heads, head_dim=hd).cpu()
        what = f"hd{hd} T{T} hw{HWg} h{heads} c{clips}"
        for form in ("select", "count-c"):
            d = lg.long_data(form, T, hd, HWg, heads, clips)
            out = run(d)
            bad = ~(out == d.expect)
            assert not bool(bad.any()), f"{what} {form}: {int(bad.sum())} elements differ, first at " \
                                        f"{d.where(*torch.nonzero(bad)[0].tolist())}"
        out = run(lg.long_data("count-one", T, hd, HWg, heads, clips))
        err = (out.double() - 1.0 / T).abs().max().item() / lg.ulp16(1.0 / T)
        print(f"ATTN-STREAM-DENSE {what} count-one: {err:.2f} fp16 ulps from 1 / {T}")
        assert err <= 1.0, (what, err)
        if clips == 2:
            plain, decoy = (run(lg.long_data(f, T, hd, HWg, heads, 2))[:T * HWg] for f in ("phantom-plain", "phantom-decoy"))
            assert bool(torch.isfinite(decoy.float()).all()), f"{what}: clip 0 read clip 1's rows"
            assert torch.equal(plain, decoy), f"{what}: clip 0 depends on clip 1's rows"


# ---- (c) equal calls ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T", [(64, 129), (64, 161), (64, 256), (64, 1024), (64, 97), (128, 161), (128, 257)])
def test_spellings_of_dense_are_bit_equal_and_launches_repeat(ops, D, T):
    d = dc.dense_data(D, T, None, None)
    q, k, v = _dev(d)
    run = lambda local: ops.attn_temporal_stream(q, k, v, d.clips, T, HW, d.heads, head_dim=D, local=local)
    dense = run(None)
    assert torch.equal(dense, run((T - 1, 0))) and torch.equal(dense, run((0, T))) and torch.equal(dense, run((5 * T, T)))
    if T > 128:
        assert torch.equal(dense, ops.attn_temporal(q, k, v, d.clips, T, HW, d.heads, head_dim=D))   # the dense op's route past 128
    for local in (None, (48, 1)):
        first = run(local)
        for _ in range(6):
            assert torch.equal(run(local), first), f"launches differ under {local}"


# ---- (d) invisible frames have no influence ---------------------------------------------------------------------------------------
# (D, T, radius, anchor, j, where j lies for the rows that cannot see it)
NO_INFLUENCE = [
    (64, 257, 40, 0, 10, "skipped"),          # the blocks from query 96 on never visit tile 0
    (64, 257, 48, 1, 200, "skipped"),         # the blocks up to query 127 never visit tile 6
    (64, 257, 40, 0, 100, "hidden"),          # block 1 visits tile 3 for its queries 56 .. 63; frame 100 is hidden from 32 .. 59
    (64, 161, 100, 2, 140, "hidden"),         # block 0 visits tile 4 for frames 128 .. 131
    (64, 161, 15, 0, 40, "first"),            # block 2 starts at tile 1 for frames 49 .. 63: frame 40 hidden from all, the tile from 80 ..
    (64, 161, 1, 0, 63, "first"),             # block 2 starts at tile 1 for query 64 alone
    (64, 257, 31, 0, 97, "first"),            # block 4 starts at tile 3; all of it is hidden from query 159
    (64, 161, 12, 33, 32, "anchor"),          # anchor tile 1 holds one anchor, frame 32 ...
    (64, 161, 12, 33, 33, "anchor"),          # ... and frame 33 is hidden there
    (64, 257, 4, 128, 127, "anchor"),         # the last frame of the last of four anchor tiles
    (64, 257, 4, 128, 128, "skipped"),        # the first frame that is no anchor
    (64, 257, 33, 33, 40, "anchor"),
    (128, 257, 48, 1, 100, "hidden"),
    (128, 161, 16, 0, 70, "first"),
]


@pytest.mark.parametrize("D,T,r,a,j,where", NO_INFLUENCE)
def test_invisible_frame_has_no_influence(ops, D, T, r, a, j, where):
    """frame j's K and V rows overwritten with +-6e4 (finite): every row that cannot see j keeps its bits, rows that can move"""
    clips, heads = 2, dc.HEADS[D]
    q, k, v = (dc.ac._pack_temporal(t).to(DEV) for t in dc.operands(D, T, clips))
    run = lambda kk, vv: ops.attn_temporal_stream(q, kk, vv, clips, T, HW, heads, head_dim=D, local=(r, a)).reshape(clips, T, -1)
    sees = dc.visible(T, r, a)[:, j]
    # j lies where the case says, for some rows that cannot see it
    blind = [i for i in range(T) if not bool(sees[i])]
    walks = {i: dc.visited_tiles(T, i // 32 * 32, r, a) for i in blind}
    if where == "skipped":
        assert any(j // 32 not in w for w in walks.values())
    elif where == "hidden":
        assert any(j // 32 in w for w in walks.values())
    elif where == "first":
        assert a == 0 and any(w[0] == j // 32 for w in walks.values())
    else:
        assert where == "anchor" and 1 <= j // 32 < (a + 31) // 32 and (j < a) == (not blind)
    base = run(k, v)
    k2, v2 = k.clone(), v.clone()
    sign = torch.where(torch.arange(heads * D, device=DEV) % 2 == 0, 6e4, -6e4).half()
    for t in (k2, v2):
        t.reshape(clips, T, HW, -1)[:, j] = sign
    pert = run(k2, v2)
    sees = sees.to(DEV)
    assert bool(sees.any())
    if not bool(sees.all()):
        assert bool(torch.isfinite(pert[:, ~sees].float()).all())
        assert torch.equal(pert[:, ~sees], base[:, ~sees]), f"rows that cannot see frame {j} changed"
    moved = (pert[:, sees] != base[:, sees]).flatten(1).any(1)
    assert bool(moved.any()), f"no row that sees frame {j} changed"


# ---- (e) layout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T,r,a", [(64, 161, None, None), (64, 256, 48, 1), (128, 129, 40, 0), (64, 33, 12, 33), (64, 257, 31, 0)])
def test_packed_qkv_and_guarded_output(ops, D, T, r, a):
    d = dc.dense_data(D, T, r, a)
    local = dc.local_of(r, a)
    Cc, rows = d.heads * D, d.clips * T * HW
    qkv = torch.cat([d.q, d.k, d.v], 1).to(DEV)                        # one buffer: ld = ldkv = 3 heads D
    q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
    assert q.stride(0) == k.stride(0) == v.stride(0) == 3 * Cc
    buf = torch.full((rows + 5, Cc + 24), float("nan"), dtype=torch.float16, device=DEV)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[3:3 + rows, 8:8 + Cc] = True
    out = buf[3:3 + rows, 8:8 + Cc]
    assert out.stride(0) == Cc + 24 != q.stride(0)
    ret = ops.attn_temporal_stream(q, k, v, d.clips, T, HW, d.heads, head_dim=D, out=out, local=local)
    assert ret is out
    first = buf.clone()
    assert bool(torch.isnan(first[~inside]).all()), "wrote outside the out view"
    worst, msg = dc.close_errors(out.cpu(), d.expect, dc.BOUND, f"packed hd{D} T{T} radius {r} anchor {a}")
    assert msg is None, msg
    assert torch.equal(out, ops.attn_temporal_stream(*_dev(d), d.clips, T, HW, d.heads, head_dim=D, local=local)), \
        "the layout changed the bits"
    ops.attn_temporal_stream(q, k, v, d.clips, T, HW, d.heads, head_dim=D, out=out, local=local)
    assert torch.equal(buf[inside], first[inside]) and bool(torch.isnan(buf[~inside]).all()), "the second launch differs"


# ---- (f) refusals -----------------------------------------------------------------------------------------------------------------
def test_rejections_through_lib_check(ops):
    from mofa_video_amd import lib as L
    from mofa_video_amd.lib import MofaHipError
    l = L.load()
    t = torch.zeros(161 * 2, 160 + 16, dtype=torch.float16, device=DEV)
    p = t.data_ptr()

    def call(q=p, k=p, v=p, out=p, nclips=1, T=161, HW=1, heads=1, hd=64, ld=176, ldkv=176, ldo=176, radius=48, anchor=1):
        L.check(getattr(l, NAME)(q, k, v, out, nclips, T, HW, heads, hd, ld, ldkv, ldo, 0.125, radius, anchor, L.stream_ptr()), NAME)
    bads = [dict(radius=-1), dict(anchor=-1), dict(anchor=162), dict(T=16, anchor=17), dict(T=1025), dict(T=0), dict(hd=80), dict(ld=12),
            dict(ldkv=172), dict(ldo=0), dict(nclips=0), dict(HW=0), dict(heads=0), dict(q=None), dict(k=None), dict(v=None), dict(out=None)]
    for bad in bads:
        with pytest.raises(MofaHipError, match=NAME + r" failed with code -22$"):
            call(**bad)
    o2 = torch.empty_like(t).data_ptr()
    call(out=o2, radius=1 << 30, anchor=161)                           # no upper limit on the radius; anchor = T is valid
    call(out=o2, radius=0, anchor=0)
    torch.cuda.synchronize()
    q = torch.randn(161 * 3, 64, device=DEV).half()
    with pytest.raises(ValueError, match="no key_mask and no Tq"):
        ops.attn_temporal_stream(q, q, q, 1, 161, 3, 1, key_mask=1, local=(48, 1))
    with pytest.raises(ValueError, match="no per-query mask"):
        ops.attn_temporal_stream(q, q, q, 1, 161, 3, 1, Tq=20)
    with pytest.raises(MofaHipError, match="code -22"):
        ops.attn_temporal_stream(q, q, q, 1, 161, 3, 1, local=(-1, 1))
    with pytest.raises(MofaHipError, match="code -22"):
        ops.attn_temporal_stream(q, q, q, 1, 161, 3, 1, local=(48, 162))
    with pytest.raises(ValueError, match="key mask or Tq < T"):       # the dense op's sharded forms stay at 32 key slots
        ops.attn_temporal(q, q, q, 1, 161, 3, 1, Tq=20)


# ---- (g) plumbing -----------------------------------------------------------------------------------------------------------------
PT, PH, PW, PSTEPS = 161, 64, 64, 2


@pytest.fixture(scope="module")
def tiny():
    from mofa_video_amd.adapter import FlowControlNet
    from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
    _, _, _, sdu, sdc, _ = oracle_models(TINY, seed=0, cn_cfg=TINY_CN)
    hu, hc = UNetSpatioTemporalConditionControlNetModel(sdu, TINY, DEV), FlowControlNet(sdc, TINY_CN, DEV)
    inp = synthetic_inputs(PT, PH, PW, cross_dim=TINY["cross_attention_dim"], seed=61)
    done = {}

    def run(window, graph=False, fresh=False, stream=True):
        """the latents after PSTEPS steps of PT frames under ``window``, one run per (window, graph_steps, keyword) unless ``fresh``"""
        from mofa_video_amd.pipeline import FlowControlNetPipeline
        from mofa_video_amd.scheduler import EulerDiscreteScheduler
        key = (window, graph, stream)
        if fresh or key not in done:
            kw = dict(temporal_stream=True) if stream else {}
            pipe = FlowControlNetPipeline(unet=hu, controlnet=hc, scheduler=EulerDiscreteScheduler(), max_temporal_frames=192,
                                          temporal_window=window, **kw)
            pipe.graph_steps = graph
            done[key] = pipe(None, controlnet_condition=inp["cond"], controlnet_flow=inp["flow"], height=PH, width=PW,
                             num_frames=PT, num_inference_steps=PSTEPS, latents=inp["latents"], output_type="latent",
                             image_embeddings=inp["image_embeddings"], image_latents=inp["image_latents"]).frames
        return done[key]
    return hu, hc, run


def _temporal_blocks(net):
    """every TransformerSpatioTemporal instance reachable from ``net``"""
    from mofa_video_amd.blocks import TransformerSpatioTemporal
    found, seen, todo = [], set(), [net]
    while todo:
        o = todo.pop()
        if id(o) in seen or isinstance(o, (torch.Tensor, str, int, float, type(None))):
            continue
        seen.add(id(o))
        if isinstance(o, TransformerSpatioTemporal):
            found.append(o)
        if isinstance(o, (list, tuple)):
            todo += list(o)
        elif isinstance(o, dict):
            todo += list(o.values())
        elif hasattr(o, "__dict__") and type(o).__module__.startswith("mofa_video_amd"):
            todo += list(vars(o).values())
    return found


@pytest.mark.parametrize("window", (None, (48, 1)))
def test_161_frames_reach_the_new_entry_in_every_temporal_layer(tiny, monkeypatch, window):
    from mofa_video_amd import blocks
    from mofa_video_amd import ops as o
    hu, hc, run = tiny
    calls, inside = [], []
    real_stream, real_block = o.attn_temporal_stream, blocks.TransformerSpatioTemporal.__call__

    def spy_block(self, *a, **kw):
        inside.append(self)
        try:
            return real_block(self, *a, **kw)
        finally:
            inside.pop()

    def spy_stream(*a, **kw):
        calls.append((inside[-1] if inside else None, a[4], kw.get("local")))
        return real_stream(*a, **kw)

    def other(*a, **kw):
        raise AssertionError("a temporal attention call other than the streaming entry at 161 frames")
    monkeypatch.setattr(blocks.TransformerSpatioTemporal, "__call__", spy_block)
    monkeypatch.setattr(o, "attn_temporal_stream", spy_stream)
    monkeypatch.setattr(o, "attn_temporal_local_stream", other)
    monkeypatch.setattr(o, "attn_temporal_local", other)
    monkeypatch.setattr(o, "attn_temporal_sharded", other)
    lat = run(window, fresh=True)
    nu, nc = _temporal_blocks(hu), _temporal_blocks(hc)
    assert len(nu) == 16 and len(nc) == 7, (len(nu), len(nc))
    assert calls and all(blk is not None and T == PT and loc == window for blk, T, loc in calls), {c[1:] for c in calls}
    assert {id(b) for b, _, _ in calls} == {id(b) for b in nu + nc}      # every temporal layer of both networks, nothing else
    monkeypatch.undo()
    assert bool(torch.isfinite(lat).all())


@pytest.mark.parametrize("window", (None, (48, 1)))
def test_captured_steps_equal_eager_steps_at_161_frames(tiny, window):
    """graph_steps: only scalars enter the launch, so the step stays capturable and replays the eager bits"""
    _, _, run = tiny
    eager, graph = run(window), run(window, graph=True)
    assert bool(torch.isfinite(eager).all()) and torch.equal(eager, graph)


def test_ring_window_keeps_the_ring_op_under_the_keyword(tiny, monkeypatch):
    """(12, 1) is ring-eligible: with temporal_stream=True the ring op is still the one called, and the latents are those of a
    pipeline built without the keyword"""
    from mofa_video_amd import ops as o
    _, _, run = tiny
    usual = run((12, 1), stream=False)
    ring, real_ring = [], o.attn_temporal_local_stream
    monkeypatch.setattr(o, "attn_temporal_local_stream", lambda *a, **kw: ring.append(kw.get("local")) or real_ring(*a, **kw))
    monkeypatch.setattr(o, "attn_temporal_stream", lambda *a, **kw: pytest.fail("the new entry was called under a ring-eligible window"))
    with_kw = run((12, 1), fresh=True)
    assert ring and set(ring) == {(12, 1)}
    assert bool(torch.isfinite(usual).all()) and torch.equal(with_kw, usual)


# ---- (h) a dense 130-frame pass against the fp32 oracle ---------------------------------------------------------------------------
def test_dense_130_frames_vs_oracle():
    from mofa_video_amd.adapter import FlowControlNet
    from mofa_video_amd.pipeline import FlowControlNetPipeline
    from mofa_video_amd.scheduler import EulerDiscreteScheduler
    from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
    from mofa_video_amd.vae import AutoencoderKLTemporalDecoder, decode_latents
    from oracle.pipeline import denoise
    from oracle.scheduler import EulerDiscreteScheduler as OSch
    from oracle.vae import decode_latents as odecode
    T, H, W, STEPS, CHUNK, BAR = 130, 64, 64, 2, 8, 2e-2
    ou, oc, ov, sdu, sdc, sdv = oracle_models(TINY, seed=0, vae_cfg=TINY_VAE, cn_cfg=TINY_CN)
    mods = dict(vae=AutoencoderKLTemporalDecoder(sdv, TINY_VAE, DEV), unet=UNetSpatioTemporalConditionControlNetModel(sdu, TINY, DEV),
                controlnet=FlowControlNet(sdc, TINY_CN, DEV), scheduler=EulerDiscreteScheduler())
    inp = synthetic_inputs(T, H, W, cross_dim=TINY["cross_attention_dim"], seed=52)
    with torch.no_grad():
        ref_lat = denoise(ou, oc, OSch(), inp["latents"], inp["image_latents"], inp["image_embeddings"], inp["cond"], inp["flow"],
                          num_inference_steps=STEPS)
        ref_frames = odecode(ov, ref_lat, T, decode_chunk_size=CHUNK)
    kw = dict(controlnet_condition=inp["cond"], controlnet_flow=inp["flow"], height=H, width=W, num_frames=T,
              num_inference_steps=STEPS, decode_chunk_size=CHUNK, latents=inp["latents"], output_type="latent",
              image_embeddings=inp["image_embeddings"], image_latents=inp["image_latents"])
    with pytest.raises(ValueError, match="max_temporal_frames"):       # without the keyword a dense pass stops at 128
        FlowControlNetPipeline(**mods, max_temporal_frames=160)
    lat = FlowControlNetPipeline(**mods, temporal_stream=True, max_temporal_frames=160)(None, **kw).frames
    frames = decode_latents(mods["vae"], lat, T, CHUNK)
    el, ef = frame_errors(lat, ref_lat, dim=1), frame_errors(frames, ref_frames, dim=2)
    print(f"STREAM-DENSE e2e T={T}: latents rel-L2 {el.tensor:.3e}, worst frame {max(el.rel):.3e} (frame {el.worst_rel}); "
          f"decoded frames rel-L2 {ef.tensor:.3e}, worst frame {max(ef.rel):.3e} (frame {ef.worst_rel})")
    assert tuple(lat.shape) == tuple(ref_lat.shape) and tuple(frames.shape) == tuple(ref_frames.shape)
    assert el.tensor < BAR and max(el.rel) < BAR, el.summary()
    assert ef.tensor < BAR and max(ef.rel) < BAR, ef.summary()
