"""mofa_attn_temporal_stream_local_f16 (csrc/attention.hip attn_temporal_stream_local_kernel): the local rule "query frame i sees
key frame j iff j < anchor or |i - j| <= radius" for clips of up to 1024 frames, four key tiles in LDS (tile 0 and a ring of three),
driven through ``ops.attn_temporal_local_stream`` on the cases of tests/attn_stream_cases.py (tests/test_attn_stream_cases_cpu.py
proves the table on the CPU).  Shapes are tiny on purpose: HW = 5, heads 2 (head_dim 64) / 1 (head_dim 128), 1 or 2 clips.

Against float64 under the dense kernel's bound; bit-equal to the local kernel up to 128 frames; past 128 bit-equal, row by row, to
the key-mask kernel run on the block's four tiles; invisible frames without any influence (the reused ring slot included); packed
q|k|v with guarded output; the refusals; and the plumbing through the UNet, the ControlNet and the pipeline (eager and captured)."""
import pytest
import torch

import attn_stream_cases as sc
from helpers import TINY, TINY_CN, oracle_models, synthetic_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
HW = sc.HW


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    sc.release()


def _dev(d):
    return d.q.to(DEV), d.k.to(DEV), d.v.to(DEV)


# ---- 1. every table case against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T", sorted({(c[0], c[1]) for c in sc.CASES}))
def test_table_cases_against_fp64(ops, D, T):
    bad = []
    for _, _, r, a in [c for c in sc.CASES if c[:2] == (D, T)]:
        d = sc.local_data(D, T, r, a)
        q, k, v = _dev(d)
        out = ops.attn_temporal_local_stream(q, k, v, d.clips, T, HW, d.heads, head_dim=D, local=(r, a)).cpu()
        assert bool(torch.isfinite(out.float()).all()), (D, T, r, a)
        worst, msg = sc.close_errors(out, d.expect, sc.BOUND, f"hd{D} T{T} radius {r} anchor {a} clips {d.clips}")
        print(f"ATTN-STREAM hd{D} T{T} radius {r} anchor {a}: worst err / bound {worst:.3f}")
        bad += [msg] if msg is not None else []
    assert not bad, (len(bad), bad[:4])


# ---- 2. up to 128 frames: the local kernel's bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (64, 128))
def test_short_clips_equal_the_local_kernel(ops, D):
    """both kernels add the same nonzero terms in the same tile order, and exact zeros do not move an fp32 sum"""
    cases = [c for c in sc.CASES if c[0] == D and c[1] <= 128]
    assert len(cases) >= (60 if D == 64 else 6)
    for _, T, r, a in cases:
        d = sc.local_data(D, T, r, a)
        q, k, v = _dev(d)
        got = ops.attn_temporal_local_stream(q, k, v, d.clips, T, HW, d.heads, head_dim=D, local=(r, a))
        assert torch.equal(got, ops.attn_temporal_local(q, k, v, d.clips, T, HW, d.heads, head_dim=D, local=(r, a))), (D, T, r, a)


# ---- 3. past 128 frames: row i = the key-mask kernel on the block's four tiles --------------------------------------------------------
@pytest.mark.parametrize("D,T,r,a", [(64, 161, 12, 1), (64, 257, 32, 32), (64, 193, 0, 0), (128, 161, 16, 2)])
def test_rows_equal_the_key_mask_kernel_on_four_tiles(ops, D, T, r, a):
    """per query block tq (the first, a middle one, the last and partial one): a 128-slot K / V buffer holding the frame tiles
    [0, tq - 1, tq, tq + 1] -- a slot that is out of range, a second copy of tile 0 or a frame >= T holds NaN and has its mask bit
    clear -- the block's queries in rows 0 .. 31, and per row one call of mofa_attn_temporal_long_masked_f16 (Tq = T = 128) under
    that row's visibility"""
    clips, heads = 2, sc.HEADS[D]
    q, k, v = (sc.ac._pack_temporal(t).to(DEV) for t in sc.operands(D, T, clips))
    frames = lambda t, n: t.reshape(clips, n, HW, heads * D)
    got = frames(ops.attn_temporal_local_stream(q, k, v, clips, T, HW, heads, head_dim=D, local=(r, a)), T)
    vis = sc.visible(T, r, a)
    ntiles = (T + 31) // 32
    assert ntiles >= 5 and T % 32 != 0
    differ = []
    for tq in (0, ntiles // 2, ntiles - 1):
        tiles = [0, tq - 1, tq, tq + 1]
        frame_of = torch.full((128,), -1, dtype=torch.long)              # slot -> frame, -1 = a dead slot
        for s, t in enumerate(tiles):
            if s == 0 or 0 < t < ntiles:
                f = torch.arange(32 * t, 32 * t + 32)
                frame_of[32 * s:32 * s + 32] = torch.where(f < T, f, torch.full_like(f, -1))
        live = frame_of >= 0
        kb, vb = (torch.full((clips, 128, HW, heads * D), float("nan"), dtype=torch.float16, device=DEV) for _ in range(2))
        kb[:, live], vb[:, live] = frames(k, T)[:, frame_of[live]], frames(v, T)[:, frame_of[live]]
        nq = min(32, T - 32 * tq)
        qb = torch.zeros(clips, 128, HW, heads * D, dtype=torch.float16, device=DEV)
        qb[:, :nq] = frames(q, T)[:, 32 * tq:32 * tq + nq]
        qb, kb, vb = (t.reshape(clips * 128 * HW, heads * D) for t in (qb, kb, vb))
        for n in range(nq):
            i = 32 * tq + n
            sees = torch.nonzero(live & vis[i][frame_of.clamp(min=0)]).flatten().tolist()
            assert sorted(frame_of[sees].tolist()) == torch.nonzero(vis[i]).flatten().tolist()          # every key once
            masked = frames(ops.attn_temporal_sharded(qb, kb, vb, clips, 128, HW, heads, head_dim=D, Tq=128,
                                                      key_mask=sum(1 << s for s in sees)), 128)
            if not torch.equal(masked[:, n], got[:, i]):
                differ.append(i)
    assert not differ, f"hd{D} T{T} radius {r} anchor {a}: rows {differ} differ from the key-mask kernel"


# ---- 4. invisible frames have no influence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T,r,a,j", [(64, 161, 4, 1, 63), (64, 161, 4, 1, 64), (64, 161, 12, 2, 1), (64, 161, 12, 2, 2),
                                       (64, 161, 32, 32, 31), (64, 161, 32, 32, 32), (64, 257, 4, 1, 127), (64, 257, 4, 1, 128),
                                       (64, 257, 4, 1, 40), (128, 257, 16, 2, 160), (128, 161, 0, 0, 159)])
def test_invisible_frame_has_no_influence(ops, D, T, r, a, j):
    """frame j's K and V rows overwritten with +-6e4 (finite): every row that cannot see j keeps its bits, rows that can move.
    The queries three tiles past j read their band from the ring slot that held j's tile"""
    clips, heads = 2, sc.HEADS[D]
    q, k, v = (sc.ac._pack_temporal(t).to(DEV) for t in sc.operands(D, T, clips))
    run = lambda kk, vv: ops.attn_temporal_local_stream(q, kk, vv, clips, T, HW, heads, head_dim=D, local=(r, a)).reshape(clips, T, -1)
    base = run(k, v)
    k2, v2 = k.clone(), v.clone()
    sign = torch.where(torch.arange(heads * D, device=DEV) % 2 == 0, 6e4, -6e4).half()
    for t in (k2, v2):
        t.reshape(clips, T, HW, -1)[:, j] = sign
    pert = run(k2, v2)
    sees = sc.visible(T, r, a)[:, j].to(DEV)
    assert bool(sees.any()) and (a > j or not bool(sees.all()))
    if (D, T, j) == (64, 257, 40):
        reuse = torch.arange(T, device=DEV) // 32 == j // 32 + 3        # block 4 reads tile 4 from the slot tile 1 left
        assert bool(reuse.any()) and not bool((reuse & sees).any())
    assert bool(torch.isfinite(pert[:, ~sees].float()).all())
    assert torch.equal(pert[:, ~sees], base[:, ~sees]), f"rows that cannot see frame {j} changed"
    moved = (pert[:, sees] != base[:, sees]).flatten(1).any(1)
    assert bool(moved.any()), f"no row that sees frame {j} changed"


# ---- 5. layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T,r,a", [(64, 161, 15, 2), (64, 256, 32, 32), (128, 129, 16, 1), (64, 33, 1, 2)])
def test_packed_qkv_and_guarded_output(ops, D, T, r, a):
    d = sc.local_data(D, T, r, a)
    Cc, rows = d.heads * D, d.clips * T * HW
    qkv = torch.cat([d.q, d.k, d.v], 1).to(DEV)                        # one buffer: ld = ldkv = 3 heads D
    q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
    assert q.stride(0) == k.stride(0) == v.stride(0) == 3 * Cc
    buf = torch.full((rows + 5, Cc + 24), float("nan"), dtype=torch.float16, device=DEV)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[3:3 + rows, 8:8 + Cc] = True
    out = buf[3:3 + rows, 8:8 + Cc]
    assert out.stride(0) == Cc + 24 != q.stride(0)
    ret = ops.attn_temporal_local_stream(q, k, v, d.clips, T, HW, d.heads, head_dim=D, out=out, local=(r, a))
    assert ret is out
    first = buf.clone()
    assert bool(torch.isnan(first[~inside]).all()), "wrote outside the out view"
    worst, msg = sc.close_errors(out.cpu(), d.expect, sc.BOUND, f"packed hd{D} T{T} radius {r} anchor {a}")
    assert msg is None, msg
    assert torch.equal(out, ops.attn_temporal_local_stream(*_dev(d), d.clips, T, HW, d.heads, head_dim=D, local=(r, a))), \
        "the layout changed the bits"
    ops.attn_temporal_local_stream(q, k, v, d.clips, T, HW, d.heads, head_dim=D, out=out, local=(r, a))
    assert torch.equal(buf[inside], first[inside]) and bool(torch.isnan(buf[~inside]).all()), "the second launch differs"


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_rejections_through_lib_check(ops):
    from mofa_video_amd import lib as L
    from mofa_video_amd.lib import MofaHipError
    l = L.load()
    t = torch.zeros(161 * 2, 160 + 16, dtype=torch.float16, device=DEV)
    p = t.data_ptr()

    def call(q=p, k=p, v=p, out=p, nclips=1, T=161, HW=1, heads=1, hd=64, ld=176, ldkv=176, ldo=176, radius=4, anchor=1):
        L.check(l.mofa_attn_temporal_stream_local_f16(q, k, v, out, nclips, T, HW, heads, hd, ld, ldkv, ldo, 0.125, radius, anchor,
                                                      L.stream_ptr()), "mofa_attn_temporal_stream_local_f16")
    bads = [dict(radius=-1), dict(radius=33), dict(anchor=-1), dict(anchor=33), dict(T=16, anchor=17), dict(T=1025), dict(T=0), dict(hd=80),
            dict(ld=12), dict(ldkv=172), dict(ldo=0), dict(nclips=0), dict(HW=0), dict(heads=0), dict(q=None), dict(k=None), dict(v=None),
            dict(out=None)]
    for bad in bads:
        with pytest.raises(MofaHipError, match=r"mofa_attn_temporal_stream_local_f16 failed with code -22$"):
            call(**bad)
    call(out=torch.empty_like(t).data_ptr(), radius=32, anchor=32)                                  # both limits are valid
    torch.cuda.synchronize()
    q = torch.randn(161 * 3, 64, device=DEV).half()
    with pytest.raises(ValueError, match="no key_mask and no Tq"):
        ops.attn_temporal_local_stream(q, q, q, 1, 161, 3, 1, key_mask=1, local=(4, 1))
    with pytest.raises(ValueError, match="no per-query mask"):
        ops.attn_temporal_local_stream(q, q, q, 1, 161, 3, 1, Tq=20, local=(4, 1))
    with pytest.raises(ValueError, match="is required"):
        ops.attn_temporal_local_stream(q, q, q, 1, 161, 3, 1)
    with pytest.raises(MofaHipError, match="code -22"):
        ops.attn_temporal_local_stream(q, q, q, 1, 161, 3, 1, local=(33, 1))
    with pytest.raises(MofaHipError, match="code -22"):
        ops.attn_temporal_local(q, q, q, 1, 161, 3, 1, local=(4, 1))                                 # the local kernel keeps its 128


# ---- 7. plumbing ------------------------------------------------------------------------------------------------------------------
PT, PH, PW, PSTEPS, WINDOW = 161, 64, 64, 3, (12, 1)


@pytest.fixture(scope="module")
def tiny():
    from mofa_video_amd.adapter import FlowControlNet
    from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
    _, _, _, sdu, sdc, _ = oracle_models(TINY, seed=0, cn_cfg=TINY_CN)
    hu, hc = UNetSpatioTemporalConditionControlNetModel(sdu, TINY, DEV), FlowControlNet(sdc, TINY_CN, DEV)
    inputs, done = {}, {}

    def run(T, graph=False, fresh=False):
        """the latents after PSTEPS steps of T frames under WINDOW, one run per (T, graph_steps) unless ``fresh``"""
        from mofa_video_amd.pipeline import FlowControlNetPipeline
        from mofa_video_amd.scheduler import EulerDiscreteScheduler
        if fresh or (T, graph) not in done:
            if T not in inputs:
                inputs[T] = synthetic_inputs(T, PH, PW, cross_dim=TINY["cross_attention_dim"], seed=61)
            inp = inputs[T]
            pipe = FlowControlNetPipeline(unet=hu, controlnet=hc, scheduler=EulerDiscreteScheduler(), max_temporal_frames=192,
                                          temporal_window=WINDOW)
            pipe.graph_steps = graph
            done[(T, graph)] = pipe(None, controlnet_condition=inp["cond"], controlnet_flow=inp["flow"], height=PH, width=PW,
                                    num_frames=T, num_inference_steps=PSTEPS, latents=inp["latents"], output_type="latent",
                                    image_embeddings=inp["image_embeddings"], image_latents=inp["image_latents"]).frames
        return done[(T, graph)]
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


def test_161_frames_reach_the_streaming_op_in_every_temporal_layer(tiny, monkeypatch):
    from mofa_video_amd import blocks
    from mofa_video_amd import ops as o
    hu, hc, run = tiny
    calls, inside = [], []
    real_stream, real_block = o.attn_temporal_local_stream, blocks.TransformerSpatioTemporal.__call__

    def spy_block(self, *a, **kw):
        inside.append(self)
        try:
            return real_block(self, *a, **kw)
        finally:
            inside.pop()

    def spy_stream(*a, **kw):
        calls.append((inside[-1] if inside else None, a[4], kw.get("local", "absent")))
        return real_stream(*a, **kw)

    def other(*a, **kw):
        raise AssertionError("a dense or <= 128-frame local temporal attention call at 161 frames under a window")
    monkeypatch.setattr(blocks.TransformerSpatioTemporal, "__call__", spy_block)
    monkeypatch.setattr(o, "attn_temporal_local_stream", spy_stream)
    monkeypatch.setattr(o, "attn_temporal_local", other)
    monkeypatch.setattr(o, "attn_temporal", other)
    monkeypatch.setattr(o, "attn_temporal_sharded", other)
    lat = run(PT, fresh=True)
    nu, nc = _temporal_blocks(hu), _temporal_blocks(hc)
    assert len(nu) == 16 and len(nc) == 7, (len(nu), len(nc))           # (2 + 2 + 2) + 1 + (3 + 3 + 3); (2 + 2 + 2) + 1
    assert calls and all(blk is not None and T == PT and loc == WINDOW for blk, T, loc in calls), {c[1:] for c in calls}
    assert {id(b) for b, _, _ in calls} == {id(b) for b in nu + nc}      # every temporal layer of both networks, nothing else
    monkeypatch.undo()
    assert bool(torch.isfinite(lat).all())


def test_captured_steps_equal_eager_steps_at_161_frames(tiny):
    """graph_steps: only scalars enter the launch, so the step stays capturable and replays the eager bits"""
    _, _, run = tiny
    eager, graph = run(PT), run(PT, graph=True)
    assert bool(torch.isfinite(eager).all()) and torch.equal(eager, graph)


def test_97_frames_through_the_streaming_op_give_the_local_op_bits(tiny, monkeypatch):
    """the dispatch threshold of ``blocks`` lowered to 0: every temporal layer then runs the streaming op, and three steps of both
    networks end in the latents of the unpatched run"""
    from mofa_video_amd import blocks
    from mofa_video_amd import ops as o
    _, _, run = tiny
    usual = run(97)
    monkeypatch.setattr(blocks, "LOCAL_STREAM_ABOVE", 0)
    monkeypatch.setattr(o, "attn_temporal_local", lambda *a, **kw: pytest.fail("the <= 128-frame local op was called"))
    streamed = run(97, fresh=True)
    assert bool(torch.isfinite(usual).all()) and torch.equal(streamed, usual)
