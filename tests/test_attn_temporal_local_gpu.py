"""mofa_attn_temporal_long_local_f16 (csrc/attention.hip attn_temporal_long_local_kernel): temporal attention under the per-query
rule "query frame i sees key frame j iff j < anchor or |i - j| <= radius", driven through ``ops.attn_temporal_local`` so
that the dispatch is what is tested, on the cases of tests/attn_local_cases.py (tests/test_attn_local_cases_cpu.py proves the
table on the CPU).  Shapes are tiny on purpose: HW = 5, heads 2 (head_dim 64) / 1 (head_dim 128), 1 or 2 clips.

Against float64 under the dense kernel's bound; bit-equal to the dense kernel where the rule hides nothing; bit-equal, row by row,
to the key-mask kernel called with that row's visibility as its mask; invisible frames without any influence; packed q|k|v with
guarded output; the refusals; and the plumbing through the UNet, the ControlNet and the pipeline (eager and captured)."""
import pytest
import torch

import attn_local_cases as lc
from helpers import TINY, TINY_CN, oracle_models, synthetic_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
HW = lc.HW


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    lc.release()


def _dev(d):
    return d.q.to(DEV), d.k.to(DEV), d.v.to(DEV)


def _dense_long(q, k, v, clips, T, heads, D):
    """mofa_attn_temporal_long_f16 itself (``ops.attn_temporal`` sends T <= 32 to the 32-key kernel)"""
    from mofa_video_amd import lib as L
    out = torch.empty(clips * T * HW, heads * D, dtype=torch.float16, device=DEV)
    L.check(L.load().mofa_attn_temporal_long_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), clips, T, HW, heads, D,
                                                 q.stride(0), k.stride(0), out.stride(0), D ** -0.5, L.stream_ptr()),
            "mofa_attn_temporal_long_f16")
    return out


# ---- 1. every table case against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T", sorted({(c[0], c[1]) for c in lc.CASES}))
def test_table_cases_against_fp64(ops, D, T):
    top, bad = 0.0, []
    for _, _, r, a in [c for c in lc.CASES if c[:2] == (D, T)]:
        d = lc.local_data(D, T, r, a)
        q, k, v = _dev(d)
        out = ops.attn_temporal_local(q, k, v, d.clips, T, HW, d.heads, head_dim=D, local=(r, a)).cpu()
        assert bool(torch.isfinite(out.float()).all()), (D, T, r, a)
        worst, msg = lc.close_errors(out, d.expect, lc.BOUND, f"hd{D} T{T} radius {r} anchor {a} clips {d.clips}")
        print(f"ATTN-LOCAL hd{D} T{T} radius {r} anchor {a}: worst err / bound {worst:.3f}")
        top, bad = max(top, worst), bad + ([msg] if msg is not None else [])
    assert not bad, (len(bad), bad[:4])


# ---- 2. a rule that hides nothing gives the dense kernel's bits -------------------------------------------------------------------
@pytest.mark.parametrize("D", (64, 128))
def test_all_visible_equals_dense(ops, D):
    cases = [c for c in lc.CASES if c[0] == D and lc.all_visible(*c[1:])]
    assert len(cases) >= 8
    for _, T, r, a in cases:
        d = lc.local_data(D, T, r, a)
        q, k, v = _dev(d)
        got = ops.attn_temporal_local(q, k, v, d.clips, T, HW, d.heads, head_dim=D, local=(r, a))
        assert torch.equal(got, _dense_long(q, k, v, d.clips, T, d.heads, D)), (D, T, r, a)


# ---- 3. row i = row i of the key-mask kernel under the mask {j : i sees j} ----------------------------------------------------------
ROW_CASES = [(64, 33, 0, 0), (64, 33, 4, 1), (64, 33, 16, 2), (64, 65, 1, 1), (64, 65, 31, 33), (64, 65, 32, 0), (64, 128, 12, 1),
             (64, 128, 24, 1), (64, 128, 32, 33), (64, 128, 126, 0), (128, 65, 15, 2), (128, 128, 24, 1)]


@pytest.mark.parametrize("D,T,r,a", ROW_CASES)
def test_rows_equal_the_key_mask_kernel(ops, D, T, r, a):
    clips, heads = 2, lc.HEADS[D]
    q, k, v = (lc.ac._pack_temporal(t).to(DEV) for t in lc.operands(D, T, clips))
    rows = lambda t: t.reshape(clips, T, HW * heads * D)
    local = rows(ops.attn_temporal_local(q, k, v, clips, T, HW, heads, head_dim=D, local=(r, a)))
    vis = lc.visible(T, r, a)
    same = torch.empty(T, dtype=torch.bool, device=DEV)
    for i in range(T):
        mask = sum(1 << j for j in range(T) if vis[i, j])
        masked = rows(ops.attn_temporal_sharded(q, k, v, clips, T, HW, heads, head_dim=D, Tq=T, key_mask=mask))
        same[i] = (masked[:, i] == local[:, i]).all()
    differ = torch.nonzero(~same).flatten().tolist()
    assert not differ, f"hd{D} T{T} radius {r} anchor {a}: rows {differ} differ from the key-mask kernel"


# ---- 4. invisible frames have no influence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T,r,a,j", [(64, 65, 4, 1, 31), (64, 65, 4, 1, 32), (64, 65, 4, 1, 33), (64, 97, 4, 33, 32), (64, 97, 4, 33, 33),
                                       (64, 40, 8, 2, 1), (64, 40, 8, 2, 2), (128, 97, 15, 1, 32), (128, 97, 0, 1, 33), (64, 128, 0, 0, 31)])
def test_invisible_frame_has_no_influence(ops, D, T, r, a, j):
    """frame j's K and V rows overwritten with +-6e4 (finite): every row that cannot see j keeps its bits, rows that can move"""
    clips, heads = 2, lc.HEADS[D]
    q, k, v = (lc.ac._pack_temporal(t).to(DEV) for t in lc.operands(D, T, clips))
    run = lambda kk, vv: ops.attn_temporal_local(q, kk, vv, clips, T, HW, heads, head_dim=D, local=(r, a)).reshape(clips, T, -1)
    base = run(k, v)
    k2, v2 = k.clone(), v.clone()
    sign = torch.where(torch.arange(heads * D, device=DEV) % 2 == 0, 6e4, -6e4).half()
    for t in (k2, v2):
        t.reshape(clips, T, HW, -1)[:, j] = sign
    pert = run(k2, v2)
    sees = lc.visible(T, r, a)[:, j].to(DEV)
    assert bool(sees.any()) and (a > j or not bool(sees.all()))
    assert bool(torch.isfinite(pert[:, ~sees].float()).all())
    assert torch.equal(pert[:, ~sees], base[:, ~sees]), f"rows that cannot see frame {j} changed"
    moved = (pert[:, sees] != base[:, sees]).flatten(1).any(1)
    assert bool(moved.any()), f"no row that sees frame {j} changed"


# ---- 5. layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T,r,a", [(64, 33, 4, 1), (64, 128, 24, 1), (128, 65, 12, 2), (64, 31, 3, 1)])
def test_packed_qkv_and_guarded_output(ops, D, T, r, a):
    d = lc.local_data(D, T, r, a)
    Cc, rows = d.heads * D, d.clips * T * HW
    qkv = torch.cat([d.q, d.k, d.v], 1).to(DEV)                        # one buffer: ld = ldkv = 3 heads D
    q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
    assert q.stride(0) == k.stride(0) == v.stride(0) == 3 * Cc
    buf = torch.full((rows + 5, Cc + 24), float("nan"), dtype=torch.float16, device=DEV)
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[3:3 + rows, 8:8 + Cc] = True
    out = buf[3:3 + rows, 8:8 + Cc]
    assert out.stride(0) == Cc + 24 != q.stride(0)
    ret = ops.attn_temporal_local(q, k, v, d.clips, T, HW, d.heads, head_dim=D, out=out, local=(r, a))
    assert ret is out
    first = buf.clone()
    assert bool(torch.isnan(first[~inside]).all()), "wrote outside the out view"
    worst, msg = lc.close_errors(out.cpu(), d.expect, lc.BOUND, f"packed hd{D} T{T} radius {r} anchor {a}")
    assert msg is None, msg
    assert torch.equal(out, ops.attn_temporal_local(*_dev(d), d.clips, T, HW, d.heads, head_dim=D, local=(r, a))), "the layout changed the bits"
    ops.attn_temporal_local(q, k, v, d.clips, T, HW, d.heads, head_dim=D, out=out, local=(r, a))
    assert torch.equal(buf[inside], first[inside]) and bool(torch.isnan(buf[~inside]).all()), "the second launch differs"


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_rejections_through_lib_check(ops):
    from mofa_video_amd import lib as L
    from mofa_video_amd.lib import MofaHipError
    l = L.load()
    t = torch.zeros(129 * 2, 160 + 16, dtype=torch.float16, device=DEV)
    p = t.data_ptr()

    def call(q=p, k=p, v=p, out=p, nclips=1, T=33, HW=1, heads=1, hd=64, ld=176, ldkv=176, ldo=176, radius=4, anchor=1):
        L.check(l.mofa_attn_temporal_long_local_f16(q, k, v, out, nclips, T, HW, heads, hd, ld, ldkv, ldo, 0.125, radius, anchor,
                                                    L.stream_ptr()), "mofa_attn_temporal_long_local_f16")
    bads = [dict(radius=-1), dict(anchor=-1), dict(anchor=34), dict(T=32, anchor=33), dict(T=129), dict(T=129, anchor=129), dict(T=0),
            dict(hd=80), dict(ld=12), dict(ldkv=172), dict(ldo=0), dict(nclips=0), dict(HW=0), dict(heads=0), dict(q=None), dict(k=None),
            dict(v=None), dict(out=None)]
    for bad in bads:
        with pytest.raises(MofaHipError, match=r"mofa_attn_temporal_long_local_f16 failed with code -22$"):
            call(**bad)
    call(out=torch.empty_like(t).data_ptr(), radius=1000, anchor=33)                                 # a radius above T - 1 means "all"; anchor == T is valid
    torch.cuda.synchronize()
    q = torch.randn(33 * 3, 64, device=DEV).half()
    with pytest.raises(ValueError, match="no key_mask and no Tq"):
        ops.attn_temporal_local(q, q, q, 1, 33, 3, 1, key_mask=1, local=(4, 1))
    with pytest.raises(ValueError, match="no per-query mask"):
        ops.attn_temporal_local(q, q, q, 1, 33, 3, 1, Tq=20, local=(4, 1))
    with pytest.raises(ValueError, match="is required"):
        ops.attn_temporal_local(q, q, q, 1, 33, 3, 1)
    with pytest.raises(MofaHipError, match="code -22"):
        ops.attn_temporal_local(q, q, q, 1, 33, 3, 1, local=(4, 34))


# ---- 7. plumbing ------------------------------------------------------------------------------------------------------------------
PT, PH, PW, PSTEPS = 33, 64, 64, 3


@pytest.fixture(scope="module")
def tiny():
    from mofa_video_amd.adapter import FlowControlNet
    from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
    _, _, _, sdu, sdc, _ = oracle_models(TINY, seed=0, cn_cfg=TINY_CN)
    hu, hc = UNetSpatioTemporalConditionControlNetModel(sdu, TINY, DEV), FlowControlNet(sdc, TINY_CN, DEV)
    inp = synthetic_inputs(PT, PH, PW, cross_dim=TINY["cross_attention_dim"], seed=61)
    done = {}

    def run(window, graph=False, fresh=False):
        """the latents after PSTEPS steps, one run per (temporal_window, graph_steps) unless ``fresh``"""
        from mofa_video_amd.pipeline import FlowControlNetPipeline
        from mofa_video_amd.scheduler import EulerDiscreteScheduler
        if fresh or (window, graph) not in done:
            pipe = FlowControlNetPipeline(unet=hu, controlnet=hc, scheduler=EulerDiscreteScheduler(), max_temporal_frames=64,
                                          temporal_window=window)
            pipe.graph_steps = graph
            done[(window, graph)] = pipe(None, controlnet_condition=inp["cond"], controlnet_flow=inp["flow"], height=PH, width=PW,
                                         num_frames=PT, num_inference_steps=PSTEPS, latents=inp["latents"], output_type="latent",
                                         image_embeddings=inp["image_embeddings"], image_latents=inp["image_latents"]).frames
        return done[(window, graph)]
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


def test_window_that_hides_nothing_is_bit_identical_to_dense(tiny):
    _, _, run = tiny
    dense = run(None)
    assert bool(torch.isfinite(dense).all())
    assert torch.equal(run((PT - 1, 0)), dense)                         # UNet and ControlNet forwards, three steps of both


def test_window_reaches_every_temporal_layer_and_changes_the_output(tiny, monkeypatch):
    from mofa_video_amd import blocks
    from mofa_video_amd import ops as o
    hu, hc, run = tiny
    calls, inside = [], []
    real_local, real_block = o.attn_temporal_local, blocks.TransformerSpatioTemporal.__call__

    def spy_block(self, *a, **kw):
        inside.append(self)
        try:
            return real_block(self, *a, **kw)
        finally:
            inside.pop()

    def spy_local(*a, **kw):
        calls.append((inside[-1] if inside else None, kw.get("local", "absent")))
        return real_local(*a, **kw)

    def no_dense(*a, **kw):
        raise AssertionError("a dense temporal attention call under temporal_window=4")
    monkeypatch.setattr(blocks.TransformerSpatioTemporal, "__call__", spy_block)
    monkeypatch.setattr(o, "attn_temporal_local", spy_local)
    monkeypatch.setattr(o, "attn_temporal", no_dense)
    local = run(4, fresh=True)
    nu, nc = _temporal_blocks(hu), _temporal_blocks(hc)
    assert len(nu) == 16 and len(nc) == 7, (len(nu), len(nc))           # (2 + 2 + 2) + 1 + (3 + 3 + 3); (2 + 2 + 2) + 1
    assert calls and all(blk is not None and loc == (4, 1) for blk, loc in calls), {loc for _, loc in calls}
    assert {id(b) for b, _ in calls} == {id(b) for b in nu + nc}         # every temporal layer of both networks, nothing else
    monkeypatch.undo()
    assert bool(torch.isfinite(local).all()) and not torch.equal(local, run(None))


def test_dense_calls_are_the_calls_they_were(tiny, monkeypatch):
    """temporal_window=None: ``ops.attn_temporal`` is called as it always was, the local entry point never"""
    from mofa_video_amd import ops as o
    from mofa_video_amd.pipeline import FlowControlNetPipeline
    from mofa_video_amd.scheduler import EulerDiscreteScheduler
    hu, hc, _ = tiny
    seen, real = [], o.attn_temporal

    def spy(*a, **kw):
        seen.append(sorted(kw))
        return real(*a, **kw)
    monkeypatch.setattr(o, "attn_temporal", spy)
    monkeypatch.setattr(o, "attn_temporal_local", lambda *a, **kw: pytest.fail("a local call without temporal_window"))
    inp = synthetic_inputs(4, PH, PW, cross_dim=TINY["cross_attention_dim"], seed=62)
    FlowControlNetPipeline(unet=hu, controlnet=hc, scheduler=EulerDiscreteScheduler())(
        None, controlnet_condition=inp["cond"], controlnet_flow=inp["flow"], height=PH, width=PW, num_frames=4, num_inference_steps=1,
        latents=inp["latents"], output_type="latent", image_embeddings=inp["image_embeddings"], image_latents=inp["image_latents"])
    assert seen and all(kw == ["head_dim"] for kw in seen), seen[:3]


def test_captured_steps_equal_eager_steps_under_a_window(tiny):
    """graph_steps: only the two scalars enter the launch, so the step stays capturable and replays the eager bits"""
    _, _, run = tiny
    eager, graph = run(4), run(4, graph=True)
    assert bool(torch.isfinite(eager).all()) and torch.equal(eager, graph)
