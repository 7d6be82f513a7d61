"""Local temporal attention of frame-sharded clips (band + anchor keys), the part that needs no GPU: the case table of
tests/attn_window_cases.py holds what it is for; the slot-space rule and the kernel's word formula reproduce
``attn_local_cases.visible`` on every shard of every layout (the same visible frames, none twice, no empty row); wrong rules
(mutants) are told apart; the torch stand-in passes every case under the bound the GPU test applies and has the op's signature;
``FrameParallel.window_plan`` values and refusals; the opt-in rules of ``blocks.make_ctx`` and ``pipeline._check_call``; the entry
point mofa_attn_temporal_long_window_f16 is declared, exported, bound and refuses every invalid argument before any device call;
the resource report of the kernel's eight instantiations; and the windowed sharded temporal block over gloo against the
whole-clip windowed block, on its fast and its conservative exchange.  tests/test_attn_window_gpu.py runs the same cases through
the HIP kernel."""
import ctypes
import inspect
import os
import re
import socket
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import attn_local_cases as lc
import attn_window_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mofa_attn_temporal_long_window_f16"


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    wc.release()
    lc.release()


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_table_lists_what_it_is_for():
    assert wc.LAYOUTS == ((24, 4, 4, 1), (25, 4, 6, 1), (40, 4, 8, 1), (37, 4, 9, 2), (33, 2, 0, 0), (64, 2, 16, 0), (128, 4, 31, 1),
                          (128, 3, 16, 33), (130, 2, 12, 2), (256, 4, 31, 1), (250, 4, 32, 0), (96, 3, 32, 32), (66, 2, 31, 33))
    assert len(wc.CASES) == len(set(wc.CASES)) and set(wc.HD128) <= set(wc.LAYOUTS)
    assert {c[1:5] for c in wc.CASES if c[0] == 64} == set(wc.LAYOUTS)
    assert {(c[1:5], c[5]) for c in wc.CASES if c[0] == 64} == {(lay, s) for lay in wc.LAYOUTS for s in range(lay[1])}   # every shard
    geos = [wc.geometry(*c[1:]) for c in wc.CASES]
    S = sorted({g.S for g in geos})
    assert S[0] == 11 and S[-1] == 128 and all(1 <= g.Tq <= g.L <= g.S <= 128 for g in geos)
    assert {(g.S + 31) // 32 for g in geos} == {1, 2, 3, 4}                                       # all four key-tile counts
    assert {(g.S + 31) // 32 for c, g in zip(wc.CASES, geos) if c[0] == 128} == {1, 2, 3, 4}
    assert any(c[5] == 0 and c[4] > 0 for c in wc.CASES)                                          # a first shard: its band repeats the anchors
    assert any(g.b1 == c[1] and g.b1 - g.f1 < c[3] for c, g in zip(wc.CASES, geos))               # a last shard: the band is truncated
    assert any(c[4] == 33 for c in wc.CASES) and any(c[3] == 0 for c in wc.CASES) and any(c[1] > 128 for c in wc.CASES)
    assert any(g.f0 + c[3] < c[4] for c, g in zip(wc.CASES, geos))                                # a query whose whole band lies below the anchor
    assert {wc.clips_of(*c) for c in wc.CASES} == {1, 2}
    for T, n in {(c[1], c[2]) for c in wc.CASES}:
        from mofa_video_amd.parallel import split_frames
        assert wc.bounds(T, n) == split_frames(T, n)


def test_slot_rule_and_word_formula_reproduce_the_rule_on_every_shard():
    """per rank and query: the visible slots name exactly the visible frames of the whole-clip rule, each once, and at least
    one; the lo / hi1 formula of the header gives the same table"""
    for T, n, r, a in wc.LAYOUTS:
        whole = lc.visible(T, r, a)
        for s in range(n):
            g = wc.geometry(T, n, r, a, s)
            vis, frames = wc.slot_visible(g, r, a), wc.slot_frames(g, a)
            assert vis.shape == (g.Tq, g.S) and len(frames) == g.S
            assert torch.equal(vis, wc.formula_visible(g, r, a)), (T, n, r, a, s)
            for i in range(g.Tq):
                seen = [frames[j] for j in range(g.S) if vis[i, j]]
                assert seen and len(seen) == len(set(seen)), (T, n, r, a, s, i)                 # no empty row, no duplicate
                assert sorted(seen) == torch.nonzero(whole[g.f0 + i]).flatten().tolist(), (T, n, r, a, s, i)


@pytest.mark.parametrize("defect", wc.MUTANTS)
def test_mutants_are_told_apart(defect):
    """a wrong slot-space rule differs from the true table on listed cases, and on at least one of them its float64 attention
    misses the bound the GPU test applies (or has an empty softmax row)"""
    differs, caught = [], []
    for case in [c for c in wc.CASES if c[0] == 64]:
        D, T, n, r, a, s = case
        g = wc.geometry(T, n, r, a, s)
        wrong = wc.mutant_slot_visible(defect, g, r, a)
        if torch.equal(wrong, wc.slot_visible(g, r, a)):
            continue
        differs.append(case)
        d = wc.window_data(*case)
        q, k, v = wc.split(d.q, d.clips, g.Tq, D), wc.split(d.k, d.clips, g.S, D), wc.split(d.v, d.clips, g.S, D)
        out = lc.ac._pack_temporal(lc.attention64(q, k, v, D ** -0.5, wrong)).half()
        if wc.close_errors(out, d.expect, wc.BOUND, f"{defect} {case}")[1] is not None:
            caught.append(case)
    print(f"ATTN-WINDOW mutant {defect}: differs on {len(differs)} cases, misses the bound on {len(caught)}: {caught[:3]}")
    assert differs and caught, (defect, differs, caught)
    want = {"duplicates": lambda c: wc.geometry(*c[1:]).b0 < c[4],            # the band begins below the anchor
            "slot-distance": lambda c: c[5] > 0 and c[3] > 0, "no-anchor": lambda c: c[4] > 0, "strict": lambda c: True}[defect]
    assert all(want(c) for c in differs) and any(want(c) for c in caught)


@pytest.mark.parametrize("layout", wc.LAYOUTS)
def test_cases_pass_through_the_stand_in(layout):
    ops = types.SimpleNamespace(attn_temporal_window=wc.stand_in)
    top = 0.0
    for case in [c for c in wc.CASES if c[1:5] == layout]:
        d = wc.window_data(*case)
        out = ops.attn_temporal_window(d.q, d.k, d.v, d.clips, d.g.S, d.HW, d.heads, head_dim=case[0], **d.kw)
        assert bool(torch.isfinite(out.float()).all())
        worst, msg = wc.close_errors(out, d.expect, wc.BOUND, f"hd{case[0]} {layout} shard {case[5]}")
        top = max(top, worst)
        assert msg is None, msg
    print(f"ATTN-WINDOW stand-in {layout}: worst err / bound {top:.3f}")


def test_stand_in_has_the_signature_of_the_op(monkeypatch):
    from mofa_video_amd import lib, ops
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items() if not n.startswith("_")]   # noqa: E731
    assert sig(ops.attn_temporal_window) == sig(wc.stand_in)
    assert list(inspect.signature(ops.attn_temporal_window).parameters) == \
        ["q", "k", "v", "nclips", "S", "HW", "heads", "head_dim", "scale", "out", "Tq", "local", "q_frame0", "band_frame0"]

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(lib, "load", no_load)
    q = torch.zeros(20 * 2, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match=r"local=\(radius, anchor\) is required"):
        ops.attn_temporal_window(q, q, q, 1, 20, 2, 1, Tq=8, q_frame0=4)
    with pytest.raises(AssertionError, match="the library was loaded"):
        ops.attn_temporal_window(q, q, q, 1, 20, 2, 1, Tq=8, local=(4, 1), q_frame0=4)
    # the TIMER's flops count the visible keys
    for case in wc.CASES[::5]:
        _, T, n, r, a, s = case
        g = wc.geometry(T, n, r, a, s)
        assert ops.window_visible_keys(g.S, g.Tq, r, a, g.f0, g.b0) == int(wc.slot_visible(g, r, a).sum()), case


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    from mofa_video_amd import _build, lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mofa_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", hdr)
    assert m, f"{NAME} is not declared in include/mofa_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == \
        ["q", "k", "v", "out", "nclips", "Tq", "S", "HW", "heads", "head_dim", "ld", "ldkv", "ldo", "scale", "radius", "anchor", "q_frame0",
         "band_frame0", "stream"], params
    _build.build()
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), NAME)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert lib.PROTOTYPES[NAME] == [P, P, P, P, I, I, I, I, I, I, I, I, I, F, I, I, I, I, P]


def test_every_invalid_argument_is_refused_without_a_device():
    """one violated rule at a time on otherwise valid (never dereferenced) addresses: -22 before any HIP call (there is no GPU
    here: a launch attempt would return MOFA_ELAUNCH instead).  The valid call is not made: it would reach the device"""
    from mofa_video_amd import lib
    fn = getattr(lib.load(), NAME)
    A = 0x10000
    good = dict(q=A, k=A, v=A, out=A, nclips=1, Tq=10, S=27, HW=4, heads=2, head_dim=64, ld=128, ldkv=136, ldo=144, scale=0.125, radius=8,
                anchor=1, q_frame0=20, band_frame0=12, stream=None)                 # band frames 12 .. 37, queries 20 .. 29
    bads = [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(S=0), dict(S=-3), dict(S=129), dict(S=256), dict(head_dim=80),
            dict(head_dim=32), dict(head_dim=0), dict(head_dim=256), dict(ld=132), dict(ldkv=12), dict(ldo=12), dict(ldo=150), dict(ld=0),
            dict(ldkv=0), dict(ldo=-8), dict(nclips=0), dict(nclips=-1), dict(HW=0), dict(HW=-4), dict(heads=0), dict(heads=-2),
            dict(Tq=0), dict(Tq=-1), dict(anchor=-1), dict(anchor=28), dict(anchor=129), dict(radius=-1), dict(radius=-128),
            dict(band_frame0=-1), dict(band_frame0=-12, q_frame0=-4), dict(q_frame0=11), dict(q_frame0=0), dict(q_frame0=-1),
            dict(q_frame0=29),                    # queries 29 .. 38: one past the band's last frame 37
            dict(Tq=27),                          # more queries than band slots (L = 26)
            dict(Tq=19),                          # 20 .. 38
            dict(anchor=10),                      # L = 17: the band 12 .. 28 ends before the last query (anchor = 9 would still hold it)
            dict(anchor=27, Tq=1, q_frame0=12),   # L = 0: no band slot for the query's own frame
            dict(band_frame0=2 ** 31 - 8, q_frame0=2 ** 31 - 8)]
    for bad in bads:
        kw = dict(good)
        kw.update(bad)
        assert fn(*kw.values()) == -22, bad
    for S, Tq in ((1, 1), (32, 32), (33, 33), (128, 128)):                          # every key-tile count refuses alike
        for bad in (dict(Tq=Tq + 1), dict(anchor=S + 1), dict(anchor=1), dict(q_frame0=1), dict(band_frame0=1), dict(radius=-1)):
            kw = dict(good, S=S, Tq=Tq, anchor=0, q_frame0=0, band_frame0=0)
            kw.update(bad)
            assert fn(*kw.values()) == -22, (S, bad)


# ---- parallel: the plan ----------------------------------------------------------------------------------------------------------
def _par(T, n, s, **kw):
    from mofa_video_amd.parallel import FrameParallel, Layout
    return FrameParallel(Layout(n, s, T, cfg_ranks=1), None, **kw)


def test_window_plan_values_for_the_table():
    for T, n, r, a in wc.LAYOUTS:
        plans = [_par(T, n, s, window_keys=True).window_plan(r, a) for s in range(n)]
        for s, p in enumerate(plans):
            g = wc.geometry(T, n, r, a, s)
            assert (p.b0, p.b1, p.S, p.own) == (g.b0, g.b1, g.S, g.own), (T, n, r, a, s)
            assert p.own + g.Tq <= p.S <= 128 and p.own >= a
            assert (p.recv_prev, p.recv_next) == (g.f0 - g.b0, g.b1 - g.f1) == (r if s > 0 else 0, r if s + 1 < n else 0)
            assert p.recv_anchor == (a if s > 0 else 0)
            assert p.frames_window == p.recv_prev + p.recv_next + p.recv_anchor
            assert p.frames_gathered == (n - 1) * (wc.bounds(T, n)[0][1])
            if s > 0:                                                                    # what one sends is what the other receives
                assert plans[s - 1].send_next == p.recv_prev and p.send_prev == plans[s - 1].recv_next
        assert plans[0].send_prev == 0 and plans[-1].send_next == 0
    # the issue's example: 128 frames on 4 frame shards, radius 8, anchor 1
    plans = [_par(128, 4, s, window_keys=True).window_plan(8, 1) for s in range(4)]
    assert [p.S for p in plans] == [41, 49, 49, 41] and [p.frames_window for p in plans] == [8, 17, 17, 9]
    assert {p.frames_gathered for p in plans} == {96}
    # the plan is kept per (radius, anchor) and a grouped object passes the keyword through
    from mofa_video_amd.parallel import GroupedWindowParallel
    par = _par(40, 4, 1, window_keys=True)
    assert par.window_plan(8, 1) is par.window_plan(8, 1) is par._wplan
    gw = GroupedWindowParallel(None, 5, 8, 4, 40, window_keys=True)
    assert gw.window_keys is True and gw.frame.window_keys is True and gw.frame.window_plan(8, 1).S == 1 + 20 + 8
    assert GroupedWindowParallel(None, 5, 8, 4, 40).window_keys is False and _par(40, 4, 1).window_keys is False


def test_window_plan_refusals_name_the_rule():
    with pytest.raises(ValueError, match="without window_keys=True"):
        _par(40, 4, 1).window_plan(8, 1)
    with pytest.raises(ValueError, match=r"radius 11 exceeds the smallest frame shard \(10 of 40 frames over 4 shards\)"):
        _par(40, 4, 1, window_keys=True).window_plan(11, 1)
    with pytest.raises(ValueError, match=r"radius 7 exceeds the smallest frame shard \(6 of 25"):      # 7 + 6 + 6 + 6
        _par(25, 4, 0, window_keys=True).window_plan(7, 1)
    with pytest.raises(ValueError, match="anchor 11 exceeds the 10 frames of shard 0"):
        _par(40, 4, 2, window_keys=True).window_plan(4, 11)
    with pytest.raises(ValueError, match=r"1 \+ 64 \+ 2 x 32 = 129 key slots exceed"):
        _par(256, 4, 3, window_keys=True).window_plan(32, 1)
    with pytest.raises(ValueError, match=r"33 \+ 34 \+ 2 x 31 = 129 key slots exceed"):
        _par(68, 2, 0, window_keys=True).window_plan(31, 33)
    with pytest.raises(ValueError, match="must be >= 0"):
        _par(40, 4, 1, window_keys=True).window_plan(-1, 1)
    par = _par(40, 4, 1, window_keys=True)
    with pytest.raises(ValueError, match="call window_plan"):
        par.window_buffer(4, 8, torch.device("cpu"))
    par.window_plan(8, 1)
    buf, own = par.window_buffer(4, 8, torch.device("cpu"))
    assert buf.shape == (27 * 4, 8) and own.shape == (10 * 4, 8) and own.data_ptr() == buf[9 * 4:].data_ptr()


# ---- blocks / pipeline: opt-in ----------------------------------------------------------------------------------------------------
def test_make_ctx_takes_a_window_with_a_window_keys_shard_only():
    from mofa_video_amd import blocks
    net = types.SimpleNamespace(device="cpu", time=lambda ts, ids: None, temb_batch=types.SimpleNamespace(run=lambda a: None))
    base = blocks.Ctx(2, 8)
    base.ctx16 = torch.zeros(2, 4)
    ids = torch.zeros(2, 3)
    for par in (object(), _par(40, 4, 1), types.SimpleNamespace(window_keys=False)):
        with pytest.raises(ValueError, match="^local temporal attention of frame-sharded clips: the gathered-key path has no per-query mask$"):
            blocks.make_ctx(net, 0.5, None, ids, 2, 8, base=base, par=par, local=(4, 1))
        assert blocks.make_ctx(net, 0.5, None, ids, 2, 8, base=base, par=par).par is par             # dense: as before
    par = _par(40, 4, 1, window_keys=True)
    c = blocks.make_ctx(net, 0.5, None, ids, 2, 8, base=base, par=par, local=(4, 1))
    assert c.par is par and c.local == (4, 1)


def test_check_call_with_a_window_and_frame_shards():
    from mofa_video_amd.parallel import FrameParallel, GroupedWindowParallel, Layout
    from mofa_video_amd.pipeline import FlowControlNetPipeline as Flow
    unet = types.SimpleNamespace(device="cpu")
    refusal = r"frame-sharded clips has no per-query mask \(a CFG split alone and WindowParallel are fine\)"
    for par in (FrameParallel(Layout(4, 0, 40), None), FrameParallel(Layout(4, 0, 40), None, max_key_slots=64),
                GroupedWindowParallel(None, 0, 8, 4, 40, max_key_slots=64)):
        with pytest.raises(ValueError, match=refusal):                                                # the default objects still refuse
            Flow(unet=unet, parallel=par, temporal_window=(8, 1), max_temporal_frames=64)._check_call(1, 1, 3.0, 40)
    mk = lambda T, world=4, **kw: FrameParallel(Layout(world, 0, T), None, window_keys=True, **kw)    # noqa: E731
    # max_key_slots stays at its default of 32: S replaces it
    Flow(unet=unet, parallel=mk(40), temporal_window=(8, 1), max_temporal_frames=64)._check_call(1, 1, 3.0, 40)
    Flow(unet=unet, parallel=mk(130), temporal_window=(12, 2), max_temporal_frames=256)._check_call(1, 1, 3.0, 130)
    Flow(unet=unet, parallel=mk(256, 8), temporal_window=(31, 1), max_temporal_frames=256)._check_call(1, 1, 3.0, 256)
    Flow(unet=unet, parallel=GroupedWindowParallel(None, 0, 8, 4, 40, window_keys=True), temporal_window=(8, 1),
         max_temporal_frames=64)._check_call(1, 1, 3.0, 40)
    # max_temporal_frames still caps the frames of a forward pass
    with pytest.raises(ValueError, match="^40 frames per forward pass: the temporal attention kernel handles at most 32"):
        Flow(unet=unet, parallel=mk(40), temporal_window=(8, 1))._check_call(1, 1, 3.0, 40)
    with pytest.raises(ValueError, match="temporal attention kernel handles at most 128"):
        Flow(unet=unet, parallel=mk(130), temporal_window=(12, 2), max_temporal_frames=128)._check_call(1, 1, 3.0, 130)
    with pytest.raises(ValueError, match="max_temporal_frames must be an integer"):                   # 256 needs a stream-eligible window
        Flow(unet=unet, parallel=mk(130), temporal_window=(33, 2), max_temporal_frames=256)
    # window_plan's refusals pass through
    with pytest.raises(ValueError, match="radius 21 exceeds the smallest frame shard"):
        Flow(unet=unet, parallel=mk(40), temporal_window=(21, 1), max_temporal_frames=64)._check_call(1, 1, 3.0, 40)
    with pytest.raises(ValueError, match="key slots exceed the attention kernel's 128"):
        Flow(unet=unet, parallel=mk(130), temporal_window=(32, 1), max_temporal_frames=256)._check_call(1, 1, 3.0, 130)
    with pytest.raises(ValueError, match="the parallel object's layout shards 40"):
        Flow(unet=unet, parallel=mk(40), temporal_window=(8, 1), max_temporal_frames=64)._check_call(1, 1, 3.0, 48)
    # a window_keys object without a window is the dense object it was
    with pytest.raises(ValueError, match=r"sharded over ranks are limited to 32 frames"):
        Flow(unet=unet, parallel=mk(40), max_temporal_frames=64)._check_call(1, 1, 3.0, 40)
    Flow(unet=unet, parallel=mk(40, max_key_slots=64), max_temporal_frames=64)._check_call(1, 1, 3.0, 40)


# ---- the resource report ----------------------------------------------------------------------------------------------------------
def test_window_kernel_instantiations():
    """the eight instantiations the launcher dispatches to: no scratch, no spill, and the occupancy [waves / SIMD] by (head dim,
    key tiles, waves per workgroup) that tests/test_no_scratch_cpu.py::test_long_temporal_attention_instantiations states for
    the other three kernels on the same body"""
    import test_no_scratch_cpu as ns
    if not os.path.exists(ns.HIPCC):
        pytest.skip("hipcc not found")
    occupancy = {(64, 1, 4): 4, (64, 2, 2): 3, (64, 3, 1): 2, (64, 4, 1): 2, (128, 1, 2): 2, (128, 2, 1): 2, (128, 3, 1): 1, (128, 4, 1): 1}
    rows = {}
    for n, r in ns._usage("attention.hip").items():
        m = re.match(r"_Z\d+attn_temporal_long_window_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", n)
        if m:
            inst = tuple(int(x) for x in m.groups())
            assert inst not in rows, inst
            rows[inst] = r
    assert set(rows) == set(occupancy), sorted(rows)
    for inst, r in rows.items():
        assert r == {"ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0, "Occupancy": occupancy[inst]}, (inst, r)


# ---- gloo: the windowed sharded temporal block ---------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _block_worker(rank, world, port, T, hd, radius, anchor):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sharded_long_checks as sc
        import window_shard_checks as ws
        from helpers import rel_l2
        from mofa_video_amd.parallel import FrameParallel, Layout, TorchComm
        ws.install_stand_ins()
        torch.set_num_threads(2)
        calls = []
        ws.spy_on_window_attention(calls)
        lay = Layout(world, rank, T, cfg_ranks=1)
        par = FrameParallel(lay, TorchComm(lambda r: Layout(world, r, T, cfg_ranks=1)), window_keys=True)
        report = par.self_check("cpu")
        assert report["window"] == "batched p2p + anchor broadcast" and par.window_p2p, report
        par.log = []
        blk = sc.make_block(hd, "cpu")
        x, emb = sc.block_inputs(blk, T, "cpu")
        HW = sc.H * sc.W
        ref = ws.run_block(blk, x, emb, T, (radius, anchor))[lay.f0 * HW:lay.f1 * HW]
        fast = ws.run_block(blk, x[lay.f0 * HW:lay.f1 * HW], emb, lay.T_loc, (radius, anchor), par)
        par.window_p2p = False                                          # what a failed self-check leaves on every rank
        slow = ws.run_block(blk, x[lay.f0 * HW:lay.f1 * HW], emb, lay.T_loc, (radius, anchor), par)
        e = rel_l2(fast, ref)
        assert calls == [ws.expected_call(T, world, radius, anchor, rank)] * 2, (rank, calls)
        assert par.log == [(0, "window")] * 2, par.log                  # one exchange per temporal layer, no token gather
        assert torch.equal(fast, slow), (rank, "the conservative exchange gives other bits")
        assert fast.shape == ref.shape and e < 2e-3, (rank, e)
        errs = [None] * world
        dist.all_gather_object(errs, e)
        if rank == 0:
            print(f"windowed sharded temporal block, {T} frames over {world} shards, window ({radius}, {anchor}), head dim {hd}: "
                  "rel-L2 per rank", ["%.2e" % v for v in errs])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,T,hd,radius,anchor", [(2, 66, 64, 31, 33), (4, 40, 128, 8, 1), (4, 130, 64, 12, 2), (2, 33, 64, 0, 0)])
def test_windowed_sharded_temporal_block_gloo(world, T, hd, radius, anchor):
    """one TransformerSpatioTemporal block under a window on frames-only shards (``window_keys=True``) against the same
    windowed block on the whole clip, on torch stand-ins: 33 + 33 frames with 33 anchors (97 slots on both ranks), 4 x 10
    frames, 130 frames as 33 + 33 + 32 + 32 (more than any gathered path takes), and radius 0 without anchors (nothing is
    exchanged).  The stated bound of the sharded path, rel-L2 2e-3 (tests/test_sharded_long_cpu.py); the p2p exchange and the
    conservative one bit-equal; one "window" entry per temporal layer in the log and no "tokens" entry"""
    mp.spawn(_block_worker, args=(world, _free_port(), T, hd, radius, anchor), nprocs=world, join=True)
