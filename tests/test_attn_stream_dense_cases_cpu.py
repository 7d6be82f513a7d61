"""Streaming temporal attention under any window, dense included (past 128 frames), the part that needs no GPU: the case table of
tests/attn_stream_dense_cases.py holds what it claims; the stand-in, which walks a sequence tile by tile with a running maximum as
the kernel does, passes every case under the bound the GPU test applies, and each wrong walk (mutant) misses it on a listed case;
the entry point mofa_attn_temporal_stream_f16 is declared, exported, bound and validates its arguments before any device call;
``ops.attn_temporal_stream`` and the route of ``ops.attn_temporal`` past 128 frames; the pipelines' ``temporal_stream`` keyword
matrix (``False`` is what the constructor did before the keyword); the dispatch in ``blocks``; and the resource report of the
two new instantiations.  tests/test_attn_temporal_stream_dense_gpu.py runs the same cases through the HIP kernel."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

import attn_stream_dense_cases as dc
from test_no_scratch_cpu import HIPCC, _usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mofa_attn_temporal_stream_f16"


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    dc.release()


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_table_lists_what_it_claims():
    assert len(dc.CASES) == len(set(dc.CASES)) <= 220
    assert dc.STREAM_T == (129, 159, 160, 161, 255, 256, 257, 1024) and dc.SHORT_T == (1, 33, 97, 128)
    d64 = [c for c in dc.CASES if c[0] == 64]
    for T in dc.ALL_T:
        have = {(r, a) for _, t, r, a in d64 if t == T}
        want = {(None, None), (T - 1, 0), (0, T), (33, 0), (40, 0), (48, 1), (100, 2), (12, 33), (33, 33), (4, 128),
                (1, 0), (15, 0), (16, 0), (31, 0)}
        assert have == {w for w in want if w[1] is None or w[1] <= T}, T
    for T in dc.STREAM_T:                                              # past 128 frames every listed window is valid
        assert len({(r, a) for _, t, r, a in d64 if t == T}) == 14, T
    d128 = [c for c in dc.CASES if c[0] == 128]
    assert {t for _, t, _, _ in d128} == {33, 129, 161, 257, 1024}
    assert {(r, a) for _, t, r, a in d128 if t == 257} == {(None, None), (0, 257), (40, 0), (48, 1), (12, 33), (4, 128), (15, 0), (31, 0)}
    assert {dc.clips_of(*c) for c in dc.CASES} == {1, 2}
    for D, T, r, a in dc.CASES:
        rr, aa = dc.rule(T, r, a)
        assert rr >= 0 and 0 <= aa <= T and bool(dc.visible(T, rr, aa).diagonal().all())


def test_windows_past_128_are_what_the_ring_kernel_refuses():
    """every listed window but the hazard row breaks radius <= 32 or anchor <= 32; the hazard row is ring-eligible on purpose"""
    for T in dc.STREAM_T:
        for r, a in dc.windows(T):
            rr, aa = dc.rule(T, r, a)
            assert (rr > 32 or aa > 32) != ((r, a) in dc.HAZARD), (T, r, a)


def test_visited_tiles_hold_every_visible_key_and_no_needless_tile():
    """the walk of a query block covers every key some query of the block sees, and every visited tile holds such a key"""
    for D, T, r, a in dc.CASES:
        if D != 64:
            continue
        r, a = dc.rule(T, r, a)
        r = min(r, T - 1)
        vis = dc.visible(T, r, a)
        for q0 in range(0, T, 32):
            tiles = dc.visited_tiles(T, q0, r, a)
            need = sorted({int(j) // 32 for j in torch.nonzero(vis[q0:q0 + 32].any(0)).flatten()})
            assert tiles == need, (T, r, a, q0, tiles, need)


def test_hazard_row_has_an_all_hidden_first_tile():
    """anchor 0 and radius % 32 != 0: the first visited tile of some block hides every key from the block's last query -- the
    state the stale-maximum defect needs"""
    for r, a in dc.HAZARD:
        T = 161
        vis, found = dc.visible(T, r, a), False
        for q0 in range(32, T, 32):
            first = dc.visited_tiles(T, q0, r, a)[0]
            last_q = min(q0 + 31, T - 1)
            found |= not bool(vis[last_q, 32 * first:32 * first + 32].any())
        assert found, (r, a)


@pytest.mark.parametrize("T", dc.ALL_T)
def test_cases_pass_through_the_stand_in(T):
    ops = types.SimpleNamespace(attn_temporal_stream=dc.stand_in)
    top = 0.0
    for D, t, r, a in dc.CASES:
        if t != T:
            continue
        d = dc.dense_data(D, T, r, a)
        out = ops.attn_temporal_stream(d.q, d.k, d.v, d.clips, T, d.HW, d.heads, head_dim=D, local=dc.local_of(r, a))
        assert bool(torch.isfinite(out.float()).all())
        worst, msg = dc.close_errors(out, d.expect, dc.BOUND, f"hd{D} T{T} radius {r} anchor {a}")
        top = max(top, worst)
        assert msg is None, msg
    print(f"ATTN-STREAM-DENSE stand-in T{T}: worst err / bound {top:.3f}")


# the listed cases on which each wrong walk is run (all at 161 or 257 frames, head_dim 64): each must miss the bound on one at least
MUTANT_CASES = ((64, 161, 1, 0), (64, 161, 15, 0), (64, 161, 31, 0), (64, 161, 33, 0), (64, 161, 12, 33), (64, 257, 4, 128),
                (64, 257, None, None), (64, 161, 48, 1))


@pytest.mark.parametrize("defect", dc.MUTANTS)
def test_mutants_are_told_apart(defect):
    assert set(MUTANT_CASES) <= set(dc.CASES)
    caught = []
    for D, T, r, a in MUTANT_CASES:
        d = dc.dense_data(D, T, r, a)
        out = dc.stand_in(d.q, d.k, d.v, d.clips, T, d.HW, d.heads, head_dim=D, local=dc.local_of(r, a), defect=defect)
        if not bool(torch.isfinite(out.float()).all()) or dc.close_errors(out, d.expect, dc.BOUND, defect)[1] is not None:
            caught.append((D, T, r, a))
    print(f"ATTN-STREAM-DENSE mutant {defect}: misses the bound on {caught}")
    assert caught, f"mutant {defect} passes every listed case"
    want = {"stale-max": {(64, 161, 1, 0), (64, 161, 15, 0), (64, 161, 31, 0)}, "band-last": {(64, 161, 1, 0), (64, 161, 33, 0)},
            "anchor-tile0": {(64, 161, 12, 33), (64, 257, 4, 128)}}.get(defect)
    if want is not None:
        assert want <= set(caught), (defect, caught)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    from mofa_video_amd import _build, lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mofa_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", hdr)
    assert m, f"{NAME} is not declared in include/mofa_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == \
        ["q", "k", "v", "out", "nclips", "T", "HW", "heads", "head_dim", "ld", "ldkv", "ldo", "scale", "radius", "anchor", "stream"], params
    _build.build()
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), NAME)
    assert lib.PROTOTYPES[NAME] == lib.PROTOTYPES["mofa_attn_temporal_stream_local_f16"]


def test_every_invalid_argument_is_refused_without_a_device():
    """one violated rule at a time on otherwise valid (never dereferenced) addresses: -22 before any HIP call (there is no GPU
    here: a launch attempt would return MOFA_ELAUNCH instead)"""
    from mofa_video_amd import lib
    fn = getattr(lib.load(), NAME)
    A = 0x10000
    good = dict(q=A, k=A, v=A, out=A, nclips=1, T=160, HW=4, heads=2, head_dim=64, ld=128, ldkv=136, ldo=144, scale=0.125, radius=48,
                anchor=1, stream=None)
    bads = [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(T=0), dict(T=-3), dict(T=1025), dict(T=2048),
            dict(T=1 << 30), dict(head_dim=80), dict(head_dim=32), dict(head_dim=0), dict(head_dim=256), dict(ld=132), dict(ldkv=12),
            dict(ldo=12), dict(ldo=150), dict(ld=0), dict(nclips=0), dict(nclips=-1), dict(HW=0), dict(HW=-4), dict(heads=0),
            dict(heads=-2), dict(radius=-1), dict(radius=-(1 << 31)), dict(anchor=-1)]
    for T in (1, 128, 129, 1024):                                    # (the valid call is not made: it would reach the device)
        for bad in bads + [dict(anchor=T + 1), dict(anchor=1 << 30)]:
            kw = dict(good, T=T, anchor=min(T, 1))
            kw.update(bad)
            assert fn(*kw.values()) == -22, (T, bad)


# ---- ops ----------------------------------------------------------------------------------------------------------------------
def test_stream_op_refuses_before_the_library_loads(monkeypatch):
    from mofa_video_amd import lib, ops

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(lib, "load", no_load)
    for T in (8, 130):
        q = torch.zeros(T * 2, 64, dtype=torch.float16)
        for kw in (dict(key_mask=0xff), dict(Tq=4), dict(Tq=T), dict(Tq=4, key_mask=3)):
            for local in (None, (48, 1)):
                with pytest.raises(ValueError, match="local temporal attention takes no key_mask and no Tq"):
                    ops.attn_temporal_stream(q, q, q, 1, T, 2, 1, local=local, **kw)
        for local in (None, (48, 1)):                                  # the plain calls, dense included, go on to the library
            with pytest.raises(AssertionError, match="the library was loaded"):
                ops.attn_temporal_stream(q, q, q, 1, T, 2, 1, local=local)


def test_stream_op_has_the_local_op_signature():
    from mofa_video_amd import ops
    sig = inspect.signature(ops.attn_temporal_local)
    assert inspect.signature(ops.attn_temporal_stream) == sig
    assert list(inspect.signature(dc.stand_in).parameters) == list(sig.parameters) + ["defect"]


def _stub(monkeypatch):
    from mofa_video_amd import lib, ops
    rows, seen = [], []
    timer = types.SimpleNamespace(start=lambda: 1, stop=lambda name, t0, **kw: rows.append((name, kw)))
    stub = types.SimpleNamespace(**{NAME: lambda *a: seen.append((NAME, a)) or 0,
                                    "mofa_attn_temporal_long_f16": lambda *a: seen.append(("mofa_attn_temporal_long_f16", a)) or 0})
    monkeypatch.setattr(lib, "load", lambda: stub)
    monkeypatch.setattr(lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(ops, "TIMER", timer)
    return ops, rows, seen


def test_stream_op_timer_row_counts_visible_pairs(monkeypatch):
    ops, rows, seen = _stub(monkeypatch)
    T, HW, heads = 130, 2, 1
    q, out = torch.zeros(T * HW, 64, dtype=torch.float16), torch.zeros(T * HW, 64, dtype=torch.float16)
    for local, sent in ((None, (T - 1, 0)), ((48, 1), (48, 1)), ((0, T), (0, T)), ((40, 0), (40, 0))):
        assert ops.attn_temporal_stream(q, q, q, 1, T, HW, heads, out=out, local=local) is out
        name, a = seen.pop()
        assert name == NAME and a[4:15] == (1, T, HW, heads, 64, 64, 64, 64, 0.125, *sent) and not seen
        name, kw = rows.pop()
        pairs = int(dc.visible(T, *sent).sum())
        assert name == "attn_temporal_stream_kernel" and kw["flops"] == 4.0 * pairs * 64 * HW and not rows
    assert ops.stream_visible_pairs(130, 129, 0) == 130 * 130 and ops.stream_visible_pairs(5, 0, 0) == 5


def test_dense_op_routes_by_clip_length(monkeypatch):
    """``ops.attn_temporal``: up to 128 frames the long kernel as before, past 128 the new entry, dense; its sharded forms past 32
    key slots are refused as before"""
    ops, rows, seen = _stub(monkeypatch)
    for T, want in ((128, "mofa_attn_temporal_long_f16"), (129, NAME), (256, NAME), (1024, NAME)):
        q = torch.zeros(T * 2, 64, dtype=torch.float16)
        ops.attn_temporal(q, q, q, 1, T, 2, 1)
        name, a = seen.pop()
        assert name == want and not seen and a[4:6] == (1, T)
        if want == NAME:
            assert a[13:15] == (T - 1, 0)
        rows.clear()
    q = torch.zeros(130 * 2, 64, dtype=torch.float16)
    for kw in (dict(Tq=4), dict(key_mask=3)):
        with pytest.raises(ValueError, match="frame-sharded clips are limited to 32 key slots"):
            ops.attn_temporal(q, q, q, 1, 130, 2, 1, **kw)
    assert not seen


# ---- blocks / pipelines -----------------------------------------------------------------------------------------------------------
def _pipes():
    from mofa_video_amd.pipeline import FlowControlNetPipeline, HybridFlowControlNetPipeline, KeypointFlowControlNetPipeline
    return FlowControlNetPipeline, HybridFlowControlNetPipeline, KeypointFlowControlNetPipeline


RING_WINDOWS = (0, 12, 32, (0, 0), (12, 1), (32, 32), [32, 0])
OTHER_WINDOWS = (None, 33, 48, 500, (33, 1), (12, 33), (48, 1), (4, 128), (33, 33))
OLD_MESSAGE = (r"max_temporal_frames must be an integer in 1 \.\. 128, or up to 256 with temporal_window=\(radius <= 32, anchor <= 32\), "
               r"got ")


def _outcome(cls, **kw):
    try:
        pipe = cls(unet=types.SimpleNamespace(device="cpu"), **kw)
        return ("ok", pipe.max_temporal_frames, pipe.temporal_window)
    except ValueError as e:
        return ("refused", str(e))


@pytest.mark.parametrize("which", (0, 1, 2))
def test_temporal_stream_keyword_matrix(which):
    cls = _pipes()[which]
    assert cls(unet=types.SimpleNamespace(device="cpu")).temporal_stream is False
    for w in RING_WINDOWS + OTHER_WINDOWS:
        win = None if w is None else (w, 1) if isinstance(w, int) else tuple(w)
        for n in (1, 32, 33, 128):                                     # up to 128 frames: accepted with both values
            for ts in (False, True):
                assert _outcome(cls, max_temporal_frames=n, temporal_window=w, temporal_stream=ts) == ("ok", n, win)
        for n in (129, 160, 192, 256):
            absent = _outcome(cls, max_temporal_frames=n, temporal_window=w)
            assert _outcome(cls, max_temporal_frames=n, temporal_window=w, temporal_stream=False) == absent   # False = no keyword
            assert absent[0] == ("ok" if w in RING_WINDOWS else "refused"), (w, n)
            if absent[0] == "refused":                                 # today's message, and a hint that names the keyword
                assert re.match(OLD_MESSAGE + str(n) + " with temporal_window=" + re.escape(repr(w)), absent[1]), absent[1]
                assert "temporal_stream=True" in absent[1]
            assert _outcome(cls, max_temporal_frames=n, temporal_window=w, temporal_stream=True) == ("ok", n, win)
        for n in (0, -1, 257, 1024, 160.0, None, True):
            for ts in (False, True):
                out = _outcome(cls, max_temporal_frames=n, temporal_window=w, temporal_stream=ts)
                assert out[0] == "refused" and "max_temporal_frames" in out[1], (w, n, ts, out)
    for ts in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="temporal_stream must be True or False"):
            cls(unet=types.SimpleNamespace(device="cpu"), temporal_stream=ts)
    with pytest.raises(ValueError, match="temporal_window"):          # the window's own validation is what it was
        cls(unet=types.SimpleNamespace(device="cpu"), max_temporal_frames=160, temporal_window=(4, 129), temporal_stream=True)


def test_pipeline_constants_unchanged():
    from mofa_video_amd import blocks, pipeline
    assert (pipeline.MAX_TEMPORAL_FRAMES, pipeline.MAX_TEMPORAL_FRAMES_LONG, pipeline.MAX_TEMPORAL_FRAMES_STREAM) == (32, 128, 256)
    assert pipeline.STREAM_RADIUS == pipeline.STREAM_ANCHOR == blocks.RING_RADIUS == blocks.RING_ANCHOR == 32


@pytest.mark.parametrize("which", (0, 1, 2))
def test_from_pretrained_forwards_the_keyword(which, monkeypatch, tmp_path):
    from mofa_video_amd import clip, vae
    monkeypatch.setattr(vae.AutoencoderKLTemporalDecoder, "from_pretrained", classmethod(lambda cls, *a, **k: "vae"))
    monkeypatch.setattr(clip.CLIPVisionModelWithProjection, "from_pretrained", classmethod(lambda cls, *a, **k: "enc"))
    cls, unet = _pipes()[which], types.SimpleNamespace(device="cpu")
    pipe = cls.from_pretrained(str(tmp_path), unet=unet, max_temporal_frames=192, temporal_stream=True)
    assert (pipe.temporal_window, pipe.max_temporal_frames, pipe.temporal_stream) == (None, 192, True)
    pipe = cls.from_pretrained(str(tmp_path), unet=unet, max_temporal_frames=256, temporal_window=(48, 1), temporal_stream=True)
    assert (pipe.temporal_window, pipe.max_temporal_frames) == ((48, 1), 256)
    for kw in (dict(max_temporal_frames=192), dict(max_temporal_frames=192, temporal_stream=False),
               dict(max_temporal_frames=257, temporal_stream=True)):
        with pytest.raises(ValueError, match="max_temporal_frames"):
            cls.from_pretrained(str(tmp_path), unet=unet, **kw)


def test_check_call_and_parallel_limits_under_the_keyword():
    from mofa_video_amd.parallel import FrameParallel, GroupedWindowParallel, Layout, WindowParallel
    Flow = _pipes()[0]
    unet = types.SimpleNamespace(device="cpu", config=types.SimpleNamespace(num_frames=25))
    Flow(unet=unet, max_temporal_frames=256, temporal_stream=True)._check_call(1, 1, 3.0, 256)
    Flow(unet=unet, max_temporal_frames=192, temporal_window=(48, 1), temporal_stream=True)._check_call(1, 1, 3.0, 161)
    with pytest.raises(ValueError, match=r"^257 frames per forward pass: the temporal attention kernel handles at most 256 \(use "
                                         r"KeypointFlowControlNetPipeline's window loop for long clips\)$"):
        Flow(unet=unet, max_temporal_frames=256, temporal_stream=True)._check_call(1, 1, 3.0, 257)
    with pytest.raises(ValueError, match="anchor 128 exceeds the 100 frames"):
        Flow(unet=unet, max_temporal_frames=256, temporal_window=(4, 128), temporal_stream=True)._check_call(1, 1, 3.0, 100)
    T = 160
    for window in (None, (48, 1)):
        kw = dict(unet=unet, temporal_window=window, max_temporal_frames=256, temporal_stream=True)
        for par in (FrameParallel(Layout(2, 1, T), None), WindowParallel(None, 0, 4), types.SimpleNamespace()):
            Flow(parallel=par, **kw)._check_call(1, 1, 3.0, 32)
            with pytest.raises(ValueError, match="sharded over ranks are limited to 32"):
                Flow(parallel=par, **kw)._check_call(1, 1, 3.0, T)
        with pytest.raises(ValueError, match="at most max_key_slots = 128"):
            Flow(parallel=types.SimpleNamespace(max_key_slots=128), **kw)._check_call(1, 1, 3.0, T)
    kw = dict(unet=unet, temporal_window=(48, 1), max_temporal_frames=256, temporal_stream=True)
    for par in (FrameParallel(Layout(4, 0, T), None), GroupedWindowParallel(None, 0, 8, 4, T)):
        with pytest.raises(ValueError, match="no per-query mask"):
            Flow(parallel=par, **kw)._check_call(1, 1, 3.0, T)


def test_blocks_dispatch_by_window(monkeypatch):
    """a temporal layer past 128 frames: a ring-eligible window keeps ``ops.attn_temporal_local_stream``, one beyond the ring's limits
    goes to ``ops.attn_temporal_stream``; up to 128 frames every window keeps ``ops.attn_temporal_local``; no window keeps
    ``ops.attn_temporal``.  The layer's other launches are replaced by stand-ins that keep the shapes"""
    from mofa_video_amd import blocks, ops
    C, heads, HW, B = 64, 1, 2, 1
    calls = []

    class _Reached(Exception):
        pass

    def spy(name):
        def op(q, k, v, nclips, T, hw, h, head_dim=64, local=None):
            calls.append((name, nclips, T, hw, h, head_dim, local))
            raise _Reached()
        return op
    monkeypatch.setattr(ops, "attn_temporal_local", spy("local"))
    monkeypatch.setattr(ops, "attn_temporal_local_stream", spy("ring"))
    monkeypatch.setattr(ops, "attn_temporal_stream", spy("stream"))
    monkeypatch.setattr(ops, "attn_temporal", spy("dense"))
    monkeypatch.setattr(ops, "attn_spatial", lambda q, *a, **kw: q)
    monkeypatch.setattr(ops, "lin320_fits", lambda *a: False)
    ident = lambda x, *a, **kw: x
    blk = object.__new__(blocks.TransformerSpatioTemporal)
    blk.C, blk.heads = C, heads
    blk._invariants = lambda c: (None, None, None)
    blk.norm, blk.proj_in, blk.norm1, blk.norm3, blk.norm_in, blk.tnorm1 = (ident,) * 6
    attn = types.SimpleNamespace(can_fuse_norm=False, qkv=lambda h: (h, h, h), to_out=ident, head_dim=64, q_prescaled=False)
    blk.attn1, blk.tattn1 = attn, attn
    blk.ff = lambda x, *a, **kw: x
    blk.ff.can_fuse = False
    blk.ff_in = lambda x, *a, **kw: x
    blk.ff_in.can_fuse = False
    table = ((128, (48, 1), "local"), (128, (4, 128), "local"), (130, (12, 1), "ring"), (256, (32, 32), "ring"), (130, (33, 1), "stream"),
             (130, (12, 33), "stream"), (256, (48, 1), "stream"), (161, (4, 128), "stream"), (161, (500, 0), "stream"),
             (130, None, "dense"), (256, None, "dense"), (32, None, "dense"))
    for T, local, want in table:
        c = types.SimpleNamespace(N=B * T, T=T, B=B, par=None, local=local)
        with pytest.raises(_Reached):
            blk(torch.zeros(B * T * HW, C), c, 1, HW)
        assert calls.pop() == (want, B, T, HW, heads, 64, local) and not calls


# ---- the resource report -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_stream_instantiations_use_no_scratch():
    """exactly two instantiations (head dim 64 with four waves per workgroup, 128 with two), neither with scratch or a spilled
    register"""
    rows = {}
    for n, r in _usage("attention.hip").items():
        m = re.match(r"_Z\d+attn_temporal_stream_kernelILi(\d+)ELi(\d+)EE", n)
        if m:
            rows[tuple(int(x) for x in m.groups())] = r
    assert set(rows) == {(64, 4), (128, 2)}, sorted(rows)
    for inst, r in rows.items():
        assert (r["ScratchSize"], r["VGPRs Spill"], r["SGPRs Spill"]) == (0, 0, 0), (inst, r)
