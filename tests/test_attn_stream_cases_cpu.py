"""Streaming local temporal attention (local rule past 128 frames), the part that needs no GPU: the case table of
tests/attn_stream_cases.py holds what it claims; wrong ways to run the key-tile ring (mutants) are told apart from the rule by the
table; the block-by-block torch stand-in passes every case under the bound the GPU test applies; the entry point
mofa_attn_temporal_stream_local_f16 is declared, exported, bound and validates its arguments before any device call;
``ops.attn_temporal_local_stream`` makes the refusals of ``ops.attn_temporal_local`` before the library loads; the pipelines'
``max_temporal_frames`` x ``temporal_window`` keyword matrix, ``_check_call`` past 128 frames, the refusal of frame-sharded
layouts, the dispatch in ``blocks``; and the resource report of the two new instantiations.
tests/test_attn_temporal_stream_gpu.py runs the same cases through the HIP kernel."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

import attn_stream_cases as sc
from test_no_scratch_cpu import HIPCC, _usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mofa_attn_temporal_stream_local_f16"


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    sc.release()


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_table_lists_what_it_claims():
    assert len(sc.CASES) == len(set(sc.CASES)) <= 200
    assert sc.STREAM_T == (129, 159, 160, 161, 192, 193, 255, 256, 257, 1024)
    assert sc.SHORT_T == (1, 31, 32, 33, 64, 65, 96, 97, 127, 128)
    for D, T, r, a in sc.CASES:
        assert D in (64, 128) and T in sc.ALL_T and r in (0, 1, 15, 16, 31, 32) and a in (0, 1, 2, 31, 32) and a <= T, (D, T, r, a)
    d64 = [c for c in sc.CASES if c[0] == 64]
    for T in sc.ALL_T:                                                 # every radius and every valid anchor of every T
        assert {r for _, t, r, _ in d64 if t == T} == {0, 1, 15, 16, 31, 32}, T
        assert {a for _, t, _, a in d64 if t == T} == {a for a in (0, 1, 2, 31, 32) if a <= T}, T
    d128 = [c for c in sc.CASES if c[0] == 128]
    assert {t for _, t, _, _ in d128} >= {1, 129, 161, 257, 1024}
    assert {r for _, _, r, _ in d128} >= {0, 32} and {a for _, _, _, a in d128} >= {0, 32}
    assert {sc.clips_of(*c) for c in sc.CASES} == {1, 2}


def test_rule_is_the_local_rule_and_needs_four_tiles_only():
    """under radius <= 32 and anchor <= 32 a query of block tq sees nothing outside the frame tiles 0, tq - 1, tq, tq + 1: what the
    four score tiles of the kernel rest on"""
    for D, T, r, a in sc.CASES:
        vis = sc.visible(T, r, a)
        i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
        assert torch.equal(vis, (j < a) | ((i - j).abs() <= r)) and bool(vis.diagonal().all())
        near = (j // 32 == 0) | ((j // 32 - i // 32).abs() <= 1)
        assert not bool((vis & ~near).any()), (T, r, a)


@pytest.mark.parametrize("defect", sc.MUTANTS)
def test_mutants_are_told_apart(defect):
    """a wrong ring differs from the rule on listed cases, and on each of them its float64 attention misses the bound the GPU test
    applies (or has an empty softmax row)"""
    differs = [c for c in sc.CASES if not sc.same_attention(sc.mutant_weights(defect, *c[1:]), *c[1:])]
    assert differs, f"mutant {defect} agrees with the rule on every listed case"
    assert any(c[1] > 128 for c in differs), f"mutant {defect} differs on no case past 128 frames"
    caught = 0
    for D, T, r, a in differs:
        w = sc.mutant_weights(defect, T, r, a)
        if not bool((w.sum(1) > 0).all()):                             # an empty row: NaN, caught by the finiteness check
            caught += 1
            continue
        d = sc.local_data(D, T, r, a)
        q, k, v = (sc.split_rows(t, d.clips, T, D) for t in (d.q, d.k, d.v))
        out = sc.ac._pack_temporal(sc.attention64_weighted(q, k, v, D ** -0.5, w)).half()
        caught += sc.close_errors(out, d.expect, sc.BOUND, f"{defect} {(D, T, r, a)}")[1] is not None
    print(f"ATTN-STREAM mutant {defect}: differs on {len(differs)} cases, misses the bound on {caught}")
    assert caught == len(differs), (defect, caught, len(differs))


def test_weighted_reference_with_the_rule_is_the_reference():
    for D, T, r, a in ((64, 161, 15, 2), (128, 33, 16, 2)):
        d = sc.local_data(D, T, r, a)
        q, k, v = (sc.split_rows(t, d.clips, T, D) for t in (d.q, d.k, d.v))
        w = sc.visible(T, r, a).long()
        assert sc.same_attention(w, T, r, a) and sc.same_attention(3 * w, T, r, a)
        assert torch.equal(sc.ac._pack_temporal(sc.attention64_weighted(q, k, v, D ** -0.5, w)), d.expect)


@pytest.mark.parametrize("T", sc.ALL_T)
def test_cases_pass_through_the_stand_in(T):
    ops = types.SimpleNamespace(attn_temporal_local_stream=sc.stand_in)
    top = 0.0
    for D, t, r, a in sc.CASES:
        if t != T:
            continue
        d = sc.local_data(D, T, r, a)
        out = ops.attn_temporal_local_stream(d.q, d.k, d.v, d.clips, T, d.HW, d.heads, head_dim=D, local=(r, a))
        assert bool(torch.isfinite(out.float()).all())
        worst, msg = sc.close_errors(out, d.expect, sc.BOUND, f"hd{D} T{T} radius {r} anchor {a}")
        top = max(top, worst)
        assert msg is None, msg
    print(f"ATTN-STREAM stand-in T{T}: worst err / bound {top:.3f}")


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
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert lib.PROTOTYPES[NAME] == [P, P, P, P, I, I, I, I, I, I, I, I, F, I, I, P] == lib.PROTOTYPES["mofa_attn_temporal_long_local_f16"]


def test_every_invalid_argument_is_refused_without_a_device():
    """one violated rule at a time on otherwise valid (never dereferenced) addresses: -22 before any HIP call (there is no GPU
    here: a launch attempt would return MOFA_ELAUNCH instead).  Everything mofa_attn_temporal_long_f16 refuses with 1024 frames
    in place of 128, and the window's own limits"""
    from mofa_video_amd import lib
    fn = getattr(lib.load(), NAME)
    A = 0x10000
    good = dict(q=A, k=A, v=A, out=A, nclips=1, T=160, HW=4, heads=2, head_dim=64, ld=128, ldkv=136, ldo=144, scale=0.125, radius=4,
                anchor=1, stream=None)
    bads = [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(T=0), dict(T=-3), dict(T=1025), dict(T=2048),
            dict(T=1 << 30), dict(head_dim=80), dict(head_dim=32), dict(head_dim=0), dict(head_dim=256), dict(ld=132), dict(ldkv=12),
            dict(ldo=12), dict(ldo=150), dict(ld=0), dict(nclips=0), dict(nclips=-1), dict(HW=0), dict(HW=-4), dict(heads=0),
            dict(heads=-2), dict(radius=-1), dict(radius=33), dict(radius=127), dict(radius=1000), dict(anchor=-1), dict(anchor=33),
            dict(anchor=128)]
    for T in (1, 128, 129, 1024):                                    # (the valid call is not made: it would reach the device)
        for bad in bads + [dict(anchor=T + 1)]:
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
            with pytest.raises(ValueError, match="local temporal attention takes no key_mask and no Tq"):
                ops.attn_temporal_local_stream(q, q, q, 1, T, 2, 1, local=(2, 1), **kw)
        with pytest.raises(ValueError, match=r"local=\(radius, anchor\) is required"):
            ops.attn_temporal_local_stream(q, q, q, 1, T, 2, 1)
        with pytest.raises(AssertionError, match="the library was loaded"):   # the plain call goes on to the library
            ops.attn_temporal_local_stream(q, q, q, 1, T, 2, 1, local=(2, 1))


def test_stream_op_has_the_local_op_signature():
    from mofa_video_amd import ops
    sig = inspect.signature(ops.attn_temporal_local)
    assert inspect.signature(ops.attn_temporal_local_stream) == sig == inspect.signature(sc.stand_in)
    assert list(sig.parameters) == ["q", "k", "v", "nclips", "T", "HW", "heads", "head_dim", "scale", "out", "Tq", "key_mask", "local"]


def test_stream_op_has_a_timer_row(monkeypatch):
    """with a TIMER installed the launch is recorded under a row of its own (the library replaced by a stub that accepts the call)"""
    from mofa_video_amd import lib, ops
    rows = []
    timer = types.SimpleNamespace(start=lambda: 1, stop=lambda name, t0, **kw: rows.append((name, kw)))
    seen = []
    stub = types.SimpleNamespace(mofa_attn_temporal_stream_local_f16=lambda *a: seen.append(a) or 0)
    monkeypatch.setattr(lib, "load", lambda: stub)
    monkeypatch.setattr(lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(ops, "TIMER", timer)
    T, HW, heads = 130, 2, 1
    q, out = torch.zeros(T * HW, 64, dtype=torch.float16), torch.zeros(T * HW, 64, dtype=torch.float16)
    assert ops.attn_temporal_local_stream(q, q, q, 1, T, HW, heads, out=out, local=(12, 1)) is out
    assert len(seen) == 1 and seen[0][4:15] == (1, T, HW, heads, 64, 64, 64, 64, 0.125, 12, 1)
    assert len(rows) == 1 and rows[0][0] == "attn_temporal_stream_kernel" and rows[0][1]["nbytes"] == 8.0 * T * HW * 64


# ---- blocks / pipelines -----------------------------------------------------------------------------------------------------------
def _pipes():
    from mofa_video_amd.pipeline import FlowControlNetPipeline, HybridFlowControlNetPipeline, KeypointFlowControlNetPipeline
    return FlowControlNetPipeline, HybridFlowControlNetPipeline, KeypointFlowControlNetPipeline


def test_pipeline_constants():
    from mofa_video_amd import pipeline
    assert (pipeline.MAX_TEMPORAL_FRAMES, pipeline.MAX_TEMPORAL_FRAMES_LONG, pipeline.MAX_TEMPORAL_FRAMES_STREAM) == (32, 128, 256)
    assert pipeline.STREAM_RADIUS == pipeline.STREAM_ANCHOR == 32


WINDOWS_THAT_STREAM = (0, 12, 32, (0, 0), (12, 1), (32, 32), [32, 0], (1, 32))
WINDOWS_THAT_DO_NOT = (None, 33, 127, 500, (33, 1), (12, 33), (32, 128), (33, 33))


@pytest.mark.parametrize("which", (0, 1, 2))
def test_max_temporal_frames_by_temporal_window(which):
    cls = _pipes()[which]
    unet = types.SimpleNamespace(device="cpu")
    for w in WINDOWS_THAT_STREAM + WINDOWS_THAT_DO_NOT:
        for n in (1, 32, 33, 128):                                     # as before, whatever the window
            assert cls(unet=unet, max_temporal_frames=n, temporal_window=w).max_temporal_frames == n
        for n in (0, -1, 257, 1024, 160.0, None, True):
            with pytest.raises(ValueError, match="max_temporal_frames"):
                cls(unet=unet, max_temporal_frames=n, temporal_window=w)
    for w in WINDOWS_THAT_STREAM:
        for n in (129, 160, 192, 256):
            pipe = cls(unet=unet, max_temporal_frames=n, temporal_window=w)
            assert pipe.max_temporal_frames == n
            assert pipe.temporal_window == ((w, 1) if isinstance(w, int) else tuple(w))
    for w in WINDOWS_THAT_DO_NOT:
        for n in (129, 160, 256):
            with pytest.raises(ValueError, match=r"max_temporal_frames must be an integer in 1 \.\. 128, or up to 256 with "
                                                 r"temporal_window=\(radius <= 32, anchor <= 32\), got " + str(n)):
                cls(unet=unet, max_temporal_frames=n, temporal_window=w)
    with pytest.raises(ValueError, match="max_temporal_frames"):      # pinned: no window, 129 frames
        cls(unet=unet, max_temporal_frames=129)
    with pytest.raises(ValueError, match="temporal_window"):          # the window's own validation is what it was
        cls(unet=unet, max_temporal_frames=160, temporal_window=(4, 129))
    assert cls(unet=unet, temporal_window=(4, 128)).temporal_window == (4, 128)


@pytest.mark.parametrize("which", (0, 1, 2))
def test_from_pretrained_forwards_both_keywords(which, monkeypatch, tmp_path):
    from mofa_video_amd import clip, vae
    monkeypatch.setattr(vae.AutoencoderKLTemporalDecoder, "from_pretrained", classmethod(lambda cls, *a, **k: "vae"))
    monkeypatch.setattr(clip.CLIPVisionModelWithProjection, "from_pretrained", classmethod(lambda cls, *a, **k: "enc"))
    cls, unet = _pipes()[which], types.SimpleNamespace(device="cpu")
    pipe = cls.from_pretrained(str(tmp_path), unet=unet, temporal_window=12, max_temporal_frames=192)
    assert (pipe.temporal_window, pipe.max_temporal_frames) == ((12, 1), 192)
    for kw in (dict(max_temporal_frames=192), dict(max_temporal_frames=192, temporal_window=40), dict(max_temporal_frames=257, temporal_window=12)):
        with pytest.raises(ValueError, match="max_temporal_frames"):
            cls.from_pretrained(str(tmp_path), unet=unet, **kw)


def test_check_call_past_128_frames():
    Flow = _pipes()[0]
    unet = types.SimpleNamespace(device="cpu")
    Flow(unet=unet, max_temporal_frames=256, temporal_window=12)._check_call(1, 1, 3.0, 129)
    Flow(unet=unet, max_temporal_frames=256, temporal_window=(32, 32))._check_call(1, 1, 3.0, 256)
    Flow(unet=unet, max_temporal_frames=192, temporal_window=12)._check_call(1, 1, 3.0, 161)
    with pytest.raises(ValueError, match=r"^257 frames per forward pass: the temporal attention kernel handles at most 256 \(use "
                                         r"KeypointFlowControlNetPipeline's window loop for long clips\)$"):
        Flow(unet=unet, max_temporal_frames=256, temporal_window=12)._check_call(1, 1, 3.0, 257)
    with pytest.raises(ValueError, match="temporal attention kernel handles at most 192"):
        Flow(unet=unet, max_temporal_frames=192, temporal_window=12)._check_call(1, 1, 3.0, 193)
    # the messages for 32 / 64 / 128 are what they were, with and without a window
    for kw in (dict(), dict(temporal_window=12)):
        with pytest.raises(ValueError, match=r"^129 frames per forward pass: the temporal attention kernel handles at most 32 \(use "
                                             r"KeypointFlowControlNetPipeline's window loop for long clips, or build the pipeline with "
                                             r"max_temporal_frames=\.\.\. up to 128\)$"):
            Flow(unet=unet, **kw)._check_call(1, 1, 3.0, 129)
        with pytest.raises(ValueError, match=r"handles at most 64 \(use KeypointFlowControlNetPipeline's window loop for long clips, or "
                                             r"build the pipeline with max_temporal_frames=\.\.\. up to 128\)$"):
            Flow(unet=unet, max_temporal_frames=64, **kw)._check_call(1, 1, 3.0, 129)
        with pytest.raises(ValueError, match=r"handles at most 128 \(use KeypointFlowControlNetPipeline's window loop for long clips\)$"):
            Flow(unet=unet, max_temporal_frames=128, **kw)._check_call(1, 1, 3.0, 129)


def test_sharded_layouts_and_parallel_limits_still_hold():
    from mofa_video_amd.parallel import FrameParallel, GroupedWindowParallel, Layout, WindowParallel
    Flow = _pipes()[0]
    unet = types.SimpleNamespace(device="cpu", config=types.SimpleNamespace(num_frames=25))
    T = 160
    kw = dict(unet=unet, temporal_window=12, max_temporal_frames=256)
    for par in (FrameParallel(Layout(4, 0, T), None), FrameParallel(Layout(2, 1, T, cfg_ranks=1), None), GroupedWindowParallel(None, 0, 8, 4, T)):
        with pytest.raises(ValueError, match="no per-query mask"):
            Flow(parallel=par, **kw)._check_call(1, 1, 3.0, T)
    # parallel objects that do not shard frames take a window, but keep their own limit on the frames of a forward pass
    for par in (FrameParallel(Layout(2, 1, T), None), WindowParallel(None, 0, 4), types.SimpleNamespace()):
        Flow(parallel=par, **kw)._check_call(1, 1, 3.0, 32)
        with pytest.raises(ValueError, match="sharded over ranks are limited to 32"):
            Flow(parallel=par, **kw)._check_call(1, 1, 3.0, T)
    with pytest.raises(ValueError, match="at most max_key_slots = 128"):
        Flow(parallel=types.SimpleNamespace(max_key_slots=128), **kw)._check_call(1, 1, 3.0, T)


def test_blocks_dispatch_by_clip_length(monkeypatch):
    """a temporal layer under ``c.local``: T = 128 goes to ``ops.attn_temporal_local``, T = 130 to
    ``ops.attn_temporal_local_stream``; the layer's other launches replaced by stand-ins that keep the shapes"""
    from mofa_video_amd import blocks, ops
    assert blocks.LOCAL_STREAM_ABOVE == 128
    C, heads, HW, B = 64, 1, 2, 1
    calls = []

    def spy(name):
        def op(q, k, v, nclips, T, hw, h, head_dim=64, local=None):
            calls.append((name, nclips, T, hw, h, head_dim, local))
            raise _Reached()
        return op

    class _Reached(Exception):
        pass
    monkeypatch.setattr(ops, "attn_temporal_local", spy("local"))
    monkeypatch.setattr(ops, "attn_temporal_local_stream", spy("stream"))
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
    for T, want in ((128, "local"), (130, "stream"), (32, "local"), (256, "stream")):
        c = types.SimpleNamespace(N=B * T, T=T, B=B, par=None, local=(12, 1))
        with pytest.raises(_Reached):
            blk(torch.zeros(B * T * HW, C), c, 1, HW)
        assert calls.pop() == (want, B, T, HW, heads, 64, (12, 1)) and not calls
    c = types.SimpleNamespace(N=B * 130, T=130, B=B, par=None, local=None)
    with pytest.raises(_Reached):
        blk(torch.zeros(B * 130 * HW, C), c, 1, HW)
    assert calls.pop()[0] == "dense"


# ---- the resource report -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_stream_instantiations_use_no_scratch():
    """exactly two instantiations (head dim 64 / 128, one wave per workgroup), neither with scratch or a spilled register"""
    rows = {}
    for n, r in _usage("attention.hip").items():
        m = re.match(r"_Z\d+attn_temporal_stream_local_kernelILi(\d+)ELi(\d+)EE", n)
        if m:
            rows[tuple(int(x) for x in m.groups())] = r
    assert set(rows) == {(64, 1), (128, 1)}, sorted(rows)
    for inst, r in rows.items():
        assert (r["ScratchSize"], r["VGPRs Spill"], r["SGPRs Spill"]) == (0, 0, 0), (inst, r)
