"""Local temporal attention (band + anchor frames), the part that needs no GPU: the case table of tests/attn_local_cases.py holds
what it is for, the visibility rule has its stated properties on every listed case, wrong rules (mutants) are told apart from it
by the table, the torch stand-in passes every case under the bound the GPU test applies; the new entry point
mofa_attn_temporal_long_local_f16 is declared, exported, bound and validates its arguments before any device call;
``ops.attn_temporal_local`` refuses a key mask or ``Tq`` before the library loads and the older entries keep their signatures; the
pipelines' ``temporal_window`` keyword and the refusal of frame-sharded layouts.  tests/test_attn_temporal_local_gpu.py runs the same
cases through the HIP kernel; tests/test_no_scratch_cpu.py reads the resource report of its instantiations."""
import ctypes
import os
import re
import types

import pytest
import torch

import attn_local_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mofa_attn_temporal_long_local_f16"


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    lc.release()


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_table_lists_what_it_is_for():
    assert len(lc.CASES) == len(set(lc.CASES)) <= 200
    assert lc.LOCAL_T == (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128)
    for D, T, r, a in lc.CASES:
        assert D in (64, 128) and 1 <= T <= 128 and r >= 0 and 0 <= a <= T, (D, T, r, a)
    d64 = [c for c in lc.CASES if c[0] == 64]
    for T in lc.LOCAL_T:                                               # every valid radius and every valid anchor of every T
        assert {r for _, t, r, _ in d64 if t == T} == {r for r in (0, 1, 15, 16, 31, 32, T - 2, T - 1, 127) if r >= 0}, T
        assert {a for _, t, _, a in d64 if t == T} == {a for a in (0, 1, 2, 33, T) if a <= T}, T
    d128 = [c for c in lc.CASES if c[0] == 128]
    assert d128 and {t for _, t, _, _ in d128} >= {1, 33, 128}
    assert {lc.clips_of(*c) for c in lc.CASES} == {1, 2}
    assert {lc.clips_of(*c) * lc.HW * lc.HEADS[c[0]] for c in lc.CASES} == {5, 10, 20}                # sequences per launch
    assert any(c[0] == 64 and c[1] <= 32 and lc.clips_of(*c) == 1 for c in lc.CASES)                  # 10 over 4 waves per workgroup
    assert any(c[0] == 128 and c[1] <= 32 and lc.clips_of(*c) == 1 for c in lc.CASES)                 # 5 over 2
    assert any(lc.all_visible(*c[1:]) for c in lc.CASES) and any(not lc.all_visible(*c[1:]) for c in lc.CASES)


def test_rule_properties_on_every_case():
    for D, T, r, a in lc.CASES:
        vis = lc.visible(T, r, a)
        assert vis.shape == (T, T) and vis.dtype == torch.bool
        assert bool(vis.diagonal().all()) and bool(vis.any(1).all()), (T, r, a)          # every query sees itself: no empty row
        assert bool(vis.all()) == lc.all_visible(T, r, a), (T, r, a)                      # radius >= T - 1 or anchor == T, nothing else
        assert bool(vis[:, :a].all()), (T, r, a)                                          # anchor columns are full
        band = vis[a:, a:]
        assert torch.equal(band, band.T), (T, r, a)                                       # the band is symmetric
        i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
        assert torch.equal(vis, (j < a) | ((i - j).abs() <= r))


@pytest.mark.parametrize("defect", lc.MUTANTS)
def test_mutants_are_told_apart(defect):
    """a wrong rule differs from the true table on listed cases, and on each of them its float64 attention misses the bound the
    GPU test applies (or has an empty softmax row)"""
    differs = [c for c in lc.CASES if not torch.equal(lc.mutant_visible(defect, *c[1:]), lc.visible(*c[1:]))]
    assert differs, f"mutant {defect} agrees with the rule on every listed case"
    caught = 0
    for D, T, r, a in differs:
        wrong = lc.mutant_visible(defect, T, r, a)
        if not bool(wrong.any(1).all()):                               # an empty row: NaN, caught by the finiteness check
            caught += 1
            continue
        d = lc.local_data(D, T, r, a)
        q, k, v = (lc.split_rows(t, d.clips, T, D) for t in (d.q, d.k, d.v))
        out = lc.ac._pack_temporal(lc.attention64(q, k, v, D ** -0.5, wrong)).half()
        caught += lc.close_errors(out, d.expect, lc.BOUND, f"{defect} {(D, T, r, a)}")[1] is not None
    print(f"ATTN-LOCAL mutant {defect}: differs on {len(differs)} cases, misses the bound on {caught}")
    assert caught == len(differs), (defect, caught, len(differs))


@pytest.mark.parametrize("T", lc.LOCAL_T)
def test_cases_pass_through_the_stand_in(T):
    ops = types.SimpleNamespace(attn_temporal_local=lc.stand_in)
    top = 0.0
    for D, t, r, a in lc.CASES:
        if t != T:
            continue
        d = lc.local_data(D, T, r, a)
        out = ops.attn_temporal_local(d.q, d.k, d.v, d.clips, T, d.HW, d.heads, head_dim=D, local=(r, a))
        assert bool(torch.isfinite(out.float()).all())
        worst, msg = lc.close_errors(out, d.expect, lc.BOUND, f"hd{D} T{T} radius {r} anchor {a}")
        top = max(top, worst)
        assert msg is None, msg
    print(f"ATTN-LOCAL stand-in T{T}: worst err / bound {top:.3f}")


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
    assert lib.PROTOTYPES[NAME] == [P, P, P, P, I, I, I, I, I, I, I, I, F, I, I, P]


def test_every_invalid_argument_is_refused_without_a_device():
    """one violated rule at a time on otherwise valid (never dereferenced) addresses: -22 before any HIP call (there is no GPU
    here: a launch attempt would return MOFA_ELAUNCH instead).  Everything mofa_attn_temporal_long_f16 refuses, and the mask"""
    from mofa_video_amd import lib
    fn = getattr(lib.load(), NAME)
    A = 0x10000
    good = dict(q=A, k=A, v=A, out=A, nclips=1, T=40, HW=4, heads=2, head_dim=64, ld=128, ldkv=136, ldo=144, scale=0.125, radius=4,
                anchor=1, stream=None)
    bads = [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(T=0), dict(T=-3), dict(T=129), dict(T=256),
            dict(head_dim=80), dict(head_dim=32), dict(head_dim=0), dict(head_dim=256), dict(ld=132), dict(ldkv=12), dict(ldo=12),
            dict(ldo=150), dict(ld=0), dict(nclips=0), dict(nclips=-1), dict(HW=0), dict(HW=-4), dict(heads=0), dict(heads=-2),
            dict(radius=-1), dict(radius=-128), dict(anchor=-1)]
    for T in (1, 32, 33, 128):                                       # (the valid call is not made: it would reach the device)
        for bad in bads + [dict(anchor=T + 1), dict(anchor=129)]:
            kw = dict(good, T=T, anchor=min(T, 1))
            kw.update(bad)
            assert fn(*kw.values()) == -22, (T, bad)


# ---- ops ----------------------------------------------------------------------------------------------------------------------
def test_local_with_a_key_mask_or_tq_is_refused_before_the_library_loads(monkeypatch):
    from mofa_video_amd import lib, ops

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(lib, "load", no_load)
    for T in (8, 40):
        q = torch.zeros(T * 2, 64, dtype=torch.float16)
        for kw in (dict(key_mask=0xff), dict(Tq=4), dict(Tq=T), dict(Tq=4, key_mask=3)):
            with pytest.raises(ValueError, match="local temporal attention takes no key_mask and no Tq"):
                ops.attn_temporal_local(q, q, q, 1, T, 2, 1, local=(2, 1), **kw)
        with pytest.raises(ValueError, match=r"local=\(radius, anchor\) is required"):
            ops.attn_temporal_local(q, q, q, 1, T, 2, 1)
        with pytest.raises(AssertionError, match="the library was loaded"):   # the plain local call goes on to the library
            ops.attn_temporal_local(q, q, q, 1, T, 2, 1, local=(2, 1))


def test_older_entry_points_keep_their_signatures():
    """``local`` lives on an entry point of its own: the stand-ins of tests/emu_ops.py mirror these two parameter for parameter"""
    import inspect
    from mofa_video_amd import ops
    old = ["q", "k", "v", "nclips", "T", "HW", "heads", "head_dim", "scale", "out", "Tq", "key_mask"]
    assert list(inspect.signature(ops.attn_temporal).parameters) == old == list(inspect.signature(ops.attn_temporal_sharded).parameters)
    assert list(inspect.signature(ops.attn_temporal_local).parameters) == old + ["local"] == \
        list(inspect.signature(lc.stand_in).parameters)


# ---- blocks / pipelines -----------------------------------------------------------------------------------------------------------
def test_ctx_carries_local_and_refuses_it_with_a_frame_shard():
    from mofa_video_amd import blocks
    assert blocks.Ctx(2, 8).local is None
    net = types.SimpleNamespace(device="cpu", time=lambda ts, ids: None, temb_batch=types.SimpleNamespace(run=lambda a: None))
    base = blocks.Ctx(2, 8)
    base.ctx16 = torch.zeros(2, 4)                                     # (cached: the embedding cast is not under test)
    ids = torch.zeros(2, 3)
    assert blocks.make_ctx(net, 0.5, None, ids, 2, 8, base=base, local=(4, 1)).local == (4, 1)
    assert blocks.make_ctx(net, 0.5, None, ids, 2, 8, base=base).local is None
    with pytest.raises(ValueError, match="no per-query mask"):
        blocks.make_ctx(net, 0.5, None, ids, 2, 8, base=base, par=object(), local=(4, 1))


def _pipes():
    from mofa_video_amd.pipeline import FlowControlNetPipeline, HybridFlowControlNetPipeline, KeypointFlowControlNetPipeline
    return FlowControlNetPipeline, HybridFlowControlNetPipeline, KeypointFlowControlNetPipeline


@pytest.mark.parametrize("which", (0, 1, 2))
def test_temporal_window_keyword(which):
    cls = _pipes()[which]
    unet = types.SimpleNamespace(device="cpu")
    assert cls(unet=unet).temporal_window is None and cls(unet=unet, temporal_window=None).temporal_window is None
    for r in (0, 1, 12, 24, 127, 500):
        assert cls(unet=unet, temporal_window=r).temporal_window == (r, 1)              # an int: frame 0 stays visible
    for r, a in ((0, 0), (4, 1), (12, 2), (127, 128), (32, 0)):
        assert cls(unet=unet, temporal_window=(r, a)).temporal_window == (r, a)
        assert cls(unet=unet, temporal_window=[r, a]).temporal_window == (r, a)
    for bad in (-1, 4.0, True, "4", (4,), (4, 1, 0), (-1, 0), (4, -1), (4, 129), (4.0, 1), (4, True), (None, 1)):
        with pytest.raises(ValueError, match="temporal_window"):
            cls(unet=unet, temporal_window=bad)
    assert cls(unet=unet, temporal_window=4, max_temporal_frames=64).max_temporal_frames == 64


@pytest.mark.parametrize("which", (0, 1, 2))
def test_from_pretrained_forwards_the_keyword(which, monkeypatch, tmp_path):
    """the loaders replaced by stubs (no checkpoint here; no scheduler directory: the default scheduler)"""
    from mofa_video_amd import clip, vae
    monkeypatch.setattr(vae.AutoencoderKLTemporalDecoder, "from_pretrained", classmethod(lambda cls, *a, **k: "vae"))
    monkeypatch.setattr(clip.CLIPVisionModelWithProjection, "from_pretrained", classmethod(lambda cls, *a, **k: "enc"))
    cls, unet = _pipes()[which], types.SimpleNamespace(device="cpu")
    assert cls.from_pretrained(str(tmp_path), unet=unet).temporal_window is None
    assert cls.from_pretrained(str(tmp_path), unet=unet, temporal_window=12).temporal_window == (12, 1)
    assert cls.from_pretrained(str(tmp_path), unet=unet, temporal_window=(24, 0), max_temporal_frames=128).temporal_window == (24, 0)
    with pytest.raises(ValueError, match="temporal_window"):
        cls.from_pretrained(str(tmp_path), unet=unet, temporal_window=-2)


def test_frame_sharded_layouts_are_refused_at_entry():
    from mofa_video_amd.parallel import FrameParallel, GroupedWindowParallel, Layout, WindowParallel
    Flow, _, Keypoint = _pipes()
    unet = types.SimpleNamespace(device="cpu", config=types.SimpleNamespace(num_frames=25))
    T = 24
    sharded = [FrameParallel(Layout(4, 0, T), None), FrameParallel(Layout(2, 1, T, cfg_ranks=1), None),
               GroupedWindowParallel(None, 0, 8, 4, T)]
    allowed = [None, FrameParallel(Layout(2, 1, T), None), WindowParallel(None, 0, 4), GroupedWindowParallel(None, 0, 4, 2, T)]
    for par in sharded:
        with pytest.raises(ValueError, match="no per-query mask"):
            Flow(unet=unet, parallel=par, temporal_window=4)._check_call(1, 1, 3.0, T)
        Flow(unet=unet, parallel=par)._check_call(1, 1, 3.0, T)                           # dense: as before
    for par in allowed:
        Flow(unet=unet, parallel=par, temporal_window=4)._check_call(1, 1, 3.0, T)
    with pytest.raises(ValueError, match="no per-query mask"):                            # the whole call stops at entry
        Flow(unet=unet, parallel=sharded[0], temporal_window=4)(None, height=64, width=64, num_frames=T)
    with pytest.raises(ValueError, match="no per-query mask"):
        Keypoint(unet=unet, parallel=sharded[2], temporal_window=(4, 1))(None, window_size=T, stride=11, num_frames=46, height=64,
                                                                          width=64)
    with pytest.raises(ValueError, match="anchor 30 exceeds the 24 frames"):
        Flow(unet=unet, temporal_window=(4, 30))._check_call(1, 1, 3.0, T)
