"""More than 32 frames per forward pass, the part that needs no GPU: the new entry point mofa_attn_temporal_long_f16 is declared,
exported, bound and validates its arguments before any device call; ``ops.attn_temporal`` refuses a long masked / sharded call
before it loads the library; the pipelines' ``max_temporal_frames`` keyword; the UNet host graph at T = 40 on the torch stand-ins
(no hidden 32-frame assumption in blocks.py / unet.py); and the case tables of tests/attn_long_cases.py through the stand-in, with
mutants that prove the checks can fail."""
import ctypes
import os
import re
import types

import pytest
import torch

import attn_cases as ac
import attn_long_cases as lc
import emu_ops
from helpers import TINY, oracle_models, rel_l2, synthetic_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mofa_attn_temporal_long_f16"


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    from mofa_video_amd import _build, lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mofa_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", hdr)
    assert m, f"{NAME} is not declared in include/mofa_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 14 and [p.split()[-1].lstrip("*") for p in params] == \
        ["q", "k", "v", "out", "nclips", "T", "HW", "heads", "head_dim", "ld", "ldkv", "ldo", "scale", "stream"], params
    _build.build()
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), NAME)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert lib.PROTOTYPES[NAME] == [P, P, P, P, I, I, I, I, I, I, I, I, F, P]


def test_every_invalid_argument_is_refused_without_a_device():
    """one violated rule at a time on otherwise valid (never dereferenced) addresses: -22 before any HIP call (there is no GPU
    here: a launch attempt would return MOFA_ELAUNCH instead)"""
    from mofa_video_amd import lib
    fn = getattr(lib.load(), NAME)
    A = 0x10000
    good = dict(q=A, k=A, v=A, out=A, nclips=1, T=40, HW=4, heads=2, head_dim=64, ld=128, ldkv=136, ldo=144, scale=0.125, stream=None)
    bads = [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(T=0), dict(T=-3), dict(T=129), dict(T=256),
            dict(head_dim=80), dict(head_dim=32), dict(head_dim=0), dict(head_dim=256), dict(ld=132), dict(ldkv=12), dict(ldo=12),
            dict(ldo=150), dict(ld=0), dict(nclips=0), dict(nclips=-1), dict(HW=0), dict(HW=-4), dict(heads=0), dict(heads=-2)]
    for T in (1, 32, 33, 128):                                       # (the valid call is not made: it would reach the device)
        for bad in bads:
            kw = dict(good, T=T)
            kw.update(bad)
            assert fn(*kw.values()) == -22, (T, bad)


def test_long_masked_or_sharded_call_is_refused_before_the_library_loads(monkeypatch):
    from mofa_video_amd import lib, ops

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(lib, "load", no_load)
    q = torch.zeros(40 * 2, 64, dtype=torch.float16)
    for kw in (dict(key_mask=0xffffffff), dict(key_mask=1), dict(Tq=8), dict(Tq=39, key_mask=3)):
        with pytest.raises(ValueError, match="frame-sharded clips are limited to 32 key slots"):
            ops.attn_temporal(q, q, q, 1, 40, 2, 1, **kw)
    with pytest.raises(AssertionError, match="the library was loaded"):   # T <= 32, and plain T > 32, go on to the library
        ops.attn_temporal(q, q, q, 1, 40, 2, 1)
    with pytest.raises(AssertionError, match="the library was loaded"):
        ops.attn_temporal(q, q, q, 1, 40, 2, 1, Tq=40)


# ---- pipelines ----------------------------------------------------------------------------------------------------------------
def _pipes():
    from mofa_video_amd.pipeline import FlowControlNetPipeline, HybridFlowControlNetPipeline, KeypointFlowControlNetPipeline
    return FlowControlNetPipeline, HybridFlowControlNetPipeline, KeypointFlowControlNetPipeline


@pytest.mark.parametrize("which", (0, 1, 2))
def test_max_temporal_frames_keyword(which):
    cls = _pipes()[which]
    unet = types.SimpleNamespace(device="cpu")
    assert cls(unet=unet).max_temporal_frames == 32
    for n in (1, 32, 33, 128):
        assert cls(unet=unet, max_temporal_frames=n).max_temporal_frames == n
    for n in (0, 129, -1, 40.0, None, True):
        with pytest.raises(ValueError, match="max_temporal_frames"):
            cls(unet=unet, max_temporal_frames=n)


def test_check_call_compares_against_the_keyword():
    Flow = _pipes()[0]
    unet = types.SimpleNamespace(device="cpu")
    Flow(unet=unet, max_temporal_frames=64)._check_call(1, 1, 3.0, 40)
    Flow(unet=unet, max_temporal_frames=64)._check_call(1, 1, 3.0, 64)
    Flow(unet=unet, max_temporal_frames=128)._check_call(1, 1, 3.0, 128)
    Flow(unet=unet)._check_call(1, 1, 3.0, 32)
    with pytest.raises(ValueError, match=r"^40 frames per forward pass: the temporal attention kernel handles at most 32 \(use "
                                         r"KeypointFlowControlNetPipeline's window loop for long clips"):
        Flow(unet=unet)._check_call(1, 1, 3.0, 40)
    with pytest.raises(ValueError, match="temporal attention kernel handles at most 64"):
        Flow(unet=unet, max_temporal_frames=64)._check_call(1, 1, 3.0, 65)
    with pytest.raises(ValueError, match="temporal attention kernel handles at most 128"):
        Flow(unet=unet, max_temporal_frames=128)._check_call(1, 1, 3.0, 129)
    # sharded clips keep the 32-key-slot limit whatever the keyword says; up to 32 frames they are untouched by it
    par = types.SimpleNamespace()
    with pytest.raises(ValueError, match="sharded over ranks are limited to 32"):
        Flow(unet=unet, parallel=par, max_temporal_frames=64)._check_call(1, 1, 3.0, 40)
    Flow(unet=unet, parallel=par, max_temporal_frames=64)._check_call(1, 1, 3.0, 32)


def test_keypoint_window_size_is_governed_by_the_keyword():
    """the window loop checks ``window_size`` -- its frames per forward pass -- at entry, before it touches a model"""
    Keypoint = _pipes()[2]
    unet = types.SimpleNamespace(device="cpu", config=types.SimpleNamespace(num_frames=25))
    with pytest.raises(ValueError, match="temporal attention kernel handles at most 32"):
        Keypoint(unet=unet)(None, window_size=40, stride=21, num_frames=61, height=64, width=64)
    with pytest.raises(ValueError, match=r"num_frames \(39\) must be at least window_size \(40\)"):    # past the frame check
        Keypoint(unet=unet, max_temporal_frames=64)(None, window_size=40, stride=21, num_frames=39, height=64, width=64)


# ---- the host graph at T = 40 ---------------------------------------------------------------------------------------------------
def test_unet_host_graph_at_40_frames_matches_oracle(monkeypatch):
    """tests/test_unet_host_cpu.py's comparison at T = 40 (64 x 64 pixels): GroupNorm over the clip, conv (3,1,1), the frame
    position embedding and the temporal attention's reshapes carry no 32-frame assumption"""
    from mofa_video_amd import ops
    from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
    emu_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "TIMER", None)
    T, H, W = 40, 64, 64
    torch.manual_seed(0)
    ou, oc, ov, sdu, sdc, sdv = oracle_models(TINY, seed=3)
    hu = UNetSpatioTemporalConditionControlNetModel(sdu, config=TINY, device="cpu")
    inp = synthetic_inputs(T, H, W, cross_dim=TINY["cross_attention_dim"], seed=7)
    x = torch.cat([torch.cat([inp["latents"]] * 2), inp["image_latents"].unsqueeze(1).repeat(1, T, 1, 1, 1)], dim=2)
    t, ids = torch.tensor(0.8), torch.tensor([[6.0, 128.0, 0.02]] * 2)
    boc, h, w = TINY["block_out_channels"], H // 8, W // 8
    shapes = [(boc[0], h, w)] * 3 + [(boc[0], h // 2, w // 2)] + [(boc[1], h // 2, w // 2)] * 2 + \
             [(boc[1], h // 4, w // 4)] + [(boc[2], h // 4, w // 4)] * 2 + [(boc[2], h // 8, w // 8)] + \
             [(boc[3], h // 8, w // 8)] * 2
    g = torch.Generator().manual_seed(11)
    res = [(torch.randn(2 * T, *s, generator=g) * 0.3).half().float() for s in shapes]
    mid = (torch.randn(2 * T, boc[3], h // 8, w // 8, generator=g) * 0.3).half().float()
    with torch.no_grad():
        ref = ou(x, t, inp["image_embeddings"], down_block_additional_residuals=res, mid_block_additional_residual=mid,
                 return_dict=False, added_time_ids=ids)[0]
    got = hu(x, t, inp["image_embeddings"], down_block_additional_residuals=res, mid_block_additional_residual=mid,
             return_dict=False, added_time_ids=ids)[0]
    e = rel_l2(got, ref)
    print(f"UNet host graph at T = {T}: rel-L2 {e:.3e}")
    assert tuple(got.shape) == tuple(ref.shape) == (2, T, 4, H // 8, W // 8)
    assert e < 1e-2, e


# ---- the case tables through the stand-in, and mutants that must fail -------------------------------------------------------------
def test_case_tables_hold_what_they_are_for():
    assert {33, 63, 64, 65, 95, 96, 97, 127, 128} <= set(lc.LONG_T) and min(lc.LONG_T) > 32 and max(lc.LONG_T) == 128
    for T in lc.LONG_T:
        lc.assert_selection_perm(T)
    seqs = [HW * heads * clips for HW, heads, clips in lc.LONG_GEOM]
    assert 1 in seqs and any(s % 2 for s in seqs) and any(s % 4 and s > 4 for s in seqs)     # partly empty last workgroups
    assert any(g[2] == 2 for g in lc.LONG_GEOM)
    c = lc.COUNT_C * 128
    assert c == int(c) and lc.COUNT_C < 4
    assert lc.ulp16(1 / 33) == 2.0 ** -16 and lc.ulp16(1 / 128) == 2.0 ** -17 and lc.ulp16(1.0) == 2.0 ** -10


FORMS = ("gauss", "select", "count-one", "count-c")


@pytest.mark.parametrize("T", (33, 64, 97, 128))
@pytest.mark.parametrize("hd", lc.LONG_HD)
def test_cases_pass_through_the_stand_in(hd, T):
    for HW, heads, clips in lc.LONG_GEOM:
        for form in FORMS + (("phantom-plain", "phantom-decoy") if clips == 2 else ()):
            case = lc.long_case(form, T, hd, HW, heads, clips)
            worst, errs = lc.check_long(case, lc.run(emu_ops, case))
            assert not errs, errs
    lc.release()


def _wrong_long(defect):
    """fp64 temporal attention over all T keys with one defect of attn_cases._softmax_pv (None: the plain truth); swap-v
    exchanges key 0 with key 37, one tile further on"""
    def attn_temporal(q, k, v, nclips, T, HW, heads, head_dim=64, scale=None, out=None, Tq=None, key_mask=None):
        assert Tq in (None, T) and key_mask is None
        Q, K, V = (t.double().reshape(nclips, T, HW, heads, head_dim).permute(0, 2, 3, 1, 4) for t in (q, k, v))
        o = ac._softmax_pv(Q @ K.transpose(-1, -2) * (head_dim ** -0.5 if scale is None else scale), V, defect, T, 32, (0, 37))
        out[:] = ac._pack_temporal(o).half()
        return out
    return types.SimpleNamespace(attn_temporal=attn_temporal)


@pytest.mark.parametrize("defect,caught_by", [("phantom", ("gauss", "count-one", "count-c")), ("drop-last", ("gauss", "select", "count-one")),
                                              ("swap-v", ("gauss", "select"))])
def test_mutants_are_caught(defect, caught_by):
    """fp64 attention with one defect (attn_cases._softmax_pv): a zero key too many, the last key dropped, two keys exchanged
    on the V side only.  Each family that can see the defect must report it"""
    T, hd, (HW, heads, clips) = 65, 64, lc.LONG_GEOM[1]
    truth, mutant = _wrong_long(None), _wrong_long(defect)
    for form in FORMS:
        case = lc.long_case(form, T, hd, HW, heads, clips)
        assert not lc.check_long(case, lc.run(truth, case))[1], form
        errs = lc.check_long(case, lc.run(mutant, case))[1]
        assert bool(errs) == (form in caught_by), (defect, form, errs[:2])
    lc.release()
