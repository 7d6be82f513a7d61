"""Frame-sharded clips of 33 to 128 frames, the part that needs no GPU: the entry point mofa_attn_temporal_long_masked_f16 is
declared, exported, bound and validates its arguments before any device call; ``ops.attn_temporal_sharded`` hands T <= 32 to
``ops.attn_temporal`` unchanged; ``FrameParallel(max_key_slots=...)`` and what ``pipeline._check_call`` makes of it; the masked
case table of tests/attn_long_masked_cases.py through the stand-in of tests/emu_sharded.py, with mutants of the mask handling
that prove the checks can fail; the sharded temporal block and the whole sharded UNet over gloo at 37 ... 128 frames.  (The
resource report of the kernel's instantiations: tests/test_no_scratch_cpu.py.)"""
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

import attn_long_masked_cases as mc
import emu_sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mofa_attn_temporal_long_masked_f16"


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    from mofa_video_amd import _build, lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mofa_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", hdr)
    assert m, f"{NAME} is not declared in include/mofa_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 16 and [p.split()[-1].lstrip("*") for p in params] == \
        ["q", "k", "v", "out", "nclips", "Tq", "T", "HW", "heads", "head_dim", "ld", "ldkv", "ldo", "scale", "key_mask", "stream"], params
    assert params[14].replace(" ", "") == "constuint32_t*key_mask"
    _build.build()
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), NAME)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert lib.PROTOTYPES[NAME] == [P, P, P, P, I, I, I, I, I, I, I, I, I, F, P, P]


def _words(mask):
    return (ctypes.c_uint32 * 4)(*[(mask >> (32 * w)) & 0xffffffff for w in range(4)])


def test_every_invalid_argument_is_refused_without_a_device():
    """one violated rule at a time on otherwise valid (never dereferenced) tensor addresses: -22 before any HIP call (there is no
    GPU here: a launch attempt would return MOFA_ELAUNCH instead).  The valid call is not made: it would reach the device"""
    from mofa_video_amd import lib
    fn = getattr(lib.load(), NAME)
    A = 0x10000
    good = dict(q=A, k=A, v=A, out=A, nclips=1, Tq=20, T=40, HW=4, heads=2, head_dim=64, ld=128, ldkv=136, ldo=144, scale=0.125,
                key_mask=None, stream=None)
    bads = [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(Tq=0), dict(Tq=-1), dict(T=0), dict(T=129, Tq=129), dict(T=129),
            dict(T=256), dict(head_dim=80), dict(head_dim=32), dict(head_dim=0), dict(head_dim=256), dict(ld=132), dict(ldkv=12),
            dict(ldo=12), dict(ldo=150), dict(ld=0), dict(ldkv=0), dict(ldo=-8), dict(nclips=0), dict(nclips=-1), dict(HW=0), dict(HW=-4),
            dict(heads=0), dict(heads=-2), dict(key_mask=_words(0))]
    for T in (1, 32, 33, 40, 128):
        for bad in bads + [dict(Tq=T + 1), dict(key_mask=_words(((1 << 128) - 1) & ~((1 << T) - 1)))] + \
                ([dict(key_mask=_words(1 << T))] if T < 128 else []):
            kw = dict(good, T=T, Tq=min(20, T))
            kw.update(bad)
            assert fn(*kw.values()) == -22, (T, {k: v for k, v in bad.items() if k != "key_mask"}, list(bad))


# ---- ops --------------------------------------------------------------------------------------------------------------------
def test_stand_in_has_the_signature_of_the_op():
    from mofa_video_amd import ops
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    assert sig(ops.attn_temporal_sharded) == sig(emu_sharded.attn_temporal_sharded) == sig(ops.attn_temporal)
    assert list(inspect.signature(ops.attn_temporal_sharded).parameters) == \
        ["q", "k", "v", "nclips", "T", "HW", "heads", "head_dim", "scale", "out", "Tq", "key_mask"]


def test_up_to_32_slots_go_to_attn_temporal_unchanged(monkeypatch):
    """today's sharded clips keep their kernel: the call is handed over argument for argument, the library is not touched"""
    from mofa_video_amd import lib, ops
    seen = []

    def no_load():
        raise AssertionError("the library was loaded")

    def attn_temporal(*a, **kw):
        seen.append((a, kw))
        return "result"
    monkeypatch.setattr(lib, "load", no_load)
    monkeypatch.setattr(ops, "attn_temporal", attn_temporal)
    q = torch.zeros(8, 64, dtype=torch.float16)
    for T in (1, 25, 32):
        out = object()
        assert ops.attn_temporal_sharded(q, q, q, 1, T, 2, 1, head_dim=64, scale=0.5, out=out, Tq=1, key_mask=5) == "result"
        assert seen[-1] == ((q, q, q, 1, T, 2, 1), dict(head_dim=64, scale=0.5, out=out, Tq=1, key_mask=5))
    with pytest.raises(AssertionError, match="the library was loaded"):      # 33 slots: the new entry point
        ops.attn_temporal_sharded(q, q, q, 1, 33, 2, 1, Tq=1, key_mask=5)
    assert len(seen) == 3


def test_attn_temporal_itself_still_refuses(monkeypatch):
    from mofa_video_amd import ops
    q = torch.zeros(40 * 2, 64, dtype=torch.float16)
    for kw in (dict(key_mask=(1 << 40) - 1), dict(Tq=8)):
        with pytest.raises(ValueError, match="frame-sharded clips are limited to 32 key slots"):
            ops.attn_temporal(q, q, q, 1, 40, 2, 1, **kw)


# ---- parallel / pipeline ------------------------------------------------------------------------------------------------------
def test_frame_parallel_max_key_slots():
    from mofa_video_amd.parallel import FrameParallel, GroupedWindowParallel, Layout
    lay = Layout(4, 1, 40)
    assert FrameParallel(lay, None).max_key_slots == 32
    for n in (32, 33, 64, 128):
        assert FrameParallel(lay, None, max_key_slots=n).max_key_slots == n
        assert FrameParallel(lay, None, True, n).max_key_slots == n
    for n in (31, 0, 129, -1, 64.0, None, True, "64"):
        with pytest.raises(ValueError, match="max_key_slots"):
            FrameParallel(lay, None, max_key_slots=n)
    g = GroupedWindowParallel(None, 5, 8, 4, 40, max_key_slots=64)
    assert g.max_key_slots == g.frame.max_key_slots == 64 and g.frame.lay.T == 40
    assert GroupedWindowParallel(None, 5, 8, 4, 25).max_key_slots == 32
    with pytest.raises(ValueError, match="max_key_slots"):
        GroupedWindowParallel(None, 5, 8, 4, 40, max_key_slots=200)
    # the mask of a long layout is a plain Python int: 37 frames over 4 shards = 10 + 9 + 9 + 9 in slots of 10
    par = FrameParallel(Layout(8, 0, 37), None, max_key_slots=64)
    assert par.kv_slots == 40 and par.kv_mask == sum(((1 << n) - 1) << (10 * s) for s, n in enumerate((10, 9, 9, 9)))
    par = FrameParallel(Layout(3, 0, 128, cfg_ranks=1), None, max_key_slots=128)
    assert par.kv_slots == 129 > par.max_key_slots


def test_check_call_takes_the_smaller_of_the_two_limits():
    from mofa_video_amd.parallel import FrameParallel, GroupedWindowParallel, Layout
    from mofa_video_amd.pipeline import FlowControlNetPipeline as Flow
    unet = types.SimpleNamespace(device="cpu")
    par64 = FrameParallel(Layout(4, 0, 40), None, max_key_slots=64)
    par32 = FrameParallel(Layout(4, 0, 40), None)
    Flow(unet=unet, parallel=par64, max_temporal_frames=64)._check_call(1, 1, 3.0, 40)
    Flow(unet=unet, parallel=par64, max_temporal_frames=64)._check_call(1, 1, 3.0, 64)
    Flow(unet=unet, parallel=par64, max_temporal_frames=128)._check_call(1, 1, 3.0, 64)
    Flow(unet=unet, parallel=GroupedWindowParallel(None, 0, 8, 4, 40, max_key_slots=64), max_temporal_frames=64)._check_call(1, 1, 3.0, 40)
    with pytest.raises(ValueError, match="temporal attention kernel handles at most 64"):
        Flow(unet=unet, parallel=par64, max_temporal_frames=64)._check_call(1, 1, 3.0, 65)
    with pytest.raises(ValueError, match=r"65 frames per forward pass with parallel=\.\.\.: .*max_key_slots = 64"):
        Flow(unet=unet, parallel=par64, max_temporal_frames=128)._check_call(1, 1, 3.0, 65)
    # either keyword at its default: 40 frames are refused, with today's messages
    with pytest.raises(ValueError, match=r"^40 frames per forward pass: the temporal attention kernel handles at most 32"):
        Flow(unet=unet, parallel=par64)._check_call(1, 1, 3.0, 40)
    for par in (par32, types.SimpleNamespace(), GroupedWindowParallel(None, 0, 8, 4, 40)):
        with pytest.raises(ValueError, match=r"sharded over ranks are limited to 32 frames \(their gathered keys carry a 32-bit mask\)"):
            Flow(unet=unet, parallel=par, max_temporal_frames=64)._check_call(1, 1, 3.0, 40)
        Flow(unet=unet, parallel=par, max_temporal_frames=64)._check_call(1, 1, 3.0, 32)


# ---- the masked case table through the stand-in, and mutants that must fail ------------------------------------------------------
def test_mask_table_holds_what_it_is_for():
    mc.assert_mask_table()
    assert [mc.tqs(T) for T in (33, 64, 128)] == [[1, 20, 33], [1, 20, 33, 64], [1, 20, 33, 128]]
    assert any(g[2] == 2 for g in mc.LONG_GEOM)                          # two clips: both clip strides (Tq HW and T HW) are pinned
    d = mc.masked_data("count-one", 65, 20, "lay3", 64, 5, 2, 2)
    assert len(d.live) == 61 and d.q.shape == (2 * 20 * 5, 128) and d.k.shape == (2 * 65 * 5, 128)
    assert bool(torch.isnan(d.k).any()) and bool(torch.isnan(d.v).any())   # dead slots hold NaN rows


@pytest.mark.parametrize("T", mc.MASKED_T)
@pytest.mark.parametrize("hd", mc.LONG_HD)
def test_cases_pass_through_the_stand_in(hd, T):
    n = 0
    for case in mc.cases_of(T, hd):
        worst, errs = mc.check_masked(case, mc.run(emu_sharded, case))
        assert not errs, errs
        n += 1
    assert n == len(mc.tqs(T)) * len(mc.KINDS) * len(mc.LONG_GEOM) * len(mc.FORMS)
    mc.release()


ALL = mc.FORMS
CAUGHT_BY = {  # (mutant, fill of the dead slots' rows) -> the families that must report it (the others must pass)
    ("mask-shift", "nan"): ALL, ("mask-shift", "decoy"): ALL,
    ("swap-words", "nan"): ALL, ("swap-words", "decoy"): ALL,
    ("low-only", "nan"): ALL, ("low-only", "decoy"): ALL,
    # weight 0 times a finite value is 0: only never-written (NaN) rows show a V row that entered the sum
    ("dead-v", "nan"): ALL, ("dead-v", "decoy"): (),
}


@pytest.mark.parametrize("defect,fill", sorted(CAUGHT_BY))
def test_mutants_are_caught(defect, fill):
    """T = 97 under the mask of 4 uneven shards (dead slots 47, 71, 95, 96: the three mask words that matter all differ), 33
    queries, two clips.  Each family that can see the defect must report it; the truth passes every family"""
    T, Tq, hd, (HW, heads, clips) = 97, 33, 64, mc.LONG_GEOM[1]
    assert sorted(set(range(T)) - set(mc.mask_kinds(T)["lay4"][1])) == [47, 71, 95, 96]
    truth, mutant = mc.wrong_sharded(None), mc.wrong_sharded(defect)
    for form in mc.FORMS:
        case = mc.masked_case(form, T, Tq, "lay4", hd, HW, heads, clips, fill)
        assert not mc.check_masked(case, mc.run(truth, case))[1], form
        errs = mc.check_masked(case, mc.run(mutant, case))[1]
        assert bool(errs) == (form in CAUGHT_BY[(defect, fill)]), (defect, fill, form, errs[:2])
    mc.release()


# ---- gloo: the sharded temporal block and the whole UNet ---------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _block_worker(rank, world, port, T, hd, slots):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sharded_long_checks as sc
        from helpers import rel_l2
        from mofa_video_amd.parallel import FrameParallel, Layout, TorchComm
        emu_sharded.install()
        torch.set_num_threads(2)
        calls = []
        sc.spy_on_sharded_attention(calls)
        lay = Layout(world, rank, T, cfg_ranks=1)
        par = FrameParallel(lay, TorchComm(lambda r: Layout(world, r, T, cfg_ranks=1)), max_key_slots=slots)
        blk = sc.make_block(hd, "cpu")
        x, emb = sc.block_inputs(blk, T, "cpu")
        HW = sc.H * sc.W
        ref = sc.run_block(blk, x, emb, T)[lay.f0 * HW:lay.f1 * HW]
        got = sc.run_block(blk, x[lay.f0 * HW:lay.f1 * HW], emb, lay.T_loc, par)
        e = rel_l2(got, ref)
        assert calls == [sc.expected_call(lay, slots)], (rank, calls)
        assert got.shape == ref.shape and e < 2e-3, (rank, e)
        errs = [None] * world
        dist.all_gather_object(errs, e)
        if rank == 0:
            print(f"sharded temporal block, {T} frames over {world} shards, head dim {hd}: rel-L2 per rank", ["%.2e" % v for v in errs])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,T,hd,slots", [(2, 40, 64, 64), (4, 37, 128, 64), (3, 128, 64, 128), (4, 128, 128, 128)])
def test_sharded_long_temporal_block_gloo(world, T, hd, slots):
    """one TransformerSpatioTemporal block on frames-only shards against the block on the whole clip: 20 + 20 frames (40 slots,
    every one live), 10 + 9 + 9 + 9 (40 slots, three of them padding), 43 + 43 + 42 (129 padded slots: more than the limit of 128,
    so the block compacts to 128 frames and calls the attention with Tq = T_loc and no mask) and 4 x 32 (all four key tiles).
    The stated bound of the sharded path, rel-L2 2e-3 (tests/test_parallel_gloo.py: the stand-ins' sgemm blocks by row count)"""
    mp.spawn(_block_worker, args=(world, _free_port(), T, hd, slots), nprocs=world, join=True)


def _unet_worker(rank, world, port, T):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from helpers import TINY, rel_l2
        from mofa_video_amd import ops, schema
        from mofa_video_amd.parallel import FrameParallel, Layout, TorchComm
        from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
        emu_sharded.install()
        torch.set_num_threads(2)
        hu = UNetSpatioTemporalConditionControlNetModel(schema.synthetic_state_dict(schema.unet_schema(TINY), seed=3), config=TINY,
                                                        device="cpu")
        H = W = 64
        h, w = H // 8, W // 8
        g = torch.Generator().manual_seed(5)                       # the same clip on every rank
        x = ops.nchw_to_tokens(torch.randn(2 * T, 8, h, w, generator=g), ld=hu.in_ld)
        emb = torch.randn(2, 1, TINY["cross_attention_dim"], generator=g)
        ids = torch.tensor([[6.0, 128.0, 0.02]] * 2)
        boc = TINY["block_out_channels"]
        dims = [(boc[0], h * w)] * 3 + [(boc[0], h * w // 4)] + [(boc[1], h * w // 4)] * 2 + [(boc[1], h * w // 16)] + \
               [(boc[2], h * w // 16)] * 2 + [(boc[2], h * w // 64)] + [(boc[3], h * w // 64)] * 2
        down = [(torch.randn(2 * T * hw, Cc, generator=g) * 0.3).half() for Cc, hw in dims]
        mid = (torch.randn(2 * T * h * w // 64, boc[3], generator=g) * 0.3).half()
        ref = hu.forward_tokens(x, hu.make_ctx(0.7, emb, ids, 2, T), h, w, down, mid)          # [2 T h w, 4], unsharded
        lay = Layout(world, rank, T)
        par = FrameParallel(lay, TorchComm(lambda r: Layout(world, r, T)), max_key_slots=64)
        assert lay.sharded_frames and par.kv_slots == 40 and bin(par.kv_mask).count("1") == T

        def rows(t):
            hw = t.shape[0] // (2 * T)
            return t[(lay.half * T + lay.f0) * hw:(lay.half * T + lay.f1) * hw]
        c = hu.make_ctx(0.7, emb, ids, 1, lay.T_loc, half=lay.half, par=par)
        out = hu.forward_tokens(rows(x), c, h, w, [rows(d) for d in down], rows(mid))
        e = rel_l2(out, rows(ref))
        assert out.shape == rows(ref).shape and e < 2e-3, (rank, e)
        errs = [None] * world
        dist.all_gather_object(errs, e)
        if rank == 0:
            print(f"sharded UNet forward at {T} frames vs unsharded, rel-L2 per rank:", ["%.2e" % v for v in errs])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,T", [(4, 40), (8, 37)])
def test_sharded_long_unet_forward_gloo(world, T):
    """2-way CFG x {2, 4} frame shards of 20 + 20 / 10 + 9 + 9 + 9 frames (40 key slots, every one live / three of them padding):
    every rank's noise prediction for its frames against the rows of the unsharded forward at 64 x 64 pixels, under the 2e-3
    that tests/test_parallel_gloo.py::test_sharded_unet_forward_gloo states for this comparison on the stand-ins"""
    mp.spawn(_unet_worker, args=(world, _free_port(), T), nprocs=world, join=True)
