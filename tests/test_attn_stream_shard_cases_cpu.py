"""Frame-sharded clips past 128 key slots (streaming attention on a rank's keys), the part that needs no GPU: the case table of
tests/attn_stream_shard_cases.py holds what it claims; its stand-in, which walks a sequence tile by tile with a running maximum as
the kernel does, passes every case under the bound the GPU test applies, and each wrong slot-space rule (mutant) misses it on a
listed case; the entry point mofa_attn_temporal_stream_shard_f16 is declared, exported, bound and refuses every violated rule of
both modes before any device call; ``ops.attn_temporal_stream_shard`` (refusals before the library loads, the TIMER row); the
``stream_keys`` keyword of ``FrameParallel`` / ``GroupedWindowParallel`` / ``pipeline._check_call``; the routing in ``blocks``; the
resource report of the two instantiations; and one temporal block over gloo against the unsharded block.
tests/test_attn_temporal_stream_shard_gpu.py runs the same cases through the HIP kernel."""
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
import attn_stream_shard_cases as sh
import attn_window_cases as wc
from test_no_scratch_cpu import HIPCC, _usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mofa_attn_temporal_stream_shard_f16"
PARAMS = ["q", "k", "v", "out", "nclips", "Tq", "S", "HW", "heads", "head_dim", "ld", "ldkv", "ldo", "scale", "radius", "anchor", "q_frame0",
          "band_frame0", "key_mask", "stream"]


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    sh.release()
    lc.release()


# ---- 1. the table ----------------------------------------------------------------------------------------------------------------
def test_table_holds_what_it_claims():
    sh.assert_table()
    assert len(sh.DENSE_CASES) <= 200 and len(sh.WINDOW_CASES) == 34
    ids = [c.id for c in sh.dense_cases() + sh.window_cases()]
    assert len(ids) == len(set(ids))
    for T, n in {(c[1], c[2]) for c in sh.WINDOW_CASES}:
        from mofa_video_amd.parallel import split_frames
        assert wc.bounds(T, n) == split_frames(T, n)


def test_slot_rule_names_the_visible_frames_of_the_whole_clip():
    """per shard and query: the visible slots name exactly the frames the rule on the whole clip makes visible, each once"""
    for T, n, r, a in sh.LAYOUTS:
        whole = lc.visible(T, r, a)
        for s in range(n):
            g = wc.geometry(T, n, r, a, s)
            vis, frames = sh.slot_visible(g.S, g.Tq, (r, a), g.f0, g.b0, None), wc.slot_frames(g, a)
            for i in range(0, g.Tq, 7):
                seen = [frames[j] for j in range(g.S) if vis[i, j]]
                assert seen and len(seen) == len(set(seen)), (T, n, r, a, s, i)
                assert sorted(seen) == torch.nonzero(whole[g.f0 + i]).flatten().tolist(), (T, n, r, a, s, i)


# ---- 2. the stand-in -------------------------------------------------------------------------------------------------------------
STAND_IN = types.SimpleNamespace(**{sh.OP: sh.stand_in})


def _through(module, cases, what):
    top, errs = 0.0, []
    for case in cases:
        worst, e = sh.check(case, sh.run(module, case))
        top, errs = max(top, worst), errs + e
    print(f"ATTN-STREAM-SHARD stand-in {what}: {len(cases)} cases, worst err / bound {top:.3f}")
    return errs


@pytest.mark.parametrize("S", sorted({c[1] for c in sh.DENSE_CASES}))
def test_dense_cases_pass_through_the_stand_in(S):
    errs = _through(STAND_IN, [c for c in sh.dense_cases() if c.S == S], f"dense S{S}")
    assert not errs, errs[:5]


@pytest.mark.parametrize("layout", sh.LAYOUTS)
def test_window_cases_pass_through_the_stand_in(layout):
    errs = _through(STAND_IN, [c for c in sh.window_cases() if c.key[1:5] == layout], f"window {layout}")
    assert not errs, errs[:5]


def test_stand_in_has_the_signature_of_the_op():
    from mofa_video_amd import ops
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items() if not n.startswith("_")]   # noqa: E731
    assert sig(ops.attn_temporal_stream_shard) == sig(sh.stand_in)
    assert list(inspect.signature(ops.attn_temporal_stream_shard).parameters) == \
        ["q", "k", "v", "nclips", "S", "HW", "heads", "head_dim", "scale", "out", "Tq", "local", "q_frame0", "band_frame0", "key_mask"]


# ---- 3. mutants --------------------------------------------------------------------------------------------------------------------
MUTANT_LAYOUTS = ((256, 4, 48, 1), (256, 2, 31, 33), (200, 2, 33, 0))


@pytest.mark.parametrize("defect", sh.MUTANTS)
def test_mutants_are_told_apart(defect):
    """each wrong slot-space rule of tests/attn_window_cases.py, walked by the stand-in, misses the bound (or leaves a query
    without a slot) on a listed case"""
    caught = []
    for case in [c for c in sh.window_cases() if c.key[0] == 64 and c.key[1:5] in MUTANT_LAYOUTS]:
        try:
            worst, errs = sh.check(case, sh.run(sh.mutant(defect), case))
        except AssertionError as e:
            assert "a query that sees no slot" in str(e)
            errs = [str(e)]
        if errs:
            caught.append(case.key)
    print(f"ATTN-STREAM-SHARD mutant {defect}: misses the bound on {caught}")
    assert caught, f"mutant {defect} passes every listed case"
    want = {"duplicates": lambda c: c[5] == 0 and c[4] > 0, "slot-distance": lambda c: c[5] > 0 and c[3] > 0,
            "no-anchor": lambda c: c[4] > 0, "strict": lambda c: c[3] > 0}[defect]
    assert all(want(c) for c in caught), (defect, caught)


# ---- 4. / 5. C ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    from mofa_video_amd import _build, lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mofa_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", hdr)
    assert m, f"{NAME} is not declared in include/mofa_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == PARAMS, params
    _build.build()
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), NAME)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert lib.PROTOTYPES[NAME] == [P, P, P, P, I, I, I, I, I, I, I, I, I, F, I, I, I, I, P, P]


def test_every_violated_rule_is_refused_without_a_device():
    """one violated rule at a time on otherwise valid (never dereferenced) addresses: -22 before any HIP call (there is no GPU
    here: a launch attempt would return MOFA_ELAUNCH instead).  The valid calls are not made: they would reach the device"""
    from mofa_video_amd import lib
    fn = getattr(lib.load(), NAME)
    A = 0x10000
    common = [dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(S=0), dict(S=-3), dict(S=1025), dict(S=2048), dict(S=1 << 30),
              dict(head_dim=80), dict(head_dim=32), dict(head_dim=0), dict(head_dim=256), dict(ld=132), dict(ldkv=12), dict(ldo=12),
              dict(ldo=150), dict(ld=0), dict(ldkv=0), dict(ldo=-8), dict(nclips=0), dict(nclips=-1), dict(HW=0), dict(HW=-4), dict(heads=0),
              dict(heads=-2), dict(Tq=0), dict(Tq=-1), dict(radius=-2), dict(radius=-(1 << 31))]
    # window mode at S > 128: band frames 12 .. 170 (L = 159 slots behind one anchor slot), queries 60 .. 109
    good = dict(q=A, k=A, v=A, out=A, nclips=1, Tq=50, S=160, HW=4, heads=2, head_dim=64, ld=128, ldkv=136, ldo=144, scale=0.125, radius=48,
                anchor=1, q_frame0=60, band_frame0=12, key_mask=None, stream=None)
    assert list(good) == PARAMS
    words = (ctypes.c_uint32 * 32)(*([0xffffffff] * 32))
    window = [dict(key_mask=words),                                     # a mask in window mode
              dict(anchor=-1), dict(anchor=161), dict(anchor=1025), dict(band_frame0=-1), dict(band_frame0=-12, q_frame0=-4),
              dict(q_frame0=11), dict(q_frame0=0), dict(q_frame0=-1),
              dict(q_frame0=122),                                       # queries 122 .. 171: one past the band's last frame 170
              dict(Tq=160),                                             # more queries than band slots (L = 159)
              dict(Tq=112),                                             # 60 .. 171
              dict(anchor=63),                                          # L = 97: the band 12 .. 108 ends before the last query (62 holds it)
              dict(anchor=160, Tq=1, q_frame0=12),                      # L = 0: no band slot for the query's own frame
              dict(band_frame0=(1 << 30) + 1, q_frame0=(1 << 30) + 1), dict(band_frame0=2 ** 31 - 8, q_frame0=2 ** 31 - 8)]
    for bad in common + window:
        kw = dict(good)
        kw.update(bad)
        assert fn(*kw.values()) == -22, ("window", bad)
    for S, Tq in ((1, 1), (128, 128), (129, 129), (1024, 1024)):        # every slot count refuses alike
        for bad in (dict(Tq=Tq + 1), dict(anchor=S + 1), dict(anchor=1), dict(q_frame0=1), dict(band_frame0=1), dict(radius=-2),
                    dict(key_mask=words)):
            kw = dict(good, S=S, Tq=Tq, anchor=0, q_frame0=0, band_frame0=0)
            kw.update(bad)
            assert fn(*kw.values()) == -22, (S, bad)
    # dense mode
    dense = dict(good, radius=-1, anchor=0, q_frame0=0, band_frame0=0, Tq=33, S=161)
    empty = (ctypes.c_uint32 * 32)()
    beyond = (ctypes.c_uint32 * 32)(*([0] * 5 + [0xfffffffe] + [0xffffffff] * 26))     # S = 161: bit 0 of word 5 is the last slot
    mixups = [dict(anchor=1), dict(anchor=-1), dict(q_frame0=1), dict(band_frame0=1), dict(q_frame0=-1), dict(band_frame0=-1),
              dict(q_frame0=3, band_frame0=3)]
    for bad in common + mixups + [dict(key_mask=empty), dict(key_mask=beyond), dict(Tq=(1 << 30) + 1)]:
        kw = dict(dense)
        kw.update(bad)
        assert fn(*kw.values()) == -22, ("dense", bad)
    for S in (1, 32, 33, 1024):                                         # a mask whose only bits lie at or above S
        high = (ctypes.c_uint32 * 32)()
        if S < 1024:
            high[S // 32] = (0xffffffff << (S % 32)) & 0xffffffff
            assert fn(*dict(dense, S=S, Tq=1, key_mask=high).values()) == -22, S
        assert fn(*dict(dense, S=S, Tq=1, key_mask=empty).values()) == -22, S


# ---- 6. / 7. the op ------------------------------------------------------------------------------------------------------------------
def test_op_refuses_before_the_library_loads(monkeypatch):
    from mofa_video_amd import lib, ops

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(lib, "load", no_load)
    q = torch.zeros(160 * 2, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match=r"window mode \(local=\(radius, anchor\)\) takes no key_mask"):
        ops.attn_temporal_stream_shard(q, q, q, 1, 160, 2, 1, Tq=8, local=(48, 1), q_frame0=60, band_frame0=12, key_mask=0xff)
    with pytest.raises(ValueError, match="no per-query mask"):
        ops.attn_temporal_stream_shard(q, q, q, 1, 160, 2, 1, local=(48, 0), key_mask=(1 << 160) - 1)
    with pytest.raises(ValueError, match="needs radius >= 0"):
        ops.attn_temporal_stream_shard(q, q, q, 1, 160, 2, 1, local=(-1, 0))
    for kw in (dict(q_frame0=4), dict(band_frame0=4), dict(q_frame0=4, band_frame0=4, key_mask=3)):
        with pytest.raises(ValueError, match="dense mode .* takes no q_frame0 / band_frame0"):
            ops.attn_temporal_stream_shard(q, q, q, 1, 160, 2, 1, Tq=8, **kw)
    with pytest.raises(ValueError, match="key_mask must be a non-negative integer"):
        ops.attn_temporal_stream_shard(q, q, q, 1, 160, 2, 1, Tq=8, key_mask=-1)
    for kw in (dict(), dict(key_mask=5), dict(Tq=8), dict(Tq=8, local=(48, 1), q_frame0=60, band_frame0=12)):
        with pytest.raises(AssertionError, match="the library was loaded"):                # the valid calls go on to the library
            ops.attn_temporal_stream_shard(q, q, q, 1, 160, 2, 1, **kw)


def test_op_timer_row_counts_visible_pairs(monkeypatch):
    from mofa_video_amd import lib, ops
    rows, seen = [], []
    timer = types.SimpleNamespace(start=lambda: 1, stop=lambda name, t0, **kw: rows.append((name, kw)))
    monkeypatch.setattr(lib, "load", lambda: types.SimpleNamespace(**{NAME: lambda *a: seen.append(a) or 0}))
    monkeypatch.setattr(lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(ops, "TIMER", timer)
    HW, heads = 2, 1
    # dense: Tq x live slots; the words the library receives are the mask's, ceil(S / 32) of them
    S, Tq = 161, 33
    k, q = torch.zeros(S * HW, 64, dtype=torch.float16), torch.zeros(Tq * HW, 64, dtype=torch.float16)
    for kind in ("full", "lay3", "alt", "first", "tile-mid-dead"):
        m, live = sh.mask_kinds(S)[kind]
        out = torch.zeros(Tq * HW, 64, dtype=torch.float16)
        assert ops.attn_temporal_stream_shard(q, k, k, 1, S, HW, heads, out=out, Tq=Tq, key_mask=m) is out
        a = seen.pop()
        assert a[4:18] == (1, Tq, S, HW, heads, 64, 64, 64, 64, 0.125, -1, 0, 0, 0) and not seen
        if m is None:
            assert a[18] is None
        else:
            assert len(a[18]) == 6 and sum(int(w) << (32 * i) for i, w in enumerate(a[18])) == m
        name, kw = rows.pop()
        assert name == "attn_temporal_stream_kernel" and kw["flops"] == 4.0 * Tq * len(live) * 64 * HW and not rows
    # window: the visible (query, slot) pairs of the rule
    for case in sh.WINDOW_CASES[::4]:
        _, T, n, r, a_, s = case
        g = wc.geometry(T, n, r, a_, s)
        k, q = torch.zeros(g.S * HW, 64, dtype=torch.float16), torch.zeros(g.Tq * HW, 64, dtype=torch.float16)
        ops.attn_temporal_stream_shard(q, k, k, 1, g.S, HW, heads, Tq=g.Tq, local=(r, a_), q_frame0=g.f0, band_frame0=g.b0)
        a = seen.pop()
        assert a[4:19] == (1, g.Tq, g.S, HW, heads, 64, 64, 64, 64, 0.125, r, a_, g.f0, g.b0, None)
        name, kw = rows.pop()
        pairs = int(sh.slot_visible(g.S, g.Tq, (r, a_), g.f0, g.b0, None).sum())
        assert name == "attn_temporal_stream_kernel" and kw["flops"] == 4.0 * pairs * 64 * HW, case


# ---- 8. stream_keys ------------------------------------------------------------------------------------------------------------------
def _par(T, n, s, **kw):
    from mofa_video_amd.parallel import FrameParallel, Layout
    return FrameParallel(Layout(n, s, T, cfg_ranks=1), None, **kw)


def test_max_key_slots_range_with_and_without_the_keyword():
    from mofa_video_amd.parallel import GroupedWindowParallel
    assert _par(40, 4, 0).stream_keys is False and _par(40, 4, 0, stream_keys=True).stream_keys is True
    for n in (32, 64, 128):
        for sk in (False, True):
            assert _par(40, 4, 0, max_key_slots=n, stream_keys=sk).max_key_slots == n
    for n in (129, 256, 1024):
        assert _par(40, 4, 0, max_key_slots=n, stream_keys=True).max_key_slots == n
        for kw in (dict(), dict(stream_keys=False)):
            with pytest.raises(ValueError, match=rf"^max_key_slots must be an integer in 32 \.\. 128, got {n}$"):
                _par(40, 4, 0, max_key_slots=n, **kw)
    for n in (31, 0, -1, 1025, 4096, 64.0, None, True):
        with pytest.raises(ValueError, match=rf"^max_key_slots must be an integer in 32 \.\. 128, got {re.escape(repr(n))}$"):
            _par(40, 4, 0, max_key_slots=n)
        with pytest.raises(ValueError, match=rf"^max_key_slots must be an integer in 32 \.\. 1024 with stream_keys=True, got {re.escape(repr(n))}$"):
            _par(40, 4, 0, max_key_slots=n, stream_keys=True)
    gw = GroupedWindowParallel(None, 5, 8, 4, 256, max_key_slots=256, window_keys=True, stream_keys=True)
    assert gw.stream_keys is True and gw.frame.stream_keys is True and gw.max_key_slots == gw.frame.max_key_slots == 256
    assert gw.frame.window_plan(48, 1).S == 1 + 128 + 48                # 2 CFG halves x 2 frame shards of 128: the last shard
    gw = GroupedWindowParallel(None, 5, 8, 4, 40)
    assert gw.stream_keys is False and gw.frame.stream_keys is False
    with pytest.raises(ValueError, match=r"in 32 \.\. 128, got 256"):
        GroupedWindowParallel(None, 5, 8, 4, 256, max_key_slots=256)


def test_window_plan_under_the_keyword():
    for T, n, r, a in sh.LAYOUTS:
        for s in range(n):
            g = wc.geometry(T, n, r, a, s)
            p = _par(T, n, s, window_keys=True, stream_keys=True).window_plan(r, a)
            assert (p.b0, p.b1, p.S, p.own) == (g.b0, g.b1, g.S, g.own), (T, n, r, a, s)
            assert p.own + g.Tq <= p.S <= 1024 and p.own >= a
            assert (p.recv_prev, p.recv_next, p.recv_anchor) == (r if s > 0 else 0, r if s + 1 < n else 0, a if s > 0 else 0)
        t_max = wc.bounds(T, n)[0][1]
        if a + t_max + 2 * min(r, T - 1) > 128:                        # without the keyword: today's refusal, character for character
            with pytest.raises(ValueError, match=rf"^window_plan: anchor \+ T_max \+ 2 radius = {a} \+ {t_max} \+ 2 x {r} = "
                                                 rf"{a + t_max + 2 * r} key slots exceed the attention kernel's 128$"):
                _par(T, n, 0, window_keys=True).window_plan(r, a)
    assert _par(1024, 2, 0, window_keys=True, stream_keys=True).window_plan(255, 2).S == 2 + 512 + 255      # 2 + 512 + 510 = 1024
    with pytest.raises(ValueError, match=r"^window_plan: anchor \+ T_max \+ 2 radius = 3 \+ 512 \+ 2 x 255 = 1025 key slots exceed the "
                                         r"streaming attention kernel's 1024$"):
        _par(1024, 2, 0, window_keys=True, stream_keys=True).window_plan(255, 3)
    with pytest.raises(ValueError, match="without window_keys=True"):                       # stream_keys alone opens no window path
        _par(256, 4, 1, stream_keys=True).window_plan(48, 1)
    with pytest.raises(ValueError, match=r"radius 65 exceeds the smallest frame shard \(64 of 256 frames over 4 shards\)"):
        _par(256, 4, 1, window_keys=True, stream_keys=True).window_plan(65, 1)
    # up to 128 slots the plan is the plan of an object without the keyword
    a, b = _par(128, 4, 1, window_keys=True).window_plan(31, 1), _par(128, 4, 1, window_keys=True, stream_keys=True).window_plan(31, 1)
    assert vars(a) == vars(b)


def test_check_call_outcomes():
    from mofa_video_amd.parallel import FrameParallel, GroupedWindowParallel, Layout, WindowParallel
    from mofa_video_amd.pipeline import FlowControlNetPipeline as Flow
    unet = types.SimpleNamespace(device="cpu", config=types.SimpleNamespace(num_frames=25))
    mk = lambda T, world=4, **kw: FrameParallel(Layout(world, 0, T), None, **kw)    # noqa: E731  (2 CFG halves x world / 2 frame shards)
    dense = dict(unet=unet, max_temporal_frames=256, temporal_stream=True)
    # dense: stream_keys and max_key_slots large enough
    for T in (129, 160, 256):
        Flow(parallel=mk(T, stream_keys=True, max_key_slots=256), **dense)._check_call(1, 1, 3.0, T)
        Flow(parallel=GroupedWindowParallel(None, 0, 8, 4, T, max_key_slots=256, stream_keys=True), **dense)._check_call(1, 1, 3.0, T)
        with pytest.raises(ValueError, match=rf"^{T} frames per forward pass with parallel=\.\.\.: this parallel object takes clips of at most "
                                             rf"max_key_slots = 128 frames \(more than 128 frames: build it with stream_keys=True and "
                                             rf"max_key_slots >= {T}\)$"):
            Flow(parallel=mk(T, max_key_slots=128), **dense)._check_call(1, 1, 3.0, T)
        with pytest.raises(ValueError, match=r"at most max_key_slots = 128 frames$"):          # the keyword is there: the slots are named
            Flow(parallel=mk(T, max_key_slots=128, stream_keys=True), **dense)._check_call(1, 1, 3.0, T)
        with pytest.raises(ValueError, match=r"sharded over ranks are limited to 32 frames \(their gathered keys carry a 32-bit mask\); run "
                                             r"long clips on one device$"):
            Flow(parallel=mk(T, stream_keys=True), **dense)._check_call(1, 1, 3.0, T)
    with pytest.raises(ValueError, match=r"^100 frames per forward pass with parallel=\.\.\.: this parallel object takes clips of at most "
                                         r"max_key_slots = 64 frames$"):                       # up to 128 frames: the text of before
        Flow(parallel=mk(100, max_key_slots=64), **dense)._check_call(1, 1, 3.0, 100)
    # the constructor's own limits stay: 256 frames per pass, and past 128 only under temporal_stream or a ring-eligible window
    with pytest.raises(ValueError, match=r"^257 frames per forward pass: the temporal attention kernel handles at most 256"):
        Flow(parallel=mk(257, stream_keys=True, max_key_slots=512), **dense)._check_call(1, 1, 3.0, 257)
    with pytest.raises(ValueError, match="max_temporal_frames must be an integer"):
        Flow(unet=unet, parallel=mk(160, stream_keys=True, max_key_slots=256), max_temporal_frames=160)
    with pytest.raises(ValueError, match="temporal attention kernel handles at most 128"):
        Flow(unet=unet, parallel=mk(160, stream_keys=True, max_key_slots=256), max_temporal_frames=128)._check_call(1, 1, 3.0, 160)
    # window
    win = dict(unet=unet, max_temporal_frames=256, temporal_window=(48, 1), temporal_stream=True)
    Flow(parallel=mk(256, 8, window_keys=True, stream_keys=True), **win)._check_call(1, 1, 3.0, 256)
    Flow(parallel=GroupedWindowParallel(None, 0, 16, 8, 256, window_keys=True, stream_keys=True), **win)._check_call(1, 1, 3.0, 256)
    Flow(parallel=mk(256, 8, window_keys=True, stream_keys=True), unet=unet, max_temporal_frames=256,
         temporal_window=(32, 1))._check_call(1, 1, 3.0, 256)                                  # a ring-eligible window needs no temporal_stream
    with pytest.raises(ValueError, match=r"^window_plan: anchor \+ T_max \+ 2 radius = 1 \+ 64 \+ 2 x 48 = 161 key slots exceed the attention "
                                         r"kernel's 128 \(a parallel object built with stream_keys=True takes up to 1024 key slots\)$"):
        Flow(parallel=mk(256, 8, window_keys=True), **win)._check_call(1, 1, 3.0, 256)
    with pytest.raises(ValueError, match=r"frame-sharded clips has no per-query mask \(a CFG split alone and WindowParallel are fine\)$"):
        Flow(parallel=mk(256, 8, stream_keys=True, max_key_slots=256), **win)._check_call(1, 1, 3.0, 256)
    with pytest.raises(ValueError, match="radius 48 exceeds the smallest frame shard"):
        Flow(parallel=mk(160, 8, window_keys=True, stream_keys=True), **win)._check_call(1, 1, 3.0, 160)
    with pytest.raises(ValueError, match="the parallel object's layout shards 256"):
        Flow(parallel=mk(256, 8, window_keys=True, stream_keys=True), **win)._check_call(1, 1, 3.0, 200)
    # objects that do not shard frames are what they were
    for par in (WindowParallel(None, 0, 4), types.SimpleNamespace()):
        with pytest.raises(ValueError, match="sharded over ranks are limited to 32"):
            Flow(parallel=par, **dense)._check_call(1, 1, 3.0, 160)


# ---- 9. routing in blocks ------------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _routing_block(monkeypatch, calls):
    from mofa_video_amd import blocks, ops

    def spy(name):
        def op(q, k, v, nclips, S, hw, h, **kw):
            calls.append((name, (q.shape[0], k.shape[0], v.shape[0]), nclips, S, hw, h, kw))
            raise _Reached()
        return op
    monkeypatch.setattr(ops, "attn_temporal_window", spy("window"))
    monkeypatch.setattr(ops, "attn_temporal_sharded", spy("sharded"))
    monkeypatch.setattr(ops, "attn_temporal_stream_shard", spy("stream_shard"))
    for n in ("attn_temporal", "attn_temporal_local", "attn_temporal_local_stream", "attn_temporal_stream"):
        monkeypatch.setattr(ops, n, spy(n))
    monkeypatch.setattr(ops, "attn_spatial", lambda q, *a, **kw: q)
    monkeypatch.setattr(ops, "lin320_fits", lambda *a: False)
    monkeypatch.setattr(ops, "igemm", lambda x, w, *a, **kw: torch.cat([x, x], 1))
    monkeypatch.setattr(ops, "copy2d", lambda src, dst: dst.copy_(src))
    ident = lambda x, *a, **kw: x                                        # noqa: E731
    C = 64
    blk = object.__new__(blocks.TransformerSpatioTemporal)
    blk.C, blk.heads = C, 1
    blk._invariants = lambda c: (None, None, None)
    blk.norm, blk.proj_in, blk.norm1, blk.norm3, blk.norm_in, blk.tnorm1 = (ident,) * 6
    attn = types.SimpleNamespace(can_fuse_norm=False, qkv=lambda h: (h, h, h), q=ident, to_out=ident, head_dim=64, q_prescaled=False,
                                 wqkv=torch.zeros(3 * C, 1), kv_into=lambda fn, own: None)
    blk.attn1, blk.tattn1 = attn, attn
    for n in ("ff", "ff_in"):
        f = lambda x, *a, **kw: x                                        # noqa: E731
        f.can_fuse = False
        setattr(blk, n, f)
    return blk


def _routed(blk, calls, par, local, HW=2):
    done = types.SimpleNamespace(wait=lambda: None)
    par.window_begin = lambda buf, rows: done
    par.kv_gather_begin = lambda buf, rows: done
    par.gather_frames = lambda t, rows: torch.zeros(par.T_full * rows, t.shape[1], dtype=t.dtype)
    c = types.SimpleNamespace(N=par.T_loc, T=par.T_loc, B=1, par=par, local=local)
    with pytest.raises(_Reached):
        blk(torch.zeros(par.T_loc * HW, blk.C, dtype=torch.float16), c, 1, HW)
    call = calls.pop()
    assert not calls
    return call


def test_blocks_route_by_slot_count_and_keyword(monkeypatch):
    """128 slots or fewer: the calls of before with their arguments, with or without ``stream_keys``; more than 128 slots on a
    ``stream_keys`` object: ``ops.attn_temporal_stream_shard`` with the same arguments"""
    calls, HW = [], 2
    blk = _routing_block(monkeypatch, calls)
    # the window branch
    for T, n, s, r, a, kw, want in ((128, 4, 1, 31, 1, dict(), "window"), (128, 4, 1, 31, 1, dict(stream_keys=True), "window"),
                                    (130, 2, 1, 12, 2, dict(stream_keys=True), "window"), (256, 4, 1, 48, 1, dict(stream_keys=True), "stream_shard"),
                                    (256, 4, 0, 48, 1, dict(stream_keys=True), "window"),            # shard 0: 113 slots
                                    (256, 2, 0, 31, 33, dict(stream_keys=True), "stream_shard"), (1024, 8, 7, 64, 1, dict(stream_keys=True), "stream_shard")):
        par, g = _par(T, n, s, window_keys=True, **kw), wc.geometry(T, n, r, a, s)
        assert (g.S > 128) == (want == "stream_shard")
        got = _routed(blk, calls, par, (r, a))
        assert got == (want, (g.Tq * HW, g.S * HW, g.S * HW), 1, g.S, HW, 1,
                       dict(head_dim=64, Tq=g.Tq, local=(r, a), q_frame0=g.f0, band_frame0=g.b0)), (T, n, s, got)
    # the two in-place gather branches and the compacting branch
    for T, n, slots, kw, want, S in ((128, 4, 128, dict(), "sharded", 128), (128, 4, 128, dict(stream_keys=True), "sharded", 128),
                                     (100, 3, 128, dict(stream_keys=True), "sharded", 102), (160, 4, 256, dict(stream_keys=True), "stream_shard", 160),
                                     (130, 3, 132, dict(stream_keys=True), "stream_shard", 132), (250, 4, 1024, dict(stream_keys=True), "stream_shard", 252)):
        for hidden in (True, False):
            par = _par(T, n, 1, max_key_slots=slots, **kw)
            par.gather_hidden = hidden
            assert par.kv_slots == S
            got = _routed(blk, calls, par, None)
            assert got == (want, (par.T_loc * HW, S * HW, S * HW), 1, S, HW, 1, dict(head_dim=64, Tq=par.T_loc, key_mask=par.kv_mask)), (T, n, got)
    for T, n, slots, kw, want in ((128, 3, 128, dict(), "sharded"), (128, 3, 128, dict(stream_keys=True), "sharded"),
                                  (130, 3, 128, dict(stream_keys=True), "stream_shard"), (250, 4, 250, dict(stream_keys=True), "stream_shard"),
                                  (130, 3, 128, dict(), "sharded")):            # (without the keyword the C entry refuses 130 slots, as before)
        par = _par(T, n, 1, max_key_slots=slots, **kw)
        assert par.kv_slots > slots
        got = _routed(blk, calls, par, None)
        assert got == (want, (par.T_loc * HW, T * HW, T * HW), 1, T, HW, 1, dict(head_dim=64, Tq=par.T_loc)), (T, n, got)
    par = _par(160, 4, 1, max_key_slots=256, stream_keys=True)
    par.kv_inplace = False                                               # the in-place path failed its self-check: compact
    got = _routed(blk, calls, par, None)
    assert got[0] == "stream_shard" and got[3] == 160 and got[6] == dict(head_dim=64, Tq=40)


# ---- 10. the resource report ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_shard_instantiations_use_no_scratch_at_the_stream_kernel_occupancy():
    """exactly two instantiations (head dim 64 with four waves per workgroup, 128 with two): no scratch -- the 32 mask words are
    indexed by the running tile and must not become a private array --, no spilled register, and the occupancy [waves / SIMD] of
    attn_temporal_stream_kernel at the same (head dim, waves per workgroup)"""
    rows = {"stream": {}, "stream_shard": {}}
    for n, r in _usage("attention.hip").items():
        m = re.match(r"_Z\d+attn_temporal_(stream|stream_shard)_kernelILi(\d+)ELi(\d+)EE", n)
        if m:
            rows[m.group(1)][(int(m.group(2)), int(m.group(3)))] = r
    assert set(rows["stream_shard"]) == set(rows["stream"]) == {(64, 4), (128, 2)}, rows
    for inst, r in rows["stream_shard"].items():
        assert (r["ScratchSize"], r["VGPRs Spill"], r["SGPRs Spill"]) == (0, 0, 0), (inst, r)
        assert r["Occupancy"] == rows["stream"][inst]["Occupancy"] == {(64, 4): 2, (128, 2): 1}[inst], (inst, r, rows["stream"][inst])


# ---- 11. gloo: one temporal block on stand-ins ----------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _block_worker(rank, world, port, T, hd, local):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sharded_long_checks as sc
        import window_shard_checks as ws
        from helpers import rel_l2
        from mofa_video_amd import ops
        from mofa_video_amd.parallel import FrameParallel, Layout, TorchComm
        ws.install_stand_ins()
        ops.attn_temporal_stream = lc.stand_in                          # the whole clip under a window beyond the ring's limits
        torch.set_num_threads(2)
        calls = []

        def spy(q, k, v, nclips, S, HW, heads, **kw):
            calls.append((S, kw.get("Tq"), kw.get("local"), kw.get("q_frame0", 0), kw.get("band_frame0", 0), kw.get("key_mask")))
            return sh.stand_in(q, k, v, nclips, S, HW, heads, **kw)
        ops.attn_temporal_stream_shard = spy
        for n in ("attn_temporal_sharded", "attn_temporal_window"):

            def old(*a, _n=n, **kw):
                raise AssertionError(f"{_n} was called for more than 128 key slots")
            setattr(ops, n, old)
        lay = Layout(world, rank, T, cfg_ranks=1)
        par = FrameParallel(lay, TorchComm(lambda r: Layout(world, r, T, cfg_ranks=1)), max_key_slots=256, window_keys=local is not None,
                            stream_keys=True)
        if local is not None:
            report = par.self_check("cpu")
            assert report["window"] == "batched p2p + anchor broadcast" and par.window_p2p, report
        par.log = []
        blk = sc.make_block(hd, "cpu")
        x, emb = sc.block_inputs(blk, T, "cpu")
        HW = sc.H * sc.W
        mine = x[lay.f0 * HW:lay.f1 * HW]
        if local is None:
            ref = sc.run_block(blk, x, emb, T)[lay.f0 * HW:lay.f1 * HW]
            got = sc.run_block(blk, mine, emb, lay.T_loc, par)
            assert calls == [(par.kv_slots, lay.T_loc, None, 0, 0, par.kv_mask)], (rank, calls)
            assert par.kv_slots == lay.frame_ranks * lay.T_max > 128
        else:
            ref = ws.run_block(blk, x, emb, T, local)[lay.f0 * HW:lay.f1 * HW]
            got = ws.run_block(blk, mine, emb, lay.T_loc, local, par)
            assert calls == [ws.expected_call(T, world, *local, rank) + (None,)], (rank, calls)
            assert calls[0][0] > 128 and par.log == [(0, "window")], (calls, par.log)
        e = rel_l2(got, ref)
        assert got.shape == ref.shape and e < 2e-3, (rank, e)
        errs = [None] * world
        dist.all_gather_object(errs, e)
        if rank == 0:
            print(f"stream-keys sharded temporal block, {T} frames over {world} shards, window {local}, head dim {hd}: rel-L2 per rank",
                  ["%.2e" % v for v in errs])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,T,hd,local", [(4, 132, 64, None), (3, 130, 128, None), (2, 140, 64, (31, 33))])
def test_stream_keys_sharded_temporal_block_gloo(world, T, hd, local):
    """one TransformerSpatioTemporal block on frames-only shards built with ``stream_keys=True`` against the block on the whole
    clip, on torch stand-ins: dense 4 x 33 frames (132 slots, every one live), dense 44 + 43 + 43 (132 slots, two of them padding:
    the mask of ``kv_mask``), and 70 + 70 frames under the window (31, 33) (134 slots on both ranks; the plan's bound anchor +
    T_max + 2 radius is 165).  Every rank's attention goes through ``ops.attn_temporal_stream_shard``, once, with the arguments
    the layout dictates.  The stated bound of the sharded path, rel-L2 2e-3 (tests/test_sharded_long_cpu.py)"""
    mp.spawn(_block_worker, args=(world, _free_port(), T, hd, local), nprocs=world, join=True)
