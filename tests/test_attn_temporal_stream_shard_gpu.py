"""mofa_attn_temporal_stream_shard_f16 (csrc/attention.hip attn_temporal_stream_shard_kernel) on the GPU, driven through
``ops.attn_temporal_stream_shard`` on the cases of tests/attn_stream_shard_cases.py (tests/test_attn_stream_shard_cases_cpu.py
proves the table on the CPU): every case on guarded views against float64 of the whole clip under the dense kernel's bound, with
the guard cells of ``out`` unchanged; the four bit equalities the kernel's header states; the exact families; repeat launches; the
shards of a clip together against the whole clip; and one temporal block on four virtual ranks (``parallel.ThreadComm``: N ranks
as N threads on one GPU) built with ``stream_keys=True`` against the unsharded block.  Nothing here runs on more than one GPU.

Virtual ranks against the single rank: rel-L2 < 2e-3 tensor-wide and for every frame, max|delta| / max|ref| of every frame below
``ABS`` -- the bounds of tests/test_sharded_long_gpu.py and tests/test_attn_window_gpu.py, for their reason (the same arithmetic up
to the summation order of the attention's keys: slot s of a rank's buffer is not frame s of the clip)."""
import threading

import pytest
import torch

import attn_cases as ac
import attn_local_cases as lc
import attn_stream_shard_cases as sh
import attn_window_cases as wc
import sharded_long_checks as sc
import window_shard_checks as ws
from helpers import check_frames, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
HW = sh.HW
ABS = 3.5e-3               # per-frame max|delta| / max|ref| vs single rank: the bar of tests/test_sharded_long_gpu.py


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


@pytest.fixture(scope="module", autouse=True)
def _release_case_data():
    yield
    sh.release()
    lc.release()


def _through(ops, cases, what):
    top, errs = 0.0, []
    for case in cases:
        worst, e = sh.check(case, sh.run(ops, case, DEV))
        top, errs = max(top, worst), errs + e
    print(f"ATTN-STREAM-SHARD {what}: {len(cases)} cases, worst err / bound {top:.3f}")
    assert cases and not errs, errs[:5]


# ---- 1. every table case against fp64, on guarded views ----------------------------------------------------------------------------
@pytest.mark.parametrize("S", sorted({c[1] for c in sh.DENSE_CASES}))
def test_dense_cases_against_fp64(ops, S):
    _through(ops, [c for c in sh.dense_cases() if c.S == S and c.form == "gauss"], f"dense S{S}")


@pytest.mark.parametrize("layout", sh.LAYOUTS)
def test_window_cases_against_fp64(ops, layout):
    _through(ops, [c for c in sh.window_cases() if c.key[1:5] == layout], f"window {layout}")


# ---- 3. the exact families ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sh.FORMS[1:])
def test_exact_families(ops, form):
    """select: the output equals one live v row element for element; count-one: 1 / L to one fp16 ulp; count-c: exact"""
    _through(ops, [c for c in sh.dense_cases() if c.form == form], form)


# ---- 2. the bit-level anchors ------------------------------------------------------------------------------------------------------
def _dev(d):
    return d.q.to(DEV), d.k.to(DEV), d.v.to(DEV)


@pytest.mark.parametrize("D,S", [(64, 129), (64, 161), (64, 257), (64, 1024), (128, 129), (128, 257)])
def test_anchors_a_b_c_equal_the_whole_clip_kernel(ops, D, S):
    """(a) dense, no mask, Tq == S: ``ops.attn_temporal_stream`` dense; (b) Tq < S on q rows f0 .. f0 + Tq - 1: those rows of (a),
    whatever the alignment of the 32-query blocks; (c) window with anchor 0 and both frames 0: the stream kernel under (radius, 0)"""
    d = sh.dense_data(D, S, S, "full", "plain", "gauss")
    q, k, v = _dev(d)
    kw = dict(head_dim=D)
    whole = ops.attn_temporal_stream(q, k, v, d.clips, S, HW, d.heads, **kw)
    assert torch.equal(ops.attn_temporal_stream_shard(q, k, v, d.clips, S, HW, d.heads, **kw), whole), "(a)"
    assert torch.equal(ops.attn_temporal_stream_shard(q, k, v, d.clips, S, HW, d.heads, Tq=S, key_mask=(1 << S) - 1, **kw), whole), "(a), full mask"
    w3 = whole.reshape(d.clips, S, HW, -1)
    q3 = q.reshape(d.clips, S, HW, -1)
    for f0, Tq in ((0, 33), (37, 45), (S - 1, 1), (64, S - 64), (1, 32)):
        part = ops.attn_temporal_stream_shard(q3[:, f0:f0 + Tq].reshape(-1, q.shape[1]), k, v, d.clips, S, HW, d.heads, Tq=Tq, **kw)
        assert torch.equal(part.reshape(d.clips, Tq, HW, -1), w3[:, f0:f0 + Tq]), ("(b)", f0, Tq)
    for r in (15, 33, 48, S - 1, S + 7):
        assert torch.equal(ops.attn_temporal_stream_shard(q, k, v, d.clips, S, HW, d.heads, local=(r, 0), **kw),
                           ops.attn_temporal_stream(q, k, v, d.clips, S, HW, d.heads, local=(r, 0), **kw)), ("(c)", r)


@pytest.mark.parametrize("D,S,Tq", [(64, 161, 33), (64, 257, 65), (128, 257, 32), (64, 1024, 33)])
def test_anchor_d_dead_slot_contents_change_no_bit(ops, D, S, Tq):
    """NaN, decoy keys with NaN values and zeros in the K / V rows of dead slots: equal bits"""
    for kind in ("lay3", "alt", "tile-mid-dead", "pad-edges", "first", "last"):
        outs = []
        for fill in ("nan", "decoy-nan"):
            d = sh.dense_data(D, S, Tq, kind, fill, "gauss")
            outs.append(ops.attn_temporal_stream_shard(*_dev(d), d.clips, S, HW, d.heads, head_dim=D, **d.kw))
        dead = torch.tensor([j not in set(d.live) for j in range(S)])
        k0, v0 = (t.reshape(d.clips, S, HW, -1).masked_fill(dead[None, :, None, None], 0.0).reshape(t.shape).to(DEV) for t in (d.k, d.v))
        outs.append(ops.attn_temporal_stream_shard(d.q.to(DEV), k0, v0, d.clips, S, HW, d.heads, head_dim=D, **d.kw))
        assert bool(torch.isfinite(outs[0]).all()), kind
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (S, kind)


# ---- 4. repeat launches ------------------------------------------------------------------------------------------------------------
def test_two_launches_on_the_same_buffers_give_equal_bits(ops):
    for case in (sh.dense_case(64, 257, 65, "lay4", "nan", "gauss"), sh.window_case(64, 256, 4, 48, 1, 1), sh.window_case(128, 200, 2, 33, 0, 1)):
        d = case.data()
        q, k, v = _dev(d)
        out = torch.full((d.expect.shape[0], d.expect.shape[1]), float("nan"), dtype=torch.float16, device=DEV)
        assert ops.attn_temporal_stream_shard(q, k, v, d.clips, case.S, HW, d.heads, head_dim=case.hd, out=out, **d.kw) is out
        first = out.clone()
        ops.attn_temporal_stream_shard(q, k, v, d.clips, case.S, HW, d.heads, head_dim=case.hd, out=out, **d.kw)
        assert torch.equal(out, first), case.id
        assert torch.equal(ops.attn_temporal_stream_shard(q, k, v, d.clips, case.S, HW, d.heads, head_dim=case.hd, **d.kw), first), case.id


# ---- 5. the shards together cover the clip -----------------------------------------------------------------------------------------
def test_window_shards_cover_the_clip(ops):
    D, T, n, r, a = 64, 256, 4, 48, 1
    q, k, v = wc.operands(D, T, 1)
    P = ac._pack_temporal
    outs = []
    for s in range(n):
        g = wc.geometry(T, n, r, a, s)
        outs.append(ops.attn_temporal_stream_shard(P(q[..., g.f0:g.f1, :]).to(DEV), P(wc.slot_rows(k, g, a)).to(DEV), P(wc.slot_rows(v, g, a)).to(DEV),
                                                   1, g.S, HW, lc.HEADS[D], head_dim=D, Tq=g.Tq, local=(r, a), q_frame0=g.f0, band_frame0=g.b0).cpu())
    worst, msg = sh.close_errors(torch.cat(outs), P(wc.expectation(D, T, r, a, 1)), sh.BOUND, "window shards, concatenated")
    print(f"ATTN-STREAM-SHARD window shards of {T} frames over {n}: worst err / bound {worst:.3f}")
    assert msg is None, msg


def test_dense_shards_cover_the_clip(ops):
    """250 frames over 4 shards: the gathered buffer (252 slots, NaN in the two padding slots) under ``kv_mask`` against fp64 of
    the whole clip; and with compacted keys (250 slots, no mask) the rows of ``ops.attn_temporal_stream`` on the whole clip, bit
    for bit"""
    from mofa_video_amd.parallel import FrameParallel, Layout
    D, T, n = 64, 250, 4
    heads = lc.HEADS[D]
    q, k, v = lc.operands(D, T, 1)
    P = ac._pack_temporal
    whole = ops.attn_temporal_stream(P(q).to(DEV), P(k).to(DEV), P(v).to(DEV), 1, T, HW, heads, head_dim=D).reshape(T, HW, -1)
    pars = [FrameParallel(Layout(n, s, T, cfg_ranks=1), None, max_key_slots=256, stream_keys=True) for s in range(n)]
    t_max, slots = pars[0].lay.T_max, pars[0].kv_slots
    assert slots == 252 and len({p.kv_mask for p in pars}) == 1
    gk, gv = (torch.full((*t.shape[:3], slots, D), float("nan"), dtype=torch.float16) for t in (k, v))
    for s, (a, b) in enumerate(pars[0].lay.bounds):
        gk[..., s * t_max:s * t_max + (b - a), :], gv[..., s * t_max:s * t_max + (b - a), :] = k[..., a:b, :], v[..., a:b, :]
    outs = []
    for p in pars:
        mine = P(q[..., p.f0:p.f1, :]).to(DEV)
        outs.append(ops.attn_temporal_stream_shard(mine, P(gk).to(DEV), P(gv).to(DEV), 1, slots, HW, heads, head_dim=D, Tq=p.T_loc,
                                                   key_mask=p.kv_mask).cpu())
        compact = ops.attn_temporal_stream_shard(mine, P(k).to(DEV), P(v).to(DEV), 1, T, HW, heads, head_dim=D, Tq=p.T_loc)
        assert torch.equal(compact.reshape(p.T_loc, HW, -1), whole[p.f0:p.f1]), p.lay.shard
    expect = P(lc.attention64(q, k, v, D ** -0.5, torch.ones(T, T, dtype=torch.bool)))
    worst, msg = sh.close_errors(torch.cat(outs), expect, sh.BOUND, "dense shards, concatenated")
    print(f"ATTN-STREAM-SHARD dense shards of {T} frames over {n}: worst err / bound {worst:.3f}")
    assert msg is None, msg


# ---- 6. virtual ranks --------------------------------------------------------------------------------------------------------------
def _threads(world, fn):
    """fn(rank, ThreadWorld) on ``world`` threads -> the results in rank order"""
    from mofa_video_amd.parallel import ThreadWorld
    tw = ThreadWorld(world)
    results, errors = [None] * world, []

    def worker(r):
        try:
            torch.cuda.set_device(0)
            results[r] = fn(r, tw)
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))
            for b in tw.barriers.values():
                b.abort()
    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors, errors
    return results


@pytest.mark.parametrize("local", (None, (48, 1)))
@pytest.mark.parametrize("hd", (64, 128))
def test_stream_keys_temporal_block_on_virtual_ranks(ops, monkeypatch, hd, local):
    """one TransformerSpatioTemporal block of 160 frames on four virtual ranks -- 2 CFG halves x 2 frame shards of 80 frames, the
    largest shards four ranks give a radius of 48 room in -- built with ``stream_keys=True``, against the unsharded block on the
    same GPU: dense (160 gathered key slots) and under the window (48, 1) (1 + 80 + 48 = 129 slots).  Every rank's attention
    goes through ``ops.attn_temporal_stream_shard``"""
    from mofa_video_amd.parallel import FrameParallel, Layout, ThreadComm
    T, world = 160, 4
    blk = sc.make_block(hd, DEV)
    x, emb = sc.block_inputs(blk, T, DEV)
    HWb = sc.H * sc.W
    run = (lambda xx, t, par=None: sc.run_block(blk, xx, emb, t, par)) if local is None else \
        (lambda xx, t, par=None: ws.run_block(blk, xx, emb, t, local, par))
    ref = run(x, T).reshape(T, HWb * blk.C)
    calls, inner = [], ops.attn_temporal_stream_shard

    def spy(q, k, v, nclips, S, hw, heads, **kw):
        calls.append((S, kw.get("Tq"), kw.get("local"), kw.get("key_mask")))
        return inner(q, k, v, nclips, S, hw, heads, **kw)
    monkeypatch.setattr(ops, "attn_temporal_stream_shard", spy)
    for n in ("attn_temporal_sharded", "attn_temporal_window"):
        monkeypatch.setattr(ops, n, lambda *a, _n=n, **kw: pytest.fail(f"{_n} was called for more than 128 key slots"))

    def rank(r, tw):
        lay = Layout(world, r, T)
        par = FrameParallel(lay, ThreadComm(tw, r), max_key_slots=256, window_keys=local is not None, stream_keys=True)
        return lay, run(x[lay.f0 * HWb:lay.f1 * HWb], lay.T_loc, par)
    outs = _threads(world, rank)
    want_call = (160, 80, None, (1 << 160) - 1) if local is None else (129, 80, local, None)
    assert calls == [want_call] * world, calls
    for r, (lay, o) in enumerate(outs):
        assert lay.T_loc == 80
        o, want = o.reshape(lay.T_loc, HWb * blk.C), ref[lay.f0:lay.f1]
        e = rel_l2(o, want)
        print(f"ATTN-STREAM-SHARD block {T} frames on {world} virtual ranks, window {local}, head dim {hd}, rank {r}: rel-L2 {e:.3e}")
        assert e < 2e-3, (r, e)
        check_frames(o, want, 2e-3, ABS, dim=0, f0=lay.f0, what=f"ATTN-STREAM-SHARD block rank {r}")
