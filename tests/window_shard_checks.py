"""TEST INFRASTRUCTURE ONLY: one TransformerSpatioTemporal block under a temporal window (``Ctx.local``) on a frame shard built
with ``window_keys=True`` against the same windowed block on the whole clip -- shared by the gloo test
(tests/test_attn_window_cpu.py, torch stand-ins) and the virtual-rank GPU test (tests/test_attn_window_gpu.py).  The block, its
inputs and the frames-only layout are those of tests/sharded_long_checks.py."""
import attn_local_cases as lc
import attn_window_cases as wc
import sharded_long_checks as sc


def install_stand_ins():
    """emu_sharded's stand-ins plus the three local ones (whole clip: up to 128 frames and beyond; frame shard)"""
    import emu_sharded
    from mofa_video_amd import ops
    emu_sharded.install()
    ops.attn_temporal_local = lc.stand_in
    ops.attn_temporal_local_stream = lc.stand_in
    ops.attn_temporal_window = wc.stand_in


def run_block(blk, x, emb, T, local, par=None):
    """the block on ``x`` = the T frames this rank holds (all of them without ``par``) under the window ``local``"""
    from mofa_video_amd import blocks
    c = blocks.Ctx(1, T)
    c.ctx16, c.par, c.local = emb, par, local
    return blk(x.contiguous(), c, sc.H, sc.W)


def spy_on_window_attention(calls):
    """wrap ``ops.attn_temporal_window`` so that it records (S, Tq, local, q_frame0, band_frame0) of every call"""
    from mofa_video_amd import ops
    inner = ops.attn_temporal_window

    def spy(q, k, v, nclips, S, HW, heads, head_dim=64, scale=None, out=None, Tq=None, local=None, q_frame0=0, band_frame0=0):
        calls.append((S, Tq, tuple(local), q_frame0, band_frame0))
        return inner(q, k, v, nclips, S, HW, heads, head_dim=head_dim, scale=scale, out=out, Tq=Tq, local=local, q_frame0=q_frame0,
                     band_frame0=band_frame0)
    ops.attn_temporal_window = spy
    return inner


def expected_call(T, shards, radius, anchor, shard):
    g = wc.geometry(T, shards, radius, anchor, shard)
    return (g.S, g.Tq, (radius, anchor), g.f0, g.b0)
