"""TEST INFRASTRUCTURE ONLY: one TransformerSpatioTemporal block (blocks.py) on a frame shard of a long clip against the same
block on the whole clip -- shared by the gloo test (tests/test_sharded_long_cpu.py, torch stand-ins) and the virtual-rank GPU
test (tests/test_sharded_long_gpu.py).  Frames-only layout (``cfg_ranks=1``) with one clip per rank (B = 1), as the sharded
norm + convolution block test of tests/test_parallel_gloo.py."""
import torch

from helpers import TINY

# (state-dict prefix of a TINY UNet transformer, heads): 64 channels / 1 head and 256 channels / 2 heads = head dims 64 and 128
BLOCKS = {64: ("down_blocks.0.attentions.0.", 1), 128: ("down_blocks.2.attentions.0.", 2)}
H = W = 4


def make_block(head_dim, device, seed=3):
    from mofa_video_amd import blocks, schema
    prefix, heads = BLOCKS[head_dim]
    sd = schema.synthetic_state_dict(schema.unet_schema(TINY), seed=seed)
    blk = blocks.TransformerSpatioTemporal(blocks.Sub(sd, prefix, device), heads)
    assert blk.C // heads == head_dim
    return blk


def block_inputs(blk, T, device, seed=21):
    """-> x fp16 [T * H * W, C] (the whole clip), the image embedding fp16 [1, cross_dim]"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T * H * W, blk.C, generator=g) * 0.8).half().to(device)
    emb = torch.randn(1, TINY["cross_attention_dim"], generator=g).half().to(device)
    return x, emb


def run_block(blk, x, emb, T, par=None):
    """the block on ``x`` = the T frames this rank holds (all of them without ``par``)"""
    from mofa_video_amd import blocks
    c = blocks.Ctx(1, T)
    c.ctx16, c.par = emb, par
    return blk(x.contiguous(), c, H, W)


def spy_on_sharded_attention(calls):
    """wrap ``ops.attn_temporal_sharded`` (whatever is installed there) so that it records (T, Tq, key_mask) of every call"""
    from mofa_video_amd import ops
    inner = ops.attn_temporal_sharded

    def spy(q, k, v, nclips, T, HW, heads, head_dim=64, scale=None, out=None, Tq=None, key_mask=None):
        calls.append((T, Tq, key_mask))
        return inner(q, k, v, nclips, T, HW, heads, head_dim=head_dim, scale=scale, out=out, Tq=Tq, key_mask=key_mask)
    ops.attn_temporal_sharded = spy
    return inner


def expected_call(lay, max_key_slots):
    """what the temporal block must ask of the attention for this layout: the gathered buffer in place with its mask, or -- more
    padded slots than the limit -- the compacted T_full frames without one"""
    slots = lay.frame_ranks * lay.T_max
    if slots <= max_key_slots:
        mask = 0
        for s, (a, b) in enumerate(lay.bounds):
            mask |= ((1 << (b - a)) - 1) << (s * lay.T_max)
        return (slots, lay.T_loc, mask)
    return (lay.T, lay.T_loc, None)
