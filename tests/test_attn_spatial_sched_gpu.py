"""The hand-scheduled spatial-attention kernel for 64 queries per wave (head_dim 64, query_blocks = 2) against the untouched
128-row kernel (query_blocks = 1), BIT for bit.

A query row's arithmetic does not depend on the rows that share its wave: both kernels run, per row, the same MFMAs, v_exp_f32,
adds and fp16 roundings in the same order, so their outputs are equal as bit patterns (established on the parent commit for
every case of this file: all bit-equal, a NaN row being NaN in both).  The new kernel changes only what a wave issues around that
arithmetic -- fragment read-ahead, peeled first / ragged last tile, a loop unrolled over the two LDS buffers, a lane-local
pre-check in front of the reference rule -- and each case below aims at one of those.  q | k | v are column slices of one
[rows, 3C] tensor, as the pipeline passes them.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = 64


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


def _bits(t):
    return t.contiguous().view(torch.int16)


def _both(ops, qkv, frames, heads, S, prescaled=False):
    """(64 queries per wave, 32 queries per wave) on the same q | k | v"""
    Cc = heads * HD
    d = qkv.to(DEV)
    run = lambda qb: ops.attn_spatial(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], frames, heads, S, prescaled=prescaled,   # noqa: E731
                                      query_blocks=qb)
    new, ref = run(2), run(1)
    torch.cuda.synchronize()
    return new, ref


def _assert_same(new, ref, what, nan_rows=False):
    same = _bits(new) == _bits(ref)
    if nan_rows:                                     # a NaN has no defined sign or payload: NaN where the oracle has NaN
        same |= torch.isnan(new) & torch.isnan(ref)
    assert same.all(), f"{what}: {(~same).sum().item()} / {same.numel()} halves differ, first at {(~same).flatten().nonzero()[0].item()}"


def _randn_qkv(frames, heads, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(frames * S, 3 * heads * HD, generator=g).half()


# 1 .. 5 key tiles: tile 0 alone (peeled first and last tile coincide), both buffers, the unrolled loop leaving after its first
# and its second body, the read-ahead wrapping into the other buffer
@pytest.mark.parametrize("S,frames,heads", [(64, 1, 1), (128, 2, 1), (192, 1, 2), (256, 2, 2), (320, 2, 1)])
def test_tile_counts(ops, S, frames, heads):
    new, ref = _both(ops, _randn_qkv(frames, heads, S, seed=100 + S), frames, heads, S)
    assert torch.isfinite(new).all()
    _assert_same(new, ref, f"S={S}")


# a masked last tile (peeled) and query rows beyond S
@pytest.mark.parametrize("S,frames,heads", [(255, 2, 1), (257, 1, 2), (300, 2, 2)])
def test_ragged_ends(ops, S, frames, heads):
    new, ref = _both(ops, _randn_qkv(frames, heads, S, seed=200 + S), frames, heads, S)
    assert torch.isfinite(new).all()
    _assert_same(new, ref, f"S={S}")


# several 256-row blocks per (frame, head); work counts 48 (a multiple of the 8 XCDs) and 15 (not)
@pytest.mark.parametrize("S,frames,heads", [(512, 8, 3), (768, 5, 1)])
def test_work_order_remainders(ops, S, frames, heads):
    new, ref = _both(ops, _randn_qkv(frames, heads, S, seed=300 + S), frames, heads, S)
    assert torch.isfinite(new).all()
    _assert_same(new, ref, f"S={S} {frames}f {heads}h")


# the gains of test_attn_spatial_reference_moves: logits over hundreds of units, the reference moving tile after tile (rising),
# never after the first tiles (falling), or at isolated late keys (spikes)
@pytest.mark.parametrize("pattern", ["rising", "falling", "spikes"])
def test_reference_moves(ops, pattern):
    S, frames, heads = 512, 2, 2
    Cc = heads * HD
    g = torch.Generator().manual_seed(77)
    q = torch.randn(frames * S, Cc, generator=g) * 2.0
    k = torch.randn(frames * S, Cc, generator=g)
    v = torch.randn(frames * S, Cc, generator=g)
    pos = torch.arange(S).repeat(frames).float()
    if pattern == "rising":
        gain = 0.5 + 6.0 * pos / S
    elif pattern == "falling":
        gain = 6.5 - 6.0 * pos / S
    else:
        gain = torch.where((pos % 97) == 96, torch.tensor(8.0), torch.tensor(0.5))
    qkv = torch.cat([q, k * gain[:, None], v], 1).half()
    new, ref = _both(ops, qkv, frames, heads, S)
    assert torch.isfinite(new).all()
    _assert_same(new, ref, pattern)


# Tile sums of a query row's two lanes (half sums) and the outcome the reference rule must have:
#   half sums below 8192 on every lane of the wave: the pre-check does not trip, nothing happens;
#   a half sum of 8192 with a total below 16384: the pre-check trips, the rule runs and decides that no row moves;
#   a total of 16384: the row moves.
HALF_SUM_PATTERNS = ((8191, 8191), (8192, 8191), (8192, 8192), (8191, 1), (16383, 0), (16384, 0))


def _scores_with_sum(total):
    """integer scores whose exp2 sum to ``total`` exactly (distinct powers of two, the smallest one split in two if needed)"""
    if total == 0:
        return []
    bits = [e for e in range(15) if (total >> e) & 1]
    return sorted(bits, reverse=True) if len(bits) > 1 or bits[0] == 0 else [bits[0] - 1, bits[0] - 1]


def test_half_sums_at_the_pre_check(ops):
    """Exact scores from one-hot keys.  Key n is a_n * e_(n % 64), so inside a key tile every key has a column of its own, and
    with Q pre-scaled (no rescaling of Q in the kernel) the exp2-domain score of query i for the key at tile position p is
    a_n * Q[i][p]: exact in fp16 and fp32.  a_n = 0 in tile 0 and the plain tiles (score 0, probability 1, reference 0), a_n = 1
    in the two special tiles (one per LDS buffer), where Q[i][p] is an integer: 12, 11, ... so that the probabilities are
    distinct powers of two summing to the wanted half sum (fp32-exact in any order), or -200 (probability exactly 0).  Position p
    belongs to the lane half (p >> 2) & 1.  Waves 0 .. 5 hold one pattern each (so that on wave 0 NO lane trips the pre-check),
    waves 6 and 7 mix them row by row."""
    S, frames, heads = 512, 1, 1
    special = (2, 5)
    q = torch.full((S, HD), -200.0)
    for i in range(S):
        wave = i // 64
        lo, hi = HALF_SUM_PATTERNS[wave % 6 if wave < 6 else i % 6]
        for half, total in ((0, lo), (1, hi)):
            ps = [p for p in range(64) if (p >> 2) & 1 == half]
            for p, sc in zip(ps, _scores_with_sum(total)):
                q[i, p] = float(sc)
    amp = torch.zeros(S)
    for t in special:
        amp[64 * t:64 * t + 64] = 1.0
    k = torch.zeros(S, HD)
    k[torch.arange(S), torch.arange(S) % 64] = amp
    g = torch.Generator().manual_seed(5)
    v = torch.randn(S, HD, generator=g)
    qkv = torch.cat([q, k, v], 1).half()
    # the construction is what it claims: per row and special tile, the half sums of exp2(score)
    # (in fp32 as the kernel computes them: exp2(-200) is 0, the sums are exact)
    sc = qkv[:, :HD].float() @ qkv[64 * special[0]:64 * special[0] + 64, HD:2 * HD].float().t()
    halves = torch.stack([torch.exp2(sc[:, [p for p in range(64) if (p >> 2) & 1 == h]]).sum(1) for h in (0, 1)], 1)
    want = torch.tensor([HALF_SUM_PATTERNS[(i // 64) % 6 if i // 64 < 6 else i % 6] for i in range(S)], dtype=torch.float32)
    assert torch.equal(halves, want)
    new, ref = _both(ops, qkv, frames, heads, S, prescaled=True)
    assert torch.isfinite(new).all()
    _assert_same(new, ref, "half sums at the pre-check")
    # and the result is the softmax it should be (fp32 reference on the GPU, the tolerance of the attention tests)
    d = qkv.to(DEV).float()
    logits = (d[:, :HD] @ d[:, HD:2 * HD].t()) * 0.6931471805599453
    want_o = torch.softmax(logits, -1) @ d[:, 2 * HD:]
    err = (new.float() - want_o).abs()
    assert (err <= 4e-3 * want_o.abs().max() + 4e-3 * want_o.abs()).all(), err.max().item()


def test_nan_score_row(ops):
    """one query row with a NaN score (its half sums are NaN: the pre-check trips, the rule runs): that row comes out NaN in
    both kernels (a NaN never compares equal and its sign / payload are not defined by the arithmetic, so it is matched as
    NaN), every other row of its wave is untouched, bit for bit"""
    S, frames, heads = 512, 1, 2
    qkv = _randn_qkv(frames, heads, S, seed=9)
    qkv[300, 3] = float("nan")                       # head 0, query 300
    new, ref = _both(ops, qkv, frames, heads, S)
    assert torch.isnan(new[300, :HD]).all()
    rest = torch.ones(S, dtype=torch.bool)
    rest[300] = False
    assert torch.isfinite(new[rest.to(DEV)]).all() and torch.isfinite(new[300, HD:]).all()
    assert torch.equal(torch.isnan(new), torch.isnan(ref))
    _assert_same(new, ref, "NaN row", nan_rows=True)


@pytest.mark.parametrize("S", [256, 300])
def test_output_rows_not_16_byte_aligned(ops, S):
    """O normally leaves as 16-byte pieces of whole rows; an output view whose rows start 8 bytes off a 16-byte boundary (the C
    ABI asks for a row stride that is a multiple of 4 halves only) takes the 8-byte stores, and the columns next to the view
    stay untouched"""
    frames, heads = 2, 2
    Cc = heads * HD
    d = _randn_qkv(frames, heads, S, seed=400 + S).to(DEV)
    outs = []
    for qb in (2, 1):
        wide = torch.full((frames * S, Cc + 12), 7.0, dtype=torch.float16, device=DEV)
        ops.attn_spatial(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], frames, heads, S, out=wide[:, 4:4 + Cc], query_blocks=qb)
        outs.append(wide)
    torch.cuda.synchronize()
    assert (outs[0][:, :4] == 7.0).all() and (outs[0][:, 4 + Cc:] == 7.0).all()
    assert torch.isfinite(outs[0]).all()
    _assert_same(outs[0], outs[1], f"S={S}, unaligned output rows")
    aligned = ops.attn_spatial(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], frames, heads, S, query_blocks=2)
    _assert_same(outs[0][:, 4:4 + Cc], aligned, f"S={S}, unaligned against aligned output")


def test_repeat_launches(ops):
    """the level-1 shape of a clip (36 key tiles per block) launched again and again: a fragment read that outruns the barrier
    or the DMA shows as a run-to-run difference"""
    S, frames, heads = 2304, 10, 5
    Cc = heads * HD
    d = _randn_qkv(frames, heads, S, seed=11).to(DEV)
    run = lambda: ops.attn_spatial(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], frames, heads, S, query_blocks=2)   # noqa: E731
    first = run()
    again = [run() for _ in range(6)]
    ref = ops.attn_spatial(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], frames, heads, S, query_blocks=1)
    torch.cuda.synchronize()
    for i, o in enumerate(again):
        _assert_same(o, first, f"launch {i + 2} against launch 1")
    _assert_same(first, ref, "launch 1 against the 128-row kernel")
