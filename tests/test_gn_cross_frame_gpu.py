"""The GroupNorm entry points that combine statistics across frames or ranks, element by element against an fp64 F.group_norm
(+ SiLU) over the WHOLE statistics set (all T * HW rows of the clip), computed on the GPU:

  mofa_gn_partial_f16        partial entries (frame, row chunk, group) -> {sum, sum of squares} and their layout, also written into
                             the rows of the frame-sharded gather buffer (ops.gn_partial_into, parallel.FrameParallel.part_buffer)
  mofa_gn_apply_f16          the fused path, up to ops.GN_FUSED_MAX_ENTRIES partial entries per set
  mofa_gn_finalize +         sets with more entries (the temporal VAE decoder's 8-frame chunks: 1 024 entries), and both sides of
  mofa_affine_act_f16        the switch-over
  mofa_gn_apply_gathered_f16 every temporal GroupNorm of a sharded rank: its own frames and each halo frame received raw from a
                             neighbour, over the split_frames layouts of the product
  mofa_gn_reduce +           the split form for callers that all-reduce the sums
  mofa_gn_finalize_sums

Inputs are seeded with a different mean and scale per channel and a shift per frame, so that a wrong channel-to-group or
frame-to-set mapping fails.  Bar: |err| <= 2e-3 * (max|ref| + |ref|) per element (tests/test_kernels_gpu.py); partial entries
1e-5 of the fp64 sum of |x| (or x^2) over the entry.  Two applications of the same statistics agree to within 1 fp16 ulp; the
halo-frame application is bit-identical to the owner's (bit-identical statistics everywhere)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
EINVAL = -22


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _cdiv(a, b):
    return -(-a // b)


def _clip(T, HW, C, seed, mean=0.0, std=1.0):
    """[T * HW, C] fp16: per-channel mean and scale, per-frame shift"""
    g = _gen(seed)
    cm = mean + 0.7 * std * torch.randn(C, generator=g, device=DEV)
    cs = std * (0.3 + 1.2 * torch.rand(C, generator=g, device=DEV))
    fs = 0.4 * std * torch.randn(T, 1, 1, generator=g, device=DEV)
    x = torch.randn(T, HW, C, generator=g, device=DEV) * cs + cm + fs
    return x.reshape(T * HW, C).clamp(-6e4, 6e4).half()


def _affine(C, seed):
    g = _gen(seed)
    return 1 + 0.3 * torch.randn(C, generator=g, device=DEV), 0.3 * torch.randn(C, generator=g, device=DEV)


def _ref(x, gamma, beta, T, HW, fps, silu):
    """fp64 GroupNorm(32) over sets of ``fps`` frames (all fps * HW rows of each) (+ SiLU) -> [T * HW, C]"""
    C = x.shape[1]
    xr = x.double().reshape(T // fps, fps * HW, C).transpose(1, 2)
    y = F.group_norm(xr, 32, gamma.double(), beta.double(), eps=EPS)
    if silu:
        y = F.silu(y)
    return y.transpose(1, 2).reshape(T * HW, C)


def _close(out, ref, what, tol=2e-3):
    o = out.double()
    assert tuple(o.shape) == tuple(ref.shape), (tuple(o.shape), tuple(ref.shape))
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite output"
    err = (o - ref).abs()
    scale = float(ref.abs().max())
    bad = err > tol * (scale + ref.abs())
    n = int(bad.sum())
    k = int(err.argmax())
    assert n == 0, (f"{what}: {n} / {err.numel()} elements out of tolerance; max err {float(err.max()):.4e} "
                    f"(scale {scale:.4e}) at row {k // o.shape[1]}, column {k % o.shape[1]}")


def _ulps(a, b):
    """element-wise distance of two fp16 tensors in units in the last place"""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -32768 - i, i)
    return (key(a) - key(b)).abs()


def _within_ulp(a, b, what):
    d = _ulps(a, b)
    k = int(d.argmax())
    assert int(d.max()) <= 1, (f"{what}: {int((d > 1).sum())} elements differ by more than 1 fp16 ulp (max {int(d.max())} at "
                               f"row {k // a.shape[1]}, column {k % a.shape[1]}: {float(a.reshape(-1)[k])} vs {float(b.reshape(-1)[k])})")


def _strided(x, pad=16):
    """x as the column slice [:, 8 : 8 + C] of a wider buffer (ldx = C + pad)"""
    w = torch.zeros((x.shape[0], x.shape[1] + pad), dtype=x.dtype, device=x.device)
    w[:, 8:8 + x.shape[1]] = x
    return w[:, 8:8 + x.shape[1]]


def _nchunks(HW):
    """row chunks per frame, the rule of csrc/norm.hip (gn_nchunks)"""
    n = _cdiv(HW, 576) if HW >= 9216 else _cdiv(HW, 144)
    cap = 128 if HW >= 9216 else 16
    return max(1, min(n, cap))


# ---------------------------------------------------------------------------------------------------------------------
# 1. partial entries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 320, 1280])
@pytest.mark.parametrize("HW", [37, 144, 2304, 9215, 9216, 9217, 36864])
def test_partial_entries_and_layout(ops, HW, C):
    frames = 2
    nparts = ops.gn_nparts(HW, C)
    assert nparts == _nchunks(HW), (HW, nparts)
    rpc = _cdiv(HW, nparts)
    x = _clip(frames, HW, C, seed=HW + C)
    part = torch.full((frames * nparts, 64), float("nan"), dtype=torch.float32, device=DEV)
    ops.gn_partial_into(x, part, frames, HW)
    part_s = torch.full_like(part, float("nan"))
    ops.gn_partial_into(_strided(x), part_s, frames, HW)
    assert torch.equal(part, part_s), "strided input (ldx > C) changes the partial entries"
    xd = F.pad(x.double().reshape(frames, HW, 32, C // 32), (0, 0, 0, 0, 0, nparts * rpc - HW))
    xd = xd.reshape(frames, nparts, rpc, 32, C // 32)                 # entry (frame, chunk, group): rows [chunk * rpc, ...)
    s, q, a = xd.sum((2, 4)), (xd * xd).sum((2, 4)), xd.abs().sum((2, 4))
    got = part.double().reshape(frames, nparts, 32, 2)
    for k, (ref, mag) in enumerate(((s, a), (q, q))):
        err = (got[..., k] - ref).abs()
        bad = ~(err <= 1e-5 * mag)
        assert not bool(bad.any()), (f"{'sum' if k == 0 else 'sum of squares'}: {int(bad.sum())} entries off, worst "
                                     f"(frame, chunk, group) {tuple(int(i) for i in (bad.nonzero()[0]))}, "
                                     f"max err / magnitude {float((err / mag.clamp_min(1e-30)).max()):.3e}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. both sides of the fused / finalize switch
# ---------------------------------------------------------------------------------------------------------------------
SWITCH = {"fused, 512 entries": (36864, 8, 320, 512), "finalize, 513 entries": (32832, 9, 320, 513),
          "decoder 8-frame chunk, 1024 entries": (147456, 8, 128, 1024)}


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("case", list(SWITCH))
def test_group_norm_clip_statistics_both_paths(ops, case, silu):
    HW, T, C, entries = SWITCH[case]
    assert T * ops.gn_nparts(HW, C) == entries
    assert (entries <= ops.GN_FUSED_MAX_ENTRIES) == case.startswith("fused")
    x = _clip(T, HW, C, seed=entries)
    gamma, beta = _affine(C, 1)
    out = ops.group_norm(x, gamma, beta, T, HW, EPS, frames_per_stat=T, silu=silu)
    _close(out, _ref(x, gamma, beta, T, HW, T, silu), f"group_norm {case}, silu {silu}")


def test_group_norm_finalize_path_large_offset(ops):
    """mean ~6e3, std ~2.5e3 (test_fp16_range_gpu.py): sums of squares ~1e14 per set, 513 entries"""
    HW, T, C, _ = SWITCH["finalize, 513 entries"]
    x = _clip(T, HW, C, seed=7, mean=6e3, std=2.5e3)
    assert float(x.float().abs().max()) > 1.5e4
    gamma, beta = _affine(C, 2)
    out = ops.group_norm(x, gamma, beta, T, HW, 1e-6, frames_per_stat=T, silu=True)
    xr = x.double().reshape(1, T * HW, C).transpose(1, 2)
    ref = F.silu(F.group_norm(xr, 32, gamma.double(), beta.double(), eps=1e-6)).transpose(1, 2).reshape(T * HW, C)
    _close(out, ref, "group_norm finalize path, mean 6e3")


@pytest.mark.parametrize("silu", [False, True])
def test_fused_and_finalize_paths_agree(ops, monkeypatch, silu):
    """the same 512-entry set through both paths (the switch moved by one entry)"""
    HW, T, C, _ = SWITCH["fused, 512 entries"]
    x = _clip(T, HW, C, seed=11)
    gamma, beta = _affine(C, 3)
    fused = ops.group_norm(x, gamma, beta, T, HW, EPS, frames_per_stat=T, silu=silu)
    monkeypatch.setattr(ops, "GN_FUSED_MAX_ENTRIES", 511)
    fin = ops.group_norm(x, gamma, beta, T, HW, EPS, frames_per_stat=T, silu=silu)
    _within_ulp(fused, fin, "fused vs finalize + affine")


def test_finalize_two_statistics_sets(ops):
    """plain mofa_gn_finalize with frames_per_stat = 3 over 6 frames (two sets), then mofa_affine_act_f16 on strided x / y"""
    from mofa_video_amd import lib as L
    lib = L.load()
    T, fps, HW, C = 6, 3, 2304, 320
    x = _clip(T, HW, C, seed=13)
    gamma, beta = _affine(C, 4)
    nparts = ops.gn_nparts(HW, C)
    part = torch.empty((T * nparts, 64), dtype=torch.float32, device=DEV)
    ops.gn_partial_into(x, part, T, HW)
    scale = torch.empty((T, C), dtype=torch.float32, device=DEV)
    shift = torch.empty_like(scale)
    st = L.stream_ptr()
    assert lib.mofa_gn_finalize(L.ptr(part), L.ptr(gamma), L.ptr(beta), L.ptr(scale), L.ptr(shift), T, HW, C, fps, EPS, st) == 0
    xs = _strided(x)
    yw = torch.full((T * HW, C + 32), 3.0, dtype=torch.float16, device=DEV)
    y = yw[:, 16:16 + C]
    assert lib.mofa_affine_act_f16(L.ptr(xs), L.ptr(scale), L.ptr(shift), L.ptr(y), T, HW, C, xs.stride(0), y.stride(0), 1, st) == 0
    _close(y, _ref(x, gamma, beta, T, HW, fps, True), "finalize (2 sets) + affine_act")
    assert bool((yw[:, :16] == 3.0).all()) and bool((yw[:, 16 + C:] == 3.0).all()), "affine_act wrote outside its columns"


# ---------------------------------------------------------------------------------------------------------------------
# 3. the gathered path across shard layouts, 4. the split all-reduce form
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = [(25, 4), (25, 2), (7, 4), (5, 2)]           # (frames, frame shards): split_frames 7/6/6/6, 13/12, 2/2/2/1, 3/2
GEOMS = [(9216, 320), (2304, 640), (576, 1280), (144, 1280), (999, 320)]


def _gather_buffer(ops, xs, T, HW, C, n):
    """every shard's partials written into its rows of FrameParallel.part_buffer, then 'all-gathered' (copied) into one buffer
    laid out the same: frame_ranks x T_max x nparts rows, the padding rows of shorter shards zero"""
    from mofa_video_amd.parallel import FrameParallel, Layout
    nparts = ops.gn_nparts(HW, C)
    gathered = None
    for s in range(n):
        lay = Layout(n, s, T, cfg_ranks=1)
        buf, own = FrameParallel(lay, None).part_buffer(nparts, xs.device)
        assert tuple(buf.shape) == (n * lay.T_max * nparts, 64)
        ops.gn_partial_into(xs[lay.f0 * HW:lay.f1 * HW], own, lay.T_loc, HW)
        r0, r1 = s * lay.T_max * nparts, (s * lay.T_max + lay.T_loc) * nparts
        assert own.data_ptr() == buf[r0:].data_ptr() and own.shape[0] == r1 - r0
        assert int(torch.count_nonzero(buf[:r0])) == 0 and int(torch.count_nonzero(buf[r1:])) == 0, "rows beyond the shard's own written"
        if gathered is None:
            gathered = torch.zeros_like(buf)
        gathered[r0:r1] = own
    return gathered


def _apply_gathered_all(ops, xs, gathered, gamma, beta, T, HW, C, n, silu):
    """every shard's own frames through gn_apply_gathered into a column slice of a wider buffer with guard rows; returns the
    clip [T * HW, C] (fp16) and the outputs per shard"""
    from mofa_video_amd.parallel import split_frames
    cnt = float(T) * HW * (C // 32)
    outs = []
    G = 5
    for s, (f0, f1) in enumerate(split_frames(T, n)):
        ow = torch.full(((f1 - f0) * HW + 2 * G, C + 24), -7.0, dtype=torch.float16, device=DEV)
        out = ow[G:G + (f1 - f0) * HW, 8:8 + C]
        ops.gn_apply_gathered(xs[f0 * HW:f1 * HW], gathered, cnt, gamma, beta, EPS, out, f1 - f0, HW, silu=silu)
        guard = torch.ones_like(ow, dtype=torch.bool)
        guard[G:G + (f1 - f0) * HW, 8:8 + C] = False
        assert bool((ow[guard] == -7.0).all()), f"shard {s}: guard rows / columns of the output written"
        outs.append(out)
    return torch.cat(outs, 0), outs


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("HW,C", GEOMS)
@pytest.mark.parametrize("T,n", LAYOUTS)
def test_gathered_across_shard_layouts(ops, T, n, HW, C, silu):
    from mofa_video_amd.parallel import split_frames
    x = _clip(T, HW, C, seed=T * 1000 + HW + C)
    xs = _strided(x)
    gamma, beta = _affine(C, 5)
    gathered = _gather_buffer(ops, xs, T, HW, C, n)
    clip, outs = _apply_gathered_all(ops, xs, gathered, gamma, beta, T, HW, C, n, silu)
    ref = _ref(x, gamma, beta, T, HW, T, silu)
    bounds = split_frames(T, n)
    for s, (f0, f1) in enumerate(bounds):
        _close(outs[s], ref[f0 * HW:f1 * HW], f"{T} frames / {n} shards, shard {s} (frames {f0}..{f1 - 1}), HW {HW}, C {C}")
    # halo frames: the raw boundary frame of a neighbour, normalised on the receiving shard alone (nframes = 1)
    cnt = float(T) * HW * (C // 32)
    for s, (f0, f1) in enumerate(bounds):
        for hf in (f0 - 1, f1):
            if not 0 <= hf < T:
                continue
            y = torch.empty((HW, C), dtype=torch.float16, device=DEV)
            ops.gn_apply_gathered(x[hf * HW:(hf + 1) * HW], gathered, cnt, gamma, beta, EPS, y, 1, HW, silu=silu)
            assert torch.equal(y, clip[hf * HW:(hf + 1) * HW]), f"shard {s}: halo frame {hf} differs from its owner's output"
    single = ops.group_norm(x, gamma, beta, T, HW, EPS, frames_per_stat=T, silu=silu)
    _within_ulp(clip, single, f"gathered ({T} frames / {n} shards) vs single-rank group_norm")


@pytest.mark.parametrize("HW,C", [(2304, 640), (999, 320)])
@pytest.mark.parametrize("T,n", LAYOUTS)
def test_split_allreduce_form(ops, T, n, HW, C):
    """per shard mofa_gn_partial_f16 -> mofa_gn_reduce, fp64 sums added on the host (the all-reduce), then
    mofa_gn_finalize_sums with the clip's element count -> mofa_affine_act_f16"""
    from mofa_video_amd import lib as L
    from mofa_video_amd.parallel import split_frames
    lib = L.load()
    silu = True
    x = _clip(T, HW, C, seed=T * 7 + HW + C)
    gamma, beta = _affine(C, 6)
    nparts = ops.gn_nparts(HW, C)
    st = L.stream_ptr()
    bounds = split_frames(T, n)
    total = torch.zeros((1, 32, 2), dtype=torch.float64)
    for f0, f1 in bounds:
        part = torch.empty(((f1 - f0) * nparts, 64), dtype=torch.float32, device=DEV)
        ops.gn_partial_into(x[f0 * HW:f1 * HW], part, f1 - f0, HW)
        sums = torch.full((1, 32, 2), float("nan"), dtype=torch.float64, device=DEV)
        assert lib.mofa_gn_reduce(L.ptr(part), L.ptr(sums), f1 - f0, HW, C, f1 - f0, st) == 0
        total += sums.cpu()
    cnt = float(T) * HW * (C // 32)
    sums = total.to(DEV)
    outs = []
    for f0, f1 in bounds:
        scale = torch.empty((f1 - f0, C), dtype=torch.float32, device=DEV)
        shift = torch.empty_like(scale)
        assert lib.mofa_gn_finalize_sums(L.ptr(sums), L.ptr(gamma), L.ptr(beta), L.ptr(scale), L.ptr(shift), f1 - f0, C, f1 - f0,
                                         cnt, EPS, st) == 0
        y = torch.empty(((f1 - f0) * HW, C), dtype=torch.float16, device=DEV)
        xs = x[f0 * HW:f1 * HW]
        assert lib.mofa_affine_act_f16(L.ptr(xs), L.ptr(scale), L.ptr(shift), L.ptr(y), f1 - f0, HW, C, C, C, 1, st) == 0
        outs.append(y)
    clip = torch.cat(outs, 0)
    _close(clip, _ref(x, gamma, beta, T, HW, T, silu), f"split form, {T} frames / {n} shards")
    gathered, _ = _apply_gathered_all(ops, x, _gather_buffer(ops, x, T, HW, C, n), gamma, beta, T, HW, C, n, silu)
    _within_ulp(clip, gathered, "split all-reduce form vs gathered")


# ---------------------------------------------------------------------------------------------------------------------
# 5. argument edges
# ---------------------------------------------------------------------------------------------------------------------
def test_gathered_4096_entries(ops):
    """the largest set mofa_gn_apply_gathered_f16 takes: 32 frames x 128 chunks (C = 32: one channel per group)"""
    T, HW, C = 32, 73728, 32
    assert ops.gn_nparts(HW, C) * T == 4096
    x = _clip(T, HW, C, seed=17)
    gamma, beta = _affine(C, 8)
    part = torch.empty((4096, 64), dtype=torch.float32, device=DEV)
    ops.gn_partial_into(x, part, T, HW)
    out = torch.empty_like(x)
    ops.gn_apply_gathered(x, part, float(T) * HW * (C // 32), gamma, beta, EPS, out, T, HW, silu=True)
    _close(out, _ref(x, gamma, beta, T, HW, T, True), "gathered, 4096 entries")


def test_argument_edges_rejected_without_launch(ops):
    """nentries > 4096, count_per_group <= 0 and C % 32 != 0 return MOFA_EINVAL, and nothing is written"""
    from mofa_video_amd import lib as L
    lib = L.load()
    st = L.stream_ptr()
    HW, C = 64, 64
    x = _clip(2, HW, C, seed=19)
    gamma, beta = _affine(C, 9)
    part = torch.zeros((4097, 64), dtype=torch.float32, device=DEV)
    y = torch.full_like(x, 5.0)

    def gathered(nentries, cnt, C_=C, nframes=1):
        return lib.mofa_gn_apply_gathered_f16(L.ptr(x), L.ptr(part), nentries, cnt, L.ptr(gamma), L.ptr(beta), L.ptr(y), nframes,
                                              HW, C_, C, C, EPS, 1, st)
    assert gathered(4097, 1.0 * HW * 2) == EINVAL
    for cnt in (0.0, -1.0, -float(HW)):
        assert gathered(16, cnt) == EINVAL, cnt
    assert gathered(16, float(HW) * 2, C_=40) == EINVAL
    sums = torch.zeros((1, 32, 2), dtype=torch.float64, device=DEV)
    sc = torch.full((2, C), 9.0, dtype=torch.float32, device=DEV)
    sh = torch.full_like(sc, 9.0)
    for cnt in (0.0, -2.0):
        assert lib.mofa_gn_finalize_sums(L.ptr(sums), L.ptr(gamma), L.ptr(beta), L.ptr(sc), L.ptr(sh), 2, C, 2, cnt, EPS, st) == EINVAL
    assert lib.mofa_gn_finalize_sums(L.ptr(sums), L.ptr(gamma), L.ptr(beta), L.ptr(sc), L.ptr(sh), 2, 40, 2, 1.0, EPS, st) == EINVAL
    assert lib.mofa_gn_finalize(L.ptr(part), L.ptr(gamma), L.ptr(beta), L.ptr(sc), L.ptr(sh), 2, HW, 40, 2, EPS, st) == EINVAL
    assert lib.mofa_gn_partial_f16(L.ptr(x), L.ptr(part), 2, HW, 40, C, st) == EINVAL
    assert lib.mofa_gn_reduce(L.ptr(part), L.ptr(sums), 2, HW, 40, 2, st) == EINVAL
    assert lib.mofa_gn_apply_f16(L.ptr(x), L.ptr(part), L.ptr(gamma), L.ptr(beta), L.ptr(y), 2, HW, 40, C, C, 2, EPS, 1, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((y == 5.0).all()) and bool((sc == 9.0).all()) and bool((sh == 9.0).all())
    assert int(torch.count_nonzero(part)) == 0 and int(torch.count_nonzero(sums)) == 0
    # ... and the ops wrapper raises
    with pytest.raises(L.MofaHipError):
        ops.gn_apply_gathered(x[:HW], part[:16], 0.0, gamma, beta, EPS, y[:HW], 1, HW)
