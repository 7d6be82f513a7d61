"""The 256x320 implicit-GEMM tile with its K loop on 16x16x32 MFMAs (csrc/igemm320.hip): the accumulators are built as 16x16
tiles, with the weight rows of a fragment loaded in a permuted order, and brought back into the 32x32 register layout by
lane-row swaps before the unchanged epilogues.  A wrong row permutation, a wrong swap partner or a wrong initial-value
column moves outputs to other rows / columns / lane halves, so every case here is EXACT: operands are small integers (or
integers / 16), every product and every partial sum is exact in fp32 whatever the summation order, and the fp16 result has
to ``torch.equal`` the fp32 reference rounded once.  The bias is n / 16: distinct in every column.

One K loop ships (no K threshold between two loops); the K values are nk = 1, 2, 3, 5 K tiles: both ring parities and, in
the persistent walk, tiles that start on either ring slot.

Two kinds apply a function that the kernels evaluate with fast approximations (exp2 / rcp, an erf polynomial), which no
reference reproduces bit for bit.  Their operands are chosen so that the function is exact after the one rounding to fp16:
  * SiLU: the bias is 32 + n / 16, every pre-activation v is >= 9, where v * sigmoid(v) = v (1 - e^-v) differs from v by less
    than 1.3e-4 v, under half an fp16 ulp (2^-12 v .. 2^-11 v): the rounded result is v itself, in the kernel and in F.silu.
  * GEGLU pair: the gate rows have zero weights and a bias of 8, 16 or 32 (by column, period 3: no multiple of 4 or 8 columns
    maps a column onto one with the same gate): gelu(g) = g (1 - 1.5e-5 at most, the polynomial's error) and val * g is a shift of
    the exponent, so the rounded product is val * g exactly.  Gates that come out of the MFMAs are covered bit for bit by the
    tile-agreement test against the 256x256 tile (same formula, K loop untouched by this change).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
T320, T256, T192 = 6, 5, 4
S_ACC = 0.75
KINDS = ["plain", "silu", "rvu", "rv", "r1", "r1 s1=0.5", "r1r2", "geglu"]


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import lib
    from mofa_video_amd import ops as o
    lib.load()
    return o


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(lo, hi, shape, g, div=1):
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV).float() / div


def _operands(M, N, K, seed):
    """x in {-3 .. 3}, w in {-2 .. 2} / 16, bias n / 16: |sum| <= 6 K / 16, on a 2^-4 grid -- exact in fp32 up to K = 2^21"""
    g = _gen(seed)
    x = _ints(-3, 3, (M, K), g).half()
    w = _ints(-2, 2, (N, K), g, 16).half()
    bias = torch.arange(N, device=DEV).float() / 16
    return x, w, bias, g


def _epilogue(kind, M, N, g):
    """kwargs of ops.igemm and the reference's epilogue on the exact fp32 sums (acc + bias already added)"""
    kw = dict(s_acc=S_ACC)
    r1 = r2 = None
    rowvec = rv = None
    if kind.startswith("r1"):                                   # residuals on a 2^-6 grid, |r| <= 8: the adds are exact in fp32
        r1 = _ints(-512, 512, (M, N), g, 64).half()
        kw.update(r1=r1, s1=0.5 if kind == "r1 s1=0.5" else 1.0)
    if kind == "r1r2":
        r2 = _ints(-512, 512, (M, N), g, 64).half()
        kw.update(r2=r2, s2=0.25)
    if kind in ("rv", "rvu") or kind.endswith("+rvu"):
        # "rvu": one row of the vector per 64 rows (a wave's rows: folded into the accumulators' initial value);
        # "rv": it changes with every row (per-row path of the fp32 row epilogue)
        rv = (64, 3, 1, 5) if "rvu" in kind else (7, 3, 4, 5)
        rowvec = _ints(-64, 64, (5, N), g, 16)
        kw.update(rowvec=rowvec, rv=rv)

    def apply(acc):
        if rowvec is not None:
            m = torch.arange(M, device=DEV)
            acc = acc + rowvec[((m // rv[0]) * rv[1] + (m % rv[2])) % rv[3]]
        y = S_ACC * acc
        if r1 is not None:                                       # the layer's output is rounded to fp16 before the residual add
            y = y.half().float() + kw["s1"] * r1.float()
        if r2 is not None:
            y = y + kw["s2"] * r2.float()
        return y.half()
    return kw, apply


def _run_gemm(ops, kind, M, N, K, seed, tile=T320, split_k=False):
    """-> (output of the forced tile, exact reference)"""
    x, w, bias, g = _operands(M, N, K, seed)
    if kind == "silu":
        from mofa_video_amd import lib as L
        bias = bias + 32.0
        v = x.float() @ w.float().t() + bias
        assert v.min().item() >= 9.0                              # (see the module docstring)
        return ops.igemm(x, w, bias, act=L.ACT_SILU, tile=tile, split_k=split_k), F.silu(v).half()
    if kind == "geglu":
        from mofa_video_amd import lib as L
        from mofa_video_amd.weights import interleave_geglu
        ch = N // 2                                              # N weight rows: value rows, then gate rows
        w[ch:] = 0
        bias[ch:] = 8.0 * 2.0 ** (torch.arange(ch, device=DEV) % 3)
        wi, bi = interleave_geglu(w, bias)
        h = x.float() @ w.float().t() + bias
        return ops.igemm(x, wi, bi, act=L.ACT_GEGLU_PAIR, tile=tile, split_k=split_k), (h[:, :ch] * F.gelu(h[:, ch:])).half()
    kw, apply = _epilogue(kind, M, N, g)
    return ops.igemm(x, w, bias, tile=tile, split_k=split_k, **kw), apply(x.float() @ w.float().t() + bias)


def _assert_equal(out, ref, what):
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    if not torch.equal(out, ref):
        bad = (out != ref) | torch.isnan(out)
        i = int(bad.flatten().nonzero()[0].item())
        r, c = i // ref.shape[1], i % ref.shape[1]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ from the exact reference; first at row {r} "
                             f"col {c}: {out[r, c].item()} != {ref[r, c].item()}; rows {sorted(set((bad.any(1).nonzero().flatten() % 64).tolist()))[:16]} "
                             f"(mod 64), cols {sorted(set((bad.any(0).nonzero().flatten() % 32).tolist()))} (mod 32)")


@pytest.mark.parametrize("K", [64, 128, 192, 320])
@pytest.mark.parametrize("kind", KINDS)
def test_placement_every_kind_every_ring_phase(ops, kind, K):
    """M = 293 (a full tile + 37 ragged rows) and 64, N = 320 and 640, nk = 1, 2, 3, 5"""
    for M in (293, 64):
        for N in (320, 640):
            out, ref = _run_gemm(ops, kind, M, N, K, seed=1000 + K)
            _assert_equal(out, ref, f"{kind} M={M} N={N} K={K}")


@pytest.mark.parametrize("K", [128, 192])
@pytest.mark.parametrize("kind", ["plain", "r1", "rvu", "geglu"])
def test_persistent_walk_reinitialises_and_swaps_per_tile(ops, kind, K):
    """A workgroup that walks several tiles takes the next tile's initial values from the other bias slot and converts the
    accumulators after each tile.  M = 256 * 3 + 40, N = 640 is 8 tiles; a workgroup runs more than one tile only where there are
    more tiles than CUs, so the same columns also run with CU-count + 6 tiles (whole tiles: no workspace), two tiles on the
    first workgroups; K = 192 (3 K tiles) starts the second tile on the other ring slot."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for M in (256 * 3 + 40, 256 * ((n_cu + 6 + 1) // 2 - 1) + 40):
        out, ref = _run_gemm(ops, kind, M, 640, K, seed=2000 + K)
        _assert_equal(out, ref, f"persistent walk {kind} M={M} K={K}")


def _conv_x(n, Cin, H, W, g):
    return _ints(-3, 3, (n, Cin, H, W), g)


@pytest.mark.parametrize("Cin", [64, 128])
@pytest.mark.parametrize("mode", ["conv3x3", "convt3"])
def test_convolution_k_order(ops, mode, Cin):
    """6 frames of 9 x 13, Cout = 320: the tap changes with every K tile (Cin = 64) or every second one (Cin = 128).  The reference
    is a sum of per-tap matrix products (exact in fp32), not a library convolution."""
    from mofa_video_amd.weights import pack_conv3d_t3, pack_conv3x3
    n, H, W, Cout = 6, 9, 13, 320
    g = _gen(3000 + Cin)
    x = _conv_x(n, Cin, H, W, g)
    bias = torch.arange(Cout, device=DEV).float() / 16
    xt = x.permute(0, 2, 3, 1).reshape(n * H * W, Cin).half().contiguous()
    r1 = _ints(-512, 512, (n * H * W, Cout), g, 64).half()
    if mode == "conv3x3":
        w = _ints(-2, 2, (Cout, Cin, 3, 3), g, 16)
        cols = F.unfold(x, 3, padding=1)                          # [n, Cin * 9, H W], (c, ky, kx) major
        acc = (w.reshape(Cout, Cin * 9) @ cols).permute(0, 2, 1).reshape(-1, Cout)
        wk, geom = pack_conv3x3(w.cpu()).to(DEV), ops.conv3x3_geom(H, W)
    else:
        w = _ints(-2, 2, (Cout, Cin, 3, 1, 1), g, 16)
        xf = torch.zeros(n + 2, H * W, Cin, device=DEV)           # one clip of n frames between two zero frames
        xf[1:-1] = xt.float().reshape(n, H * W, Cin)
        acc = sum(xf[t:t + n] @ w[:, :, t, 0, 0].t() for t in range(3)).reshape(-1, Cout)
        wk, geom = pack_conv3d_t3(w.cpu()).to(DEV), ops.convt3_geom(n, H * W)
    out = ops.igemm(xt, wk, bias, geom=geom, tile=T320, split_k=False, s_acc=S_ACC)
    _assert_equal(out, (S_ACC * (acc + bias)).half(), f"{mode} Cin={Cin} plain")
    out = ops.igemm(xt, wk, bias, geom=geom, tile=T320, split_k=False, s_acc=S_ACC, r1=r1, s1=1.0)
    _assert_equal(out, ((S_ACC * (acc + bias)).half().float() + r1.float()).half(), f"{mode} Cin={Cin} r1")


@pytest.mark.parametrize("mode", ["conv3x3", "convt3"])
def test_split_k_exact_with_and_without_workspace(ops, mode):
    """The shapes of test_split_k_convolutions_slices_start_inside_a_tap (46 tiles: every tile is a remainder tile and is cut into
    K slices that start inside a tap; that test shows that the split path runs on them), with exact operands: the fp32 partial
    tiles leave the kernel through the converted accumulators, so the split launch, the whole-tile launch and the reference
    agree bit for bit."""
    from mofa_video_amd.weights import pack_conv3d_t3, pack_conv3x3
    g = _gen(4000)
    Cout = 320
    bias = torch.arange(Cout, device=DEV).float() / 16
    if mode == "conv3x3":
        n, Cin, H, W = 6, 256, 37, 53                             # K = 2304 = 36 K tiles, 4 per tap
        x = _conv_x(n, Cin, H, W, g)
        w = _ints(-2, 2, (Cout, Cin, 3, 3), g, 16)
        xt = x.permute(0, 2, 3, 1).reshape(n * H * W, Cin).half().contiguous()
        wm = w.reshape(Cout, Cin * 9)
        acc = torch.cat([(wm @ F.unfold(x[i:i + 1], 3, padding=1))[0].t() for i in range(n)])
        wk, geom = pack_conv3x3(w.cpu()).to(DEV), ops.conv3x3_geom(H, W)
    else:
        B, T, HW, Cin = 2, 5, 1153, 1024                          # K = 3072 = 48 K tiles, 16 per tap
        xt = _ints(-3, 3, (B * T * HW, Cin), g).half()
        w = _ints(-2, 2, (Cout, Cin, 3, 1, 1), g, 16)
        xf = torch.zeros(B, T + 2, HW, Cin, device=DEV)
        xf[:, 1:-1] = xt.float().reshape(B, T, HW, Cin)
        acc = sum(xf[:, t:t + T] @ w[:, :, t, 0, 0].t() for t in range(3)).reshape(-1, Cout)
        wk, geom = pack_conv3d_t3(w.cpu()).to(DEV), ops.convt3_geom(T, HW)
    M = acc.shape[0]
    kw, apply = _epilogue("r1+rvu", M, Cout, g)
    ref = apply(acc + bias)
    whole = ops.igemm(xt, wk, bias, geom=geom, tile=T320, split_k=False, **kw)
    split = ops.igemm(xt, wk, bias, geom=geom, tile=T320, split_k=True, **kw)
    _assert_equal(whole, ref, f"{mode} whole tiles")
    _assert_equal(split, ref, f"{mode} split-K")
    assert torch.equal(whole, split)


@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("kind", ["plain", "r1", "rvu", "r1+rvu"])
def test_stats_pair_sums_exact(ops, kind, K):
    """STATS kernels (kinds 0, 1, 4, 5) at M = 256, N = 320 with integer-valued outputs (|out| <= 2 K + 24): the pair sums and the
    sums of squares (<= 128 * 280^2 < 2^24) are exact in fp32 in any order, so they equal the sums of the returned outputs."""
    M, N = 256, 320
    g = _gen(5000 + K)
    x = _ints(-2, 2, (M, K), g).half()
    w = _ints(-1, 1, (N, K), g).half()
    bias = (torch.arange(N, device=DEV) % 17 - 8).float()
    kw = dict()
    acc = x.float() @ w.float().t() + bias
    if "rvu" in kind:
        rowvec = _ints(-8, 8, (5, N), g)
        kw.update(rowvec=rowvec, rv=(64, 3, 1, 5))
        acc = acc + rowvec[((torch.arange(M, device=DEV) // 64) * 3) % 5]
    if "r1" in kind:
        r1 = _ints(-8, 8, (M, N), g).half()
        kw.update(r1=r1, s1=1.0)
        acc = acc + r1.float()
    out = ops.igemm(x, w, bias, tile=T320, stats=True, **kw)
    st = getattr(out, "gn_stats", None)
    assert st is not None, "the launch was expected to take the stats path"
    _assert_equal(out, acc.half(), f"stats {kind} outputs")
    o = out.float().reshape(M // 64, 64, N // 2, 2)
    ref = torch.stack([o.sum(dim=(1, 3)), (o * o).sum(dim=(1, 3))], dim=-1).reshape(M // 64, N)
    assert torch.equal(st[0], ref), f"stats {kind}: max difference {(st[0] - ref).abs().max().item()}"


@pytest.mark.parametrize("kind", ["plain", "rv", "r1", "r1+rvu", "silu", "geglu"])
def test_agrees_with_the_other_tiles_bit_for_bit(ops, kind):
    """On exact operands the 256x320 tile gives the bits of the 256x256 and 192x128 tiles.  SiLU and the GEGLU pair (gates from
    the MFMAs here, random) are compared with the 256x256 tile, which evaluates them with the same expressions."""
    M, N, K = 2309, 640, 512
    if kind in ("silu", "geglu"):
        from mofa_video_amd import lib as L
        from mofa_video_amd.weights import interleave_geglu
        x, w, bias, g = _operands(M, N, K, seed=6000)
        if kind == "geglu":
            w, bias = interleave_geglu(w, bias)
        act = L.ACT_SILU if kind == "silu" else L.ACT_GEGLU_PAIR
        a, b = (ops.igemm(x, w, bias, act=act, tile=t, split_k=False) for t in (T320, T256))
        assert torch.isfinite(a).all() and a.float().abs().max().item() > 1.0
        assert torch.equal(a, b), f"{kind}: {int((a != b).sum())} outputs differ from the 256x256 tile"
        return
    outs = {t: _run_gemm(ops, kind, M, N, K, seed=6000, tile=t) for t in (T320, T256, T192)}
    _assert_equal(outs[T320][0], outs[T320][1], f"{kind} 256x320")
    for t in (T256, T192):
        assert torch.equal(outs[T320][0], outs[t][0]), f"{kind}: differs from tile {t}"


def test_two_launches_bit_equal_on_random_data(ops):
    M, N, K = 2309, 640, 512
    g = _gen(7000)
    x = torch.randn(M, K, generator=g, device=DEV).half()
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.05).half()
    bias = torch.randn(N, generator=g, device=DEV)
    r1 = torch.randn(M, N, generator=g, device=DEV).half()
    first = ops.igemm(x, w, bias, r1=r1, s1=1.0, tile=T320, split_k=False).clone()
    assert torch.equal(ops.igemm(x, w, bias, r1=r1, s1=1.0, tile=T320, split_k=False), first)
    ref = x.float() @ w.float().t() + bias + r1.float()
    assert (first.float() - ref).abs().max().item() <= 2e-3 * ref.abs().max().item()
