"""GPU parity tests of every kernel behind the C ABI against plain fp32 PyTorch references (floating-point
kernels) and the CPU oracle (softsplat, scheduler math).  Inputs are seeded, asymmetric random data so a
transposed MFMA fragment or output layout cannot pass.

Tolerances (stated): fp16 storage, fp32 accumulate -> |err| <= 2e-3 * max|ref| + 2e-3 * |ref| per element
for GEMM-class kernels; 4e-3 for attention (P is rounded to fp16 before P.V).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _close(out, ref, tol=2e-3, what=""):
    out = out.float().cpu()
    ref = ref.float().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    scale = ref.abs().max().item() + 1e-12
    err = (out - ref).abs()
    bound = tol * scale + tol * ref.abs()
    bad = (err > bound)
    assert not bad.any(), (f"{what}: {bad.sum().item()} / {bad.numel()} elements out of tolerance; "
                           f"max err {err.max().item():.4e} (scale {scale:.4e}) at {err.argmax().item()}")


def _h(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


@pytest.fixture(scope="module")
def ops():
    from mofa_video_amd import ops as o
    from mofa_video_amd import lib
    lib.load()
    return o


# ---------------------------------------------------------------------------------------------------------
# implicit GEMM
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(300, 320, 192), (128, 128, 64), (1000, 4, 320), (77, 2560, 128)])
def test_igemm_plain_epilogue(ops, M, N, K):
    x, w = _h(M, K, seed=1), _h(N, K, seed=2, scale=0.1)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3))
    rowvec = torch.randn(5, N, generator=torch.Generator().manual_seed(4))
    r1, r2 = _h(M, N, seed=5), _h(M, N, seed=6)
    rv = (7, 3, 4, 5)  # idx = ((m/7)*3 + m%4) % 5
    out = ops.igemm(x.to(DEV), w.to(DEV), bias.to(DEV), rowvec=rowvec.to(DEV), rv=rv, r1=r1.to(DEV), s1=0.5,
                    r2=r2.to(DEV), s2=-1.25, s_acc=0.75)
    m = torch.arange(M)
    idx = ((m // 7) * 3 + m % 4) % 5
    ref = 0.75 * (x.float() @ w.float().t() + bias + rowvec[idx]) + 0.5 * r1.float() - 1.25 * r2.float()
    _close(out, ref, what="igemm plain")


def test_igemm_identity_asymmetric(ops):
    """A = I check with asymmetric B (guide rule: catches row/col swapped fragments)."""
    K = 128
    x = torch.eye(K).half()
    w = (torch.arange(K * K, dtype=torch.float32).reshape(K, K) % 251 / 251.0 - 0.3).half()  # w[n][k]
    out = ops.igemm(x.to(DEV), w.to(DEV))
    _close(out, w.float().t(), tol=1e-3, what="igemm identity")


def test_igemm_silu_and_strided_views(ops):
    M, N, K = 260, 192, 128
    xbig = _h(M, K + 64, seed=7)
    w = _h(N, K, seed=8, scale=0.1)
    outbig = torch.zeros(M, N + 64, dtype=torch.float16, device=DEV)
    ops.igemm(xbig.to(DEV)[:, 64:], w.to(DEV), act=1, out=outbig[:, 64:])
    ref = F.silu(xbig[:, 64:].float() @ w.float().t())
    _close(outbig[:, 64:], ref, what="igemm silu strided")
    assert outbig[:, :64].abs().max().item() == 0.0


def test_igemm_geglu_pair(ops):
    from mofa_video_amd.weights import interleave_geglu
    M, Cc = 200, 64
    x = _h(M, Cc, seed=9)
    w = _h(8 * Cc, Cc, seed=10, scale=0.2)
    b = torch.randn(8 * Cc, generator=torch.Generator().manual_seed(11))
    wi, bi = interleave_geglu(w, b)
    out = ops.igemm(x.to(DEV), wi.to(DEV).contiguous(), bi.to(DEV), act=2)
    h = x.float() @ w.float().t() + b
    ref = h[:, :4 * Cc] * F.gelu(h[:, 4 * Cc:])
    _close(out, ref, what="igemm geglu pair")


@pytest.mark.parametrize("stride,up,H,W", [(1, 1, 9, 13), (2, 1, 10, 14), (1, 2, 5, 7), (2, 1, 9, 13)])
def test_igemm_conv3x3(ops, stride, up, H, W):
    from mofa_video_amd.weights import pack_conv3x3
    n, Cin, Cout = 3, 64, 96
    x = _h(n, Cin, H, W, seed=12)
    w = _h(Cout, Cin, 3, 3, seed=13, scale=0.05)
    b = torch.randn(Cout, generator=torch.Generator().manual_seed(14))
    xt = x.permute(0, 2, 3, 1).reshape(n * H * W, Cin).contiguous()
    geom = ops.conv3x3_geom(H, W, stride=stride, up=up)
    out = ops.igemm(xt.to(DEV), pack_conv3x3(w).to(DEV), b.to(DEV), geom=geom)
    xi = x.float()
    if up == 2:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xi, w.float(), b, stride=stride, padding=1)
    assert (geom.Hout, geom.Wout) == tuple(ref.shape[2:])
    ref = ref.permute(0, 2, 3, 1).reshape(-1, Cout)
    _close(out, ref, what=f"conv3x3 s{stride} up{up}")


def test_igemm_convt3(ops):
    from mofa_video_amd.weights import pack_conv3d_t3
    B, T, HW, Cc = 2, 5, 33, 64
    x = _h(B, Cc, T, HW, 1, seed=15)
    w = _h(Cc, Cc, 3, 1, 1, seed=16, scale=0.1)
    b = torch.randn(Cc, generator=torch.Generator().manual_seed(17))
    xt = x[..., 0].permute(0, 2, 3, 1).reshape(B * T * HW, Cc).contiguous()
    out = ops.igemm(xt.to(DEV), pack_conv3d_t3(w).to(DEV), b.to(DEV), geom=ops.convt3_geom(T, HW))
    ref = F.conv3d(x.float(), w.float(), b, padding=(1, 0, 0))[..., 0].permute(0, 2, 3, 1).reshape(-1, Cc)
    _close(out, ref, what="conv3d (3,1,1)")


def test_igemm_large_k_accumulation(ops):
    M, N, K = 256, 256, 2560
    x, w = _h(M, K, seed=18), _h(N, K, seed=19, scale=0.05)
    out = ops.igemm(x.to(DEV), w.to(DEV))
    _close(out, x.float() @ w.float().t(), what="igemm K=2560")


def test_igemm_rejects_bad_args(ops):
    from mofa_video_amd.lib import MofaHipError
    x, w = _h(64, 48, seed=1).to(DEV), _h(64, 48, seed=2).to(DEV)  # Cin % 64 != 0
    with pytest.raises(MofaHipError):
        ops.igemm(x, w)


# ---------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,heads,frames,hd", [(200, 3, 2, 64), (64, 1, 1, 64), (16, 2, 3, 64), (1024, 5, 2, 64),
                                                 (200, 2, 2, 128), (576, 10, 1, 128), (16, 1, 2, 128)])
def test_attn_spatial(ops, S, heads, frames, hd):
    Cc = heads * hd
    qkv = _h(frames * S, 3 * Cc, seed=20)
    d = qkv.to(DEV)
    out = ops.attn_spatial(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], frames, heads, S, head_dim=hd)
    q, k, v = [t.float().reshape(frames, S, heads, hd).transpose(1, 2) for t in qkv.split(Cc, dim=1)]
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(frames * S, Cc)
    _close(out, ref, tol=4e-3, what="attn spatial")


def test_attn_spatial_online_softmax_rescale(ops):
    """Force the running max to jump at a late key tile (rare-branch test)."""
    S, heads, frames = 256, 1, 1
    qkv = _h(S, 192, seed=21, scale=0.5)
    qkv[200, 64:128] = qkv[5, 0:64] * 6.0  # key 200 strongly aligned with query 5
    d = qkv.to(DEV)
    out = ops.attn_spatial(d[:, :64], d[:, 64:128], d[:, 128:], frames, heads, S)
    q, k, v = [t.float().reshape(1, S, 1, 64).transpose(1, 2) for t in qkv.split(64, dim=1)]
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(S, 64)
    _close(out, ref, tol=4e-3, what="attn spatial rescale")


@pytest.mark.parametrize("hd,qb", [(64, 1), (64, 2), (128, 1)])
@pytest.mark.parametrize("pattern", ["rising", "falling", "spikes"])
def test_attn_spatial_reference_moves(ops, hd, qb, pattern):
    """The kernel exponentiates scores relative to a REFERENCE that is only moved when a key tile's probabilities near the
    fp16 range.  Logits spanning hundreds of units: rising along the keys (the reference must move tile after tile, each
    time rescaling O and l), falling (everything after the first tiles underflows to 0 exactly as in the reference), and
    isolated spikes in late tiles -- against fp32 softmax attention."""
    S = 1024 if qb == 2 else 200                       # 64 queries per wave need S % 256 == 0 and enough workgroups
    frames, heads = (64, 4) if qb == 2 else (2, 1)
    Cc = heads * hd
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
    k = k * gain[:, None]
    qkv = torch.cat([q, k, v], 1).half()
    d = qkv.to(DEV)
    out = ops.attn_spatial(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], frames, heads, S, head_dim=hd, query_blocks=qb)
    qf, kf, vf = [t.float().reshape(frames, S, heads, hd).transpose(1, 2) for t in d.split(Cc, dim=1)]   # fp32, on the GPU
    ref, top = [], 0.0
    for f0 in range(0, frames, 8):
        logits = (qf[f0:f0 + 8] @ kf[f0:f0 + 8].transpose(-1, -2)) * hd ** -0.5
        top = max(top, logits.abs().max().item())
        ref.append((torch.softmax(logits, -1) @ vf[f0:f0 + 8]).transpose(1, 2).reshape(-1, Cc))
    assert top > 40                                     # well outside what fp16 probabilities hold without moving
    _close(out, torch.cat(ref, 0), tol=4e-3, what=f"attn spatial reference moves ({pattern})")
    # the production form: head_dim^-0.5 * log2(e) folded into Q before its (single) fp16 rounding, 1.5 x the logits
    from mofa_video_amd.ops import Q_FOLD_LOG2E
    qs = (d[:, :Cc].float() * 1.5 * (hd ** -0.5 * Q_FOLD_LOG2E)).half()
    out = ops.attn_spatial(qs, d[:, Cc:2 * Cc], d[:, 2 * Cc:], frames, heads, S, head_dim=hd, prescaled=True, query_blocks=qb)
    qf = qs.float().reshape(frames, S, heads, hd).transpose(1, 2)
    ref, top = [], 0.0
    for f0 in range(0, frames, 8):
        logits = (qf[f0:f0 + 8] @ kf[f0:f0 + 8].transpose(-1, -2)) * 0.6931471805599453    # exp2 domain -> natural
        top = max(top, logits.abs().max().item())
        ref.append((torch.softmax(logits, -1) @ vf[f0:f0 + 8]).transpose(1, 2).reshape(-1, Cc))
    assert top > 60
    _close(out, torch.cat(ref, 0), tol=4e-3, what=f"attn spatial, Q pre-scaled, reference moves ({pattern})")


@pytest.mark.parametrize("T,HW,heads,clips,hd", [(25, 37, 2, 2, 64), (8, 16, 1, 2, 64), (32, 5, 3, 1, 64), (1, 9, 1, 1, 64),
                                                 (25, 19, 2, 2, 128), (32, 3, 1, 1, 128)])
def test_attn_temporal(ops, T, HW, heads, clips, hd):
    Cc = heads * hd
    qkv = _h(clips * T * HW, 3 * Cc, seed=22)
    d = qkv.to(DEV)
    out = ops.attn_temporal(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], clips, T, HW, heads, head_dim=hd)
    q, k, v = [t.float().reshape(clips, T, HW, heads, hd).permute(0, 2, 3, 1, 4) for t in qkv.split(Cc, dim=1)]
    ref = F.scaled_dot_product_attention(q, k, v)  # [clips, HW, heads, T, 64]
    ref = ref.permute(0, 3, 1, 2, 4).reshape(clips * T * HW, Cc)
    _close(out, ref, tol=2e-3, what="attn temporal")


def test_softmax_rows_and_transpose(ops):
    x = _h(33, 520, seed=23, scale=3.0)
    out = ops.softmax_rows_(x.to(DEV).clone())
    _close(out, torch.softmax(x.float(), dim=1), what="softmax rows")
    frames, heads, S = 2, 3, 200
    v = _h(frames * S, heads * 64 + 64, seed=24)
    vt = ops.transpose_v(v.to(DEV)[:, 64:], frames, heads, S)
    ref = v[:, 64:].reshape(frames, S, heads, 64).permute(0, 2, 3, 1).reshape(frames * heads * 64, S)
    assert torch.equal(vt.cpu(), ref)


# ---------------------------------------------------------------------------------------------------------
# normalisation
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,HW,frames,fps", [(320, 300, 4, 1), (64, 37, 6, 3), (2560, 20, 2, 1), (128, 5000, 2, 2)])
@pytest.mark.parametrize("silu", [False, True])
def test_group_norm(ops, C, HW, frames, fps, silu):
    x = _h(frames * HW, C, seed=25) + 0.5
    g = torch.randn(C, generator=torch.Generator().manual_seed(26))
    b = torch.randn(C, generator=torch.Generator().manual_seed(27))
    out = ops.group_norm(x.to(DEV), g.to(DEV), b.to(DEV), frames, HW, 1e-5, frames_per_stat=fps, silu=silu)
    xr = x.float().reshape(frames // fps, fps * HW, C).transpose(1, 2)  # [stat, C, L]
    ref = F.group_norm(xr, 32, g, b, eps=1e-5)
    if silu:
        ref = F.silu(ref)
    ref = ref.transpose(1, 2).reshape(frames * HW, C)
    _close(out, ref, what="group norm")


@pytest.mark.parametrize("C", [64, 320, 1280])
def test_layer_norm(ops, C):
    M = 101
    x = _h(M, C, seed=28) * 2 + 0.3
    g = torch.randn(C, generator=torch.Generator().manual_seed(29))
    b = torch.randn(C, generator=torch.Generator().manual_seed(30))
    rv = torch.randn(3, C, generator=torch.Generator().manual_seed(31))
    out = ops.layer_norm(x.to(DEV), g.to(DEV), b.to(DEV), 1e-5, rowvec=rv.to(DEV), rv_div=10, rv_mod=3)
    idx = (torch.arange(M) // 10) % 3
    ref = F.layer_norm(x.float() + rv[idx], (C,), g, b, 1e-5)
    _close(out, ref, what="layer norm + rowvec")
    out2 = ops.layer_norm(x.to(DEV), g.to(DEV), b.to(DEV), 1e-5)
    _close(out2, F.layer_norm(x.float(), (C,), g, b, 1e-5), what="layer norm")


# ---------------------------------------------------------------------------------------------------------
# element-wise
# ---------------------------------------------------------------------------------------------------------
def test_elementwise(ops):
    x, y = _h(50, 64, seed=32), _h(50, 64, seed=33)
    out = ops.axpby_(x.to(DEV), y.to(DEV).clone(), 0.5, 2.0)
    _close(out, 0.5 * x.float() + 2.0 * y.float(), tol=1e-3, what="axpby")
    g = _h(50, 256, seed=34)
    _close(ops.geglu(g.to(DEV)), g[:, :128].float() * F.gelu(g[:, 128:].float()), tol=1e-3, what="geglu")
    a, b = _h(40, 64, seed=35), _h(40, 128, seed=36)
    cat = ops.concat_channels(a.to(DEV), b.to(DEV))
    assert torch.equal(cat.cpu(), torch.cat([a, b], 1))
    v = torch.randn(300, generator=torch.Generator().manual_seed(37))
    _close(ops.silu_f32(v.to(DEV)), F.silu(v), tol=1e-5, what="silu f32")
    img = torch.randn(2, 3, 7, 9, generator=torch.Generator().manual_seed(38))
    tok = ops.nchw_to_tokens(img.to(DEV), ld=64)
    assert tok.shape == (2 * 63, 64) and tok[:, 3:].abs().max().item() == 0
    _close(tok[:, :3], img.permute(0, 2, 3, 1).reshape(-1, 3), tol=1e-3, what="nchw->tokens")
    back = ops.tokens_to_nchw(tok, 2, 3, 7, 9)
    _close(back, img.half().float(), tol=1e-6, what="tokens->nchw")
    assert torch.equal(ops.cast_f16_to_f32(ops.cast_f32_to_f16(v.to(DEV))).cpu(), v.half().float())


def test_timestep_embedding_and_flow_downscale(ops):
    from oracle.blocks import get_timestep_embedding
    t = torch.tensor([1.6378, 6.0, 128.0, 0.02, 24.0])
    out = ops.timestep_embedding(t.to(DEV), 320)
    ref = get_timestep_embedding(t, 320, flip_sin_to_cos=True, downscale_freq_shift=0)
    _close(out, ref, tol=2e-5, what="timestep embedding")
    flow = torch.randn(3, 2, 64, 128, generator=torch.Generator().manual_seed(39)) * 20
    for s in (8, 16, 32, 64):
        ref = F.interpolate(flow, scale_factor=1 / s) / s
        out = ops.flow_downscale(flow.to(DEV), s)
        assert torch.equal(out.cpu(), ref)


# ---------------------------------------------------------------------------------------------------------
# softsplat (vs the CPU oracle) and scheduler math
# ---------------------------------------------------------------------------------------------------------
def _flows(n, H, W, seed, mag):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n, 2, H, W, generator=g) * mag
    f[0, :, 0, 0] = float("nan")            # non-finite flow is skipped (softsplat.py:301-302)
    f[-1, 0, 1, 1] = float("inf")
    f[0, :, 2, 2] = torch.tensor([1.0, -2.0])  # integer shift
    f[0, :, 3, 3] = torch.tensor([1000.0, 5.0])  # out of bounds
    return f


@pytest.mark.parametrize("H,W,C,mag", [(9, 16, 64, 1.5), (18, 32, 128, 4.0), (36, 64, 320, 0.3)])
def test_softsplat_gather_vs_oracle(ops, H, W, C, mag):
    from oracle.softsplat import softsplat
    nfl = 5
    feat = _h(1, C, H, W, seed=40)
    flow = _flows(nfl, H, W, 41, mag)
    tok = feat[0].permute(1, 2, 0).reshape(H * W, C).contiguous()
    out = ops.softsplat_avg_tokens(tok.to(DEV), flow.to(DEV), H, W)
    ref = torch.stack([softsplat(feat.float(), flow[i:i + 1], None, "avg")[0] for i in range(nfl)])
    ref = ref.permute(0, 2, 3, 1).reshape(nfl * H * W, C)
    _close(out, ref, tol=1.5e-3, what="softsplat gather")
    # deterministic: bitwise reproducible run to run
    out2 = ops.softsplat_avg_tokens(tok.to(DEV), flow.to(DEV), H, W)
    assert torch.equal(out, out2)


def test_softsplat_convergent_flow(ops):
    """every source splats onto (nearly) one pixel: segments of up to 4 HW entries on a target -- the per-target ordering
    must stay bounded in time (heap sort beyond 48 entries) and equal the oracle; run to run bit-identical"""
    import time
    from oracle.softsplat import softsplat
    H, W, C = 72, 128, 64
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    flow = torch.stack([40.3 - xs, 30.6 - ys], 0)[None].repeat(2, 1, 1, 1)       # all sources -> (40.3, 30.6)
    flow[1] = flow[1] * 0.9                                                       # second flow: a tight cluster
    feat = _h(1, C, H, W, seed=45)
    tok = feat[0].permute(1, 2, 0).reshape(H * W, C).contiguous()
    out = ops.softsplat_avg_tokens(tok.to(DEV), flow.to(DEV), H, W)
    torch.cuda.synchronize()
    t0 = time.time()
    out2 = ops.softsplat_avg_tokens(tok.to(DEV), flow.to(DEV), H, W)
    torch.cuda.synchronize()
    assert time.time() - t0 < 1.0                        # the quadratic sort took seconds on 36 864 entries
    assert torch.equal(out, out2)
    ref = torch.stack([softsplat(feat.float(), flow[i:i + 1], None, "avg")[0] for i in range(2)])
    _close(out, ref.permute(0, 2, 3, 1).reshape(2 * H * W, C), tol=1.5e-3, what="softsplat, convergent flow")


def test_softsplat_scatter_vs_oracle(ops):
    from oracle.softsplat import softsplat_sum
    N, C, H, W = 2, 7, 12, 20
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(42))
    flow = _flows(N, H, W, 43, 2.0)
    out = ops.softsplat_scatter_f32(x.to(DEV), flow.to(DEV))
    _close(out, softsplat_sum(x, flow), tol=1e-5, what="softsplat scatter")


@pytest.mark.parametrize("mode", ["linear", "soft", "linear-zeroeps", "soft-clipeps", "soft-addeps", "avg-zeroeps", "avg", "sum", "sum-addeps"])
def test_softsplat_modes_vs_oracle(mode):
    """the reference wrapper's strMode surface (Traj/models/softsplat.py:232-274) through mofa_video_amd.softsplat, vs the oracle"""
    from mofa_video_amd.softsplat import softsplat as splat
    from oracle.softsplat import softsplat as splat_ref
    N, C, H, W = 2, 8, 12, 20
    g = torch.Generator().manual_seed(52)
    x = torch.randn(N, C, H, W, generator=g)
    if mode == "avg":
        x = x.half().float()                      # (the 'avg' path works on fp16 features)
    if mode == "avg-zeroeps":
        x = x.abs() + 0.1                         # (reference quirk: 'avg-<suffix>' normalises by the input's own last channel)
    metric = torch.randn(N, 1, H, W, generator=g) if mode.split("-")[0] in ("linear", "soft") else None
    if mode.startswith("linear"):
        metric = metric.abs() + 0.1               # a positive importance metric, as the mode is meant for
    flow = _flows(N, H, W, 53, 2.0)
    out = splat(x.to(DEV), flow.to(DEV), metric.to(DEV) if metric is not None else None, mode)
    ref = splat_ref(x, flow, metric, mode)
    _close(out, ref, tol=1.5e-3 if mode == "avg" else 2e-5, what=f"softsplat {mode}")


def test_scheduler_kernels_vs_oracle(ops):
    from oracle.scheduler import EulerDiscreteScheduler
    T, h, w = 5, 6, 8
    g = torch.Generator().manual_seed(44)
    lat = torch.randn(T, 4, h, w, generator=g) * 50
    img = torch.randn(2, 4, h, w, generator=g)
    npred = (torch.randn(2, T, h * w, 4, generator=g)).half()
    sch = EulerDiscreteScheduler()
    sch.set_timesteps(25)
    i = 3
    sigma, sigma_next = sch.sigmas[i].item(), sch.sigmas[i + 1].item()
    out = torch.zeros(2 * T * h * w, 64, dtype=torch.float16, device=DEV)
    ops.prepare_model_input(lat.to(DEV), img.to(DEV), out, sigma)
    ref_lat = (lat / (sigma ** 2 + 1) ** 0.5).permute(0, 2, 3, 1).reshape(T * h * w, 4)
    ref_img = img.permute(0, 2, 3, 1).reshape(2, h * w, 4)
    for half in range(2):
        blk = out[half * T * h * w:(half + 1) * T * h * w]
        _close(blk[:, :4], ref_lat, tol=1e-3, what="model input latents")
        _close(blk[:, 4:8].reshape(T, h * w, 4), ref_img[half].expand(T, -1, -1), tol=1e-3, what="model input image")
        assert blk[:, 8:].abs().max().item() == 0
    # CFG + Euler vs the oracle scheduler
    sch._step_index = i
    npf = npred.float().reshape(2, T, h, w, 4).permute(0, 1, 4, 2, 3)  # [2,T,4,h,w]
    gs = torch.linspace(1.0, 3.0, T).view(T, 1, 1, 1)
    v = npf[0] + gs * (npf[1] - npf[0])
    ref = sch.step(v, sch.timesteps[i], lat)
    latd = lat.to(DEV).clone()
    ops.cfg_euler_step_(latd, npred.to(DEV).reshape(2 * T * h * w, 4), sigma, sigma_next, 1.0, 3.0)
    _close(latd, ref, tol=1e-5, what="cfg + euler")


# the device-scalar forms every denoise step of the headline path calls (pipeline.py: prepare_model_input_dev, cfg_euler_step_dev_,
# step_select as the first node of the captured step): the step's scalars come from a row of the per-clip table on the device
def _step_table():
    from mofa_video_amd.scheduler import EulerDiscreteScheduler
    sch = EulerDiscreteScheduler()
    sch.set_timesteps(25)
    return torch.from_numpy(sch.step_table().copy())


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_step_select_walks_the_table_and_clamps_at_the_last_row(ops):
    tab_h = _step_table()
    n = tab_h.shape[0]
    assert tab_h.shape == (25, ops.STEP_SCALARS)
    tab = tab_h.to(DEV)
    cur_buf = torch.full((24,), float("nan"), device=DEV)                     # cur = words 8 .. 15 between guard words
    cnt_buf = torch.tensor([0x5A5A5A5A, 0, 0x3C3C3C3C], dtype=torch.int32, device=DEV)
    cur, counter = cur_buf[8:16], cnt_buf[1:2]
    guard0 = cur_buf.clone()
    for i in range(n + 2):
        ops.step_select(tab, counter, cur)
        row = min(i, n - 1)
        assert torch.equal(_bits(cur).cpu(), _bits(tab_h[row])), f"call {i}: cur is not row {row}"
        assert cnt_buf.tolist() == [0x5A5A5A5A, i + 1, 0x3C3C3C3C], (i, cnt_buf.tolist())
        assert torch.equal(_bits(cur_buf[:8]), _bits(guard0[:8])) and torch.equal(_bits(cur_buf[16:]), _bits(guard0[16:])), f"call {i}"
    assert torch.equal(_bits(tab.cpu()), _bits(tab_h))


def _scheduler_case(T, h, w, seed=44):
    """latents, image latents, and the network's prediction / the model input as views (ldn = 16 > 4, ldo = 24 > 8) into
    NaN-filled guard buffers"""
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(T, 4, h, w, generator=g) * 50
    img = torch.randn(2, 4, h, w, generator=g)
    npred = torch.randn(2 * T * h * w, 4, generator=g).half()
    M = 2 * T * h * w
    np_buf = torch.full((M + 4, 16), float("nan"), dtype=torch.float16)
    np_buf[2:2 + M, 4:8] = npred
    return lat, img, npred, np_buf, M


def _model_input(ops, lat, img, M, scal):
    """-> (buffer, view [M, 16] at ldo = 24) written by the host-scalar form (scal a float) or the device-scalar form"""
    buf = torch.full((M + 4, 24), float("nan"), dtype=torch.float16, device=DEV)
    before = buf.clone()
    view = buf[2:2 + M, 8:24]
    if torch.is_tensor(scal):
        ops.prepare_model_input_dev(lat.to(DEV), img.to(DEV), view, scal)
    else:
        ops.prepare_model_input(lat.to(DEV), img.to(DEV), view, scal)
    keep = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    keep[2:2 + M, 8:16] = False                                               # the 8 written columns of the view's rows
    assert torch.equal(_bits(buf)[keep], _bits(before)[keep]), "model input: columns >= 8 or guard rows / columns were written"
    assert torch.isfinite(view[:, :8]).all()
    return view[:, :8].cpu()


@pytest.mark.parametrize("T", [1, 5])
def test_device_scalar_scheduler_kernels(ops, T):
    """the device-scalar forms on rows of scheduler.step_table() (first, last -- sigma_next == 0 --, and two between) against
    (a) the host-scalar forms given the same row's sigma / sigma_next as Python floats: latents bit-equal (same kernel, scalars
    from another source), fp16 model input within 1 fp16 ulp (the host form computes 1 / sqrt(sigma^2 + 1) in the launcher, the
    table carries it pre-computed by numpy), and (b) the oracle scheduler at the tolerances of test_scheduler_kernels_vs_oracle.
    T = 1 takes the g = gmin branch of the guidance ramp."""
    from oracle.scheduler import EulerDiscreteScheduler
    h, w = 6, 8
    tab_h = _step_table()
    tab = tab_h.to(DEV)
    n = tab_h.shape[0]
    sch = EulerDiscreteScheduler()
    sch.set_timesteps(n)
    assert tab_h[n - 1, 1].item() == 0.0
    lat, img, npred, np_buf, M = _scheduler_case(T, h, w)
    for i in (0, 3, 12, n - 1):
        sigma, sigma_next = tab_h[i, 0].item(), tab_h[i, 1].item()
        assert abs(sigma - sch.sigmas[i].item()) <= 1e-6 * sigma and abs(sigma_next - sch.sigmas[i + 1].item()) <= 1e-6 * sigma
        # model input
        x_dev = _model_input(ops, lat, img, M, tab[i])
        x_host = _model_input(ops, lat, img, M, sigma)
        ulps = (_bits(x_dev[:, :4]).int() - _bits(x_host[:, :4]).int()).abs().max().item()
        print(f"T={T} row {i}: model input, device-scalar vs host-scalar form: {ulps} fp16 ulp")
        assert ulps <= 1, (i, ulps)
        assert torch.equal(x_dev[:, 4:], x_host[:, 4:])
        ref_lat = (lat / (sigma ** 2 + 1) ** 0.5).permute(0, 2, 3, 1).reshape(T * h * w, 4)
        ref_img = img.permute(0, 2, 3, 1).reshape(2, h * w, 4)
        for half in range(2):
            blk = x_dev[half * T * h * w:(half + 1) * T * h * w]
            _close(blk[:, :4], ref_lat, tol=1e-3, what=f"row {i}: model input latents (device scalars)")
            _close(blk[:, 4:8].reshape(T, h * w, 4), ref_img[half].expand(T, -1, -1), tol=1e-3, what=f"row {i}: model input image")
        # CFG + Euler
        npd = np_buf.to(DEV)
        np_before = npd.clone()
        lat_dev, lat_host = lat.to(DEV).clone(), lat.to(DEV).clone()
        ops.cfg_euler_step_dev_(lat_dev, npd[2:2 + M, 4:8], tab[i], 1.0, 3.0)
        ops.cfg_euler_step_(lat_host, npd[2:2 + M, 4:8], sigma, sigma_next, 1.0, 3.0)
        assert torch.equal(_bits(npd), _bits(np_before))
        assert torch.equal(_bits(lat_dev), _bits(lat_host)), f"row {i}: device-scalar and host-scalar Euler steps differ"
        sch._step_index = i
        npf = npred.float().reshape(2, T, h, w, 4).permute(0, 1, 4, 2, 3)      # [2,T,4,h,w]
        gs = (torch.linspace(1.0, 3.0, T) if T > 1 else torch.tensor([1.0])).view(T, 1, 1, 1)
        v = npf[0] + gs * (npf[1] - npf[0])
        _close(lat_dev, sch.step(v, sch.timesteps[i], lat), tol=1e-5, what=f"row {i}: cfg + euler (device scalars)")
    assert torch.equal(_bits(tab.cpu()), _bits(tab_h))


# ---------------------------------------------------------------------------------------------------------
# kernels of the landmark / Hybrid / Keypoint paths
# ---------------------------------------------------------------------------------------------------------
def test_igemm_conv7x7_relu(ops):
    from mofa_video_amd.weights import pack_conv3x3, pad_rows
    n, Cin, Cout, H, W = 2, 64, 1, 11, 9
    x = _h(n, Cin, H, W, seed=50)
    w = _h(Cout, Cin, 7, 7, seed=51, scale=0.03)
    b = torch.randn(Cout, generator=torch.Generator().manual_seed(52))
    xt = x.permute(0, 2, 3, 1).reshape(n * H * W, Cin).contiguous()
    out = ops.igemm(xt.to(DEV), pack_conv3x3(pad_rows(w)).to(DEV), pad_rows(b).to(DEV), geom=ops.conv3x3_geom(H, W, ksize=7),
                    act=3)
    ref = F.relu(F.conv2d(x.float(), w.float(), b, padding=3)).permute(0, 2, 3, 1).reshape(-1, 1)
    _close(out[:, :1], ref, what="conv7x7 + relu")
    assert out[:, 1:].abs().max().item() == 0


def test_blend_resize_subsample_axpby(ops):
    M, C, HW = 6 * 35, 64, 35
    a, b = _h(M, C, seed=53), _h(M, C, seed=54)
    w = torch.rand(HW, generator=torch.Generator().manual_seed(55))
    out = ops.mask_blend(a.to(DEV), b.to(DEV), w.to(DEV), HW)
    wr = w.repeat(M // HW)[:, None]
    _close(out, a.float() * wr + b.float() * (1 - wr), tol=1e-3, what="mask blend")
    lg = _h(M, 8, seed=56, scale=2.0)
    o2, mk = ops.matting_blend(a.to(DEV), b.to(DEV), lg.to(DEV))
    m = torch.sigmoid(lg[:, :1].float())
    _close(o2, a.float() * m + b.float() * (1 - m), tol=1e-3, what="matting blend")
    _close(mk, m[:, 0], tol=1e-5, what="matting mask")
    msk = torch.rand(2, 48, 80, generator=torch.Generator().manual_seed(57))
    for (h2, w2) in [(6, 10), (12, 20), (5, 7)]:
        ref = F.interpolate(msk[None], (h2, w2), mode="nearest")[0]
        assert torch.equal(ops.resize_nearest_f32(msk.to(DEV), h2, w2).cpu(), ref)
    t = _h(3 * 8 * 12, 64, seed=58)
    sub = ops.subsample_tokens(t.to(DEV), 3, 8, 12, 2)
    ref = F.interpolate(t.reshape(3, 8, 12, 64).permute(0, 3, 1, 2).float(), scale_factor=0.5).permute(0, 2, 3, 1)
    assert torch.equal(sub.cpu().float(), ref.reshape(-1, 64))
    x32 = torch.randn(1000, generator=torch.Generator().manual_seed(59))
    y32 = torch.randn(1000, generator=torch.Generator().manual_seed(60))
    got = ops.axpby_f32_(x32.to(DEV), y32.to(DEV).clone(), 0.25, 1.0)
    _close(got, 0.25 * x32 + y32, tol=1e-6, what="axpby f32")
    got = ops.axpby_f32_(x32.to(DEV), torch.full((1000,), float("nan"), device=DEV), 0.5, 0.0)   # b == 0 overwrites
    _close(got, 0.5 * x32, tol=1e-6, what="axpby f32 overwrite")


def test_igemm_unclipped_temporal_halo(ops):
    """MOFA_MODE_CONVT3 with T = 0: the caller supplies halo frames (frame-sharded clips)."""
    from mofa_video_amd.weights import pack_conv3d_t3
    T, HW, Cc = 6, 10, 64
    x = _h(1, Cc, T, HW, 1, seed=61)
    w = _h(Cc, Cc, 3, 1, 1, seed=62, scale=0.1)
    full = F.conv3d(x.float(), w.float(), None, padding=(1, 0, 0))[0, :, :, :, 0].permute(1, 2, 0)   # [T,HW,C]
    xt = x[0, :, :, :, 0].permute(1, 2, 0).reshape(T * HW, Cc).contiguous().to(DEV)                  # [T*HW, C]
    f0, f1 = 2, 5                                                 # this "rank" owns frames 2..4, halo = frames 1 and 5
    ext = xt[(f0 - 1) * HW:(f1 + 1) * HW].contiguous()
    out = ops.igemm(ext[HW:], pack_conv3d_t3(w).to(DEV), None, geom=ops.convt3_geom(0, HW), M=(f1 - f0) * HW)
    _close(out, full[f0:f1].reshape(-1, Cc), what="unclipped temporal conv with halo")


def test_attn_temporal_sharded_queries(ops):
    T, Tq, HW, heads = 7, 3, 9, 2
    Cc = heads * 64
    qkv = _h(T * HW, 3 * Cc, seed=63)
    d = qkv.to(DEV)
    full = ops.attn_temporal(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], 1, T, HW, heads)
    f0 = 2
    q = d[f0 * HW:(f0 + Tq) * HW, :Cc]
    kv = d[:, Cc:].contiguous()
    part = ops.attn_temporal(q, kv[:, :Cc], kv[:, Cc:], 1, T, HW, heads, Tq=Tq)
    assert torch.equal(part, full[f0 * HW:(f0 + Tq) * HW])


@pytest.mark.parametrize("T,R,hd", [(25, 4, 64), (25, 2, 64), (7, 2, 128), (5, 4, 64), (32, 4, 64)])
def test_attn_temporal_masked_padded_shards(ops, T, R, hd):
    """K|V laid out as the frame-sharded all-gather leaves them: R slots of T_max frames, the shorter shards' padding
    frames holding NaN (never-written memory); with the key mask the result equals attention over the T real frames"""
    from mofa_video_amd.parallel import split_frames
    HW, heads = 11, 2
    Cc = heads * hd
    qkv = _h(T * HW, 3 * Cc, seed=64)
    d = qkv.to(DEV)
    full = ops.attn_temporal(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], 1, T, HW, heads, head_dim=hd)
    bounds = split_frames(T, R)
    T_max = bounds[0][1] - bounds[0][0]
    pad = torch.full((R * T_max * HW, 2 * Cc), float("nan"), dtype=torch.float16, device=DEV)
    mask = 0
    for s_, (a, b) in enumerate(bounds):
        pad[s_ * T_max * HW:(s_ * T_max + b - a) * HW] = d[a * HW:b * HW, Cc:]
        mask |= ((1 << (b - a)) - 1) << (s_ * T_max)
    for (a, b) in bounds:                                           # every shard's queries against the padded buffer
        part = ops.attn_temporal(d[a * HW:b * HW, :Cc], pad[:, :Cc], pad[:, Cc:], 1, R * T_max, HW, heads, head_dim=hd,
                                 Tq=b - a, key_mask=mask)
        assert torch.isfinite(part).all()
        _close(part, full[a * HW:b * HW].float().cpu(), tol=1e-3, what="masked temporal attention")
    with pytest.raises(Exception):                                  # an all-zero mask is an argument error, not a NaN
        ops.attn_temporal(d[:HW, :Cc], pad[:, :Cc], pad[:, Cc:], 1, R * T_max, HW, heads, head_dim=hd, Tq=1, key_mask=0)


@pytest.mark.parametrize("N,kinds", [(64, ("r1",)), (64, ("r1", "rv")), (64, ("bias", "r1", "r2", "rv")), (256, ("r1",)),
                                     (256, ("bias",)), (128, ("bias", "r1"))])
def test_igemm_repeat_launches_bit_identical(ops, N, kinds):
    """Regression for an intermittent epilogue fault (dropped residual term in lanes 48..63 of the 128x128-tile kernel,
    see the comment on the scale factors in csrc/igemm.hip): repeated launches of one conv + epilogue must agree bit
    for bit, and with a torch fp32 reference within fp16 rounding."""
    torch.manual_seed(5)
    n, H, W, C = 4, 128, 128, 64
    x = torch.randn(n * H * W, C, device=DEV).half()
    w = (torch.randn(N, 9 * C, device=DEV) * 0.05).half()
    kw = {}
    if "bias" in kinds:
        kw["bias"] = torch.randn(N, device=DEV)
    if "r1" in kinds:
        kw["r1"] = torch.randn(n * H * W, N, device=DEV).half()
    if "r2" in kinds:
        kw["r2"] = torch.randn(n * H * W, N, device=DEV).half()
        kw["s2"] = 0.5
    if "rv" in kinds:
        kw["rowvec"] = torch.randn(n, N, device=DEV)
        kw["rv"] = (H * W, 1, 1, n)
    g = ops.conv3x3_geom(H, W)
    outs = [ops.igemm(x, w, geom=g, **kw).clone() for _ in range(6)]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    ref = torch.nn.functional.conv2d(x.view(n, H, W, C).permute(0, 3, 1, 2).float(),
                                     w.view(N, 3, 3, C).permute(0, 3, 1, 2).float(), padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, N)
    if "bias" in kinds:
        ref = ref + kw["bias"]
    if "rv" in kinds:
        ref = ref + kw["rowvec"].repeat_interleave(H * W, 0)
    if "r1" in kinds:
        ref = ref + kw["r1"].float()
    if "r2" in kinds:
        ref = ref + 0.5 * kw["r2"].float()
    _close(outs[0], ref, tol=4e-3, what="conv + epilogue vs torch fp32")
