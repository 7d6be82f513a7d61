"""Cases and models of the folded up-sampler convolution (MOFA_MODE_CONV3X3_UP2F, include/mofa_hip.h), shared by
test_up2_fold_cpu.py and test_igemm_up2_fold_gpu.py:

  * small-integer data on which every sum is exact in fp16 / fp32 / fp64 alike (x in -2..2, weights in -1..1, integer bias);
  * the reference: ``F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)`` in fp64;
  * ``folded_conv``: the algebra alone -- four 2x2 convolutions with ``weights.fold_up2``'s weights, one per output parity;
  * ``launch_model``: the launch AS THE KERNELS ADDRESS IT -- phase-padded 256-row tiles, the exported row map
    (``mofa_igemm_up2f_row``), the per-tile weight base, the tap origin 1 - a / 1 - b -- and its mutants;
  * ``make_args``: the ``mofa_igemm_args`` of such a launch on never dereferenced addresses, for the plan queries."""
import ctypes

import torch
import torch.nn.functional as F

from mofa_video_amd import lib as L
from mofa_video_amd.weights import fold_up2

GEOMS = [(2, 1, 1), (1, 1, 4), (1, 3, 1), (3, 2, 3), (2, 5, 7)]          # (nimg, H, W)
CINS = (3, 64)                                                            # 3 is padded to 64
# the six up-sampler launches of the bench: (nimg, Hin, Win, Cin, N); rows out x N x 9 Cin = 28 800 x 1280 x 11 520, ...
BENCH = [(50, 9, 16, 1280, 1280), (50, 18, 32, 1280, 1280), (50, 36, 64, 640, 640),
         (8, 72, 128, 512, 512), (8, 144, 256, 512, 512), (8, 288, 512, 256, 256)]
X, W, B, OUT, WS = 0x10000, 0x20000000, 0x30000, 0x40000000, 0x50000000   # aligned, never dereferenced
WS_BYTES = 256 * 256 * 320 * 4
MUTANTS = ("taps_swapped", "tytx_swapped", "phase_2b_a", "origin_no_phase", "padding_stored", "wbase_fixed")


def int_data(nimg, H, Wd, Cin, N, seed=0):
    """(x [nimg, Cin, H, W], w [N, Cin, 3, 3], b [N]) of small integers, fp64"""
    g = torch.Generator().manual_seed(seed + 1000 * nimg + 100 * H + 10 * Wd + Cin)
    x = torch.randint(-2, 3, (nimg, Cin, H, Wd), generator=g).double()
    w = torch.randint(-1, 2, (N, Cin, 3, 3), generator=g).double()
    b = torch.randint(-3, 4, (N,), generator=g).double()
    return x, w, b


def reference(x, w, b):
    """fp64 [nimg, N, 2H, 2W]"""
    return F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), None if b is None else b.double(), padding=1)


def tokens(t):
    """[nimg, C, H, W] -> token-major [nimg * H * W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def pad_channels(x, Cp):
    return torch.cat([x, x.new_zeros(x.shape[0], Cp - x.shape[1], *x.shape[2:])], 1) if Cp > x.shape[1] else x


def folded_conv(x, wf, b):
    """the four 2x2 convolutions: wf = fold_up2(w) as [4N, 4 Cinpad]; phase (a, b) pads one row above / left for a, b = 0 and one
    below / right for 1 -- the taps the classic form pads"""
    N, Cp = wf.shape[0] // 4, wf.shape[1] // 4
    xp = pad_channels(x.double(), Cp)
    n, _, H, Wd = xp.shape
    out = xp.new_zeros(n, N, 2 * H, 2 * Wd)
    for p in range(4):
        a, bb = p >> 1, p & 1
        k = wf[p * N:(p + 1) * N].double().reshape(N, 2, 2, Cp).permute(0, 3, 1, 2)
        out[:, :, a::2, bb::2] = F.conv2d(F.pad(xp, (1 - bb, bb, 1 - a, a)), k, None if b is None else b.double())
    return out


def make_args(nimg, H, Wd, Cin, N, tile=0, ws=True, **fields):
    a = L.IgemmArgs(x=X, w=W, bias=B, out=OUT, M=nimg * 4 * H * Wd, N=N, Cin=Cin, ldx=Cin, ldo=N, mode=L.MODE_CONV3X3_UP2F,
                    Hin=H, Win=Wd, Hout=2 * H, Wout=2 * Wd, stride=1, up=2, ksize=3, rv_div=1, rv_mul=1, rv_mod_in=1, rv_mod_out=1 << 30,
                    act=L.ACT_NONE, s_acc=1.0, s1=1.0, s2=1.0, dil=1, pad=L.PAD_SAME, tile=tile,
                    workspace=WS if ws else None, workspace_bytes=WS_BYTES if ws else 0)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def plan(a, n_cu=256):
    p = L.IgemmPlan()
    assert L.load().mofa_igemm_plan(ctypes.byref(a), n_cu, ctypes.byref(p)) == 0
    return p


def row_map(a):
    """the exported row map of every tile row of the launch: list of output rows / -1"""
    fn, ref, p = L.load().mofa_igemm_up2f_row, ctypes.byref(a), plan(a, 256)
    assert p.rc == 0
    return [fn(ref, r) for r in range(256 * p.tiles_m)]


def launch_model(xt, wf, b, nimg, H, Wd, rows, mutant=None):
    """torch-CPU model of the launch (fp64): xt tokens [nimg H W, Cinpad], wf [4N, 4 Cinpad], rows = row_map(args).  Row tile t
    holds source pixels 256 (t >> 2) .. + 255 of phase t & 3 = 2 a + b; its weight rows start at (t & 3) * N; tap t = 2 ty + tx
    reads pixel (y - (1 - a) + ty, x - (1 - b) + tx) or zero; rows the map answers -1 for are not stored.  Returns [M, N]
    (NaN where nothing was stored)."""
    N, Cp = wf.shape[0] // 4, wf.shape[1] // 4
    Mq, M = nimg * H * Wd, 4 * nimg * H * Wd
    out = torch.full((M, N), float("nan"), dtype=torch.float64)
    xt, wf = xt.double(), wf.double()
    i = torch.arange(256)
    for t in range(len(rows) // 256):
        ph = t & 3
        a, bb = (ph & 1, ph >> 1) if mutant == "phase_2b_a" else (ph >> 1, ph & 1)
        q = (t >> 2) * 256 + i
        valid = q < Mq
        qc = torch.where(valid, q, torch.zeros_like(q))
        img, rem = qc // (H * Wd), qc % (H * Wd)
        y, x = rem // Wd, rem % Wd
        wt = wf[0:N] if mutant == "wbase_fixed" else wf[ph * N:(ph + 1) * N]
        oy_org, ox_org = (1, 1) if mutant == "origin_no_phase" else ((a, bb) if mutant == "taps_swapped" else (1 - a, 1 - bb))
        acc = torch.zeros(256, N, dtype=torch.float64)
        for ty in range(2):
            for tx in range(2):
                sy, sx = y - oy_org + ty, x - ox_org + tx
                ok = valid & (sy >= 0) & (sy < H) & (sx >= 0) & (sx < Wd)
                src = torch.where(ok, (img * H + sy) * Wd + sx, torch.zeros_like(q))
                xs = xt[src] * ok[:, None].double()
                tap = 2 * tx + ty if mutant == "tytx_swapped" else 2 * ty + tx
                acc += xs @ wt[:, tap * Cp:(tap + 1) * Cp].T
        if b is not None:
            acc += b.double()[None, :]
        dst = torch.tensor(rows[256 * t:256 * t + 256])
        if mutant == "padding_stored":                         # the row map without its padding check (decoded past the last image)
            dst = ((q // (H * Wd) * 2 * H + 2 * (q % (H * Wd) // Wd) + (ph >> 1)) * 2 * Wd + 2 * (q % Wd) + (ph & 1)) % M
        keep = dst >= 0
        out[dst[keep]] = acc[keep]
    return out
