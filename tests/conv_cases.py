"""TEST INFRASTRUCTURE ONLY: the convolution-geometry case tables of the implicit GEMM (csrc/igemm*.hip), their fp64 reference,
the preconditions of the exact family and the "wrong convolution" mutants that prove the checks can fail.

Built on tests/op_cases.py: a case is an ``op_cases.Case`` whose ``build()`` gives the keyword arguments of ``igemm`` with every
``x``, ``out`` and ``r1`` a guarded view (NaN guard rows before and after, 8 NaN guard columns on the left, a leading dimension
larger than the width and different for every argument of a call), so ``op_cases.run`` takes the identical case through
tests/emu_ops.py on the CPU (tests/test_conv_cases_cpu.py) and through ``mofa_video_amd.ops`` on the GPU
(tests/test_igemm_conv_edges_gpu.py).

The expectation is an fp64 sum PER TAP, straight from the definition in include/mofa_hip.h (``acc64``; no F.conv2d: the stand-in
uses that, and the CPU file compares the two): tap origin org = ksize // 2 (PAD_SAME) or 0 (PAD_TRAILING); virtual pixel
v = o * stride + (k - org) * dil; in the image iff 0 <= v < Hin * up; source pixel v // up.

Two input families:

  E "exact"  x = integers in [-3, 3], w = integers in [-2, 2] / 16, bias = integers in [-64, 64] / 16, r1 = integers in
             [-64, 64] / 16.  Every partial sum is a multiple of 1/16 of magnitude at most taps * Cin * 6 + 128 units
             (49 taps x 128 channels: 37 760) < 2^24 in ANY order, so the fp32 accumulator is exact whatever the summation order
             (tile, K split, MFMA tree), and -- asserted per case in the builder -- every expected value and every intermediate the
             epilogue rounds is exactly representable in fp16, so no rounding mode can matter: the output must be EQUAL to the
             fp64 reference.  One misplaced, dropped or doubled tap anywhere changes it.
  A "gauss"  x, r1 ~ N(0, 1), w ~ N(0, 1 / K), bias ~ N(0, 1): the project's stated GEMM class (op_cases.TOL["gemm"]); carries the
             split-K "really ran" proof (a different fp32 summation order shows) and rounding realism.

Three epilogues: ``bias``, ``relu`` (bias + ReLU, the CMP encoder's form) and ``r1`` (bias, then the residual with s1 = 1:
round16(round16(acc + bias) + r1), the formula of test_igemm_tiles_gpu.py::test_all_tiles_round_residual_adds_alike)."""
import ctypes
import functools
import os
import sys
import types

import torch

import op_cases as oc
from op_cases import F16, NAN, TOL, Case, close_errors, guard, run  # noqa: F401  (re-exported for the two test files)
from mofa_video_amd import lib as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import igemm_plan_table as plan_table  # noqa: E402  (the rows of tests/igemm_plan_table.json and their mofa_igemm_args)

EPIS = ("bias", "relu", "r1")
FAMILIES = ("E", "A")
TILES = {"128x128": L.TILE_128X128, "192x128": L.TILE_192X128, "256x256": L.TILE_256X256, "256x320": L.TILE_256X320}
PIPE = ("256x256", "256x320")                     # the 8-wave kernels: 10-bit oy / ox, at most 2047 images, N % 8 == 0
TILE_M = {"128x128": 128, "192x128": 192, "256x256": 256, "256x320": 256}
TILE_N = {"128x128": 128, "192x128": 128, "256x256": 256, "256x320": 320}
PIPE_HW_MAX, PIPE_IMG_MAX, WAVE4_HW_MAX = 1024, 2047, 65535
E_UNITS_MAX = 2 ** 24                             # units of 1/16: the fp32 accumulator holds every such integer exactly


class Spec:
    """one problem of the implicit GEMM: ``mode`` conv / convt / plain, its geometry and sizes.  conv: n images of H x W,
    M = n * Hout * Wout; convt: clips x T frames of HW rows (T = 0: the unclipped halo form, M = frames * HW and one real halo
    frame in front of and behind the view); plain: M x K"""

    def __init__(self, id, mode, Cin=64, N=72, **kw):
        self.id, self.mode, self.Cin, self.N = id, mode, Cin, N
        self.__dict__.update(kw)

    def __repr__(self):
        return self.id

    @property
    def taps(self):
        return {"conv": getattr(self, "k", 0) ** 2, "convt": 3, "plain": 1}[self.mode]

    @property
    def geom(self):
        from mofa_video_amd import ops
        if self.mode == "conv":
            return ops.conv3x3_geom(self.H, self.W, stride=self.stride, up=self.up, ksize=self.k, dil=self.dil, pad=self.pad)
        return ops.convt3_geom(self.T, self.HW) if self.mode == "convt" else ops.PLAIN

    @property
    def rows_in(self):                            # rows of x the builder draws (the halo form: two frames more than the view)
        if self.mode == "conv":
            return self.n * self.H * self.W
        return self.M + (2 * self.HW if self.mode == "convt" and self.T == 0 else 0)

    def where(self, m):
        if self.mode == "conv":
            g = self.geom
            return f"image {m // (g.Hout * g.Wout)} oy {m // g.Wout % g.Hout} ox {m % g.Wout}"
        if self.mode == "convt":
            fr = m // self.HW
            return f"frame {fr}" + (f" (clip {fr // self.T} position {fr % self.T})" if self.T else "") + f" pixel {m % self.HW}"
        return f"row {m}"


def conv(id, H, W, k=3, dil=1, stride=1, up=1, pad=L.PAD_SAME, Cin=64, N=72, n=None, M=None):
    """``n`` None: the smallest image count with M >= 257 and M % 256 != 0 -- the last row of every tile height is ragged and
    tiles straddle images; ``M``: what the table says, asserted"""
    s = Spec(id, "conv", Cin, N, H=H, W=W, k=k, dil=dil, stride=stride, up=up, pad=pad)
    g = s.geom
    hw = g.Hout * g.Wout
    if n is None:
        n = next(i for i in range(-(-257 // hw), 1 << 20) if (i * hw) % 256)
    s.n, s.M = n, n * hw
    assert M is None or s.M == M, (id, s.M, M)
    return s


_T = L.PAD_TRAILING
CONV_ROWS = [
    conv("k1s2", 11, 13, k=1, stride=2, M=294),
    conv("k3", 11, 13, Cin=128, N=328, M=286),
    conv("k3s2-odd", 11, 13, stride=2, M=294),
    conv("k3s2-even", 10, 14, stride=2, Cin=128, M=280),
    conv("k3up2", 5, 7, up=2, M=280),
    conv("k3up2s2", 5, 7, up=2, stride=2, M=280),
    conv("k3s2-trail-even", 10, 14, stride=2, pad=_T, M=280),
    conv("k3s2-trail-odd", 11, 13, stride=2, pad=_T, Cin=128, M=270),
    conv("k3-trail", 11, 13, pad=_T, M=360),
    conv("k3up2-trail-s2", 5, 7, up=2, stride=2, pad=_T, M=280),
    conv("k3d2", 11, 13, dil=2, Cin=128, M=286),
    conv("k3d4", 11, 13, dil=4, M=286),
    conv("k3d4-H3", 3, 13, dil=4, M=273),                    # every off-centre row tap outside the image
    conv("k3d2s2", 11, 13, dil=2, stride=2, M=294),
    conv("k5", 11, 13, k=5, Cin=128, M=286),
    conv("k5s2", 11, 13, k=5, stride=2, M=294),
    conv("k5d2", 11, 13, k=5, dil=2, M=286),
    conv("k5-trail-s2", 11, 13, k=5, stride=2, pad=_T, M=270),
    conv("k7", 11, 13, k=7, Cin=128, M=286),
    conv("k7s2", 10, 14, k=7, stride=2, M=280),
    conv("k7-H1", 1, 17, k=7, M=272),
    conv("k3-W1", 17, 1, M=272),
    conv("k5-1x1img", 1, 1, k=5, n=300, M=300),              # a tile spans 256 images, only the centre tap lives
    # the size bounds of the packed row geometry
    conv("k3-W1024", 1, 1024, n=1, M=1024),                  # last value of the 8-wave kernels' 10-bit ox field
    conv("k3-H1024", 1024, 1, n=1, M=1024),                  # ... of the 10-bit oy field
    conv("k3-2047img", 2, 2, n=2047, M=8188),                # last image count of img << 20
    conv("k3-H40000", 40000, 1, N=8, n=1, M=40000),          # 4-wave (oy << 16) | ox: oy needs bit 31 of the word
]
CONV_BY_ID = {s.id: s for s in CONV_ROWS}
WAVE4_ONLY = ("k3-H40000",)                                  # Hout > 1024: the 8-wave tiles refuse, the default falls back

# split-K on the 256x320 tile with a K slice that starts inside a tap of a k != 3 / dilated conv: two remainder tiles (M in
# 257 ... 512, N = 320) cut into SPLIT_SLICES[id] slices for any CU count >= 16 (assert_table asks mofa_igemm_plan)
SPLIT_ROWS = [
    conv("split-k5-c128", 11, 13, k=5, Cin=128, N=320, M=286),
    conv("split-k5d2-c128", 11, 13, k=5, dil=2, Cin=128, N=320, M=286),
    conv("split-k7s2-c64", 10, 14, k=7, stride=2, Cin=64, N=320, M=280),         # one K tile per tap
    conv("split-k7-c128", 11, 13, k=7, Cin=128, N=320, M=286),
    conv("split-k3d2-c256", 11, 13, dil=2, Cin=256, N=320, M=286),
]
SPLIT_SLICES = {"split-k5-c128": 6, "split-k5d2-c128": 6, "split-k7s2-c64": 6, "split-k7-c128": 8, "split-k3d2-c256": 4}

# packing edges one past the last value: the forced 8-wave tiles refuse, the default launcher takes a 4-wave tile
PIPE_OVER_ROWS = [conv("k3-W1025", 1, 1025, n=1, M=1025), conv("k3-2048img", 2, 2, n=2048, M=8192)]
WAVE4_OVER_ROW = conv("k3-H65536", 65536, 1, N=8, n=1, M=65536)      # Hout > 65535: every launcher refuses


def convt(T, HW, clips, Cin=64, N=72):
    """T > 0: ``clips`` clips of T frames; T == 0: the unclipped halo form with ``clips`` frames in the view"""
    frames = clips * (T or 1)
    return Spec(f"convT3-T{T}-HW{HW}-x{clips}", "convt", Cin, N, T=T, HW=HW, clips=clips, M=frames * HW)


def _convt_rows():
    """T x HW with at least two clips (the clip boundary exists) and at least 257 rows, never a multiple of 256; Cin 64 / 128
    alternate; the halo form; two clips whose boundary (row 160) lies inside tile 0 or 1 of every tile height"""
    rows = []
    for i, T in enumerate((1, 2, 3)):
        for j, HW in enumerate((1, 33, 300)):
            clips = max(2, -(-257 // (T * HW)))
            while (clips * T * HW) % 256 == 0:
                clips += 1
            rows.append(convt(T, HW, clips, Cin=(64, 128)[(i + j) % 2]))
    rows.append(convt(0, 33, 3))
    rows.append(convt(0, 100, 3, Cin=128))
    rows.append(convt(4, 40, 2))
    rows.append(convt(5, 77, 2, Cin=128))                    # boundary at row 385: inside tile 3 / 2 / 1
    return rows


CONVT_ROWS = _convt_rows()
PLAIN_K, PLAIN_M, PLAIN_N = (64, 128, 192), (1, 255, 256, 257, 513), (8, 72, 256, 264, 320, 328)


@functools.lru_cache(maxsize=None)
def plain(K, M, N):
    return Spec(f"plain-K{K}-M{M}-N{N}", "plain", K, N, M=M)


def plain_rows(K):
    return [plain(K, M, N) for M in PLAIN_M for N in PLAIN_N]


def plain_epi(s):
    """the epilogue of a plain-table case: cycled, so that every (M, N) meets each of the three over the three K"""
    return EPIS[(PLAIN_K.index(s.Cin) + PLAIN_M.index(s.M) + PLAIN_N.index(s.N)) % 3]


def plan(s, epi="bias", tile=None, n_cu=256, split_k=True):
    """mofa_igemm_plan (csrc/igemm_plan.h, no device call) for the launch ``case(s, "E", epi, tile, split_k)`` makes: the case's
    leading dimensions, fake 16-byte aligned addresses (the guarded views are aligned alike) -> lib.IgemmPlan"""
    mode = {"plain": L.MODE_PLAIN, "conv": L.MODE_CONV3X3, "convt": L.MODE_CONVT3}[s.mode]
    a = plan_table.make_args(s.M, s.N, s.Cin, 1 if "r1" in epi else 0, mode, None if s.mode == "plain" else s.geom,
                             L.ACT_RELU if "relu" in epi else None, split_k is not False, False, TILES[tile] if tile else L.TILE_AUTO,
                             ldx=s.Cin + 24, ldo=(s.N + 39) // 8 * 8, ldr=(s.N + 55) // 8 * 8)
    p = L.IgemmPlan()
    assert L.load().mofa_igemm_plan(ctypes.byref(a), n_cu, ctypes.byref(p)) == 0
    return p


def assert_table():
    """the tables hold what they are there for: every kernel size and dilation, both strides, both ``up``, both pads, one and
    two K tiles per tap, more than one column tile for each tile width, each packing edge (and the shapes beyond them)"""
    R = CONV_ROWS
    assert len(R) == 27 and len({s.id for s in R}) == 27
    assert {s.k for s in R} == {1, 3, 5, 7} and {s.dil for s in R} == {1, 2, 4}
    assert {s.stride for s in R} == {1, 2} and {s.up for s in R} == {1, 2} and {s.pad for s in R} == {L.PAD_SAME, L.PAD_TRAILING}
    for k in (3, 5, 7):                                     # every kernel size with both strides; 3 and 5 dilated and trailing
        assert {s.stride for s in R if s.k == k} == {1, 2}, k
    assert {s.k for s in R if s.dil > 1} == {3, 5} and {s.k for s in R if s.pad == _T} == {3, 5}
    assert any(s.up == 2 and s.stride == 2 and s.pad == _T for s in R)
    assert {s.Cin // 64 for s in R} == {1, 2}               # kpt = K tiles per tap
    for k in (3, 5, 7):
        assert {s.Cin // 64 for s in R if s.k == k} == {1, 2}, k
    for name, tn in TILE_N.items():
        assert any(s.N > tn for s in R), name
    for s in R[:-4]:                                        # ragged last tile of every height, more than one row tile
        assert s.M >= 257 and s.M % 256 and s.M % 192 and s.M % 128, s.id
    assert any(s.geom.Hout == 1 for s in R) and any(s.geom.Wout == 1 for s in R) and any(s.H * s.W == 1 for s in R)
    assert any(s.H < s.dil * (s.k // 2) + 1 for s in R)     # a dilated tap row that never meets the image
    g = {s.id: s.geom for s in R}
    assert g["k3-W1024"].Wout == PIPE_HW_MAX and g["k3-H1024"].Hout == PIPE_HW_MAX and CONV_BY_ID["k3-2047img"].n == PIPE_IMG_MAX
    assert 32768 <= g["k3-H40000"].Hout <= WAVE4_HW_MAX     # (oy << 16) sets bit 31
    assert [s.geom.Wout for s in PIPE_OVER_ROWS[:1]] == [PIPE_HW_MAX + 1] and PIPE_OVER_ROWS[1].n == PIPE_IMG_MAX + 1
    assert WAVE4_OVER_ROW.geom.Hout == WAVE4_HW_MAX + 1
    T = CONVT_ROWS
    assert {s.T for s in T} >= {0, 1, 2, 3} and {s.HW for s in T} >= {1, 33, 300} and {s.Cin for s in T} == {64, 128}
    assert all(s.clips >= 2 for s in T if s.T) and all(s.M >= 257 or s.T == 0 for s in T)
    for th in set(TILE_M.values()):                         # a clip boundary strictly inside a tile, for every tile height
        assert any(s.T and (s.T * s.HW) % th for s in T), th
    assert len(PLAIN_K) * len(PLAIN_M) * len(PLAIN_N) == 90 and {K // 64 for K in PLAIN_K} == {1, 2, 3}
    assert all(n % 8 == 0 for n in PLAIN_N)                 # (the refused N % 8 != 0 has a test of its own)
    for s in SPLIT_ROWS:
        nk = s.taps * s.Cin // 64
        assert 256 < s.M <= 512 and s.N <= 320 and (s.k != 3 or s.dil != 1), s.id
        for n_cu in (16, 64, 256, 304):
            p = plan(s, tile="256x320", n_cu=n_cu)
            assert (p.rc, p.tile, p.rem_tiles, p.split) == (0, L.TILE_256X320, 2, SPLIT_SLICES[s.id]), (s.id, n_cu, p.split)
        assert any((i * nk // SPLIT_SLICES[s.id]) % (s.Cin // 64) for i in range(1, SPLIT_SLICES[s.id])) or s.Cin == 64, s.id
        # ^ a slice starts in the middle of a tap wherever a tap has more than one K tile


# ---------------------------------------------------------------------------------------------------------------------------
# the fp64 reference, per tap from the definition; ``defect`` makes it one of the mutants
# ---------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("origin", "no-dil", "swap-kykx", "col-overrun", "up-round-up", "clip-late", "drop-ktile")


def _axis(n_out, size, up, stride, dil, org, k, defect):
    """-> (virtual pixel, in-image mask, source pixel) of tap k for the n_out outputs of one axis"""
    v = torch.arange(n_out) * stride + (k - org) * dil
    ok = (v >= 0) & (v < size * up)
    src = (v + 1) // 2 if (up == 2 and defect == "up-round-up") else v // up
    return v, ok, src


def acc64(s, x, w, defect=None):
    """sum over taps and channels in fp64 -> [M, N].  ``x``: the rows_in rows the builder drew (the halo form: with its halo)"""
    Cin, N = s.Cin, s.N
    X, Wd = x[:, :Cin].double(), w.double()
    if defect == "drop-ktile":                               # the first K tile of the tap at offset 0 (in the image for every
        o = 0 if s.mode != "conv" or s.pad == L.PAD_TRAILING else s.k // 2       # output pixel) never arrives
        t0 = {"plain": 0, "convt": 1, "conv": o * getattr(s, "k", 0) + o}[s.mode] * Cin
        Wd = Wd.clone()
        Wd[:, t0:t0 + 64] = 0.0
    if s.mode == "plain":
        return X[:s.M] @ Wd.T
    if s.mode == "convt":
        Wt, HW, T, M = Wd.reshape(N, 3, Cin), s.HW, s.T, s.M
        m = torch.arange(M)
        if T == 0:
            return sum(X[m + t * HW] @ Wt[:, t].T for t in range(3))
        pos = m // HW % T
        acc = X[:M] @ Wt[:, 1].T
        acc += (X[(m - HW).clamp(min=0)] * (pos > 0)[:, None]) @ Wt[:, 0].T
        src = m + HW                                         # clip-late: the boundary test one frame late (pos < T, always true)
        live = (src < M) if defect == "clip-late" else (pos < T - 1)
        acc += (X[src.clamp(max=M - 1)] * live[:, None]) @ Wt[:, 2].T
        return acc
    g, k, n = s.geom, s.k, s.n
    org = (0 if s.pad == L.PAD_TRAILING else k // 2) + (1 if defect == "origin" else 0)
    dil = 1 if defect == "no-dil" else s.dil
    Wt = Wd.reshape(N, k, k, Cin)
    if defect == "swap-kykx":
        Wt = Wt.transpose(1, 2)
    rows = n * s.H * s.W
    img = torch.arange(n)[:, None, None]
    acc = torch.zeros(s.M, N, dtype=torch.float64)
    for ky in range(k):
        _, oky, iy = _axis(g.Hout, s.H, s.up, s.stride, dil, org, ky, defect)
        if not oky.any():
            continue
        for kx in range(k):
            vx, okx, ix = _axis(g.Wout, s.W, s.up, s.stride, dil, org, kx, defect)
            iyc = iy.clamp(0, s.H - 1)
            if defect == "col-overrun":                      # vx < Win * up is never tested: the flat index runs into the next row
                okx = vx >= 0
                flat = (img * s.H + iyc[None, :, None]) * s.W + ix.clamp(min=0)[None, None, :]
            else:
                flat = (img * s.H + iyc[None, :, None]) * s.W + ix.clamp(0, s.W - 1)[None, None, :]
            ok = (oky[:, None] & okx[None, :])[None] & (flat < rows)
            if not ok.any():
                continue
            src = X[flat.clamp(max=rows - 1).reshape(-1)] * ok.reshape(-1, 1)
            acc += src @ Wt[:, ky, kx].T
    return acc


def mutant_differs(defect, s):
    """does the defect change the arithmetic of this case?  Stated from the geometry alone; where it does not the mutant is
    asserted EQUAL to the truth, where it does family E must fail (tests/test_conv_cases_cpu.py, which also checks this rule
    against the two fp64 accumulators)"""
    if defect == "drop-ktile":
        return True                                          # every case: plain, conv, convT3
    if defect == "clip-late":                                # the last frame of every clip but the last reads the next clip
        return s.mode == "convt" and s.T > 0 and s.clips > 1
    if s.mode != "conv":
        return False
    g = s.geom
    Hv, Wv = s.H * s.up, s.W * s.up
    if defect == "origin":                                   # every tap moves, the 1 x 1 kernel's too
        return True
    if defect == "no-dil":
        return s.dil > 1 and s.k > 1
    if defect == "swap-kykx":                                # some off-centre tap meets the image (else only w[c, c] is used)
        return s.k > 1 and (s.dil < Hv or s.dil < Wv)
    if defect == "up-round-up":
        return s.up == 2
    if defect == "col-overrun":                              # the last tap passes the last column, and the element the flat
        org = 0 if s.pad == L.PAD_TRAILING else s.k // 2     # index then reaches lies inside the buffer (not for one single row)
        return (g.Wout - 1) * s.stride + (s.k - 1 - org) * s.dil >= Wv and (s.n > 1 or s.H > 1)
    raise KeyError(defect)


# ---------------------------------------------------------------------------------------------------------------------------
# operands, expectation, cases
# ---------------------------------------------------------------------------------------------------------------------------
def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=512)
def _data(s, family, seed=11):
    g = torch.Generator().manual_seed(seed + sum(map(ord, s.id)))
    K = s.taps * s.Cin
    if family == "E":
        x, w = _ints(g, -3, 3, s.rows_in, s.Cin).half(), (_ints(g, -2, 2, s.N, K) / 16).half()
        bias, r1 = _ints(g, -64, 64, s.N) / 16, (_ints(g, -64, 64, s.M, s.N) / 16).half()
        units = K * 3 * 2 + 64 + 64                          # |x| <= 3, |16 w| <= 2 per product; bias and r1 <= 64 units each
        assert units < E_UNITS_MAX and x.abs().max() <= 3 and (w * 16).abs().max() <= 2, (s.id, units)
    else:
        x = torch.randn(s.rows_in, s.Cin, generator=g).half()
        w = (torch.randn(s.N, K, generator=g) * K ** -0.5).half()
        bias, r1 = torch.randn(s.N, generator=g), torch.randn(s.M, s.N, generator=g).half()
        units = None
    return types.SimpleNamespace(x=x, w=w, bias=bias, r1=r1, acc=acc64(s, x, w), units=units)


def _f16_exact(t):
    return bool((t.half().double() == t).all())


@functools.lru_cache(maxsize=1024)
def expect(s, family, epi):
    """fp64 [M, N].  Family E: the accumulator's bound, and every value the epilogue rounds is representable in fp16"""
    d = _data(s, family)
    y = d.acc + d.bias.double()
    if family == "E":
        assert (d.acc * 16).abs().max() <= d.units - 128 and bool(((d.acc * 16) == (d.acc * 16).round()).all()), s.id
        assert _f16_exact(y), (s.id, "acc + bias not representable in fp16", y.abs().max().item())
    if "r1" in epi:
        y = y.half().double() + d.r1.double()                # round16(acc + bias), then the residual (s1 = 1)
        assert family != "E" or _f16_exact(y), (s.id, "round16(acc + bias) + r1 not representable in fp16")
    if "relu" in epi:                                        # (the activation comes last: "r1-relu", outside EPIS, is the kind
        y = y.clamp(min=0.0)                                 # the 8-wave tiles refuse)
    return y


def case(s, family="E", epi="bias", tile=None, split_k=None):
    def build():
        d = _data(s, family)
        halo = s.mode == "convt" and s.T == 0
        kw = dict(x=guard(d.x, ld=s.Cin + 24, trim=(s.HW, s.HW) if halo else (0, 0)), w=d.w, bias=d.bias,
                  out=guard(shape=(s.M, s.N), ld=(s.N + 39) // 8 * 8))
        if s.mode != "plain":
            kw["geom"] = s.geom
        if halo:
            kw["M"] = s.M
        if "relu" in epi:
            kw["act"] = L.ACT_RELU
        if "r1" in epi:
            kw.update(r1=guard(d.r1, ld=(s.N + 55) // 8 * 8), s1=1.0)
        if tile is not None:
            kw["tile"] = TILES[tile]
        if split_k is not None:
            kw["split_k"] = split_k
        return kw
    c = Case(f"{s.id}/{family}-{epi}" + (f"-{tile}" if tile else "") + ("" if split_k is None else f"-split{int(split_k)}"),
             "igemm", build, "exact" if family == "E" else "gemm")
    c.spec, c.family, c.epi = s, family, epi
    return c


def release():
    """drop the cached operands and references; the two test files call it when their last test is done"""
    _data.cache_clear()
    expect.cache_clear()


# ---------------------------------------------------------------------------------------------------------------------------
# the checks, the same for the stand-in, the kernels and the mutants
# ---------------------------------------------------------------------------------------------------------------------------
def check_output(c, out):
    """-> (worst err / bound; inf for a failed equality, [messages])"""
    s, ref = c.spec, expect(c.spec, c.family, c.epi)
    out = out.detach().cpu()
    if tuple(out.shape) != tuple(ref.shape):
        return float("inf"), [f"{c.id}: shape {tuple(out.shape)} != {tuple(ref.shape)}"]
    if c.tol == "exact":
        bad = ~(out.double() == ref)                         # by value (-0 == 0); a NaN is unequal to everything
        if bad.any():
            r, col = torch.nonzero(bad)[0].tolist()
            rows = bad.any(1)
            return float("inf"), [f"{c.id}: {int(bad.sum())} / {bad.numel()} elements in {int(rows.sum())} rows differ from the fp64 "
                                  f"reference, first at [{r}, {col}] = {s.where(r)}, last row {int(torch.nonzero(rows)[-1])}: got "
                                  f"{out[r, col].item()!r}, expected {ref[r, col].item()!r}"]
        return 0.0, []
    worst, msg = close_errors(out, ref, TOL[c.tol], c.id)
    return worst, ([] if msg is None else [msg])


def check_run(c, r, fresh=False):
    """guards intact and read-only arguments unchanged; the result is the ``out`` buffer (``fresh``: a tensor of its own);
    then the family's comparison"""
    errs = list(r.guard_errors())
    if fresh:
        got = r.ret
        if any(got is p.t for p in r.placed.values()):
            errs.append(f"{c.id}: the call without out= returns one of its arguments")
    else:
        got = r.placed["out"].t
        if r.ret is not got:
            errs.append(f"{c.id}: the call does not return its out buffer")
    worst, e = check_output(c, got)
    return worst, errs + e


# ---------------------------------------------------------------------------------------------------------------------------
# mutants: the fp64 reference with one defect each, in the signature of the op, so they go through op_cases.run like the real
# thing (``defect`` None: the plain truth)
# ---------------------------------------------------------------------------------------------------------------------------
def wrong_igemm(s, defect):
    def igemm(x, w, bias=None, geom=None, M=None, r1=None, s1=1.0, act=L.ACT_NONE, out=None, tile=None, split_k=True):
        if s.mode == "convt" and s.T == 0:                   # the halo frames are real rows in front of and behind the view
            x = torch.as_strided(x, (s.M + 2 * s.HW, x.shape[1]), (x.stride(0), 1), x.storage_offset() - s.HW * x.stride(0))
        y = acc64(s, x, w, defect) + bias.double()
        if r1 is not None:
            y = y.half().double() + s1 * r1.double()
        if act == L.ACT_RELU:
            y = y.clamp(min=0.0)
        out[:, :s.N] = y.half()
        return out
    return types.SimpleNamespace(igemm=igemm)
