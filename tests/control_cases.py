"""TEST INFRASTRUCTURE ONLY: the case table of the control-signal kernels (csrc/control.hip), shared by
tests/test_control_device_cpu.py (the shared header run on the host by tests/control_points_main.hip) and
tests/test_control_device_gpu.py (``ops.sparse_points`` / ``ops.flow_finish``).  Every expectation comes from the host
functions the device path replaces and is compared by equality:
  ADD     ``control.get_sparseflow_and_mask_forward`` re-laid as fp32 [n,4,H,W];
  LAST    ``control.get_sparse_flow`` on the CPU, cast to fp32;
  finish  the torch composition of ``cmp.get_cmp_flow``'s brush multiply, ``cmp.get_flow``'s nearest resize and scalings
          (``F.interpolate(mode='nearest')`` has the index rule of ``ops.resize_nearest_f32``) and ``merge_inmask_outmask``.
Device buffers are views into NaN-filled guard buffers (``Guarded``), checked intact after the call."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from mofa_video_amd import control

ADD, LAST = 0, 1
NAN = float("nan")
EXACT = 1 << 24


# ---- ADD ------------------------------------------------------------------------------------------------------------------
def _add_points(scenario, H, W, n, seed):
    """(pos int32 [K,2] (row, col), disp int64 [K,n,2] (dx, dy))"""
    rng = np.random.RandomState(seed)
    if scenario == "k0":
        pos = np.zeros((0, 2))
    elif scenario == "k1":
        pos = np.array([[H // 2, W - 3]])
    elif scenario == "corners":
        pos = np.array([[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1]])
    elif scenario == "shared":
        # two adjacent tracks on pixel p, three non-adjacent ones on pixel q, others in between
        p, q = [1, W - 2], [H - 2, 3]
        pos = np.array([[3, 4], p, p, q, [0, 5], q, [5, 0], [H - 1, W - 1], q])
    elif scenario == "k130":
        # more than a wave, more than 64 points per frame, drawn from 40 pixels: many shared ones
        pix = np.stack([rng.randint(0, H, 40), rng.randint(0, W, 40)], axis=1)
        pos = pix[rng.randint(0, 40, 130)]
    elif scenario == "negzero":
        pos = np.array([[2, 3], [2, 3], [4, 1], [H - 1, 2]])
    else:
        raise KeyError(scenario)
    K = pos.shape[0]
    disp = rng.randint(-300, 301, (K, n, 2))
    if scenario == "negzero" and K:
        disp[0] = -np.abs(disp[0]) - 1
        disp[1, :, 0] = 0                                    # dx = 0 on a shared pixel
        disp[2] = 0                                          # a track that does not move: flow 0, mask 1
        disp[3] = -disp[3]
    return pos.astype(np.int32).reshape(K, 2), disp.astype(np.int64)


ADD_CASES = {}
for _H, _W, _n in ((8, 8, 1), (32, 48, 3)):
    for _s in ("k0", "k1", "corners", "shared", "k130", "negzero"):
        ADD_CASES[f"{_s}-{_H}x{_W}-n{_n}"] = (_s, _H, _W, _n)
for _s in ("k0", "corners", "k130"):
    ADD_CASES[f"{_s}-384x384-n24"] = (_s, 384, 384, 24)


def add_case(name):
    """-> pos int32 [K,2], val fp32 [n,K,2], H, W, expectation fp32 [n,4,H,W], largest |sum| of the case"""
    scenario, H, W, n = ADD_CASES[name]
    pos, disp = _add_points(scenario, H, W, n, seed=len(name))
    K = pos.shape[0]
    start_xy = pos[:, ::-1].astype(np.float64)
    tracks = np.concatenate([start_xy[:, None], start_xy[:, None] + disp], axis=1)             # [K, n+1, 2] (x, y)
    flow, mask = control.get_sparseflow_and_mask_forward(tracks, n, H, W) if K else (np.zeros((n, H, W, 2)), np.zeros((n, H, W)))
    want = np.concatenate([flow.transpose(0, 3, 1, 2), mask[:, None], mask[:, None]], axis=1)
    val = torch.from_numpy(np.ascontiguousarray(disp.transpose(1, 0, 2)).astype(np.float32)).reshape(n, K, 2)
    return torch.from_numpy(pos), val, H, W, torch.from_numpy(want.astype(np.float32)), float(np.abs(flow).max())


# ---- LAST -----------------------------------------------------------------------------------------------------------------
LAST_CASES = {"8x8-n1": (8, 8, 1), "40x56-n4": (40, 56, 4), "40x56-n96": (40, 56, 96), "384x384-n1": (384, 384, 1),
              "384x384-n96": (384, 384, 96)}
LAST_DUP = (5, 20, 41)        # landmarks on one pixel; 41 wins, and it is not the last point of the array
LAST_NAN = 30                 # a landmark whose displacement is NaN in frame 1 (x) and in the last frame (y)


@contextlib.contextmanager
def one_thread():
    """``sample_optical_flow`` writes with ``index_put_``, which keeps "later points overwrite earlier ones" on the CPU only while
    it runs serially: with several threads torch splits the index list into chunks and, where two points of one pixel fall
    into different chunks (seen at 96 frames: frames 19, 38, 57 took an earlier point), either may win.  The expectation is
    therefore computed on one thread, where the last point wins as the docstring promises."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def last_landmarks(H, W, n, dtype=torch.float32):
    """[1, n+1, 68, 2] (x, y): fractional coordinates over the canvas and a little beyond it, with the planted edge points"""
    g = torch.Generator().manual_seed(H * 1000 + W + n)
    lm = torch.rand(1, n + 1, 68, 2, generator=g) * torch.tensor([W + 4.0, H + 4.0]) - 2.0
    f0 = lm[0, 0]
    f0[0] = torch.tensor([-0.5, -0.5])                       # .long() truncates toward zero: pixel (0, 0)
    f0[1] = torch.tensor([-1.5, 2.25])                       # -1 -> clipped to column 0
    f0[2] = torch.tensor([3.75, -1.5])                       # -1 -> clipped to row 0
    f0[3] = torch.tensor([W + 5.0, H + 9.0])                 # beyond both far borders: all three clip onto (H-1, W-1)
    f0[4] = torch.tensor([W + 0.5, H - 0.5])
    f0[50] = torch.tensor([W - 0.25, H + 100.0])
    for k in LAST_DUP:
        f0[k] = torch.tensor([W / 2 + 0.3, H / 2 + 0.6]) + 0.1 * LAST_DUP.index(k)
    f0[LAST_NAN] = torch.tensor([1.5, H - 1.5])
    f0[67] = torch.tensor([W - 2.5, 1.5])
    lm[0, 1, LAST_NAN, 0] = NAN
    lm[0, n, LAST_NAN, 1] = NAN
    return lm.to(dtype)


def last_case(name, dtype=torch.float32):
    """-> pos int32 [68,2], val fp32 [n,68,2], H, W, expectation fp32 [n,4,H,W]"""
    H, W, n = LAST_CASES[name]
    lm = last_landmarks(H, W, n, dtype)
    with one_thread():
        flow, mask = control.get_sparse_flow(lm, H, W, n + 1)
    want = torch.cat([flow[0].float(), mask[0].float()], dim=1).contiguous()
    pos, val = control.landmark_points(lm)
    return pos, val, H, W, want


# ---- finish ---------------------------------------------------------------------------------------------------------------
# name: (hs, ws, H, W, n, flow_in?, flow_out?, brush: None | "255" | "values", offset of the views into their guard buffers)
FINISH_CASES = {
    "equal_size": (8, 8, 8, 8, 2, True, True, "values", 4),
    "equal_size_no_brush": (8, 8, 8, 8, 2, True, True, None, 4),
    "equal_size_unaligned": (8, 8, 8, 8, 2, True, True, "values", 1),      # pointers off 16 bytes: the scalar paths
    "equal_size_odd_width": (6, 7, 6, 7, 2, True, True, "values", 4),
    "upscale": (8, 8, 12, 20, 2, True, True, None, 4),
    "mixed": (16, 16, 8, 24, 2, True, True, "255", 4),
    "ratio_384": (24, 24, 36, 64, 3, True, True, "values", 4),             # 384 -> 576 x 1024; more than one workgroup
    "fp32_product": (7, 5, 23, 13, 2, True, True, "values", 4),
    "fp32_product_differs": (14, 26, 46, 22, 2, True, True, None, 4),      # floorf(o * scale) != floor(o * in / out) at o = 23 / 11
    "tail": (8, 12, 10, 13, 2, True, True, "values", 4),                   # W % 4 = 1
    "in_only": (8, 8, 12, 20, 2, True, False, "values", 4),
    "in_only_equal": (8, 8, 8, 8, 2, True, False, "255", 4),
    "out_only": (8, 8, 12, 20, 2, False, True, "values", 4),               # the brush applies to flow_in only: ignored
    "out_only_equal": (8, 8, 8, 8, 1, False, True, None, 4),
}
_SPECIAL = [(0.0, 1.5), (2.5, 0.0), (-0.0, 1.5), (2.5, -0.0), (NAN, 1.5), (2.5, NAN), (0.0, 0.0), (-0.0, -0.0), (NAN, NAN), (-0.0, NAN)]


def _flow(n, hs, ws, seed, special):
    f = torch.randn(n, 2, hs, ws, generator=torch.Generator().manual_seed(seed)) * 7
    if special:                                               # pixels with one zero component, -0.0, NaN
        for j, (vx, vy) in enumerate(_SPECIAL):
            y, x = (3 * j + 1) % hs, (5 * j + 2) % ws
            f[j % n, 0, y, x], f[j % n, 1, y, x] = vx, vy
            f[(j + 1) % n, 0, (y + 2) % hs, x], f[(j + 1) % n, 1, (y + 2) % hs, x] = vy, vx
    return f


def nearest_rows(out, inp):
    """source index per output index, as resize_nearest_kernel forms it: fp32 scale in / out, fp32 product, floorf, clamp"""
    scale = np.float32(inp) / np.float32(out)
    return np.minimum(np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64), inp - 1)


def finish_expect(flow_in, flow_out, brush, H, W):
    """cmp.get_cmp_flow's brush multiply + cmp.get_flow's resize and scalings for each group (zeros for an absent one, as
    control.controlnet_flow_from_drags has it), then control.merge_inmask_outmask"""
    ref = flow_in if flow_in is not None else flow_out
    n, _, hs, ws = ref.shape

    def tail(flow, brush_mask):
        if flow is None:
            return torch.zeros(1, n, 2, H, W)
        flow = flow.clone()
        if brush_mask is not None:
            bm = (torch.as_tensor(brush_mask) / 255.).to(dtype=flow.dtype)
            flow = flow * bm.unsqueeze(0).unsqueeze(0)
        flow = flow.reshape(1, n, 2, hs, ws)
        if H != hs or W != ws:
            f = F.interpolate(flow.reshape(n * 2, 1, hs, ws), (H, W), mode="nearest")
            flow = f.reshape(1, n, 2, H, W)
            flow[:, :, 0] *= W / ws
            flow[:, :, 1] *= H / hs
        return flow
    return control.merge_inmask_outmask(tail(flow_in, brush), tail(flow_out, None))[0].contiguous()


def finish_case(name):
    """-> flow_in, flow_out (fp32 [n,2,hs,ws] or None), brush (uint8 [hs,ws] or None), H, W, expectation fp32 [n,2,H,W], offset"""
    hs, ws, H, W, n, has_in, has_out, brush_kind, off = FINISH_CASES[name]
    seed = sorted(FINISH_CASES).index(name)
    fin = _flow(n, hs, ws, 2 * seed, True) if has_in else None
    fout = _flow(n, hs, ws, 2 * seed + 1, not has_in) if has_out else None      # alone it is not merged: (0, v) pixels stay
    if fout is not None:
        fout[0, 0, 0, 0], fout[0, 1, hs - 1, ws - 1] = NAN, -0.0
    brush = None
    if brush_kind == "255":
        brush = torch.full((hs, ws), 255, dtype=torch.uint8)
    elif brush_kind == "values":
        pick = torch.randint(0, 5, (hs, ws), generator=torch.Generator().manual_seed(seed + 100))
        brush = torch.tensor([0, 1, 128, 254, 255], dtype=torch.uint8)[pick]
    return fin, fout, brush, H, W, finish_expect(fin, fout, brush, H, W), off


# ---- guard buffers and comparison -------------------------------------------------------------------------------------------
class Guarded:
    """a contiguous tensor placed ``off`` elements into a 1-D guard buffer filled with NaN (0xA5 bytes for integers), with as
    much guard behind it; ``intact()`` says whether everything outside the view still has its fill"""

    def __init__(self, shape, dtype, device, data=None, off=4, pad=64):
        numel = int(np.prod(shape))
        self.float = dtype.is_floating_point
        self.buf = torch.full((off + numel + pad,), NAN if self.float else 0xA5 - 256 * (dtype != torch.uint8), dtype=dtype, device=device)
        self.lo, self.hi = off, off + numel
        self.t = self.buf[self.lo:self.hi].view(shape)
        if data is not None:
            self.t.copy_(data)
        self.fill = self.buf[:1].clone()

    def intact(self):
        g = torch.cat([self.buf[:self.lo], self.buf[self.hi:]])
        return bool(torch.isnan(g).all()) if self.float else bool((g == self.fill).all())


def same_bits(a, b):
    """byte equality of two fp32 tensors: NaNs compare by their bits, -0.0 differs from 0.0"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
