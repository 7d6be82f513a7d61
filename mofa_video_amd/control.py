"""Control-signal rasterisers: host-side conversion of user trajectories / facial landmarks into the sparse
flow + mask the CMP encoder consumes, with the reference's function names and array conventions.  Plain numpy / torch on
the host, as in the reference (these are format conversions of a few dozen points, not kernels).

  interpolate_trajectory, divide_points_afterinterpolate, get_sparseflow_and_mask_forward   Traj/run_gradio.py:41-86, :162-177
  tracking_points_to_drags                                                                   Traj/run_gradio.py:487-535 (glue of `run`)
  merge_inmask_outmask, controlnet_flow_from_drags                                           Traj/run_gradio.py:290-330 (forward_sample)
  sample_optical_flow, get_sparse_flow                                                       Keypoint/utils/utils.py:81-119
  sample_inputs_face                                                                         Keypoint/mofa_keypoint.py:36-63

The functions above stay on the host and are what the device path is compared against.  ``controlnet_flow_from_tracks`` and
``controlnet_flow_from_landmarks`` are that device path: the host keeps only the few hundred numbers (PCHIP, truncation,
brush test), ``ops.sparse_points`` writes the dense CMP input on the device and ``ops.flow_finish`` turns CMP's output
into ``controlnet_flow`` in one pass (csrc/control.hip), bit-equal to the host compositions."""
import numpy as np
import torch
from scipy.interpolate import PchipInterpolator


def interpolate_trajectory(points, n_points):
    """PCHIP through the user's control points (parameter = index / (len-1)), resampled at n_points."""
    pts = np.asarray(points, dtype=np.float64)
    t = np.linspace(0, 1, len(pts))
    s = np.linspace(0, 1, n_points)
    return list(zip(PchipInterpolator(t, pts[:, 0])(s), PchipInterpolator(t, pts[:, 1])(s)))


def divide_points_afterinterpolate(resized_all_points, motion_brush_mask):
    """tracks [K,T,2] (x,y) split by whether their START pixel lies inside the motion brush (mask == 255)."""
    pts = np.asarray(resized_all_points)
    inside = [motion_brush_mask[int(p[0][1])][int(p[0][0])] == 255 for p in pts]
    return (np.array([p for p, i in zip(pts, inside) if i]), np.array([p for p, i in zip(pts, inside) if not i]))


def get_sparseflow_and_mask_forward(resized_all_points, n_steps, H, W, is_backward_flow=False):
    """[K, n_steps+1, 2] tracks -> flow [n_steps,H,W,2] / mask [n_steps,H,W]: at every track's start pixel, step i holds
    the INTEGER displacement to its (i+1)-th point; tracks starting on the same pixel add up."""
    pts = np.asarray(resized_all_points)
    flow = np.zeros((n_steps, H, W, 2))
    mask = np.zeros((n_steps, H, W))
    sign = -1 if is_backward_flow is True else 1
    for track in pts:
        x0, y0 = int(track[0][0]), int(track[0][1])
        for i in range(n_steps):
            flow[i, y0, x0] += np.int64(track[i + 1] - track[0]) * sign
            mask[i, y0, x0] += 1
    return flow, mask


def tracking_points_to_drags(tracking_points, width, height, model_length, motion_brush_mask, work=384,
                             original_size=None):
    """The glue of DragNUWA-style `run`: user tracks (pixel coordinates at original_size) -> in-brush / out-of-brush sparse
    drags at the CMP working size.  Returns dict(drag_in, mask_in, drag_out, mask_out [1,T-1,work,work(,2)] tensors,
    in_flag, out_flag)."""
    ow, oh = original_size if original_size is not None else (width, height)
    tracks_work = [[(int(x * work / ow), int(y * work / oh)) for x, y in tr] for tr in tracking_points]
    pts = np.array([interpolate_trajectory(tr, model_length) for tr in tracks_work])
    brush = np.asarray(motion_brush_mask)
    if brush.shape != (work, work):
        # cv2.resize(mask, (work, work), cv2.INTER_NEAREST) passes the flag as dst, i.e. it is a BILINEAR resize in the
        # reference (run_gradio.py:394); brushes already at the working size avoid the ambiguity
        raise ValueError("pass the motion brush mask at the CMP working size")
    inm, outm = divide_points_afterinterpolate(pts, brush)
    n = model_length - 1
    out = {}
    for name, group in (("in", inm), ("out", outm)):
        if group.shape[0] != 0:
            f, m = get_sparseflow_and_mask_forward(group, n, work, work)
        else:
            f, m = np.zeros((n, work, work, 2)), np.zeros((n, work, work))
        out["drag_" + name], out["mask_" + name] = torch.from_numpy(f).unsqueeze(0), torch.from_numpy(m).unsqueeze(0)
        out[name + "_flag"] = group.shape[0] != 0
    return out


def track_points(tracking_points, width, height, model_length, motion_brush_mask, work=384, original_size=None):
    """The host half of ``tracking_points_to_drags`` without the dense arrays: user tracks -> per track
    ``start`` int32 [K,2] = (row, col) of its start pixel at the working size, ``disp`` int32 [K,T-1,2] = (dx, dy) =
    ``np.int64(track[i+1] - track[0])`` of the float64 PCHIP points (truncated toward zero) and ``inside`` bool [K] = the
    start pixel lies inside the motion brush (== 255).  Scattering them (adding tracks that share a start pixel) gives
    ``tracking_points_to_drags``'s arrays."""
    ow, oh = original_size if original_size is not None else (width, height)
    tracks_work = [[(int(x * work / ow), int(y * work / oh)) for x, y in tr] for tr in tracking_points]
    pts = np.array([interpolate_trajectory(tr, model_length) for tr in tracks_work], dtype=np.float64).reshape(-1, model_length, 2)
    brush = np.asarray(motion_brush_mask)
    if brush.shape != (work, work):
        raise ValueError("pass the motion brush mask at the CMP working size")
    x0, y0 = pts[:, 0, 0].astype(np.int64), pts[:, 0, 1].astype(np.int64)       # int(): toward zero
    inside = (brush[y0, x0] == 255).reshape(-1)
    start = np.stack([y0, x0], axis=1).astype(np.int32)
    disp = np.int64(pts[:, 1:] - pts[:, 0:1]).astype(np.int32)
    return start, disp, inside


SPARSE_EXACT = 1 << 24         # integer sums below this are exact in fp32


def controlnet_flow_from_tracks(cmp, first_frame, tracking_points, height, width, model_length, motion_brush_mask=None, work=384,
                                original_size=None):
    """``controlnet_flow_from_drags(cmp, first_frame, tracking_points_to_drags(...), ...)`` with the dense work on the device:
    first_frame [1,3,H,W] in (0,1), user tracks as for ``tracking_points_to_drags`` -> controlnet_flow fp32 [1,T-1,2,H,W] on
    ``cmp.device``, bit-equal to that composition.  ``motion_brush_mask``: uint8 [work,work] or None (= no brush: every track
    is out-of-brush).  Start pixels must lie on the working canvas (ValueError; the host path wraps negative ones the numpy
    way and raises IndexError beyond it), and a start pixel's summed displacement must stay below 2^24, where fp32 sums of
    integers are exact (ValueError)."""
    from . import lib as L
    from . import ops
    dev = cmp.device
    brush = np.zeros((work, work), dtype=np.uint8) if motion_brush_mask is None else np.asarray(motion_brush_mask)
    start, disp, inside = track_points(tracking_points, width, height, model_length, brush, work, original_size)
    n = model_length - 1
    ff = torch.nn.functional.interpolate(first_frame.float(), (work, work)).repeat(n, 1, 1, 1).to(dev)
    flows = {}
    for name, sel in (("in", inside), ("out", ~inside)):
        flows[name] = None
        if not sel.any():
            continue                                                             # an empty group skips CMP
        pos, d = start[sel], disp[sel]
        shared = int(np.unique(pos, axis=0, return_counts=True)[1].max())
        if shared * int(np.abs(d.astype(np.int64)).max(initial=0)) >= SPARSE_EXACT:
            raise ValueError(f"{shared} tracks on one start pixel with displacements up to {int(np.abs(d).max())}: the sum is not "
                             f"exact in fp32")
        val = torch.from_numpy(np.ascontiguousarray(d.transpose(1, 0, 2)).astype(np.float32)).to(dev)      # [n,K,2]
        sp = ops.sparse_points(torch.from_numpy(pos), val, work, work, L.SPARSE_ADD)
        flows[name] = cmp.run(ff, sp[:, :2], sp[:, 2:]).float().contiguous()
    if flows["in"] is None and flows["out"] is None:
        return torch.zeros(1, n, 2, height, width, device=dev)
    bm = None
    if motion_brush_mask is not None and flows["in"] is not None:
        bm = torch.from_numpy(np.ascontiguousarray(brush, dtype=np.uint8)).to(dev)
    return ops.flow_finish(flows["in"], flows["out"], bm, height, width).unsqueeze(0)


def merge_inmask_outmask(flow_inmask, flow_outmask):
    """forward_sample: where BOTH components of the in-brush flow are non-zero it wins, elsewhere the out-of-brush flow."""
    keep = (flow_inmask != 0).all(dim=2).unsqueeze(2).expand_as(flow_inmask)
    return torch.where(keep, flow_inmask, flow_outmask)


def controlnet_flow_from_drags(cmp, first_frame, drags, height, width, motion_brush_mask=None, work=384):
    """first_frame [1,3,H,W] in (0,1); drags = tracking_points_to_drags(...).  Returns controlnet_flow [1,T-1,2,H,W]."""
    from .cmp import get_flow
    n = drags["drag_in"].shape[1]
    ff = torch.nn.functional.interpolate(first_frame.float(), (work, work)).repeat(n, 1, 1, 1).unsqueeze(0)
    flows = {}
    for name in ("in", "out"):
        if drags[name + "_flag"]:
            d = drags["drag_" + name].permute(0, 1, 4, 2, 3).float()
            m = drags["mask_" + name].unsqueeze(2).repeat(1, 1, 2, 1, 1).float()
            flows[name] = get_flow(cmp, ff, d, m, height, width, motion_brush_mask if name == "in" else None)
        else:
            flows[name] = torch.zeros(1, n, 2, height, width, device=cmp.device)
    return merge_inmask_outmask(flows["in"], flows["out"])


def sample_optical_flow(A, B, h, w):
    """A [b,l,k,2] integer-valued (row, col) positions, B [b,l,k,2] values -> dense [b,l,h,w,2] + uint8 mask [b,l,h,w,2].
    Positions are clipped as the reference clips them (rows to h-1, cols to w-1); later points overwrite earlier ones."""
    b, l, k, _ = A.shape
    flow = torch.zeros((b, l, h, w, 2), dtype=B.dtype, device=B.device)
    mask = torch.zeros((b, l, h, w), dtype=torch.uint8, device=B.device)
    rows = torch.clip(A[..., 0].long(), 0, h - 1)
    cols = torch.clip(A[..., 1].long(), 0, w - 1)
    bi = torch.arange(b)[:, None, None].expand(b, l, k)
    li = torch.arange(l)[None, :, None].expand(b, l, k)
    flow[bi, li, rows, cols] = B
    mask[bi, li, rows, cols] = 1
    return flow, mask.unsqueeze(-1).repeat(1, 1, 1, 1, 2)


@torch.no_grad()
def get_sparse_flow(landmarks, h, w, t):
    """landmarks [b,t,68,2] (x,y) pixels -> forward sparse flow of frames 1..t-1 w.r.t. frame 0, sampled at frame 0's
    landmark pixels: ([b,t-1,2,h,w] flow (dx,dy), [b,t-1,2,h,w] mask)."""
    yx = torch.flip(landmarks, dims=[3])
    disp = torch.flip((yx - yx[:, 0:1])[:, 1:], dims=[3])            # back to (dx, dy)
    pos = yx[:, 0:1].repeat(1, t - 1, 1, 1)
    flow, mask = sample_optical_flow(pos, disp, h, w)
    return flow.permute(0, 1, 4, 2, 3), mask.permute(0, 1, 4, 2, 3)


def sample_inputs_face(first_frame, landmarks):
    """mofa_keypoint.py:36-63: first_frame [3,H,W], landmarks [N,68,2] (x, y) pixels -> (controlnet_image [1,3,H,W], sparse flow
    and mask at H x W, first_frame_384, sparse flow and mask at 384 x 384).  Everything is computed in the landmarks' dtype, as
    the reference does; it passes fp16 landmarks, so the 384-grid positions are fp16 quotients (``x / W * 384`` rounded to
    fp16 after each operation), not fp32 ones."""
    pc, ph, pw = first_frame.shape
    landmarks = landmarks.unsqueeze(0)
    pl = landmarks.shape[1]
    sparse_optical_flow, mask = get_sparse_flow(landmarks, ph, pw, pl)
    if ph != 384 or pw != 384:
        first_frame_384 = torch.nn.functional.interpolate(first_frame.unsqueeze(0), (384, 384))
        landmarks_384 = torch.zeros_like(landmarks)
        landmarks_384[:, :, :, 0] = landmarks[:, :, :, 0] / pw * 384
        landmarks_384[:, :, :, 1] = landmarks[:, :, :, 1] / ph * 384
        sparse_optical_flow_384, mask_384 = get_sparse_flow(landmarks_384, 384, 384, pl)
    else:
        first_frame_384 = first_frame
        sparse_optical_flow_384, mask_384 = sparse_optical_flow, mask
    return first_frame.unsqueeze(0), sparse_optical_flow, mask, first_frame_384, sparse_optical_flow_384, mask_384


@torch.no_grad()
def landmark_points(landmarks):
    """landmarks [1,t,k,2] (x, y) on the host -> what ``get_sparse_flow`` hands to ``sample_optical_flow``, as the arguments of
    ``ops.sparse_points(..., SPARSE_LAST)``: int32 [k,2] (row, col) positions of frame 0 (``.long()``, unclipped: the kernel
    clips) and fp32 [t-1,k,2] (dx, dy) displacements, formed in the input dtype."""
    yx = torch.flip(landmarks, dims=[3])
    disp = torch.flip((yx - yx[:, 0:1])[:, 1:], dims=[3])[0]
    pos = yx[0, 0].long().clamp(-2 ** 31, 2 ** 31 - 1).int()
    return pos.contiguous(), disp.float().contiguous()


@torch.no_grad()
def controlnet_flow_from_landmarks(cmp, first_frame, landmarks, work=384):
    """The Keypoint counterpart (mofa_keypoint.py:318-337): first_frame [3,H,W], landmarks [N,68,2] (x, y) pixels ->
    controlnet_flow fp32 [1,N-1,2,H,W] on ``cmp.device``, bit-equal to ``get_sparse_flow`` of the working-size landmarks on
    the host + ``cmp.get_flow``.  Positions and displacements are formed on the host exactly as ``get_sparse_flow`` forms
    them (flip, subtract frame 0, ``.long()``, in the landmarks' dtype -- see ``sample_inputs_face``); the dense input, CMP
    and the resize + rescale (``ops.flow_finish`` without a merge partner) run on the device.  The full-resolution sparse flow of ``sample_inputs_face`` is not built: nothing
    consumes it."""
    from . import lib as L
    from . import ops
    dev = cmp.device
    _, ph, pw = first_frame.shape
    lm = landmarks.detach().cpu().unsqueeze(0)
    n = lm.shape[1] - 1
    ff = first_frame.unsqueeze(0)
    if ph != work or pw != work:
        ff = torch.nn.functional.interpolate(ff, (work, work))
        lw = torch.zeros_like(lm)
        lw[:, :, :, 0] = lm[:, :, :, 0] / pw * work
        lw[:, :, :, 1] = lm[:, :, :, 1] / ph * work
        lm = lw
    pos, disp = landmark_points(lm)
    sp = ops.sparse_points(pos, disp.to(dev), work, work, L.SPARSE_LAST)
    flow = cmp.run(ff.repeat(n, 1, 1, 1).to(dev), sp[:, :2], sp[:, 2:]).float().contiguous()
    # as the out-of-brush flow: the Keypoint path has no in-brush / out-of-brush merge, and the merge's test "both components
    # non-zero" would zero the other component of a pixel whose flow has one exact zero
    return ops.flow_finish(None, flow, None, ph, pw).unsqueeze(0)
