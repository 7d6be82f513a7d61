"""The case table of the pose-image tests (test_pose_images_cpu.py runs the shared rasteriser on the host over it,
test_pose_images_gpu.py the HIP entry point): seeded landmark sets [N, 68, 2] (x, y) in the pixel coordinates of a
320 x 320 frame drawn at draw_size = 320, so that the scaling is x / 320 * 320 and the resize the identity.  The oracle of
every case is mofa_video_amd/landmarks.py on the host."""
import functools

import numpy as np

from mofa_video_amd import landmarks as L

SIZE = 320
SEGMENTS = [(idx[i] - 1, idx[i + 1] - 1, part) for part, (_n, idx, _c) in enumerate(L.PARTS) for i in range(len(idx) - 1)]
# canvas value -> colour: 0 = background, s + 1 = segment s
COLOURS = np.array([(0, 0, 0)] + [L.PARTS[part][2] for _a, _b, part in SEGMENTS], dtype=np.float64)


def faces(n=3, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(40, 280, (1, 68, 2)) + rng.normal(0, 3, (n, 68, 2))


def _clipped():
    return np.random.default_rng(1).uniform(-40, 360, (3, 68, 2))


def _all_equal(points):
    return np.stack([np.tile(np.array(p, dtype=np.float64), (68, 1)) for p in points])


def _lattice():
    """the FACE polyline walks horizontal, vertical and 45-degree steps in both directions and a steep and a shallow step
    in every sign combination; the other landmarks sit on a 10-pixel lattice.  Frames 2 and 3 are the same set shifted so that
    it crosses the top-left and the bottom-right corner."""
    steps = [(30, 0), (0, 30), (-30, 0), (0, -30), (25, 25), (-25, -25), (25, -25), (-25, 25),
             (3, 40), (-3, -40), (40, 3), (-40, -3), (3, -40), (-3, 40), (40, -3), (-40, 3)]
    pts = [(120, 120)]
    for dx, dy in steps:
        pts.append((pts[-1][0] + dx, pts[-1][1] + dy))
    pts += [((i * 37) % 29 * 10 + 15, (i * 53) % 31 * 10 + 5) for i in range(17, 68)]
    base = np.array(pts, dtype=np.float64)
    return np.stack([base, base - 110.0, base + 150.0])


def _tiny_box():
    rng = np.random.default_rng(6)
    box = rng.integers(0, 6, (3, 68, 2)).astype(np.float64)
    return box + np.array([157.0, -2.0, 316.0])[:, None, None]


def _fractional_negatives():
    lm = faces(2, seed=7)
    vals = [-0.5, -0.999, -1.0, -1.5]
    for k, v in enumerate(vals):
        lm[0, k, 0] = v                  # x just left of the canvas, FACE polyline
        lm[0, 8 + k, 1] = v              # y just above it
        lm[1, 36 + k, :] = v             # both, RIGHT_EYE
        lm[1, 48 + k, 0] = v + 0.25      # lips
    return lm


def _far_ends():
    """one end on the canvas, the other at +-32767 on each axis and on the diagonals (FACE polyline alternates on / far)"""
    lm = faces(1, seed=8)
    far = [(32767, 160), (-32767, 170), (150, 32767), (140, -32767), (32767, 32767), (-32767, -32767), (32767, -32767), (-32767, 32767)]
    on = [(160, 160), (100, 200), (0, 0), (319, 319), (10, 300), (300, 10), (160, 5), (5, 160), (250, 250)]
    for k in range(17):
        lm[0, k] = on[k // 2] if k % 2 == 0 else far[k // 2]
    return lm


RASTER_CASES = {
    "faces": faces,
    "clipped_all_borders": _clipped,
    "circles_only_on_canvas": lambda: _all_equal([(160, 160), (0, 0), (319, 319)]),
    "circles_only_off_canvas": lambda: _all_equal([(-1, -1), (320, 320)]),
    "off_canvas": lambda: faces() + 1000.0,
    "lattice_directions": _lattice,
    "tiny_box_overdraw": _tiny_box,
    "fractional_negatives": _fractional_negatives,
    "far_ends": _far_ends,
}


def scaled(lm, height, width, draw_size):
    """the float64 scaling of landmarks.pose_images"""
    lm = np.array(lm, dtype=np.float64).copy()
    lm[:, :, 0] = lm[:, :, 0] / width * draw_size
    lm[:, :, 1] = lm[:, :, 1] / height * draw_size
    return lm


@functools.lru_cache(maxsize=None)
def raster_case(name):
    """(landmarks [N, 68, 2], the host's drawn canvases [N, 320, 320, 3] float64); computed once, read-only"""
    lm = RASTER_CASES[name]()
    drawn = np.stack([L.draw_landmarks(f, SIZE, SIZE) for f in scaled(lm, SIZE, SIZE, SIZE)])
    lm.setflags(write=False)
    drawn.setflags(write=False)
    return lm, drawn
