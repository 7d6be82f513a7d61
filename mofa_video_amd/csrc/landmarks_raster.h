// Per-segment rasteriser of the landmark pose images: mofa_video_amd/landmarks.py, operation by operation, as
// __host__ __device__ functions that paint through a "plot pixel" callable -- the same text runs in the kernel of
// landmarks.hip (plot = atomicMax of the segment number into an int32 canvas) and on the host in tests/pose_raster_main.hip.
// One segment = landmarks.line(p1, p2, thickness = 2) = cv::ThickLine: FillConvexPoly of the 16.16 fixed-point quad (its four
// Line2 edges after clipLine, then one span per scanline) and a filled radius-1 Circle at both ends.  The rasterisers only
// write and a segment's coverage does not depend on the canvas, so the frame landmarks.draw_landmarks paints is, per pixel,
// the colour of the highest-numbered segment that covers it: 63 independent segments per frame.
// All fixed-point arithmetic is int64_t (|coordinate| <= 32767 -> |16.16 value| < 2^31, products < 2^49); `/` is C's
// truncating division where the Python uses _tdiv, `>>` an arithmetic shift as Python's, `* 65536` stands for `<< 16` of a
// possibly negative value.  Floating point is double with contraction off, as numpy computes it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

constexpr int POSE_XY_SHIFT = 16;
constexpr int64_t POSE_XY_ONE = 65536;
constexpr int POSE_POINTS = 68;       // landmarks per frame
constexpr int POSE_SEGMENTS = 63;     // the 15 polylines of landmarks.PARTS, in drawing order
constexpr int POSE_PARTS = 15;
constexpr int POSE_MAX_COORD = 32767; // the wrapper's limit on a scaled coordinate: bounds the scanline walk of one segment

// segment s (0-based, in landmarks.PARTS order) joins landmarks a and b (0-based) and belongs to polyline `part`
__host__ __device__ inline void pose_segment(int s, int& a, int& b, int& part) {
    const unsigned char A[POSE_SEGMENTS] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15,   // FACE
                                            42, 43, 44, 45, 46, 47,                                          // LEFT_EYE
                                            22, 23, 24, 25,                                                  // LEFT_EYEBROW
                                            36, 37, 38, 39, 40, 41,                                          // RIGHT_EYE
                                            17, 18, 19, 20,                                                  // RIGHT_EYEBROW
                                            27, 28, 29,                                                      // NOSE_UP
                                            31, 32, 33, 34,                                                  // NOSE_DOWN
                                            54, 55, 56,                                                      // LIPS_OUTER_BOTTOM_LEFT
                                            48, 59, 58,                                                      // LIPS_OUTER_BOTTOM_RIGHT
                                            64, 65,                                                          // LIPS_INNER_BOTTOM_LEFT
                                            60, 67,                                                          // LIPS_INNER_BOTTOM_RIGHT
                                            51, 52, 53,                                                      // LIPS_OUTER_TOP_LEFT
                                            51, 50, 49,                                                      // LIPS_OUTER_TOP_RIGHT
                                            62, 63,                                                          // LIPS_INNER_TOP_LEFT
                                            62, 61};                                                         // LIPS_INNER_TOP_RIGHT
    const unsigned char B[POSE_SEGMENTS] = {1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16,
                                            43, 44, 45, 46, 47, 42,
                                            23, 24, 25, 26,
                                            37, 38, 39, 40, 41, 36,
                                            18, 19, 20, 21,
                                            28, 29, 30,
                                            32, 33, 34, 35,
                                            55, 56, 57,
                                            59, 58, 57,
                                            65, 66,
                                            67, 66,
                                            52, 53, 54,
                                            50, 49, 48,
                                            63, 64,
                                            61, 60};
    const unsigned char P[POSE_SEGMENTS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3,
                                            4, 4, 4, 4, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 8, 8, 8, 9, 9, 10, 10, 11, 11, 11, 12, 12, 12,
                                            13, 13, 14, 14};
    a = A[s]; b = B[s]; part = P[s];
}

// colour channel c (0..2) of polyline `part` (landmarks.PARTS)
__host__ __device__ inline int pose_part_colour(int part, int c) {
    const unsigned char COL[POSE_PARTS][3] = {{10, 200, 10},  {180, 200, 10}, {180, 220, 10}, {10, 200, 180}, {10, 220, 180},
                                              {10, 200, 250}, {250, 200, 10}, {10, 180, 20},  {20, 10, 180},  {100, 100, 30},
                                              {100, 150, 50}, {20, 80, 100},  {80, 100, 20},  {120, 100, 200}, {150, 120, 100}};
    return COL[part][c];
}

__host__ __device__ inline int64_t pose_abs64(int64_t v) { return v < 0 ? -v : v; }

template <class Plot>
__host__ __device__ inline void pose_hline(int y, int64_t x1, int64_t x2, Plot& plot) {
    for (int64_t x = x1; x <= x2; ++x) plot((int)x, y);
}

// landmarks._clip_line: cv::clipLine on fixed-point coordinates; the double-precision products truncate
__host__ __device__ inline bool pose_clip_line(int64_t w_fx, int64_t h_fx, int64_t& x1, int64_t& y1, int64_t& x2, int64_t& y2) {
#pragma clang fp contract(off)
    const int64_t right = w_fx - 1, bottom = h_fx - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        if (c1 & 12) {
            const int64_t a = c1 < 8 ? 0 : bottom;
            x1 += (int64_t)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            const int64_t a = c2 < 8 ? 0 : bottom;
            x2 += (int64_t)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                const int64_t a = c1 == 1 ? 0 : right;
                y1 += (int64_t)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                const int64_t a = c2 == 1 ? 0 : right;
                y2 += (int64_t)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// landmarks._line2: cv::Line2 between 16.16 end points, one pixel per step along the major axis
template <class Plot>
__host__ __device__ inline void pose_line2(int w, int h, int64_t x1, int64_t y1, int64_t x2, int64_t y2, Plot& plot) {
    if (!pose_clip_line((int64_t)w * POSE_XY_ONE, (int64_t)h * POSE_XY_ONE, x1, y1, x2, y2)) return;
    int64_t dx = x2 - x1, dy = y2 - y1;
    const int64_t ax = pose_abs64(dx), ay = pose_abs64(dy);
    const bool wide = ax > ay;
    int64_t x_step, y_step, ecount, t;
    if (wide) {
        if (dx < 0) {                                     // walk left to right
            dy = -dy;
            t = x1; x1 = x2; x2 = t;
            t = y1; y1 = y2; y2 = t;
        }
        x_step = POSE_XY_ONE; y_step = dy * POSE_XY_ONE / (ax | 1);
        ecount = (x2 - x1) >> POSE_XY_SHIFT;
    } else {
        if (dy < 0) {                                     // walk top to bottom
            dx = -dx;
            t = x1; x1 = x2; x2 = t;
            t = y1; y1 = y2; y2 = t;
        }
        x_step = dx * POSE_XY_ONE / (ay | 1); y_step = POSE_XY_ONE;
        ecount = (y2 - y1) >> POSE_XY_SHIFT;
    }
    x1 += POSE_XY_ONE >> 1;
    y1 += POSE_XY_ONE >> 1;
    auto put = [&](int64_t x, int64_t y) {
        if (0 <= x && x < w && 0 <= y && y < h) plot((int)x, (int)y);
    };
    put((x2 + (POSE_XY_ONE >> 1)) >> POSE_XY_SHIFT, (y2 + (POSE_XY_ONE >> 1)) >> POSE_XY_SHIFT);
    if (wide) {
        x1 >>= POSE_XY_SHIFT;
        for (; ecount >= 0; --ecount) {
            put(x1, y1 >> POSE_XY_SHIFT);
            x1 += 1;
            y1 += y_step;
        }
    } else {
        y1 >>= POSE_XY_SHIFT;
        for (; ecount >= 0; --ecount) {
            put(x1 >> POSE_XY_SHIFT, y1);
            x1 += x_step;
            y1 += 1;
        }
    }
}

// landmarks._fill_convex_poly for the quad of ThickLine (npts = 4, shift = XY_SHIFT): the outline by Line2, then one span per
// scanline between the two active edges
template <class Plot>
__host__ __device__ inline void pose_fill_quad(int w, int h, const int64_t (&vx)[4], const int64_t (&vy)[4], Plot& plot) {
    const int npts = 4;
    const int64_t delta = POSE_XY_ONE >> 1;
    int64_t xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0];
    int imin = 0;
    int64_t px = vx[npts - 1], py = vy[npts - 1];
    for (int i = 0; i < npts; ++i) {
        if (vy[i] < ymin) { ymin = vy[i]; imin = i; }
        ymax = vy[i] > ymax ? vy[i] : ymax;
        xmax = vx[i] > xmax ? vx[i] : xmax;
        xmin = vx[i] < xmin ? vx[i] : xmin;
        pose_line2(w, h, px, py, vx[i], vy[i], plot);
        px = vx[i]; py = vy[i];
    }
    xmin = (xmin + delta) >> POSE_XY_SHIFT; xmax = (xmax + delta) >> POSE_XY_SHIFT;
    ymin = (ymin + delta) >> POSE_XY_SHIFT; ymax = (ymax + delta) >> POSE_XY_SHIFT;
    if (xmax < 0 || ymax < 0 || xmin >= w || ymin >= h) return;
    ymax = ymax < h - 1 ? ymax : h - 1;
    int e_idx[2] = {imin, imin};
    const int e_di[2] = {1, npts - 1};
    int64_t e_x[2] = {-POSE_XY_ONE, -POSE_XY_ONE}, e_dx[2] = {0, 0}, e_ye[2] = {ymin, ymin};
    int edges = npts;
    int64_t y = ymin;
    do {
        for (int i = 0; i < 2; ++i) {
            if (y < e_ye[i]) continue;
            int idx0 = e_idx[i];
            const int di = e_di[i];
            int idx = idx0 + di;
            if (idx >= npts) idx -= npts;
            for (;;) {
                if (--edges < 0) break;                   // `for (; edges-- > 0; )` ran out
                const int64_t ty = (vy[idx] + delta) >> POSE_XY_SHIFT;
                if (ty > y) {
                    const int64_t xs = vx[idx0], xe = vx[idx];
                    e_ye[i] = ty;
                    e_dx[i] = ((xe - xs) * 2 + (ty - y)) / (2 * (ty - y));
                    e_x[i] = xs;
                    e_idx[i] = idx;
                    break;
                }
                idx0 = idx;
                idx += di;
                if (idx >= npts) idx -= npts;
            }
        }
        if (edges < 0) break;
        if (y >= 0) {
            const int left = e_x[0] > e_x[1] ? 1 : 0, right = 1 - left;
            const int64_t xx1 = (e_x[left] + delta) >> POSE_XY_SHIFT, xx2 = (e_x[right] + delta) >> POSE_XY_SHIFT;
            if (xx2 >= 0 && xx1 < w) pose_hline((int)y, xx1 > 0 ? xx1 : 0, xx2 < w - 1 ? xx2 : w - 1, plot);
        }
        e_x[0] += e_dx[0];
        e_x[1] += e_dx[1];
        ++y;
    } while (y <= ymax);
}

// landmarks._circle_filled: cv::Circle(fill), midpoint circle drawn as horizontal spans
template <class Plot>
__host__ __device__ inline void pose_circle_filled(int w, int h, int64_t cx, int64_t cy, int radius, Plot& plot) {
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        const int64_t y11 = cy - dy, y12 = cy + dy, y21 = cy - dx, y22 = cy + dx;
        const int64_t x11 = cx - dx, x12 = cx + dx, x21 = cx - dy, x22 = cx + dy;
        if (x11 < w && x12 >= 0 && y21 < h && y22 >= 0) {
            int64_t a = x11 > 0 ? x11 : 0, b = x12 < w - 1 ? x12 : w - 1;
            if (0 <= y11 && y11 < h) pose_hline((int)y11, a, b, plot);
            if (0 <= y12 && y12 < h) pose_hline((int)y12, a, b, plot);
            if (x21 < w && x22 >= 0) {
                a = x21 > 0 ? x21 : 0; b = x22 < w - 1 ? x22 : w - 1;
                if (0 <= y21 && y21 < h) pose_hline((int)y21, a, b, plot);
                if (0 <= y22 && y22 < h) pose_hline((int)y22, a, b, plot);
            }
        }
        dy += 1;
        err += plus;
        plus += 2;
        const int mask = err > 0 ? -1 : 0;                // (err <= 0) - 1
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

// landmarks.line(img, (x0, y0), (x1, y1), colour, thickness = 2) on a w x h canvas: every pixel it paints goes to plot(x, y),
// 0 <= x < w, 0 <= y < h.  |coordinate| <= POSE_MAX_COORD (the caller checks).
template <class Plot>
__host__ __device__ inline void pose_thick_line(int w, int h, int x0, int y0, int x1, int y1, Plot& plot) {
#pragma clang fp contract(off)
    const int thickness = 2;
    const int64_t p0x = (int64_t)x0 * POSE_XY_ONE, p0y = (int64_t)y0 * POSE_XY_ONE;
    const int64_t p1x = (int64_t)x1 * POSE_XY_ONE, p1y = (int64_t)y1 * POSE_XY_ONE;
    const double inv = 1.0 / (double)POSE_XY_ONE;
    const double dx = (double)(p0x - p1x) * inv, dy = (double)(p1y - p0y) * inv;
    double r = dx * dx + dy * dy;
    const int odd = thickness & 1;
    const int64_t th = (int64_t)thickness << (POSE_XY_SHIFT - 1);
    if (fabs(r) > 2.220446049250313e-16) {
        r = ((double)th + (double)(odd * POSE_XY_ONE) * 0.5) / sqrt(r);
        const int64_t dpx = (int64_t)rint(dy * r), dpy = (int64_t)rint(dx * r);   // cvRound: half to even
        const int64_t vx[4] = {p0x + dpx, p0x - dpx, p1x - dpx, p1x + dpx};
        const int64_t vy[4] = {p0y + dpy, p0y - dpy, p1y - dpy, p1y + dpy};
        pose_fill_quad(w, h, vx, vy, plot);
    }
    const int radius = (int)((th + (POSE_XY_ONE >> 1)) >> POSE_XY_SHIFT);
    pose_circle_filled(w, h, (p0x + (POSE_XY_ONE >> 1)) >> POSE_XY_SHIFT, (p0y + (POSE_XY_ONE >> 1)) >> POSE_XY_SHIFT, radius, plot);
    pose_circle_filled(w, h, (p1x + (POSE_XY_ONE >> 1)) >> POSE_XY_SHIFT, (p1y + (POSE_XY_ONE >> 1)) >> POSE_XY_SHIFT, radius, plot);
}

// segment s of one frame: pts = that frame's [68][2] (x, y).  A segment with an end point beyond POSE_MAX_COORD is not drawn
// (its scanline walk would be unbounded); the Python wrapper raises before it comes to that.
template <class Plot>
__host__ __device__ inline void pose_draw_segment(int w, int h, const int32_t* pts, int s, Plot& plot) {
    int a, b, part;
    pose_segment(s, a, b, part);
    const int x0 = pts[2 * a], y0 = pts[2 * a + 1], x1 = pts[2 * b], y1 = pts[2 * b + 1];
    if (x0 < -POSE_MAX_COORD || x0 > POSE_MAX_COORD || y0 < -POSE_MAX_COORD || y0 > POSE_MAX_COORD || x1 < -POSE_MAX_COORD ||
        x1 > POSE_MAX_COORD || y1 < -POSE_MAX_COORD || y1 > POSE_MAX_COORD)
        return;
    pose_thick_line(w, h, x0, y0, x1, y1, plot);
}
