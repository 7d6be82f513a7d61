// Decision logic of the control-signal kernels (csrc/control.hip) as __host__ __device__ functions: the same text
// runs in the kernels and on the host in tests/control_points_main.hip.
//   * sparse points (mofa_sparse_points_f32): a point's pixel key, "am I the thread that writes this pixel", and the value
//     it writes.  Every pixel has exactly one writer, chosen by position in the point list alone, so there are no atomics
//     and nothing depends on the order threads run in.
//   * flow finish (mofa_flow_finish_f32): the nearest-neighbour source index (shared with resize_nearest_kernel of
//     elementwise.hip) and the per-pixel brush multiply, rescale and in-brush / out-of-brush merge, every operation
//     rounded on its own (contraction off), as the torch composition of cmp.get_flow + control.merge_inmask_outmask does.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

constexpr int CONTROL_MAX_POINTS = 4096;   // K of one launch: the keys of all points sit in LDS (16 KB)
constexpr int CONTROL_SPARSE_ADD = 0;      // = MOFA_SPARSE_ADD
constexpr int CONTROL_SPARSE_LAST = 1;     // = MOFA_SPARSE_LAST

// F.interpolate(mode='nearest'): source index of output index o, scale = (float)in / (float)out
__host__ __device__ inline int nearest_src(const int o, const float scale, const int in) {
    const int i = (int)floorf((float)o * scale);
    return i < in - 1 ? i : in - 1;
}

__host__ __device__ inline int control_clip(const int v, const int size) { return v < 0 ? 0 : (v > size - 1 ? size - 1 : v); }

// pixel key row * W + col of point k.  LAST clips the position onto the canvas (sample_optical_flow); ADD takes it as it is
// and gives -1 for a position off the canvas: such a point neither writes nor counts (callers refuse it beforehand).
__host__ __device__ inline int control_point_key(const int* pos, const int k, const int H, const int W, const int mode) {
    int r = pos[2 * k], c = pos[2 * k + 1];
    if (mode == CONTROL_SPARSE_LAST) {
        r = control_clip(r, H);
        c = control_clip(c, W);
    } else if (r < 0 || r >= H || c < 0 || c >= W) {
        return -1;
    }
    return r * W + c;
}

// the one point that writes its pixel: the first of its key in ADD (it then forms the whole sum), the last in LAST
__host__ __device__ inline bool control_is_writer(const int* keys, const int K, const int k, const int mode) {
    const int key = keys[k];
    if (key < 0) return false;
    if (mode == CONTROL_SPARSE_LAST) {
        for (int j = k + 1; j < K; ++j)
            if (keys[j] == key) return false;
    } else {
        for (int j = 0; j < k; ++j)
            if (keys[j] == key) return false;
    }
    return true;
}

// ADD: sum of val[j] over the points j >= k that share k's key, added in ascending j, and their number.  val: [K][2].
__host__ __device__ inline void control_add_sum(const int* keys, const float* val, const int K, const int k, float& sx, float& sy,
                                                float& count) {
    const int key = keys[k];
    sx = val[2 * k];
    sy = val[2 * k + 1];
    count = 1.0f;
    for (int j = k + 1; j < K; ++j)
        if (keys[j] == key) {
            sx += val[2 * j];
            sy += val[2 * j + 1];
            count += 1.0f;
        }
}

// uint8 / 255. as torch forms it: the correctly rounded fp32 quotient.  Formed as a double quotient rounded to fp32, which is
// the same number (a quotient rounded at p' >= 2 p + 2 bits and then at p bits is the correctly rounded one: 53 >= 50) and
// does not depend on how a compiler expands fp32 division for the device.
__host__ __device__ inline float control_brush_weight(const unsigned char b) { return (float)((double)b / 255.0); }

// one output pixel of mofa_flow_finish_f32 from its source values: a = in-brush flow (x, y), b = out-of-brush flow
__host__ __device__ inline void control_finish_pixel(float ax, float ay, float bx, float by, const bool has_brush, const unsigned char brush,
                                                     const bool scaled, const float fx, const float fy, float& ox, float& oy) {
#pragma clang fp contract(off)
    if (has_brush) {
        const float m = control_brush_weight(brush);
        ax = ax * m;
        ay = ay * m;
    }
    if (scaled) {
        ax = ax * fx;
        ay = ay * fy;
        bx = bx * fx;
        by = by * fy;
    }
    const bool keep = ax != 0.0f && ay != 0.0f;          // -0.0 is zero, NaN is not
    ox = keep ? ax : bx;
    oy = keep ? ay : by;
}
