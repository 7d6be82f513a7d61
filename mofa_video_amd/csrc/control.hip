// Control signals on the device: the two ends of the path from user tracks / facial landmarks to controlnet_flow.
//   * mofa_sparse_points_f32: K (pixel, value) pairs per frame -> the dense fp32 [n][4][H][W] input of the CMP encoder
//     (dx, dy, mask, mask).  The launch clears the output (a memset on the stream), then one thread per (frame, point):
//     the workgroup holds the pixel keys of all K points in LDS, a thread scans them (control_points.h) and writes only if
//     it is the first (ADD) or the last (LAST) point of its pixel; in ADD it forms the whole sum itself in ascending point
//     order.  One writer per pixel: no atomics, bit-identical from launch to launch.
//   * mofa_flow_finish_f32: the tail of cmp.get_flow (brush multiply, nearest resize, rescale) and merge_inmask_outmask
//     in one pass: one thread per four output pixels along x, both components, 16-byte loads where the four sources are a
//     contiguous aligned run, 16-byte stores where rows are 16-byte aligned; the result is written once.
#include "common.h"
#include "control_points.h"

static_assert(CONTROL_SPARSE_ADD == MOFA_SPARSE_ADD && CONTROL_SPARSE_LAST == MOFA_SPARSE_LAST, "mode values");

__global__ __launch_bounds__(256) void sparse_points_kernel(const int* __restrict__ pos, const float* __restrict__ val,
                                                            float* __restrict__ out, const int K, const int H, const int W,
                                                            const int mode) {
    __shared__ int keys[CONTROL_MAX_POINTS];
    for (int j = threadIdx.x; j < K; j += 256) keys[j] = control_point_key(pos, j, H, W, mode);
    __syncthreads();
    const int k = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (k >= K || !control_is_writer(keys, K, k, mode)) return;
    const float* v = val + (size_t)i * K * 2;
    float sx, sy, count;
    if (mode == CONTROL_SPARSE_ADD) {
        control_add_sum(keys, v, K, k, sx, sy, count);
    } else {
        sx = v[2 * k];                                       // copied as they are, NaN included
        sy = v[2 * k + 1];
        count = 1.0f;
    }
    const size_t hw = (size_t)H * W;
    float* o = out + (size_t)i * 4 * hw + keys[k];           // 0 <= keys[k] < H * W (control_point_key)
    o[0] = sx;
    o[hw] = sy;
    o[2 * hw] = count;
    o[3 * hw] = count;
}

extern "C" int mofa_sparse_points_f32(const int* pos, const float* val, int K, int n, int H, int W, int mode, float* out,
                                      mofa_stream_t stream) {
    if (!out || K < 0 || K > CONTROL_MAX_POINTS || n <= 0 || H <= 0 || W <= 0 || n > 65535) return MOFA_EINVAL;
    if (mode != MOFA_SPARSE_ADD && mode != MOFA_SPARSE_LAST) return MOFA_EINVAL;
    if ((long long)H * W > 0x7fffffffLL || (K > 0 && (!pos || !val))) return MOFA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, (size_t)n * 4 * H * W * sizeof(float), st) != hipSuccess) return MOFA_ELAUNCH;
    if (K == 0) return MOFA_OK;
    hipLaunchKernelGGL(sparse_points_kernel, dim3((K + 255) / 256, n), dim3(256), 0, st, pos, val, out, K, H, W, mode);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

struct FinishArgs {
    const float* flow_in;
    const float* flow_out;
    const unsigned char* brush;
    float* out;
    long long items;                 // n * H * ceil(W / 4)
    int hs, ws, H, W;
    float sy, sx;                    // nearest scales hs / H, ws / W
    float fy, fx;                    // flow rescale H / hs, W / ws
    int scaled, vec_load, vec_store;
};

__global__ __launch_bounds__(256) void flow_finish_kernel(const FinishArgs a) {
    const int W4 = (a.W + 3) / 4;
    const size_t src_hw = (size_t)a.hs * a.ws, dst_hw = (size_t)a.H * a.W;
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    if (it >= a.items) return;
    {
        const int x0 = (int)(it % W4) * 4;
        const long long r = it / W4;
        const int y = (int)(r % a.H);
        const long long i = r / a.H;
        const int iy = nearest_src(y, a.sy, a.hs);
        int ix[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ix[e] = nearest_src(x0 + e < a.W ? x0 + e : a.W - 1, a.sx, a.ws);
        const size_t row = (size_t)iy * a.ws;
        // a contiguous, 16-byte aligned run of four sources (the equal-size case): one load per plane
        const bool run = a.vec_load && ix[3] == ix[0] + 3 && ix[1] == ix[0] + 1 && ix[2] == ix[0] + 2 && (ix[0] & 3) == 0;
        float av[2][4], bv[2][4];
        unsigned char br[4] = {255, 255, 255, 255};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const size_t plane = ((size_t)i * 2 + c) * src_hw + row;
            if (run) {
                const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                const f32x4 va = a.flow_in ? *(const f32x4*)(a.flow_in + plane + ix[0]) : z;
                const f32x4 vb = a.flow_out ? *(const f32x4*)(a.flow_out + plane + ix[0]) : z;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    av[c][e] = va[e];
                    bv[c][e] = vb[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    av[c][e] = a.flow_in ? a.flow_in[plane + ix[e]] : 0.0f;
                    bv[c][e] = a.flow_out ? a.flow_out[plane + ix[e]] : 0.0f;
                }
            }
        }
        const bool has_brush = a.brush != nullptr && a.flow_in != nullptr;
        if (has_brush) {
#pragma unroll
            for (int e = 0; e < 4; ++e) br[e] = a.brush[row + ix[e]];
        }
        f32x4 ox, oy;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float px, py;
            control_finish_pixel(av[0][e], av[1][e], bv[0][e], bv[1][e], has_brush, br[e], a.scaled != 0, a.fx, a.fy, px, py);
            ox[e] = px;
            oy[e] = py;
        }
        float* dx = a.out + ((size_t)i * 2) * dst_hw + (size_t)y * a.W + x0;
        float* dy = dx + dst_hw;
        if (a.vec_store) {                                   // W % 4 == 0 and out 16-byte aligned: every run is whole and aligned
            *(f32x4*)dx = ox;
            *(f32x4*)dy = oy;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x0 + e < a.W) {
                    dx[e] = ox[e];
                    dy[e] = oy[e];
                }
        }
    }
}

extern "C" int mofa_flow_finish_f32(const float* flow_in, const float* flow_out, const unsigned char* brush, int n, int hs, int ws,
                                    int H, int W, float* out, mofa_stream_t stream) {
    if (!out || n <= 0 || hs <= 0 || ws <= 0 || H <= 0 || W <= 0) return MOFA_EINVAL;
    if ((long long)H * W > 0x7fffffffLL || (long long)hs * ws > 0x7fffffffLL) return MOFA_EINVAL;
    FinishArgs a;
    a.flow_in = flow_in;
    a.flow_out = flow_out;
    a.brush = brush;
    a.out = out;
    a.items = (long long)n * H * ((W + 3) / 4);
    a.hs = hs, a.ws = ws, a.H = H, a.W = W;
    a.sy = (float)hs / (float)H;                             // resize_nearest_kernel's scales
    a.sx = (float)ws / (float)W;
    a.scaled = (H != hs || W != ws) ? 1 : 0;
    a.fy = (float)((double)H / (double)hs);
    a.fx = (float)((double)W / (double)ws);
    a.vec_load = (ws % 4 == 0 && ((uintptr_t)flow_in & 15) == 0 && ((uintptr_t)flow_out & 15) == 0) ? 1 : 0;
    a.vec_store = (W % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    const long long nb = (a.items + 255) / 256;
    if (nb > 0x7fffffffLL) return MOFA_EINVAL;
    hipLaunchKernelGGL(flow_finish_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, a);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}
