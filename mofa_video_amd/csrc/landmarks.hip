// Landmark pose images: what mofa_video_amd/landmarks.py's pose_images computes on the host -- draw_landmarks
// (the restated cv2.line(thickness = 2) over the 15 polylines of a 68-point face, on a draw_size x draw_size canvas), the
// cv2.resize(INTER_LINEAR) of the float64 canvas to the clip size, and / 255 -- bit for bit, from int32 landmark coordinates.
//   * pose_raster: one wave per frame, one lane per segment.  Each lane runs the literal serial rasteriser of
//     landmarks_raster.h for its segment and combines into an int32 canvas with atomicMax of (segment number + 1): a pixel's
//     colour is that of the highest-numbered segment covering it, whatever the order the lanes arrive in.
//   * pose_resize: one thread per output pixel; computes its own taps as numpy does (position in double, rounded to fp32),
//     reads four canvas entries, looks the colours up and blends in double -- each product and each sum rounded on its own
//     (contraction off), horizontal pair first, then the vertical pair, then fp32 and a correctly rounded / 255.
#include "common.h"
#include "landmarks_raster.h"

struct CanvasMax {
    int* canvas;
    int w, h, value;
    __device__ void operator()(int x, int y) const {
        if ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) atomicMax(canvas + (size_t)y * w + x, value);
    }
};

__global__ __launch_bounds__(64) void pose_raster_kernel(const int32_t* __restrict__ pts, int* __restrict__ canvas, const int size) {
    const int n = blockIdx.x, s = threadIdx.x;
    if (s >= POSE_SEGMENTS) return;
    CanvasMax plot{canvas + (size_t)n * size * size, size, size, s + 1};
    pose_draw_segment(size, size, pts + (size_t)n * POSE_POINTS * 2, s, plot);
}

// landmarks.resize_linear's taps(): source index s0 (s1 = min(s0 + 1, ssize - 1)) and the weights (1 - f, f) in double
__device__ __forceinline__ void pose_tap(const int d, const double scale, const int ssize, int& s0, int& s1, double& w0, double& w1) {
#pragma clang fp contract(off)
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= ssize - 1) { f = 0.0f; s = ssize - 1; }
    s0 = s;
    s1 = s + 1 < ssize - 1 ? s + 1 : ssize - 1;
    w0 = (double)(1.0f - f);
    w1 = (double)f;
}

__global__ __launch_bounds__(256) void pose_resize_kernel(const int* __restrict__ canvas, float* __restrict__ out, const long long npix,
                                                          const int H, const int W, const int size) {
#pragma clang fp contract(off)
    __shared__ float colour[POSE_SEGMENTS + 1][3];           // canvas value -> colour; 0 = background
    if (threadIdx.x <= POSE_SEGMENTS) {
        int a = 0, b = 0, part = 0;
        if (threadIdx.x > 0) pose_segment(threadIdx.x - 1, a, b, part);
#pragma unroll
        for (int c = 0; c < 3; ++c) colour[threadIdx.x][c] = threadIdx.x > 0 ? (float)pose_part_colour(part, c) : 0.0f;
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // over N * H * W
    if (i >= npix) return;
    const long long hw = (long long)H * W;
    const long long n = i / hw;
    const int p = (int)(i - n * hw), y = p / W, x = p - y * W;
    int x0, x1, y0, y1;
    double ax0, ax1, by0, by1;
    pose_tap(x, (double)size / (double)W, size, x0, x1, ax0, ax1);
    pose_tap(y, (double)size / (double)H, size, y0, y1, by0, by1);
    const int* cv = canvas + n * size * size;
    const int i00 = cv[y0 * size + x0], i01 = cv[y0 * size + x1], i10 = cv[y1 * size + x0], i11 = cv[y1 * size + x1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double r0 = (double)colour[i00][c] * ax0 + (double)colour[i01][c] * ax1;
        const double r1 = (double)colour[i10][c] * ax0 + (double)colour[i11][c] * ax1;
        const double v = r0 * by0 + r1 * by1;
        out[(n * 3 + c) * hw + p] = __fdiv_rn((float)v, 255.0f);
    }
}

extern "C" int mofa_pose_images_f32(const int32_t* pts, float* out, void* workspace, int N, int H, int W, int draw_size,
                                    mofa_stream_t stream) {
    if (!pts || !out || !workspace || N <= 0 || H <= 0 || W <= 0 || draw_size <= 0 || draw_size > 4096) return MOFA_EINVAL;
    const long long npix = (long long)N * H * W;
    if (((uintptr_t)workspace & 15) != 0 || (long long)H * W > 0x7fffffffLL || npix > 0x7fffffffLL * 256) return MOFA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int* canvas = (int*)workspace;
    if (hipMemsetAsync(canvas, 0, (size_t)N * draw_size * draw_size * sizeof(int), st) != hipSuccess) return MOFA_ELAUNCH;
    hipLaunchKernelGGL(pose_raster_kernel, dim3(N), dim3(64), 0, st, pts, canvas, draw_size);
    hipLaunchKernelGGL(pose_resize_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, (const int*)canvas, out, npix, H, W,
                       draw_size);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}
