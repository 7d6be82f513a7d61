// Forward splatting ("softsplat", mode 'avg') for the MOFA-Adapter warp.
//
// Reference semantics: MOFA-Video-Traj/models/softsplat.py:232-274 (append ones channel, splat, divide by
// splatted ones + 1e-7) and the CUDA kernel softsplat_out at :284-345 (every source pixel scatters to its
// 4 bilinear neighbours with fp32 atomicAdd; a non-finite target skips the pixel; each corner is bounds
// checked separately).
//
// mofa_softsplat_avg_f16 -- deterministic GATHER form.  The (target, weight) pairs depend only on the flow,
// not on the channel, so per flow frame we build once a CSR "target -> (corner*HW + source, weight)" and then
// every target row gathers its sources across all C channels with 16-byte loads along the channel axis
// (the feature map is token-major: one source = one contiguous C-vector).  The contributions of a target are
// summed in (corner, source-raster) order -- the same order as the CPU oracle -- so the result is
// run-to-run reproducible (the reference's atomicAdd order is not).  The ones-channel and the final division
// are fused: norm = sum of weights.
//
// mofa_softsplat_scatter_f32 -- the literal scatter/atomicAdd form on NCHW fp32 (for parity classing and as
// the baseline the gather form is measured against).
#include "common.h"

struct Corners {
    int t[4];
    float w[4];
};

// floor of a finite coordinate, kept within +-2^30: converting a float beyond the int range to int is undefined, and so is
// x0 + 1 at INT_MAX.  A plane has fewer than 2^29 pixels, so every corner of such a source is out of bounds before and after
// the clamp, and no coordinate within +-2^30 changes.
__device__ __forceinline__ float ss_floor(float f) { return fminf(fmaxf(floorf(f), -1073741824.0f), 1073741824.0f); }

// softsplat.py:298-334
__device__ __forceinline__ bool splat_corners(const float* __restrict__ flow, int s, int H, int W, Corners& c) {
    const int HW = H * W;
    const int y = s / W, x = s - y * W;
    const float fx = (float)x + flow[s];
    const float fy = (float)y + flow[HW + s];
    if (!isfinite(fx) || !isfinite(fy)) return false;
    const float flx = ss_floor(fx), fly = ss_floor(fy);
    const int x0 = (int)flx, y0 = (int)fly;
    const float x1f = (float)(x0 + 1), y1f = (float)(y0 + 1), x0f = (float)x0, y0f = (float)y0;
    c.w[0] = (x1f - fx) * (y1f - fy);  // NW
    c.w[1] = (fx - x0f) * (y1f - fy);  // NE
    c.w[2] = (x1f - fx) * (fy - y0f);  // SW
    c.w[3] = (fx - x0f) * (fy - y0f);  // SE
    const int cx[4] = {x0, x0 + 1, x0, x0 + 1};
    const int cy[4] = {y0, y0, y0 + 1, y0 + 1};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        c.t[k] = (cx[k] >= 0 && cx[k] < W && cy[k] >= 0 && cy[k] < H) ? cy[k] * W + cx[k] : -1;
    return true;
}

// workspace per flow frame: count[HW] | offset[HW+1] | cursor[HW] | keys[4HW] | wts[4HW]
static inline int64_t ws_ints_per_flow(int64_t HW) { return HW * 3 + 1 + HW * 8; }
extern "C" int64_t mofa_softsplat_ws_bytes(int nflows, int H, int W) {
    return ws_ints_per_flow((int64_t)H * W) * 4 * (int64_t)nflows + 64;
}

// one image plane holds fewer than 2^29 pixels: the CSR keys corner * HW + source are int
static bool ss_plane_ok(int H, int W) { return H > 0 && W > 0 && (int64_t)H * W < (1LL << 29); }

__global__ void ss_count_kernel(const float* __restrict__ flow, int* __restrict__ ws, int H, int W, long long per) {
    const int HW = H * W, i = blockIdx.y;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= HW) return;
    Corners c;
    if (!splat_corners(flow + (size_t)i * 2 * HW, s, H, W, c)) return;
    int* count = ws + per * i;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (c.t[k] >= 0) atomicAdd(&count[c.t[k]], 1);
}

// exclusive scan of count[HW] -> offset[HW+1]; one 1024-thread block per flow frame
__global__ __launch_bounds__(1024) void ss_scan_kernel(int* __restrict__ ws, int HW, long long per) {
    __shared__ int sums[1024];
    int* count = ws + per * blockIdx.x;
    int* offset = count + HW;
    const int tid = threadIdx.x;
    const int seg = (HW + 1023) / 1024;
    const int a = tid * seg;
    int b = a + seg;
    b = b < HW ? b : HW;
    int local = 0;
    for (int j = a; j < b; ++j) local += count[j];
    sums[tid] = local;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = (tid >= o) ? sums[tid - o] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    int run = sums[tid] - local;
    for (int j = a; j < b; ++j) {
        offset[j] = run;
        run += count[j];
    }
    if (tid == 1023) offset[HW] = sums[1023];
}

__global__ void ss_fill_kernel(const float* __restrict__ flow, int* __restrict__ ws, int H, int W, long long per) {
    const int HW = H * W, i = blockIdx.y;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= HW) return;
    Corners c;
    if (!splat_corners(flow + (size_t)i * 2 * HW, s, H, W, c)) return;
    int* base = ws + per * i;
    const int* offset = base + HW;
    int* cursor = base + 2 * HW + 1;
    int* keys = base + 3 * HW + 1;
    float* wts = (float*)(base + 3 * HW + 1 + 4 * HW);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (c.t[k] >= 0) {
            const int pos = offset[c.t[k]] + atomicAdd(&cursor[c.t[k]], 1);
            keys[pos] = k * HW + s;
            wts[pos] = c.w[k];
        }
}

// order every target's segment by key = corner*HW + source (keys are distinct).  Segments are short for real flows (a
// handful of sources per pixel): insertion sort.  A strongly convergent flow can put up to 4 HW entries on one pixel, where
// the quadratic sort of one thread would run for seconds -- beyond SS_INSERTION_MAX entries the segment is heap-sorted in
// place instead (O(n log n): 36 864 entries ~ 1 M steps).  Same result either way (a total order on distinct keys).
#define SS_INSERTION_MAX 48
__device__ __forceinline__ void ss_sift_down(int* keys, float* wts, int root, int n) {
    const int kr = keys[root];
    const float wr = wts[root];
    int hole = root;
    for (;;) {
        int child = 2 * hole + 1;
        if (child >= n) break;
        if (child + 1 < n && keys[child + 1] > keys[child]) ++child;
        if (keys[child] <= kr) break;
        keys[hole] = keys[child];
        wts[hole] = wts[child];
        hole = child;
    }
    keys[hole] = kr;
    wts[hole] = wr;
}
__global__ void ss_sort_kernel(int* __restrict__ ws, int HW, long long per) {
    const int i = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= HW) return;
    int* base = ws + per * i;
    const int* offset = base + HW;
    int* keys = base + 3 * HW + 1;
    float* wts = (float*)(base + 3 * HW + 1 + 4 * HW);
    const int a = offset[t], b = offset[t + 1];
    if (b - a <= SS_INSERTION_MAX) {
        for (int j = a + 1; j < b; ++j) {
            const int kj = keys[j];
            const float wj = wts[j];
            int m = j - 1;
            while (m >= a && keys[m] > kj) {
                keys[m + 1] = keys[m];
                wts[m + 1] = wts[m];
                --m;
            }
            keys[m + 1] = kj;
            wts[m + 1] = wj;
        }
    } else {
        int* k = keys + a;
        float* w = wts + a;
        const int n = b - a;
        for (int r = n / 2 - 1; r >= 0; --r) ss_sift_down(k, w, r, n);
        for (int end = n - 1; end > 0; --end) {
            const int kt = k[0]; k[0] = k[end]; k[end] = kt;
            const float wt = w[0]; w[0] = w[end]; w[end] = wt;
            ss_sift_down(k, w, 0, end);
        }
    }
}

// one wave per target pixel; lanes span the channel vectors
__global__ __launch_bounds__(256) void ss_gather_kernel(const f16* __restrict__ feat, const int* __restrict__ ws,
                                                        f16* __restrict__ out, int HW, int C, int ldf, int ldo,
                                                        long long per) {
    const int i = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 4 + wave;
    if (t >= HW) return;
    const int* base = ws + per * i;
    const int* offset = base + HW;
    const int* keys = base + 3 * HW + 1;
    const float* wts = (const float*)(base + 3 * HW + 1 + 4 * HW);
    const int a = offset[t], b = offset[t + 1];
    const int CV = C >> 3;
    float norm = 0.f;
    for (int j = a; j < b; ++j) norm += wts[j];
    const float inv = 1.0f / (norm + 0.0000001f);
    f16* op = out + ((size_t)i * HW + t) * ldo;
    for (int cv = lane; cv < CV; cv += 64) {
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int j = a; j < b; ++j) {
            const int src = keys[j] % HW;
            const float w = wts[j];
            const f16x8 v = *(const f16x8*)(feat + (size_t)src * ldf + cv * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)v[e] * w;
        }
        f16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (f16)(acc[e] * inv);
        *(f16x8*)(op + cv * 8) = o;
    }
}

// the per-flow CSR "target -> sorted (key, weight)" in ws (count, scan, fill, sort)
static void ss_launch_sort_wg(int* ws, const float* flow, int nflows, int H, int W, long long per, hipStream_t st);
static int ss_build_csr(const float* flow, void* ws, int nflows, int H, int W, hipStream_t st, bool wg_sort = false) {
    const int HW = H * W;
    const long long per = ws_ints_per_flow(HW);
    if (hipMemsetAsync(ws, 0, (size_t)per * 4 * nflows, st) != hipSuccess) return MOFA_ELAUNCH;
    dim3 gpix(cdiv(HW, 256), nflows);
    hipLaunchKernelGGL(ss_count_kernel, gpix, dim3(256), 0, st, flow, (int*)ws, H, W, per);
    hipLaunchKernelGGL(ss_scan_kernel, dim3(nflows), dim3(1024), 0, st, (int*)ws, HW, per);
    hipLaunchKernelGGL(ss_fill_kernel, gpix, dim3(256), 0, st, flow, (int*)ws, H, W, per);
    if (wg_sort) ss_launch_sort_wg((int*)ws, flow, nflows, H, W, per, st);
    else hipLaunchKernelGGL(ss_sort_kernel, gpix, dim3(256), 0, st, (int*)ws, HW, per);
    return MOFA_OK;
}

// the argument rules of mofa_softsplat_avg_f16 (include/mofa_hip.h), host arithmetic only: nflows is a grid dimension
static int ss_avg_check(const void* feat, const float* flow, const void* out, const void* ws, int nflows, int H, int W, int C,
                        int ldf, int ldo) {
    if (!feat || !flow || !out || !ws || nflows <= 0 || nflows > 65535 || !ss_plane_ok(H, W) || C <= 0 || C % 8 != 0 ||
        ldf % 8 != 0 || ldo % 8 != 0)
        return MOFA_EINVAL;
    return MOFA_OK;
}

extern "C" int mofa_softsplat_avg_f16(const void* feat, const float* flow, void* out, void* ws, int nflows, int H, int W,
                                      int C, int ldf, int ldo, mofa_stream_t stream) {
    if (ss_avg_check(feat, flow, out, ws, nflows, H, W, C, ldf, ldo) != MOFA_OK) return MOFA_EINVAL;
    const int HW = H * W;
    const long long per = ws_ints_per_flow(HW);
    hipStream_t st = (hipStream_t)stream;
    if (ss_build_csr(flow, ws, nflows, H, W, st) != MOFA_OK) return MOFA_ELAUNCH;
    hipLaunchKernelGGL(ss_gather_kernel, dim3(cdiv(HW, 4), nflows), dim3(256), 0, st, (const f16*)feat, (const int*)ws,
                       (f16*)out, HW, C, ldf, ldo, per);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

// literal form of the reference kernel (NCHW fp32, atomicAdd): out_sum must be zero-initialised by the caller
__global__ void ss_scatter_kernel(const float* __restrict__ in, const float* __restrict__ flow, float* __restrict__ out,
                                  long long total, int C, int H, int W) {
    const int HW = H * W;
    for (long long idx = (long long)blockIdx.x * 512 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 512) {
        const int s = (int)(idx % HW);
        const long long r = idx / HW;
        const int c = (int)(r % C);
        const int n = (int)(r / C);
        Corners cr;
        if (!splat_corners(flow + (size_t)n * 2 * HW, s, H, W, cr)) continue;
        const float v = in[idx];
        float* o = out + ((size_t)n * C + c) * HW;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cr.t[k] >= 0) atomicAdd(&o[cr.t[k]], v * cr.w[k]);
    }
}
extern "C" int mofa_softsplat_scatter_f32(const float* in, const float* flow, float* out_sum, int N, int C, int H, int W,
                                          mofa_stream_t stream) {
    if (!in || !flow || !out_sum || N <= 0 || C <= 0 || H <= 0 || W <= 0) return MOFA_EINVAL;
    const long long total = (long long)N * C * H * W;
    long long nb = (total + 511) / 512;
    nb = nb > 65535 ? 65535 : nb;
    hipLaunchKernelGGL(ss_scatter_kernel, dim3((int)nb), dim3(512), 0, (hipStream_t)stream, in, flow, out_sum, total, C,
                       H, W);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

// ---- the metric-weighted modes of the reference wrapper (Traj/models/softsplat.py:243-270), off the inference path: 'linear' /
//      'soft' splat [in * w | w] with w = metric / exp(metric) and divide by the splatted last channel ------------------------------
__global__ __launch_bounds__(256) void splat_weight_kernel(const float* __restrict__ in, const float* __restrict__ metric,
                                                           float* __restrict__ out, int C, long long HW, long long total, int mode) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long p = i % HW, r = i / HW;               // r = n * (C + 1) + c
        const int c = (int)(r % (C + 1));
        const long long n = r / (C + 1);
        float w = metric[n * HW + p];
        if (mode == 2) w = expf(w);
        out[i] = c < C ? in[(n * C + c) * HW + p] * w : w;
    }
}
extern "C" int mofa_softsplat_weight_f32(const float* in, const float* metric, float* out, int N, int C, int H, int W, int mode,
                                         mofa_stream_t stream) {
    if (!in || !metric || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0 || (mode != 1 && mode != 2)) return MOFA_EINVAL;
    const long long HW = (long long)H * W, total = (long long)N * (C + 1) * HW;
    long long nb = (total + 255) / 256;
    nb = nb > 16384 ? 16384 : nb;
    hipLaunchKernelGGL(splat_weight_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, in, metric, out, C, HW, total, mode);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

// out[n][c] = summed[n][c] / norm(summed[n][C]); eps_mode 0: + 1e-7 ('' / 'addeps'), 1: 0 -> 1 ('zeroeps'), 2: max(., 1e-7)
// ('clipeps'), 3: as it is (any other suffix: the reference leaves the channel untouched)
__global__ __launch_bounds__(256) void splat_normalize_kernel(const float* __restrict__ summed, float* __restrict__ out, int C,
                                                              long long HW, long long total, int eps_mode) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long p = i % HW, r = i / HW;               // r = n * C + c
        const int c = (int)(r % C);
        const long long n = r / C;
        float d = summed[(n * (C + 1) + C) * HW + p];
        if (eps_mode == 0) d = d + 0.0000001f;
        else if (eps_mode == 1) d = d == 0.0f ? 1.0f : d;
        else if (eps_mode == 2) d = fmaxf(d, 0.0000001f);
        out[i] = summed[(n * (C + 1) + c) * HW + p] / d;
    }
}
extern "C" int mofa_softsplat_normalize_f32(const float* summed, float* out, int N, int C, int H, int W, int eps_mode,
                                            mofa_stream_t stream) {
    if (!summed || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0 || eps_mode < 0 || eps_mode > 3) return MOFA_EINVAL;
    const long long HW = (long long)H * W, total = (long long)N * C * HW;
    long long nb = (total + 255) / 256;
    nb = nb > 16384 ? 16384 : nb;
    hipLaunchKernelGGL(splat_normalize_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, summed, out, C, HW, total, eps_mode);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

// ---- backward: softsplat_func.backward (softsplat_ingrad :368-435, softsplat_flowgrad :439-524) through the wrapper's mode prep
//      and normalisation (:243-270).  No atomics: every sum runs in a fixed order, so the gradients are reproducible bit for bit.
//      Element offsets are 64-bit; one image plane must hold fewer than 2^29 pixels (the CSR keys corner * HW + source are int).

// 'avg' normaliser before its + 1e-7: the per-target sum of splat weights in ss_gather_kernel's CSR order (bit-identical)
__global__ void ss_norm_kernel(const int* __restrict__ ws, float* __restrict__ norm, int HW, long long per) {
    const int i = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= HW) return;
    const int* base = ws + per * i;
    const int* offset = base + HW;
    const float* wts = (const float*)(base + 3 * HW + 1 + 4 * HW);
    const int a = offset[t], b = offset[t + 1];
    float s = 0.f;
    for (int j = a; j < b; ++j) s += wts[j];
    norm[(size_t)i * HW + t] = s;
}

extern "C" int mofa_softsplat_norm_f32(const float* flow, float* norm, void* ws, int N, int H, int W, mofa_stream_t stream) {
    if (!flow || !norm || !ws || N <= 0 || N > 65535 || !ss_plane_ok(H, W)) return MOFA_EINVAL;
    const int HW = H * W;
    hipStream_t st = (hipStream_t)stream;
    if (ss_build_csr(flow, ws, N, H, W, st) != MOFA_OK) return MOFA_ELAUNCH;
    hipLaunchKernelGGL(ss_norm_kernel, dim3(cdiv(HW, 256), N), dim3(256), 0, st, (const int*)ws, norm, HW, ws_ints_per_flow(HW));
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

// per target: nu = n(norm) as splat_normalize_kernel forms it, inv = 1 / nu, glast = -n'(norm) * sum_c grad_c * out_c / nu.
// 64 targets per block, the channels strided over the block's waves; the wave sums are added in wave order.
#define SSG_PRO_WAVES 8
__global__ __launch_bounds__(64 * SSG_PRO_WAVES) void ss_grad_prologue_kernel(const float* __restrict__ grad, const float* __restrict__ out,
                                                                             const float* __restrict__ norm, float* __restrict__ inv,
                                                                             float* __restrict__ glast, int C, int HW, int eps_mode) {
    __shared__ float part[SSG_PRO_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const int p = blockIdx.x * 64 + lane;
    float dot = 0.f;
    if (p < HW) {
        const float* g = grad + (size_t)n * C * HW + p;
        const float* o = out + (size_t)n * C * HW + p;
        for (int c = wave; c < C; c += SSG_PRO_WAVES) dot = fmaf(g[(size_t)c * HW], o[(size_t)c * HW], dot);
    }
    part[wave][lane] = dot;
    __syncthreads();
    if (wave != 0 || p >= HW) return;
    float d = part[0][lane];
#pragma unroll
    for (int w = 1; w < SSG_PRO_WAVES; ++w) d += part[w][lane];
    const float s = norm[(size_t)n * HW + p];
    float nu = s;
    bool live = true;                         // n'(s) = 1; 0 where 'zeroeps' replaced a zero or 'clipeps' clamped
    if (eps_mode == 0) nu = s + 0.0000001f;
    else if (eps_mode == 1) { live = s != 0.0f; nu = live ? s : 1.0f; }
    else if (eps_mode == 2) { live = s >= 0.0000001f; nu = fmaxf(s, 0.0000001f); }
    const float r = 1.0f / nu;
    inv[(size_t)n * HW + p] = r;
    glast[(size_t)n * HW + p] = live ? -(d * r) : 0.0f;
}

extern "C" int mofa_softsplat_grad_prologue_f32(const float* grad, const float* out, const float* norm, float* inv, float* glast,
                                                int N, int C, int H, int W, int eps_mode, mofa_stream_t stream) {
    if (!grad || !out || !norm || !inv || !glast || N <= 0 || N > 65535 || C <= 0 || !ss_plane_ok(H, W) || eps_mode < 0 ||
        eps_mode > 3)
        return MOFA_EINVAL;
    const int HW = H * W;
    hipLaunchKernelGGL(ss_grad_prologue_kernel, dim3(cdiv(HW, 64), N), dim3(64 * SSG_PRO_WAVES), 0, (hipStream_t)stream, grad, out, norm,
                       inv, glast, C, HW, eps_mode);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

// splat_corners plus the weights' derivatives in x and y with the floor held fixed (softsplat_flowgrad :477-488)
__device__ __forceinline__ bool splat_corners_grad(const float* __restrict__ flow, int s, int H, int W, Corners& c, float dx[4],
                                                   float dy[4]) {
    if (!splat_corners(flow, s, H, W, c)) return false;
    const int y = s / W, x = s - y * W;
    const float fx = (float)x + flow[s];
    const float fy = (float)y + flow[H * W + s];
    const float x0f = ss_floor(fx), y0f = ss_floor(fy);
    const float x1f = (float)((int)x0f + 1), y1f = (float)((int)y0f + 1);
    dx[0] = -(y1f - fy); dx[1] = y1f - fy; dx[2] = -(fy - y0f); dx[3] = fy - y0f;
    dy[0] = -(x1f - fx); dy[1] = -(fx - x0f); dy[2] = x1f - fx; dy[3] = fx - x0f;
    return true;
}
__device__ __forceinline__ bool ss_source_live(const float* __restrict__ flow, int s, int W, int HW) {
    const int y = s / W, x = s - y * W;
    return isfinite((float)x + flow[s]) && isfinite((float)y + flow[HW + s]);
}
// the mode prep's factor a: Ĩ = [I * a | a] ('avg': 1, 'linear': m, 'soft': e^m); 1 without prep
__device__ __forceinline__ float ss_prep_factor(const float* __restrict__ metric, int prep, size_t i) {
    return prep == 2 ? metric[i] : prep == 3 ? expf(metric[i]) : 1.0f;
}
__device__ __forceinline__ void ss_grad_store(const mofa_softsplat_grad_args& a, int n, int q, int HW, float sx, float sy, float sm) {
    const bool live = ss_source_live(a.flow + (size_t)n * 2 * HW, q, a.W, HW);
    const float f = live ? ss_prep_factor(a.metric, a.prep, (size_t)n * HW + q) : 0.0f;
    if (a.grad_flow) {
        a.grad_flow[((size_t)n * 2) * HW + q] = live ? f * sx : 0.0f;
        a.grad_flow[((size_t)n * 2 + 1) * HW + q] = live ? f * sy : 0.0f;
    }
    if (a.grad_metric) a.grad_metric[(size_t)n * HW + q] = live ? (a.prep == 3 ? f * sm : sm) : 0.0f;
}

// One source pixel per lane, 64 per block, the splatted channels [c0, c1) of this block's slice strided over its waves.  Per
// channel c: G_c = sum_k w_k ghat_c(t_k), D_c = sum_k dw_k ghat_c(t_k) (x and y), grad_in_c = a G_c; the flow / metric sums
// sum_c Ĩ_c / a * (D_c, G_c) are added over the wave's channels in order, then over the waves in order (LDS), then -- with
// slices > 1 -- over the slices in order by ss_grad_reduce_kernel.
#define SSG_WAVES 4
__global__ __launch_bounds__(64 * SSG_WAVES) void ss_grad_kernel(const mofa_softsplat_grad_args a, int chunk) {
    __shared__ float red[3][SSG_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = blockIdx.y, n = blockIdx.z;
    const int HW = a.H * a.W, C = a.C;
    const int q = blockIdx.x * 64 + lane;
    const bool normed = a.inv != nullptr;
    const int Cs = C + (a.prep > 0);          // splatted channels
    const int Cg = Cs - (normed ? 1 : 0);     // channels of grad; with normed, channel Cg is the normaliser
    const bool sums = a.grad_flow || a.grad_metric;
    const int c0 = slice * chunk, c1 = min(c0 + chunk, Cs);
    float sx = 0.f, sy = 0.f, sm = 0.f;
    if (q < HW) {
        Corners cr;
        float dx[4], dy[4];
        const bool live = splat_corners_grad(a.flow + (size_t)n * 2 * HW, q, a.H, a.W, cr, dx, dy);
        const float f = live ? ss_prep_factor(a.metric, a.prep, (size_t)n * HW + q) : 0.0f;
        float cw[4], cx[4], cy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!live) cr.t[k] = -1;
            const float r = (normed && cr.t[k] >= 0) ? a.inv[(size_t)n * HW + cr.t[k]] : 1.0f;
            cw[k] = cr.w[k] * r;
            cx[k] = dx[k] * r;
            cy[k] = dy[k] * r;
        }
        const float* g = a.grad + (size_t)n * Cg * HW;
        const float* in = a.in + (size_t)n * C * HW + q;
        float* gi = a.grad_in ? a.grad_in + (size_t)n * C * HW + q : nullptr;
        for (int c = c0 + wave; c < min(c1, Cg); c += SSG_WAVES) {
            const float* gc = g + (size_t)c * HW;
            float G = 0.f, Dx = 0.f, Dy = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (cr.t[k] >= 0) {
                    const float v = gc[cr.t[k]];
                    G = fmaf(cw[k], v, G);
                    Dx = fmaf(cx[k], v, Dx);
                    Dy = fmaf(cy[k], v, Dy);
                }
            if (gi) gi[(size_t)c * HW] = f * G;
            if (sums && live) {
                const float v = in[(size_t)c * HW];
                sx = fmaf(v, Dx, sx);
                sy = fmaf(v, Dy, sy);
                sm = fmaf(v, G, sm);
            }
        }
        // the normaliser channel: ghat = glast at the corners, unscaled weights; Ĩ / a = I_Cg ('avg-<suffix>') or 1
        if (normed && Cg >= c0 && Cg < c1 && (Cg - c0) % SSG_WAVES == wave) {
            float G = 0.f, Dx = 0.f, Dy = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (cr.t[k] >= 0) {
                    const float v = a.glast[(size_t)n * HW + cr.t[k]];
                    G = fmaf(cr.w[k], v, G);
                    Dx = fmaf(dx[k], v, Dx);
                    Dy = fmaf(dy[k], v, Dy);
                }
            if (Cg < C && gi) gi[(size_t)Cg * HW] = f * G;
            if (sums && live) {
                const float v = Cg < C ? in[(size_t)Cg * HW] : 1.0f;
                sx = fmaf(v, Dx, sx);
                sy = fmaf(v, Dy, sy);
                sm = fmaf(v, G, sm);
            }
        }
    }
    if (!sums) return;
    red[0][wave][lane] = sx;
    red[1][wave][lane] = sy;
    red[2][wave][lane] = sm;
    __syncthreads();
    if (wave != 0 || q >= HW) return;
#pragma unroll
    for (int w = 1; w < SSG_WAVES; ++w) {
        sx += red[0][w][lane];
        sy += red[1][w][lane];
        sm += red[2][w][lane];
    }
    if (gridDim.y == 1) {
        ss_grad_store(a, n, q, HW, sx, sy, sm);
    } else {
        float* p = a.partial + (((size_t)slice * gridDim.z + n) * 3) * HW + q;
        p[0] = sx;
        p[HW] = sy;
        p[2 * (size_t)HW] = sm;
    }
}

__global__ __launch_bounds__(256) void ss_grad_reduce_kernel(const mofa_softsplat_grad_args a) {
    const int HW = a.H * a.W, n = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= HW) return;
    float sx = 0.f, sy = 0.f, sm = 0.f;
    for (int s = 0; s < a.slices; ++s) {
        const float* p = a.partial + (((size_t)s * a.N + n) * 3) * HW + q;
        sx += p[0];
        sy += p[HW];
        sm += p[2 * (size_t)HW];
    }
    ss_grad_store(a, n, q, HW, sx, sy, sm);
}

extern "C" int mofa_softsplat_grad_f32(const mofa_softsplat_grad_args* a, mofa_stream_t stream) {
    if (!a || !a->grad || !a->flow || a->N <= 0 || a->N > 65535 || a->C <= 0 || !ss_plane_ok(a->H, a->W) || a->prep < 0 || a->prep > 3)
        return MOFA_EINVAL;
    if (a->reserved[0] || a->reserved[1] || a->reserved[2] || a->reserved[3]) return MOFA_EINVAL;
    const bool normed = a->inv != nullptr;
    const int Cs = a->C + (a->prep > 0);
    if (normed != (a->glast != nullptr) || (a->prep > 0 && !normed) || Cs - (normed ? 1 : 0) <= 0) return MOFA_EINVAL;
    if ((a->prep >= 2) != (a->metric != nullptr) || (a->grad_metric && a->prep < 2)) return MOFA_EINVAL;
    const bool sums = a->grad_flow || a->grad_metric;
    if ((!a->grad_in && !sums) || (sums && !a->in) || a->slices < 1 || a->slices > Cs || a->slices > 65535 ||
        (sums && a->slices > 1 && !a->partial))
        return MOFA_EINVAL;
    const int HW = a->H * a->W;
    const int chunk = (Cs + a->slices - 1) / a->slices;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ss_grad_kernel, dim3(cdiv(HW, 64), a->slices, a->N), dim3(64 * SSG_WAVES), 0, st, *a, chunk);
    if (sums && a->slices > 1)
        hipLaunchKernelGGL(ss_grad_reduce_kernel, dim3(cdiv(HW, 256), a->N), dim3(256), 0, st, *a);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

// ---- fp32 gather forward of every mode (mofa_softsplat_gather_f32): the splat of Ĩ = prep(I, m) as a per-target sum over the CSR,
//      fp32 NCHW in and out, the normalisation fused, no atomics on a value.  Per target the contributions are added in CSR order
//      (corners NW, NE, SW, SE; sources in raster order within a corner) as acc = acc + ((I * a) * w), every product and sum rounded
//      on its own -- the CPU oracle's index_add_ order and operations, so the raw sum equals it bit for bit.
#define SSF_WAVES 4
#define SSF_REG 8        // CSR entries of its segment a lane keeps in registers; the rest it re-reads per channel
#define SSF_LONG 128     // a longer segment is walked by the whole workgroup, one channel per thread

// ss_sort_kernel for the gather forward: the same order, but a segment of more than SSF_LONG entries is not left to one thread
// (a convergent flow puts up to 4 HW entries on a target: tens of milliseconds of serial heap sort).  Its keys are distinct
// integers below 4 HW, so the workgroup marks them in a bitmap in LDS, and the set bits in ascending order ARE the sorted keys;
// a key's position is the number of set bits below it, and its weight is recomputed from the flow (the same function that
// ss_fill_kernel called: the same bits).  Nothing depends on the order in which ss_fill_kernel's atomics arrived.
// Dynamic LDS: ceil(4 HW / 32) words; planes too large for it keep ss_sort_kernel (ss_wg_sort_fits).
static inline int ss_bitmap_words(int HW) { return (int)((4LL * HW + 31) / 32); }
static inline bool ss_wg_sort_fits(int HW) { return (ss_bitmap_words(HW) + 768) * 4LL <= 65536; }
__global__ __launch_bounds__(256) void ss_sort_wg_kernel(const float* __restrict__ flow, int* __restrict__ ws, int H, int W,
                                                         long long per, int words) {
    extern __shared__ unsigned ss_bits[];
    __shared__ int is_long[256];
    __shared__ int part[256];
    const int HW = H * W, i = blockIdx.y, tid = threadIdx.x;
    const int t = blockIdx.x * 256 + tid;
    int* base = ws + per * i;
    const int* offset = base + HW;
    int* keys = base + 3 * HW + 1;
    float* wts = (float*)(base + 3 * HW + 1 + 4 * HW);
    const float* fl = flow + (size_t)i * 2 * HW;
    int a = 0, b = 0;
    if (t < HW) {
        a = offset[t];
        b = offset[t + 1];
    }
    is_long[tid] = b - a > SSF_LONG;
    if (b - a <= SS_INSERTION_MAX) {
        for (int j = a + 1; j < b; ++j) {
            const int kj = keys[j];
            const float wj = wts[j];
            int m = j - 1;
            while (m >= a && keys[m] > kj) {
                keys[m + 1] = keys[m];
                wts[m + 1] = wts[m];
                --m;
            }
            keys[m + 1] = kj;
            wts[m + 1] = wj;
        }
    } else if (b - a <= SSF_LONG) {
        int* k = keys + a;
        float* w = wts + a;
        const int n = b - a;
        for (int r = n / 2 - 1; r >= 0; --r) ss_sift_down(k, w, r, n);
        for (int end = n - 1; end > 0; --end) {
            const int kt = k[0]; k[0] = k[end]; k[end] = kt;
            const float wt = w[0]; w[0] = w[end]; w[end] = wt;
            ss_sift_down(k, w, 0, end);
        }
    }
    __syncthreads();
    const int wpt = (words + 255) / 256;                       // bitmap words per thread, a contiguous run
    const int w0 = min(tid * wpt, words), w1 = min(w0 + wpt, words);
    for (int l = 0; l < 256; ++l) {
        if (!is_long[l]) continue;                             // (uniform: LDS)
        const int tl = blockIdx.x * 256 + l;
        const int la = offset[tl], lb = offset[tl + 1];
        for (int w = tid; w < words; w += 256) ss_bits[w] = 0u;
        __syncthreads();
        for (int j = la + tid; j < lb; j += 256) {
            const int key = keys[j];
            atomicOr(&ss_bits[key >> 5], 1u << (key & 31));
        }
        __syncthreads();
        int mine = 0;
        for (int w = w0; w < w1; ++w) mine += __popc(ss_bits[w]);
        part[tid] = mine;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int v = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        int pos = la + part[tid] - mine;
        for (int w = w0; w < w1; ++w) {
            unsigned word = ss_bits[w];
            while (word) {
                const int key = w * 32 + __ffs((int)word) - 1;
                word &= word - 1;
                const int k = (key >= HW) + (key >= 2 * HW) + (key >= 3 * HW);
                Corners c;
                splat_corners(fl, key - k * HW, H, W, c);
                keys[pos] = key;
                wts[pos] = k == 0 ? c.w[0] : k == 1 ? c.w[1] : k == 2 ? c.w[2] : c.w[3];
                ++pos;
            }
        }
        __syncthreads();
    }
}
static void ss_launch_sort_wg(int* ws, const float* flow, int nflows, int H, int W, long long per, hipStream_t st) {
    const int HW = H * W, words = ss_bitmap_words(HW);
    hipLaunchKernelGGL(ss_sort_wg_kernel, dim3(cdiv(HW, 256), nflows), dim3(256), (size_t)words * 4, st, flow, ws, H, W, per, words);
}

__device__ __forceinline__ int ss_key_source(int key, int HW) {      // key = corner * HW + source, corner 0..3
    if (key >= 2 * HW) key -= 2 * HW;
    return key >= HW ? key - HW : key;
}
__device__ __forceinline__ float ss_normaliser(float s, int eps_mode) {   // as splat_normalize_kernel forms it
    if (eps_mode == 0) return s + 0.0000001f;
    if (eps_mode == 1) return s == 0.0f ? 1.0f : s;
    if (eps_mode == 2) return fmaxf(s, 0.0000001f);
    return s;
}
// acc + ((v * f) * w), each product and the sum rounded on its own: the oracle's operations (a fused multiply-add is not)
__device__ __forceinline__ float ss_term(float acc, float v, float f, float w) {
#pragma clang fp contract(off)
    const float p = (v * f) * w;
    return acc + p;
}

// 64 consecutive targets per workgroup, one per lane; the output channels [c0, c1) of this workgroup's slice strided over its
// waves.  Every wave forms its targets' normaliser itself (one more channel), so neither waves nor slices depend on each other.
// Targets with more than SSF_LONG entries are left out of the lane phase and then taken one after the other by the whole
// workgroup: one channel per thread, the segment walked in the same order.
__global__ __launch_bounds__(64 * SSF_WAVES) void ss_gather_f32_kernel(const mofa_softsplat_gather_args a, int chunk, long long per) {
    __shared__ float long_norm;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = blockIdx.y, n = blockIdx.z;
    const int HW = a.H * a.W, C = a.C, prep = a.prep;
    const bool normed = a.normalize != 0;
    const int Co = C - ((normed && prep == 0) ? 1 : 0);      // channels of out; 'avg-<suffix>': the input's last one normalises
    const int c0 = slice * chunk, c1 = min(c0 + chunk, Co);
    const int* base = (const int*)a.ws + per * n;
    const int* offset = base + HW;
    const int* keys = base + 3 * HW + 1;
    const float* wts = (const float*)(base + 3 * HW + 1 + 4 * HW);
    const float* in = a.in + (size_t)n * C * HW;
    const float* metric = a.metric ? a.metric + (size_t)n * HW : nullptr;
    const float* nplane = prep == 0 ? in + (size_t)(C - 1) * HW : nullptr;   // the normaliser's own plane, if it has one
    float* out = a.out + (size_t)n * Co * HW;
    float* norm = (a.norm && slice == 0) ? a.norm + (size_t)n * HW : nullptr;
    const int t = blockIdx.x * 64 + lane;
    int ja = 0, jb = 0;
    if (t < HW) {
        ja = offset[t];
        jb = offset[t + 1];
    }
    const bool is_long = jb - ja > SSF_LONG;
    if (t < HW && !is_long) {
        int rs[SSF_REG];
        float rw[SSF_REG], rf[SSF_REG];
#pragma unroll
        for (int k = 0; k < SSF_REG; ++k) {
            const bool on = ja + k < jb;
            rs[k] = on ? ss_key_source(keys[ja + k], HW) : 0;
            rw[k] = on ? wts[ja + k] : 0.0f;
            rf[k] = on ? ss_prep_factor(metric, prep, rs[k]) : 0.0f;
        }
        float d = 1.0f;
        if (normed) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < SSF_REG; ++k)
                if (ja + k < jb) s = ss_term(s, nplane ? nplane[rs[k]] : 1.0f, rf[k], rw[k]);
            for (int j = ja + SSF_REG; j < jb; ++j) {
                const int src = ss_key_source(keys[j], HW);
                s = ss_term(s, nplane ? nplane[src] : 1.0f, ss_prep_factor(metric, prep, src), wts[j]);
            }
            if (norm && wave == 0) norm[t] = s;
            d = ss_normaliser(s, a.eps_mode);
        }
        for (int c = c0 + wave; c < c1; c += SSF_WAVES) {
            const float* plane = in + (size_t)c * HW;
            float v[SSF_REG];
#pragma unroll
            for (int k = 0; k < SSF_REG; ++k) v[k] = ja + k < jb ? plane[rs[k]] : 0.0f;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < SSF_REG; ++k)
                if (ja + k < jb) acc = ss_term(acc, v[k], rf[k], rw[k]);
            for (int j = ja + SSF_REG; j < jb; ++j) {
                const int src = ss_key_source(keys[j], HW);
                acc = ss_term(acc, plane[src], ss_prep_factor(metric, prep, src), wts[j]);
            }
            out[(size_t)c * HW + t] = normed ? acc / d : acc;
        }
    }
    // the long targets of this workgroup, in target order (the ballot is the same in every wave: they hold the same 64 targets)
    unsigned long long todo = __ballot(t < HW && is_long);
    const int items = (c1 - c0) + (normed ? 1 : 0);            // item c1 - c0 is the normaliser
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int tl = blockIdx.x * 64 + l;
        const int la = offset[tl], lb = offset[tl + 1];
        for (int i = threadIdx.x; i < items; i += 64 * SSF_WAVES) {
            const bool is_norm = i == c1 - c0;
            const float* plane = is_norm ? nplane : in + (size_t)(c0 + i) * HW;
            float acc = 0.0f;
#pragma unroll 4
            for (int j = la; j < lb; ++j) {
                const int src = ss_key_source(keys[j], HW);
                acc = ss_term(acc, plane ? plane[src] : 1.0f, ss_prep_factor(metric, prep, src), wts[j]);
            }
            if (is_norm) long_norm = acc;
            else out[(size_t)(c0 + i) * HW + tl] = acc;
        }
        if (normed) {                                          // (uniform: every thread of the workgroup walks the same `todo`)
            __syncthreads();
            const float s = long_norm;
            const float d = ss_normaliser(s, a.eps_mode);
            for (int i = threadIdx.x; i < c1 - c0; i += 64 * SSF_WAVES) {
                float* o = out + (size_t)(c0 + i) * HW + tl;   // this thread's own raw sum
                *o = *o / d;
            }
            if (norm && threadIdx.x == 0) norm[tl] = s;
            __syncthreads();
        }
    }
}

extern "C" int mofa_softsplat_gather_f32(const mofa_softsplat_gather_args* a, mofa_stream_t stream) {
    if (!a || !a->in || !a->flow || !a->out || !a->ws || a->N <= 0 || a->N > 65535 || a->C <= 0 || !ss_plane_ok(a->H, a->W))
        return MOFA_EINVAL;
    if (a->prep < 0 || a->prep > 3 || a->eps_mode < 0 || a->eps_mode > 3 || (a->normalize != 0 && a->normalize != 1)) return MOFA_EINVAL;
    if (a->reserved[0] || a->reserved[1] || a->reserved[2] || a->reserved[3]) return MOFA_EINVAL;
    if ((a->prep >= 2) != (a->metric != nullptr) || (a->prep >= 1 && !a->normalize) || (a->norm && !a->normalize)) return MOFA_EINVAL;
    const int Co = a->C - ((a->normalize && a->prep == 0) ? 1 : 0);
    if (Co <= 0 || a->slices < 1 || a->slices > Co || a->slices > 65535) return MOFA_EINVAL;
    const int HW = a->H * a->W;
    const int chunk = (Co + a->slices - 1) / a->slices;
    hipStream_t st = (hipStream_t)stream;
    if (ss_build_csr(a->flow, a->ws, a->N, a->H, a->W, st, ss_wg_sort_fits(HW)) != MOFA_OK) return MOFA_ELAUNCH;
    hipLaunchKernelGGL(ss_gather_f32_kernel, dim3(cdiv(HW, 64), a->slices, a->N), dim3(64 * SSF_WAVES), 0, st, *a, chunk,
                       (long long)ws_ints_per_flow(HW));
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}
