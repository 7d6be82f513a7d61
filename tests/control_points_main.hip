// Host execution of the shared decision logic of the control-signal kernels (mofa_video_amd/csrc/control_points.h): the text
// the kernels of control.hip run, here on the CPU, one loop iteration per device thread.
//   control_points_main IN OUT [first_writer | swap_rc]
// IN, little-endian, first word int32 kind:
//   kind 0 (sparse points): int32 mode, K, n, H, W; int32 pos[K][2]; fp32 val[n][K][2]      -> OUT fp32 [n][4][H][W]
//   kind 1 (flow finish):   int32 has_in, has_out, has_brush, n, hs, ws, H, W; fp32 flow_in[n][2][hs][ws] (if has_in);
//                           fp32 flow_out (if has_out); uint8 brush[hs][ws] (if has_brush)  -> OUT fp32 [n][2][H][W]
// Exit status 22: an ADD position off the canvas (what the wrapper refuses).  The optional third argument runs a deliberately
// wrong variant, to show that the case table tells it apart: first_writer = LAST decided by ADD's first-writer rule,
// swap_rc = rows and columns of the positions exchanged.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../mofa_video_amd/csrc/control_points.h"

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}

static int sparse(FILE* f, std::vector<float>& out, const bool first_writer, const bool swap_rc) {
    int32_t h[5];
    if (fread(h, sizeof(int32_t), 5, f) != 5) return 2;
    const int mode = h[0], K = h[1], n = h[2], H = h[3], W = h[4];
    if ((mode != CONTROL_SPARSE_ADD && mode != CONTROL_SPARSE_LAST) || K < 0 || K > CONTROL_MAX_POINTS || n <= 0 || n > 4096 || H <= 0 ||
        H > 4096 || W <= 0 || W > 4096)
        return 2;
    std::vector<int32_t> pos;
    std::vector<float> val;
    if (!rd(f, pos, (size_t)K * 2) || !rd(f, val, (size_t)n * K * 2)) return 2;
    if (swap_rc)
        for (int k = 0; k < K; ++k) {
            const int32_t t = pos[2 * k];
            pos[2 * k] = pos[2 * k + 1];
            pos[2 * k + 1] = t;
        }
    std::vector<int> keys(K);
    for (int k = 0; k < K; ++k) {
        keys[k] = control_point_key(pos.data(), k, H, W, mode);
        if (keys[k] < 0) return 22;
        if (keys[k] >= H * W) {                              // the key function promises a pixel of the canvas
            fprintf(stderr, "key %d beyond %d x %d\n", keys[k], H, W);
            return 3;
        }
    }
    const size_t hw = (size_t)H * W;
    out.assign((size_t)n * 4 * hw, 0.0f);                    // the launch's clear
    for (int i = n - 1; i >= 0; --i)                         // any order of (i, k) gives the same result: run it backwards
        for (int k = K - 1; k >= 0; --k) {
            if (!control_is_writer(keys.data(), K, k, first_writer ? CONTROL_SPARSE_ADD : mode)) continue;
            const float* v = val.data() + (size_t)i * K * 2;
            float sx, sy, count;
            if (mode == CONTROL_SPARSE_ADD) {
                control_add_sum(keys.data(), v, K, k, sx, sy, count);
            } else {
                sx = v[2 * k];
                sy = v[2 * k + 1];
                count = 1.0f;
            }
            float* o = out.data() + (size_t)i * 4 * hw + keys[k];
            o[0] = sx;
            o[hw] = sy;
            o[2 * hw] = count;
            o[3 * hw] = count;
        }
    return 0;
}

static int finish(FILE* f, std::vector<float>& out) {
    int32_t h[8];
    if (fread(h, sizeof(int32_t), 8, f) != 8) return 2;
    const bool has_in = h[0] != 0, has_out = h[1] != 0, has_brush = h[2] != 0 && has_in;
    const int n = h[3], hs = h[4], ws = h[5], H = h[6], W = h[7];
    for (int i = 3; i < 8; ++i)
        if (h[i] <= 0 || h[i] > 4096) return 2;
    std::vector<float> fin, fout;
    std::vector<unsigned char> brush;
    const size_t shw = (size_t)hs * ws, dhw = (size_t)H * W;
    if (!rd(f, fin, has_in ? n * 2 * shw : 0) || !rd(f, fout, has_out ? n * 2 * shw : 0) || !rd(f, brush, h[2] != 0 ? shw : 0)) return 2;
    const float sy = (float)hs / (float)H, sx = (float)ws / (float)W;              // as mofa_flow_finish_f32 sets them up
    const bool scaled = H != hs || W != ws;
    const float fy = (float)((double)H / (double)hs), fx = (float)((double)W / (double)ws);
    out.assign((size_t)n * 2 * dhw, 0.0f);
    for (int i = 0; i < n; ++i)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int iy = nearest_src(y, sy, hs), ix = nearest_src(x, sx, ws);
                if (iy < 0 || iy >= hs || ix < 0 || ix >= ws) {
                    fprintf(stderr, "source (%d, %d) beyond %d x %d\n", iy, ix, hs, ws);
                    return 3;
                }
                const size_t s = (size_t)iy * ws + ix, p0 = ((size_t)i * 2) * shw + s, p1 = p0 + shw;
                float ox, oy;
                control_finish_pixel(has_in ? fin[p0] : 0.0f, has_in ? fin[p1] : 0.0f, has_out ? fout[p0] : 0.0f, has_out ? fout[p1] : 0.0f,
                                     has_brush, has_brush ? brush[s] : (unsigned char)255, scaled, fx, fy, ox, oy);
                out[((size_t)i * 2) * dhw + (size_t)y * W + x] = ox;
                out[((size_t)i * 2 + 1) * dhw + (size_t)y * W + x] = oy;
            }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) {
        fprintf(stderr, "usage: %s IN OUT [first_writer | swap_rc]\n", argv[0]);
        return 2;
    }
    const bool first_writer = argc == 4 && !strcmp(argv[3], "first_writer"), swap_rc = argc == 4 && !strcmp(argv[3], "swap_rc");
    if (argc == 4 && !first_writer && !swap_rc) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t kind;
    if (fread(&kind, sizeof(int32_t), 1, f) != 1) return 2;
    std::vector<float> out;
    const int rc = kind == 0 ? sparse(f, out, first_writer, swap_rc) : (kind == 1 ? finish(f, out) : 2);
    fclose(f);
    if (rc != 0) return rc;
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 2;
    return fclose(f) == 0 ? 0 : 2;
}
