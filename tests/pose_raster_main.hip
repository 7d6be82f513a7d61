// Host execution of the shared per-segment rasteriser (mofa_video_amd/csrc/landmarks_raster.h): the text the kernel of
// landmarks.hip runs, here on the CPU with a plain array as the canvas and a max-combine as the plot.
//   pose_raster_main IN OUT
// IN:  int32 little-endian: N, w, h, then N * 68 * 2 coordinates (x, y).
// OUT: int32 [N][h][w]: 0 = background, s + 1 = the highest-numbered segment s that covers the pixel.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../mofa_video_amd/csrc/landmarks_raster.h"

struct HostMax {
    int32_t* canvas;
    int w, h, value;
    void operator()(int x, int y) const {
        if (x < 0 || x >= w || y < 0 || y >= h) {            // the rasteriser promises in-range pixels
            fprintf(stderr, "plot out of range: (%d, %d) on %d x %d\n", x, y, w, h);
            exit(3);
        }
        int32_t& p = canvas[(size_t)y * w + x];
        p = p > value ? p : value;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (fread(hdr, sizeof(int32_t), 3, f) != 3) return 2;
    const int N = hdr[0], w = hdr[1], h = hdr[2];
    if (N <= 0 || N > 4096 || w <= 0 || w > 4096 || h <= 0 || h > 4096) return 2;
    std::vector<int32_t> pts((size_t)N * POSE_POINTS * 2);
    if (fread(pts.data(), sizeof(int32_t), pts.size(), f) != pts.size()) return 2;
    fclose(f);
    std::vector<int32_t> canvas((size_t)N * h * w, 0);
    for (int n = 0; n < N; ++n)
        for (int s = POSE_SEGMENTS - 1; s >= 0; --s) {       // any order gives the same canvas: run it backwards
            HostMax plot{canvas.data() + (size_t)n * h * w, w, h, s + 1};
            pose_draw_segment(w, h, pts.data() + (size_t)n * POSE_POINTS * 2, s, plot);
        }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (fwrite(canvas.data(), sizeof(int32_t), canvas.size(), f) != canvas.size()) return 2;
    return fclose(f) == 0 ? 0 : 2;
}
