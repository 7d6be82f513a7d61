// The host-side launch plan of the implicit GEMM: everything mofa_igemm_f16 decides before it launches -- the argument checks,
// the epilogue kind, the output tile (cost model, then the fall-back chain), split-K of the last round and the grid.  Host
// code only (no HIP header; compiles with plain g++ -std=c++17): mofa_igemm_f16 launches what igemm_plan() says, and
// mofa_igemm_plan exports the same answer, so tests/igemm_plan_table.json can pin the decision of every shape without a GPU.
#pragma once
#include <stdint.h>
#include "../../include/mofa_hip.h"

typedef mofa_igemm_plan_t IgemmPlan;

// the four output tiles (igemm.hip: the 4-wave kernels, two workgroups per CU; igemm8.hip, igemm320.hip: 8 waves, one)
struct IgemmTile { int tm, tn, threads, lds, wg_per_cu; };
static inline const IgemmTile& igemm_tile(int id) {
    static const IgemmTile tiles[4] = {
        {128, 128, 256, 2 * 256 * 128, 2},   // 128^2 tile, 2 workgroups per CU
        {192, 128, 256, 2 * 320 * 128, 2},   // 192x128 tile: 2 x 80 KB = the whole LDS of a CU
        {256, 256, 512, 163840, 1},          // 256x256: the CU's whole LDS
        {256, 320, 512, 159744, 1},          // 256x320
    };
    return tiles[id == MOFA_TILE_128X128 ? 0 : id == MOFA_TILE_192X128 ? 1 : id == MOFA_TILE_256X256 ? 2 : 3];
}

static inline int igemm_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// (constexpr: host code here, and hipcc lets the kernels call a constexpr function too; always inlined there, as ever)
// (igemm_taps_classic: modes 0-2 alone -- what the kernel instantiations of those modes evaluate, so that they compile to the
// code they had before MOFA_MODE_CONV3X3_UP2F existed; the folded mode's instantiations know their 4 taps at compile time)
__attribute__((always_inline)) constexpr int igemm_taps_classic(const mofa_igemm_args& a) {
    return (a.mode == MOFA_MODE_CONV3X3) ? (a.ksize > 0 ? a.ksize * a.ksize : 9) : (a.mode == MOFA_MODE_CONVT3 ? 3 : 1);
}
__attribute__((always_inline)) constexpr int igemm_taps(const mofa_igemm_args& a) {
    return a.mode == MOFA_MODE_CONV3X3_UP2F ? 4 : igemm_taps_classic(a);
}

// ---- MOFA_MODE_CONV3X3_UP2F: the row tiles are NOT the output rows ------------------------------------------------------------
// A 256-row tile multiplies all its rows by one weight tile, so it belongs to one phase p = 2 a + b: the Mq = M / 4 source pixels
// (img, y, x) are padded to whole tiles per phase, and the phases are INTERLEAVED tile by tile: row tile t holds pixels
// 256 (t >> 2) .. + 255 of phase t & 3.  The tile walk hands an XCD a contiguous range of tile ids (row tile major), so the four
// passes over one 256-pixel input region (and its halo rows) run back to back on the same XCD and find the region in its L2;
// phase-major order would put 1/4 of the launch between two reads of the same input rows.
// Rows of the weight matrix [4 N][4 Cin] a launch addresses / its row tiles:
static inline long long igemm_w_rows(const mofa_igemm_args* a) { return a->mode == MOFA_MODE_CONV3X3_UP2F ? 4ll * a->N : a->N; }
static inline int igemm_tiles_m(const mofa_igemm_args* a, int tm) {
    return a->mode == MOFA_MODE_CONV3X3_UP2F ? 4 * (int)((a->M / 4 + 255) / 256) : (int)(((long long)a->M + tm - 1) / tm);
}
// THE decode of a tile row r (row r & 255 of row tile r >> 8): its phase and source pixel; valid = 0 for a padding row.  The
// producer side of the kernels (which source rows to fetch) and the row map below (where the result is stored) both start here.
// div_hw / div_w divide by Hin * Win / Win (the kernels pass their magic-number dividers, the host plain division).
struct IgemmUp2fPixel { int ph, img, y, x, valid; };
template <class DivHW, class DivW>
__attribute__((always_inline)) constexpr IgemmUp2fPixel igemm_up2f_pixel(const mofa_igemm_args& a, int r, DivHW div_hw, DivW div_w) {
    const int q = ((r >> 10) << 8) | (r & 255);
    const int img = div_hw(q), rem = q - img * (a.Hin * a.Win);
    const int y = div_w(rem);
    return IgemmUp2fPixel{(r >> 8) & 3, img, y, rem - y * a.Win, q < (a.M >> 2) ? 1 : 0};
}
// THE row map: tile row r -> the output row it is stored to, or -1 for a padding row
template <class DivHW, class DivW>
__attribute__((always_inline)) constexpr int igemm_up2f_out_row(const mofa_igemm_args& a, int r, DivHW div_hw, DivW div_w) {
    const IgemmUp2fPixel s = igemm_up2f_pixel(a, r, div_hw, div_w);
    const int o = (s.img * a.Hout + 2 * s.y + (s.ph >> 1)) * a.Wout + 2 * s.x + (s.ph & 1);
    return s.valid ? o : -1;
}
struct IgemmPlainDiv { int d; constexpr int operator()(int n) const { return n / d; } };
constexpr int igemm_up2f_out_row(const mofa_igemm_args& a, int r) {
    return igemm_up2f_out_row(a, r, IgemmPlainDiv{a.Hin * a.Win}, IgemmPlainDiv{a.Win});
}

// the grid of the XCD-aware persistent tile walk (TileWalk, igemm_common.h): one workgroup per tile up to `slots` resident
// workgroups, a multiple of 8 (equal shares per XCD), at least 8
static inline int igemm_grid(long long ntiles, int slots) {
    const int grid = (int)(ntiles < slots ? ((ntiles + 7) / 8) * 8 : (slots / 8) * 8);
    return grid < 8 ? 8 : grid;
}

// rows of the activation buffer the launch may address (convT3 without clipping: one halo frame on either side)
static inline long long igemm8_rows_in(const mofa_igemm_args* a) {
    if (a->mode == MOFA_MODE_CONV3X3 || a->mode == MOFA_MODE_CONV3X3_UP2F) return a->M / ((long long)a->Hout * a->Wout) * a->Hin * a->Win;
    if (a->mode == MOFA_MODE_CONVT3 && a->T == 0) return (long long)a->M + 2ll * a->HW;
    return a->M;
}

// the 8-wave tiles: 16-byte row alignment everywhere (the kernels have no narrow-store path); packed row geometry and 32-bit
// offsets in range
static inline bool igemm_pipe_eligible(const mofa_igemm_args* a, int kind, long long Ktot) {
    const int nout = kind == 8 ? a->N / 2 : a->N;
    if ((a->ldo & 7) || (nout & 7) || (a->N & 7) || (((uintptr_t)a->out) & 15) || (((uintptr_t)a->x) & 15)) return false;
    if (a->r1 && ((a->ldr1 & 7) || (((uintptr_t)a->r1) & 15))) return false;
    if (a->r2 && ((a->ldr2 & 7) || (((uintptr_t)a->r2) & 15))) return false;
    if (a->bias && (((uintptr_t)a->bias) & 15)) return false;
    if ((a->r1 || a->r2 || a->rowvec) && a->act != MOFA_ACT_NONE) return false;   // only the plain kind carries activation code here
    if (a->rowvec && (((uintptr_t)a->rowvec) & 15)) return false;
    if (igemm_w_rows(a) * Ktot * 2 >= (1ll << 32) || (((uintptr_t)a->w) & 15)) return false;
    if (a->mode == MOFA_MODE_CONV3X3_UP2F) {
        if (a->M > 0x7fff0000) return false;                   // (padded tile rows stay below 2^31; Hin, Win, images: igemm_check_args)
    } else if (a->mode == MOFA_MODE_CONV3X3) {
        const long long nimg = a->M / ((long long)a->Hout * a->Wout);
        if (a->Hout > 1024 || a->Wout > 1024 || nimg > 2047) return false;
    } else if (a->mode == MOFA_MODE_CONVT3) {
        if (a->M >= (1 << 29)) return false;
    }
    if (igemm8_rows_in(a) * a->ldx * 2 >= (1ll << 32) - 65536) return false;   // 32-bit buffer offsets
    return true;
}

// can the 256x320 tile run these arguments?  (kind 7 = row vector + two residuals does not fit the register file beside 160
// accumulators and has no kernel there)
static inline bool igemm320_eligible(const mofa_igemm_args* a, int kind, int taps) {
    if (kind == 7 || !igemm_pipe_eligible(a, kind, (long long)taps * a->Cin)) return false;
    return (igemm_w_rows(a) + 320) * taps * a->Cin * 2 < 0x7ff00000LL;   // unclamped W row offsets stay below W_DEAD
}

// can a launch with these arguments emit mofa_igemm_args.stats?  (a->stats itself is not looked at)
static inline bool igemm320_stats_ok(const mofa_igemm_args* a) {
    if (!a || !a->x || !a->w || !a->out || a->M <= 0 || a->N <= 0 || a->Cin <= 0 || a->Cin % 64 != 0) return false;
    if (a->act != MOFA_ACT_NONE || a->r2 || (a->r1 && a->s1 != 1.0f)) return false;
    if (a->M % 64 != 0 || a->N % 320 != 0) return false;
    if (a->rowvec && (a->rv_mod_in != 1 || a->rv_div <= 0 || a->rv_div % 64 != 0)) return false;   // constant over a wave's 64 rows
    if (a->tile != 0 && a->tile != MOFA_TILE_256X320) return false;
    return igemm320_eligible(a, (a->r1 ? 1 : 0) | (a->rowvec ? 4 : 0), igemm_taps(*a));
}

// Split-K for the tiles of a partial last round.  T tiles on n_cu persistent workgroups take ceil(T / n_cu) tile times although
// the last round may hold only a few tiles (M = 460800, N = 320: 1800 tiles = 7 rounds + 8 tiles; M = 7200: 116 tiles on 256
// CUs).  When a workspace is supplied, the R = T mod n_cu remainder tiles are cut into S K-slices (R * S <= n_cu work items of
// nk / S K tiles each, fp32 partial tiles in the workspace) and a small fix-up kernel adds the slices in slice order and
// applies the epilogue: the round shrinks to about 1 / S of a tile time.  Returns S (1 = no split).
static inline int igemm320_split(long long T, int nk, int n_cu, long long ws_bytes) {
    const long long R = T % n_cu;
    if (ws_bytes <= 0 || R == 0) return 1;
    if (T > n_cu && R * 10 > (long long)n_cu * 6) return 1;   // a last round that is more than 60 % full stays whole
    long long s = n_cu / R;
    if (s > 8) s = 8;
    if (s > nk / 8) s = nk / 8;                                // at least eight K tiles per slice, and ... (r04: up to 16 slices
                                                               // of >= 4 K tiles changes nothing on the per-rank shapes of an
                                                               // 8-GPU run: mix 691 against 693 TF/s, profiles/r04_shard_shapes_tiles.log)
    // ... only where it pays: a slice saves (1 - 1 / S) of a tile's K loop (about 2 us per K tile) but costs the partial-tile
    // dump and the fix-up launch (about 25 us; profiles/archive/r03b_kernel_stats_bench.md: splitting the shallow-K launches of the
    // clip -- 5 100 of 12 012 -- made it 4 % SLOWER)
    if (s >= 2 && 2.0 * nk * (1.0 - 1.0 / (double)s) < 50.0) s = 1;
    const long long per = (long long)256 * 320 * 4;
    while (s >= 2 && R * s * per > ws_bytes) --s;
    return s >= 2 ? (int)s : 1;
}

// The argument checks mofa_igemm_f16 makes before it touches the device: MOFA_OK or MOFA_EINVAL.
static inline int igemm_check_args(const mofa_igemm_args* a) {
    if (!a || !a->x || !a->w || !a->out) return MOFA_EINVAL;
    if (a->M <= 0 || a->N <= 0 || a->Cin <= 0) return MOFA_EINVAL;
    if (a->Cin % 64 != 0 || a->N % 4 != 0) return MOFA_EINVAL;
    if (a->mode < 0 || a->mode > MOFA_MODE_CONV3X3_UP2F || a->act < 0 || a->act > MOFA_ACT_GELU) return MOFA_EINVAL;
    if (a->mode == MOFA_MODE_CONV3X3) {
        if (a->Hin <= 0 || a->Win <= 0 || a->Hout <= 0 || a->Wout <= 0) return MOFA_EINVAL;
        if ((a->stride != 1 && a->stride != 2) || (a->up != 1 && a->up != 2)) return MOFA_EINVAL;
        if (a->ksize != 0 && a->ksize != 1 && a->ksize != 3 && a->ksize != 5 && a->ksize != 7) return MOFA_EINVAL;
        if (a->dil < 0 || (a->dil > 1 && a->up != 1)) return MOFA_EINVAL;
        if (a->pad != MOFA_PAD_SAME && a->pad != MOFA_PAD_TRAILING) return MOFA_EINVAL;
        if (a->M % (a->Hout * a->Wout) != 0 || a->Hout > 65535 || a->Wout > 65535) return MOFA_EINVAL;
    }
    if (a->mode == MOFA_MODE_CONV3X3_UP2F) {                   // the folded nearest-2x + 3x3 (mofa_hip.h): plain epilogue, 8-wave tiles
        if (a->Hin <= 0 || a->Win <= 0 || a->Hin > 1024 || a->Win > 1024) return MOFA_EINVAL;
        if (a->Hout != 2 * a->Hin || a->Wout != 2 * a->Win || a->stride != 1 || a->up != 2) return MOFA_EINVAL;
        if ((a->ksize != 0 && a->ksize != 3) || (a->dil != 0 && a->dil != 1) || a->pad != MOFA_PAD_SAME) return MOFA_EINVAL;
        if (a->M % (a->Hout * a->Wout) != 0 || a->M / (a->Hout * a->Wout) > 2047) return MOFA_EINVAL;
        if (a->act != MOFA_ACT_NONE || a->r1 || a->r2 || a->rowvec || a->stats) return MOFA_EINVAL;
        if (a->tile == MOFA_TILE_128X128 || a->tile == MOFA_TILE_192X128) return MOFA_EINVAL;
        if (!igemm_pipe_eligible(a, 0, 4ll * a->Cin)) return MOFA_EINVAL;   // no 4-wave kernel to fall back to: the 8-wave rules
    }
    if (a->mode == MOFA_MODE_CONVT3 && (a->T < 0 || a->HW <= 0 || (a->T > 0 && a->M % (a->T * a->HW) != 0)))
        return MOFA_EINVAL;
    if (a->rowvec && (a->rv_div <= 0 || a->rv_mod_in <= 0 || a->rv_mod_out <= 0)) return MOFA_EINVAL;
    if (a->act == MOFA_ACT_GEGLU_PAIR && (a->N % 64 != 0 || a->r1 || a->r2 || a->rowvec)) return MOFA_EINVAL;
    if (a->ldx % 8 != 0 || a->ldo % 4 != 0) return MOFA_EINVAL;
    if ((a->r1 && a->ldr1 % 4 != 0) || (a->r2 && a->ldr2 % 4 != 0)) return MOFA_EINVAL;
    if (a->tile != 0 && a->tile != MOFA_TILE_128X128 && a->tile != MOFA_TILE_192X128 && a->tile != MOFA_TILE_256X256 &&
        a->tile != MOFA_TILE_256X320)
        return MOFA_EINVAL;
    if (a->stats && !igemm320_stats_ok(a)) return MOFA_EINVAL;   // GroupNorm pair sums from the epilogue: the 256x320 tile only
    return MOFA_OK;
}

// The cost model: the MOFA_TILE_* of the cheapest tile for these (checked) arguments on n_cu compute units.
static inline int igemm_model_tile(const mofa_igemm_args* a, int kind, long long Ktot, int n_cu) {
    // Tile choice = the cheapest of  rounds of resident workgroups x CU time of one round, the latter modelled as
    //   workgroups per CU x tile area x relative K-loop cost per flop x (1 + epilogue / K loop),  epilogue in K tiles:
    //     128x128   1.00   two workgroups per CU
    //     192x128   0.86   two workgroups fill the CU's 160 KB of LDS exactly; 17 % less fill / LDS-read traffic per
    //                      flop, 50 % more MFMA work per barrier
    //     256x256   0.62   8 waves, phase-pipelined K loop (igemm8.hip; needs 16-byte aligned rows)
    // fitted to tools/igemm_tiles_bench.py on the denoise step's shapes (profiles/r02_igemm_tiles.md).  Rounds count the
    // padding waste of partial tiles and the idle slots of the last round (e.g. N = 320: 2 x 256 wastes 37 %, 3 x 128
    // 17 %; M = 7200: 570 tiles of 128x128 need two rounds of 512 slots, 380 tiles of 192x128 one).
    static const double rel[2] = {1.00, 0.86};
    static const int ids[2] = {MOFA_TILE_128X128, MOFA_TILE_192X128};
    // epilogue cost in K tiles per epilogue kind (index = kind): 4-wave tiles (their epilogue overlaps the co-resident
    // workgroup's K loop) / the 8-wave tile
    static const double epi4[9] = {2.0, 3.5, 4.0, 4.0, 3.5, 4.0, 4.5, 4.5, 4.0};
    static const double epi8[9] = {2.2, 5.2, 5.2, 6.0, 5.6, 5.5, 5.5, 6.3, 2.4};   // ([4]: fitted to the N = 320 choice, not the 2.6 measured)
    const double nk = (double)(Ktot / 64);
    int choice = 0;
    double best = 0;
    for (int k = 0; k < 2 && a->mode != MOFA_MODE_CONV3X3_UP2F; ++k) {   // (the folded mode has no 4-wave kernel)
        const IgemmTile& c = igemm_tile(ids[k]);
        const long long t = (long long)igemm_cdiv(a->M, c.tm) * igemm_cdiv(a->N, c.tn);
        const long long slots_k = (long long)n_cu * c.wg_per_cu;
        const double cost = (double)((t + slots_k - 1) / slots_k) * c.tm * c.tn * rel[k] * c.wg_per_cu * (1.0 + epi4[kind] / nk);
        if (choice == 0 || cost < best) { best = cost; choice = ids[k]; }
    }
    {
        const long long t = (long long)igemm_tiles_m(a, 256) * igemm_cdiv(a->N, 256);
        const double cost = (double)((t + n_cu - 1) / n_cu) * 256 * 256 * 0.62 * (1.0 + epi8[kind] / nk);
        if (choice == 0 || cost < best) { best = cost; choice = MOFA_TILE_256X256; }
    }
    if (kind != 7) {
        // 256x320 (igemm320.hip): 0.58 per area (10 % less LDS-DMA, 7 % fewer fragment reads per flop than 256x256); its
        // epilogues move 25 % more outputs per tile
        static const double epi320[9] = {3.0, 7.5, 8.5, 9.5, 3.5, 7.9, 9.0, 12.0, 5.0};   // fitted: profiles/archive/r03_igemm_tiles_bench.log; r04: the
        // residual kinds [1] [2] [3] [5] [6] lowered by 1.5-2 with the fp16-transposed residual epilogue (profiles/r04_res16_tiles_ab.log);
        // [1], [5] lowered from 10.0 / 10.5 in r03c so that the K = N = 320 residual launches leave the 192x128 tile (alone a
        // draw: 352-414 against 372-403 TF/s by box; in the clip - 0.27 %, profiles/archive/r03c_cost_model_and_splitk_ab.log:
        // beside a second stream the 17 % of padded columns of 3 x 128 are no longer free)
        const long long t = (long long)igemm_tiles_m(a, 256) * igemm_cdiv(a->N, 320);
        // a partial last round split along K (igemm320_split) costs 1 / S of a round + the fix-up pass.  QUIRK, kept as it
        // is: the model prices the split for ANY workspace pointer, while igemm_plan() below declines it for one that is not
        // 16-byte aligned -- such a launch is costed with a split it does not get.
        const int S = kind == 8 ? 1 : igemm320_split(t, (int)nk, n_cu, a->workspace ? a->workspace_bytes : 0);
        const double rounds = S > 1 ? (double)(t / n_cu) + 1.0 / S + 0.12 : (double)((t + n_cu - 1) / n_cu);
        // wide outputs (many column tiles: every CU of an XCD streams its own weight tile through the fabric) run
        // relatively slower on this tile than on 256x256 (profiles/archive/r03_igemm_tiles_bench_geglu320.log: N = 3840 / 10240
        // 7 / 15 % behind): +2 % per column tile beyond 6, at most +25 %
        const int tn320 = igemm_cdiv(a->N, 320);
        const double wide = 1.0 + (tn320 > 6 ? (tn320 - 6 > 12 ? 0.25 : 0.02 * (tn320 - 6)) : 0.0);
        const double cost = rounds * 256 * 320 * 0.58 * wide * (1.0 + epi320[kind] / nk);
        if (cost < best) { best = cost; choice = MOFA_TILE_256X320; }
    }
    return choice;
}

// The plan of a launch whose arguments passed igemm_check_args, on a device of n_cu > 0 compute units.
static inline IgemmPlan igemm_plan_checked(const mofa_igemm_args* a, int n_cu) {
    IgemmPlan p = {};
    const IgemmPlan refused = {MOFA_EINVAL};
    n_cu = n_cu >= 8 ? (n_cu / 8) * 8 : 8;                    // persistent grids are multiples of 8 (one per XCD): every tile /
                                                              // round / split-K count below uses the SAME rounded figure
    const int taps = igemm_taps(*a);
    const long long Ktot = (long long)taps * a->Cin;
    const int kind = a->act == MOFA_ACT_GEGLU_PAIR ? 8 : ((a->r1 ? 1 : 0) | (a->r2 ? 2 : 0) | (a->rowvec ? 4 : 0));
    // QUIRK, kept as it is: a->stats forces the 256x320 tile like a->tile does (igemm_check_args has asked igemm320_stats_ok,
    // which implies igemm320_eligible for this kind), and a stats pointer that is not 16-byte aligned is refused below
    const bool forced = a->tile != 0 || a->stats;
    int choice = a->stats ? MOFA_TILE_256X320 : a->tile != 0 ? a->tile : igemm_model_tile(a, kind, Ktot, n_cu);
    // The fall-back chain, in this order: a tile the MODEL chose that cannot run these arguments hands over to the next one;
    // a tile the CALLER forced is refused instead.  Both 8-wave tiles share igemm_pipe_eligible, so what 256x320 alone refuses
    // (W offsets beyond its bound) goes to 256x256, and what both refuse to 192x128, the cheaper 4-wave tile per flop and the
    // end of the chain: it takes every checked argument set.  128x128 runs only as the model's or the caller's FIRST choice.
    static const int chain[3] = {MOFA_TILE_256X320, MOFA_TILE_256X256, MOFA_TILE_192X128};
    for (int i = 0; i < 2; ++i) {
        if (choice != chain[i]) continue;
        if (i == 0 ? (a->stats || igemm320_eligible(a, kind, taps)) : igemm_pipe_eligible(a, kind, Ktot)) break;
        if (forced) return refused;
        choice = chain[i + 1];
    }
    if (a->mode == MOFA_MODE_CONV3X3_UP2F && choice != MOFA_TILE_256X320 && choice != MOFA_TILE_256X256) return refused;
    const IgemmTile& c = igemm_tile(choice);
    const int tilesM = igemm_tiles_m(a, c.tm), tilesN = igemm_cdiv(a->N, c.tn);
    const long long nt = (long long)tilesM * tilesN;
    if (nt > 0x7fffffffLL) return refused;
    if (a->stats && (((uintptr_t)a->stats) & 15)) return refused;
    const int slots = n_cu * c.wg_per_cu;                     // resident workgroups (a multiple of 8 on gfx950)
    p.tile = choice; p.kind = kind; p.tiles_m = tilesM; p.tiles_n = tilesN; p.threads = c.threads; p.lds_bytes = c.lds;
    p.grid = igemm_grid(nt, slots);
    p.split = 1; p.full_tiles = (int)nt; p.launches = 1;
    p.stats = a->stats ? 1 : 0;
    if (choice == MOFA_TILE_256X320 && kind != 8) {           // (the fix-up has no GEGLU form)
        const bool ws_ok = a->workspace && (((uintptr_t)a->workspace) & 15) == 0;
        p.split = igemm320_split(nt, (int)(Ktot / 64), n_cu, ws_ok ? a->workspace_bytes : 0);
    }
    if (p.split > 1) {                                        // (what is launched then: igemm320_launch)
        p.full_tiles = (int)(nt - nt % n_cu);
        p.rem_tiles = (int)(nt % n_cu);
        p.grid = p.full_tiles > 0 ? (n_cu / 8) * 8 : ((p.rem_tiles * p.split + 7) / 8) * 8;
        p.launches = a->stats ? 3 : 2;
        if (p.grid < p.rem_tiles * p.split) return refused;   // (R * S <= n_cu by construction)
    }
    return p;
}

static inline IgemmPlan igemm_plan(const mofa_igemm_args* a, int n_cu) {
    const IgemmPlan refused = {igemm_check_args(a)};
    return refused.rc == MOFA_OK ? igemm_plan_checked(a, n_cu) : refused;
}
