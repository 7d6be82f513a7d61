// Implicit GEMM, 256 (M) x 320 (N) output tile, 8 waves, phase-pipelined K loop: the tile of the UNet's channel counts.
//
// Every N of the SVD UNet / ControlNet trunk is a multiple of 320 (320, 640, 960, 1280, 1920, 2560, 3840, ...): a
// 320-wide tile has NO padded columns on any of them (256-wide tiles waste 37.5 % of their MFMA issue at N = 320, 17 % at
// N = 640), reads the activation tile ONCE where N = 320 (the 256x256 and 192x128 kernels stream it 2 and 3 times), and
// moves 10 % fewer bytes through the LDS-DMA path per flop than the 256x256 tile ((256 + 320) / (256 * 320) rows per
// output).  Same contract (mofa_hip.h), operand roles (MFMA A = weight tile, B = activation tile: an accumulator lane owns
// one output row), buffer-descriptor DMA with bounds-check zero fill, persistent XCD-aware tile walk and two-wave-group
// stagger as igemm8.hip; what differs:
//
//   * wave (wm, wn) of 4 x 2 owns 64 (M) x 160 (N) outputs = 2 x 5 accumulator blocks of 32x32 (160 accumulator registers).
//     A K tile (64 deep) is consumed in TWO PHASES BY K HALVES: phase p multiplies K columns [32 p, 32 p + 32) of all the
//     wave's rows -- 4 X + 10 W fragment reads (56 registers), 40 MFMAs (640 matrix-pipe cycles) -- so both phases carry
//     the same reads and the same MFMA count (the 256x256 kernel splits by X rows: 16 + 8 reads).
//   * the K loop runs on v_mfma_f32_16x16x32_f16: a K half is ONE K step of that shape, each fragment (16 rows x 32 K) one
//     ds_read_b128, each 32x32 block four 16x16 tiles in the quarters of its 16 registers.  Same reads, same matrix-pipe
//     cycles and -- measured -- the same bits as two 32x32x16 steps, but the power-limited chip holds a higher clock on this
//     shape (tools/lds_mfma_bench.hip, profiles/igemm320_k16_loop_bench.log: + 14 % bare, + 7 % beside the DMA issue;
//     tile bench + 5-9 % on the deep-K shapes, clip + 2.1 %: profiles/igemm320_k16_*.log).  The W rows of a fragment are read
//     in an order (bits 2 and 3 of the row swapped) that makes 80 v_permlane16_swap_b32 per tile turn the accumulators into
//     the 32x32 register layout (to_layout32); every epilogue, the split-K dump and the GroupNorm sums work on that layout.
//   * LDS: a ring of 2 K tiles, each as two K-HALF PLANES [X 256 rows | W 320 rows] x 64 B (36 KB per plane, 72 KB per K
//     tile, 144 KB ring + 8 x 2 KB wave scratch = the CU's 160 KB).  A plane is released when its phase's fragments are in
//     registers and refilled in the NEXT phase: phase 0 issues plane 1 of K tile t + 1, phase 1 issues plane 0 of K tile
//     t + 2 -- 4 or 5 DMA pieces per wave and phase (9 per K tile; waves 0-3 take the ring's 4 odd W pieces in plane 0,
//     waves 4-7 in plane 1), each with one K tile of flight before the counted wait `vmcnt(9)`.  A DMA piece is 16 rows x
//     64 B (tools/dmabench.hip, profiles/archive/r03_dmabench.log: up to 5 such half-line pieces per phase hide completely behind
//     20 32x32x16 MFMAs of the partner wave; 6 do not).  64-byte rows: the 16-byte chunk c of row r sits in slot
//     c ^ slot_swz((r >> 2) & 3) (applied to the DMA source address and to the fragment read; tools/lds_bank_sim.py:
//     conflict-free for the 16-row fragment reads; the plain c ^ ((r >> 2) & 3) of the 32-row reads is 2-way on them).
//   * bias (and the row vector when the wave's 64 rows share one row of it: every tile that does not straddle a frame) is
//     the INITIAL VALUE of the accumulators -- no bias handling in any epilogue.  The bias arrives through LDS one tile
//     ahead (LDS-DMA into a 768-byte slot per wave and tile parity), the uniform row-vector row by global loads.
//   * epilogues: no residual, uniform row vector -> activation in the fragment layout, fp16, 32 x 32 transposes, 16-byte
//     stores; residuals / per-row row vector -> 16 x 32 fp32 transposes (half the lanes write at a time), the sum rounded once.
// Kinds: plain (+ SiLU / ReLU / GELU), row vector, one or two residuals, GEGLU pair (value / gate rows interleaved by 16).
#include "igemm_common.h"
#include "igemm_pipe.h"

namespace {

constexpr int WN3 = 2, MI3 = 2;                                // wave grid 4 x 2, accumulator row tiles per wave
constexpr int TBM3 = 256;
constexpr int RBH = 64;                                        // bytes of one K half of a row
constexpr int XPL = TBM3 * RBH;                                // X part of a plane (16 KB)
// NJ3 = accumulator column tiles per wave: 5 -> the 256x320 tile.  NJ = 4 (a 256x256 tile with the same K-half schedule, incl.
// the GEGLU pair epilogue below) was built and measured in round 3: it is 5-10 % SLOWER than igemm8.hip's X-row split on every
// shape (profiles/archive/r03_igemm_tiles_bench_with_ksplit256.log: GEGLU L0 / L1 / L2 750 / 920 / 1039 against 833 / 1017 / 1141
// TF/s) -- the 256x320 tile's advantage is its shape (load segment of 14 reads + 4.5 DMA pieces under 640 MFMA cycles; 256x256:
// 12 + 4 under 512), not the K-half split.
constexpr int NJ3 = 5;
constexpr int TBN3 = WN3 * NJ3 * 32;                           // 320
constexpr int PLANE = (TBM3 + TBN3) * RBH;                     // 36 KB
constexpr int SLOT = 2 * PLANE;                                // one K tile
constexpr int BIAS0 = 2 * SLOT;                                // per wave 2 x 768 B: the bias of this tile and of the next one
constexpr int LDS_BYTES3 = BIAS0 + 8 * 2 * 768;                // 159744 (the epilogue transposes through a free ring plane)
constexpr int LOOKAHEAD3 = 4 + NJ3;                            // DMA instructions of the last two phases may be in flight

// epilogue scratch row r (128 bytes) of a wave: rows 8 b .. 8 b + 7 in its 1 KB block b, the blocks 8 KB apart (see the kernel)
struct ScratchRows { __device__ __forceinline__ int operator()(int r) const { return (r >> 3) * 8192 + (r & 7) * 128; } };

// slot swizzle of the K-half planes: the 16-byte chunk c of row r sits in slot c ^ slot_swz((r >> 2) & 3) = c ^ {0, 3, 2, 1}.  A
// ds_read_b128 is served in four groups of 16 lanes (0-3 12-15 20-27 | 4-11 16-19 28-31 | + 32); with lane l on row l & 15, chunk
// l >> 4, a group holds rows {0-3, 12-15} of one chunk and rows 4-11 of its neighbour: the four row quads need four different slots
// (the plain c ^ ((r >> 2) & 3) puts quads 0 and 1, 2 and 3 on the same banks: 2-way).  tools/lds_bank_sim.py: conflict-free.
__device__ __forceinline__ int slot_swz(int q) { return q ^ ((q & 1) << 1); }

struct Cursor3 {                    // one K-half plane of the persistent K-tile stream
    int local;                      // walk position of the output tile it is in
    int ikc, ksw, ky, kx;           // K tile within the tap / overall, tap coordinates (convT3: ky = tap)
    int gx0, gx1;                   // packed row geometry of this wave's two X pieces (16 rows each)
    unsigned xo0, xo1;              // source row of the current tap + this lane's swizzled chunk, bytes from aux.xbase
    int phase;                      // 0: whole tiles of the walk, 1: this workgroup's split-K item, 2: past the end
    int kend;                       // first K tile beyond the current item's K range
    unsigned wo0;                   // weight row of W piece `wave` + this lane's swizzled chunk, bytes from a.w; the
                                    // wave's other pieces are a uniform number of rows further (rows beyond N: out of the
                                    // descriptor's range = zeros, no clamp)
};

// SPLIT: after its whole tiles (tile ids [0, ntiles)) workgroup b < aux.nitems computes ONE split-K item: K slice b % nsplit of
// remainder tile aux.tile0 + b / nsplit (see igemm320_launch).  Its accumulators start at zero and leave as an fp32 partial
// tile in aux.ws; bias, row vector, residuals and activation are applied by igemm320_fixup_kernel.  The item follows the
// whole tiles in the same persistent stream (the cursors prefetch it during the last whole tile's epilogue).
// STATS: the epilogue also emits the GroupNorm pair sums of the outputs (mofa_igemm_args.stats); kinds 0 / 1 / 4 / 5, no
// activation, no per-row vector (igemm320_stats_ok)
// UP2F: MOFA_MODE_CONV3X3_UP2F (plain epilogue only): row tiles of one phase each (igemm_plan.h), per-tile weight base and tap
// origin, output rows through the row map
template <int EPI, bool SPLIT = false, bool STATS = false, bool UP2F = false>
__global__ __launch_bounds__(512, 2) void igemm320_f16_kernel(const mofa_igemm_args a, const int tilesN, const int ntiles,
                                                              const Aux aux) {
    constexpr bool R1 = (EPI & EPI_R1) != 0, R2 = (EPI & EPI_R2) != 0, RV = (EPI & EPI_RV) != 0, GEGLU = (EPI & EPI_GEGLU) != 0;
    typedef typename SelectT<UP2F, CursorUp2f<::Cursor3>, ::Cursor3>::type Cursor3;   // (UP2F: + the tile's phase)
    extern __shared__ __attribute__((aligned(16))) char smem[];   // the ONLY shared object
    TileWalk walk;
    walk.init(ntiles);
    const bool has_item = SPLIT && (int)blockIdx.x < aux.nitems;
    if (walk.local >= walk.count && !has_item) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;                                     // waves w and w + 4 share a SIMD
    const int wm = wave / WN3, wn = wave - wm * WN3;
    const int l31 = lane & 31, lh = lane >> 5;

    const int taps = kernel_taps<UP2F>(a);
    const int kpt = a.Cin / 64, nk = taps * kpt;
    const size_t Ktot = (size_t)taps * a.Cin;

    // ---- producer side ----------------------------------------------------------------------------------------------
    // plane p of a K tile = 16 X pieces + 20 W pieces of 16 rows x 64 B; wave w issues X pieces w, w + 8, W pieces w, w + 8
    // and, when p == grp, W piece 16 + (w & 3).  Lane l of a piece: row l / 4, slot l % 4 <- source chunk
    // slot ^ slot_swz((row >> 2) & 3) = slot ^ slot_swz((l >> 4) & 3) (piece rows start at multiples of 16)
    auto swz_bytes = [&](int l, int p) __attribute__((always_inline)) { return (((l & 3) ^ slot_swz((l >> 4) & 3)) * 16 + p * RBH); };
    const TapGeo tg(a);
    // W pieces w + 8 and 16 + (w & 3) start 128 and 256 + 16 (w & 3) - 16 w rows after piece w (uniform byte distances)
    const unsigned wd1 = 128u * (unsigned)(Ktot * 2), wd2 = (unsigned)(256 + 16 * (wave & 3) - 16 * wave) * (unsigned)(Ktot * 2);
    constexpr unsigned W_DEAD = 0x80000000u;                       // past the end of the walk: beyond any weight tensor (< 2 GB)
    const BufRsrc rsx = buf_rsrc(aux.xbase, aux.x_bytes), rsw = buf_rsrc(a.w, aux.w_bytes);
    const LdsDma16 bglds16;
    // position in the workgroup's stream -> output tile and K-tile range [kb, ke)
    auto item_decode = [&](int phase, int local, int& tile, int& kb, int& ke) __attribute__((always_inline)) {
        tile = walk.start + (phase == 0 ? local : 0); kb = 0; ke = nk;
        if constexpr (SPLIT) {
            const int q = fdiv((int)blockIdx.x, aux.nsplit_d), ks = (int)blockIdx.x - q * aux.nsplit;
            const int kb1 = fdiv(ks * nk, aux.nsplit_d), ke1 = fdiv((ks + 1) * nk, aux.nsplit_d);
            const bool it = phase == 1;
            tile = it ? aux.tile0 + q : tile;
            kb = it ? kb1 : 0;
            ke = it ? ke1 : nk;
        }
    };
    auto next_pos = [&](int& phase, int& local) __attribute__((always_inline)) {
        if (phase == 0) {
            local += walk.stride;
            if (local >= walk.count) phase = has_item ? 1 : 2;
        } else {
            phase = 2;
        }
    };
    auto cur_setup = [&](Cursor3& c, const int p) __attribute__((always_inline)) {
        // branch-free on purpose (selects on the uniform `live`; see igemm8.hip)
        const bool live = c.phase < 2;
        int tile, kb, ke;
        item_decode(c.phase, c.local, tile, kb, ke);
        const int tm = fdiv(tile, aux.tiles_n), tn = tile - tm * tilesN;
        const int l = lane_now(lane), r_l = l >> 2;
        if constexpr (UP2F) {                                      // the tile's phase: its weight rows start at ph * N
            const int g0 = pack_geo_up2f(a, aux, tm * TBM3 + 16 * wave + r_l), g1 = pack_geo_up2f(a, aux, tm * TBM3 + 16 * (wave + 8) + r_l);
            c.gx0 = live ? g0 : -1;
            c.gx1 = live ? g1 : -1;
            c.ph = tm & 3;
            // (the W rows of a column tile that reaches past N are NOT clamped: for phases 0-2 they are the next phase's weight rows,
            // not the zeros the descriptor returns past the matrix -- columns >= N are never stored, by the epilogue or the fix-up)
            const unsigned wo = (unsigned)(c.ph * a.N + tn * TBN3 + 16 * wave + r_l) * (unsigned)(Ktot * 2) + swz_bytes(l, p);
            c.wo0 = live ? wo : W_DEAD;
        } else {
            const int g0 = pack_geo(a, aux, tm * TBM3 + 16 * wave + r_l), g1 = pack_geo(a, aux, tm * TBM3 + 16 * (wave + 8) + r_l);
            c.gx0 = live ? g0 : -1;
            c.gx1 = live ? g1 : -1;
            const unsigned wo = (unsigned)(tn * TBN3 + 16 * wave + r_l) * (unsigned)(Ktot * 2) + swz_bytes(l, p);
            c.wo0 = live ? wo : W_DEAD;
        }
        c.ikc = 0; c.ksw = 0; c.ky = 0; c.kx = 0;
        c.kend = ke;
        if constexpr (SPLIT) {                                     // a slice may start in the middle of a tap
            int tap = fdiv(kb, aux.kpt_d);
            c.ikc = kb - tap * kpt;
            c.ksw = kb;
            if constexpr (UP2F) {
                c.ky = tap >> 1; c.kx = tap & 1;
                c.xo0 = tap_src_up2f(a, aux, c.gx0, c.ky, c.kx, c.ph, swz_bytes(l, p));
                c.xo1 = tap_src_up2f(a, aux, c.gx1, c.ky, c.kx, c.ph, swz_bytes(l, p));
            } else {
                if (a.mode == MOFA_MODE_CONV3X3) { c.ky = fdiv(tap, aux.ks_d); c.kx = tap - c.ky * tg.ks; } else c.ky = tap;
                c.xo0 = tap_src(a, aux, tg, c.gx0, c.ky, c.kx, swz_bytes(l, p));
                c.xo1 = tap_src(a, aux, tg, c.gx1, c.ky, c.kx, swz_bytes(l, p));
            }
        }
    };
    auto issue = [&](Cursor3& c, const int p, const int slot) __attribute__((always_inline)) {
        if (c.ikc == 0) {
            const int l = lane_now(lane);
            if constexpr (UP2F) {
                c.xo0 = tap_src_up2f(a, aux, c.gx0, c.ky, c.kx, c.ph, swz_bytes(l, p));
                c.xo1 = tap_src_up2f(a, aux, c.gx1, c.ky, c.kx, c.ph, swz_bytes(l, p));
            } else {
                c.xo0 = tap_src(a, aux, tg, c.gx0, c.ky, c.kx, swz_bytes(l, p));
                c.xo1 = tap_src(a, aux, tg, c.gx1, c.ky, c.kx, swz_bytes(l, p));
            }
        }
        char* pl = smem + slot + p * PLANE;
        const int wk = c.ksw * 128;
        bglds16(rsx, c.xo0, c.ikc * 128, pl + wave * 1024);
        bglds16(rsx, c.xo1, c.ikc * 128, pl + (wave + 8) * 1024);
        bglds16(rsw, c.wo0, wk, pl + XPL + wave * 1024);
        bglds16(rsw, c.wo0 + wd1, wk, pl + XPL + (wave + 8) * 1024);
        if (grp == p) bglds16(rsw, c.wo0 + wd2, wk, pl + XPL + (16 + (wave & 3)) * 1024);
    };
    auto advance = [&](Cursor3& c, const int p) __attribute__((always_inline)) {
        if constexpr (UP2F) tap_advance_up2f(c, kpt); else tap_advance(c, a, kpt, tg.ks);
        if (c.ksw == c.kend) { next_pos(c.phase, c.local); cur_setup(c, p); }
    };

    // ---- consumer side ----------------------------------------------------------------------------------------------
    // fragment read addresses of ring slot 0, plane 0 (fragment and plane are immediates, the ring slot is added / subtracted
    // per K tile).  A plane is one 16x16x32 K step: lane l reads chunk l >> 4 of X row l & 15 of a 16-row fragment, and of the W
    // row with bits 2 and 3 of l & 15 SWAPPED (16 v + 8 ((a >> 2) & 1) + 4 (a >> 3) + (a & 3) for A row a): with that row order
    // the accumulators return to the 32x32 layout by lane-row swaps alone (see to_layout32 below)
    int xa, wa;
    {
        const int r = lane & 15, c = lane >> 4;
        const int rw = 8 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3);
        xa = (wm * MI3 * 32 + r) * RBH + (c ^ slot_swz((r >> 2) & 3)) * 16;
        wa = XPL + (wn * NJ3 * 32 + rw) * RBH + (c ^ slot_swz((rw >> 2) & 3)) * 16;
    }

    // The wave's 160 bias values travel through LDS one tile AHEAD: three 4-byte-per-lane LDS-DMA instructions issued at the
    // start of tile t bring tile t + 1's bias (columns beyond N read as zero through the descriptor's bounds check; no bias: an
    // empty descriptor, zeros arrive), landed long before tile t + 1 starts (every phase's counted wait covers them), so the
    // accumulator initialisation is 10 LDS reads with no VMEM operation queued behind the previous epilogue's stores.  (The
    // first version loaded the bias straight from global memory at tile start; tools/bias_probe.py shows no measurable
    // difference between the two, nor between bias and no bias -- its first reading, "bias costs 15 %", was the slower first
    // measurement after fresh allocations.)
    const BufRsrc rsb = buf_rsrc(a.bias, a.bias ? (unsigned)a.N * 4u : 0u);
    char* bias_lds = smem + BIAS0 + wave * 1536;
    auto bias_prefetch = [&](int phase_, int local_, int slot) __attribute__((always_inline)) {
        if (phase_ != 0) return;                                   // (a split-K item starts from zero; past the end: nothing)
        int tile_, kb_, ke_;
        item_decode(phase_, local_, tile_, kb_, ke_);
        const int tm_ = fdiv(tile_, aux.tiles_n), tn_ = tile_ - tm_ * tilesN;
        const unsigned n0 = (unsigned)(tn_ * TBN3 + wn * NJ3 * 32 + lane_now(lane));
#pragma unroll
        for (int k = 0; k < 3; ++k)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsb, (__attribute__((address_space(3))) void*)(bias_lds + slot * 768 + k * 256), 4,
                                                     (n0 + 64u * k) * 4u, 0, 0, 0);
    };

    Cursor3 ca, cb;                                                // plane 0 stream, plane 1 stream
    ca.local = cb.local = walk.local;
    ca.phase = cb.phase = walk.local < walk.count ? 0 : 1;     // (no whole tile: the workgroup was kept for its split-K item)
    cur_setup(ca, 0);
    cur_setup(cb, 1);
    // prologue: the first tile's bias, K tile 0 complete, plane 0 of K tile 1
    bias_prefetch(walk.local < walk.count ? 0 : 1, walk.local, 0);
    issue(ca, 0, 0); advance(ca, 0);
    issue(cb, 1, 0); advance(cb, 1);
    issue(ca, 0, SLOT); advance(ca, 0);
    wait_vmcnt_only<LOOKAHEAD3>();                                 // plane 0 of K tile 0 has landed
    __builtin_amdgcn_s_barrier();

    f32x16 acc[MI3][NJ3];
    // The K loop runs on 16x16x32 MFMAs (the chip holds a higher clock on them than on 32x32x16 at the same matrix-pipe cycles:
    // profiles/igemm320_k16_loop_bench.log).  The 16x16 tile with row half u and column half v of 32x32 block (I, J) lives in
    // elements 4 (2 v + u) .. + 3 of acc[I][J]; its MFMA takes X fragment 2 I + u and W fragment 2 J + v.
    f16x8 xf[2 * MI3], wf[2 * NJ3];
    auto phase = [&](auto pc, const int bo, const int bn) __attribute__((always_inline)) {
        constexpr int P = decltype(pc)::v;                         // K half
#pragma unroll
        for (int i = 0; i < 2 * MI3; ++i) xf[i] = *(const f16x8*)(smem + xa + P * PLANE + i * 16 * RBH);
#pragma unroll
        for (int j = 0; j < 2 * NJ3; ++j) wf[j] = *(const f16x8*)(smem + wa + P * PLANE + j * 16 * RBH);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (P == 0) { issue(cb, 1, bn); advance(cb, 1); }   // plane 1 of the next K tile
        else { issue(ca, 0, bo); advance(ca, 0); }                    // plane 0 of the K tile after it (this slot)
        // DMA older than the last two phases has landed (read from the next phase on); this phase's fragment reads have
        // returned BEFORE the barrier, so their plane may be refilled from the next phase on
        wait_vmcnt<LOOKAHEAD3>();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < MI3; ++i)
#pragma unroll
            for (int j = 0; j < NJ3; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {                      // q = 2 v + u
                    f32x4 c = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[2 * j + (q >> 1)], xf[2 * i + (q & 1)], c, 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] = c[e];
                }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };

    // ---- back to the 32x32 layout, once per tile / split-K item ---------------------------------------------------------------
    // A 16x16x32 result has its column on l & 15 and row 4 (l >> 4) + r in register r.  With lane l = (c = l & 15, g0 = (l >> 4) & 1,
    // g1 = l >> 5), A row a = 8 g1 + 4 g0 + r was loaded from W row 16 v + 8 g0 + 4 g1 + r (bits 2 and 3 swapped), so element
    // 4 (2 v + u) + r of a block holds output row m = 16 u + c, column n = 16 v + 8 g0 + 4 g1 + r.  The 32x32 layout wants element
    // 4 G + r of lane (c, bit 4 = u', bit 5 = h) to be m = 16 u' + c, n = 8 G + 4 h + r: h = g1 (lane bit 5 stays), G = 2 v + g0,
    // u' = u.  Where u = g0 the value is in place; the others are element 8 v + r in the odd 16-lane rows (u = 0 held by g0 = 1,
    // wanted at element 8 v + 4 + r of lane bit 4 = 0) and element 8 v + 4 + r in the even rows (u = 1 held by g0 = 0, wanted at
    // element 8 v + r of lane bit 4 = 1): v_permlane16_swap_b32, which exchanges the odd rows of its first operand with the even
    // rows of its second.  8 swaps per block, 80 per tile and wave, in place; afterwards register r of tile (i, j) is row
    // 32 i + (l & 31), column 32 j + 8 (r >> 2) + 4 (l >> 5) + (r & 3), as every epilogue below expects.
    auto to_layout32 = [&](f32x16 (&acc)[MI3][NJ3]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MI3; ++i)
#pragma unroll
            for (int j = 0; j < NJ3; ++j)
#pragma unroll
                for (int v = 0; v < 2; ++v)
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        // (scalar copies: __builtin_bit_cast applied to a vector ELEMENT reads element 0 of the vector)
                        const float lo = acc[i][j][8 * v + s], hi = acc[i][j][8 * v + 4 + s];
                        const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi), false, false);
                        const unsigned slo = sw[0], shi = sw[1];
                        acc[i][j][8 * v + s] = __builtin_bit_cast(float, slo);
                        acc[i][j][8 * v + 4 + s] = __builtin_bit_cast(float, shi);
                    }
    };

    // (every block is ONE 16-register tuple at the points where this is called -- after the initial values, around the swaps --
    // so that the register allocator keeps the 160 accumulators in place as ten tuples instead of 160 separately split values)
    auto pin_tuples = [&](f32x16 (&acc)[MI3][NJ3]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MI3; ++i)
#pragma unroll
            for (int j = 0; j < NJ3; ++j) asm volatile("" : "+v"(acc[i][j]));
    };

    // ---- epilogue scratch: the ring plane that is FREE while an epilogue runs ---------------------------------------------
    // When a tile's K loop ends, the ring holds the next tile's K tile 0 (other slot, both planes) and plane 0 of its K tile 1
    // (this slot); plane 1 of the last K tile's slot was read for the last time in the final phase and is refilled only by
    // phase 0 of the NEXT tile -- by every wave into its own pieces.  Each wave therefore transposes through the four 1 KB
    // blocks it will DMA into itself (X pieces w, w + 8 and W pieces w, w + 8 of that plane: 8 KB apart): 32 rows x 128 B,
    // rows 8 b .. 8 b + 7 in block b.  No other wave touches those blocks before its fragment reads two barriers later, the
    // wave's own DMA is issued after its epilogue (program order, lgkmcnt(0) at the end), and no barrier is needed.
    const ScratchRows srow;
    // register r of accumulator tile (i, j) is row 32 i + l31, column 32 j + 8 (r >> 2) + 4 lh + (r & 3)
    // ---- no residual, no per-row vector: activation in the fragment layout, fp16; two accumulator tiles (64 columns) per
    //      transpose so that a store instruction covers 8 whole 128-byte rows.  The wave's 160 columns start at byte 0 (wn = 0)
    //      or 320 (wn = 1) of a 640-byte-aligned row: the pairs are (0,1) (2,3) + tile 4, or tile 0 + (1,2) (3,4), so that
    //      every pair starts on a 128-byte boundary -----------------------------------------------------------------------------
    auto epilogue_light = [&](auto ac, auto wnc, f32x16 (&acc)[MI3][NJ3], const int mw, const int nw, char* eb) __attribute__((always_inline)) {
        constexpr int J0 = decltype(wnc)::v ? 1 : 0;   // first tile of the first pair
        constexpr int JS = decltype(wnc)::v ? 0 : 4;                 // the tile without a partner
        const int lane_e = lane_now(lane);                         // (lane-derived offsets are not kept live across the K loop)
        const int lane = lane_e, l31 = lane & 31, lh = lane >> 5;
        f16* out = (f16*)a.out;
        float saccv = a.s_acc;                                     // VGPR operand on purpose (see igemm.hip's epilogue)
        asm volatile("" : "+v"(saccv));
        char* wr = eb + srow(l31);
#pragma unroll
        for (int i = 0; i < MI3; ++i) {
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {                       // the two pairs
                const int j0 = J0 + 2 * pr;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f16x4 o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (f16)act_apply(ac, saccv * acc[i][j0 + jj][4 * g + e]);
                        const int c8 = 8 * jj + 2 * g + lh;
                        *(f16x4*)h16_off(wr, l31, c8) = o;
                    }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const H16Piece r = h16_row<8>(eb, srow, lane, p);
                    const int mr = mw + 32 * i + r.row, n = nw + 32 * j0 + 8 * r.blk;
                    if constexpr (UP2F) {                          // tile row -> output row (-1: padding row)
                        const int orow = up2f_out_row(a, aux, mr);
                        if (orow >= 0 && n + 8 <= a.N) *(f16x8*)(out + (size_t)orow * a.ldo + n) = r.v;
                    } else if (mr < a.M && n + 8 <= a.N) {
                        *(f16x8*)(out + (size_t)mr * a.ldo + n) = r.v;
                    }
                }
            }
            {                                                      // the single tile: 32 columns per row
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f16x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (f16)act_apply(ac, saccv * acc[i][JS][4 * g + e]);
                    const int c8 = 2 * g + lh;
                    *(f16x4*)h16_off(wr, l31, c8) = o;
                }
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const H16Piece r = h16_row<4>(eb, srow, lane, p);
                    const int mr = mw + 32 * i + r.row, n = nw + 32 * JS + 8 * r.blk;
                    if constexpr (UP2F) {
                        const int orow = up2f_out_row(a, aux, mr);
                        if (orow >= 0 && n + 8 <= a.N) *(f16x8*)(out + (size_t)orow * a.ldo + n) = r.v;
                    } else if (mr < a.M && n + 8 <= a.N) {
                        *(f16x8*)(out + (size_t)mr * a.ldo + n) = r.v;
                    }
                }
            }
        }
        wait_lds();
    };
    // ---- residual(s) without a per-row vector (r04): the light epilogue's fp16 pair transposes -- whole 128-byte lines per store,
    //      half the LDS traffic of the fp32 32 x 32 transposes of epilogue_rows below -- and the residual(s) added in the ROW
    //      layout afterwards: a lane holds 8 consecutive columns of one row, i.e. exactly one 16-byte residual load.  The
    //      accumulator is rounded to fp16 BEFORE the add, which is what the reference's fp16 modules do (the layer's output in
    //      fp16, then `+`); with one residual and s1 == 1 (every residual add of the networks except the AlphaBlender mixes) the
    //      add is 4 v_pk_add_f16 per 8 outputs.  A ring of D residual pieces is in flight ahead of the transposes. --------------
    auto epilogue_res16 = [&](auto wnc, auto unit, f32x16 (&acc)[MI3][NJ3], const int mw, const int nw, char* eb) __attribute__((always_inline)) {
        constexpr int J0 = decltype(wnc)::v ? 1 : 0;   // first tile of the first pair
        constexpr int JS = decltype(wnc)::v ? 0 : 4;                 // the tile without a partner
        constexpr bool UNIT = decltype(unit)::v != 0;                // one residual, s1 == 1: packed fp16 adds
        constexpr int PPI = 10, NP = MI3 * PPI;       // store pieces (16 bytes per lane) per row tile / per tile
        const int lane_e = lane_now(lane);
        const int lane = lane_e, l31 = lane & 31, lh = lane >> 5;
        f16* out = (f16*)a.out;
        const f16* r1 = (const f16*)a.r1;
        const f16* r2 = (const f16*)a.r2;
        float s1v = a.s1, s2v = a.s2, saccv = a.s_acc;
        asm volatile("" : "+v"(s1v), "+v"(s2v), "+v"(saccv));
        // piece q of row tile i: q < 8 -> pair q / 4, rows 8 (q % 4) + lane / 8, columns 8 (lane % 8) of the pair's 64;
        //                       q >= 8 -> the single tile, rows 16 (q - 8) + lane / 4, columns 8 (lane % 4) of its 32
        auto piece_pos = [&](int st, int& mr, int& n) __attribute__((always_inline)) {
            const int i = st / PPI, q = st % PPI;
            if (q < 8) {
                mr = mw + 32 * i + 8 * (q & 3) + (lane >> 3);
                n = nw + 32 * (J0 + 2 * (q >> 2)) + 8 * (lane & 7);
            } else {
                mr = mw + 32 * i + 16 * (q - 8) + (lane >> 2);
                n = nw + 32 * JS + 8 * (lane & 3);
            }
        };
        constexpr int D = (R1 && R2) ? 2 : 5;
        f16x8 L1[D], L2[D];
        auto piece_loads = [&](int st, int slot) __attribute__((always_inline)) {
            int mr, n;
            piece_pos(st, mr, n);
            mr = mr < a.M ? mr : a.M - 1;
            n = n + 8 <= a.N ? n : 0;
            if (R1) L1[slot] = *(const f16x8*)(r1 + (size_t)mr * a.ldr1 + n);
            if (R2) L2[slot] = *(const f16x8*)(r2 + (size_t)mr * a.ldr2 + n);
        };
#pragma unroll
        for (int st = 0; st < D; ++st) piece_loads(st, st);
        auto finish = [&](int st, f16x8 o) __attribute__((always_inline)) {
            int mr, n;
            piece_pos(st, mr, n);
            if constexpr (UNIT) {
                o = o + L1[st % D];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float x = (float)o[e];
                    if (R1) x += s1v * (float)L1[st % D][e];
                    if (R2) x += s2v * (float)L2[st % D][e];
                    o[e] = (f16)x;
                }
            }
            if (mr < a.M && n + 8 <= a.N) *(f16x8*)(out + (size_t)mr * a.ldo + n) = o;
            if (st + D < NP) piece_loads(st + D, st % D);           // refill the ring slot just consumed
        };
        char* wr = eb + srow(l31);
#pragma unroll
        for (int i = 0; i < MI3; ++i) {
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {                       // the two pairs
                const int j0 = J0 + 2 * pr;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f16x4 o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (f16)(saccv * acc[i][j0 + jj][4 * g + e]);
                        const int c8 = 8 * jj + 2 * g + lh;
                        *(f16x4*)h16_off(wr, l31, c8) = o;
                    }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const H16Piece r = h16_row<8>(eb, srow, lane, p);
                    finish(i * PPI + pr * 4 + p, r.v);
                }
            }
            {                                                      // the single tile: 32 columns per row
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f16x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (f16)(saccv * acc[i][JS][4 * g + e]);
                    const int c8 = 2 * g + lh;
                    *(f16x4*)h16_off(wr, l31, c8) = o;
                }
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const H16Piece r = h16_row<4>(eb, srow, lane, p);
                    finish(i * PPI + 8 + p, r.v);
                }
            }
        }
        wait_lds();
    };
    // ---- STATS kernels: epilogue_res16 (or its residual-free form) with the store pieces walked COLUMN SET by column set -- the
    //      tile pairs (J0, J0 + 1), (J0 + 2, J0 + 3), then the single tile, each over both row tiles -- so that only one set's
    //      accumulators (4 column pairs x {sum, sum of squares}) are live at a time (a residual is added in fp16: s1 == 1 only).  A finished piece is 8 consecutive fp16
    //      outputs of one row: 2 x 4 v_dot2_f32_f16 add the pairs and their squares; after a set, xor-shuffles over the lanes that
    //      hold the same columns (8 rows each -> the wave's 64 rows), and lanes 0-7 (0-3) write 32 bytes each:
    //      stats[(m / 64) * N + n .. n + 7] = {s, q} x 4 pairs.  Fixed order: bit-identical run to run. -------------------------
    auto epilogue_stats = [&](auto wnc, f32x16 (&acc)[MI3][NJ3], const int mw, const int nw, char* eb) __attribute__((always_inline)) {
        constexpr int J0 = decltype(wnc)::v ? 1 : 0, JS = decltype(wnc)::v ? 0 : 4;
        constexpr int NP = 20;                                       // pieces: 2 sets x 2 row tiles x 4, then 2 row tiles x 2
        const int lane_e = lane_now(lane);
        const int lane = lane_e, l31 = lane & 31, lh = lane >> 5;
        f16* out = (f16*)a.out;
        const f16* r1 = (const f16*)a.r1;
        float saccv = a.s_acc;
        asm volatile("" : "+v"(saccv));
        auto piece_pos = [&](int st, int& mr, int& n) __attribute__((always_inline)) {
            if (st < 16) {                                           // set st / 8, row tile (st / 4) % 2, piece st % 4
                mr = mw + 32 * ((st >> 2) & 1) + 8 * (st & 3) + (lane >> 3);
                n = nw + 32 * (J0 + 2 * (st >> 3)) + 8 * (lane & 7);
            } else {                                                 // the single tile: row tile (st - 16) / 2, piece (st - 16) % 2
                mr = mw + 32 * ((st - 16) >> 1) + 16 * ((st - 16) & 1) + (lane >> 2);
                n = nw + 32 * JS + 8 * (lane & 3);
            }
        };
        constexpr int D = 5;                                         // residual pieces in flight ahead of the transposes
        f16x8 L1[D];
        auto piece_loads = [&](int st, int slot) __attribute__((always_inline)) {
            int mr, n;
            piece_pos(st, mr, n);
            mr = mr < a.M ? mr : a.M - 1;
            L1[slot] = *(const f16x8*)(r1 + (size_t)mr * a.ldr1 + n);
        };
        if constexpr (R1) {
#pragma unroll
            for (int st = 0; st < D; ++st) piece_loads(st, st);
        }
        float S[4], Q[4];
        const f16x2 one2 = {(f16)1.0f, (f16)1.0f};
        auto finish = [&](int st, f16x8 o) __attribute__((always_inline)) {
            int mr, n;
            piece_pos(st, mr, n);
            if constexpr (R1) o = o + L1[st % D];                   // (s1 == 1: the residual add in fp16, as the reference's modules)
            if (mr < a.M) *(f16x8*)(out + (size_t)mr * a.ldo + n) = o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f16x2 h = {o[2 * k], o[2 * k + 1]};
                S[k] = __builtin_amdgcn_fdot2(h, one2, S[k], false);
                Q[k] = __builtin_amdgcn_fdot2(h, h, Q[k], false);
            }
            // (pins the eight v_dot2 HERE: left alone the compiler sinks them to the end of the column set and keeps all eight
            // pieces' outputs -- 32 registers -- live until then, which spills)
            asm volatile("" : "+v"(S[0]), "+v"(S[1]), "+v"(S[2]), "+v"(S[3]), "+v"(Q[0]), "+v"(Q[1]), "+v"(Q[2]), "+v"(Q[3]));
            if constexpr (R1) {
                if (st + D < NP) piece_loads(st + D, st % D);       // refill the ring slot just consumed
            }
        };
        auto reduce_store = [&](const int from, const int n0, const bool writer) __attribute__((always_inline)) {
            // (ds_bpermute addressed from the laundered lane id: __shfl_xor's own lane id is loop invariant, gets hoisted out of the
            // tile loop and then lives -- spilled -- across the K loop)
#pragma unroll
            for (int o = from; o < 64; o <<= 1) {
                const int src = (lane ^ o) << 2;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    S[k] += __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, S[k])));
                    Q[k] += __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, Q[k])));
                }
            }
            if (writer && mw < a.M) {                                // (M % 64 == 0: the wave's 64 rows are all inside or all outside)
                float* sp = a.stats + (size_t)(mw >> 6) * a.N + n0;
                *(f32x4*)sp = (f32x4){S[0], Q[0], S[1], Q[1]};
                *(f32x4*)(sp + 4) = (f32x4){S[2], Q[2], S[3], Q[3]};
            }
        };
        char* wr = eb + srow(l31);
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {                           // the two pairs
            const int j0 = J0 + 2 * pr;
#pragma unroll
            for (int k = 0; k < 4; ++k) { S[k] = 0.f; Q[k] = 0.f; }
#pragma unroll
            for (int i = 0; i < MI3; ++i) {
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f16x4 o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (f16)(saccv * acc[i][j0 + jj][4 * g + e]);
                        const int c8 = 8 * jj + 2 * g + lh;
                        *(f16x4*)h16_off(wr, l31, c8) = o;
                    }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const H16Piece r = h16_row<8>(eb, srow, lane, p);
                    finish(pr * 8 + i * 4 + p, r.v);
                }
            }
            reduce_store(8, nw + 32 * j0 + 8 * (lane & 7), lane < 8);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { S[k] = 0.f; Q[k] = 0.f; }
#pragma unroll
        for (int i = 0; i < MI3; ++i) {                            // the single tile: 32 columns per row
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (f16)(saccv * acc[i][JS][4 * g + e]);
                const int c8 = 2 * g + lh;
                *(f16x4*)h16_off(wr, l31, c8) = o;
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const H16Piece r = h16_row<4>(eb, srow, lane, p);
                finish(16 + i * 2 + p, r.v);
            }
        }
        reduce_store(4, nw + 32 * JS + 8 * (lane & 3), lane < 4);
        wait_lds();
    };
    // ---- GEGLU pair kind: the weight rows are interleaved in blocks of 16 (weights.interleave_geglu), so accumulator tile j
    //      holds the value columns of outputs 16 j .. 16 j + 15 in registers 0-7 and the matching gate columns in registers
    //      8-15 of the SAME lane: the product is lane-local and a wave's NJ3 tiles give 16 NJ3 output columns (80 of the tile's
    //      160).  out = s_acc * val * gelu(s_acc * gate), erf GELU as x * Phi(x) (common.h).  Tiles 0-3 (64 output columns)
    //      go through one 32 x 64 fp16 transpose and whole 128-byte row pieces, tile 4 (16 columns) through a second one ------
    auto epilogue_geglu = [&](auto s1c, f32x16 (&acc)[MI3][NJ3], const int mw, const int nw, char* eb) __attribute__((always_inline)) {
        constexpr bool SACC1 = decltype(s1c)::v != 0;              // s_acc == 1: the multiplies drop out
        const int lane_e = lane_now(lane);
        const int lane = lane_e, l31 = lane & 31, lh = lane >> 5;
        f16* out = (f16*)a.out;
        float saccv = a.s_acc;
        asm volatile("" : "+v"(saccv));
        const int nout = a.N / 2, no0 = nw / 2;                    // first output column of this wave
        char* wr = eb + srow(l31);
        auto product = [&](int i, int j, int g) __attribute__((always_inline)) -> f16x4 {
            f16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float val = acc[i][j][4 * g + e], gate = acc[i][j][8 + 4 * g + e];
                if constexpr (SACC1) o[e] = (f16)(val * (gate * gelu_phi_f(gate)));
                else o[e] = (f16)(saccv * val * gelu_erf_f(saccv * gate));
            }
            return o;
        };
#pragma unroll
        for (int i = 0; i < MI3; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const int c8 = 4 * j + 2 * g + lh;             // 8-byte chunk (4 columns) of the 64-column row
                    *(f16x4*)h16_off(wr, l31, c8) = product(i, j, g);
                }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const H16Piece r = h16_row<8>(eb, srow, lane, p);
                const int mr = mw + 32 * i + r.row, n = no0 + 8 * r.blk;
                if (mr < a.M && n + 8 <= nout) *(f16x8*)(out + (size_t)mr * a.ldo + n) = r.v;
            }
            {                                                      // tile 4: 16 columns per row
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const int c8 = 2 * g + lh;
                    *(f16x4*)h16_off(wr, l31, c8) = product(i, 4, g);
                }
                const H16Piece r = h16_row<2>(eb, srow, lane, 0);
                const int mr = mw + 32 * i + r.row, n = no0 + 64 + 8 * r.blk;
                if (mr < a.M && n + 8 <= nout) *(f16x8*)(out + (size_t)mr * a.ldo + n) = r.v;
            }
        }
        wait_lds();
    };
    // ---- residuals and / or a per-row vector: 32 x 32 fp32 transposes; a lane owns 8 consecutive
    //      columns of one row.  The loads of step s + D are issued before step s is processed (ring of D steps in registers) ----
    auto epilogue_rows = [&](auto un, f32x16 (&acc)[MI3][NJ3], const int mw, const int nw, char* eb) __attribute__((always_inline)) {
        constexpr bool RVROW = RV && decltype(un)::v == 0;         // the row vector was NOT folded into the accumulators
        constexpr int STEPS = MI3 * NJ3;                           // (i, j): one accumulator tile per step
        const int lane_e = lane_now(lane);
        const int lane = lane_e, l31 = lane & 31, lh = lane >> 5;
        f16* out = (f16*)a.out;
        const f16* r1 = (const f16*)a.r1;
        const f16* r2 = (const f16*)a.r2;
        float s1v = a.s1, s2v = a.s2, saccv = a.s_acc;
        asm volatile("" : "+v"(s1v), "+v"(s2v), "+v"(saccv));
        int rv_div = a.rv_div, rv_mod_in = a.rv_mod_in, rv_mod_out = a.rv_mod_out;
        asm volatile("" : "+s"(rv_div), "+s"(rv_mod_in), "+s"(rv_mod_out));
        const int piece = lane & 3, rrow = lane >> 2;
        // ring of D steps of loads in registers (8 VGPRs per residual, 16 for a per-row vector): the epilogue of a shallow-K
        // launch is bound by the latency of exactly these loads
        constexpr int REGS = (R1 ? 8 : 0) + (R2 ? 8 : 0) + (RVROW ? 16 : 0);
        constexpr int D = RVROW ? 1 : (REGS <= 8 ? 6 : 3);       // (the per-row vector path is rare: tiles that straddle a frame)
        struct StepLoads { f16x8 t1[2], t2[2]; f32x4 rv0[2], rv1[2]; };
        StepLoads L[D];
        auto step_loads = [&](int st, StepLoads& l) __attribute__((always_inline)) {
            const int i = st / NJ3, j = st % NJ3;
            const int n = nw + 32 * j + 8 * piece;
            const int nc = n + 8 <= a.N ? n : 0;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                int m = mw + 32 * i + 16 * p + rrow;
                m = m < a.M ? m : a.M - 1;
                if (R1) l.t1[p] = *(const f16x8*)(r1 + (size_t)m * a.ldr1 + nc);
                if (R2) l.t2[p] = *(const f16x8*)(r2 + (size_t)m * a.ldr2 + nc);
                if (RVROW) {
                    const int idx = ((m / rv_div) * a.rv_mul + (m % rv_mod_in)) % rv_mod_out;
                    const float* q = a.rowvec + (size_t)idx * a.N + nc;
                    l.rv0[p] = *(const f32x4*)q;
                    l.rv1[p] = *(const f32x4*)(q + 4);
                }
            }
        };
#pragma unroll
        for (int st = 0; st < D; ++st) step_loads(st, L[st]);
        char* wr = eb + srow(l31);
        const int wsw = ((l31 >> 1) & 3) | ((l31 & 1) << 2);
#pragma unroll
        for (int st = 0; st < STEPS; ++st) {
            const int i = st / NJ3, j = st % NJ3;
            StepLoads& l = L[st % D];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * g + e];
                *(f32x4*)(wr + (((2 * g + lh) ^ wsw) << 4)) = v;
            }
            const int n = nw + 32 * j + 8 * piece;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int row = 16 * p + rrow;
                const int rsw = ((row >> 1) & 3) | ((row & 1) << 2);
                const f32x4 v0 = *(const f32x4*)(eb + srow(row) + (((2 * piece) ^ rsw) << 4));
                const f32x4 v1 = *(const f32x4*)(eb + srow(row) + (((2 * piece + 1) ^ rsw) << 4));
                f16x8 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x0 = v0[e], x1 = v1[e];
                    if (RVROW) { x0 += l.rv0[p][e]; x1 += l.rv1[p][e]; }
                    x0 *= saccv; x1 *= saccv;
                    // (with residuals the layer's own output is rounded to fp16 BEFORE the add, like epilogue_res16 and the
                    //  reference's fp16 modules: every tile of a launch rounds the same way -- round-4 advice)
                    if (R1 || R2) { x0 = (float)(f16)x0; x1 = (float)(f16)x1; }
                    if (R1) { x0 += s1v * (float)l.t1[p][e]; x1 += s1v * (float)l.t1[p][4 + e]; }
                    if (R2) { x0 += s2v * (float)l.t2[p][e]; x1 += s2v * (float)l.t2[p][4 + e]; }
                    o[e] = (f16)x0; o[4 + e] = (f16)x1;
                }
                const int m = mw + 32 * i + row;
                if (m < a.M && n + 8 <= a.N) *(f16x8*)(out + (size_t)m * a.ldo + n) = o;
            }
            if (st + D < STEPS) step_loads(st + D, L[st % D]);     // refill the ring slot just consumed
        }
        wait_lds();
    };

    // ---- split-K: the fp32 partial tile, row-major [256][TBN], through the same 32 x 32 fp32 transposes ------------------------
    auto epilogue_dump = [&](f32x16 (&acc)[MI3][NJ3], float* wst, char* eb) __attribute__((always_inline)) {
        const int lane_e = lane_now(lane);
        const int lane = lane_e, l31 = lane & 31, lh = lane >> 5;
        const int piece = lane & 3, rrow = lane >> 2;
        char* wr = eb + srow(l31);
        const int wsw = ((l31 >> 1) & 3) | ((l31 & 1) << 2);
#pragma unroll
        for (int st = 0; st < MI3 * NJ3; ++st) {
            const int i = st / NJ3, j = st % NJ3;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * g + e];
                *(f32x4*)(wr + (((2 * g + lh) ^ wsw) << 4)) = v;
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int row = 16 * p + rrow;
                const int rsw = ((row >> 1) & 3) | ((row & 1) << 2);
                const f32x4 v0 = *(const f32x4*)(eb + srow(row) + (((2 * piece) ^ rsw) << 4));
                const f32x4 v1 = *(const f32x4*)(eb + srow(row) + (((2 * piece + 1) ^ rsw) << 4));
                float* d = wst + (size_t)(wm * MI3 * 32 + 32 * i + row) * TBN3 + wn * NJ3 * 32 + 32 * j + 8 * piece;
                *(f32x4*)d = v0;
                *(f32x4*)(d + 4) = v1;
            }
        }
        wait_lds();
    };

    int gt = 0;                                                    // K tiles consumed so far (ring slot = gt & 1)
    int cph = walk.local < walk.count ? 0 : 1, cl = walk.local, bslot = 0;
    for (; cph < 2; next_pos(cph, cl), bslot ^= 1) {
        int tile, kb, ke;
        item_decode(cph, cl, tile, kb, ke);
        {                                                          // the NEXT tile's bias into the other slot
            int nph = cph, nl = cl;
            next_pos(nph, nl);
            bias_prefetch(nph, nl, bslot ^ 1);
        }
        const int tm = fdiv(tile, aux.tiles_n), tn = tile - tm * tilesN;
        const int mw = tm * TBM3 + wm * MI3 * 32;                  // first output row / column of this wave
        const int nw = tn * TBN3 + wn * NJ3 * 32;
        int idx_u = -1;                                            // >= 0: the one row-vector row of this wave's 64 rows
        if constexpr (RV) idx_u = rowvec_uniform_idx<32 * MI3>(a, mw);
        // accumulators start at bias (from its LDS slot) + the wave's row of the row vector, in the K loop's layout: elements
        // 8 v + 4 u .. + 3 of block (I, J) are columns 32 J + 16 v + 8 g0 + 4 g1 .. + 3 for both u and both I
        if (SPLIT && cph == 1) {
#pragma unroll
            for (int i = 0; i < MI3; ++i)
#pragma unroll
                for (int j = 0; j < NJ3; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
        } else {
            const int lane_e = lane_now(lane);
            const int col_e = 8 * ((lane_e >> 4) & 1) + 4 * (lane_e >> 5);
#pragma unroll
            for (int j = 0; j < NJ3; ++j)
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    f32x4 b = *(const f32x4*)(bias_lds + bslot * 768 + (32 * j + 16 * v + col_e) * 4);
                    if (RV && idx_u >= 0) {
                        int n = nw + 32 * j + 16 * v + col_e;
                        n = n + 4 <= a.N ? n : 0;                   // columns beyond N are never stored
                        b += *(const f32x4*)(a.rowvec + (size_t)idx_u * a.N + n);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[0][j][8 * v + e] = b[e]; acc[0][j][8 * v + 4 + e] = b[e];
                        acc[1][j][8 * v + e] = b[e]; acc[1][j][8 * v + 4 + e] = b[e];
                    }
                }
        }
        pin_tuples(acc);
        if (grp == 1) __builtin_amdgcn_s_barrier();                // second wave group runs one barrier behind
        for (int kt = kb; kt < ke; ++kt, ++gt) {
            const int bo = (gt & 1) * SLOT, bn = SLOT - bo;        // ring slot of this K tile / of the next one
            phase(IC<0>{}, bo, bn);
            phase(IC<1>{}, bo, bn);
            const int d = (gt & 1) ? -SLOT : SLOT;                 // the next K tile's ring slot
            xa += d;
            wa += d;
        }
        if (grp == 0) __builtin_amdgcn_s_barrier();                // both groups meet again: equal barrier counts per tile
        pin_tuples(acc);
        to_layout32(acc);
        pin_tuples(acc);

        // ---- epilogue (no barriers; scratch = this wave's blocks of the free ring plane) --------------------------------
        char* eb = smem + ((gt - 1) & 1) * SLOT + PLANE + wave * 1024;
        if (SPLIT && cph == 1) {
            epilogue_dump(acc, aux.ws + (size_t)blockIdx.x * (TBM3 * TBN3), eb);
        } else if constexpr (STATS) {                              // (kinds 0 / 1 / 4 / 5; the launcher excluded a per-row vector and s1 != 1)
            if (wn == 0) epilogue_stats(IC<0>{}, acc, mw, nw, eb);
            else epilogue_stats(IC<1>{}, acc, mw, nw, eb);
        } else if constexpr (GEGLU) {
            if (a.s_acc == 1.0f) epilogue_geglu(IC<1>{}, acc, mw, nw, eb);
            else epilogue_geglu(IC<0>{}, acc, mw, nw, eb);
        } else if constexpr (R1 || R2) {
            if (RV && idx_u < 0) {
                epilogue_rows(IC<0>{}, acc, mw, nw, eb);           // a per-row vector (tile straddles a frame): fp32 row path
            } else {                                               // (a uniform row-vector row is already in the accumulators)
                const bool unit = R1 && !R2 && a.s1 == 1.0f;
                if (wn == 0) {
                    if (unit) epilogue_res16(IC<0>{}, IC<1>{}, acc, mw, nw, eb);
                    else epilogue_res16(IC<0>{}, IC<0>{}, acc, mw, nw, eb);
                } else {
                    if (unit) epilogue_res16(IC<1>{}, IC<1>{}, acc, mw, nw, eb);
                    else epilogue_res16(IC<1>{}, IC<0>{}, acc, mw, nw, eb);
                }
            }
        } else if constexpr (UP2F) {                               // (plain kind, no activation: igemm_check_args)
            if (wn == 0) epilogue_light(IC<MOFA_ACT_NONE>{}, IC<0>{}, acc, mw, nw, eb);
            else epilogue_light(IC<MOFA_ACT_NONE>{}, IC<1>{}, acc, mw, nw, eb);
        } else if (RV && idx_u < 0) {
            epilogue_rows(IC<0>{}, acc, mw, nw, eb);
        } else if (wn == 0) {
            if (RV || a.act == MOFA_ACT_NONE) epilogue_light(IC<MOFA_ACT_NONE>{}, IC<0>{}, acc, mw, nw, eb);
            else if (a.act == MOFA_ACT_SILU) epilogue_light(IC<MOFA_ACT_SILU>{}, IC<0>{}, acc, mw, nw, eb);
            else if (a.act == MOFA_ACT_RELU) epilogue_light(IC<MOFA_ACT_RELU>{}, IC<0>{}, acc, mw, nw, eb);
            else epilogue_light(IC<MOFA_ACT_GELU>{}, IC<0>{}, acc, mw, nw, eb);
        } else {
            if (RV || a.act == MOFA_ACT_NONE) epilogue_light(IC<MOFA_ACT_NONE>{}, IC<1>{}, acc, mw, nw, eb);
            else if (a.act == MOFA_ACT_SILU) epilogue_light(IC<MOFA_ACT_SILU>{}, IC<1>{}, acc, mw, nw, eb);
            else if (a.act == MOFA_ACT_RELU) epilogue_light(IC<MOFA_ACT_RELU>{}, IC<1>{}, acc, mw, nw, eb);
            else epilogue_light(IC<MOFA_ACT_GELU>{}, IC<1>{}, acc, mw, nw, eb);
        }
    }
    // a wave must not retire with an LDS DMA in flight (the cursors' run-ahead past the last tile)
    wait_vmcnt_only<0>();
}

typedef void (*igemm320_kern_t)(const mofa_igemm_args, const int, const int, const Aux);

// split-K fix-up: out = act(s_acc * (sum over the K slices + bias + rowvec[idx(m)]) + s1 r1 + s2 r2) for the R remainder tiles,
// one thread per 8 output columns of a row; the slices are added in slice order (deterministic)
template <bool UP2F = false>
__global__ __launch_bounds__(256) void igemm320_fixup_kernel(const mofa_igemm_args a, const float* __restrict__ ws, const int tile0,
                                                             const int nsplit, const int tilesN, const int R) {
    constexpr int PPR = TBN3 / 8, PPT = TBM3 * PPR;   // pieces per row / per tile
    const long long total = (long long)R * PPT;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int r = (int)(idx / PPT), rem = (int)(idx - (long long)r * PPT);
        const int rr = rem / PPR, pc = rem - rr * PPR;
        const int tile = tile0 + r, tm = tile / tilesN, tn = tile - tm * tilesN;
        int m = tm * TBM3 + rr;
        const int n = tn * TBN3 + pc * 8;
        if constexpr (UP2F) {                                      // tile row -> output row (plain kind: no residual / row vector below)
            m = igemm_up2f_out_row(a, m);
            if (m < 0 || n + 8 > a.N) continue;
        } else if (m >= a.M || n + 8 > a.N) {
            continue;
        }
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
        for (int sl = 0; sl < nsplit; ++sl) {
            const float* q = ws + ((size_t)(r * nsplit + sl) * TBM3 + rr) * TBN3 + pc * 8;
            const f32x4 p0 = *(const f32x4*)q, p1 = *(const f32x4*)(q + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] += p0[e]; v[4 + e] += p1[e]; }
        }
        if (a.bias) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += a.bias[n + e];
        }
        if (a.rowvec) {
            const int idx_rv = ((m / a.rv_div) * a.rv_mul + (m % a.rv_mod_in)) % a.rv_mod_out;
            const float* q = a.rowvec + (size_t)idx_rv * a.N + n;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += q[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= a.s_acc;
        if (a.r1 || a.r2) {                                        // rounded to fp16 before the residual add, as in the whole tiles
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (float)(f16)v[e];
        }
        if (a.r1) {
            const f16x8 t = *(const f16x8*)((const f16*)a.r1 + (size_t)m * a.ldr1 + n);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += a.s1 * (float)t[e];
        }
        if (a.r2) {
            const f16x8 t = *(const f16x8*)((const f16*)a.r2 + (size_t)m * a.ldr2 + n);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += a.s2 * (float)t[e];
        }
        f16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float x = v[e];
            if (a.act == MOFA_ACT_SILU) x = silu_f(x);
            else if (a.act == MOFA_ACT_RELU) x = fmaxf(x, 0.0f);
            else if (a.act == MOFA_ACT_GELU) x = gelu_erf_f(x);
            o[e] = (f16)x;
        }
        *(f16x8*)((f16*)a.out + (size_t)m * a.ldo + n) = o;
    }
}

// STATS launches with a split-K last round: the remainder tiles get their outputs from the fix-up kernel, so their pair sums are
// taken from the finished outputs (R tiles x 4 row blocks; a few MB, L2 / MALL resident): one workgroup per (tile, 64-row block),
// one thread per column pair, rows in order
__global__ __launch_bounds__(192) void igemm320_tile_stats_kernel(const f16* __restrict__ out, const int ldo, float* __restrict__ stats,
                                                                  const int M, const int N, const int tile0, const int tilesN) {
    const int tile = tile0 + (int)(blockIdx.x >> 2), tm = tile / tilesN, tn = tile - tm * tilesN;
    const int m0 = tm * TBM3 + 64 * (int)(blockIdx.x & 3), n = tn * TBN3 + 2 * (int)threadIdx.x;
    if (m0 >= M || (int)threadIdx.x >= TBN3 / 2 || n + 2 > N) return;
    const f16x2 one2 = {(f16)1.0f, (f16)1.0f};
    float sm = 0.f, q = 0.f;
    const f16* p = out + (size_t)m0 * ldo + n;
#pragma unroll 8
    for (int r = 0; r < 64; ++r) {
        const f16x2 h = *(const f16x2*)(p + (size_t)r * ldo);
        sm = __builtin_amdgcn_fdot2(h, one2, sm, false);
        q = __builtin_amdgcn_fdot2(h, h, q, false);
    }
    float* sp = stats + (size_t)(m0 >> 6) * N + n;
    sp[0] = sm;
    sp[1] = q;
}

}  // namespace

// (kind 7 = row vector + two residuals does not fit the register file beside 160 accumulators and occurs nowhere in the
// model graph: it runs on the 4-wave tiles, igemm320_eligible in igemm_plan.h)
static const igemm320_kern_t k_igemm320[9] = {igemm320_f16_kernel<0>, igemm320_f16_kernel<1>, igemm320_f16_kernel<2>,
                                               igemm320_f16_kernel<3>, igemm320_f16_kernel<4>, igemm320_f16_kernel<5>,
                                               igemm320_f16_kernel<6>, nullptr, igemm320_f16_kernel<8>};
// the folded nearest-2x + 3x3 mode: plain kind, whole tiles / with a split-K item
static const igemm320_kern_t k_igemm320_up2f[2] = {igemm320_f16_kernel<0, false, false, true>, igemm320_f16_kernel<0, true, false, true>};
static const igemm320_kern_t k_igemm320_split[7] = {
    igemm320_f16_kernel<0, true>, igemm320_f16_kernel<1, true>, igemm320_f16_kernel<2, true>, igemm320_f16_kernel<3, true>,
    igemm320_f16_kernel<4, true>, igemm320_f16_kernel<5, true>, igemm320_f16_kernel<6, true>};

// STATS instantiations (GroupNorm pair sums from the epilogue): the kinds the networks' GroupNorm producers use -- plain (down-sampling
// conv), one residual (conv2 / the temporal conv2 / proj_out), uniform row vector (conv1 + time embedding), both
static const igemm320_kern_t k_igemm320_stats[7] = {igemm320_f16_kernel<0, false, true>, igemm320_f16_kernel<1, false, true>, nullptr,
                                                     nullptr, igemm320_f16_kernel<4, false, true>, igemm320_f16_kernel<5, false, true>, nullptr};
static const igemm320_kern_t k_igemm320_split_stats[7] = {igemm320_f16_kernel<0, true, true>, igemm320_f16_kernel<1, true, true>, nullptr,
                                                           nullptr, igemm320_f16_kernel<4, true, true>, igemm320_f16_kernel<5, true, true>, nullptr};

int igemm320_init() {
    return mofa_lds_optin(k_igemm320, LDS_BYTES3) == MOFA_OK && mofa_lds_optin(k_igemm320_split, LDS_BYTES3) == MOFA_OK &&
                   mofa_lds_optin(k_igemm320_up2f, LDS_BYTES3) == MOFA_OK &&
                   mofa_lds_optin(k_igemm320_stats, LDS_BYTES3) == MOFA_OK && mofa_lds_optin(k_igemm320_split_stats, LDS_BYTES3) == MOFA_OK
               ? MOFA_OK
               : MOFA_ELAUNCH;
}

// One launch, or with plan.split > 1 (igemm320_split, igemm_plan.h): the whole tiles of the full rounds, then one K slice of a
// remainder tile per workgroup; then the fix-up, and with stats the remainder tiles' pair sums from their finished outputs
static_assert(TBM3 == 256 && TBN3 == 320 && LDS_BYTES3 == 159744, "igemm_plan.h's MOFA_TILE_256X320 row");
int igemm320_launch(const mofa_igemm_args* a, const IgemmPlan& plan, hipStream_t stream) {
    const int kind = plan.kind, S = plan.split, R = plan.rem_tiles, tilesN = plan.tiles_n;
    Aux aux = igemm_pipe_aux(a, igemm_taps(*a), tilesN);
    const bool up2f = a->mode == MOFA_MODE_CONV3X3_UP2F;      // (kind 0, no stats: igemm_check_args)
    igemm320_kern_t kern = up2f ? k_igemm320_up2f[0] : a->stats ? k_igemm320_stats[kind] : k_igemm320[kind];
    if (S > 1) {
        kern = up2f ? k_igemm320_up2f[1] : a->stats ? k_igemm320_split_stats[kind] : k_igemm320_split[kind];
        aux.nsplit = S, aux.nsplit_d = fastdiv_make(S);
        aux.tile0 = plan.full_tiles, aux.nitems = R * S, aux.ws = (float*)a->workspace;
    }
    hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(plan.threads), plan.lds_bytes, stream, *a, tilesN, plan.full_tiles, aux);
    MOFA_CHECK_LAUNCH();
    if (S == 1) return MOFA_OK;
    const long long pieces = (long long)R * TBM3 * (TBN3 / 8);
    if (up2f)
        hipLaunchKernelGGL(igemm320_fixup_kernel<true>, dim3((int)((pieces + 255) / 256)), dim3(256), 0, stream, *a,
                           (const float*)a->workspace, plan.full_tiles, S, tilesN, R);
    else
        hipLaunchKernelGGL(igemm320_fixup_kernel<false>, dim3((int)((pieces + 255) / 256)), dim3(256), 0, stream, *a,
                       (const float*)a->workspace, plan.full_tiles, S, tilesN, R);
    MOFA_CHECK_LAUNCH();
    if (a->stats) {
        hipLaunchKernelGGL(igemm320_tile_stats_kernel, dim3(R * 4), dim3(192), 0, stream, (const f16*)a->out, a->ldo, a->stats, a->M,
                           a->N, plan.full_tiles, tilesN);
        MOFA_CHECK_LAUNCH();
    }
    return MOFA_OK;
}
