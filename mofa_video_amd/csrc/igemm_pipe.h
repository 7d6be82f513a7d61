// Pieces shared by the two 8-wave phase-pipelined implicit-GEMM kernels (igemm8.hip: 256x256 tile, igemm320.hip: 256x320
// tile).  Device side: magic-number division, the launch-invariant scalars (Aux), the laundered lane id, the packed row
// geometry of a DMA row group and its tap source, the buffer-descriptor LDS-DMA wrapper, the cursors' tap advance, the
// wave-uniform row-vector index, the activation and the epilogue's scratch images (32 x 64 fp16 with its row read-back, 32 x 32
// fp32).
// Host side: fastdiv_make and the set-up of Aux (eligibility: igemm_plan.h).
#pragma once
#include "igemm_common.h"

namespace {

// division by a launch-invariant divisor without v_rcp sequences (whose loop-invariant parts hipcc hoists out of the
// persistent loop and then spills): q = umulhi(n, mul) >> shr, exact for 0 <= n < 2^31 (host side: fastdiv_make)
struct FastDiv { unsigned mul, shr; };
__device__ __forceinline__ int fdiv(int n, const FastDiv d) { return d.mul ? (int)(__umulhi((unsigned)n, d.mul) >> d.shr) : n; }

struct Aux {                        // launch-invariant scalars computed by the launcher
    FastDiv tiles_n, hw, wout, t3hw, t3t;
    int ldxb;                       // activation row stride in bytes
    int row_shift;                  // rows between xbase and a.x (convT3 with caller-supplied halo frames: HW, else 0)
    const void* xbase;              // base of the activation buffer descriptor
    unsigned x_bytes, w_bytes;      // extents of the two buffer descriptors
    unsigned long long* trace;      // VAR & 64: [workgroup][group][16] cycle sums
    // split-K launches of igemm320.hip (remainder tiles of a partial last round): work item = (tile0 + item / nsplit, K slice
    // item % nsplit); fp32 partial tiles [item][256][320] go to ws
    FastDiv nsplit_d, kpt_d, ks_d;
    int nsplit, tile0, nitems;
    float* ws;
};

// One DMA row group = ONE packed register (Cursor::gx), decoded at every tap switch:
//   plain    m                                         conv     img << 20 | oy << 10 | ox
//   convT3   m | (frame > 0 or unclipped) << 29 | (frame < T - 1 or unclipped) << 30
//   -1       row beyond M
// DMA sources are addressed through BUFFER descriptors (buffer_load_dwordx4 ... lds): a 32-bit byte offset per lane, the
// K offset in an SGPR, no 64-bit address arithmetic -- and an offset beyond the descriptor's extent reads as ZERO, which
// is how rows of an out-of-image tap / beyond M / past the end of the tile walk are sourced (no zero page, no select).
constexpr unsigned XO_INVALID = 0xffffffffu;

template <int V> struct IC { static constexpr int v = V; };

// The lane id behind an empty asm: lane-derived values (LDS / global offsets, swizzles) are recomputed from it where they
// are used -- per tap / per tile -- instead of being hoisted out of the persistent tile loop, where they stay live across
// the K loop and get spilled to scratch (and reloaded in the epilogue, latency-bound).
__device__ __forceinline__ int lane_now(int lane) { asm volatile("" : "+v"(lane)); return lane; }

struct TapGeo {                         // conv: kernel size, dilation, tap origin (computed once per kernel)
    int ks, dil, org;
    __device__ __forceinline__ TapGeo(const mofa_igemm_args& a)
        : ks(a.ksize > 0 ? a.ksize : 3), dil(a.dil > 0 ? a.dil : 1), org(a.pad == MOFA_PAD_TRAILING ? 0 : (ks >> 1)) {}
};

// (pack_geo, tap_src: single exit -- with several return statements hipcc leaves the result slots in scratch memory)
__device__ __forceinline__ int pack_geo(const mofa_igemm_args& a, const Aux& aux, int m) {
    int g = m;
    if (a.mode == MOFA_MODE_CONV3X3) {
        const int img = fdiv(m, aux.hw), rem = m - img * (a.Hout * a.Wout);
        const int oy = fdiv(rem, aux.wout);
        g = (img << 20) | (oy << 10) | (rem - oy * a.Wout);
    } else if (a.mode == MOFA_MODE_CONVT3) {
        int lo = 1, hi = 1;
        if (a.T > 0) {
            const int fr = fdiv(m, aux.t3hw);                      // frame index; its position within the clip of T
            const int f = fr - fdiv(fr, aux.t3t) * a.T;
            lo = f > 0; hi = f < a.T - 1;
        }
        g = m | (lo << 29) | (hi << 30);
    }
    return m < a.M ? g : -1;
}

// source of row group g at tap (ky, kx) + the lane's swizzled chunk: bytes from aux.xbase
__device__ __forceinline__ unsigned tap_src(const mofa_igemm_args& a, const Aux& aux, const TapGeo& t, int g, int ky, int kx, int swzb) {
    int row = g;                                                   // plain: the output row itself
    bool ok = g >= 0;
    if (a.mode == MOFA_MODE_CONV3X3) {
        const int vy = ((g >> 10) & 1023) * a.stride + (ky - t.org) * t.dil;
        const int vx = (g & 1023) * a.stride + (kx - t.org) * t.dil;
        ok = ok && vy >= 0 && vx >= 0 && vy < a.Hin * a.up && vx < a.Win * a.up;
        const int iy = (a.up == 2) ? (vy >> 1) : vy, ix = (a.up == 2) ? (vx >> 1) : vx;
        row = ((g >> 20) * a.Hin + iy) * a.Win + ix;
    } else if (a.mode == MOFA_MODE_CONVT3) {                       // tap ky - 1 frames away
        ok = ok && !(ky == 0 && !((g >> 29) & 1)) && !(ky == 2 && !((g >> 30) & 1));
        row = (g & 0x1fffffff) + (ky - 1) * a.HW + aux.row_shift;
    }
    const unsigned off = (unsigned)row * (unsigned)aux.ldxb + (unsigned)swzb;
    return ok ? off : XO_INVALID;
}

// ---- MOFA_MODE_CONV3X3_UP2F (the nearest-2x up-sampling folded into 2x2 phase weights; template flag UP2F of the kernels) -------
// The instantiations of modes 0-2 call none of this and evaluate igemm_taps_classic, as before the mode existed.
template <bool UP2F>
__device__ __forceinline__ int kernel_taps(const mofa_igemm_args& a) {
    if constexpr (UP2F) return 4; else return igemm_taps_classic(a);
}
template <bool B, class T, class F> struct SelectT { typedef T type; };
template <class T, class F> struct SelectT<false, T, F> { typedef F type; };
template <class C> struct CursorUp2f : C { int ph; };     // a kernel's cursor + the phase 2 a + b of the row tile it is in
struct FDivBy { FastDiv d; __device__ __forceinline__ int operator()(int n) const { return fdiv(n, d); } };
// tile row m (igemm_plan.h: row m & 255 of row tile m >> 8 = pixels 256 (m >> 10) .. of phase (m >> 8) & 3) -> img << 20 | y << 10 | x
// of its SOURCE pixel (aux.hw / aux.wout divide by Hin * Win / Win in this mode), -1 for a padding row
__device__ __forceinline__ int pack_geo_up2f(const mofa_igemm_args& a, const Aux& aux, int m) {
    const IgemmUp2fPixel s = igemm_up2f_pixel(a, m, FDivBy{aux.hw}, FDivBy{aux.wout});   // (the one decode of igemm_plan.h)
    const int g = (s.img << 20) | (s.y << 10) | s.x;
    return s.valid ? g : -1;
}
// tap (ky, kx) of phase ph = 2 a + b reads source pixel (y - 1 + a + ky, x - 1 + b + kx): the CONV3X3 tap with ks = 2, stride = up = 1
// and the per-axis origin 1 - a / 1 - b
__device__ __forceinline__ unsigned tap_src_up2f(const mofa_igemm_args& a, const Aux& aux, int g, int ky, int kx, int ph, int swzb) {
    const int vy = ((g >> 10) & 1023) + ky - (1 - (ph >> 1)), vx = (g & 1023) + kx - (1 - (ph & 1));
    const bool ok = g >= 0 && vy >= 0 && vx >= 0 && vy < a.Hin && vx < a.Win;
    const int row = ((g >> 20) * a.Hin + vy) * a.Win + vx;
    const unsigned off = (unsigned)row * (unsigned)aux.ldxb + (unsigned)swzb;
    return ok ? off : XO_INVALID;
}
template <class C>
__device__ __forceinline__ void tap_advance_up2f(C& c, const int kpt) {
    ++c.ksw;
    if (++c.ikc == kpt) {
        c.ikc = 0;
        if (++c.kx == 2) { c.kx = 0; ++c.ky; }
    }
}
// the output row of tile row mr, or -1 (the one row map of igemm_plan.h on the launch's magic-number dividers)
__device__ __forceinline__ int up2f_out_row(const mofa_igemm_args& a, const Aux& aux, int mr) {
    return igemm_up2f_out_row(a, mr, FDivBy{aux.hw}, FDivBy{aux.wout});
}

// a cursor (ikc, ksw: K tile within the tap / overall; ky, kx: tap coordinates, convT3: ky = tap) moves one K tile on
template <class C>
__device__ __forceinline__ void tap_advance(C& c, const mofa_igemm_args& a, const int kpt, const int ks) {
    ++c.ksw;
    if (++c.ikc == kpt) {
        c.ikc = 0;
        if (a.mode == MOFA_MODE_CONV3X3) { if (++c.kx == ks) { c.kx = 0; ++c.ky; } } else ++c.ky;
    }
}

// buffer descriptor over [p, p + bytes), and one 16-byte-per-lane LDS-DMA through it: voff = per-lane byte offset, soff =
// uniform byte offset, the wave's 1 KB lands at lds_wave_base.  (A function object like the lambda it replaces, one instance
// per kernel: as a plain function the kernels' register allocation comes out differently.)
typedef decltype(__builtin_amdgcn_make_buffer_rsrc((void*)nullptr, (short)0, 0, 0)) BufRsrc;
__device__ __forceinline__ BufRsrc buf_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, 0x00020000);
}
struct LdsDma16 {
    __device__ __forceinline__ void operator()(const BufRsrc& rs, unsigned voff, int soff, char* lds_wave_base) const {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voff, soff, 0, 0);
    }
};

template <int ACT>
__device__ __forceinline__ float act_apply(IC<ACT>, float v) {
    if constexpr (ACT == MOFA_ACT_SILU) return silu_f(v);
    else if constexpr (ACT == MOFA_ACT_RELU) return fmaxf(v, 0.0f);
    else if constexpr (ACT == MOFA_ACT_GELU) return gelu_erf_f(v);
    else return v;
}

// The one row-vector row that ALL of a wave's ROWS output rows (from mw on) take, or -1 (wave-uniform).  With rv_mod_in == 1,
// idx(m) = ((m / div) * mul) % mod_out is a step function: time embedding per frame / cross-attention vector per clip, the
// same row for every tile that does not straddle a frame.
template <int ROWS>
__device__ __forceinline__ int rowvec_uniform_idx(const mofa_igemm_args& a, const int mw) {
    int idx_u = -1;
    if (a.rv_mod_in == 1) {
        int rv_div = a.rv_div;
        asm volatile("" : "+s"(rv_div));
        const int m0 = mw < a.M ? mw : a.M - 1, m1 = mw + ROWS - 1 < a.M ? mw + ROWS - 1 : a.M - 1;
        const int q0 = m0 / rv_div, q1 = m1 / rv_div;
        if (q0 == q1) idx_u = (q0 * a.rv_mul) % a.rv_mod_out;
    }
    return __builtin_amdgcn_readfirstlane(idx_u);
}

// ---- epilogue scratch images (tools/lds_bank_sim.py: writes and reads conflict-free) -------------------------------------
// 32 rows of 128 bytes.  rb = where row r's line starts, as a byte offset or as a pointer: the kernels' row maps differ
// (igemm8.hip: 128 r; igemm320.hip: four blocks 8 KB apart), and the swizzle is added to rb term by term because the shape of
// the address expression decides hipcc's code.
struct RowLines128 { __device__ __forceinline__ int operator()(int r) const { return r * 128; } };   // row map: rows back to back
template <class B>
__device__ __forceinline__ B h16_off(B rb, int r, int c8) {       // 32 rows x 64 fp16; c8 = 8-byte chunk (4 columns)
    return rb + (((c8 >> 1) ^ ((r >> 1) & 7)) << 4) + (((c8 & 1) ^ (r & 1)) << 3);
}
__device__ __forceinline__ f16x8 h16_row_fix(int r, f16x8 v) {    // 16 bytes read back from row r: odd rows hold the halves swapped
    f16x8 o = v;
    if (r & 1) o = (f16x8){v[4], v[5], v[6], v[7], v[0], v[1], v[2], v[3]};
    return o;
}
template <class B>
__device__ __forceinline__ B f32_off(B rb, int r, int c) {        // 32 rows x 32 fp32; c = 16-byte chunk (4 columns)
    return rb + ((c ^ (((r >> 1) & 3) | ((r & 1) << 2))) << 4);
}

// Row side of the fp16 transpose: the p-th piece a lane reads back, halves in order.  The row is computed from `lane` HERE,
// next to the swizzle, so that hipcc folds the two together as it did when every epilogue spelled them out (a helper is
// simplified before it is inlined: with the row passed in, the code differs); rl(row) = byte offset of a row's line from sb
// (the kernel's row map).  CPR pieces of 8 columns per row (8: two 32-column tiles, 4: one, 2: GEGLU's 16-column half), CPR / 2
// passes p.  (The fp32 image has no such helper: every form tried changed the kernels' code.)
struct H16Piece { int row, blk; f16x8 v; };                     // row (64 / CPR) p + lane / CPR, piece lane % CPR of it
template <int CPR, class RowLines>
__device__ __forceinline__ H16Piece h16_row(const char* sb, RowLines rl, int lane, int p) {
    constexpr int SH = CPR == 8 ? 3 : (CPR == 4 ? 2 : 1);
    static_assert(CPR == 1 << SH, "8, 4 or 2 pieces per row");
    const int row = (64 >> SH) * p + (lane >> SH), blk = lane & (CPR - 1);
    const f16x8 v = *(const f16x8*)(sb + rl(row) + ((blk ^ ((row >> 1) & 7)) << 4));
    return H16Piece{row, blk, h16_row_fix(row, v)};
}

}  // namespace

// q = umulhi(n, mul) >> shr == n / d for 0 <= n < 2^31 (mul == 0: d == 1)
static inline FastDiv fastdiv_make(int d) {
    FastDiv f = {0, 0};
    if (d > 1) {
        unsigned lg = 0;
        while ((1u << lg) < (unsigned)d) ++lg;                     // ceil(log2 d)
        const unsigned p = 31 + lg;
        f.mul = (unsigned)(((1ull << p) + (unsigned)d - 1) / (unsigned)d);
        f.shr = p - 32;
    }
    return f;
}

// launch-invariant scalars of a launch (tilesN = output tile columns of the chosen tile)
static inline Aux igemm_pipe_aux(const mofa_igemm_args* a, int taps, int tilesN) {
    Aux aux;
    aux.tiles_n = fastdiv_make(tilesN);
    const bool up2f = a->mode == MOFA_MODE_CONV3X3_UP2F;      // (its rows are SOURCE pixels: divisors Hin * Win and Win)
    aux.hw = fastdiv_make(up2f ? a->Hin * a->Win : a->mode == MOFA_MODE_CONV3X3 ? a->Hout * a->Wout : 1);
    aux.wout = fastdiv_make(up2f ? a->Win : a->mode == MOFA_MODE_CONV3X3 ? a->Wout : 1);
    aux.t3hw = fastdiv_make(a->mode == MOFA_MODE_CONVT3 ? a->HW : 1);
    aux.t3t = fastdiv_make(a->mode == MOFA_MODE_CONVT3 && a->T > 0 ? a->T : 1);
    const bool halo = a->mode == MOFA_MODE_CONVT3 && a->T == 0;   // rows before a.x are read (tap -1 of the first frame)
    aux.ldxb = a->ldx * 2;
    aux.row_shift = halo ? a->HW : 0;
    aux.xbase = (const char*)a->x - (halo ? (size_t)a->HW * a->ldx * 2 : 0);
    aux.x_bytes = (unsigned)(igemm8_rows_in(a) * a->ldx * 2 - (a->ldx - a->Cin) * 2);
    aux.w_bytes = (unsigned)(igemm_w_rows(a) * taps * a->Cin * 2);
    aux.trace = nullptr;
    aux.nsplit_d = fastdiv_make(1);
    aux.kpt_d = fastdiv_make(a->Cin / 64);
    aux.ks_d = fastdiv_make(a->mode == MOFA_MODE_CONV3X3 ? (a->ksize > 0 ? a->ksize : 3) : 1);
    aux.nsplit = 1;
    aux.tile0 = 0;
    aux.nitems = 0;
    aux.ws = nullptr;
    return aux;
}
