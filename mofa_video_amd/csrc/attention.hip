// Attention kernels for gfx950 (head_dim 64 or 128).
//
// mofa_attn_spatial_f16: flash-style self-attention over the S = h*w tokens of one frame.
//   One workgroup = 4 waves = 128 (or 256: two 32-query blocks per wave) query rows of one (frame, head); K and V
//   tiles of 64 keys are staged through double-buffered LDS (V row-major; its transposed fragments come from the LDS
//   transpose read ds_read_b64_tr_b16).  Scores are computed TRANSPOSED (S^T = K . Q^T, MFMA
//   32x32x16 f16) so every lane owns one query row: the softmax statistics are per-lane scalars
//   (one cross-half exchange per tile) and the probabilities are already laid out as the B operand of
//   O^T += V^T . P^T -- the k-slot -> key permutation of that MFMA is chosen to match the accumulator
//   layout of S^T, so P never leaves registers.  fp32 accumulation, online softmax in exp2 domain.
//
// mofa_attn_temporal_f16: self-attention over the T <= 32 frames of one (clip, pixel, head); HBM-bound, one wave per
//   sequence on the matrix cores (S^T = K . Q^T as one 32x32 tile, softmax per lane, O^T = V^T . P^T with P taken from the
//   S^T accumulators; V row-major in LDS, read through the LDS transpose read).
//
// mofa_attn_temporal_long_f16: the same for 1 <= T <= 128 frames (clips of more than 32 frames per forward pass): ceil(T / 32)
//   key tiles of K and V in the wave's LDS, one 32-query block at a time with all of its score tiles in registers.
//   mofa_attn_temporal_long_masked_f16: its form for frame-sharded clips (Tq <= T query frames, a key mask);
//   mofa_attn_temporal_long_local_f16: its form under a per-query rule (a band round the query plus the first frames).
//   mofa_attn_temporal_long_window_f16: that rule for a frame shard (Tq query frames, key slots = anchor frames + band frames).
//   One body (attn_temporal_long_body.inc) included by the four kernels, one launcher, one dispatch, one argument check.
//   mofa_attn_temporal_stream_local_f16: the per-query rule for 1 <= T <= 1024 under radius <= 32 and anchor <= 32 (four key tiles);
//   mofa_attn_temporal_stream_f16: any radius and anchor, dense included, 1 <= T <= 1024: an online-softmax walk over the key tiles.
//   mofa_attn_temporal_stream_shard_f16: that walk for a frame shard, Tq query frames against 1 <= S <= 1024 key slots: the window
//   rule on anchor + band slots, or dense under a key mask whose dead slots are never read.
//   One body (attn_temporal_stream_body.inc) included by the two walks; the ring kernel shares their decode, Q load, store and tile.
//
// mofa_transpose_v_f16, mofa_softmax_rows_f16: the two helpers of the VAE mid-block attention (scores materialised by implicit GEMMs).

#include "common.h"

#define ATT_TILE 64
#define ATT_DEFER_SUM 16384.0f   // a tile whose row sum of exp2(score - reference) reaches this moves the reference (fp16 P < 65504)

// D = head dim (64 or 128).  K tile row stride D+8 halves (144 / 272 B: conflict-free ds_read_b128).
// QB = 32-query blocks per wave (1 or 2).  With QB = 2 every K / V^T fragment read from LDS feeds two MFMAs and the
// per-tile costs (tile loads, LDS store, barrier, 24 fragment reads) are paid once per 64 queries of a wave: used when
// a frame has enough query rows to fill the chip with 256-row workgroups.
// V stays ROW-major ([key][d], as the QKV projection writes it): the V^T fragments of O^T += V^T P^T are read with
// ds_read_b64_tr_b16, the LDS transpose read of gfx950.  Semantics (measured, tools note in DESIGN.md): within each group of
// 16 lanes, lane j supplies the address of an 8-byte chunk C_j (4 halves); lane i = 4 q + e of the group receives
// (C_q[e], C_{q+4}[e], C_{q+8}[e], C_{q+12}[e]).  With lane j = q + 4 r addressing V[k0 + r][d0 + 4 q .. + 3], lane i gets
// V[k0 .. k0 + 3][d0 + i]: four consecutive keys of ONE column d -- a V^T fragment piece -- from row-major data.  Row stride
// D + 32 halves: the 32 lanes of a half-wave (4 key rows x 8 chunks) then hit 32 distinct bank pairs.
typedef short att_s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f16x4 lds_read_tr4(const f16* p) {
    const att_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) att_s16x4*)p);
    return __builtin_bit_cast(f16x4, v);
}

template <int D, int QB>
__global__ __launch_bounds__(256, 2) void attn_spatial_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                              const f16* __restrict__ v, f16* __restrict__ out,
                                                              int heads, int S, int ldq, int ldk, int ldv, int ldo, float c,
                                                              int nqb, int total) {
    // D = 64: K / V tiles arrive by LDS-DMA (buffer_load ... lds: no VGPR staging, no per-tile address arithmetic -- the tile
    // index is the instruction's scalar offset, rows beyond S read as zero through the descriptor's bounds check).  The DMA
    // image is lane-linear, so rows are exactly 128 bytes and conflicts are avoided by swizzling the SOURCE chunk instead of
    // padding: K chunk c of row r sits in slot c ^ ((r >> 1) & 7) (ds_read_b128 fragments), V's two 64-byte halves are
    // swapped in rows with bit 1 set (the 4 key rows x 64 bytes of a transpose read then cover 4 distinct bank quarters).
    // D = 128 (0.1 % of a clip) keeps the register-staged, padded form.
    constexpr bool DMA = D == 64;
    // Two buffers, tile t + 1 fetched while tile t is computed.  (A ring of three, fetched TWO tiles ahead with a counted
    // end-of-tile wait -- the landing time of a piece is NOT what the end-of-tile wait stalls on: same results bit for bit,
    // 1-2 % slower at S = 9216 and 2304, profiles/r06_attn_anatomy.log)
    constexpr int NBUF = 2;
    constexpr int ATT_KSTR = DMA ? D : D + 8;
    constexpr int ATT_VSTR = DMA ? D : D + 32; // V tile row stride (halves)
    constexpr int KK = D / 16;       // MFMA k-steps of S^T
    constexpr int DB = D / 32;       // 32-wide output d-blocks
    constexpr int NCH = D / 32;      // 16-byte chunks per thread per tile (K and V each)
    extern __shared__ __attribute__((aligned(16))) char smem_att[];
    f16* sKb = (f16*)smem_att;                          // [NBUF][64 * ATT_KSTR]
    f16* sVb = sKb + NBUF * ATT_TILE * ATT_KSTR;        // [NBUF][64 * ATT_VSTR]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    // XCD-aware work order (r04b; 1-D grid of 8 * ceil(total / 8) workgroups): the hardware deals workgroup ids round-robin over
    // the 8 XCDs, so workgroup b lives on XCD b & 7; each XCD takes a CONTIGUOUS range of work ids w = (frame * heads + head) *
    // nqb + query block (the bijective split of igemm_common.h's TileWalk), i.e. the query blocks of one (frame, head) -- which
    // all stream the same K / V (2.4 MB at level 0) -- run side by side on ONE XCD and find each other's tiles in its L2, instead
    // of every XCD pulling every (frame, head)'s K / V through the fabric once: fabric reads per level-0 launch 5.4 -> 1.5 GB,
    // 964 -> 988 TF/s at S = 9216, 772 -> 815 at S = 2304, bit-identical (profiles/r04b_attn_xcd_order_ab.log).
    int head, frame, qb_;
    {
        const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3, qn = total >> 3, rn = total & 7;
        const int start = xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn;
        if (local >= qn + (xcd < rn ? 1 : 0)) return;
        const int w = start + local, pair = w / nqb;
        qb_ = w - pair * nqb;
        frame = pair / heads;
        head = pair - frame * heads;
    }
    const int q0 = qb_ * (128 * QB) + wave * (32 * QB);

    const f16* kbase = k + (size_t)frame * S * ldk + head * D;
    const f16* vbase = v + (size_t)frame * S * ldv + head * D;

    // Q fragments (B operand of S^T): lane (query l31, half lh) holds Q[q][16*kk + 8*lh .. +8)
    f16x8 qf[QB][KK];
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        const int qi = q0 + b * 32 + l31;
        const f16* qp = q + ((size_t)frame * S + (qi < S ? qi : 0)) * ldq + head * D + lh * 8;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            // Q is held pre-multiplied by c = scale * log2(e) (here: one more fp16 rounding of Q, random, 2^-11 relative --
            // callers that can fold c into their Q projection pass scale <= 0 and skip it): the
            // MFMA then yields the scores in the exp2 domain and, with the accumulator started at -m, already minus the
            // running maximum -- no per-score VALU work before v_exp_f32 (this kernel is bound by VALU issue, not by MFMA)
            const f16x8 v = (qi < S) ? *(const f16x8*)(qp + kk * 16) : zero8;
            qf[b][kk] = v;
            if (c != 1.0f) {                               // (c == 1: the caller folded scale * log2(e) into the Q projection)
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[b][kk][e] = (f16)((float)v[e] * c);
            }
        }
    }

    constexpr bool NEGM = D == 64;
    f32x16 o[QB][DB];
    f32x16 negm[QB];                                      // (NEGM) -m_run[b] in all 16 registers
    float m_run[QB], l_run[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[b][r] = 0.f;
        m_run[b] = 0.f; l_run[b] = 0.f;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[b][db][r] = 0.f;
    }

    // loader mapping: K tile = 64 keys x D/8 chunks(16 B); V^T tile = D rows x 8 chunks; NCH chunks per thread each
    constexpr int CPR = D / 8;
    f16x8 gk[NCH], gv[NCH];
    // per-thread source pointers of tile 0 (K and V rows have the same shape: 64 keys x D), advanced by 64 rows per load:
    // 4 64-bit adds per tile instead of the address arithmetic from scratch; only a tile that reaches beyond S is
    // bounds-checked (wave-uniform branch)
    const f16* kptr[NCH];
    const f16* vptr[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int cidx = tid + 256 * i;
        const int krow = cidx / CPR, kcol = cidx - krow * CPR;
        kptr[i] = kbase + (size_t)krow * ldk + kcol * 8;
        vptr[i] = vbase + (size_t)krow * ldv + kcol * 8;
    }
    const size_t kstep = (size_t)ATT_TILE * ldk, vstep = (size_t)ATT_TILE * ldv;
    auto load_tile = [&](int k0) {
        if (__builtin_amdgcn_readfirstlane(k0 + ATT_TILE <= S)) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                gk[i] = *(const f16x8*)kptr[i];
                gv[i] = *(const f16x8*)vptr[i];
            }
        } else {                                            // rows of keys beyond S are zero (K: score masked; V: 0 * p)
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const bool ok = k0 + (tid + 256 * i) / CPR < S;
                gk[i] = ok ? *(const f16x8*)kptr[i] : zero8;
                gv[i] = ok ? *(const f16x8*)vptr[i] : zero8;
            }
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) { kptr[i] += kstep; vptr[i] += vstep; }
    };
    auto store_tile = [&](int buf) {
        f16* sK = sKb + buf * ATT_TILE * ATT_KSTR;
        f16* sV = sVb + buf * ATT_TILE * ATT_VSTR;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int cidx = tid + 256 * i;
            const int krow = cidx / CPR, kcol = cidx - krow * CPR;
            *(f16x8*)&sK[krow * ATT_KSTR + kcol * 8] = gk[i];
            *(f16x8*)&sV[krow * ATT_VSTR + kcol * 8] = gv[i];
        }
    };
    // transpose-read address of this lane inside a V tile (see lds_read_tr4): key row (lane & 15) >> 2 (+ 4 lh), column
    // chunk 4 ((lane & 15) & 3) of the 16-column group (lane >> 4) & 1
    const int tr_off = (((lane & 15) >> 2) + 4 * lh) * ATT_VSTR + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

    // ---- DMA form: descriptors over this (frame, head)'s K / V rows; per-lane byte offset of tile 0 ----
    const auto rsk = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, (unsigned)(((size_t)(S - 1) * ldk + D) * 2), 0x00020000);
    const auto rsv = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, (unsigned)(((size_t)(S - 1) * ldv + D) * 2), 0x00020000);
    unsigned dko[2], dvo[2];                              // instruction i of this wave: tile rows (2 wave + i) * 8 + lane / 8
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (2 * wave + i) * 8 + (lane >> 3), slot = lane & 7;
        dko[i] = (unsigned)row * (unsigned)ldk * 2u + (unsigned)((slot ^ ((row >> 1) & 7)) * 16);
        dvo[i] = (unsigned)row * (unsigned)ldv * 2u + (unsigned)((slot ^ (4 * ((row >> 1) & 1))) * 16);
    }
    auto dma_tile = [&](int t, int buf) __attribute__((always_inline)) {
        char* bk = (char*)(sKb + buf * ATT_TILE * ATT_KSTR) + (2 * wave) * 1024;
        char* bv = (char*)(sVb + buf * ATT_TILE * ATT_VSTR) + (2 * wave) * 1024;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsk, (__attribute__((address_space(3))) void*)(bk + i * 1024), 16, dko[i],
                                                     t * ATT_TILE * ldk * 2, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsv, (__attribute__((address_space(3))) void*)(bv + i * 1024), 16, dvo[i],
                                                     t * ATT_TILE * ldv * 2, 0, 0);
        }
    };
    const int ksw = (l31 >> 1) & 7;                       // K fragment reads: slot = chunk ^ ksw
    const int vsw = (lane >> 3) & 1;                      // V transpose reads: this lane's key row has bit 1 set -> other half

    const int ntiles = (S + ATT_TILE - 1) / ATT_TILE;
    if constexpr (DMA) {
        dma_tile(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        load_tile(0);
        store_tile(0);
    }
    __syncthreads();

    int buf = 0;                                                    // t % NBUF
    for (int t = 0; t < ntiles; ++t, buf = (buf + 1 == NBUF ? 0 : buf + 1)) {
        const int k0 = t * ATT_TILE;
        if (t + 1 < ntiles) {
            if constexpr (DMA) dma_tile(t + 1, buf ^ 1);            // (the other buffer was released by the last barrier)
            else load_tile(k0 + ATT_TILE);
        }

        // ---- S^T tiles: s[b][ts][r] = score(key = k0 + 32*ts + (r&3) + 8*(r>>2) + 4*lh, query = 32*b + l31) ----
        // the accumulators start at -m_run: NEGM keeps that as a 16-register tuple per query block (it changes only when the
        // reference moves) and the first k-step takes it as its C operand -- no 32 v_mov per tile; the register-staged
        // D = 128 form has no registers to spare for it
        f32x16 s[QB][2];
#pragma unroll
        for (int ts = 0; ts < 2; ++ts) {
            if constexpr (!NEGM) {
#pragma unroll
                for (int b = 0; b < QB; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[b][ts][r] = -m_run[b];
            }
            const f16* kp = sKb + buf * ATT_TILE * ATT_KSTR + (ts * 32 + l31) * ATT_KSTR + (DMA ? 0 : lh * 8);
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const f16x8 kf = *(const f16x8*)(kp + (DMA ? ((2 * kk + lh) ^ ksw) * 8 : kk * 16));
#pragma unroll
                for (int b = 0; b < QB; ++b)
                    s[b][ts] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[b][kk], (NEGM && kk == 0) ? negm[b] : s[b][ts], 0, 0, 0);
            }
        }
        // ---- mask (tail tile only) + online softmax (per-lane query row; the two halves hold disjoint keys) ----
        if (__builtin_amdgcn_readfirstlane(k0 + ATT_TILE > S)) {
            asm volatile("; tail tile" ::: "memory");   // keep this a real (wave-uniform) branch, not 64 selects per tile
#pragma unroll
            for (int b = 0; b < QB; ++b)
#pragma unroll
                for (int ts = 0; ts < 2; ++ts)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = k0 + ts * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        if (key >= S) s[b][ts][r] = -1e30f;
                    }
        }
        // s = score * c - m_run (exp2 domain), and the probabilities are v_exp_f32 of the accumulators as they are.  m_run is
        // a REFERENCE, not the maximum: it is the first tile's row maximum and moves only when a tile's probabilities come
        // near the fp16 range (row sum of the tile >= 2^ATT_DEFER; then the true maximum is taken, O, l and this tile's
        // scores are rescaled by the same factor and the tile's probabilities recomputed) -- the quotient O / l does not
        // depend on the reference, fp16 keeps its relative precision at any magnitude, l and O are fp32.  So the common tile
        // needs no row maximum at all: one compare of the row sum it computes anyway (this kernel is VALU-issue bound).
        // (r04: the row sums taken from the matrix core instead -- ones[32x16] . P^T, four extra MFMAs per query block and tile,
        // 132 v_add_f32 fewer -- measured SLOWER, 946 against 972 TF/s on the L0 shape: the sums gate the reference check, so
        // the PV MFMAs wait for the extra MFMAs' results; profiles/r04_attn_rowsum_mfma_ab.log)
        f16x8 pf[QB][2][2];
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            float psum = 0.f;
#pragma unroll
            for (int ts = 0; ts < 2; ++ts)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(s[b][ts][r]);   // raw v_exp_f32
                    psum += p;
                    pf[b][ts][r >> 3][r & 7] = (f16)p;
                }
            const float ptot = psum + __shfl_xor(psum, 32, 64);           // both key halves of the query row
            const bool move = !(ptot < ATT_DEFER_SUM) || t == 0;           // (NaN-safe; tile 0: m_run = 0 is no reference yet)
            if (__any(move)) {
                asm volatile("; reference moves" ::: "memory");
                float mx = s[b][0][0];
#pragma unroll
                for (int ts = 0; ts < 2; ++ts)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[b][ts][r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float delta = move ? mx : 0.f;
                const float alpha = __builtin_amdgcn_exp2f(-delta);
                m_run[b] += delta;
                if constexpr (NEGM) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) negm[b][r] = -m_run[b];
                }
                l_run[b] *= alpha;
#pragma unroll
                for (int db = 0; db < DB; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[b][db][r] *= alpha;
                psum = 0.f;
#pragma unroll
                for (int ts = 0; ts < 2; ++ts)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float p = __builtin_amdgcn_exp2f(s[b][ts][r] - delta);
                        psum += p;
                        pf[b][ts][r >> 3][r & 7] = (f16)p;
                    }
            }
            l_run[b] += psum;
        }

        // ---- O^T[d][q] += V^T[d][key] * P^T[key][q]; k-slot (8*lh + jj) of MFMA (ts,u) = key
        //      32*ts + 16*u + 4*lh + (jj&3) + 8*(jj>>2), identical for both operands ---------------
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const f16* vp = sVb + buf * ATT_TILE * ATT_VSTR + tr_off + (DMA ? (db ^ vsw) : db) * 32;
#pragma unroll
            for (int ts = 0; ts < 2; ++ts)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const f16x4 lo = lds_read_tr4(vp + (ts * 32 + u * 16) * ATT_VSTR);        // keys k0 + 4 lh + 0..3
                    const f16x4 hi = lds_read_tr4(vp + (ts * 32 + u * 16 + 8) * ATT_VSTR);    // keys k0 + 4 lh + 8..11
                    const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                    for (int b = 0; b < QB; ++b) o[b][db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[b][ts][u], o[b][db], 0, 0, 0);
                }
        }
        if (t + 1 < ntiles) {
            // this wave's pieces of tile t + 1 have landed (the loop has no other vector-memory operation)
            if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else store_tile(buf ^ 1);
        }
        __syncthreads();
    }

#pragma unroll
    for (int b = 0; b < QB; ++b) {
        const float l_tot = l_run[b] + __shfl_xor(l_run[b], 32, 64);
        const float inv = 1.0f / l_tot;
        const int qi = q0 + b * 32 + l31;
        if (qi < S) {
            f16* op = out + ((size_t)frame * S + qi) * ldo + head * D;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    f16x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (f16)(o[b][db][4 * qd + e] * inv);
                    *(f16x4*)(op + db * 32 + 8 * qd + 4 * lh) = v;
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// attn_spatial_q64_kernel: the D = 64, QB = 2 case (64 queries per wave; the level-0 / level-1 launches of a clip) with its
// key-tile schedule laid out by hand.  Grid, XCD-aware work order, LDS image (two buffers, the swizzles above), DMA pieces,
// one barrier per tile, the reference rule and -- per query row -- the sequence of MFMAs, v_exp_f32, adds and fp16 roundings are
// those of attn_spatial_kernel<64, 2>: the output is bit-identical.  What differs is what a wave issues around them:
//   * tile 0 (always moves the reference) and a ragged last tile (key mask) run the straight code of the template OUTSIDE the
//     loop; the loop body has neither test.  It is unrolled over the two buffers, so every K / V^T fragment is read at
//     base + immediate (4 + 2 address registers for the whole kernel) and the DMA destinations are wave base + immediate in M0
//     (wave index made uniform once).
//   * fragment read-ahead: K fragments are read ATT_Q64_KAHEAD MFMA pairs ahead of their use, the first ones of the next tile
//     right after the barrier; V^T fragments one group of four transpose reads ahead, the first group before the softmax of
//     query block 1; the compiler counts the waits (lgkmcnt(n)).  sched_barrier after every MFMA pair and every eight
//     probabilities keeps that order (without them hipcc regroups the reads: - 1.5 %).
//   * the reference check is lane-local on the common path (no shuffle, no LDS round trip in front of the branch), see the
//     comment at the check.
//   * O leaves through the LDS as whole 128-byte rows.
// Measured and dropped (profiles/attn_spatial_sched_bench.log): the exp / add / pack of key half 0 beside the S^T MFMAs of
// key half 1 (- 1.4 %: with two waves per SIMD the partner wave's MFMAs already fill the softmax), three K fragments ahead,
// pinning each P fragment's pack to its eight probabilities, the DMA of tile 0 in front of the Q loads.
constexpr int ATT_Q64_KAHEAD = 2;
template <int V> struct AttIC { static constexpr int v = V; };

__global__ __launch_bounds__(256, 2) void attn_spatial_q64_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                  const f16* __restrict__ v, f16* __restrict__ out,
                                                                  int heads, int S, int ldq, int ldk, int ldv, int ldo, float c,
                                                                  int nqb, int total) {
    constexpr int D = 64, KK = 4, DB = 2;
    constexpr int TILE_B = ATT_TILE * D * 2;             // bytes of one K (or V) tile image
    constexpr int V_B = 2 * TILE_B;                      // V buffers behind the two K buffers
    extern __shared__ __attribute__((aligned(16))) char smem_att[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    int head, frame, qb_;                                 // (the work order of attn_spatial_kernel)
    {
        const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3, qn = total >> 3, rn = total & 7;
        const int start = xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn;
        if (local >= qn + (xcd < rn ? 1 : 0)) return;
        const int w = start + local, pair = w / nqb;
        qb_ = w - pair * nqb;
        frame = pair / heads;
        head = pair - frame * heads;
    }
    const int q0 = qb_ * 256 + wave * 64;
    const f16* kbase = k + (size_t)frame * S * ldk + head * D;
    const f16* vbase = v + (size_t)frame * S * ldv + head * D;

    // ---- LDS-DMA: descriptors over this (frame, head)'s K / V rows; instruction i of this wave brings tile rows
    //      (2 wave + i) * 8 + lane / 8 to the lane-linear kilobyte (2 wave + i) of the tile image ----
    const auto rsk = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, (unsigned)(((size_t)(S - 1) * ldk + D) * 2), 0x00020000);
    const auto rsv = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, (unsigned)(((size_t)(S - 1) * ldv + D) * 2), 0x00020000);
    unsigned dko[2], dvo[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (2 * wave + i) * 8 + (lane >> 3), slot = lane & 7;
        dko[i] = (unsigned)row * (unsigned)ldk * 2u + (unsigned)((slot ^ ((row >> 1) & 7)) * 16);
        dvo[i] = (unsigned)row * (unsigned)ldv * 2u + (unsigned)((slot ^ (4 * ((row >> 1) & 1))) * 16);
    }
    char* const dma_base = smem_att + wave * 2048;        // wave-uniform: the destinations are this + immediate
    auto dma_tile = [&](int t, int buf_bytes) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsk, (__attribute__((address_space(3))) void*)(dma_base + buf_bytes + i * 1024),
                                                     16, dko[i], t * ATT_TILE * ldk * 2, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsv, (__attribute__((address_space(3))) void*)(dma_base + V_B + buf_bytes + i * 1024),
                                                     16, dvo[i], t * ATT_TILE * ldv * 2, 0, 0);
        }
    };
    const int ntiles = (S + ATT_TILE - 1) / ATT_TILE;

    // Q fragments (B operand of S^T): lane (query l31, half lh) holds Q[q][16*kk + 8*lh .. +8), times c unless c == 1
    f16x8 qf[2][KK];
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int qi = q0 + b * 32 + l31;
        const f16* qp = q + ((size_t)frame * S + (qi < S ? qi : 0)) * ldq + head * D + lh * 8;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const f16x8 v = (qi < S) ? *(const f16x8*)(qp + kk * 16) : zero8;
            qf[b][kk] = v;
            if (c != 1.0f) {
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[b][kk][e] = (f16)((float)v[e] * c);
            }
        }
    }

    f32x16 o[2][DB];
    f32x16 negm[2];                                       // -m_run[b] in all 16 registers: the C operand of every S^T chain
    float l_run[2];                                       // (the reference m_run[b] is -negm[b][0])
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[b][r] = 0.f;
        l_run[b] = 0.f;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[b][db][r] = 0.f;
    }

    // fragment addresses (bytes, buffer 0): K fragment (ts, kk) at kaddr[kk] + ts * 4096, V^T pieces at vaddr[db] + key row * 128
    const int ksw = (l31 >> 1) & 7, vsw = (lane >> 3) & 1;
    int kaddr[KK], vaddr[DB];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) kaddr[kk] = l31 * (D * 2) + ((2 * kk + lh) ^ ksw) * 16;
#pragma unroll
    for (int db = 0; db < DB; ++db)
        vaddr[db] = V_B + 2 * ((((lane & 15) >> 2) + 4 * lh) * D + 16 * ((lane >> 4) & 1) + 4 * (lane & 3) + (db ^ vsw) * 32);
    auto k_frag = [&](int buf_bytes, int i) __attribute__((always_inline)) {     // i = 4 ts + kk
        return *(const f16x8*)(smem_att + kaddr[i & 3] + buf_bytes + (i >> 2) * 4096);
    };
    auto v_frag = [&](int buf_bytes, int j) __attribute__((always_inline)) {     // j = 4 db + 2 ts + u
        const char* vp = smem_att + vaddr[j >> 2] + buf_bytes + (((j >> 1) & 1) * 32 + (j & 1) * 16) * (D * 2);
        const f16x4 lo = lds_read_tr4((const f16*)vp);                            // keys k0 + 4 lh + 0..3
        const f16x4 hi = lds_read_tr4((const f16*)(vp + 8 * D * 2));              // keys k0 + 4 lh + 8..11
        return f16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };

    // N probabilities (registers r0 .. r0 + N - 1 of one S^T tile, inside one P fragment): exp2 of the accumulators as they
    // are, summed in key order, packed; a key half of a query block is registers 0 .. 15 in this order
    auto soft_piece = [&](const f32x16& sv, auto r0c, auto nc, float& psum, f16x8 (&pf)[2]) __attribute__((always_inline)) {
        constexpr int R0 = decltype(r0c)::v, N = decltype(nc)::v;
#pragma unroll
        for (int r = R0; r < R0 + N; ++r) {
            const float p = __builtin_amdgcn_exp2f(sv[r]);
            psum += p;
            pf[r >> 3][r & 7] = (f16)p;
        }
    };
    auto soft_half = [&](const f32x16& sv, float& psum, f16x8 (&pf)[2]) __attribute__((always_inline)) {
        soft_piece(sv, AttIC<0>{}, AttIC<16>{}, psum, pf);
    };
    // the reference rule of attn_spatial_kernel for query block b, given the lane's half sum; first = tile 0
    auto reference_rule = [&](int b, f32x16 (&s)[2][2], float& psum, f16x8 (&pf)[2][2][2], bool first) __attribute__((always_inline)) {
        const float ptot = psum + __shfl_xor(psum, 32, 64);               // both key halves of the query row
        const bool move = !(ptot < ATT_DEFER_SUM) || first;               // (NaN-safe)
        if (__any(move)) {
            asm volatile("; reference moves" ::: "memory");
            float mx = s[b][0][0];
#pragma unroll
            for (int ts = 0; ts < 2; ++ts)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[b][ts][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float delta = move ? mx : 0.f;
            const float alpha = __builtin_amdgcn_exp2f(-delta);
            const float m_new = -negm[b][0] + delta;                       // m_run[b] += delta
#pragma unroll
            for (int r = 0; r < 16; ++r) negm[b][r] = -m_new;
            l_run[b] *= alpha;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[b][db][r] *= alpha;
            psum = 0.f;
#pragma unroll
            for (int ts = 0; ts < 2; ++ts)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(s[b][ts][r] - delta);
                    psum += p;
                    pf[b][ts][r >> 3][r & 7] = (f16)p;
                }
        }
    };

    // ---- an edge tile (tile 0, a ragged last tile): the straight code of attn_spatial_kernel ----
    auto edge_tile = [&](int t, int buf_bytes) __attribute__((always_inline)) {
        const int k0 = t * ATT_TILE;
        if (t + 1 < ntiles) dma_tile(t + 1, buf_bytes ^ TILE_B);
        f32x16 s[2][2];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f16x8 kf = k_frag(buf_bytes, i);
#pragma unroll
            for (int b = 0; b < 2; ++b)
                s[b][i >> 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[b][i & 3], (i & 3) == 0 ? negm[b] : s[b][i >> 2], 0, 0, 0);
        }
        if (__builtin_amdgcn_readfirstlane(k0 + ATT_TILE > S)) {
            asm volatile("; tail tile" ::: "memory");
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int ts = 0; ts < 2; ++ts)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = k0 + ts * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        if (key >= S) s[b][ts][r] = -1e30f;
                    }
        }
        f16x8 pf[2][2][2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float psum = 0.f;
            soft_half(s[b][0], psum, pf[b][0]);
            soft_half(s[b][1], psum, pf[b][1]);
            reference_rule(b, s, psum, pf, t == 0);
            l_run[b] += psum;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const f16x8 vf = v_frag(buf_bytes, j);
#pragma unroll
            for (int b = 0; b < 2; ++b)
                o[b][j >> 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[b][(j >> 1) & 1][j & 1], o[b][j >> 2], 0, 0, 0);
        }
        if (t + 1 < ntiles) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };

    // ---- a tile of the loop: neither the first nor masked; BUF = its buffer, kr = its first K fragments (read after the
    //      barrier that released the buffer) ----
    f16x8 kr[ATT_Q64_KAHEAD];
    auto k_head = [&](int buf_bytes) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < ATT_Q64_KAHEAD; ++i) kr[i] = k_frag(buf_bytes, i);
    };
    auto loop_tile = [&](auto bufc, int t) __attribute__((always_inline)) {
        constexpr int BUF_B = decltype(bufc)::v * TILE_B;
        if (t + 1 < ntiles) dma_tile(t + 1, BUF_B ^ TILE_B);
        f32x16 s[2][2];
        f16x8 pf[2][2][2];
        float psum[2] = {0.f, 0.f};
        f16x8 kf[8];
#pragma unroll
        for (int i = 0; i < ATT_Q64_KAHEAD; ++i) kf[i] = kr[i];
        // slot i: the K fragment ATT_Q64_KAHEAD slots ahead and the MFMA pair of fragment i; sched_barrier keeps a slot's work in it
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i + ATT_Q64_KAHEAD < 8) kf[i + ATT_Q64_KAHEAD] = k_frag(BUF_B, i + ATT_Q64_KAHEAD);
#pragma unroll
            for (int b = 0; b < 2; ++b)
                s[b][i >> 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[i], qf[b][i & 3], (i & 3) == 0 ? negm[b] : s[b][i >> 2], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        soft_piece(s[0][0], AttIC<0>{}, AttIC<8>{}, psum[0], pf[0][0]);
        __builtin_amdgcn_sched_barrier(0);
        soft_piece(s[0][0], AttIC<8>{}, AttIC<8>{}, psum[0], pf[0][0]);
        __builtin_amdgcn_sched_barrier(0);
        // Reference check, lane-local on the common path.  The rule is: a query row whose tile sum ptot = psum + psum' (its two
        // lanes' half sums) is not < ATT_DEFER_SUM moves, and anything happens only if some row of the wave moves.  A half sum
        // is a sum of exp2 values: non-negative or NaN.  If every lane has psum < ATT_DEFER_SUM / 2, no half sum is NaN and
        // every ptot is the fp32 sum of two values below 8192: exact or rounded, it is below 16384 (rounding is monotonic and
        // 16384 - ulp is representable), so no row moves and the rule does nothing: skipping it leaves the same bits.
        // Otherwise (some psum >= 8192 or NaN) the rule itself runs, shuffle and all, unchanged.  So the pre-check only ever
        // ADDS evaluations of the rule, never replaces its outcome.
        f16x8 vf[8];
        soft_piece(s[0][1], AttIC<0>{}, AttIC<8>{}, psum[0], pf[0][1]);
        __builtin_amdgcn_sched_barrier(0);
        soft_piece(s[0][1], AttIC<8>{}, AttIC<8>{}, psum[0], pf[0][1]);
        if (__any(!(psum[0] < 0.5f * ATT_DEFER_SUM))) reference_rule(0, s, psum[0], pf, false);
        l_run[0] += psum[0];
        vf[0] = v_frag(BUF_B, 0);
        vf[1] = v_frag(BUF_B, 1);
        soft_piece(s[1][0], AttIC<0>{}, AttIC<8>{}, psum[1], pf[1][0]);
        __builtin_amdgcn_sched_barrier(0);
        soft_piece(s[1][0], AttIC<8>{}, AttIC<8>{}, psum[1], pf[1][0]);
        __builtin_amdgcn_sched_barrier(0);
        soft_piece(s[1][1], AttIC<0>{}, AttIC<8>{}, psum[1], pf[1][1]);
        __builtin_amdgcn_sched_barrier(0);
        soft_piece(s[1][1], AttIC<8>{}, AttIC<8>{}, psum[1], pf[1][1]);
        if (__any(!(psum[1] < 0.5f * ATT_DEFER_SUM))) reference_rule(1, s, psum[1], pf, false);
        l_run[1] += psum[1];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j + 2 < 8) vf[j + 2] = v_frag(BUF_B, j + 2);
#pragma unroll
            for (int b = 0; b < 2; ++b)
                o[b][j >> 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[j], pf[b][(j >> 1) & 1][j & 1], o[b][j >> 2], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (t + 1 < ntiles) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        k_head(BUF_B ^ TILE_B);                           // (the last tile's are not used: reads inside the LDS image)
    };

    dma_tile(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    edge_tile(0, 0);
    const bool ragged = (S & (ATT_TILE - 1)) != 0;
    const int loop_end = ragged ? ntiles - 1 : ntiles;   // loop tiles: [1, loop_end)
    if (1 < loop_end) {
        k_head(TILE_B);
        for (int t = 1;;) {
            loop_tile(AttIC<1>{}, t);
            if (++t >= loop_end) break;
            loop_tile(AttIC<0>{}, t);
            if (++t >= loop_end) break;
        }
    }
    if (ragged && ntiles > 1) edge_tile(ntiles - 1, ((ntiles - 1) & 1) * TILE_B);

    // O leaves through the K / V buffers (free after the last barrier) as whole 128-byte rows per (token, head): the wave's 64
    // rows x 128 B in its own 8 KB, 16-byte chunk c of row r in slot c ^ (r & 7); then 8 lanes store one row, 16 bytes each
    if (__builtin_amdgcn_readfirstlane((((size_t)out | (size_t)(ldo * 2)) & 15) == 0)) {
        char* ob = smem_att + wave * (64 * D * 2);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float l_tot = l_run[b] + __shfl_xor(l_run[b], 32, 64);
            const float inv = 1.0f / l_tot;
            const int row = b * 32 + l31;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    f16x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (f16)(o[b][db][4 * qd + e] * inv);
                    *(f16x4*)(ob + row * (D * 2) + (((db * 4 + qd) ^ (row & 7)) * 16) + lh * 8) = v;
                }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = i * 8 + (lane >> 3), ch = lane & 7, qi = q0 + row;
            const f16x8 v = *(const f16x8*)(ob + row * (D * 2) + ((ch ^ (row & 7)) * 16));
            if (qi < S) *(f16x8*)(out + ((size_t)frame * S + qi) * ldo + head * D + ch * 8) = v;
        }
        return;
    }
    // (an output whose rows are not 16-byte aligned: per-lane 8-byte stores, as attn_spatial_kernel)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const float l_tot = l_run[b] + __shfl_xor(l_run[b], 32, 64);
        const float inv = 1.0f / l_tot;
        const int qi = q0 + b * 32 + l31;
        if (qi < S) {
            f16* op = out + ((size_t)frame * S + qi) * ldo + head * D;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    f16x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (f16)(o[b][db][4 * qd + e] * inv);
                    *(f16x4*)(op + db * 32 + 8 * qd + 4 * lh) = v;
                }
        }
    }
}

template <int D, int QB>
static int launch_attn_spatial(const void* q, const void* k, const void* v, void* out, int nframes, int heads, int S,
                               int ldq, int ldk, int ldv, int ldo, float c, hipStream_t st) {
    constexpr int LDS = D == 64 ? 2 * (ATT_TILE * D + ATT_TILE * D) * 2 : 2 * (ATT_TILE * (D + 8) + ATT_TILE * (D + 32)) * 2;
    const int nqb = cdiv(S, 128 * QB);
    const long long total = (long long)nqb * heads * nframes;
    if (total > 0x7ffffff0LL) return MOFA_EINVAL;
    // (64 queries per wave at D = 64: the hand-scheduled kernel, same grid, LDS and arguments)
    const auto kern = [] {
        if constexpr (D == 64 && QB == 2) return &attn_spatial_q64_kernel;
        else return &attn_spatial_kernel<D, QB>;
    }();
    static LaunchSetup setup;
    if (setup.cus([kern](int) { return mofa_lds_optin((const void*)kern, LDS); }) == 0) return MOFA_ELAUNCH;
    dim3 grid((unsigned)(8 * ((total + 7) / 8)));              // (the kernel's XCD-aware work order)
    hipLaunchKernelGGL(kern, grid, dim3(256), LDS, st, (const f16*)q, (const f16*)k, (const f16*)v,
                       (f16*)out, heads, S, ldq, ldk, ldv, ldo, c, nqb, (int)total);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

extern "C" int mofa_attn_spatial_qb_f16(const void* q, const void* k, const void* v, void* out, int nframes, int heads,
                                        int head_dim, int S, int ldq, int ldk, int ldv, int ldo, float scale,
                                        int query_blocks, mofa_stream_t stream) {
    if (!q || !k || !v || !out || nframes <= 0 || heads <= 0 || S <= 0) return MOFA_EINVAL;
    if (ldq % 8 != 0 || ldk % 8 != 0 || ldv % 8 != 0 || ldo % 4 != 0) return MOFA_EINVAL;
    if (query_blocks < 0 || query_blocks > 2 || (query_blocks == 2 && head_dim != 64)) return MOFA_EINVAL;
    // scale <= 0: q already holds Q * head_dim^-0.5 * log2(e) (folded into the projection weights: no rounding of Q here)
    const float c = scale > 0.f ? scale * 1.4426950408889634f : 1.0f;
    // 64 queries per wave (256-row workgroups: +6-7 % at S = 9216 / 2304) when S tiles by 256 with <= 1/16 waste and the
    // grid still gives >= 4 workgroups per CU; query_blocks = 1 | 2 forces either (parity tests)
    const bool two = query_blocks ? query_blocks == 2
                                  : ((long long)cdiv(S, 256) * 256 * 16 <= (long long)S * 17 && (long long)cdiv(S, 256) * heads * nframes >= 1024);
    if (head_dim == 64)
        return two ? launch_attn_spatial<64, 2>(q, k, v, out, nframes, heads, S, ldq, ldk, ldv, ldo, c, (hipStream_t)stream)
                   : launch_attn_spatial<64, 1>(q, k, v, out, nframes, heads, S, ldq, ldk, ldv, ldo, c, (hipStream_t)stream);
    if (head_dim == 128)
        return launch_attn_spatial<128, 1>(q, k, v, out, nframes, heads, S, ldq, ldk, ldv, ldo, c, (hipStream_t)stream);
    return MOFA_EINVAL;
}

extern "C" int mofa_attn_spatial_f16(const void* q, const void* k, const void* v, void* out, int nframes, int heads,
                                     int head_dim, int S, int ldq, int ldk, int ldv, int ldo, float scale,
                                     mofa_stream_t stream) {
    return mofa_attn_spatial_qb_f16(q, k, v, out, nframes, heads, head_dim, S, ldq, ldk, ldv, ldo, scale, 0, stream);
}

// ---------------------------------------------------------------------------------------------------
// V [tokens][ldv] columns c (64-column blocks) -> V^T [(frame*ncb + cb)*64 + d][S]  (= [frame][C][S], any head dim).
// Not used by the attention kernels any more (they read V row-major through the LDS transpose read): the VAE mid-block
// attention, which materialises its scores with two implicit-GEMM launches, takes V^T as the weight operand of the second.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_v_kernel(const f16* __restrict__ v, f16* __restrict__ vt, int heads,
                                                          int S, int ldv) {
    __shared__ f16 s[64][66];
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * 64, head = blockIdx.y, frame = blockIdx.z;
    {
        const int key = tid >> 2, dc = (tid & 3) * 16;
        if (k0 + key < S) {
            const f16* p = v + ((size_t)frame * S + k0 + key) * ldv + head * 64 + dc;
            const f16x8 a = *(const f16x8*)p, b = *(const f16x8*)(p + 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) { s[dc + e][key] = a[e]; s[dc + 8 + e][key] = b[e]; }
        }
    }
    __syncthreads();
    {
        const int d = tid >> 2, kc = (tid & 3) * 16;
        f16* p = vt + ((size_t)(frame * heads + head) * 64 + d) * S + k0 + kc;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (k0 + kc + half * 8 < S) {
                f16x8 a;
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] = s[d][kc + half * 8 + e];
                *(f16x8*)(p + half * 8) = a;
            }
        }
    }
}

extern "C" int mofa_transpose_v_f16(const void* v, void* vt, int nframes, int heads, int S, int ldv,
                                    mofa_stream_t stream) {
    if (!v || !vt || nframes <= 0 || heads <= 0 || S <= 0 || S % 8 != 0 || ldv % 8 != 0) return MOFA_EINVAL;
    if (nframes > 65535 || heads > 65535 || ldv < heads * 64) return MOFA_EINVAL;       // grid.z / grid.y; the row holds every block
    dim3 grid(cdiv(S, 64), heads, nframes);
    hipLaunchKernelGGL(transpose_v_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const f16*)v, (f16*)vt, heads, S,
                       ldv);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

// ---------------------------------------------------------------------------------------------------
// Temporal attention: sequence = the T <= 32 frames of one (clip, pixel, head).  One wave per sequence, on the matrix
// cores: S^T = K Q^T (one 32 x 32 tile, D / 16 MFMAs; a lane owns one query, the two lane halves disjoint keys), softmax
// per lane, O^T = V^T P^T (D / 32 d-blocks x 2 MFMAs) with P straight from the S^T accumulators -- the same fragment
// algebra as attn_spatial_kernel on a single key tile.  K and V go to LDS as they are ([key][D + 8] / [key][D + 32]); the
// V^T fragments come from the LDS transpose read (lds_read_tr4).  The r01 kernel did
// the two products with fp32 VALU FMAs (2 048 per lane and sequence = 8 192 cycles per wave for 12.8 KB of traffic):
// VALU-bound at 2.5 TB/s, not HBM-bound as its roofline entry said.
// Tq query frames (rows of q / out, clip stride Tq*HW), T key/value frames (rows of k / v, clip stride T*HW): Tq < T when
// the clip's frames are sharded over ranks and K|V were all-gathered.  key_mask: bit j clear = key frame j does not exist
// (padding rows of uneven frame shards in the gathered buffer: never read, weight exactly 0).
// ---------------------------------------------------------------------------------------------------
template <int D, int WPB>
__global__ __launch_bounds__(64 * WPB) void attn_temporal_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                 const f16* __restrict__ v, f16* __restrict__ out,
                                                                 long long nseq, int Tq, int T, int HW, int heads, int ld,
                                                                 int ldkv, int ldo, float scale, unsigned key_mask) {
    constexpr int DC = D / 8;       // 16-byte chunks per row
    constexpr int KK = D / 16;      // MFMA k-steps of S^T
    constexpr int DB = D / 32;      // 32-wide output d-blocks
    constexpr int KSTR = D + 8;     // K row stride in halves (conflict-free ds_read_b128)
    constexpr int VSTR = D + 32;    // V row stride in halves (see lds_read_tr4)
    __shared__ __attribute__((aligned(16))) f16 sK[WPB][32 * KSTR];
    __shared__ __attribute__((aligned(16))) f16 sV[WPB][32 * VSTR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long seq = (long long)blockIdx.x * WPB + wave;
    if (seq >= nseq) return;                                       // (no workgroup barrier below: LDS regions are per wave)
    const int l31 = lane & 31, lh = lane >> 5;
    const int head = (int)(seq % heads);
    const long long bp = seq / heads;
    const int p = (int)(bp % HW);
    const int b = (int)(bp / HW);
    const size_t base = ((size_t)b * T * HW + p);                  // k / v token row of frame 0
    const size_t qbase = ((size_t)b * Tq * HW + p);                // q / out token row of frame 0
    f16* wK = sK[wave];
    f16* wV = sV[wave];
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // ---- K rows and V^T columns of the existing key frames; everything else stays zero (a masked key's probability is
    //      exactly 0, but 0 * NaN from never-written memory would not be) ----
    for (int c = lane; c < 32 * DC; c += 64) {
        *(f16x8*)&wK[(c / DC) * KSTR + (c % DC) * 8] = zero8;
        *(f16x8*)&wV[(c / DC) * VSTR + (c % DC) * 8] = zero8;
    }
    // Q fragments (B operand of S^T): lane (query l31, half lh) holds Q[q][16 kk + 8 lh .. + 8)
    f16x8 qf[KK];
    {
        const f16* qp = q + (qbase + (size_t)(l31 < Tq ? l31 : 0) * HW) * ld + head * D + lh * 8;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) qf[kk] = l31 < Tq ? *(const f16x8*)(qp + kk * 16) : zero8;
    }
    for (int c = lane; c < T * DC; c += 64) {
        const int t = c / DC, cc = c - t * DC;
        if (!((key_mask >> t) & 1u)) continue;
        const size_t row = base + (size_t)t * HW;
        const f16x8 kv = *(const f16x8*)(k + row * ldkv + head * D + cc * 8);
        const f16x8 vv = *(const f16x8*)(v + row * ldkv + head * D + cc * 8);
        *(f16x8*)&wK[t * KSTR + cc * 8] = kv;
        *(f16x8*)&wV[t * VSTR + cc * 8] = vv;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // this wave's LDS writes are in place
    __builtin_amdgcn_wave_barrier();

    // ---- S^T: s[r] = score(key = (r & 3) + 8 (r >> 2) + 4 lh, query = l31) ----
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    {
        const f16* kp = wK + l31 * KSTR + lh * 8;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const f16x8 kf = *(const f16x8*)(kp + kk * 16);
            s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[kk], s, 0, 0, 0);
        }
    }
    const float c2 = scale * 1.4426950408889634f;
    float mx = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int key = (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (key >= T || !((key_mask >> key) & 1u)) s[r] = -1e30f;
        mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mc = mx * c2;
    float sum = 0.f;
    f16x8 pf[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float pr = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -mc));   // masked keys: exp2(-huge) = 0
        sum += pr;
        pf[r >> 3][r & 7] = (f16)pr;
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;

    // ---- O^T[d][q] += V^T[d][key] P^T[key][q]; k-slot (8 lh + jj) of MFMA u = key 16 u + 4 lh + (jj & 3) + 8 (jj >> 2) ----
    f32x16 o[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
        const f16* vp = wV + (((lane & 15) >> 2) + 4 * lh) * VSTR + db * 32 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f16x4 lo = lds_read_tr4(vp + (u * 16) * VSTR), hi = lds_read_tr4(vp + (u * 16 + 8) * VSTR);
            const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[u], o[db], 0, 0, 0);
        }
    }
    if (l31 < Tq) {
        f16* op = out + (qbase + (size_t)l31 * HW) * ldo + head * D;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                f16x4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = (f16)(o[db][4 * qd + e] * inv);
                *(f16x4*)(op + db * 32 + 8 * qd + 4 * lh) = w;
            }
    }
}

extern "C" int mofa_attn_temporal_masked_f16(const void* q, const void* k, const void* v, void* out, int nclips, int Tq,
                                             int T, int HW, int heads, int head_dim, int ld, int ldkv, int ldo, float scale,
                                             uint32_t key_mask, mofa_stream_t stream) {
    if (!q || !k || !v || !out || nclips <= 0 || T <= 0 || T > 32 || Tq <= 0 || Tq > T || HW <= 0 || heads <= 0)
        return MOFA_EINVAL;
    if (T < 32) key_mask &= (1u << T) - 1u;
    if (key_mask == 0) return MOFA_EINVAL;
    if (ld % 8 != 0 || ldkv % 8 != 0 || ldo % 8 != 0) return MOFA_EINVAL;
    const long long nseq = (long long)nclips * HW * heads;
    if (head_dim == 64) {
        hipLaunchKernelGGL((attn_temporal_kernel<64, 4>), dim3(cdiv(nseq, 4)), dim3(256), 0, (hipStream_t)stream,
                           (const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, nseq, Tq, T, HW, heads, ld, ldkv, ldo, scale,
                           key_mask);
    } else if (head_dim == 128) {
        hipLaunchKernelGGL((attn_temporal_kernel<128, 2>), dim3(cdiv(nseq, 2)), dim3(128), 0, (hipStream_t)stream,
                           (const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, nseq, Tq, T, HW, heads, ld, ldkv, ldo, scale,
                           key_mask);
    } else {
        return MOFA_EINVAL;
    }
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

extern "C" int mofa_attn_temporal_f16(const void* q, const void* k, const void* v, void* out, int nclips, int Tq, int T,
                                      int HW, int heads, int head_dim, int ld, int ldkv, int ldo, float scale,
                                      mofa_stream_t stream) {
    return mofa_attn_temporal_masked_f16(q, k, v, out, nclips, Tq, T, HW, heads, head_dim, ld, ldkv, ldo, scale, 0xffffffffu,
                                         stream);
}

// ---------------------------------------------------------------------------------------------------
// Long temporal attention: 1 <= T <= 128 key frames per clip.  ONE body, attn_temporal_long_body.inc, included by four kernels
// that differ only in the five rule macros they define for it (the .inc names them and says what is shared):
//   attn_temporal_long_kernel         self-attention, keys < T
//   attn_temporal_long_masked_kernel  frame-sharded clips: Tq <= T query frames against T key SLOTS under a 128-bit mask
//   attn_temporal_long_local_kernel   self-attention under a per-query rule: a band round the query + the first frames
//   attn_temporal_long_window_kernel  frame-sharded clips under that rule: Tq query frames against anchor + band key SLOTS
// The body is shared as TEXT, not as an always-inlined function taking a rule object: with the body in a __device__ function
// behind one-line __global__ wrappers the compiler no longer keeps the Q-fragment arrays as one wide value -- the dense kernel's
// own text moved into such a function, nothing else changed, shows it -- and the D = 128 instantiations ran 0.4-1.1 % slower
// than the three copies.  Included, each kernel compiles to the instructions of its former copy.
// ---------------------------------------------------------------------------------------------------
#define TL_SLOT(r) (((r) & 3) + 8 * ((r) >> 2))                    // key of score r inside its lane half's 16

// Dense: key rows >= T are neither loaded nor seen, and KT = ceil(T / 32), so only the last tile reaches beyond T: the test folds
// away at compile time in every other tile.  No words.
template <int D, int KT, int WPB>
__global__ __launch_bounds__(64 * WPB) void attn_temporal_long_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                      const f16* __restrict__ v, f16* __restrict__ out,
                                                                      long long nseq, int T, int HW, int heads, int ld,
                                                                      int ldkv, int ldo, float scale) {
#define TL_TQ T
#define TL_STAGE_WORD(t0)
#define TL_STAGED(t) ((t) < T)
#define TL_WORDS(q0)
#define TL_HIDDEN(kt, r) ((kt) == KT - 1 && (kt) * 32 + TL_SLOT(r) + 4 * lh >= T)
#include "attn_temporal_long_body.inc"
}

// Masked: four wave-uniform words m0 .. m3, bit j % 32 of word j / 32 = key slot j exists; the host clears the bits at and above
// T, so the mask alone is tested, in EVERY tile (a dead slot can lie anywhere).  A dead slot is never read, neither K nor V: the
// padding slots of the gathered buffer may hold NaN.  The rows of one staging iteration lie in one mask word (UB * RPI divides
// 32), picked per iteration.  The words as a lane half sees them: q0 >> 20 is 0 (Tq <= 128); it keeps the 16 KT bit tests inside
// the query loop -- hoisted, their lane masks take 32 KT SGPRs and spill at KT >= 3.
template <int D, int KT, int WPB>
__global__ __launch_bounds__(64 * WPB) void attn_temporal_long_masked_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                             const f16* __restrict__ v, f16* __restrict__ out,
                                                                             long long nseq, int Tq, int T, int HW, int heads,
                                                                             int ld, int ldkv, int ldo, float scale, unsigned m0,
                                                                             unsigned m1, unsigned m2, unsigned m3) {
#define TL_MASK_WORD(w) ((w) == 0 ? m0 : (w) == 1 ? m1 : (w) == 2 ? m2 : m3)
#define TL_TQ Tq
#define TL_STAGE_WORD(t0) const unsigned mw = TL_MASK_WORD((t0) >> 5);
#define TL_STAGED(t) ((mw >> ((t) & 31)) & 1u)
#define TL_WORDS(q0)                    \
    unsigned ml[KT];                    \
    _Pragma("unroll") for (int kt = 0; kt < KT; ++kt) ml[kt] = (TL_MASK_WORD(kt) >> (4 * lh)) | (unsigned)((q0) >> 20);
#define TL_HIDDEN(kt, r) (!(ml[kt] & (1u << TL_SLOT(r))))
#include "attn_temporal_long_body.inc"
#undef TL_MASK_WORD
}

// Local: query frame i sees key frame j iff j < anchor or |i - j| <= radius (every query sees itself, so no row is empty); the
// host passes radius <= 127 and 0 <= anchor <= T.  All T frames are staged (other queries of the sequence need them), so K and V
// of the clip's frames must be finite: an invisible frame IS read and multiplied by its zero probability.  The rule reaches a
// lane as KT words built per query block and tested like the masked kernel's, in every tile: three VALU instructions per score,
// 1-7 % over the dense kernel's time.  The band's keys lo .. hi lie inside [0, T) and anchor <= T, so keys >= T are invisible;
// query rows >= T are not stored and take the band of row T - 1.  below(n) = the n lowest bits, n clamped to 0 .. 32.
template <int D, int KT, int WPB>
__global__ __launch_bounds__(64 * WPB) void attn_temporal_long_local_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                            const f16* __restrict__ v, f16* __restrict__ out,
                                                                            long long nseq, int T, int HW, int heads, int ld,
                                                                            int ldkv, int ldo, float scale, int radius,
                                                                            int anchor) {
#define TL_TQ T
#define TL_STAGE_WORD(t0)
#define TL_STAGED(t) ((t) < T)
#define TL_WORDS(q0)                                                                                                \
    const int qi = min((q0) + l31, T - 1);                                                                          \
    const int lo = max(qi - radius, 0), hi1 = min(qi + radius, T - 1) + 1;                                          \
    unsigned ml[KT];                                                                                                \
    _Pragma("unroll") for (int kt = 0; kt < KT; ++kt) {                                                             \
        const auto below = [](int n) { return (unsigned)((1ull << min(max(n, 0), 32)) - 1ull); };                   \
        ml[kt] = (below(anchor - 32 * kt) | (below(hi1 - 32 * kt) & ~below(lo - 32 * kt))) >> (4 * lh);             \
    }
#define TL_HIDDEN(kt, r) (!(ml[kt] & (1u << TL_SLOT(r))))
#include "attn_temporal_long_body.inc"
}

// Window: the local rule on the key buffer of a frame shard -- Tq query rows (global frames q_frame0 .. q_frame0 + Tq - 1)
// against T key SLOTS: slots [0, anchor) hold the global frames 0 .. anchor - 1, slot s >= anchor holds the global frame
// band_frame0 + (s - anchor).  Rectangular like the masked kernel, per-query words like the local kernel.  A query of global
// frame g sees every anchor slot, and band slot s iff its frame f >= anchor (a band slot that repeats an anchor frame is staged
// but hidden: every key counts once) and |g - f| <= radius.  In slot space that is [lo, hi1) with
//   lo  = anchor + max(g - radius, anchor, band_frame0) - band_frame0    (>= anchor)
//   hi1 = anchor + min(g + radius, band_frame0 + L - 1) - band_frame0 + 1    (<= T; L = T - anchor band slots)
// and lo >= hi1 (a query below the anchor whose band lies inside the anchor frames) leaves the band empty.  The host passes
// radius <= 127, 0 <= anchor <= T and band_frame0 <= q_frame0, q_frame0 + Tq <= band_frame0 + L, so every query's own frame
// is in the band or among the anchors and no row is empty.  All T slots are staged: K and V of every slot must be finite.
// Query rows >= Tq are not stored and take the words of row Tq - 1.
template <int D, int KT, int WPB>
__global__ __launch_bounds__(64 * WPB) void attn_temporal_long_window_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                             const f16* __restrict__ v, f16* __restrict__ out,
                                                                             long long nseq, int Tq, int T, int HW, int heads,
                                                                             int ld, int ldkv, int ldo, float scale, int radius,
                                                                             int anchor, int q_frame0, int band_frame0) {
#define TL_TQ Tq
#define TL_STAGE_WORD(t0)
#define TL_STAGED(t) ((t) < T)
#define TL_WORDS(q0)                                                                                                \
    const int g = q_frame0 + min((q0) + l31, Tq - 1);                                                               \
    const int lo = anchor + max(max(g - radius, anchor), band_frame0) - band_frame0;                                \
    const int hi1 = anchor + min(g + radius, band_frame0 + (T - anchor) - 1) - band_frame0 + 1;                     \
    unsigned ml[KT];                                                                                                \
    _Pragma("unroll") for (int kt = 0; kt < KT; ++kt) {                                                             \
        const auto below = [](int n) { return (unsigned)((1ull << min(max(n, 0), 32)) - 1ull); };                   \
        ml[kt] = (below(anchor - 32 * kt) | (below(hi1 - 32 * kt) & ~below(lo - 32 * kt))) >> (4 * lh);             \
    }
#define TL_HIDDEN(kt, r) (!(ml[kt] & (1u << TL_SLOT(r))))
#include "attn_temporal_long_body.inc"
}

// ---------------------------------------------------------------------------------------------------
// Streaming local temporal attention: the local rule (above) for 1 <= T <= 1024 frames under radius <= 32 and anchor <= 32.  A
// 32-query block tq = q0 / 32 then sees only frame tile 0 (the anchors) and the frame tiles tq - 1, tq, tq + 1 (the band), so
// the wave keeps FOUR 32-row tile slots in its LDS region -- the strides and the byte count of the KT = 4 geometry -- however
// long the clip is:
//   slot 0       frame tile 0, staged once, for the whole sequence
//   slots 1 .. 3 a ring: frame tile t >= 1 lives in slot 1 + t % 3
// and every block computes four register score tiles in the order [tile 0, tq - 1, tq, tq + 1].  The first carries the full
// rule (anchor and band); a band tile that is out of range (< 0 or >= ceil(T / 32)) or IS tile 0 is hidden as a whole: score
// -1e30 before the maximum, probability exactly 0.  So every key is counted once and the tiles are visited in ascending frame
// order: the nonzero terms of the fp32 row sum and of O^T are those of the local kernel (T <= 128) in its order, and exact
// zeros move neither -- the two kernels agree bit for bit there.  No tile is skipped by a branch (see the body file).
// Ring: before block 0 tile 1 is staged into slot 2 and slots 1 and 3 are zero-filled (tile 0 never enters the ring: its band
// copy is hidden); after block tq, tile tq + 2 is staged into the slot tile tq - 1 leaves -- tq + 2 = tq - 1 (mod 3).  The
// tile's global loads are issued at the top of the block into registers (16 / 32 VGPRs each for K and V) and travel under its
// arithmetic; its LDS stores follow the block's last LDS read in program order, behind s_waitcnt lgkmcnt(0) and a wave barrier,
// and one wave's LDS operations execute in order; a second wait and barrier precede the next block's reads.  The refill is
// unconditional (the last blocks write zeros), so the loop body has no branch.  At three (D = 64) or two (D = 128) waves per CU
// -- the LDS decides, not the registers -- nothing else hides the load: without the prefetch the kernel ran 1.12-1.22 x its
// time.  K and V leave HBM once.
// Every row an MFMA can read is finite at all times: rows of frames >= T are written as zero, the slots of tile -1 (block 0) and
// of tiles past the last hold zeros or an earlier, finite tile.  Precondition as for the local kernel: K and V of all T frames
// are finite.  Query rows >= T are neither loaded nor stored.
// ---------------------------------------------------------------------------------------------------
// What the three streaming kernels (this one and the two walks below) share outside their block loops, as text: as
// __forceinline__ functions -- the fragments by reference or in a returned struct -- each of the three changed the instructions
// of every kernel that called it.
// one wave per sequence: the wave's lanes (query l31, half lh) and its sequence (clip b, pixel p, head); a workgroup's last waves
// may have none and leave (no workgroup barrier follows: LDS regions are per wave); wK / wV: the wave's LDS region of ROWS key rows
#define TEMPORAL_WAVE_DECODE(ROWS)                                 \
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6; \
    const long long seq = (long long)blockIdx.x * WPB + wave;      \
    if (seq >= nseq) return;                                       \
    const int l31 = lane & 31, lh = lane >> 5;                     \
    const int head = (int)(seq % heads);                           \
    const long long bp = seq / heads;                              \
    const int p = (int)(bp % HW);                                  \
    const int b = (int)(bp / HW);                                  \
    extern __shared__ __attribute__((aligned(16))) char smem_ts[]; \
    f16* wK = (f16*)smem_ts + (size_t)wave * ((ROWS) * (2 * D + 40)); \
    f16* wV = wK + (ROWS) * (D + 8);

// Q fragments of the 32-query block of this lane's query row `row` (B operand of S^T): lane (query l31, half lh) holds
// Q[row][16 kk + 8 lh .. + 8); rows >= Tq are not read and become zero
#define TEMPORAL_LOAD_Q(qf, row, qbase, Tq)                                                                    \
    {                                                                                                          \
        const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};                                                          \
        const int qi = (row);                                                                                  \
        const f16* qp = q + ((qbase) + (size_t)(qi < (Tq) ? qi : 0) * HW) * ld + head * D + lh * 8;            \
        _Pragma("unroll") for (int kk = 0; kk < D / 16; ++kk) (qf)[kk] = qi < (Tq) ? *(const f16x8*)(qp + kk * 16) : zero8; \
    }
// O^T of this lane's query row `row`, times inv, to its token row; rows >= Tq are not stored
#define TEMPORAL_STORE_O(o, inv, row, qbase, Tq)                                                               \
    if ((row) < (Tq)) {                                                                                        \
        f16* op = out + ((qbase) + (size_t)(row) * HW) * ldo + head * D;                                       \
        _Pragma("unroll") for (int db = 0; db < D / 32; ++db)                                                  \
            _Pragma("unroll") for (int qd = 0; qd < 4; ++qd) {                                                 \
                f16x4 w;                                                                                       \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) w[e] = (f16)((o)[db][4 * qd + e] * (inv));       \
                *(f16x4*)(op + db * 32 + 8 * qd + 4 * lh) = w;                                                 \
            }                                                                                                  \
    }

// one 32-row tile of K and V in flight between memory and its LDS slot: lane (r0, cc) holds the 16-byte chunk cc of the rows
// r0, r0 + RPI, ...
template <int D>
struct TemporalStreamTile {
    static constexpr int DC = D / 8, KSTR = D + 8, VSTR = D + 32, RPI = 64 / DC, N = 32 / RPI;
    f16x8 gk[N], gv[N];
    // frame rows t_first .. t_first + 32; rows >= T are not read and become zero
    __device__ __forceinline__ void load(const f16* __restrict__ k, const f16* __restrict__ v, size_t base, int HW, int ldkv, int head,
                                         int T, int t_first, int lane) {
        const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const int r0 = lane / DC, cc = lane % DC;
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const int t = t_first + u * RPI + r0;
            gk[u] = zero8; gv[u] = zero8;
            if (t < T) {
                const size_t off = (base + (size_t)t * HW) * ldkv + head * D + cc * 8;
                gk[u] = *(const f16x8*)(k + off);
                gv[u] = *(const f16x8*)(v + off);
            }
        }
    }
    // into the 32-row slot at rk / rv
    __device__ __forceinline__ void store(f16* rk, f16* rv, int lane) const {
        const int r0 = lane / DC, cc = lane % DC;
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const int i = u * RPI + r0;
            *(f16x8*)&rk[i * KSTR + cc * 8] = gk[u];
            *(f16x8*)&rv[i * VSTR + cc * 8] = gv[u];
        }
    }
};

template <int D, int WPB>
__global__ __launch_bounds__(64 * WPB) void attn_temporal_stream_local_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                              const f16* __restrict__ v, f16* __restrict__ out,
                                                                              long long nseq, int T, int HW, int heads, int ld,
                                                                              int ldkv, int ldo, float scale, int radius,
                                                                              int anchor) {
    constexpr int KK = D / 16, DB = D / 32, KSTR = D + 8, VSTR = D + 32;
    constexpr int NS = 4, ROWS = 32 * NS;                          // tile slots, rows of the wave's region
    TEMPORAL_WAVE_DECODE(ROWS)
    const size_t base = ((size_t)b * T * HW + p);              // q / k / v / out token row of frame 0

    f16x8 qf[KK];
    TEMPORAL_LOAD_Q(qf, l31, base, T)
    // slot 0 <- tile 0, slot 2 <- tile 1, slots 1 and 3 <- zero (t_first = T: no row is read)
    {
        TemporalStreamTile<D> t0, t1, tz;
        t0.load(k, v, base, HW, ldkv, head, T, 0, lane);
        t1.load(k, v, base, HW, ldkv, head, T, 32, lane);
        tz.load(k, v, base, HW, ldkv, head, T, T, lane);
        t0.store(wK, wV, lane);
        t1.store(wK + 64 * KSTR, wV + 64 * VSTR, lane);
        tz.store(wK + 32 * KSTR, wV + 32 * VSTR, lane);
        tz.store(wK + 96 * KSTR, wV + 96 * VSTR, lane);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // this wave's LDS writes are in place
    __builtin_amdgcn_wave_barrier();

    const float c2 = scale * 1.4426950408889634f;
    const int tr_off = (((lane & 15) >> 2) + 4 * lh) * VSTR + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    int sa = 3, sb = 1, sc = 2;                                    // the slots of tiles tq - 1, tq, tq + 1 (tile t: 1 + t % 3)
#pragma unroll 1
    for (int q0 = 0; q0 < T; q0 += 32) {
        const int tq = q0 >> 5;
        const int slot[NS] = {0, sa, sb, sc};
        // tile tq + 2 travels to registers under this block's arithmetic (rows >= T, the last blocks: nothing is read)
        TemporalStreamTile<D> nt;
        nt.load(k, v, base, HW, ldkv, head, T, q0 + 64, lane);
        // the next block's Q fragments are fetched under this block's arithmetic
        f16x8 qn[KK];
        TEMPORAL_LOAD_Q(qn, q0 + 32 + l31, base, T)
        // the rule as four words, as in the local kernel: tile 0 with anchor and band; band tiles with the band alone, which is
        // empty by itself for a tile < 0 or >= ceil(T / 32) (lo >= 0, hi1 <= T) and is emptied for the band copy of tile 0
        unsigned ml[NS];
        {
            const int qi = min(q0 + l31, T - 1);
            const int lo = max(qi - radius, 0), hi1 = min(qi + radius, T - 1) + 1;
            const auto below = [](int n) { return (unsigned)((1ull << min(max(n, 0), 32)) - 1ull); };
            ml[0] = (below(anchor) | (below(hi1) & ~below(lo))) >> (4 * lh);
#pragma unroll
            for (int j = 1; j < NS; ++j) {
                const int tt = tq + j - 2;
                const unsigned band = below(hi1 - 32 * tt) & ~below(lo - 32 * tt);
                ml[j] = (tt == 0 ? 0u : band) >> (4 * lh);
            }
        }
        // ---- S^T tiles: s[j][r] = score(key = 32 tile(j) + (r & 3) + 8 (r >> 2) + 4 lh, query = q0 + l31) ----
        f32x16 s[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[j][r] = 0.f;
            const f16* kp = wK + (slot[j] * 32 + l31) * KSTR + lh * 8;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const f16x8 kf = *(const f16x8*)(kp + kk * 16);
                s[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[kk], s[j], 0, 0, 0);
            }
        }
        float mx = -1e30f;
#pragma unroll
        for (int j = 0; j < NS; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (!(ml[j] & (1u << TL_SLOT(r)))) s[j][r] = -1e30f;
                mx = fmaxf(mx, s[j][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mc = mx * c2;
        float sum = 0.f;
        f16x8 pf[NS][2];
#pragma unroll
        for (int j = 0; j < NS; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pr = __builtin_amdgcn_exp2f(fmaf(s[j][r], c2, -mc));   // hidden keys: exp2(-huge) = 0
                sum += pr;
                pf[j][r >> 3][r & 7] = (f16)pr;
            }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;

        // ---- O^T[d][q] += V^T[d][key] P^T[key][q], k-slots as in the body file ----
        f32x16 o[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
            const f16* vp = wV + tr_off + db * 32;
#pragma unroll
            for (int j = 0; j < NS; ++j)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const f16x4 lo = lds_read_tr4(vp + (slot[j] * 32 + u * 16) * VSTR), hi = lds_read_tr4(vp + (slot[j] * 32 + u * 16 + 8) * VSTR);
                    const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[j][u], o[db], 0, 0, 0);
                }
        }
        // ---- ring refill: tile tq + 2 into the slot of tile tq - 1, after this block's last LDS read ----
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        nt.store(wK + sa * 32 * KSTR, wV + sa * 32 * VSTR, lane);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        TEMPORAL_STORE_O(o, inv, q0 + l31, base, T)
        const int s0 = sa;
        sa = sb; sb = sc; sc = s0;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) qf[kk] = qn[kk];
    }
}

// ---------------------------------------------------------------------------------------------------
// Streaming temporal attention under ANY window of the local rule, dense included: 1 <= T <= 1024 frames, radius >= 0 (the host
// clamps it to T - 1), 0 <= anchor <= T.  The online-softmax walk of attn_temporal_stream_body.inc -- the body file says what a
// wave keeps across the tiles, where the arithmetic's two hazards lie and how a tile travels -- over whole clips: per 32-query
// block q0 it visits, in ascending frame order and each once, the key tiles that hold a key some query of the block can see
//   anchor tiles  0 .. ceil(anchor / 32) - 1
//   band tiles    (max(q0 - radius, 0) >> 5) .. (min(q0 + 31 + radius, T - 1) >> 5), those not among the anchor tiles
// Every row meets a visible key in some visited tile (itself).  The walk is the same for a rule that hides nothing however it is
// spelt (radius >= T - 1, or anchor = T): all tiles, ascending, every probability from exp2 -- equal bits.
// Frame rows >= T are not read (they are the next clip's) and are written as zero; K and V of all T frames must be finite.  Query
// rows >= T take the rule of row T - 1.  What stays here is what differs from the shard kernel: the clip strides, the rows of a
// tile that are loaded, the lane's band and how the walk names its first and next tile (the body's seven macros).
// ---------------------------------------------------------------------------------------------------
template <int D, int WPB>
__global__ __launch_bounds__(64 * WPB) void attn_temporal_stream_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                        const f16* __restrict__ v, f16* __restrict__ out,
                                                                        long long nseq, int T, int HW, int heads, int ld,
                                                                        int ldkv, int ldo, float scale, int radius, int anchor) {
    TEMPORAL_WAVE_DECODE(32)
    const int Tq = T;
    const size_t base = ((size_t)b * T * HW + p), qbase = base;   // q / k / v / out token row of frame 0
    const int nA = (anchor + 31) >> 5;                             // anchor tiles
    const auto first_tile = [&](int q0) { return nA > 0 ? 0 : max(q0 - radius, 0) >> 5; };
#define TS_FIRST(t0) t0.load(k, v, base, HW, ldkv, head, T, first_tile(0) * 32, lane);
// the block's walk: tiles 0 .. nA - 1, then band0 .. last; this lane's query qi and its band
#define TS_BLOCK(q0)                                                                  \
    const int band0 = max(max((q0) - radius, 0) >> 5, nA);                            \
    const int last = max(min((q0) + 31 + radius, T - 1) >> 5, nA - 1);                \
    const int qi = min((q0) + l31, T - 1);                                            \
    const int lo = max(qi - radius, 0), hi1 = min(qi + radius, T - 1) + 1;
#define TS_START int kt = nA > 0 ? 0 : band0;
#define TS_NEXT(nt)                                                                   \
    int nk = kt + 1;                                                                  \
    if (nk >= nA && nk < band0) nk = band0;                                           \
    const bool more = nk <= last;                                                     \
    TemporalStreamTile<D> nt;                                                         \
    nt.load(k, v, base, HW, ldkv, head, T, more ? nk * 32 : q0 + 32 < T ? first_tile(q0 + 32) * 32 : T, lane); \
    const auto below = [](int n) { return (unsigned)((1ull << min(max(n, 0), 32)) - 1ull); };
#define TS_AND_WORD(kt)
#define TS_ADVANCE kt = nk;
#define TS_STORE(t) t.store(wK, wV, lane);
#include "attn_temporal_stream_body.inc"
}

// ---------------------------------------------------------------------------------------------------
// The streaming walk on the key buffer of a FRAME SHARD: Tq query rows of a clip (clip stride Tq * HW in q / out) against
// 1 <= S <= 1024 key SLOTS (clip stride S * HW in k / v).  The tile walk's step, the online softmax and the KT = 1 geometry are the
// text of attn_temporal_stream_kernel: attn_temporal_stream_body.inc (its header holds here, the two hazards and their selects
// included); what differs is which slots a query sees.  ONE rule serves both forms of a sharded clip, a slot being seen iff the window shows it AND it exists:
//   window   slots [0, anchor) hold the global frames 0 .. anchor - 1, slot s >= anchor the global frame band_frame0 + (s - anchor);
//            the query of global frame g = q_frame0 + row sees the anchor slots and the band slots [lo, hi1) of
//            attn_temporal_long_window_kernel (frame >= anchor and within radius of g: a band slot that repeats an anchor frame
//            counts zero times).  Every slot below S exists.  K and V of every slot must be finite.
//   dense    the host passes radius = 2^30, anchor = 0 and both frames 0, so the window is [0, S) for every query, and the 32 mask
//            words say which slots exist: bit j % 32 of word j / 32 (the host clears the bits at and above S).  The K / V rows of a
//            slot that does not exist are never read from memory -- the padding slots of a gathered buffer hold whatever the
//            allocator left -- and enter the tile as zeros.
// The words travel as kernel arguments and live in ONE VGPR, lane j (and j + 32) holding word j: the word of the running tile is
// read with v_readlane, so the array is never indexed in private memory, and the ballot of the non-zero words is the set of tiles
// that exist.  Per 32-query block the walk visits, ascending and once each, the anchor tiles and the band tiles that hold a slot
// some query of the block can see (the union of the queries' [lo, hi1) is [lo of the first, hi1 of the last)), each only if it
// exists; no other tile is visited.  The tiles of a block are one wave-uniform 32-bit set.
// Bit-level anchors, kept true by running the same arithmetic on the same visible keys in the same order:
//   (a) dense, every slot, Tq == S: the bits of attn_temporal_stream_kernel dense;
//   (b) dense, every slot, Tq < S, on the q rows f0 .. f0 + Tq - 1 of a clip: the bits of those rows of (a) -- in dense mode a
//       query's arithmetic depends on its own row and the ascending walk over all tiles, not on how the 32-query blocks are
//       aligned (the rescale skipped where no lane's maximum moved changes no bit);
//   (c) window with anchor = 0, q_frame0 = band_frame0 = 0, Tq == S: the bits of attn_temporal_stream_kernel under (radius, 0);
//   (d) the contents of slots that do not exist change no bit.
// Query rows >= Tq take the rule of row Tq - 1 and are neither loaded nor stored; slot rows >= S are the next clip's and are not
// read.
// ---------------------------------------------------------------------------------------------------
struct TemporalShardWords {
    unsigned w[32];
};

template <int D, int WPB>
__global__ __launch_bounds__(64 * WPB) void attn_temporal_stream_shard_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                              const f16* __restrict__ v, f16* __restrict__ out,
                                                                              long long nseq, int Tq, int S, int HW, int heads,
                                                                              int ld, int ldkv, int ldo, float scale, int radius,
                                                                              int anchor, int q_frame0, int band_frame0,
                                                                              TemporalShardWords words) {
    TEMPORAL_WAVE_DECODE(32)
    const size_t base = ((size_t)b * S * HW + p);              // k / v token row of slot 0
    const size_t qbase = ((size_t)b * Tq * HW + p);            // q / out token row of the first query frame
    const auto below = [](int n) { return (unsigned)((1ull << min(max(n, 0), 32)) - 1ull); };

    // the 32 mask words in one register: lane j holds word j; exist = the tiles that hold a slot
    unsigned mwv = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) mwv = l31 == j ? words.w[j] : mwv;
    const unsigned exist = (unsigned)__ballot(mwv != 0);
    const auto word = [&](int kt) { return (unsigned)__builtin_amdgcn_readlane((int)mwv, kt); };

    const int nA = (anchor + 31) >> 5;                             // anchor tiles
    const int hi_f = band_frame0 + (S - anchor) - 1;               // the last band frame
    // the tiles of the query block at q0 (wave-uniform): the anchor tiles and the band tiles of slots [lo of the block's first
    // query, hi1 of its last), those that exist.  Never empty: a query's own frame is a slot (window); some slot exists (dense).
    const auto tiles = [&](int q0) {
        const int g0 = q_frame0 + q0, g1 = q_frame0 + min(q0 + 31, Tq - 1);
        const int lo = anchor + max(max(g0 - radius, anchor), band_frame0) - band_frame0;
        const int hi1 = anchor + min(g1 + radius, hi_f) - band_frame0 + 1;
        unsigned t = below(nA);
        if (lo < hi1) t |= below(((hi1 - 1) >> 5) + 1) & ~below(lo >> 5);
        return t & exist;
    };
    // tile kt between memory and the slot: rows of slots that do not exist (bit i of w clear for row 32 kt + i; every row under a
    // zero word) are not read and become zero.  The load and the store stay the kernel's own text: through TemporalStreamTile's,
    // with a row predicate and the slot's pointers as arguments, the kernel compiles to other code
    constexpr int DC = D / 8, RPI = 64 / DC, NR = 32 / RPI;
    const int r0 = lane / DC, cc = lane % DC;
    const auto tile_load = [&](TemporalStreamTile<D>& t, int kt, unsigned w) {
        const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int i = u * RPI + r0;
            t.gk[u] = zero8; t.gv[u] = zero8;
            if ((w >> i) & 1u) {
                const size_t off = (base + (size_t)(kt * 32 + i) * HW) * ldkv + head * D + cc * 8;
                t.gk[u] = *(const f16x8*)(k + off);
                t.gv[u] = *(const f16x8*)(v + off);
            }
        }
    };
    const auto tile_store = [&](const TemporalStreamTile<D>& t) {
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int i = u * RPI + r0;
            *(f16x8*)&wK[i * (D + 8) + cc * 8] = t.gk[u];
            *(f16x8*)&wV[i * (D + 32) + cc * 8] = t.gv[u];
        }
    };
    unsigned tl_next;                                              // the tiles of the next block
#define TS_FIRST(t0)                        \
    tl_next = tiles(0);                     \
    const int kt0 = __builtin_ctz(tl_next); \
    tile_load(t0, kt0, word(kt0));
// the block's tiles tl, one 32-bit set (rest: those after kt); this lane's query g and its band slots (lo >= hi1: a query below
// the anchor whose band lies inside it)
#define TS_BLOCK(q0)                                                                  \
    const unsigned tl = tl_next;                                                      \
    tl_next = (q0) + 32 < Tq ? tiles((q0) + 32) : 0u;                                 \
    const int g = q_frame0 + min((q0) + l31, Tq - 1);                                 \
    const int lo = anchor + max(max(g - radius, anchor), band_frame0) - band_frame0;  \
    const int hi1 = anchor + min(g + radius, hi_f) - band_frame0 + 1;
#define TS_START                \
    int kt = __builtin_ctz(tl); \
    unsigned rest = tl & (tl - 1u);
#define TS_NEXT(nt)                               \
    const bool more = rest != 0u;                 \
    const unsigned nxt = more ? rest : tl_next;   \
    const int nk = nxt ? __builtin_ctz(nxt) : 0;  \
    TemporalStreamTile<D> nt;                     \
    tile_load(nt, nk, nxt ? word(nk) : 0u);
#define TS_AND_WORD(kt) & word(kt)
#define TS_ADVANCE \
    kt = nk;       \
    rest &= rest - 1u;
#define TS_STORE(t) tile_store(t);
#include "attn_temporal_stream_body.inc"
}
#undef TL_SLOT
#undef TEMPORAL_WAVE_DECODE
#undef TEMPORAL_LOAD_Q
#undef TEMPORAL_STORE_O

// waves per workgroup: as many as keep a workgroup's LDS at or below 42 KB (D = 64) / 37 KB (D = 128), at least one
template <int D_, int KT_>
struct TemporalLongGeom {
    static constexpr int D = D_, KT = KT_;
    static constexpr int WPB = D == 64 ? (KT == 1 ? 4 : KT == 2 ? 2 : 1) : (KT == 1 ? 2 : 1);
    static constexpr int LDS = WPB * 32 * KT * (2 * D + 40) * 2;
};

// one launcher for the three forms: Kernel is a template argument, so the LDS opt-in (per function and per device) is taken
// once per kernel instantiation
template <class G, auto Kernel, class... Args>
static int launch_temporal_long(long long nseq, hipStream_t st, Args... args) {
    const long long nwg = (nseq + G::WPB - 1) / G::WPB;
    if (nwg > 0x7fffffffLL) return MOFA_EINVAL;
    static LaunchSetup setup;
    if (setup.cus([](int) { return mofa_lds_optin((const void*)Kernel, G::LDS); }) == 0) return MOFA_ELAUNCH;
    hipLaunchKernelGGL(Kernel, dim3((unsigned)nwg), dim3(64 * G::WPB), G::LDS, st, args...);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}

// the (head dim, key tiles) instantiation of a call: f(TemporalLongGeom<D, KT>{})
template <class F>
static int temporal_long_dispatch(int head_dim, int T, F&& f) {
    const int kt = (T + 31) / 32;
#define MOFA_TL_CASE(D_, KT_) \
    if (head_dim == D_ && kt == KT_) return f(TemporalLongGeom<D_, KT_>{});
    MOFA_TL_CASE(64, 1) MOFA_TL_CASE(64, 2) MOFA_TL_CASE(64, 3) MOFA_TL_CASE(64, 4)
    MOFA_TL_CASE(128, 1) MOFA_TL_CASE(128, 2) MOFA_TL_CASE(128, 3) MOFA_TL_CASE(128, 4)
#undef MOFA_TL_CASE
    return MOFA_EINVAL;
}

// the streaming kernels' instantiation of a call, the key tiles fixed by the kernel: f(TemporalLongGeom<D, KT>{})
template <int KT, class F>
static int temporal_stream_dispatch(int head_dim, F&& f) {
    return head_dim == 64 ? f(TemporalLongGeom<64, KT>{}) : f(TemporalLongGeom<128, KT>{});
}

// the mask words of n key slots: word w of key_mask (NULL = every slot) with the bits at and above n cleared; 0 for a word that
// begins at or above n, which is not read
static uint32_t temporal_mask_word(const uint32_t* key_mask, int w, int n) {
    const int left = n - 32 * w;                                    // slots of this word below n
    const uint32_t below = left >= 32 ? 0xffffffffu : left > 0 ? (1u << left) - 1u : 0u;
    return below ? (key_mask ? key_mask[w] : 0xffffffffu) & below : 0u;
}

// what the three entry points ask of their common arguments (the streaming entry: the same with its own longest clip)
static bool temporal_long_args_ok(const void* q, const void* k, const void* v, const void* out, int nclips, int T, int HW, int heads,
                                  int head_dim, int ld, int ldkv, int ldo, int max_T = 128) {
    if (!q || !k || !v || !out || nclips <= 0 || T < 1 || T > max_T || HW <= 0 || heads <= 0) return false;
    if (head_dim != 64 && head_dim != 128) return false;
    return ld > 0 && ldkv > 0 && ldo > 0 && ld % 8 == 0 && ldkv % 8 == 0 && ldo % 8 == 0;
}

extern "C" int mofa_attn_temporal_long_f16(const void* q, const void* k, const void* v, void* out, int nclips, int T, int HW,
                                           int heads, int head_dim, int ld, int ldkv, int ldo, float scale,
                                           mofa_stream_t stream) {
    if (!temporal_long_args_ok(q, k, v, out, nclips, T, HW, heads, head_dim, ld, ldkv, ldo)) return MOFA_EINVAL;
    const long long nseq = (long long)nclips * HW * heads;
    return temporal_long_dispatch(head_dim, T, [&](auto g) {
        using G = decltype(g);
        return launch_temporal_long<G, attn_temporal_long_kernel<G::D, G::KT, G::WPB>>(
            nseq, (hipStream_t)stream, (const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, nseq, T, HW, heads, ld, ldkv, ldo, scale);
    });
}

// key_mask: host memory, four words, bit j % 32 of word j / 32 = key slot j exists; NULL = every slot below T.  Bits at and
// above T are ignored (cleared here: the kernel tests the mask alone).  The words travel as kernel arguments.
extern "C" int mofa_attn_temporal_long_masked_f16(const void* q, const void* k, const void* v, void* out, int nclips, int Tq,
                                                  int T, int HW, int heads, int head_dim, int ld, int ldkv, int ldo, float scale,
                                                  const uint32_t* key_mask, mofa_stream_t stream) {
    if (!temporal_long_args_ok(q, k, v, out, nclips, T, HW, heads, head_dim, ld, ldkv, ldo) || Tq < 1 || Tq > T) return MOFA_EINVAL;
    uint32_t m[4];
    for (int w = 0; w < 4; ++w) m[w] = temporal_mask_word(key_mask, w, T);
    if ((m[0] | m[1] | m[2] | m[3]) == 0) return MOFA_EINVAL;
    const long long nseq = (long long)nclips * HW * heads;
    return temporal_long_dispatch(head_dim, T, [&](auto g) {
        using G = decltype(g);
        return launch_temporal_long<G, attn_temporal_long_masked_kernel<G::D, G::KT, G::WPB>>(
            nseq, (hipStream_t)stream, (const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, nseq, Tq, T, HW, heads, ld, ldkv, ldo, scale,
            m[0], m[1], m[2], m[3]);
    });
}

// query frame i sees key frame j iff j < anchor or |i - j| <= radius; radius > T - 1 means "all" (clamped here: the kernel adds
// it to a frame index)
extern "C" int mofa_attn_temporal_long_local_f16(const void* q, const void* k, const void* v, void* out, int nclips, int T, int HW,
                                                 int heads, int head_dim, int ld, int ldkv, int ldo, float scale, int radius,
                                                 int anchor, mofa_stream_t stream) {
    if (!temporal_long_args_ok(q, k, v, out, nclips, T, HW, heads, head_dim, ld, ldkv, ldo)) return MOFA_EINVAL;
    if (radius < 0 || anchor < 0 || anchor > T) return MOFA_EINVAL;
    if (radius > 127) radius = 127;
    const long long nseq = (long long)nclips * HW * heads;
    return temporal_long_dispatch(head_dim, T, [&](auto g) {
        using G = decltype(g);
        return launch_temporal_long<G, attn_temporal_long_local_kernel<G::D, G::KT, G::WPB>>(
            nseq, (hipStream_t)stream, (const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, nseq, T, HW, heads, ld, ldkv, ldo, scale,
            radius, anchor);
    });
}

// the local rule on a frame shard's key buffer: Tq query frames from global frame q_frame0 on against S slots = `anchor` anchor
// frames + the band frames band_frame0 .. band_frame0 + (S - anchor) - 1 (attn_temporal_long_window_kernel).  The queries' own
// frames must lie in the band (the last two rules); band_frame0 above 2^30 is refused so that no frame sum overflows an int
extern "C" int mofa_attn_temporal_long_window_f16(const void* q, const void* k, const void* v, void* out, int nclips, int Tq,
                                                  int S, int HW, int heads, int head_dim, int ld, int ldkv, int ldo, float scale,
                                                  int radius, int anchor, int q_frame0, int band_frame0, mofa_stream_t stream) {
    if (!temporal_long_args_ok(q, k, v, out, nclips, S, HW, heads, head_dim, ld, ldkv, ldo) || Tq < 1) return MOFA_EINVAL;
    if (radius < 0 || anchor < 0 || anchor > S || band_frame0 < 0 || band_frame0 > (1 << 30)) return MOFA_EINVAL;
    if (q_frame0 < band_frame0 || (long long)q_frame0 + Tq > (long long)band_frame0 + (S - anchor)) return MOFA_EINVAL;
    if (radius > 127) radius = 127;
    const long long nseq = (long long)nclips * HW * heads;
    return temporal_long_dispatch(head_dim, S, [&](auto g) {
        using G = decltype(g);
        return launch_temporal_long<G, attn_temporal_long_window_kernel<G::D, G::KT, G::WPB>>(
            nseq, (hipStream_t)stream, (const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, nseq, Tq, S, HW, heads, ld, ldkv, ldo, scale,
            radius, anchor, q_frame0, band_frame0);
    });
}

// the local rule for 1 <= T <= 1024 frames under radius <= 32 and anchor <= 32 (attn_temporal_stream_local_kernel): the
// KT = 4 geometry -- one wave per workgroup, four tile slots -- for every T
extern "C" int mofa_attn_temporal_stream_local_f16(const void* q, const void* k, const void* v, void* out, int nclips, int T,
                                                   int HW, int heads, int head_dim, int ld, int ldkv, int ldo, float scale,
                                                   int radius, int anchor, mofa_stream_t stream) {
    if (!temporal_long_args_ok(q, k, v, out, nclips, T, HW, heads, head_dim, ld, ldkv, ldo, 1024)) return MOFA_EINVAL;
    if (radius < 0 || radius > 32 || anchor < 0 || anchor > 32 || anchor > T) return MOFA_EINVAL;
    const long long nseq = (long long)nclips * HW * heads;
    return temporal_stream_dispatch<4>(head_dim, [&](auto g) {
        using G = decltype(g);
        return launch_temporal_long<G, attn_temporal_stream_local_kernel<G::D, G::WPB>>(
            nseq, (hipStream_t)stream, (const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, nseq, T, HW, heads, ld, ldkv, ldo, scale,
            radius, anchor);
    });
}

// the local rule for 1 <= T <= 1024 frames under ANY radius >= 0 and 0 <= anchor <= T, dense (radius >= T - 1) included
// (attn_temporal_stream_kernel: an online-softmax walk over the visible key tiles).  radius >= T - 1 hides nothing and is clamped
// (the kernel adds it to a frame index).  The KT = 1 geometry: one tile slot a wave, four (D = 64) / two (D = 128) waves a workgroup
extern "C" int mofa_attn_temporal_stream_f16(const void* q, const void* k, const void* v, void* out, int nclips, int T, int HW,
                                             int heads, int head_dim, int ld, int ldkv, int ldo, float scale, int radius,
                                             int anchor, mofa_stream_t stream) {
    if (!temporal_long_args_ok(q, k, v, out, nclips, T, HW, heads, head_dim, ld, ldkv, ldo, 1024)) return MOFA_EINVAL;
    if (radius < 0 || anchor < 0 || anchor > T) return MOFA_EINVAL;
    if (radius > T - 1) radius = T - 1;
    const long long nseq = (long long)nclips * HW * heads;
    return temporal_stream_dispatch<1>(head_dim, [&](auto g) {
        using G = decltype(g);
        return launch_temporal_long<G, attn_temporal_stream_kernel<G::D, G::WPB>>(
            nseq, (hipStream_t)stream, (const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, nseq, T, HW, heads, ld, ldkv, ldo, scale,
            radius, anchor);
    });
}

// the streaming walk for a frame shard (attn_temporal_stream_shard_kernel): Tq >= 1 query frames against 1 <= S <= 1024 key slots.
//   radius >= 0   window mode: the contract and the refusals of mofa_attn_temporal_long_window_f16 with 1024 slots for 128;
//                 key_mask must be NULL.  radius is clamped to S - 1 (two band frames lie no further apart), so that no frame
//                 sum overflows
//   radius == -1  dense mode: anchor, q_frame0 and band_frame0 must be 0; key_mask is host memory of ceil(S / 32) words, bit
//                 j % 32 of word j / 32 = slot j exists, NULL = every slot; bits at and above S are ignored; an empty mask is
//                 refused.  The kernel gets the window that hides nothing (radius 2^30; Tq above 2^30 is refused for it)
// The words travel as kernel arguments in both modes (window: every slot below S): no device allocation, no copy.
extern "C" int mofa_attn_temporal_stream_shard_f16(const void* q, const void* k, const void* v, void* out, int nclips, int Tq,
                                                   int S, int HW, int heads, int head_dim, int ld, int ldkv, int ldo, float scale,
                                                   int radius, int anchor, int q_frame0, int band_frame0,
                                                   const uint32_t* key_mask, mofa_stream_t stream) {
    if (!temporal_long_args_ok(q, k, v, out, nclips, S, HW, heads, head_dim, ld, ldkv, ldo, 1024)) return MOFA_EINVAL;
    if (Tq < 1 || Tq > (1 << 30) || radius < -1) return MOFA_EINVAL;
    if (radius >= 0) {
        if (key_mask) return MOFA_EINVAL;
        if (anchor < 0 || anchor > S || band_frame0 < 0 || band_frame0 > (1 << 30)) return MOFA_EINVAL;
        if (q_frame0 < band_frame0 || (long long)q_frame0 + Tq > (long long)band_frame0 + (S - anchor)) return MOFA_EINVAL;
        if (radius > S - 1) radius = S - 1;
    } else {
        if (anchor != 0 || q_frame0 != 0 || band_frame0 != 0) return MOFA_EINVAL;
        radius = 1 << 30;
    }
    TemporalShardWords words;
    uint32_t any = 0;
    for (int w = 0; w < 32; ++w) any |= words.w[w] = temporal_mask_word(key_mask, w, S);
    if (any == 0) return MOFA_EINVAL;
    const long long nseq = (long long)nclips * HW * heads;
    return temporal_stream_dispatch<1>(head_dim, [&](auto g) {
        using G = decltype(g);
        return launch_temporal_long<G, attn_temporal_stream_shard_kernel<G::D, G::WPB>>(
            nseq, (hipStream_t)stream, (const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, nseq, Tq, S, HW, heads, ld, ldkv, ldo,
            scale, radius, anchor, q_frame0, band_frame0, words);
    });
}

// ---------------------------------------------------------------------------------------------------
// In-place row softmax(VAE mid-block attention: 1 head x 512, scores materialised per frame)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_rows_kernel(f16* __restrict__ x, int cols, int ld) {
    __shared__ float red[8];
    f16* row = x + (size_t)blockIdx.x * ld;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mx = -1e30f;
    for (int c = tid * 8; c < cols; c += 256 * 8) {
        const f16x8 a = *(const f16x8*)(row + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) mx = fmaxf(mx, (float)a[e]);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int c = tid * 8; c < cols; c += 256 * 8) {
        const f16x8 a = *(const f16x8*)(row + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += __expf((float)a[e] - mx);
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.0f / (red[4] + red[5] + red[6] + red[7]);
    for (int c = tid * 8; c < cols; c += 256 * 8) {
        f16x8 a = *(const f16x8*)(row + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (f16)(__expf((float)a[e] - mx) * inv);
        *(f16x8*)(row + c) = a;
    }
}

extern "C" int mofa_softmax_rows_f16(void* x, int rows, int cols, int ld, mofa_stream_t stream) {
    if (!x || rows <= 0 || cols <= 0 || cols % 8 != 0 || ld % 8 != 0 || ld < cols) return MOFA_EINVAL;
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, (f16*)x, cols, ld);
    MOFA_CHECK_LAUNCH();
    return MOFA_OK;
}
