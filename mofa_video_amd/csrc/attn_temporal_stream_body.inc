// The body of the two streaming walks of attention.hip (attn_temporal_stream_kernel over whole clips, attn_temporal_stream_shard_kernel
// over a frame shard's key slots), included inside each kernel's braces behind the kernel's own declarations.  In scope: template
// <int D, int WPB>, the kernel arguments q, out, HW, ld, ldo, scale, anchor; what TEMPORAL_WAVE_DECODE declares (lane, l31, lh,
// head, the wave's slot wK / wV); Tq, the query rows of a clip; qbase, the q / out token row of the clip's first query frame;
// TEMPORAL_LOAD_Q, TEMPORAL_STORE_O, TL_SLOT; and the kernel's seven walk macros, which this file undefines at its end:
//   TS_FIRST(t0)     the load of tile t0 (a TemporalStreamTile), the first tile of the first block
//   TS_BLOCK(q0)     per query block, the declarations of this lane's band [lo, hi1) in key rows and of the block's walk (wave-uniform)
//   TS_START         the declaration of kt, the block's first tile, and of what else the walk carries from tile to tile
//   TS_NEXT(nt)      per tile, the declarations of `more` (the block's walk goes on), of nk, its next tile, of tile nt and its load:
//                    tile nk, after a block's last tile the next block's first, after the last tile of all nothing; and of
//                    below(n), the n lowest bits with n clamped to 0 .. 32, unless the kernel has declared it before
//   TS_AND_WORD(kt)  `& w`, w = the key rows of tile kt that exist (bit i = row 32 kt + i), or nothing: all exist
//   TS_ADVANCE       the step to tile nk
//   TS_STORE(t)      tile t into the slot
// Seven, not the long body's five, and in this order of appearance, because the measure is the compiler's output: with kt declared
// in TS_BLOCK, below declared here, or the tiles stored by one shared call, a kernel is no longer the instructions of its former
// copy (DESIGN.md section 3).
// Everything else is shared.  One wave owns one sequence and ONE 32-row tile slot of K and V in LDS (the KT = 1 geometry: four
// waves a workgroup at D = 64, two at D = 128).  Per 32-query block it visits the tiles of the kernel's walk, in ascending order
// and each once, and never reads the others.  Across the tiles it keeps, per query, a running maximum m, this lane half's part l
// of the running sum (the halves meet once, after the last tile) and the fp32 O^T accumulators; per tile
//   m' = max(m, tile maximum over the VISIBLE keys)     a = exp2((m - m') c2)     l = a l + sum p     O^T = a O^T + V^T P^T
// with p = exp2((s - m') c2) rounded to fp16 for P V, as in the long kernel, and one multiplication by 1 / l at the end.  A key is
// visible iff it lies below the anchor or in [lo, hi1), and exists.  Two hazards, each met by a select:
//   a is SET to 1 where m' = m: mc - m' c2 may be contracted into one fma, which returns the product's rounding error instead
//   of 0 -- about 1e21 in size at m = -1e30, exp2 of which is 0 or infinity.  O^T is rescaled only where some lane's maximum
//   moved (the skip changes no bit).
//   A hidden key's probability is SET to 0, not left to exp2: a visited tile can hide every key of a row whose maximum is still
//   the initial -1e30 (anchor = 0: the block's first band tile lies wholly below the band of its last queries whenever
//   radius % 32 != 0; a tile whose visible rows are all dead slots), and there exp2((s - m') c2) is exp2(+huge) = infinity
//   (exp2(0) = 1 had the score been replaced by -1e30 first), which the rescale by a = 0 at the row's first visible key turns
//   into NaN.  With the select such a tile leaves m, l and O^T as they were.
// Every row meets a visible key in some visited tile (the kernels' rules see to it), so l > 0 at the end.  The arithmetic of a
// query depends on its visible keys and their ascending order alone, which is what the kernels' equal-bits promises rest on.
// The next tile travels to registers under the current tile's arithmetic and enters the slot behind the tile's last LDS read
// (s_waitcnt + wave barrier on both sides, as in the ring kernel).  A row that is not loaded is written as zero, so every row an
// MFMA reads is finite if the loaded ones are: a hidden row of a visited tile is read and multiplied by its zero.  Query rows
// >= Tq are neither loaded nor stored.  K and V of a sequence are read once per query block that sees them (from L2 after the
// first).
    constexpr int KK = D / 16, DB = D / 32, KSTR = D + 8, VSTR = D + 32;

    f16x8 qf[KK];
    TEMPORAL_LOAD_Q(qf, l31, qbase, Tq)
    {
        TemporalStreamTile<D> t0;
        TS_FIRST(t0)
        TS_STORE(t0)
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // this wave's LDS writes are in place
    __builtin_amdgcn_wave_barrier();

    const float c2 = scale * 1.4426950408889634f;
    const int tr_off = (((lane & 15) >> 2) + 4 * lh) * VSTR + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
#pragma unroll 1
    for (int q0 = 0; q0 < Tq; q0 += 32) {
        // the next block's Q fragments are fetched under this block's arithmetic
        f16x8 qn[KK];
        TEMPORAL_LOAD_Q(qn, q0 + 32 + l31, qbase, Tq)
        TS_BLOCK(q0)

        float m = -1e30f, mc = m * c2, l = 0.f;
        f32x16 o[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] = 0.f;

        TS_START
#pragma unroll 1
        for (;;) {
            TS_NEXT(nt)

            const unsigned ml =
                ((below(anchor - 32 * kt) | (below(hi1 - 32 * kt) & ~below(lo - 32 * kt))) TS_AND_WORD(kt)) >> (4 * lh);
            // ---- S^T tile: s[r] = score(key = 32 kt + (r & 3) + 8 (r >> 2) + 4 lh, query = q0 + l31) ----
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
            float mx = m;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (ml & (1u << TL_SLOT(r))) mx = fmaxf(mx, s[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mcn = mx * c2;
            const bool moved = mx != m;
            const float a = moved ? __builtin_amdgcn_exp2f(mc - mcn) : 1.0f;   // m = -1e30 < mx: exp2(-huge) = 0
            m = mx; mc = mcn;
            float sum = 0.f;
            f16x8 pf[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -mc));
                const float pr = (ml & (1u << TL_SLOT(r))) ? e : 0.f;      // hidden: exactly 0 whatever m is
                sum += pr;
                pf[r >> 3][r & 7] = (f16)pr;
            }
            l = fmaf(l, a, sum);
            if (__any(moved)) {
#pragma unroll
                for (int db = 0; db < DB; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[db][r] *= a;
            }
            // ---- O^T[d][q] += V^T[d][key] P^T[key][q], k-slots as in the long body file ----
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const f16* vp = wV + tr_off + db * 32;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const f16x4 vl = lds_read_tr4(vp + (u * 16) * VSTR), vh = lds_read_tr4(vp + (u * 16 + 8) * VSTR);
                    const f16x8 vf = {vl[0], vl[1], vl[2], vl[3], vh[0], vh[1], vh[2], vh[3]};
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[u], o[db], 0, 0, 0);
                }
            }
            // ---- the next tile into the slot, after this tile's last LDS read ----
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            TS_STORE(nt)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            if (!more) break;
            TS_ADVANCE
        }
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;
        TEMPORAL_STORE_O(o, inv, q0 + l31, qbase, Tq)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) qf[kk] = qn[kk];
    }
#undef TS_FIRST
#undef TS_BLOCK
#undef TS_START
#undef TS_NEXT
#undef TS_AND_WORD
#undef TS_STORE
#undef TS_ADVANCE
