// The body of the three long temporal attention kernels of attention.hip (attn_temporal_long_kernel, ..._masked_kernel,
// ..._local_kernel), included inside each kernel's braces.  In scope: template <int D, int KT, int WPB>, the kernel arguments
// q, k, v, out, nseq, T, HW, heads, ld, ldkv, ldo, scale (and the form's own), TL_SLOT, and the form's five rule macros, which this
// file undefines at its end:
//   TL_TQ              the query rows of a clip (rows of q / out, clip stride Tq*HW; k / v rows have clip stride T*HW)
//   TL_STAGE_WORD(t0)  a declaration the staging predicate of iteration t0 needs, or nothing
//   TL_STAGED(t)       whether key row t is LOADED while staging (a row that is not loaded is written to LDS as zero)
//   TL_WORDS(q0)       per query block, the declaration of its KT words ml[kt] (bit (r & 3) + 8 (r >> 2) = the key of score
//                      s[kt][r] is seen by this lane's query), where the form works with words, or nothing
//   TL_HIDDEN(kt, r)   the per-score test
// Everything else is shared: the fragment algebra of attn_temporal_kernel repeated over KT = ceil(T / 32) key tiles and
// ceil(Tq / 32) query blocks, one wave per sequence.  The wave stages ALL 32 KT key rows of K and V in its own LDS region once (K
// and V leave HBM once per sequence), then runs one query block after the other: the KT score tiles of a block stay in registers
// (<= 64 fp32), so the maximum, exp2 and the sum are taken across the tiles directly -- no online-softmax rescale -- and O^T
// accumulates over the tiles.  A hidden key's score is -1e30 before the row maximum, so its probability is exactly 0; everything
// after that test is the same arithmetic in the same order for every form, which is why a rule that hides nothing gives the
// dense kernel's bits.  Query rows >= Tq are never loaded or stored.  No key tile is skipped, whatever the rule hides:
// wave-uniform branches round the dead tiles of a query block cut the block's straight-line code, in which MFMAs and softmax
// arithmetic overlap, into pieces, and ran 1.25-1.46 x the dense time at KT >= 3 (DESIGN.md section 3).
// LDS per wave: 32 KT (2 D + 40) halves = 10.5 KT KB (D = 64) / 18.5 KT KB (D = 128); dynamic, the D = 128, KT = 4 instantiation
// (74 KB) needs the opt-in beyond 64 KB.
    constexpr int DC = D / 8;       // 16-byte chunks per row
    constexpr int KK = D / 16;      // MFMA k-steps of S^T
    constexpr int DB = D / 32;      // 32-wide output d-blocks
    constexpr int KSTR = D + 8;     // K row stride in halves (conflict-free ds_read_b128)
    constexpr int VSTR = D + 32;    // V row stride in halves (see lds_read_tr4)
    constexpr int ROWS = 32 * KT;   // staged key rows
    constexpr int RPI = 64 / DC;    // key rows one wave-wide pass of 16-byte chunks covers (8 / 4)
    constexpr int UB = 4;           // passes in flight: 2 UB 16-byte loads per lane before the first LDS store
    extern __shared__ __attribute__((aligned(16))) char smem_tl[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long seq = (long long)blockIdx.x * WPB + wave;
    if (seq >= nseq) return;                                       // (no workgroup barrier below: LDS regions are per wave)
    const int l31 = lane & 31, lh = lane >> 5;
    const int head = (int)(seq % heads);
    const long long bp = seq / heads;
    const int p = (int)(bp % HW);
    const int b = (int)(bp / HW);
    const size_t base = ((size_t)b * T * HW + p);                  // k / v token row of frame 0
    const size_t qbase = ((size_t)b * TL_TQ * HW + p);                // q / out token row of frame 0
    f16* wK = (f16*)smem_tl + (size_t)wave * (ROWS * (KSTR + VSTR));
    f16* wV = wK + ROWS * KSTR;
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // Q fragments of query block 0 (B operand of S^T): lane (query l31, half lh) holds Q[q][16 kk + 8 lh .. + 8)
    f16x8 qf[KK];
    {
        const f16* qp = q + (qbase + (size_t)(l31 < TL_TQ ? l31 : 0) * HW) * ld + head * D + lh * 8;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) qf[kk] = l31 < TL_TQ ? *(const f16x8*)(qp + kk * 16) : zero8;
    }
    // ---- K and V rows the form stages, UB passes at a time; every other row (>= T, a dead slot) is written as zero and never
    //      read from memory (its probability is exactly 0, but 0 * NaN from never-written LDS would not be) ----
    {
        const int r0 = lane / DC, cc = lane % DC;
#pragma unroll 1
        for (int t0 = 0; t0 < ROWS; t0 += UB * RPI) {
            TL_STAGE_WORD(t0)                                      // (wave-uniform)
            f16x8 gk[UB], gv[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int t = t0 + u * RPI + r0;
                gk[u] = zero8; gv[u] = zero8;
                if (TL_STAGED(t)) {
                    const size_t off = (base + (size_t)t * HW) * ldkv + head * D + cc * 8;
                    gk[u] = *(const f16x8*)(k + off);
                    gv[u] = *(const f16x8*)(v + off);
                }
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int t = t0 + u * RPI + r0;
                *(f16x8*)&wK[t * KSTR + cc * 8] = gk[u];
                *(f16x8*)&wV[t * VSTR + cc * 8] = gv[u];
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // this wave's LDS writes are in place
    __builtin_amdgcn_wave_barrier();

    const float c2 = scale * 1.4426950408889634f;
    const int tr_off = (((lane & 15) >> 2) + 4 * lh) * VSTR + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
#pragma unroll 1
    for (int q0 = 0; q0 < TL_TQ; q0 += 32) {
        // the next block's Q fragments are fetched under this block's arithmetic
        f16x8 qn[KK];
        {
            const int qi = q0 + 32 + l31;
            const f16* qp = q + (qbase + (size_t)(qi < TL_TQ ? qi : 0) * HW) * ld + head * D + lh * 8;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) qn[kk] = qi < TL_TQ ? *(const f16x8*)(qp + kk * 16) : zero8;
        }
        TL_WORDS(q0)
        // ---- S^T tiles: s[kt][r] = score(key = 32 kt + (r & 3) + 8 (r >> 2) + 4 lh, query = q0 + l31) ----
        f32x16 s[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
            const f16* kp = wK + (kt * 32 + l31) * KSTR + lh * 8;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const f16x8 kf = *(const f16x8*)(kp + kk * 16);
                s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[kk], s[kt], 0, 0, 0);
            }
        }
        float mx = -1e30f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (TL_HIDDEN(kt, r)) s[kt][r] = -1e30f;
                mx = fmaxf(mx, s[kt][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mc = mx * c2;
        float sum = 0.f;
        f16x8 pf[KT][2];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pr = __builtin_amdgcn_exp2f(fmaf(s[kt][r], c2, -mc));   // hidden keys: exp2(-huge) = 0
                sum += pr;
                pf[kt][r >> 3][r & 7] = (f16)pr;
            }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;

        // ---- O^T[d][q] += V^T[d][key] P^T[key][q]; k-slot (8 lh + jj) of MFMA (kt, u) = key
        //      32 kt + 16 u + 4 lh + (jj & 3) + 8 (jj >> 2), identical for both operands ----
        f32x16 o[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
            const f16* vp = wV + tr_off + db * 32;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const f16x4 lo = lds_read_tr4(vp + (kt * 32 + u * 16) * VSTR), hi = lds_read_tr4(vp + (kt * 32 + u * 16 + 8) * VSTR);
                    const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[kt][u], o[db], 0, 0, 0);
                }
        }
        if (q0 + l31 < TL_TQ) {
            f16* op = out + (qbase + (size_t)(q0 + l31) * HW) * ldo + head * D;
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
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) qf[kk] = qn[kk];
    }
#undef TL_TQ
#undef TL_STAGE_WORD
#undef TL_STAGED
#undef TL_WORDS
#undef TL_HIDDEN
