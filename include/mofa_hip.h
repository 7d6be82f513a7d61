/*
 * mofa_hip.h -- C ABI of libmofa_hip.so, the MI355X (gfx950) kernels behind the
 * MOFA-Video denoising hot path.
 *
 * The reference (MyNiuuu/MOFA-Video) has no C/FFI boundary of its own: its only native
 * code is three CUDA kernels held as Python strings and JIT-launched through CuPy with raw
 * device pointers + the torch stream (MOFA-Video-Traj/models/softsplat.py:219-226,
 * :341-345); everything else dispatches through torch/diffusers.  This header is the
 * boundary a maintainer binds instead -- same calling discipline as that CuPy launch:
 * plain device pointers, sizes, and the caller's stream.  No torch types, no allocation
 * inside the library, no global state.  Every entry point returns 0 on success or a
 * negative MOFA_E* code; kernels are enqueued on `stream` and nothing synchronises.
 *
 * Layout convention: activations are fp16 "token-major" (NHWC): a tensor
 * [frames, H, W, C] is a row-major matrix of frames*H*W rows by C channels, row stride
 * `ld*` in elements.  Weights are fp16 [N][K] with K contiguous (conv: K = taps*Cin,
 * tap-major).  Small per-channel vectors (bias, norm affine, row vectors) are fp32.
 *
 * Each entry point cites the reference interface it replaces (file:line under
 * /root/reference/MOFA-Video-Traj unless noted; "diffusers" = diffusers==0.24.0, the
 * reference's pinned third-party dependency that holds the block arithmetic).
 */
#ifndef MOFA_HIP_H
#define MOFA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mofa_stream_t; /* hipStream_t */

#define MOFA_OK 0
#define MOFA_EINVAL (-22)
#define MOFA_ELAUNCH (-5)

/* library version / build probe */
int mofa_version(void);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM on MFMA (v_mfma_f32_32x32x16_f16, fp32 accumulate).
 *   out[m, n] = act( s_acc * (sum_{tap,k} X[src(m,tap), k] * W[n, tap*Cin + k] + bias[n] + rowvec[idx(m), n])
 *                    + s1 * R1[m, n] + s2 * R2[m, n] )
 * Rounding: fp32 accumulate; WITH a residual (R1 or R2) the term s_acc * (...) is rounded to fp16 before the residuals are added
 * in fp32 and the sum is rounded once more -- the reference's fp16 modules produce the layer's output in fp16 and then add --;
 * without residuals there is one rounding.  Every tile kernel rounds this way, so the tile choice never changes the bits of an
 * exactly representable sum (tests/test_igemm_tiles_gpu.py::test_all_tiles_round_residual_adds_alike).
 * Geometry limits of MOFA_MODE_CONV3X3 (rows are packed into registers; beyond a limit the launcher returns MOFA_EINVAL for a
 * forced tile and never truncates): the 4-wave tiles (128x128, 192x128) take Hout, Wout <= 65535 -- (oy << 16) | ox as an
 * unsigned word -- and any image count; the 8-wave tiles (256x256, 256x320) take Hout, Wout <= 1024 and at most 2047 images
 * -- img << 20 | oy << 10 | ox -- and need input rows * ldx * 2 bytes below 4 GB - 64 KB (32-bit buffer offsets).  With
 * MOFA_TILE_AUTO a call beyond the 8-wave limits runs on a 4-wave tile; Hout or Wout > 65535 is MOFA_EINVAL for every tile.
 * tests/test_igemm_conv_edges_gpu.py runs the last value of every field, and the first refused one, on every tile.
 * Replaces every nn.Linear / nn.Conv2d(1x1, 3x3 s1/s2, nearest-2x + 3x3) / nn.Conv3d((3,1,1))
 * the reference reaches through diffusers blocks (ResnetBlock2D, TemporalResnetBlock,
 * Downsample2D, Upsample2D, Attention.to_q/k/v/out, FeedForward; built at
 * models/unet_spatio_temporal_condition_controlnet.py:169-232, models/controlnet_sdv.py:259-309)
 * and the adapter's own convs (models/svdxt_featureflow_forward_controlnet_s2d_fixcmp_norefine.py:66-155).
 * ---------------------------------------------------------------------------------------- */
enum { MOFA_MODE_PLAIN = 0, MOFA_MODE_CONV3X3 = 1, MOFA_MODE_CONVT3 = 2,       /* CONV3X3 = k x k conv, k = ksize (1, 3, 5 or 7) */
       MOFA_MODE_CONV3X3_UP2F = 3 };
/* MOFA_MODE_CONV3X3_UP2F: the 3x3 convolution over a nearest-2x up-sampled image (CONV3X3 with up = 2: diffusers Upsample2D) with
 * the up-sampling FOLDED into the weights.  Two of the three taps of an output pixel along an axis always read the same source
 * pixel, so output (2y + a, 2x + b) depends only on source pixels {y - 1 + a, y + a} x {x - 1 + b, x + b}: four 2x2
 * convolutions, one per output parity (a, b), on the low-resolution input -- 4 taps instead of 9, 4/9 of the MACs.
 *   Hin, Win   the low-resolution image; Hout = 2 Hin, Wout = 2 Win; M = nimg * Hout * Wout output rows in the ordinary
 *              (img, oy, ox) order at out + row * ldo; stride = 1, up = 2, ksize 0 or 3, dil 0 or 1, MOFA_PAD_SAME
 *   w          fp16 [4][N][4 * Cin]: phase p = 2 a + b major, then output channel, then tap t = 2 ty + tx, then Cin; tap (ty, tx)
 *              of phase (a, b) reads source pixel (y - 1 + a + ty, x - 1 + b + tx), zero outside the image -- exactly the taps
 *              the classic form pads.  Each folded weight is the fp32 sum of the 1, 2 or 4 coinciding fp16 taps, rounded once
 *              (mofa_video_amd/weights.py: fold_up2).
 *   limits     the plain epilogue only (bias; no activation, row vector, residual or stats), the two 8-wave tiles only (a forced
 *              4-wave tile is MOFA_EINVAL), Hin, Win <= 1024, at most 2047 images, and the 8-wave tiles' alignment rules: every
 *              other combination is MOFA_EINVAL.
 * Inside the kernels a 256-row tile belongs to ONE phase (it multiplies all its rows by one weight tile): the Mq = nimg * Hin * Win
 * rows of a phase are padded to whole tiles, tiles_m = 4 * ceil(Mq / 256), row tile t holds rows 256 (t / 4) .. + 255 of phase
 * t % 4 (the four passes over one input region are neighbours in the tile walk), and the epilogue scatters row (img, y, x) of
 * phase (a, b) to output row (img * Hout + 2 y + a) * Wout + 2 x + b: mofa_igemm_up2f_row. */
/* MOFA_ACT_GEGLU_PAIR: W holds the GEGLU projection with value and gate rows INTERLEAVED IN BLOCKS OF 16 (rows 32 b .. 32 b + 15 =
 * value rows of outputs 16 b .. 16 b + 15, rows 32 b + 16 .. 32 b + 31 = their gate rows; bias alike): out[m][16 b + c] =
 * s_acc * val * gelu(s_acc * gate), N / 2 output columns (diffusers GEGLU, erf GELU).  mofa_video_amd/weights.py packs it. */
enum { MOFA_ACT_NONE = 0, MOFA_ACT_SILU = 1, MOFA_ACT_GEGLU_PAIR = 2, MOFA_ACT_RELU = 3,
       MOFA_ACT_GELU = 4 /* exact (erf) GELU: CLIP vision MLP, transformers CLIPMLP with hidden_act = "gelu" */ };

typedef struct mofa_igemm_args {
    const void* x;      /* fp16 activations                                                  */
    const void* w;      /* fp16 weights [N][taps*Cin]                                        */
    const float* bias;  /* fp32 [N] or NULL                                                  */
    const float* rowvec;/* fp32 [nvec][N] or NULL; idx(m) = ((m / rv_div) * rv_mul + (m % rv_mod_in)) % rv_mod_out */
    const void* r1;     /* fp16 residual [M][ldr1] or NULL                                   */
    const void* r2;     /* fp16 residual [M][ldr2] or NULL                                   */
    void* out;          /* fp16 [M][ldo]  (N columns; N/2 for MOFA_ACT_GEGLU_PAIR)           */
    int32_t M, N, Cin;  /* Cin % 64 == 0, N % 4 == 0                                         */
    int32_t ldx, ldo, ldr1, ldr2;
    int32_t mode;       /* MOFA_MODE_*                                                       */
    /* MOFA_MODE_CONV3X3: rows are (img, oy, ox); k x k taps (ksize 1, 3, 5 or 7; 0 means 3), dilation dil,  */
    /* pad dil*(k/2); stride 1|2; up = 1|2 (nearest-neighbour upsampling of the input before the conv)      */
    int32_t Hin, Win, Hout, Wout, stride, up, ksize;
    /* MOFA_MODE_CONVT3: rows are (frame, pixel); frames grouped in clips of T; T = 0: no     */
    /* clipping at clip ends (the caller placed halo frames before/after the rows)           */
    int32_t T, HW;
    int32_t rv_div, rv_mul, rv_mod_in, rv_mod_out;
    int32_t act;        /* MOFA_ACT_*                                                        */
    float s_acc, s1, s2;
    int32_t dil;        /* MOFA_MODE_CONV3X3: tap dilation (0 means 1); the CMP encoder's de-strided ResNet stages use 2 and 4
                         * (Traj/models/cmp/models/backbone/resnet.py:118-129) */
    int32_t pad;        /* MOFA_MODE_CONV3X3: MOFA_PAD_SAME (0) = dil*(k/2) on every side; MOFA_PAD_TRAILING (1) = no
                         * leading padding, taps start at input pixel stride*o (diffusers Downsample2D(padding=0) of the
                         * VAE encoder: F.pad(x, (0,1,0,1)) then a stride-2 conv)                                    */
    int32_t tile;       /* MOFA_TILE_AUTO (0): the launcher's cost model picks the output tile; any other MOFA_TILE_*
                         * forces it (parity tests run every shape through every tile) */
    void* workspace;    /* optional device scratch (16-byte aligned) owned by the caller, private to `stream` for the duration
                         * of the launch, or NULL.  With it the 256x320 tile splits the tiles of a partial last round of
                         * workgroups along K (fp32 partial tiles here, added in a fixed order by a fix-up launch on the same
                         * stream); without it every tile is computed whole.  Same result up to fp32 summation order.          */
    int64_t workspace_bytes;   /* 84 MB (256 partial tiles of 256 x 320 fp32) is never exceeded.                              */
    float* stats;       /* optional fp32 [M / 64][N]: for every block of 64 output rows and every PAIR of output columns (2 p, 2 p + 1)
                         * the sum (element 2 p) and the sum of squares (element 2 p + 1) of the fp16 outputs just written -- the
                         * GroupNorm partial sums of the layer that follows (diffusers ResnetBlock2D / TemporalResnetBlock: conv ->
                         * GroupNorm, models/controlnet_sdv.py:270-309), emitted by the producing epilogue so that the consumer does
                         * not read the activations a third time (mofa_gn_partial_from_stats turns them into `part` entries).
                         * Only where mofa_igemm_stats_ok() says so (256x320 tile; M % 64 == 0, N % 320 == 0, no activation, at most
                         * one residual, a row vector that is constant over 64-row blocks); MOFA_EINVAL otherwise.
                         * sizeof(mofa_igemm_args) = 192 */
} mofa_igemm_args;
enum { MOFA_PAD_SAME = 0, MOFA_PAD_TRAILING = 1 };
/* output tiles of the implicit GEMM: 4 waves / 2 workgroups per CU (128x128, 192x128) and the 8-wave phase-pipelined
 * 256x256 tile (needs 16-byte aligned rows and no activation on residual kinds: MOFA_EINVAL if forced on an ineligible
 * call) */
enum { MOFA_TILE_AUTO = 0, MOFA_TILE_128X128 = 2, MOFA_TILE_192X128 = 4, MOFA_TILE_256X256 = 5, MOFA_TILE_256X320 = 6 };

int mofa_igemm_f16(const mofa_igemm_args* a, mofa_stream_t stream);
/* 1 when a launch with these arguments can emit `stats` (the value of a->stats itself is ignored), else 0 */
int mofa_igemm_stats_ok(const mofa_igemm_args* a);
/* What mofa_igemm_f16 would launch for `a` on a device of n_cu compute units, decided on the host alone (no device call; the
 * pointers are looked at for NULL and alignment only).  All fields but rc are 0 when rc != MOFA_OK. */
typedef struct mofa_igemm_plan_t {
    int32_t rc;                        /* MOFA_OK, or the MOFA_EINVAL mofa_igemm_f16 returns without launching */
    int32_t tile, kind;                /* the MOFA_TILE_* that runs; epilogue kind: bit 0 r1, bit 1 r2, bit 2 rowvec, 8 = GEGLU pair */
    int32_t tiles_m, tiles_n, grid, threads, lds_bytes;
    int32_t split;                     /* K slices of each remainder tile (1 = none) */
    int32_t full_tiles, rem_tiles;     /* tiles computed whole / cut into `split` slices (split == 1: all tiles, 0) */
    int32_t stats;                     /* the epilogue emits GroupNorm pair sums */
    int32_t launches;                  /* 1, + 1 split-K fix-up, + 1 pair sums of the remainder tiles */
    int32_t reserved[4];
} mofa_igemm_plan_t;
/* MOFA_EINVAL for a NULL a or out, or n_cu <= 0; else MOFA_OK with the launch's own verdict in out->rc */
int mofa_igemm_plan(const mofa_igemm_args* a, int n_cu, mofa_igemm_plan_t* out);
/* MOFA_MODE_CONV3X3_UP2F: the output row that row `tile_row` (0 <= tile_row < 256 * tiles_m) of the kernels' phase-padded row
 * tiles is stored to, or -1 for a padding row; MOFA_EINVAL for a tile_row out of range, another mode or arguments mofa_igemm_f16
 * refuses.  Host only. */
int64_t mofa_igemm_up2f_row(const mofa_igemm_args* a, int64_t tile_row);

/* ------------------------------------------------------------------------------------------
 * Attention.  q/k/v are column blocks of token-major matrices: element (token, head, d) at
 * base[token*ld + head*head_dim + d].  Replaces diffusers AttnProcessor2_0 / F.scaled_dot_product_attention
 * inside BasicTransformerBlock.attn1 (spatial) and TemporalBasicTransformerBlock.attn1 (temporal), and the
 * softmax(QK^T)V of transformers CLIPAttention (head dim 80 in 128-column slots, mofa_video_amd/clip.py).
 * ---------------------------------------------------------------------------------------- */
/* spatial self-attention, head_dim 64 or 128: batch = nframes, sequence = S tokens per frame.
 * (The MOFA ControlNet trunk is built with heads (5,10,10,20) -- FlowControlNet calls super().__init__()
 *  without arguments, svdxt_..._norefine.py:213 -> controlnet_sdv.py:180 -- so its 1280-channel level runs
 *  10 heads x 128; the SVD-XT UNet runs 64 everywhere.)
 * v is read as it is, row-major [tokens][ldv] like q and k (the transposed fragments of the PV product come from the LDS
 * transpose read of gfx950; no pre-transposed copy of V).
 * scale > 0: softmax(scale * Q K^T) V.  scale <= 0: q already holds Q * head_dim^-0.5 * log2(e) -- the caller folded
 * that constant into its Q projection weights (blocks.SelfAttn(fold_q_scale=True)), so the kernel neither multiplies nor
 * re-rounds Q; with scale > 0 Q is multiplied by scale * log2(e) and rounded to fp16 once more inside the kernel. */
int mofa_attn_spatial_f16(const void* q, const void* k, const void* v, void* out,
                          int nframes, int heads, int head_dim, int S, int ldq, int ldk, int ldv, int ldo, float scale,
                          mofa_stream_t stream);
/* the same with the number of 32-query blocks per wave chosen by the caller: 0 = the launcher's rule (as above), 1 = 128-row
 * workgroups, 2 = 256-row workgroups (head_dim 64 only).  Same result up to fp32 summation order; the parity tests drive
 * both kernels over the bench's shapes with it. */
int mofa_attn_spatial_qb_f16(const void* q, const void* k, const void* v, void* out,
                             int nframes, int heads, int head_dim, int S, int ldq, int ldk, int ldv, int ldo, float scale,
                             int query_blocks, mofa_stream_t stream);
/* [tokens][ld] columns in blocks of 64 (ncb = C/64 blocks) -> vt[((frame*ncb + cb)*64 + d)*S + key] = [frame][C][S]: the
 * weight operand of the VAE mid-block attention's second implicit GEMM (vae.py); the attention kernels do not need it.
 * S % 8 == 0 (any S: the last block of 64 keys may be ragged), ldv % 8 == 0, ldv >= ncb * 64; ncb and nframes are grid
 * dimensions, at most 65535 each.  MOFA_EINVAL otherwise, before any device call. */
int mofa_transpose_v_f16(const void* v, void* vt, int nframes, int ncb, int S, int ldv, mofa_stream_t stream);
/* temporal self-attention over T frames per (clip, pixel, head), head_dim 64 or 128, T <= 32.
 * k/v: token row of (clip b, frame t, pixel p) = (b*T + t)*HW + p, leading dim ldkv.
 * q/out: Tq <= T query frames, row (b*Tq + i)*HW + p (Tq < T when a clip's frames are sharded over ranks and the
 * keys/values were all-gathered; Tq == T otherwise). */
int mofa_attn_temporal_f16(const void* q, const void* k, const void* v, void* out,
                           int nclips, int Tq, int T, int HW, int heads, int head_dim, int ld, int ldkv, int ldo,
                           float scale, mofa_stream_t stream);
/* the same with a key-frame validity mask (bit j = key frame j exists).  Frame-sharded clips all-gather K|V into ONE
 * buffer of ranks x (largest shard) frames; with uneven shards (25 frames over 4 ranks = 7/6/6/6) the padding frames of
 * the shorter shards are masked here instead of being compacted away by a copy (rows of masked frames are never read). */
int mofa_attn_temporal_masked_f16(const void* q, const void* k, const void* v, void* out,
                                  int nclips, int Tq, int T, int HW, int heads, int head_dim, int ld, int ldkv, int ldo,
                                  float scale, uint32_t key_mask, mofa_stream_t stream);
/* temporal self-attention over 1 <= T <= 128 frames per (clip, pixel, head), head_dim 64 or 128: the entry point for clips
 * of more than 32 frames (it accepts shorter ones too, and then agrees with mofa_attn_temporal_f16 up to fp32 summation
 * order).  Row layout of mofa_attn_temporal_f16 with Tq == T: q / k / v / out token row of (clip b, frame t, pixel p) =
 * (b*T + t)*HW + p, leading dims ld (q), ldkv (k and v), ldo (out), all multiples of 8.  No key mask and no Tq < T:
 * frame-sharded clips take the 32-key entry points above or mofa_attn_temporal_long_masked_f16 below.  One wave per sequence keeps ceil(T/32) key tiles of K and
 * V in LDS (read from memory once) and the score tiles of one 32-query block in registers; rows of frames >= T are never
 * read or written.  MOFA_EINVAL for NULL pointers, T < 1 or T > 128, another head_dim, a leading dimension that is not a
 * positive multiple of 8, or a non-positive count -- all checked before any device call. */
int mofa_attn_temporal_long_f16(const void* q, const void* k, const void* v, void* out,
                                int nclips, int T, int HW, int heads, int head_dim, int ld, int ldkv, int ldo,
                                float scale, mofa_stream_t stream);
/* The long temporal attention of a frame-sharded clip: Tq query frames (rows of q / out, clip stride Tq*HW) against
 * 1 <= Tq <= T <= 128 key slots of the gathered K|V buffer (rows of k / v, clip stride T*HW).  key_mask: HOST memory, four
 * 32-bit words read during the call, bit j % 32 of word j / 32 = key slot j exists; NULL = every slot below T; bits at or
 * above T are ignored.  The words travel as kernel arguments (no device buffer, no extra launch).  A slot whose bit is clear
 * is never read, neither K nor V (padding slots of uneven shards may hold NaN), and has weight exactly 0; query rows >= Tq
 * are neither read nor written.  Every slot live and Tq == T: bit-identical with mofa_attn_temporal_long_f16.  MOFA_EINVAL
 * for NULL tensor pointers, Tq < 1, Tq > T, T > 128, another head_dim, a leading dimension that is not a positive multiple
 * of 8, a non-positive count, or a mask with no live slot below T -- all checked before any device call. */
int mofa_attn_temporal_long_masked_f16(const void* q, const void* k, const void* v, void* out,
                                       int nclips, int Tq, int T, int HW, int heads, int head_dim, int ld, int ldkv, int ldo,
                                       float scale, const uint32_t* key_mask, mofa_stream_t stream);
/* Local temporal self-attention over 1 <= T <= 128 frames: mofa_attn_temporal_long_f16 (the same layout, the same kernel
 * body) under a per-QUERY visibility rule given by two integers, radius >= 0 and 0 <= anchor <= T:
 *     query frame i sees key frame j  iff  j < anchor  or  |i - j| <= radius
 * -- a band around the query plus the first `anchor` frames (anchor = 1: the conditioning frame).  Every query sees itself,
 * so no softmax row is empty; an invisible key has probability exactly 0; radius >= T - 1 (larger values are accepted and mean
 * "all") or anchor == T makes every key visible.  The two integers travel as kernel arguments.  Precondition: K and V of all
 * T frames are finite -- an invisible frame is still staged and multiplied by its zero probability, so its inf or NaN would
 * reach the output (only slots that do not exist are protected, by mofa_attn_temporal_long_masked_f16).  Two equalities hold
 * bit for bit: with every key visible the output is that of mofa_attn_temporal_long_f16; and row i of the output is row i of
 * mofa_attn_temporal_long_masked_f16 called with Tq == T and the key mask {j : i sees j}.  MOFA_EINVAL for everything
 * mofa_attn_temporal_long_f16 refuses and for radius < 0, anchor < 0 or anchor > T -- all checked before any device call. */
int mofa_attn_temporal_long_local_f16(const void* q, const void* k, const void* v, void* out,
                                      int nclips, int T, int HW, int heads, int head_dim, int ld, int ldkv, int ldo,
                                      float scale, int radius, int anchor, mofa_stream_t stream);
/* Local temporal attention of a frame-sharded clip: the rule of mofa_attn_temporal_long_local_f16 on GLOBAL frame numbers,
 * for Tq query frames (rows of q / out, clip stride Tq*HW; query row i is global frame q_frame0 + i) against 1 <= S <= 128
 * key SLOTS (rows of k / v, clip stride S*HW) that hold only what those queries can see:
 *     slots [0, anchor)   the global frames 0 .. anchor - 1
 *     slot s >= anchor    the global frame band_frame0 + (s - anchor); the band has L = S - anchor slots
 * Query row i (global frame g) sees slot s iff s < anchor, or s >= anchor and frame(s) >= anchor and |g - frame(s)| <= radius.
 * A band slot that repeats an anchor frame (a shard next to the clip's start) is staged but has probability exactly 0, so
 * every key counts once.  Precondition: K and V of all S slots are finite -- every slot is staged and an invisible one is
 * multiplied by its zero probability (as for mofa_attn_temporal_long_local_f16).  Query rows >= Tq are neither read nor
 * written.  Two equalities hold bit for bit: (a) with anchor = 0, q_frame0 = band_frame0 = 0 and Tq = S = T the output is that
 * of mofa_attn_temporal_long_local_f16(radius, 0); (b) row i is row i of mofa_attn_temporal_long_masked_f16 called with the
 * same Tq and T = S under the key mask {s : i sees s}.  MOFA_EINVAL for everything mofa_attn_temporal_long_f16 refuses (with S
 * in place of T) and for Tq < 1, anchor < 0, anchor > S, radius < 0 (values above 127 are clamped: a band has at most 128
 * slots), band_frame0 < 0 or above 2^30, q_frame0 < band_frame0 or q_frame0 + Tq > band_frame0 + L (every query's own frame
 * lies in the band, so every query sees itself, directly or through its anchor slot) -- all checked before any device call. */
int mofa_attn_temporal_long_window_f16(const void* q, const void* k, const void* v, void* out,
                                       int nclips, int Tq, int S, int HW, int heads, int head_dim, int ld, int ldkv, int ldo,
                                       float scale, int radius, int anchor, int q_frame0, int band_frame0, mofa_stream_t stream);
/* Streaming local temporal self-attention over 1 <= T <= 1024 frames: the rule, the row layout and the scale convention of
 * mofa_attn_temporal_long_local_f16,
 *     query frame i sees key frame j  iff  j < anchor  or  |i - j| <= radius
 * under 0 <= radius <= 32 and 0 <= anchor <= min(T, 32).  A 32-query block then needs frame tile 0 and three band tiles only,
 * so one wave keeps four 32-frame tile slots in LDS (tile 0 and a ring of three, refilled after each block) whatever T is; K
 * and V are read from memory once, rows of frames >= T are never read or written.  Precondition: K and V of all T frames are
 * finite -- an invisible frame of a staged tile is multiplied by its zero probability.  Two equalities hold bit for bit: for
 * T <= 128 the output is that of mofa_attn_temporal_long_local_f16 under the same (radius, anchor); and for every T, row i of
 * query block tq = i / 32 is row i % 32 of mofa_attn_temporal_long_masked_f16 called with Tq == T == 128 on the frame tiles
 * [0, tq - 1, tq, tq + 1] (a slot that is out of range or a second copy of tile 0 dead) under the mask {slots i sees}.
 * MOFA_EINVAL for everything mofa_attn_temporal_long_f16 refuses, with T > 1024 in place of T > 128, and for radius < 0,
 * radius > 32, anchor < 0, anchor > 32 or anchor > T -- all checked before any device call. */
int mofa_attn_temporal_stream_local_f16(const void* q, const void* k, const void* v, void* out,
                                        int nclips, int T, int HW, int heads, int head_dim, int ld, int ldkv, int ldo,
                                        float scale, int radius, int anchor, mofa_stream_t stream);
/* Streaming temporal self-attention over 1 <= T <= 1024 frames under ANY window of the rule above, dense included: the row
 * layout, the strides, head_dim in {64, 128} and the scale convention of mofa_attn_temporal_stream_local_f16,
 *     query frame i sees key frame j  iff  j < anchor  or  |i - j| <= radius
 * under radius >= 0 (no upper limit: radius >= T - 1 hides nothing and is clamped; that is dense attention) and
 * 0 <= anchor <= T.  One wave owns a sequence and one 32-frame tile slot of K and V in LDS.  Per 32-query block it walks, in
 * ascending order and each once, the key tiles that hold a key visible to some query of the block -- tiles 0 .. ceil(anchor /
 * 32) - 1 and the tiles of frames q0 - radius .. q0 + 31 + radius, clipped to the clip -- and does not read the others; across
 * the tiles it keeps a running maximum, a running sum and fp32 accumulators, rescaled when the maximum moves (exp2 form, P
 * rounded to fp16 before P V, one multiplication by 1 / sum at the end).  A hidden key of a visited tile contributes an exact 0
 * whatever the running maximum is.  K and V of a sequence are read once per query block that sees them; rows of frames >= T are
 * never read or written.  Precondition: K and V of all T frames are finite -- an invisible frame of a visited tile is multiplied
 * by its zero probability.  Calls whose rules hide nothing (radius >= T - 1, or anchor == T) give equal bits; the output is NOT
 * bitwise that of the one-pass kernels (mofa_attn_temporal_long*_f16, ..._stream_local_f16) where both apply: the sum is taken
 * in another order.  MOFA_EINVAL for everything mofa_attn_temporal_long_f16 refuses, with T > 1024 in place of T > 128, and for
 * radius < 0, anchor < 0 or anchor > T -- all checked before any device call. */
int mofa_attn_temporal_stream_f16(const void* q, const void* k, const void* v, void* out,
                                  int nclips, int T, int HW, int heads, int head_dim, int ld, int ldkv, int ldo,
                                  float scale, int radius, int anchor, mofa_stream_t stream);
/* The streaming walk of mofa_attn_temporal_stream_f16 on the key buffer of a FRAME SHARD: Tq >= 1 query frames (rows of q / out,
 * clip stride Tq*HW) against 1 <= S <= 1024 key SLOTS (rows of k / v, clip stride S*HW), head_dim 64 or 128.  `radius` selects
 * one of two modes.
 * Window mode, radius >= 0: the contract of mofa_attn_temporal_long_window_f16 with 1024 slots for 128 -- slots [0, anchor) are
 * the global frames 0 .. anchor - 1, slot s >= anchor is the global frame band_frame0 + (s - anchor); the query of global frame
 * g = q_frame0 + row sees the anchor slots and every band slot whose frame is >= anchor and within radius of g (a band slot that
 * repeats an anchor frame counts zero times).  key_mask must be NULL.  Refused: anchor < 0 or > S, band_frame0 < 0 or above
 * 2^30, q_frame0 < band_frame0 or q_frame0 + Tq > band_frame0 + (S - anchor) (the queries' frames lie in the band); radius above
 * S - 1 is clamped (it hides nothing), so that no frame sum overflows.  Per 32-query block the walk visits, ascending and once
 * each, the anchor tiles and then the band tiles that hold a slot some query of the block can see, and no other tile.
 * Precondition: K and V of all S slots are finite -- a hidden slot of a visited tile is multiplied by its exact 0.
 * Dense mode, radius == -1: anchor, q_frame0 and band_frame0 must be 0.  key_mask is HOST memory of ceil(S / 32) words read
 * during the call, bit j % 32 of word j / 32 = slot j exists; NULL = every slot; bits at or above S are ignored; a mask with no
 * live slot is refused.  Every query sees every live slot; the walk visits the tiles whose mask word is non-zero; the K / V rows
 * of a dead slot are never read from memory (the padding slots of a gathered buffer may hold anything, NaN included) and have
 * weight exactly 0.  Tq above 2^30 is refused.
 * In both modes the mask words travel as kernel arguments (no device allocation, no copy), query rows >= Tq are neither read nor
 * written, and slot rows >= S (the next clip's) are not read.  Equal bits: (a) dense, NULL mask, Tq == S: those of
 * mofa_attn_temporal_stream_f16 dense; (b) dense, NULL mask, Tq < S on the q rows f0 .. f0 + Tq - 1 of a clip: those rows of (a);
 * (c) window with anchor = 0, q_frame0 = band_frame0 = 0, Tq == S: mofa_attn_temporal_stream_f16 under (radius, 0); (d) the
 * contents of dead slots change no bit.  MOFA_EINVAL for everything mofa_attn_temporal_long_f16 refuses (with S in place of T
 * and 1024 in place of 128), for Tq < 1, radius < -1 and for every rule above -- all checked before any device call. */
int mofa_attn_temporal_stream_shard_f16(const void* q, const void* k, const void* v, void* out,
                                        int nclips, int Tq, int S, int HW, int heads, int head_dim, int ld, int ldkv, int ldo,
                                        float scale, int radius, int anchor, int q_frame0, int band_frame0,
                                        const uint32_t* key_mask, mofa_stream_t stream);
/* in-place row softmax of an fp16 [rows][cols] matrix (VAE mid-block attention, 1 head x 512): fp32 maximum, exponentials
 * and sum, one rounding to fp16 (subnormal results kept).  cols % 8 == 0, ld % 8 == 0, ld >= cols, x 16-byte aligned; any
 * number of columns (a row is walked in passes of 2048), one workgroup per row.  MOFA_EINVAL otherwise, before any device call. */
int mofa_softmax_rows_f16(void* x, int rows, int cols, int ld, mofa_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Normalisation.  GroupNorm(32) over token-major data; statistics either per frame (2-D
 * ResnetBlock2D / transformer norm) or per clip of T frames (TemporalResnetBlock: stats span
 * T*H*W).  Three launches: partial sums -> finalize to per-(frame,channel) scale/shift -> apply.
 * Replaces nn.GroupNorm + SiLU in diffusers ResnetBlock2D / TemporalResnetBlock /
 * TransformerSpatioTemporalModel.norm / conv_norm_out (unet_..._controlnet.py:236).
 * ---------------------------------------------------------------------------------------- */
/* workspace `part`: fp32 [nframes][nparts][32][2], nparts = mofa_gn_nparts(HW, C).
 * Every entry point below returns MOFA_EINVAL without a launch unless nframes > 0, HW > 0 (where it takes one), 0 < C,
 * C % 32 == 0 (mofa_affine_act_f16: C % 8 == 0), frames_per_stat > 0 divides nframes and every ld is a multiple of 8;
 * the entry points that stage C channels in LDS (partial, apply, apply_gathered) also want C <= 4096. */
int mofa_gn_nparts(int HW, int C);
int mofa_gn_partial_f16(const void* x, float* part, int nframes, int HW, int C, int ldx, mofa_stream_t stream);
/* the same `part` entries from the pair sums an implicit-GEMM epilogue emitted (mofa_igemm_args.stats: fp32 [nframes * HW / 64][C]),
 * 64-row blocks dealt to the nparts entries of a frame in order, fixed summation order; HW % 64 == 0, (C / 32) even */
int mofa_gn_partial_from_stats(const float* stats, float* part, int nframes, int HW, int C, mofa_stream_t stream);
/* frames_per_stat = 1 (spatial) or T (temporal); writes scale/shift fp32 [nframes][C].  HW > 0, C > 0, C % 32 == 0 */
int mofa_gn_finalize(const float* part, const float* gamma, const float* beta, float* scale, float* shift,
                     int nframes, int HW, int C, int frames_per_stat, float eps, mofa_stream_t stream);
/* split form for frame-sharded clips: partials -> fp64 [nstat][32][2] (sum, sum of squares); the caller all-reduces
 * them over the ranks holding the clip's other frames, then finalizes with the global per-group element count
 * (mofa_gn_reduce: HW > 0, C > 0, C % 32 == 0; mofa_gn_finalize_sums: C > 0, C % 32 == 0, count_per_group > 0) */
int mofa_gn_reduce(const float* part, double* sums, int nframes, int HW, int C, int frames_per_stat, mofa_stream_t stream);
int mofa_gn_finalize_sums(const double* sums, const float* gamma, const float* beta, float* scale, float* shift,
                          int nframes, int C, int frames_per_stat, double count_per_group, float eps,
                          mofa_stream_t stream);
/* fused finalize + apply (single-rank path): every workgroup combines the partial sums of its statistics set itself (fp64,
 * fixed order) and applies y = (x - mean) * rstd * gamma + beta, optional SiLU -- no scale / shift buffers, no finalize launch.
 * Meant for frames_per_stat * mofa_gn_nparts(HW, C) <= 512 entries (100 KB of partials re-read per workgroup from L2).
 * 0 < C <= 4096 (the same limit as mofa_gn_partial_f16), C % 32 == 0. */
int mofa_gn_apply_f16(const void* x, const float* part, const float* gamma, const float* beta, void* y,
                      int nframes, int HW, int C, int ldx, int ldy, int frames_per_stat, float eps, int silu,
                      mofa_stream_t stream);
/* the same for a statistics set whose frames are sharded over ranks (new work; the reference is single-GPU): `part_all` = the
 * all-gathered partials of the WHOLE set, `nentries` x [32][2] fp32 (zero entries for padding frames), combined by every
 * workgroup in entry order; `count_per_group` = elements per group over the whole set.  Applies that one set to the `nframes`
 * frames of x (the rank's own frames, or a halo frame received raw from a neighbour shard).  0 < C <= 4096, C % 32 == 0,
 * 0 < nentries <= 4096, count_per_group > 0. */
int mofa_gn_apply_gathered_f16(const void* x, const float* part_all, int nentries, double count_per_group,
                               const float* gamma, const float* beta, void* y, int nframes, int HW, int C,
                               int ldx, int ldy, float eps, int silu, mofa_stream_t stream);
/* y = x*scale[frame][c] + shift[frame][c]; optional SiLU.  C > 0, C % 8 == 0 */
int mofa_affine_act_f16(const void* x, const float* scale, const float* shift, void* y,
                        int nframes, int HW, int C, int ldx, int ldy, int silu, mofa_stream_t stream);
/* LayerNorm over C per token (eps, affine); optional pre-add of rowvec[(m / rv_div) % rv_mod][C].  0 < C <= 1280, C % 8 == 0,
 * ld* % 8 == 0; with a row vector rv_div > 0 and rv_mod > 0 */
int mofa_layernorm_f16(const void* x, const float* gamma, const float* beta, void* y, int M, int C,
                       int ldx, int ldy, float eps, const float* rowvec, int rv_div, int rv_mod,
                       mofa_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused feed-forward for 320-channel tokens (level 0 of the UNet / ControlNet): ONE launch for
 *   LayerNorm -> GEGLU projection (320 -> 2 x 1280) -> value * gelu(gate) -> output projection (1280 -> 320) -> residuals
 * i.e. the feed-forward legs of diffusers' BasicTransformerBlock (norm3 -> ff) and TemporalBasicTransformerBlock (norm_in -> ff_in,
 * norm3 -> ff) as the reference builds them (models/unet_spatio_temporal_condition_controlnet.py:169-232,
 * models/controlnet_sdv.py:259-309); replaces mofa_layernorm_f16 + two mofa_igemm_f16 launches and the [M, 1280] hidden tensor.
 *   x'[m]   = x[m] + pos[(m / HW) % T]                                  (pos == NULL: x' = x)
 *   out[m]  = f16( f16( s_acc * (W2 . (val * gelu_erf(gate)) + b2) ) + s1 * x'[m] + s2 * r2[m] ),
 *             [val | gate] = W1 . LayerNorm_eps(x'[m]) + b1
 *   out_ln[m] = LayerNorm_ln_eps(out[m]) * ln_gamma + ln_beta          (optional second output: the norm of the NEXT projection)
 * Packed operands (mofa_video_amd/weights.py::pack_ff320 writes them; all index ranges below are inclusive-exclusive):
 *   w1p  fp16 [40 chunks][2 (value, gate)][20 k-steps][64 lanes][8]: element e of lane l = W1g[t * 1280 + 32 c + (l & 31)]
 *        [16 s + 8 (l >> 5) + e], W1g = net.0.proj.weight * LayerNorm gain (per input channel), rows [0,1280) value, [1280,2560) gate
 *   b1   fp32 [2560] = net.0.proj.bias + net.0.proj.weight . LayerNorm bias                      (natural order)
 *   w2p  fp16 [40 chunks][10 out tiles][2 k-steps][64 lanes][8]: element jj of lane l = net.2.weight[32 j + (l & 31)]
 *        [32 c + 16 u + 4 (l >> 5) + (jj & 3) + 8 (jj >> 2)]
 *   b2   fp32 [320]
 * All pointers 16-byte aligned, ld* % 8 == 0.  fp16 MFMA, fp32 accumulation / LayerNorm / GELU / residual arithmetic.
 * tests/test_l0_matrix_gpu.py runs the row edges, three tiles per workgroup on periodic rows and poisoned rows. */
typedef struct mofa_ff320_args {
    const void* x;          /* fp16 [M][ldx]                                    */
    const float* pos;       /* fp32 [T][320] or NULL                            */
    const void* w1p;        /* packed, see above                                */
    const float* b1;
    const void* w2p;
    const float* b2;
    const void* r2;         /* fp16 [M][ldr2] or NULL                           */
    void* out;              /* fp16 [M][ldo]                                    */
    void* out_ln;           /* fp16 [M][ldoln] or NULL                          */
    const float* ln_gamma;  /* fp32 [320] (with out_ln)                         */
    const float* ln_beta;
    int32_t M, ldx, ldo, ldr2, ldoln, HW, T;
    float eps, s_acc, s1, s2, ln_eps;
    int32_t reserved[4];    /* must be 0; sizeof(mofa_ff320_args) = 152         */
} mofa_ff320_args;
int mofa_ff320_f16(const mofa_ff320_args* a, mofa_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Linear layers on 320-channel tokens (level 0), transposed form, optional LayerNorm in front:
 *   out[m, n] = f16( f16( s_acc * (W[n, :] . xhat[m] + bias[n] + rowvec[idx(m), n]) ) + s1 * r1[m, n] ),     n < N, N % 64 == 0
 *   xhat[m] = norm ? LayerNorm_eps(x[m]) without affine part (the norm's gain / bias are folded into W / bias) : x[m]
 *   idx(m) = ((m / rv_div) * rv_mul + (m % rv_mod_in)) % rv_mod_out          (as mofa_igemm_f16; rowvec row idx at rowvec + idx * N)
 * i.e. norm1 -> to_q | to_k | to_v (N = 960), to_out.0 + attn2's vector + residual, proj_in of diffusers' BasicTransformerBlock /
 * TemporalBasicTransformerBlock / TransformerSpatioTemporalModel at 320 channels (built at
 * models/unet_spatio_temporal_condition_controlnet.py:169-232, models/controlnet_sdv.py:259-309); replaces mofa_layernorm_f16 +
 * mofa_igemm_f16 for them.  wp: fp16 [N / 64 chunks][2 tiles][20 k-steps][64 lanes][8]: element e of lane l =
 * W'[64 c + 32 t + (l & 31)][16 s + 8 (l >> 5) + e], W' = W * LayerNorm gain (mofa_video_amd/weights.py::pack_lin320);
 * bias fp32 [N] (+ W . LayerNorm bias) or NULL.  Pointers 16-byte aligned, ld* % 8 == 0.  The output is addressed through a 32-bit
 * buffer descriptor (rows beyond M are dropped by its bounds check): (M + 256) * ldo * 2 bytes must stay below 4 GB, MOFA_EINVAL
 * otherwise (the caller then uses mofa_layernorm_f16 + mofa_igemm_f16: mofa_video_amd/ops.py::lin320_fits).
 * tests/test_l0_matrix_gpu.py holds all eight instances to the two roundings above bit for bit, on exactly representable sums. */
typedef struct mofa_lin320_args {
    const void* x;          /* fp16 [M][ldx], 320 channels                      */
    const void* wp;         /* packed, see above                                */
    const float* bias;      /* fp32 [N] or NULL                                 */
    const float* rowvec;    /* fp32 rows of N or NULL                           */
    const void* r1;         /* fp16 [M][ldr1] or NULL                           */
    void* out;              /* fp16 [M][ldo]                                    */
    int32_t M, N, ldx, ldo, ldr1, norm;
    int32_t rv_div, rv_mul, rv_mod_in, rv_mod_out;
    float eps, s_acc, s1;
    int32_t reserved[3];    /* must be 0; sizeof(mofa_lin320_args) = 112         */
} mofa_lin320_args;
int mofa_lin320_f16(const mofa_lin320_args* a, mofa_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Element-wise / data movement
 * ---------------------------------------------------------------------------------------- */
/* y = a*x + b*y on contiguous fp32 vectors (latent window accumulation / averaging of the Keypoint loop,
 * MOFA-Video-Keypoint/pipeline/svdxt_pipeline_ctrlnet_loop.py:502-511) */
int mofa_axpby_f32(const float* x, float* y, int64_t n, float a, float b, mofa_stream_t stream);
/* nearest-neighbour resize of fp32 planes [n][H][W] -> [n][h][w], src = floor(dst * in/out) (F.interpolate 'nearest') */
int mofa_resize_nearest_f32(const float* x, float* y, int n, int H, int W, int h, int w, mofa_stream_t stream);
/* out[m][c] = a[m][c]*w[m % HW] + b[m][c]*(1 - w[m % HW]): Hybrid residual blend by the user mask
 * (MOFA-Video-Hybrid/pipeline/pipeline.py:479-489); w fp32 [HW]; C % 8 == 0 */
int mofa_mask_blend_f16(const void* a, const void* b, const float* w, void* out, int M, int C, int HW, int lda,
                        int ldb, int ldo, mofa_stream_t stream);
/* ForegroundMatting tail (MOFA-Video-Hybrid/models/occlusion/hourglass.py:266-280):
 * mask = sigmoid(logit[m]); out[m][c] = warped[m][c]*mask + matting[m][c]*(1-mask); mask_out fp32 [M] (optional) */
int mofa_matting_blend_f16(const void* warped, const void* matting, const void* logit, void* out, float* mask_out,
                           int M, int C, int ldw, int ldm, int ldl, int ldo, mofa_stream_t stream);
/* F.interpolate(scale_factor=1/s, nearest) of token-major maps [n][H][W][C] -> [n][H/s][W/s][C]
 * (landmark embedding pyramid, MOFA-Video-Hybrid/models/ldmk_ctrlnet.py:399-403) */
int mofa_subsample_tokens_f16(const void* x, void* y, int n, int H, int W, int s, int C, int ldx, int ldy,
                              mofa_stream_t stream);
/* y[m][c] = a * x[m][c] + b * y[m][c]  (fp16 storage, fp32 math); C % 8 == 0 */
int mofa_axpby_f16(const void* x, void* y, int M, int C, int ldx, int ldy, float a, float b, mofa_stream_t stream);
/* out[m][c] = a * x[m][c] + b * y[m][c], written elsewhere (x, y untouched): the UNet's skip + ControlNet residual sum goes
 * straight into its column slice of the decoder's concat buffer (unet_spatio_temporal_condition_controlnet.py:447-459, :478-483) */
int mofa_axpby_out_f16(const void* x, const void* y, void* out, int M, int C, int ldx, int ldy, int ldo, float a, float b,
                       mofa_stream_t stream);
/* out[m][j] = x[m][j] * gelu(x[m][Ch + j]), j < Ch  (diffusers GEGLU, erf gelu).  gelu(g) = g * erfc(-g / sqrt2) / 2 with
 * fp32 relative accuracy in both tails (the fused MOFA_ACT_GEGLU_PAIR epilogue uses a clamped polynomial, 5e-5 absolute) */
int mofa_geglu_f16(const void* x, void* out, int M, int Ch, int ldx, int ldo, mofa_stream_t stream);
/* strided 2-D copy of a column block: dst[m][0..C) = src[m][0..C); C % 8 == 0 */
int mofa_copy2d_f16(const void* src, void* dst, int M, int C, int lds, int ldd, mofa_stream_t stream);
/* y = silu(x) on fp32 vectors (time-embedding non-linearity) */
int mofa_silu_f32(const float* x, float* y, int n, mofa_stream_t stream);
/* fp32 -> fp16 / fp16 -> fp32 contiguous casts */
int mofa_cast_f32_to_f16(const float* x, void* y, int64_t n, mofa_stream_t stream);
int mofa_cast_f16_to_f32(const void* x, float* y, int64_t n, mofa_stream_t stream);
/* NCHW fp32 [n][C][H][W] * scale -> token-major fp16 [n][H*W][ldo] (channels >= C left untouched) and back.  The value is
 * one fp32 product rounded once to fp16 (back: the fp16 value as fp32).  Any C, HW >= 1 (tiles of 32 channels x 32 pixels,
 * ragged edges masked); ldo / ldx >= C, no alignment asked; the image count n is a grid dimension, at most 65535 (and
 * C <= 32 * 65535).  MOFA_EINVAL otherwise, before any device call. */
int mofa_nchw_f32_to_nhwc_f16(const float* x, void* y, int n, int C, int HW, int ldo, float scale,
                              mofa_stream_t stream);
int mofa_nhwc_f16_to_nchw_f32(const void* x, float* y, int n, int C, int HW, int ldx, mofa_stream_t stream);
/* sinusoidal Timesteps(dim, flip_sin_to_cos=True, shift=0): out fp32 [n][dim]  (diffusers embeddings.py) */
int mofa_timestep_embedding(const float* t, float* out, int n, int dim, mofa_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * MOFA-Adapter warp: softsplat(tenIn, tenFlow, None, 'avg')  (models/softsplat.py:232-274 +
 * kernel softsplat_out :284-345).  Deterministic gather form, fused normalisation.
 *   feat : fp16 token-major [HW][ldf]      (first-frame feature, one image)
 *   flow : fp32 [nflows][2][H][W]          (flow frame 0 -> frame i+1 at feature resolution)
 *   out  : fp16 token-major [nflows][HW][ldo]
 *   ws   : int32/fp32 workspace, mofa_softsplat_ws_bytes(nflows, H, W) bytes (formed in 64 bits), cleared by every call:
 *          what it held before does not matter, and nothing beyond that size is touched
 * Limits of mofa_softsplat_avg_f16, checked before any device call (MOFA_EINVAL): no NULL pointer; 1 <= nflows <= 65535 (a grid
 * dimension); H, W >= 1 and H * W < 2^29 (the CSR keys corner * HW + source are int; the product is formed in 64 bits); C >= 8
 * and a multiple of 8; ldf and ldo multiples of 8.  A source whose target x + flow is not finite is skipped; a finite target
 * however far outside the plane (beyond the int range included) contributes to no pixel.
 * mofa_softsplat_scatter_f32 is the atomicAdd form of the reference kernel on NCHW fp32
 * (same op order class as the CUDA kernel; used for parity classing and as a bench baseline).
 * ---------------------------------------------------------------------------------------- */
int64_t mofa_softsplat_ws_bytes(int nflows, int H, int W);
int mofa_softsplat_avg_f16(const void* feat, const float* flow, void* out, void* ws,
                           int nflows, int H, int W, int C, int ldf, int ldo, mofa_stream_t stream);
int mofa_softsplat_scatter_f32(const float* in, const float* flow, float* out_sum, int N, int C, int H, int W,
                               mofa_stream_t stream);
/* the wrapper's metric-weighted modes (models/softsplat.py:243-270; not on the inference path): 'linear' (mode 1) / 'soft' (mode 2)
 * build [in * w | w], w = metric / exp(metric), fp32 [N][C+1][H][W]; after mofa_softsplat_scatter_f32 of that, the normalisation
 * divides by the splatted last channel: eps_mode 0 '+1e-7' ('' / 'addeps'), 1 'zeroeps', 2 'clipeps', 3 unchanged */
int mofa_softsplat_weight_f32(const float* in, const float* metric, float* out, int N, int C, int H, int W, int mode,
                              mofa_stream_t stream);
int mofa_softsplat_normalize_f32(const float* summed, float* out, int N, int C, int H, int W, int eps_mode, mofa_stream_t stream);
/* Backward of the warp (softsplat_func.backward, models/softsplat.py:349-524, through the wrapper's mode prep and normalisation
 * :243-270), fp32 NCHW, no atomics: every sum runs in a fixed order, so the gradients are reproducible bit for bit.  Element
 * offsets are 64-bit; H * W must stay below 2^29 and N at most 65535 (MOFA_EINVAL otherwise).
 *   mofa_softsplat_norm_f32: norm fp32 [N][H][W] = the per-target sum of splat weights of flow [N][2][H][W], added in the order
 *     mofa_softsplat_avg_f16 adds them, so norm + 1e-7 is bit for bit what its 'avg' forward divided by.  ws: the CSR workspace,
 *     mofa_softsplat_ws_bytes(N, H, W) bytes.
 *   mofa_softsplat_grad_prologue_f32: per target of the normalised modes, with S = norm (the splatted last channel), nu = n(S) as
 *     mofa_softsplat_normalize_f32's eps_mode forms it, grad / out the fp32 [N][C][H][W] gradient and value of the normalised
 *     output:  inv = 1 / nu,  glast = -n'(S) * sum_c grad_c * out_c / nu  (both fp32 [N][H][W]; n' = 0 where 'zeroeps' replaced a
 *     zero or 'clipeps' clamped, 1 otherwise).
 *   mofa_softsplat_grad_f32: the gradients of one splat of Ĩ = prep(I, m), Ĩ with Cs channels:
 *     prep 0  Ĩ = I              ('sum*' with inv = NULL; 'avg-<suffix>', whose normaliser is I's own last channel)  Cs = C
 *     prep 1  Ĩ = [I | 1]        ('avg')                                                                           Cs = C + 1
 *     prep 2  Ĩ = [I * m | m]    ('linear*')                                                                       Cs = C + 1
 *     prep 3  Ĩ = [I e^m | e^m]  ('soft*')                                                                         Cs = C + 1
 *     grad has Cg = Cs - 1 channels when inv / glast are given (the normalised modes: ghat_c = grad_c * inv for c < Cg, ghat_Cg =
 *     glast), Cg = Cs without them (the raw sum: ghat = grad).  A source whose target is not finite gets 0 in every gradient.
 *     Every output is optional (NULL = not computed; at least one); `in` is read only for grad_flow / grad_metric.  The channels
 *     are split into `slices` (1 <= slices <= Cs) of ceil(Cs / slices) channels, one workgroup row each; with slices > 1 and
 *     grad_flow or grad_metric, `partial` holds slices * N * 3 * H * W floats (the per-slice flow / metric sums, added in slice
 *     order by a second launch).  The result depends on `slices`; for a given shape the caller keeps it fixed. */
typedef struct mofa_softsplat_grad_args {
    const float* grad;      /* fp32 [N][Cg][H][W]                               */
    const float* flow;      /* fp32 [N][2][H][W]                                */
    const float* in;        /* fp32 [N][C][H][W] (with grad_flow / grad_metric) */
    const float* metric;    /* fp32 [N][H][W], prep 2 / 3 only                  */
    const float* inv;       /* fp32 [N][H][W] or NULL (prologue)                */
    const float* glast;     /* fp32 [N][H][W], with inv                         */
    float* grad_in;         /* fp32 [N][C][H][W] or NULL                        */
    float* grad_flow;       /* fp32 [N][2][H][W] or NULL                        */
    float* grad_metric;     /* fp32 [N][H][W] or NULL, prep 2 / 3 only          */
    float* partial;         /* fp32 [slices][N][3][H][W], see above             */
    int32_t N, C, H, W, prep, slices;
    int32_t reserved[4];    /* must be 0; sizeof(mofa_softsplat_grad_args) = 120 */
} mofa_softsplat_grad_args;
int mofa_softsplat_norm_f32(const float* flow, float* norm, void* ws, int N, int H, int W, mofa_stream_t stream);
int mofa_softsplat_grad_prologue_f32(const float* grad, const float* out, const float* norm, float* inv, float* glast,
                                     int N, int C, int H, int W, int eps_mode, mofa_stream_t stream);
int mofa_softsplat_grad_f32(const mofa_softsplat_grad_args* a, mofa_stream_t stream);
/* Forward of the warp in gather form, every mode of the wrapper (models/softsplat.py:232-274) in one call: fp32 NCHW in and out as
 * the reference computes it (custom_fwd(cast_inputs=torch.float32)), the normalisation fused, no atomics on any value that reaches
 * an output, so two calls on one input give the same bits.  One splat of Ĩ = prep(I, m), prep as in mofa_softsplat_grad_args:
 *     strMode               prep  normalize  channels of out  normaliser S
 *     'sum', 'sum-*'        0     0          C                -
 *     'avg'                 1     1 (eps 0)  C                sum w
 *     'avg-<suffix>'        0     1          C - 1            sum w * I_last   (the input's own last channel)
 *     'linear*' / 'soft*'   2 / 3 1          C                sum w * m  /  sum w * e^m
 *   in fp32 [N][C][H][W]; flow fp32 [N][2][H][W]; metric fp32 [N][H][W] with prep 2 / 3 and NULL otherwise; out fp32
 *   [N][Co][H][W]; norm (optional, normalize = 1 only) fp32 [N][H][W] = S before its eps handling, what
 *   mofa_softsplat_grad_prologue_f32 takes; ws the CSR workspace, mofa_softsplat_ws_bytes(N, H, W) bytes, rebuilt by every call.
 *   Order of summation: per target the contributions are added in CSR order -- corners NW, NE, SW, SE, sources in raster order
 *   within a corner -- as acc = acc + ((I * a) * w) with a = 1 / m / e^m, every product and every sum rounded on its own (no fused
 *   multiply-add); with normalize = 1, out = acc / n(S), n as mofa_softsplat_normalize_f32's eps_mode forms it, a correctly rounded
 *   division.  That is the order and the operation set of the CPU oracle: the raw sum equals it bit for bit.  A target with more
 *   than 128 entries is summed by a whole workgroup, one channel per thread, in the same order.
 *   The output channels are split into `slices` (1 <= slices <= Co) of ceil(Co / slices), one workgroup row each; every slice
 *   forms the normaliser itself, so the result does not depend on `slices`.  Limits: N <= 65535, H * W < 2^29; prep >= 1 needs
 *   normalize = 1; every rule is checked before any device call (MOFA_EINVAL).  No allocation, the caller's stream, no
 *   synchronisation. */
typedef struct mofa_softsplat_gather_args {
    const float* in;        /* fp32 [N][C][H][W]                                 */
    const float* flow;      /* fp32 [N][2][H][W]                                 */
    const float* metric;    /* fp32 [N][H][W], prep 2 / 3 only                   */
    float* out;             /* fp32 [N][Co][H][W]                                */
    float* norm;            /* fp32 [N][H][W] or NULL                            */
    void* ws;               /* mofa_softsplat_ws_bytes(N, H, W) bytes            */
    int32_t N, C, H, W, prep, normalize, eps_mode, slices;
    int32_t reserved[4];    /* must be 0; sizeof(mofa_softsplat_gather_args) = 96 */
} mofa_softsplat_gather_args;
int mofa_softsplat_gather_f32(const mofa_softsplat_gather_args* a, mofa_stream_t stream);
/* F.interpolate(flow, scale_factor=1/s) (nearest) / s  (svdxt_..._norefine.py:302-309): fp32 [n][2][H][W] -> [n][2][H/s][W/s] */
int mofa_flow_downscale_f32(const float* flow, float* out, int n, int H, int W, int s, mofa_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Scheduler math (pipeline/pipeline.py:449-452, :495-500; utils/scheduling_euler_discrete_karras_fix.py:264-288, :418-528)
 * ---------------------------------------------------------------------------------------- */
/* model input: out[2][T][HW][ldo] fp16: cols 0..3 = latents/sqrt(sigma^2+1) (both CFG halves),
 * cols 4..7 = image_latents[half] ; latents fp32 [T][4][HW] (NCHW), image_latents fp32 [2][4][HW].  The latent columns are
 * one fp32 product with fl32(1/sqrt(sigma^2+1)) rounded once to fp16; columns >= 8 of a row are left untouched.
 * T, HW >= 1, ldo % 8 == 0, ldo >= 8 (and for the step below ldn % 4 == 0, sigma > 0), MOFA_EINVAL otherwise. */
int mofa_prepare_model_input(const float* latents, const float* image_latents, void* out,
                             int T, int HW, int ldo, float sigma, mofa_stream_t stream);
/* CFG + v-prediction Euler step, fp32 latents in place.
 * noise_pred fp16 token-major [2][T][HW][ldn] (uncond first), g_f = gmin + (gmax-gmin)*f/(T-1) */
int mofa_cfg_euler_step(float* latents, const void* noise_pred, int T, int HW, int ldn,
                        float sigma, float sigma_next, float gmin, float gmax, mofa_stream_t stream);
/* The same two with the step's scalars read from DEVICE memory: `step_scalars` = one row of a per-clip step table, fp32
 * [MOFA_STEP_SCALARS] = {sigma, sigma_next, timestep, timestep, 1/sqrt(sigma^2+1), 0, 0, 0} (the scheduler's sigma table
 * :337-349 uploaded once per clip; columns 2..3 double as the fp32 [2] timestep tensor of mofa_timestep_embedding).  No
 * host scalar enters a denoise step, so a whole step can be captured in a hipGraph and replayed: mofa_step_select is the
 * graph's first node -- cur[..] = table[*counter][..]; ++*counter -- and every other node reads `cur`. */
#define MOFA_STEP_SCALARS 8
int mofa_prepare_model_input_dev(const float* latents, const float* image_latents, void* out,
                                 int T, int HW, int ldo, const float* step_scalars, mofa_stream_t stream);
int mofa_cfg_euler_step_dev(float* latents, const void* noise_pred, int T, int HW, int ldn,
                            const float* step_scalars, float gmin, float gmax, mofa_stream_t stream);
int mofa_step_select(const float* table, int* counter, float* cur, int nsteps, mofa_stream_t stream);


/* ---- output stage (the step after the path) -------------------------------------------------------------
 * Replaces tensor2vid -> VaeImageProcessor.postprocess (Traj/pipeline/pipeline.py:57-69, :518): decoded fp32 frames
 * [nframes][3][H][W] -> (x/2+0.5).clamp(0,1) as fp32 NCHW ("pt"), fp32 NHWC ("np") or uint8 NHWC ("pil":
 * round-half-even(x*255)).  A NaN input stays NaN in the two float modes, as torch's clamp propagates it (a broken decode
 * must not come out as clean black frames); the uint8 mode, which has no NaN, writes 0 for it.  +-inf clamp to 1 / 0. */
#define MOFA_FRAMES_PT 0
#define MOFA_FRAMES_NP 1
#define MOFA_FRAMES_U8 2
int mofa_frames_postprocess_f32(const float* frames_nchw, void* out, int nframes, int H, int W, int mode,
                                mofa_stream_t stream);
/* Middlebury colour coding of one flow field, fp32 [H][W][2] -> uint8 [H][W][3]; replaces flow_to_image
 * (Traj/utils/flow_viz.py:241-277 with compute_color :196-238).  workspace: mofa_flow_to_image_ws_bytes(H, W).
 * A pixel with a component beyond 1e7 in magnitude (exactly 1e7 is not) is unknown: black, and left out of the maximum
 * radius that scales the picture.  A pixel with a NaN component is treated the same way: black, excluded from the maximum,
 * and every other pixel is as if it held zero flow.  This deliberately does not copy the reference's accident: there
 * compute_color also blackens the pixel, but max(-1, nan) makes the maximum -1, which negates and rescales all the others.
 * The maximum is sqrt(u*u + v*v) with every operation rounded to fp32 on its own, as torch computes it. */
int64_t mofa_flow_to_image_ws_bytes(int H, int W);
int mofa_flow_to_image_u8(const float* flow_hw2, unsigned char* out_hw3, int H, int W, void* workspace,
                          mofa_stream_t stream);

/* ---- landmark pose images (the `landmarks` argument of the Keypoint / Hybrid pipelines) ---------------------
 * Replaces draw_landmarks (MOFA-Video-Keypoint/utils/utils.py:26-46: the 15 polylines of a 68-point face, 63 segments,
 * cv2.line(thickness=2) on a draw_size x draw_size float64 canvas) + cv2.resize to the clip size + / 255
 * (mofa_keypoint.py:299-316), bit-equal to mofa_video_amd/landmarks.py's restatement of them.
 * pts: device int32 [N][68][2] (x, y), landmark coordinates already scaled to the draw_size canvas and truncated toward
 * zero (as draw_landmarks' int() does), each within +-32767: a segment with an end point beyond that is not drawn.
 * out: device fp32 [N][3][H][W], values in [0, 1].
 * workspace: device, N * draw_size * draw_size * 4 bytes, 16-byte aligned (the int32 segment-index canvases; the call
 * clears them itself).  draw_size <= 4096; H * W < 2^31. */
int mofa_pose_images_f32(const int32_t* pts, float* out, void* workspace, int N, int H, int W, int draw_size,
                         mofa_stream_t stream);

/* ---- control signals: sparse CMP input from points, controlnet_flow from CMP's output ------------------------
 * mofa_sparse_points_f32: K points per frame -> the dense input of the CMP encoder, out fp32 [n][4][H][W] = dx, dy, mask,
 * mask.  pos: device int32 [K][2] (row, col), shared by all n frames; val: device fp32 [n][K][2], (dx, dy) of point k in
 * frame i.  The launch clears `out` itself (a memset on the stream, ordered before the point writes); K = 0 with
 * pos = val = NULL is valid and only clears.  Every pixel has one writing thread, chosen by the point order alone: no
 * atomics, bit-identical repeat launches.
 *   MOFA_SPARSE_ADD (get_sparseflow_and_mask_forward, MOFA-Video-Traj/run_gradio.py:61-86): the pixel of point k gets the sum
 *     of val[i][k'] over all k' on the same pixel, added in ascending k', and both mask channels their number.  Positions
 *     must lie in [0,H) x [0,W).  They are device memory, which the launcher cannot inspect: the caller checks them
 *     (mofa_video_amd/ops.py::sparse_points raises ValueError on the host); a point off the canvas is never written and
 *     never counted.  The sums are exact while |sum| < 2^24 for integer-valued val.
 *   MOFA_SPARSE_LAST (sample_optical_flow, MOFA-Video-Keypoint/utils/utils.py:81-103): positions are clipped to [0,H-1] /
 *     [0,W-1]; the point with the highest k on a pixel wins, its val is copied bit for bit (NaN included), masks are 1.
 * Limits: K <= 4096, n <= 65535, H * W < 2^31; beyond them, for NULL out, negative sizes or an unknown mode: MOFA_EINVAL. */
enum { MOFA_SPARSE_ADD = 0, MOFA_SPARSE_LAST = 1 };
int mofa_sparse_points_f32(const int* pos, const float* val, int K, int n, int H, int W, int mode, float* out,
                           mofa_stream_t stream);
/* mofa_flow_finish_f32: the tail of get_flow (run_gradio.py:236-277: brush multiply, nearest resize, rescale) and
 * merge_inmask_outmask (:290-330) in one pass.  flow_in / flow_out: device fp32 [n][2][hs][ws] or NULL (= zeros: a group
 * without tracks); brush: device uint8 [hs][ws] or NULL, applies to flow_in only; out: device fp32 [n][2][H][W].
 * Per output pixel: src = the index of mofa_resize_nearest_f32; a = flow_in[src] * ((float)brush[src] / 255.0f) (no multiply
 * without a brush); if (H, W) != (hs, ws), a.x and b.x are multiplied by (float)((double)W / ws), a.y and b.y by
 * (float)((double)H / hs); out = (a.x != 0 && a.y != 0) ? a : b.  Every operation is rounded on its own.  -0.0 counts as
 * zero, NaN as non-zero and is kept.  A flow that has no merge partner (Keypoint) goes in as flow_out with flow_in = NULL: it
 * is resized and rescaled only -- as flow_in its pixels with one zero component would lose the other.  16-byte accesses are used where pointers and rows are 16-byte aligned, scalar ones
 * elsewhere: no alignment is required.  H * W and hs * ws < 2^31, n * H * ceil(W / 4) < 2^39. */
int mofa_flow_finish_f32(const float* flow_in, const float* flow_out, const unsigned char* brush, int n, int hs, int ws, int H,
                         int W, float* out, mofa_stream_t stream);

/* ---- image conditioning front end (the step before the loop) ------------------------------------------------
 * _resize_with_antialiasing (MOFA-Video-Traj/pipeline/pipeline.py:531-562) = separable Gaussian blur with reflect
 * padding (_gaussian_blur2d :632-645, _filter2d :587-610; x pass then y pass) + F.interpolate(bicubic, align_corners=True).
 * fp32 planes [nplanes][H][W]; taps = k fp32 weights on the device; axis 1 = along W, 0 = along H; out != x. */
int mofa_filter1d_reflect_f32(const float* x, float* out, const float* taps, int nplanes, int H, int W, int k, int axis,
                              mofa_stream_t stream);
int mofa_resize_bicubic_ac_f32(const float* x, float* out, int nplanes, int Hin, int Win, int Hout, int Wout,
                               mofa_stream_t stream);
/* operand of the CLIP patch embedding (transformers CLIPVisionEmbeddings.patch_embedding, stride = kernel = p):
 * fp32 [nimg][C][H][W] -> fp16 [nimg*(H/p)*(W/p)][ld], column c*p*p + py*p + px, columns >= C*p*p zero */
int mofa_patchify_f16(const float* x, void* out, int nimg, int C, int H, int W, int p, int ld, mofa_stream_t stream);

/* ---- CMP sparse-to-dense motion encoder, non-convolution pieces (the step before the path) -----------------
 * Token-major fp16 maps [nimg*H*W][ld].  pool2d: nn.MaxPool2d (mode 0, padding ignored) / nn.AvgPool2d (mode 1)
 * (Traj/models/cmp/models/backbone/resnet.py:108, modules/shallownet.py:16-21, modules/decoder.py:115-139).
 * Output size floor((Hin + 2*pad - k) / stride) + 1 per axis.  As in torch the window must fit into the padded map and the
 * padding is at most half a window: k > Hin + 2*pad, k > Win + 2*pad or 2*pad > k return MOFA_EINVAL (so the numerator is
 * never negative and every window holds at least one pixel of the map); mode 1 takes pad == 0 only; C, ldx, ldo % 8 == 0. */
int mofa_pool2d_f16(const void* x, void* out, int nimg, int Hin, int Win, int C, int ldx, int ldo, int k, int stride, int pad,
                    int mode, mofa_stream_t stream);
/* F.interpolate(mode="bilinear", align_corners=True): token-major fp16 maps (modules/decoder.py:192-211) and fp32
 * planes [nplanes][H][W] (svdxt_..._norefine.py:58-60). */
int mofa_resize_bilinear_ac_f16(const void* x, void* out, int nimg, int Hin, int Win, int Hout, int Wout, int C, int ldx, int ldo,
                                mofa_stream_t stream);
int mofa_resize_bilinear_ac_f32(const float* x, float* out, int nplanes, int Hin, int Win, int Hout, int Wout,
                                mofa_stream_t stream);
/* Fuser.convert_flow (cmp/utils/visualize_utils.py:6-19): logits fp16 [nimg*HW][ld], bins [0,nbins) x, [nbins,2nbins) y
 * -> fp32 flow [nimg][2][HW] = per-axis softmax expectation over the bin centres (b + 1/2) * 2*fmax/nbins - fmax. */
int mofa_flow_expectation_f16(const void* logits, float* flow_nchw, int nimg, int HW, int ld, int nbins, float fmax,
                              mofa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MOFA_HIP_H */
