// igemm_tn8: weight gradients of the 4x4 / stride-2 / pad-1 convolutions (every big layer of the CelebA and dSprites networks, in
// conv view also the transposed convolutions), 16-bit types:
//
//     S[n][t][c] = sum_m P[m][n] * X[pix(m, t)][c]        P = output gradient [M][N], X = layer input [B,H,W,C], t = filter tap
//
// split over m into fp32 slabs [split][N][16][C] (the layout of igemm_tn_kernel: the slab reductions are shared).
//
// What igemm_tn_kernel does per workgroup and tap -- 32 rows of P and 32 gathered rows of X per barrier through registers, 16 MFMAs
// per wave between barriers, every input pixel fetched once per tap (16 x) and every P row once per tap and channel tile -- is
// replaced by:
//   * one workgroup = 128 output channels x 128 input channels x the FOUR taps of one input-parity class (ty = ry + 2 ay,
//     tx = rx + 2 ax): the four taps of a class read one pixel lattice at offsets (ay, ax), so the 64 lattice rows of a K step need
//     ONE input patch of (rows + 1) x (OW + 1) pixels (81..130 pixels instead of 4 x 64 gathered rows) and ONE 64 x 128 tile of P
//     for 4 x 2 x 64 x 128 x 128 FLOP: 200+ FLOP per staged byte instead of 64;
//   * 8 waves: wave w owns tap w / 2 and output-channel half w % 2 -> 64 x 128 accumulators (32 MFMA tiles), 64 MFMAs per wave and
//     barrier; both operands are K-major in memory, fragments come from `ds_read_b64_tr_b16` (transposed LDS reads);
//   * both operands staged by LDS-DMA (buffer descriptors, 256-byte rows, 32-byte blocks XOR-swizzled on the source side) into a ring
//     of three stages, two K steps in flight behind a counted vmcnt, one barrier per K step.
//
// K loop (software-pipelined, the shape of igemm_nt8s.hip).  A K step is two 32-row halves; the fragments of a half are 16 registers
// of P (af0 / af1, double buffered) and 32 of the patch (bfr[j], column tile j).  Every half walks its MFMAs column tile by column tile:
// the NI MFMAs of column tile j, then the reads of the NEXT half's bfr[j] and of one row tile of its P fragments, then -- in the second
// half -- one DMA piece of the step three ahead with its address arithmetic, then __builtin_amdgcn_sched_barrier(0).  No MFMA waits for
// a read issued in its own group, and nothing but four fragment reads stands in front of an iteration's first MFMA.  The order in which
// an accumulator tile receives its MFMAs (K steps in order, half 0 before half 1, the same operands) is that of the loop this replaced:
// the slabs are bit-identical.
//
//     iteration t, stage st = t % 3:
//       half A   MFMA(step t, half 0)  |  reads (step t, half 1) from stage st
//       s_waitcnt vmcnt(pieces of step t+2) lgkmcnt(0) ; s_barrier
//       half B   MFMA(step t, half 1)  |  reads (step t+1, half 0) from stage (t+1) % 3  |  DMA of step t+3 into stage st
//
// Hazards.  Before the loop steps 0, 1, 2 are issued, step 0 is waited for and published by a barrier, and its half 0 is read.
// RAW: the pieces of step t+1 were issued in iteration t-2 (or the prologue); the only pieces issued after them are those of step t+2,
// so the counted vmcnt in the middle of iteration t has them landed for this wave and the barrier behind it for every wave; the first
// read of step t+1 is in half B of iteration t, behind that barrier (its half 1 is read in half A of iteration t+1).
// WAR: stage st is read for the last time in half A of iteration t (step t, half 1); the lgkmcnt(0) in front of the barrier retires those
// reads in every wave before any wave issues a piece of step t+3 into the stage, in half B behind the barrier.  Stage (t+1) % 3 is
// written next in half B of iteration t+1, behind that iteration's barrier, when its last reads (half A of t+1) are retired the same way.
// Past the last step the reads of half B fetch stale bytes of a valid stage that no MFMA uses (no DMA is in flight then).
// The builtins do not touch memory as far as the optimiser knows: the empty asm statements in publish() keep the reads on their side
// of wait and barrier at IR level, sched_barrier(0) in the machine scheduler; the emitted loop was read against this list.
#include <string.h>
#include <algorithm>

#include "eg_common.h"
#include "igemm_nt.h"

__device__ __forceinline__ void tn8_wait(int n) {        // vmcnt(n) lgkmcnt(0) through the builtin (see igemm_nt8s.hip), n in 0..7
    switch (n) {
        case 0: __builtin_amdgcn_s_waitcnt(0 | (7 << 4)); break;
        case 1: __builtin_amdgcn_s_waitcnt(1 | (7 << 4)); break;
        case 2: __builtin_amdgcn_s_waitcnt(2 | (7 << 4)); break;
        case 3: __builtin_amdgcn_s_waitcnt(3 | (7 << 4)); break;
        case 4: __builtin_amdgcn_s_waitcnt(4 | (7 << 4)); break;
        case 5: __builtin_amdgcn_s_waitcnt(5 | (7 << 4)); break;
        case 6: __builtin_amdgcn_s_waitcnt(6 | (7 << 4)); break;
        default: __builtin_amdgcn_s_waitcnt(7 | (7 << 4)); break;
    }
}
__device__ __forceinline__ void tn8_wait2(int n) {       // the prologue's: two K steps may stay in flight, n = 2 * (0..7)
    switch (n) {
        case 2: __builtin_amdgcn_s_waitcnt(2 | (7 << 4)); break;
        case 4: __builtin_amdgcn_s_waitcnt(4 | (7 << 4)); break;
        case 6: __builtin_amdgcn_s_waitcnt(6 | (7 << 4)); break;
        case 8: __builtin_amdgcn_s_waitcnt(8 | (7 << 4)); break;
        case 10: __builtin_amdgcn_s_waitcnt(10 | (7 << 4)); break;
        case 12: __builtin_amdgcn_s_waitcnt(12 | (7 << 4)); break;
        case 14: __builtin_amdgcn_s_waitcnt(14 | (7 << 4)); break;
        default: __builtin_amdgcn_s_waitcnt(0 | (7 << 4)); break;
    }
}

// CH: channels per tile on both sides (128: the CelebA layers; 64: the dSprites generators; 32: the first trunk layers of the dSprites networks,
// whose 64 x 32 tile of P is four DMA pieces: waves 0..3 issue one each) = 16-bit elements per LDS row
template <typename T, int CH>
__global__ __launch_bounds__(512) void igemm_tn8_kernel(const Tn8Params p) {
    constexpr int ROWB = CH * 2;                         // bytes per LDS row (a K row of P, a patch pixel of X)
    constexpr int RPP = 1024 / ROWB;                     // rows per 1 KiB DMA piece
    constexpr int CPR = ROWB / 16;                       // 16-byte chunks per row
    constexpr int NBLK = ROWB / 32;                      // 32-byte (16-channel) blocks per row: the swizzle unit
    constexpr int NI = CH / 32, NJ = CH / 16;            // MFMA tiles per wave: output channels (half of CH) x input channels
    constexpr int NPP_P = (64 / RPP + 7) / 8;            // P pieces per wave and K step
    constexpr int PW_P = 64 / RPP < 8 ? 64 / RPP : 8;    // waves that issue P pieces
    constexpr int NPP_X = (EG_TN8_XSLOTS / RPP + 7) / 8; // patch pieces per wave and K step, at most (5, 3, 2)
    constexpr int PPG = (NPP_P + NPP_X + NJ - 1) / NJ;   // DMA pieces per MFMA group of the issuing half (1, 1, 2)
    constexpr int STAGE_P = 64 * ROWB, STAGE_X = EG_TN8_XSLOTS * ROWB, STAGE = STAGE_P + STAGE_X;
    static_assert(STAGE % ROWB == 0 && STAGE_P % ROWB == 0, "stage offsets keep the block bits of a row address clear");
    static_assert(NPP_X <= 5 && NPP_P <= 2 && 2 * (NPP_P + NPP_X) <= 14, "piece tables, vmcnt range of tn8_wait");
    extern __shared__ __attribute__((aligned(256))) char smem[];     // (a row address keeps its block bits clear: see xk[])
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tp = wave >> 1, nh = wave & 1;             // this wave's tap of the class and half of the 128 output channels
    const int ay = tp >> 1, ax = tp & 1;
    const int tn_i = blockIdx.x / p.ntc, tc_i = blockIdx.x - tn_i * p.ntc;
    const int n0 = tn_i * CH, c0 = tc_i * CH;
    const int ry = blockIdx.y >> 1, rx = blockIdx.y & 1;  // parity class: taps (ry + 2 ay, rx + 2 ax), source = 2 * lattice + (r - 1)
    const int mbeg = blockIdx.z * p.rows_per_split;
    const int mend = min(p.M, mbeg + p.rows_per_split);
    const int nk = (mend - mbeg) >> 6;
    const int OWm = (1 << p.lOW) - 1, OHm = (1 << p.lOH) - 1;
    const unsigned row_bytes = (unsigned)p.C * 2u;
    const int g = lane >> 4, li = lane & 15, q = li >> 2, pc = li & 3;

    // ---- fragment addresses (loop invariant) ----
    // A lane reads K rows r = 32 kb + 8 g + 4 h + q (kb: 32-row half of the step, h: low / high transposed read).  The 16-channel block
    // `blk` of row r lives at r * ROWB + ((blk ^ key(r)) << 5), key(r) = tn8_fsw(r) mod NBLK.  As rows of P the four r of a lane share
    // one key (bits 0, 1 and 3 of r are q and g & 1): one register per output-channel tile, the four rows are `offset:` immediates.  As
    // patch pixels their keys differ: one register per row with the key folded in, the block of column tile j is one XOR away.
    int pk[NI], xk[4];
    {
        const int r = 8 * g + q, key = tn8_fsw(r) & (NBLK - 1);
#pragma unroll
        for (int i = 0; i < NI; ++i) pk[i] = r * ROWB + ((((nh * NI + i) ^ key) << 5) | (pc << 3));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (i >> 1) * 32 + 8 * g + (i & 1) * 4 + q;
        int img, oy;
        if (p.nimg == 1) { img = 0; oy = r >> p.lOW; }
        else { img = r >> (p.lOH + p.lOW); oy = (r >> p.lOW) & OHm; }
        const int px = (img * p.PH + oy + ay) * p.PW + (r & OWm) + ax;
        xk[i] = STAGE_P + px * ROWB + (((tn8_fsw(px) & (NBLK - 1)) << 5) | (pc << 3));
    }

    // ---- DMA source offsets ----
    const int c16 = lane % CPR, rsub = lane / CPR;       // a piece = RPP rows x ROWB bytes; lane -> (row, 16-byte chunk)
    const u32x4_t srdP = eg_make_srd(p.P, (unsigned)((size_t)p.M * p.N * 2));
    const u32x4_t srdX = eg_make_srd(p.src, (unsigned)((size_t)p.B * p.H * p.W * p.C * 2));
    unsigned vP[NPP_P];
#pragma unroll
    for (int j = 0; j < NPP_P; ++j) {
        const int r = RPP * (wave + 8 * j) + rsub;
        const int src16 = (((c16 >> 1) ^ (tn8_fsw(r) & (NBLK - 1))) << 1) | (c16 & 1);
        vP[j] = (unsigned)r * (unsigned)p.N * 2u + (unsigned)n0 * 2u + (unsigned)src16 * 16u;
    }
    // patch pieces w, w + 8, ...: the lane's source offset relative to (image of the step, source row 2 * first lattice row, column 0)
    // and its source row relative to that row; a pixel slot outside the patch or the image in x gets a row no step can make valid
    int xa[NPP_X], xdy[NPP_X];
#pragma unroll
    for (int j = 0; j < NPP_X; ++j) {
        const unsigned ps = (unsigned)(RPP * (wave + 8 * j) + rsub);
        const unsigned img = (ps * p.inv_plane) >> 20;
        const unsigned rem = ps - img * (unsigned)(p.PH * p.PW);
        const unsigned qy = (rem * p.inv_pw) >> 20, qx = rem - qy * (unsigned)p.PW;
        const int ix = (int)qx * 2 + rx - 1;
        const int src16 = (((c16 >> 1) ^ (tn8_fsw((int)ps) & (NBLK - 1))) << 1) | (c16 & 1);
        const bool ok = (int)ps < p.npix && ix >= 0 && ix < p.W;
        const int dy = (int)qy * 2 + ry - 1;            // source row = 2 * (first lattice row of the step) + dy
        xdy[j] = ok ? dy : 0x40000000;
        xa[j] = (int)(((img * (unsigned)(p.H * p.W) + (unsigned)ix) * row_bytes) + (unsigned)c0 * 2u + (unsigned)src16 * 16u) + dy * p.W * (int)row_bytes;
    }
    const unsigned sm0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned lds0 = sm0 + (unsigned)wave * 1024u;
    const bool p_wave = PW_P == 8 || wave < PW_P;        // this wave issues P pieces
    int nxp = 0;                                         // patch pieces this wave issues per K step (pieces past the patch would land in the next stage)
    for (int j = 0; j < p.npp; ++j) nxp += (wave + 8 * j) * RPP < p.npix;
    const int per = (p_wave ? NPP_P : 0) + nxp;          // pieces this wave issues per K step

    // the DMA of one K step, piece by piece: the step's scalar terms, then piece k = 0 .. NPP_P + NPP_X - 1 (P first)
    struct Step { unsigned base, soffP; int ybase, pixoff; };
    auto step_of = [&](int s, int stage) {
        Step d;
        const int m0s = mbeg + (s << 6);
        d.base = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)stage * STAGE);
        d.soffP = (unsigned)m0s * (unsigned)p.N * 2u;
        const int b_s = m0s >> (p.lOH + p.lOW);
        d.ybase = p.nimg == 1 ? ((m0s >> p.lOW) & OHm) * 2 : 0;
        d.pixoff = (b_s * p.H + d.ybase) * p.W * (int)row_bytes;      // source pixel of (image b_s, row 2 * oy_s, column 0)
        return d;
    };
    auto issue_piece = [&](const Step& d, int k) {       // k is a constant after unrolling
        if (k < NPP_P) {
            if (p_wave) {
                if (k == 0) eg_bufdma1f<0>(srdP, vP[0], d.soffP, d.base);
                if (k == 1) eg_bufdma1f<0x2000>(srdP, vP[NPP_P - 1], d.soffP, d.base);
            }
        } else if (k - NPP_P < NPP_X) {
            const int j = k - NPP_P;
            if (j < nxp) {
                const int jj = j < NPP_X ? j : 0;        // (j itself; keeps the index in range where the compiler cannot see the guard above)
                const unsigned v = (unsigned)(d.ybase + xdy[jj]) < (unsigned)p.H ? (unsigned)(xa[jj] + d.pixoff) : EG_OOB;
                if (j == 0) eg_bufdma1f<STAGE_P>(srdX, v, 0u, d.base);
                if (j == 1) eg_bufdma1f<STAGE_P + 0x2000>(srdX, v, 0u, d.base);
                if (j == 2) eg_bufdma1f<STAGE_P + 0x4000>(srdX, v, 0u, d.base);
                if (j == 3) eg_bufdma1f<STAGE_P + 0x6000>(srdX, v, 0u, d.base);
                if (j == 4) eg_bufdma1f<STAGE_P + 0x8000>(srdX, v, 0u, d.base);
            }
        }
    };

    f32x4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
    auto tr2 = [&](unsigned a_lo, unsigned a_hi) {       // 8 K-consecutive 16-bit elements of one column: two transposed reads (LDS addresses)
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(size_t)a_lo);
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(size_t)a_hi);
        return make_uint4(((uint32_t)(uint16_t)lo[0]) | ((uint32_t)(uint16_t)lo[1] << 16), ((uint32_t)(uint16_t)lo[2]) | ((uint32_t)(uint16_t)lo[3] << 16),
                          ((uint32_t)(uint16_t)hi[0]) | ((uint32_t)(uint16_t)hi[1] << 16), ((uint32_t)(uint16_t)hi[2]) | ((uint32_t)(uint16_t)hi[3] << 16));
    };
    uint4 af0[NI], af1[NI], bfr[NJ];                     // P fragments of the two 32-row halves (double buffered), patch fragments (reloaded column tile by column tile)
    // the counted wait + barrier that publishes a K step.  The empty asm statements pin the fragment reads at IR level: to the optimiser
    // neither builtin touches memory, and a read whose only users sit behind the barrier may otherwise sink past both (the prologue's
    // reads did); sched_barrier(0) pins the machine scheduler.
    auto publish = [&](int n, auto widec) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (decltype(widec)::value) tn8_wait2(n);
        else tn8_wait(n);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    // one half of a K step, column tile by column tile: the NI MFMAs of column tile j on the fragments in registers, then the reads of
    // the NEXT half (half `kb` of the stage at byte offset `soff`) -- bfr[j] into the registers those MFMAs have just released, one row
    // tile of `na` per group -- then, in the issuing half, PPG DMA pieces of the step `d` describes.
    auto half = [&](const uint4 (&ca)[NI], uint4 (&na)[NI], int soff, auto kbc, auto dmc, const Step& d, bool dm) {
        constexpr int kb = decltype(kbc)::value;
        constexpr bool DM = decltype(dmc)::value;
        const unsigned sb = sm0 + (unsigned)soff, sp = sb + kb * 32 * ROWB;      // (xk[] holds the rows of both halves, pk[] those of half 0)
        const unsigned x_lo = sb + (unsigned)xk[2 * kb], x_hi = sb + (unsigned)xk[2 * kb + 1];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                if constexpr (std::is_same<T, f16_t>::value)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, ca[i]), __builtin_bit_cast(f16x8_t, bfr[j]), acc[i][j], 0, 0, 0);
                else
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ca[i]), __builtin_bit_cast(bf16x8_t, bfr[j]), acc[i][j], 0, 0, 0);
            }
            bfr[j] = tr2(x_lo ^ (unsigned)(j << 5), x_hi ^ (unsigned)(j << 5));
            if (j < NI) na[j] = tr2(sp + (unsigned)pk[j], sp + (unsigned)pk[j] + 4 * ROWB);
            if constexpr (DM) {
                if (dm) {
#pragma unroll
                    for (int k = j * PPG; k < (j + 1) * PPG; ++k) issue_piece(d, k);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // ring: K step s lives in stage s % 3.  Prologue: steps 0, 1, 2 in flight, step 0 landed and published, its first half in registers.
    const int npro = min(nk, 3);
    for (int s = 0; s < npro; ++s) {
        const Step d = step_of(s, s);
#pragma unroll
        for (int k = 0; k < NPP_P + NPP_X; ++k) issue_piece(d, k);
    }
    publish(per * max(npro - 1, 0), std::true_type{});
    {
        const unsigned x_lo = sm0 + (unsigned)xk[0], x_hi = sm0 + (unsigned)xk[1];
#pragma unroll
        for (int j = 0; j < NJ; ++j) bfr[j] = tr2(x_lo ^ (unsigned)(j << 5), x_hi ^ (unsigned)(j << 5));
#pragma unroll
        for (int i = 0; i < NI; ++i) af0[i] = tr2(sm0 + (unsigned)pk[i], sm0 + (unsigned)pk[i] + 4 * ROWB);
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xc07f);                  // lgkmcnt(0) alone: the loop's own waits then count the loop's reads only
    __builtin_amdgcn_sched_barrier(0);
    int st = 0;
    for (int t = 0; t < nk; ++t) {
        const int st1 = st == 2 ? 0 : st + 1;            // stage of K step t + 1
        const bool dm = t + 3 < nk;
        const Step d = step_of(t + 3, st);               // K step t + 3 goes where K step t is
        // half 0 of step t | reads of its half 1
        half(af0, af1, st * STAGE, std::integral_constant<int, 1>{}, std::false_type{}, d, false);
        // K step t + 1 has landed (everything but the pieces of step t + 2); this wave's reads of stage st are retired
        publish(t + 2 < nk ? per : 0, std::false_type{});
        // half 1 of step t | reads of half 0 of step t + 1 (past the last step: stale bytes of a valid stage that nobody uses) | DMA
        half(af1, af0, st1 * STAGE, std::integral_constant<int, 0>{}, std::true_type{}, d, dm);
        st = st1;
    }

    // ---- slab[split][n][tap][c] ----
    const int tap = (ry + 2 * ay) * 4 + (rx + 2 * ax);
    float* slab = p.slab + (size_t)blockIdx.z * p.N * 16 * p.C;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + (nh * NI + i) * 16 + g * 4 + r;
            float* row = slab + ((size_t)n * 16 + tap) * p.C + c0 + li;
#pragma unroll
            for (int j = 0; j < NJ; ++j) row[j * 16] = acc[i][j][r];
        }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// geometry + split plan; false if this convolution is not a 16-bit 4x4 / stride-2 / pad-1 layer of the supported sizes
bool eg_tn8_plan(const eg_conv* c, int dtype, Tn8Params& p, int* nsplit, int wgs_target) {
    if (dtype == EG_F32 || c->k != 4 || c->stride != 2 || c->pad != 1 || c->up != 0) return false;
    const int ch = ((c->Cin % 128) == 0 && (c->Cout % 128) == 0) ? 128 : (((c->Cin % 64) == 0 && (c->Cout % 64) == 0) ? 64
                   : (((c->Cin % 32) == 0 && (c->Cout % 32) == 0) ? 32 : 0));
    if (ch == 0 || (c->H & 1) || (c->W & 1)) return false;
    const int OH = c->H / 2, OW = c->W / 2;
    const int lOH = ilog2_exact(OH), lOW = ilog2_exact(OW);
    const long long M = (long long)c->B * OH * OW;
    if (lOH < 0 || lOW < 0 || OW > 64 || (M % 64) != 0) return false;
    if ((size_t)c->B * c->H * c->W * c->Cin * 2 >= 0x7fffffffull || (size_t)M * c->Cout * 2 >= 0x7fffffffull) return false;
    memset(&p, 0, sizeof(p));
    p.B = c->B; p.H = c->H; p.W = c->W; p.C = c->Cin; p.N = c->Cout;
    p.lOH = lOH; p.lOW = lOW; p.M = (int)M;
    if (OH * OW >= 64) { p.nimg = 1; p.OHt = 64 / OW; }
    else { p.nimg = 64 / (OH * OW); p.OHt = OH; }
    p.PH = p.OHt + 1; p.PW = OW + 1;
    p.npix = p.nimg * p.PH * p.PW;
    p.ch = ch;
    const int rpp = 1024 / (ch * 2);                    // patch pixels per DMA piece
    if ((p.npix + rpp - 1) / rpp * rpp > EG_TN8_XSLOTS) return false;      // (whole pieces land in the stage)
    p.npp = ((p.npix + rpp - 1) / rpp + 7) / 8;
    if (p.npp > 5) return false;
    p.inv_pw = (1u << 20) / (unsigned)p.PW + 1;
    p.inv_plane = (1u << 20) / (unsigned)(p.PH * p.PW) + 1;
    for (unsigned x = 0; x < 512; ++x)
        if (((x * p.inv_pw) >> 20) != x / (unsigned)p.PW || ((x * p.inv_plane) >> 20) != x / (unsigned)(p.PH * p.PW)) return false;
    p.ntn = c->Cout / ch; p.ntc = c->Cin / ch;
    // one workgroup per CU (150 KiB of LDS): split m until about 256 workgroups exist, at least 4 K steps each
    const long long base = (long long)p.ntn * p.ntc * 4;
    // (wgs_target: the caller's share of the chip -- a launch forked beside the main chain's GEMMs runs the step fastest at 128: half the
    //  slab bytes to write and reduce, and the other CUs stay with the main chain; profiles/r02_i_ab_tn8_target.txt)
    // (never above the whole-chip 256 that eg_conv_wgrad_ws_bytes sizes the slab for: the split count grows with the target)
    const int target = wgs_target > 0 ? std::min(wgs_target, 256) : 256;
    long long want = base >= target ? 1 : (target + base - 1) / base;
    const long long steps = M / 64;
    want = std::min(want, std::max(1LL, steps / 4));
    const long long sps = (steps + want - 1) / want;    // K steps per split
    p.rows_per_split = (int)(sps * 64);
    *nsplit = (int)((steps + sps - 1) / sps);
    return true;
}

template <typename T, int CH>
static void launch_tn8_ch(const Tn8Params& p, int nsplit, hipStream_t st) {
    constexpr size_t lds = 3 * (size_t)(64 + EG_TN8_XSLOTS) * CH * 2;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&igemm_tn8_kernel<T, CH>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((igemm_tn8_kernel<T, CH>), dim3(p.ntn * p.ntc, 4, nsplit), dim3(512), lds, st, p);
}

template <typename T>
void eg_launch_tn8(const Tn8Params& p, int nsplit, hipStream_t st) {
    if (p.ch == 32) launch_tn8_ch<T, 32>(p, nsplit, st);
    else if (p.ch == 64) launch_tn8_ch<T, 64>(p, nsplit, st);
    else launch_tn8_ch<T, 128>(p, nsplit, st);
}
template void eg_launch_tn8<bf16_t>(const Tn8Params&, int, hipStream_t);
template void eg_launch_tn8<f16_t>(const Tn8Params&, int, hipStream_t);
