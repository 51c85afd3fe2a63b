// Implicit-GEMM convolution family for gfx950 (MFMA, 64-wide waves, LDS-staged 128-byte K rows).
//
//   igemm_nt : C[m][n] = sum_k A[m][k] * Wp[n][k]       A rows gathered from an NHWC tensor
//              (conv forward, conv backward-data == ConvTranspose forward, linear)
//
// This file: the 4-wave NT kernels, the planner that chooses among them and the 8-wave kernels (igemm_nt8s.hip, igemm_nt8h.hip), and the
// entry points.  Weight packing is pack.hip, the weight gradient igemm_tn.hip / igemm_tn8.hip, its reductions grad_reduce.hip.
//
// It runs in fp32 (v_mfma_f32_16x16x4_f32, exact fp32) or bf16 (v_mfma_f32_16x16x32_bf16, fp32
// accumulate).  K rows in LDS are always 128 bytes (32 fp32 / 64 bf16) and XOR-swizzled in 16-byte
// chunks so that ds_read_b128 fragment reads are bank-conflict free without padding.
#include <algorithm>
#include <vector>
#include <type_traits>

#include "eg_common.h"
#include "igemm_nt.h"
#include "conv_geom.h"

// This file is compiled with -ffp-contract=off (Makefile): every NT variant must round the epilogue (acc / sigma + bias) alike -- the
// variants are tested bit for bit against each other -- and clang contracts `a * b + c` depending on where the operands come from.

// ------------------------------------------------------------------------------------------------
// igemm_nt
// ------------------------------------------------------------------------------------------------
// STAT: the epilogue with column statistics (eg_epilogue.stat_mode; 16-bit types, whole 128-row tiles, ONE column tile: N == BN) -- the
// small networks' 32- and 64-channel layers, whose BatchNorm / bias-gradient reductions were 2-3 extra launches per layer on a chain
// that is launch-bound end to end
// SPLITK: blockIdx.z = phase * nsplit + split; every workgroup runs a slice of the K loop, the last of a tile's workgroups to arrive adds
// the fp32 partial tiles in split order (its own from registers) and runs the epilogue (protocol and comments: igemm_nt8s.hip).  For the
// small networks' few-row / deep-K launches (a 4 x 4 output map: 16-48 tiles on 256 CUs, 16 dependent K steps of ~1.4 us each).
template <typename T, int BM, int BN, int WGM, int WGN, bool STAT = false, bool SPLITK = false>
__global__ __launch_bounds__(256) void igemm_nt_kernel(const NtParams p) {
    constexpr int VEC = Elt<T>::VEC;
    constexpr int BK = 8 * VEC;
    constexpr int TM = BM / WGM / 16, TN = BN / WGN / 16;
    constexpr int A_LD = BM / 32;
    constexpr int B_LD = (BN + 31) / 32;
    constexpr int STAGE = (BM + BN) * 128;
    static_assert(WGM * WGN == 4, "4 waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int nsplit = SPLITK && p.nsplit > 1 ? p.nsplit : 1;
    const int phase = blockIdx.z / nsplit, split = blockIdx.z - phase * nsplit;
    const NtPhase ph = p.ph[phase];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int chunk = tid & 7, rbase = tid >> 3;
    const int OWm = (1 << p.lOW) - 1, OHm = (1 << p.lOH) - 1;
    const int HU = p.H << p.up, WU = p.W << p.up;

    // per-thread A rows
    int a_pix0[A_LD];   // b*H*W (pixel base of the image) or -1 when the row is out of range
    int a_y[A_LD], a_x[A_LD];
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
        const int m = m0 + rbase + 32 * i;
        const int b = m >> (p.lOW + p.lOH);
        a_pix0[i] = (m < p.M) ? b * p.H * p.W : -1;
        a_y[i] = ((m >> p.lOW) & OHm) * p.sy + ph.dy0;
        a_x[i] = (m & OWm) * p.sx + ph.dx0;
    }
    const T* __restrict__ src = reinterpret_cast<const T*>(p.src);
    const T* __restrict__ wp = reinterpret_cast<const T*>(p.wp) + ph.w_off;
    const int nk_all = ph.Kpad / BK;
    const int per = (nk_all + nsplit - 1) / nsplit;
    const int kt0 = split * per;
    const int nk = max(0, min(per, nk_all - kt0));
    // tap state of this thread's 16-byte chunk at K tile kt0
    int kc = kt0 * BK + chunk * VEC, ty = 0, tx = 0;
    if (kc >= p.C) {
        const int tap = kc / p.C;
        kc -= tap * p.C;
        ty = tap / ph.TW;
        tx = tap - ty * ph.TW;
    }

    uint4 ra[A_LD], rb[B_LD];
    auto gload = [&](int kt) {
        const bool tap_ok = ty < ph.TH;
        const int oy = ty * ph.dys, ox = tx * ph.dxs;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int iy = a_y[i] + oy, ix = a_x[i] + ox;
            const bool ok = tap_ok && a_pix0[i] >= 0 && iy >= 0 && iy < HU && ix >= 0 && ix < WU;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ok) {
                const size_t pix = (size_t)a_pix0[i] + (size_t)((iy >> p.up) * p.W + (ix >> p.up));
                v = *reinterpret_cast<const uint4*>(src + pix * p.C + kc);
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int r = rbase + 32 * i;
            const int n = n0 + r;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r < BN && n < p.N) v = *reinterpret_cast<const uint4*>(wp + (size_t)n * ph.Kpad + (size_t)kt * BK + chunk * VEC);
            rb[i] = v;
        }
        kc += BK;
        while (kc >= p.C) { kc -= p.C; if (++tx == ph.TW) { tx = 0; ++ty; } }
    };
    auto lstore = [&](int stage) {
        char* sa = smem + stage * STAGE;
        char* sb = sa + BM * 128;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) *reinterpret_cast<uint4*>(sa + lds_off(rbase + 32 * i, chunk)) = ra[i];
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int r = rbase + 32 * i;
            if (r < BN) *reinterpret_cast<uint4*>(sb + lds_off(r, chunk)) = rb[i];
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4;
    if (nk > 0) {
        gload(kt0);
        lstore(0);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) gload(kt0 + kt + 1);
        const char* sa = smem + (kt & 1) * STAGE;
        const char* sb = sa + BM * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const uint4*>(sa + lds_off((wm * TM + i) * 16 + frow, ks * 4 + fq));
#pragma unroll
            for (int j = 0; j < TN; ++j) bfr[j] = *reinterpret_cast<const uint4*>(sb + lds_off((wn * TN + j) * 16 + frow, ks * 4 + fq));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) mfma_step<T>(af[i], bfr[j], acc[i][j]);
        }
        if (kt + 1 < nk) lstore((kt + 1) & 1);
        __syncthreads();
    }

    if (SPLITK && nsplit > 1) {
        const int nphase = gridDim.z / nsplit;
        const size_t Mpad = (size_t)gridDim.x * BM;
        const size_t slab = (size_t)nphase * Mpad * p.N;
        float* part = p.part + ((size_t)phase * Mpad + m0) * p.N + n0;
        float* mine = part + (size_t)split * slab;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = (wm * TM + i) * 16 + frow;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                float* a = mine + (size_t)row * p.N + (wn * TN + j) * 16 + fq * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) __hip_atomic_store(a + r, acc[i][j][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // written through
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        unsigned* cnt = p.split_cnt + ((size_t)phase * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        volatile unsigned* flag = reinterpret_cast<volatile unsigned*>(smem);
        if (tid == 0) flag[0] = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (flag[0] != (unsigned)(nsplit - 1)) return;
        if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        f32x4 sum[TM][TN];
        for (int s = 0; s < nsplit; ++s) {             // uniform; own partial from registers: the order does not depend on who is last
            if (s == split) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) sum[i][j] = s == 0 ? acc[i][j] : sum[i][j] + acc[i][j];
                continue;
            }
            const float* other = part + (size_t)s * slab;
            f32x4 ld[TM][TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = (wm * TM + i) * 16 + frow;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const float* a = other + (size_t)row * p.N + (wn * TN + j) * 16 + fq * 4;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ld[i][j][r] = __hip_atomic_load(a + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) sum[i][j] = s == 0 ? ld[i][j] : sum[i][j] + ld[i][j];
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = sum[i][j];
        __syncthreads();
    }

    // ---- epilogue ----
    // acc[i][j][r] = C[m = m0 + (wm*TM+i)*16 + frow][n = n0 + (wn*TN+j)*16 + fq*4 + r]
    if (STAT || (p.out_mode == EG_OUT_NHWC && (p.N % VEC) == 0)) {
        // the shared epilogue through LDS
        NtEpiPre<T, TM, TN, 0> epi;
        nt_epi_fetch_reg(epi, p, m0 + wm * TM * 16 + frow, n0 + wn * TN * 16 + fq * 4);
        if constexpr (STAT)
            nt_epilogue_lds_stat<T, BM, BN, TM, TN, 256, 0>(epi, p, ph, acc, smem, m0, n0, wm * TM * 16, wn * TN * 16, tid, frow, fq,
                                                            phase * gridDim.x + blockIdx.x, 0, 1);
        else nt_epilogue_lds_reg<T, BM, BN, TM, TN, 256>(epi, p, ph, acc, smem, m0, n0, wm * TM * 16, wn * TN * 16, tid, frow, fq);
        return;
    }
    // scalar path: NCHW fp32 image outputs (N = 1..4) and channel counts that are not a multiple of the vector width
    const EgActFast af = eg_act_fast(p.act, p.slope);
    const EgGradFast gf = eg_grad_fast(p.mask_act, p.mask_slope);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + (wm * TM + i) * 16 + frow;
        if (m >= p.M) continue;
        const float inv_sigma = nt_inv_sigma(p, nt_sigma_at(p, m));
        const NtPix px = nt_out_byx(p, m, ph.ooy, ph.oox);
        const size_t pix = nt_pix_index(p, px);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + (wn * TN + j) * 16 + fq * 4 + r;
                if (n >= p.N) continue;
                float v = nt_epi_finish(acc[i][j][r], inv_sigma, p.bias != nullptr, nt_bias_at(p, n), p, af);
                if (p.out_mode == EG_OUT_NHWC) {
                    const size_t o = pix * p.N + n;
                    if (p.mask) nt_epi_mask<T, 1>(&v, reinterpret_cast<const T*>(p.mask) + o, p, gf);
                    nt_epi_store<T, 1>(reinterpret_cast<T*>(p.dst) + o, &v);
                } else {
                    const size_t o = (((size_t)px.b * p.N + n) * p.DH + px.y) * p.DW + px.x;
                    if (p.mask) nt_epi_mask<float, 1>(&v, reinterpret_cast<const float*>(p.mask) + o, p, gf);
                    nt_epi_store<float, 1>(reinterpret_cast<float*>(p.dst) + o, &v);
                }
            }
        }
    }
}


// ------------------------------------------------------------------------------------------------
// igemm_nt_buf: 128x128 tile, 2-stage LDS-DMA ring like igemm_nt_dma<.,128,2>, but the gather goes through buffer descriptors
// (`buffer_load_dwordx4 ... offen lds`): the per-lane part of every address is a 32-bit byte offset that only changes when the
// K loop moves to the next filter tap, the walk along the channels of a tap is the instruction's SGPR offset, and padded /
// out-of-range rows carry an offset beyond num_records (the hardware range check returns zeros) -> no branches, no 64-bit
// address math and no EXEC juggling in the K loop.  Needs C % BK == 0 (every lane of a K step sits in the same tap) and
// tensors below 2 GiB; the dispatcher falls back to igemm_nt_dma otherwise.
// ------------------------------------------------------------------------------------------------
template <typename T, bool PROF = false, bool SPLITK = false>   // SPLITK: its own instantiation so that profilers list the split launches apart
__global__ __launch_bounds__(256) void igemm_nt_buf_kernel(const NtParams p, unsigned long long* prof = nullptr) {
    unsigned long long t_begin = 0, t_wait = 0, t_issue = 0, t_comp = 0, t0 = 0, t1 = 0;
    if (PROF) t_begin = __builtin_amdgcn_s_memtime();
    constexpr int VEC = Elt<T>::VEC;
    constexpr int BK = 8 * VEC;
    constexpr int BM = 128, BN = 128;
    constexpr int STAGE = (BM + BN) * 128;
    constexpr int TM = 4, TN = 4;                  // waves 2 x 2, wave tile 64 x 64
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int nsplit = SPLITK && p.nsplit > 1 ? p.nsplit : 1;
    const int phase = blockIdx.z / nsplit, split = blockIdx.z - phase * nsplit;
    const NtPhase ph = p.ph[phase];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    // XCD-aware tile order: workgroup ids go round robin over the 8 XCDs (each with its own L2), so neighbouring M tiles -- which share input
    // halo rows in an implicit convolution -- would sit on different L2s.  With gridDim.x a multiple of 8, XCD c takes tiles [c, c+1) * gridDim.x / 8.
    const int bx = (p.xcd_remap && (gridDim.x & 7) == 0) ? (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int m0 = bx * BM, n0 = blockIdx.y * BN;
    const int OWm = (1 << p.lOW) - 1, OHm = (1 << p.lOH) - 1;
    const int HU = p.H << p.up, WU = p.W << p.up;
    const int rsub = lane >> 3, pos = lane & 7;
    const int srcchunk = pos ^ ((((wave & 1) << 2) + (lane >> 4)) & 7);

    int a_pix0[4], a_y[4], a_x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + (j * 4 + wave) * 8 + rsub;
        const int b = m >> (p.lOW + p.lOH);
        a_pix0[j] = (m < p.M) ? b * p.H * p.W : -1;
        a_y[j] = ((m >> p.lOW) & OHm) * p.sy + ph.dy0;
        a_x[j] = (m & OWm) * p.sx + ph.dx0;
    }
    const unsigned row_bytes = (unsigned)p.C * sizeof(T);
    unsigned va[4], vb[4];
    auto tap_offsets = [&](int ty, int tx) {
        const int oy = ty * ph.dys, ox = tx * ph.dxs;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int iy = a_y[j] + oy, ix = a_x[j] + ox;
            const bool ok = a_pix0[j] >= 0 && iy >= 0 && iy < HU && ix >= 0 && ix < WU;
            const unsigned pix = (unsigned)(a_pix0[j] + (iy >> p.up) * p.W + (ix >> p.up));
            va[j] = ok ? pix * row_bytes + (unsigned)srcchunk * 16u : EG_OOB;
        }
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + (j * 4 + wave) * 8 + rsub;
        vb[j] = n < p.N ? (unsigned)n * (unsigned)ph.Kpad * (unsigned)sizeof(T) + (unsigned)srcchunk * 16u : EG_OOB;
    }
    const u32x4_t srdA = eg_make_srd(p.src, (unsigned)((size_t)p.B * p.H * p.W * p.C * sizeof(T)));
    const u32x4_t srdB = eg_make_srd(reinterpret_cast<const T*>(p.wp) + ph.w_off, (unsigned)((size_t)p.N * ph.Kpad * sizeof(T)));
    // this block's K steps [kt0, kt0 + nk)
    const int nk_all = ph.Kpad / BK;
    const int per = (nk_all + nsplit - 1) / nsplit;
    const int kt0 = split * per;
    const int nk = min(per, nk_all - kt0);

    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem + (unsigned)wave * 1024u;
    // wave-uniform walk over (tap, channel block)
    const int steps_per_tap = p.C / BK;
    const int tap0 = kt0 / steps_per_tap;
    int ty = tap0 / ph.TW, tx = tap0 - ty * ph.TW;
    unsigned kc_bytes = (unsigned)(kt0 - tap0 * steps_per_tap) * 128u;
    if (ty < ph.TH) tap_offsets(ty, tx);
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j) va[j] = EG_OOB;
    }
    auto issue = [&](int kt, int stage) {
        const unsigned sa = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)stage * STAGE);
        // four 1-KiB pieces each (tile rows (j*4+wave)*8 .. +7, j = 0..3): LDS bases sa, sa+4K, sa+8K, sa+12K
        eg_bufdma4s<0x1000>(srdA, va[0], va[1], va[2], va[3], kc_bytes, sa);
        eg_bufdma4s<0x1000>(srdB, vb[0], vb[1], vb[2], vb[3], (unsigned)(kt0 + kt) * 128u, sa + BM * 128);
        kc_bytes += 128u;
        if (kc_bytes >= row_bytes) {               // next tap (uniform branch)
            kc_bytes = 0;
            if (++tx == ph.TW) { tx = 0; ++ty; }
            if (ty < ph.TH) tap_offsets(ty, tx);
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) va[j] = EG_OOB;     // K padding beyond the last tap
            }
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4;
    auto compute = [&](int stage) {
        const char* sa = smem + stage * STAGE;
        const char* sb = sa + BM * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 bfr[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) bfr[j] = *reinterpret_cast<const uint4*>(sb + lds_off((wn * TN + j) * 16 + frow, ks * 4 + fq));
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const uint4 af = *reinterpret_cast<const uint4*>(sa + lds_off((wm * TM + i) * 16 + frow, ks * 4 + fq));
#pragma unroll
                for (int j = 0; j < TN; ++j) mfma_step<T>(af, bfr[j], acc[i][j]);
            }
        }
    };
    if (nk > 0) issue(0, 0);
    for (int kt = 0; kt + 1 < nk; ++kt) {
        if (PROF) t0 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                 // everyone's stage kt landed; everyone finished reading stage kt-1
        __builtin_amdgcn_sched_barrier(0);
        if (PROF) { t1 = __builtin_amdgcn_s_memtime(); t_wait += t1 - t0; }
        issue(kt + 1, (kt + 1) & 1);
        if (PROF) { __builtin_amdgcn_sched_barrier(0); t0 = __builtin_amdgcn_s_memtime(); t_issue += t0 - t1; __builtin_amdgcn_sched_barrier(0); }
        compute(kt & 1);
        if (PROF) { __builtin_amdgcn_sched_barrier(0); t1 = __builtin_amdgcn_s_memtime(); t_comp += t1 - t0; __builtin_amdgcn_sched_barrier(0); }
    }
    // last K step: nothing left to issue -> fetch the epilogue operands instead, their latency hides behind the MFMAs
    constexpr int PF = 8;
    NtEpiPre<T, TM, TN, PF> epi;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (nsplit == 1) nt_epi_prefetch<T, BM, BN, TM, TN, 256, PF>(epi, p, ph, m0, n0, wm * TM * 16, wn * TN * 16, tid, frow, fq);
    if (nk > 0) compute((nk - 1) & 1);
    if (PROF) t0 = __builtin_amdgcn_s_memtime();
    if (nsplit > 1) {
        // raw fp32 partial tile; nt_splitk_epilogue_kernel sums the splits and applies the epilogue
        const int nphase = gridDim.z / nsplit;
        float* part = p.part + ((size_t)(split * nphase + phase) * (gridDim.x * BM) + m0) * p.N + n0;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = (wm * TM + i) * 16 + frow;
#pragma unroll
            for (int j = 0; j < TN; ++j)
                *reinterpret_cast<f32x4*>(part + (size_t)row * p.N + (wn * TN + j) * 16 + fq * 4) = acc[i][j];
        }
        return;
    }
    __syncthreads();
    nt_epilogue_lds_pre<T, BM, BN, TM, TN, 256, PF>(epi, p, ph, acc, smem, m0, n0, wm * TM * 16, wn * TN * 16, tid, frow, fq);
    if (PROF && lane == 0) {
        t1 = __builtin_amdgcn_s_memtime();
        unsigned long long* o = prof + ((size_t)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 4 + wave) * 8;
        o[0] = t1 - t_begin; o[1] = t_wait; o[2] = t_issue; o[3] = t_comp; o[4] = t1 - t0; o[5] = t_begin; o[6] = t1; o[7] = 0;
    }
}

// ------------------------------------------------------------------------------------------------
// igemm_nt_pers: the 128x128 buffer-descriptor kernel as a persistent pipeline.  A workgroup walks tiles t = blockIdx.x, +gridDim.x, ...
// with ONE continuous 2-stage LDS-DMA ring: the first K step of the next tile is in flight while the last step of the current tile is
// computed, the epilogue operands (1/sigma, bias, activation-gradient mask in accumulator layout) are fetched during that last step,
// and the results leave straight from the accumulators as 8/16-byte stores that nobody waits for -- no LDS staging, no barriers and no
// idle MFMA pipe at tile seams (in igemm_nt_buf the epilogue of every workgroup ran at the same time and cost 15-45 % of a launch).
// vmcnt discipline: the epilogue's TM*TN stores are the wave's youngest operations when the next step's DMA must have landed, so that
// wait is vmcnt(TM*TN) (vmcnt(0) for ragged tiles, where waves may skip stores).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256, 2) void igemm_nt_pers_kernel(const NtParams p, int tiles_m, int tiles_n, int ntiles) {
    constexpr int VEC = Elt<T>::VEC;
    constexpr int BK = 8 * VEC;
    constexpr int BM = 128, BN = 128;
    constexpr int STAGE = (BM + BN) * 128;
    constexpr int TM = 4, TN = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int OWm = (1 << p.lOW) - 1, OHm = (1 << p.lOH) - 1;
    const int HU = p.H << p.up, WU = p.W << p.up;
    const int rsub = lane >> 3, pos = lane & 7;
    const int srcchunk = pos ^ ((((wave & 1) << 2) + (lane >> 4)) & 7);
    const int frow = lane & 15, fq = lane >> 4;
    const unsigned row_bytes = (unsigned)p.C * sizeof(T);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem + (unsigned)wave * 1024u;
    const u32x4_t srdA = eg_make_srd(p.src, (unsigned)((size_t)p.B * p.H * p.W * p.C * sizeof(T)));

    // ---- load side: the tile whose K steps are being issued ----
    int lt = blockIdx.x, lkt = 0, lnk = 0;
    int l_dys = 0, l_dxs = 0, l_TW = 1, l_TH = 0;
    int a_pix0[4], a_y[4], a_x[4];
    unsigned va[4], vb[4];
    u32x4_t srdB = srdA;
    int ty = 0, tx = 0;
    unsigned kc_bytes = 0;
    auto tap_offsets = [&]() {
        const int oy = ty * l_dys, ox = tx * l_dxs;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int iy = a_y[j] + oy, ix = a_x[j] + ox;
            const bool ok = ty < l_TH && a_pix0[j] >= 0 && iy >= 0 && iy < HU && ix >= 0 && ix < WU;
            const unsigned pix = (unsigned)(a_pix0[j] + (iy >> p.up) * p.W + (ix >> p.up));
            va[j] = ok ? pix * row_bytes + (unsigned)srcchunk * 16u : EG_OOB;
        }
    };
    auto setup_load = [&]() {
        const int mt = lt % tiles_m, q = lt / tiles_m;
        const int nt = q % tiles_n, phase = q / tiles_n;
        const NtPhase& ph = p.ph[phase];
        const int m0 = mt * BM, n0 = nt * BN;
        l_dys = ph.dys; l_dxs = ph.dxs; l_TW = ph.TW; l_TH = ph.TH;
        lnk = ph.Kpad / BK;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + (j * 4 + wave) * 8 + rsub;
            const int b = m >> (p.lOW + p.lOH);
            a_pix0[j] = (m < p.M) ? b * p.H * p.W : -1;
            a_y[j] = ((m >> p.lOW) & OHm) * p.sy + ph.dy0;
            a_x[j] = (m & OWm) * p.sx + ph.dx0;
            const int n = n0 + (j * 4 + wave) * 8 + rsub;
            vb[j] = n < p.N ? (unsigned)n * (unsigned)ph.Kpad * (unsigned)sizeof(T) + (unsigned)srcchunk * 16u : EG_OOB;
        }
        srdB = eg_make_srd(reinterpret_cast<const T*>(p.wp) + ph.w_off, (unsigned)((size_t)p.N * ph.Kpad * sizeof(T)));
        ty = 0; tx = 0; kc_bytes = 0; lkt = 0;
        tap_offsets();
    };
    // K step lkt of tile lt -> LDS stage: 8 pieces (A slots 0..3, B slots 0..3), issued in one burst right after the barrier (spreading
    // them between the MFMA groups of the step was measured 8 % slower)
    auto issue_piece = [&](int q, int stage) {
        const unsigned sa = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)stage * STAGE);
        // (single-tap launches whose row is not a whole number of K tiles: chunks past the end of the row read as zeros)
        if (q < 4) eg_bufdma1s(srdA, kc_bytes + (unsigned)srcchunk * 16u < row_bytes ? va[q] : EG_OOB, kc_bytes, sa + q * 0x1000);
        else eg_bufdma1s(srdB, vb[q - 4], (unsigned)lkt * 128u, sa + BM * 128 + (q - 4) * 0x1000);
    };
    auto issue_advance = [&]() {
        ++lkt;
        kc_bytes += 128u;
        if (kc_bytes >= row_bytes) {               // next tap (uniform branch)
            kc_bytes = 0;
            if (++tx == l_TW) { tx = 0; ++ty; }
            tap_offsets();
        }
    };

    // ---- compute side: the tile whose accumulators are live ----
    int ct = blockIdx.x, ckt = 0, cnk = 0, c_m0 = 0, c_n0 = 0, c_ooy = 0, c_oox = 0;
    auto setup_comp = [&]() {
        const int mt = ct % tiles_m, q = ct / tiles_m;
        const int nt = q % tiles_n, phase = q / tiles_n;
        c_m0 = mt * BM; c_n0 = nt * BN;
        c_ooy = p.ph[phase].ooy; c_oox = p.ph[phase].oox;
        cnk = p.ph[phase].Kpad / BK;
        ckt = 0;
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (lt < ntiles) {
        setup_load();
#pragma unroll
        for (int q = 0; q < 8; ++q) issue_piece(q, 0);
        issue_advance();
    }
    if (ct < ntiles) setup_comp();
    unsigned g = 0;                                   // global K step: LDS stage = g & 1
    bool stores_pending = false;
    const T* __restrict__ maskp = reinterpret_cast<const T*>(p.mask);
    typedef NtVec<T, 4> OutVec;                       // 4 outputs of one accumulator

    while (ct < ntiles) {
        if (stores_pending) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                 // everyone's stage g landed; everyone finished reading stage g-1
        __builtin_amdgcn_sched_barrier(0);
        stores_pending = false;
        if (lkt == lnk) {                             // load side moves on to this workgroup's next tile
            lt += gridDim.x;
            if (lt < ntiles) setup_load();
        }
        if (lt < ntiles) {
#pragma unroll
            for (int q = 0; q < 8; ++q) issue_piece(q, (g + 1) & 1);
            issue_advance();
        }
        const bool last = ckt + 1 == cnk;
        // epilogue operands in accumulator layout, fetched under the last MFMA block of the tile
        float e_sigma[TM], e_bias[TN][4];
        OutVec e_mask[TM][TN];
        size_t e_off[TM];
        bool e_ok[TM];
        if (last) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = c_m0 + (wm * TM + i) * 16 + frow;
                e_ok[i] = m < p.M;
                const int mc = min(m, p.M - 1);
                e_sigma[i] = nt_sigma_at(p, mc);
                e_off[i] = nt_out_off(p, mc, c_ooy, c_oox, c_n0) + wn * 64 + fq * 4;
            }
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) e_bias[j][r] = nt_bias_at(p, c_n0 + (wn * TN + j) * 16 + fq * 4 + r);
            if (maskp) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) e_mask[i][j] = *reinterpret_cast<const OutVec*>(maskp + e_off[i] + j * 16);
            }
        }
        {
            const char* sa = smem + (g & 1) * STAGE;
            const char* sb = sa + BM * 128;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                uint4 bfr[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) bfr[j] = *reinterpret_cast<const uint4*>(sb + lds_off((wn * TN + j) * 16 + frow, ks * 4 + fq));
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const uint4 af = *reinterpret_cast<const uint4*>(sa + lds_off((wm * TM + i) * 16 + frow, ks * 4 + fq));
#pragma unroll
                    for (int j = 0; j < TN; ++j) mfma_step<T>(af, bfr[j], acc[i][j]);
                }
            }
        }
        ++g;
        if (!last) { ++ckt; continue; }
        // ---- epilogue straight from the accumulators: acc[i][j][r] = C[c_m0 + (wm*TM+i)*16 + frow][c_n0 + (wn*TN+j)*16 + fq*4 + r]
        const EgActFast eaf = eg_act_fast(p.act, p.slope);
        const EgGradFast egf = eg_grad_fast(p.mask_act, p.mask_slope);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float inv_sigma = nt_inv_sigma(p, e_sigma[i]);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                float f[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) f[r] = nt_epi_finish(acc[i][j][r], inv_sigma, p.bias != nullptr, e_bias[j][r], p, eaf);
                if (maskp) nt_epi_mask<T, 4>(f, reinterpret_cast<const T*>(&e_mask[i][j]), p, egf);
                if (e_ok[i]) nt_epi_store<T, 4>(reinterpret_cast<T*>(p.dst) + e_off[i] + j * 16, f);
                acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
        stores_pending = c_m0 + BM <= p.M;            // full tile: every wave issued exactly TM*TN stores
        ct += gridDim.x;
        if (ct < ntiles) setup_comp();
    }
}

// sum of the split-K partial tiles + the fused epilogue (1/sigma, bias, activation, activation-gradient mask), NHWC store.
// blockIdx.y = phase; 32-bit index arithmetic (M * N / VEC < 2^31, checked by the planner's size limits), shifts when N / VEC is a power
// of two (lvpr >= 0), one bias modulo per vector: with 64-bit divisions and a modulo per element this copy was ALU-bound.
template <typename T>
__global__ __launch_bounds__(256) void nt_splitk_epilogue_kernel(const NtParams p, int nphase, int Mpad, int lvpr) {
    constexpr int VEC = Elt<T>::VEC;
    const EgActFast saf = eg_act_fast(p.act, p.slope);
    const EgGradFast sgf = eg_grad_fast(p.mask_act, p.mask_slope);
    const unsigned vpr = p.N / VEC;
    const unsigned total = (unsigned)p.M * vpr;
    const int phase = blockIdx.y;
    const T* __restrict__ mask = reinterpret_cast<const T*>(p.mask);
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const unsigned vc = lvpr >= 0 ? (i & (vpr - 1)) : (i % vpr);
        const int m = (int)(lvpr >= 0 ? (i >> lvpr) : (i / vpr));
        const int n = (int)vc * VEC;
        float f[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) f[q] = 0.f;
        for (int sp = 0; sp < p.nsplit; ++sp) {
            const float* src = p.part + ((size_t)(sp * nphase + phase) * Mpad + m) * p.N + n;
#pragma unroll
            for (int q = 0; q < VEC / 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(src + 4 * q);
                f[4 * q] += v.x; f[4 * q + 1] += v.y; f[4 * q + 2] += v.z; f[4 * q + 3] += v.w;
            }
        }
        const float inv_sigma = nt_inv_sigma(p, nt_sigma_at(p, m));
        const size_t o = nt_out_off(p, m, p.ph[phase].ooy, p.ph[phase].oox, n);
        // bias index of element q: (n + q) % bias_mod; n is a multiple of VEC, so when VEC divides bias_mod it is (n % bias_mod) + q
        const bool bias_vec = p.bias_mod == 0 || (p.bias_mod % VEC) == 0;
        const int nb = p.bias_mod ? n % p.bias_mod : n;
#pragma unroll
        for (int q = 0; q < VEC; ++q)
            f[q] = nt_epi_finish(f[q], inv_sigma, p.bias != nullptr, p.bias ? p.bias[bias_vec ? nb + q : (n + q) % p.bias_mod] : 0.f, p, saf);
        if (mask) {
            const uint4 mv = *reinterpret_cast<const uint4*>(mask + o);
            nt_epi_mask<T, VEC>(f, reinterpret_cast<const T*>(&mv), p, sgf);
        }
        nt_epi_store<T, VEC>(reinterpret_cast<T*>(p.dst) + o, f);
    }
}

// ------------------------------------------------------------------------------------------------
// dispatch.  The planner is a pure function of the problem and of the caller's per-call hints (eg_epilogue.nt_variant / nt_splitk):
// the library keeps no tuning state, so two trainers (or a test and a trainer) in one process cannot interfere.
//   EG_NT_REG     register-staged 128 x {16,32,64,128} tiles: everything (N < 128, NCHW image outputs, ragged channel counts); the
//                 bit-exact reference of the other variants
//   EG_NT_BUF128  128 x 128, 4 waves, 2-stage buffer-descriptor LDS-DMA ring (+ split-K): launches too small for 256-row tiles
//   EG_NT_PERS    persistent 128 x 128 pipeline: the 1-2-step image-side layers
//   EG_NT_S8      igemm_nt8s.hip: 256 x 128 tiles, 8 waves, 3-K-tile ring, one barrier per K tile, register double buffering (+ split-K)
//   EG_NT_S8P     the same with A held in LDS as an input patch shared by the taps of a class
//   EG_NT_S8H     igemm_nt8h.hip: the 8-wave design on 128 x 128 tiles (+ split-K): launches with too few 256-row tiles
// Every call is described once (nt_describe -> NtCall); the launch and the four queries read that description.
// ------------------------------------------------------------------------------------------------
struct NtPlan { int kind, ns; };

// geometry facts every DMA variant needs
struct NtFacts { bool dma_ok, c_tiles; int nk_min, nk_max; long long tiles128; bool half; };
static NtFacts nt_facts(const NtParams& p, int nphase, int vec, size_t esize) {
    NtFacts f{false, false, 1 << 30, 0, 0, esize == 2};
    f.tiles128 = (long long)cdiv(p.M, 128) * cdiv(p.N, 128) * nphase;
    if (p.out_mode != EG_OUT_NHWC || (p.N % 128) != 0 || (p.C % vec) != 0) return f;
    if ((size_t)p.B * p.H * p.W * p.C * esize >= 0x7fffffffull) return f;
    bool single_tap = true;
    for (int i = 0; i < nphase; ++i) {
        if ((size_t)p.N * p.ph[i].Kpad * esize >= 0x7fffffffull) return f;
        f.nk_min = std::min(f.nk_min, p.ph[i].Kpad / (8 * vec));
        f.nk_max = std::max(f.nk_max, p.ph[i].Kpad / (8 * vec));
        single_tap = single_tap && p.ph[i].TH * p.ph[i].TW == 1;
    }
    f.c_tiles = (p.C % (8 * vec)) == 0;              // every lane of a K step sits in the same filter tap
    f.dma_ok = f.c_tiles || single_tap;
    return f;
}

// split count: enough workgroups to reach `target`, at least 8 K steps per split, partial tiles must fit the lent scratch
static int nt_splits(long long wgs, int target, int nk_min, size_t bytes_per_split, size_t ws_bytes, int forced) {
    if (ws_bytes == 0 || bytes_per_split == 0) return 1;
    int ns = 1;
    if (forced > 0) {
        while (ns * 2 <= forced && nk_min / (ns * 2) >= 1) ns *= 2;
    } else {
        while (wgs * ns < target && ns < 16 && nk_min / (ns * 2) >= 8) ns *= 2;
    }
    while (ns > 1 && (size_t)ns * bytes_per_split > ws_bytes) ns /= 2;
    return ns;
}

static NtPlan nt_plan_auto(const NtParams& p, int nphase, const NtFacts& f, size_t ws_bytes, int splitk);

// variant > 0: that kernel or an error; variant < 0: that kernel where it can run the problem, else the planner's choice (A/B runs)
static NtPlan nt_plan(const NtParams& p, int nphase, int vec, size_t esize, size_t ws_bytes, int variant, int splitk) {
    const NtFacts f = nt_facts(p, nphase, vec, esize);
    const bool prefer = variant < 0;
    if (prefer) variant = -variant;
    const NtPlan bad = prefer ? nt_plan_auto(p, nphase, f, ws_bytes, splitk) : NtPlan{-1, 1};
    const size_t part128 = (size_t)nphase * cdiv(p.M, 128) * 128 * p.N * 4, part256 = (size_t)nphase * cdiv(p.M, 256) * 256 * p.N * 4;
    switch (variant) {
        case EG_NT_REG: return {EG_NT_REG, 1};
        case EG_NT_BUF128:
            if (!f.dma_ok || !f.c_tiles || f.nk_max < 2) return bad;
            return {EG_NT_BUF128, nt_splits(f.tiles128, 512, f.nk_min, part128, ws_bytes, splitk)};
        case EG_NT_PERS: return f.dma_ok ? NtPlan{EG_NT_PERS, 1} : bad;
        case EG_NT_S8P: {
            Nt8pGeom g;
            if (!f.dma_ok || !f.c_tiles || !eg_nt8p_geometry(p, nphase, g)) return bad;
            return {variant, nt_splits((long long)cdiv(p.M, 256) * (p.N / 128) * nphase, 224, f.nk_min, part256, ws_bytes, splitk)};
        }
        case EG_NT_S8:
            if (!f.dma_ok || !f.c_tiles) return bad;
            return {variant, nt_splits((long long)cdiv(p.M, 256) * (p.N / 128) * nphase, 224, f.nk_min, part256, ws_bytes, splitk)};
        case EG_NT_S8H:
            if (!f.dma_ok || !f.c_tiles) return bad;
            return {variant, nt_splits(f.tiles128, 224, f.nk_min, part128, ws_bytes, splitk)};
        case EG_NT_AUTO: return nt_plan_auto(p, nphase, f, ws_bytes, splitk);
        default: return {-1, 1};
    }
}

static NtPlan nt_plan_auto(const NtParams& p, int nphase, const NtFacts& f, size_t ws_bytes, int splitk) {
    const size_t part128 = (size_t)nphase * cdiv(p.M, 128) * 128 * p.N * 4, part256 = (size_t)nphase * cdiv(p.M, 256) * 256 * p.N * 4;
    if (!f.dma_ok) return {EG_NT_REG, 1};
    // shallow launches (1-2 K steps: the image-side layers as 1x1 convolutions over patches) are all prologue and epilogue for a
    // workgroup-per-tile kernel: only the persistent pipeline overlaps them
    if (f.nk_max < 3 || !f.c_tiles) return f.tiles128 >= 128 ? NtPlan{EG_NT_PERS, 1} : NtPlan{EG_NT_REG, 1};
    // 256 x 128 tiles, one 8-wave workgroup per CU (igemm_nt8s): where the launch fills the chip in whole rounds and the K loop is long
    // enough to pay for a prologue and an epilogue that nothing overlaps (measured per shape: profiles/r02_d_layers_nt8s.txt); shorter
    // or fewer tiles run better as 128 x 128 tiles with two workgroups per CU (one's epilogue beside the other's K loop)
    const long long wgs256 = (long long)cdiv(p.M, 256) * (p.N / 128) * nphase;
    const long long rounds = (wgs256 + 255) / 256;
    // Measured in the whole (overlapped) step, the big tile wins beyond the shapes where it wins back to back: S8 wherever it can run
    // 4.70 ms, this rule set 4.76, 128 x 128 everywhere 4.93 (profiles/r02_r_ab_nt_variant.txt)
    // (16-bit launches of at least 48 such tiles: below that -- the small networks' layers -- and in fp32 the rule set below stays ahead,
    //  profiles/r02_r_ab_auto_s8.txt)
    // fewer than ~200 tiles of 256 x 128 (the single-tape layers: 64 or 128 such tiles on 256 CUs): the same 8-wave design on 128 x 128
    // tiles (igemm_nt8h) -- whole K loops in place of one K split level (profiles/r03_n_nt8h_layers.txt)
    constexpr int h_below = 200;
    if (f.half && wgs256 >= 48 && wgs256 < h_below && f.nk_min >= 8)
        return {EG_NT_S8H, nt_splits(f.tiles128, 224, f.nk_min, part128, ws_bytes, splitk)};
    if (f.half && wgs256 >= 48) return {EG_NT_S8, nt_splits(wgs256, 224, f.nk_min, part256, ws_bytes, splitk)};
    if (splitk <= 1 && f.nk_min >= 32 && wgs256 >= 200 && wgs256 * 100 >= rounds * 256 * 85) return {EG_NT_S8, 1};
    // split K only below one workgroup per CU: at 256..511 tiles the unsplit launch wins or ties (M=8192 N=512 K=4096: 52 vs 58 us,
    // the 4-phase M=2048 N=512 K=4096: 50 vs 48 us -- profiles/r02_i_t1_splits.txt) and saves the slab round trip and the epilogue launch
    constexpr int split_below = 256;
    // ... except very long K loops (>= 128 K tiles: the 512 -> 1024 layer, K = 8192), which still gain from two splits at 256 tiles
    // (in-step 110 -> 79 us, profiles/r02_q_step_detail.txt)
    const bool long_k = f.nk_min >= 128 && f.tiles128 <= 256;         // (at 384 tiles the split loses: 143 vs 116 us)
    if ((f.tiles128 < (splitk > 1 ? 512 : split_below) || long_k) && ws_bytes > 0) {
        const int ns = nt_splits(f.tiles128, 512, f.nk_min, part128, ws_bytes, splitk);
        if (ns > 1) return {EG_NT_BUF128, ns};
    }
    return f.tiles128 >= 256 ? NtPlan{EG_NT_BUF128, 1} : NtPlan{EG_NT_REG, 1};
}

template <typename T, int BM, int BN, int WGM, int WGN>
static void launch_nt_cfg(const NtParams& p, int nphase, hipStream_t st) {
    const int ns = p.nsplit > 1 ? p.nsplit : 1;
    dim3 grid(cdiv(p.M, BM), cdiv(p.N, BN), nphase * ns);
    const size_t lds = 2 * (BM + BN) * 128 > BM * BN * 4 ? 2 * (BM + BN) * 128 : BM * BN * 4;
    if constexpr (sizeof(T) == 2 && (BN == 64 || BN == 32)) {
        if (p.stat_mode != EG_STAT_NONE) {              // (nt_stat_blocks has checked: whole tiles, N == BN)
            // fp32 tile + the statistics' reduction scratch [2][rows lanes][BN] behind its first row
            const size_t need = (size_t)(1 + 2 * (256 / (BN / 8))) * BN * 4;
            if (ns > 1) hipLaunchKernelGGL((igemm_nt_kernel<T, BM, BN, WGM, WGN, true, true>), grid, dim3(256), lds > need ? lds : need, st, p);
            else hipLaunchKernelGGL((igemm_nt_kernel<T, BM, BN, WGM, WGN, true>), grid, dim3(256), lds > need ? lds : need, st, p);
            return;
        }
    }
    if constexpr (BN == 64 || BN == 32) {
        if (ns > 1) {
            hipLaunchKernelGGL((igemm_nt_kernel<T, BM, BN, WGM, WGN, false, true>), grid, dim3(256), lds, st, p);
            return;
        }
    }
    hipLaunchKernelGGL((igemm_nt_kernel<T, BM, BN, WGM, WGN>), grid, dim3(256), lds, st, p);
}

// K splits of the register-staged kernel (N = 32 / 64, NHWC output): few tiles and a deep K loop
// EXPERIMENT, off unless eg_epilogue.nt_splitk > 1 asks for it: correct (tested) but slower in the small networks'
// steps -- dSprites 1.415 -> 1.503 ms, colored / MNIST +0.2-0.8 % (profiles/r03_zg_ab_reg_split.txt): the 16-48-tile launches it targets
// are not the ~22 us the profiler shows for them once the profiler is off, and the split adds partial-tile traffic and a serial finish.
template <typename T>
static int nt_reg_splits(const NtParams& p, int nphase, int forced) {
    if (forced <= 1 || p.out_mode != EG_OUT_NHWC || !(p.N == 64 || p.N == 32) || (p.N % Elt<T>::VEC) != 0 || !p.part || p.part_bytes <= EG_SPLIT_CNT_BYTES) return 1;
    const long long tiles = (long long)cdiv(p.M, 128) * nphase;
    int nk = 1 << 30;
    for (int i = 0; i < nphase; ++i) nk = std::min(nk, p.ph[i].Kpad / (8 * Elt<T>::VEC));
    if (tiles >= 96 || nk < 8 || tiles > EG_SPLIT_CNT_BYTES / 4) return 1;
    int ns = 1;
    while (tiles * ns < 128 && ns < 16 && nk / (ns * 2) >= 2 && (forced <= 1 || ns * 2 <= forced)) ns *= 2;
    const size_t per_split = (size_t)nphase * cdiv(p.M, 128) * 128 * p.N * 4;
    while (ns > 1 && (size_t)ns * per_split > p.part_bytes - EG_SPLIT_CNT_BYTES) ns /= 2;
    return ns;
}

template <typename T>
static void launch_splitk_epilogue(const NtParams& q, int nphase, int Mpad, hipStream_t st) {
    // split launches have at most a few thousand tiles: M * N / VEC is far below 2^31
    const int vpr = q.N / Elt<T>::VEC;
    const long long vecs = (long long)q.M * vpr;
    const int blocks = (int)std::min<long long>((vecs + 255) / 256, std::max(1, 256 * 16 / nphase));
    int lvpr = -1;
    if ((vpr & (vpr - 1)) == 0) { lvpr = 0; while ((1 << lvpr) < vpr) ++lvpr; }
    hipLaunchKernelGGL((nt_splitk_epilogue_kernel<T>), dim3(blocks, nphase), dim3(256), 0, st, q, nphase, Mpad, lvpr);
}

static void fill_epilogue(NtParams& p, const eg_epilogue* ep) {
    p.bias = ep ? ep->bias : nullptr;
    p.bias_mod = ep ? ep->bias_mod : 0;
    p.sigma = ep ? ep->sigma : nullptr;
    p.act = ep ? ep->act : EG_ACT_NONE;
    p.slope = ep ? ep->slope : 0.f;
    p.mask = ep ? ep->mask : nullptr;
    p.mask_act = ep ? ep->mask_act : EG_ACT_NONE;
    p.mask_slope = ep ? ep->mask_slope : 0.f;
    p.out_mode = ep ? ep->out_mode : EG_OUT_NHWC;
    p.sigma_rows = ep ? ep->sigma_rows : 0;
    p.part = ep ? reinterpret_cast<float*>(ep->splitk_ws) : nullptr;
    p.part_bytes = ep ? ep->splitk_ws_bytes : 0;
    p.stat_mode = ep ? ep->stat_mode : EG_STAT_NONE;
    p.stat_out = ep ? ep->stat_out : nullptr;
    p.stat_aux = ep ? ep->stat_aux : nullptr;
    p.stat_p[0] = ep ? ep->stat_p0 : nullptr; p.stat_p[1] = ep ? ep->stat_p1 : nullptr;
    p.stat_p[2] = ep ? ep->stat_p2 : nullptr; p.stat_p[3] = ep ? ep->stat_p3 : nullptr;
    p.stat_act = ep ? ep->stat_act : EG_ACT_NONE;
    p.stat_slope = ep ? ep->stat_slope : 0.f;
}

// The one validator of eg_epilogue, run by nt_describe before any launch and before any query answers.  Everything it refuses would
// otherwise compute something else without a word: the kernels' switches fall through to EG_ACT_NONE for an unknown act / mask_act /
// stat_act (the mask's gradient becomes 1), every out_mode but EG_OUT_NHWC stores NCHW fp32, `n % bias_mod` of a negative bias_mod is
// `n % -bias_mod`, and a negative sigma_rows reads sigma[] in front of its first element.
static int check_epilogue(const eg_epilogue* ep) {
    if (!ep) return 0;
    EG_REQUIRE(ep->act >= EG_ACT_NONE && ep->act <= EG_ACT_SIGMOID, "eg_epilogue.act %d is no EG_ACT_* code", ep->act);
    EG_REQUIRE(ep->mask_act >= EG_ACT_NONE && ep->mask_act <= EG_ACT_SIGMOID, "eg_epilogue.mask_act %d is no EG_ACT_* code", ep->mask_act);
    EG_REQUIRE(ep->out_mode == EG_OUT_NHWC || ep->out_mode == EG_OUT_NCHW_F32, "eg_epilogue.out_mode %d is no EG_OUT_* code", ep->out_mode);
    EG_REQUIRE(ep->bias_mod >= 0 && ep->sigma_rows >= 0, "eg_epilogue.bias_mod (%d) and sigma_rows (%d) must not be negative", ep->bias_mod, ep->sigma_rows);
    EG_REQUIRE(ep->stat_mode == EG_STAT_NONE || (ep->stat_act >= EG_ACT_NONE && ep->stat_act <= EG_ACT_SIGMOID),
               "eg_epilogue.stat_act %d is no EG_ACT_* code", ep->stat_act);
    return 0;
}

// row blocks of the fused column statistics if this plan can produce them (the 8-wave kernel on whole 256-row tiles, K splits reduced
// inside the launch), else 0
static int nt_stat_blocks(const NtParams& p, int nphase, const NtPlan& plan, bool half) {
    if (!half || p.out_mode != EG_OUT_NHWC) return 0;
    if (plan.kind == EG_NT_S8H) return (p.M % 128) == 0 ? nphase * (p.M / 128) : 0;          // row blocks of 128
    // the register-staged kernel on 128 x 64 / 128 x 32 tiles (the small networks' layers): one column tile, whole row tiles
    if (plan.kind == EG_NT_REG) return ((p.N == 64 || p.N == 32) && (p.M % 128) == 0) ? nphase * (p.M / 128) : 0;
    if (plan.kind != EG_NT_S8 || (p.M % 256) != 0) return 0;
    return nphase * (p.M / 256);
}
static int check_stat(const NtParams& p) {
    if (p.stat_mode == EG_STAT_NONE) return 0;
    EG_REQUIRE(p.stat_mode >= EG_STAT_MOMENTS && p.stat_mode <= EG_STAT_SN_BIAS && p.stat_out, "eg_epilogue.stat_mode %d: bad mode or no stat_out", p.stat_mode);
    if (p.stat_mode == EG_STAT_BN_BWD)
        EG_REQUIRE(p.stat_aux && p.stat_p[0] && p.stat_p[1] && p.stat_p[2] && p.stat_p[3] && !p.mask, "EG_STAT_BN_BWD needs stat_aux (z), stat_p0..p3 (mean, invstd, gamma, beta) and no mask");
    if (p.stat_mode == EG_STAT_SN_BIAS)
        EG_REQUIRE(p.mask && p.mask_act == EG_ACT_LRELU && p.mask_slope > 0.f && p.stat_p[0] && p.stat_slope == p.mask_slope, "EG_STAT_SN_BIAS needs the LeakyReLU mask, stat_p0 (bias) and stat_slope == mask_slope");
    return 0;
}

// ---- one description per call: the launch and every query read the same NtCall, so a label, a buffer size and the launch cannot disagree
struct NtCall {
    NtParams p;
    int nphase;
    int variant, splitk;   // the caller's hints (eg_epilogue.nt_variant / nt_splitk)
    NtPlan plan;           // plan.kind < 0: the forced variant cannot run this problem
    int stat_nrb;          // row blocks of the fused column statistics under this plan; 0 = it cannot fuse them
};

// `unlimited`: plan as if any amount of split-K scratch were lent (what the problem could use, asked before there is a scratch)
static int nt_describe(const eg_conv* c, int dtype, int bwd, const eg_epilogue* ep, bool unlimited, NtCall& call) {
    if (int e = check_conv(c, dtype, bwd ? NEED_COUT : NEED_CIN)) return e;
    if (int e = check_epilogue(ep)) return e;
    NtParams& p = call.p;
    memset(&p, 0, sizeof(p));
    call.nphase = 1;
    if (bwd) { if (int e = geom_bwd(c, dtype, p, &call.nphase)) return e; }
    else geom_fwd(c, dtype, p);
    fill_epilogue(p, ep);
    call.variant = ep ? ep->nt_variant : EG_NT_AUTO;
    call.splitk = ep ? ep->nt_splitk : 0;
    // the tail of the scratch is kept for the arrival counters (nt_split_counters): no variant's partial tiles may reach it
    const size_t ws = unlimited ? (size_t)1 << 40 : (p.part && p.part_bytes > EG_SPLIT_CNT_BYTES) ? p.part_bytes - EG_SPLIT_CNT_BYTES : 0;
    call.plan = nt_plan(p, call.nphase, vec_of(dtype), dtype == EG_F32 ? 4 : 2, ws, call.variant, call.splitk);
    call.stat_nrb = nt_stat_blocks(p, call.nphase, call.plan, dtype != EG_F32);
    return 0;
}

static unsigned* nt_split_counters(const NtParams& p) {
    return reinterpret_cast<unsigned*>(reinterpret_cast<char*>(p.part) + p.part_bytes - EG_SPLIT_CNT_BYTES);
}

// column tile of the register-staged kernel (rows: 128)
static int nt_reg_bn(const NtCall& call) {
    const NtParams& p = call.p;
    if (p.N <= 16) return 16;
    if (p.N <= 32) return 32;
    if (p.N <= 64 || (call.variant != EG_NT_REG && (long long)cdiv(p.M, 128) * cdiv(p.N, 128) * call.nphase < 512)) return 64;
    return 128;
}

/* BM * 1000 + code, code = BN of the register-staged kernels, 131 / 132 = 128 x 128 buffer-descriptor kernel (plain / split-K), 135 =
 * persistent pipeline, 147 / 148 = igemm_nt8s, 149 / 150 = igemm_nt8s with the input patch, 151 / 152 = igemm_nt8h; -1 = the forced variant
 * cannot run the problem. */
static int nt_label(const NtCall& call) {
    const NtPlan& plan = call.plan;
    if (plan.kind < 0) return -1;
    if (plan.kind == EG_NT_S8) return 256 * 1000 + (plan.ns > 1 ? 148 : 147);
    if (plan.kind == EG_NT_S8P) return 256 * 1000 + (plan.ns > 1 ? 150 : 149);
    if (plan.kind == EG_NT_S8H) return 128 * 1000 + (plan.ns > 1 ? 152 : 151);
    if (plan.kind == EG_NT_PERS) return 128 * 1000 + 135;
    if (plan.kind == EG_NT_BUF128) return 128 * 1000 + (plan.ns > 1 ? 132 : 131);
    return 128 * 1000 + nt_reg_bn(call);
}

// one flag per kernel instantiation (the kernel is the template argument): each gets the attribute once, before its first launch
template <auto KERNEL>
static void nt_allow_lds(size_t lds) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
}

template <typename T>
static int launch_nt(const NtCall& call, hipStream_t st) {
    const NtParams& p = call.p;
    const NtPlan& plan = call.plan;
    const int nphase = call.nphase;
    EG_REQUIRE(plan.kind > 0, "eg_epilogue.nt_variant %d cannot run this problem (M=%d N=%d C=%d)", call.variant, p.M, p.N, p.C);
    EG_REQUIRE(p.stat_mode == EG_STAT_NONE || call.stat_nrb > 0, "eg_epilogue.stat_mode is set but this launch cannot fuse column statistics (eg_conv_stat_blocks() == 0: M=%d N=%d C=%d)", p.M, p.N, p.C);
    // what the kernels read beyond the description: the split count, the workgroup order (a runtime field of the parameter block) and, for the
    // kernels that reduce their K splits inside the launch, the arrival counters
    NtParams q = p;
    q.nsplit = plan.kind == EG_NT_REG ? nt_reg_splits<T>(p, nphase, call.splitk) : plan.ns;
    q.xcd_remap = 1;
    q.stat_nrb = call.stat_nrb;
    q.split_cnt = q.nsplit > 1 ? nt_split_counters(p) : nullptr;
    if (plan.kind == EG_NT_S8 || plan.kind == EG_NT_S8P) {
        Nt8pGeom g;
        memset(&g, 0, sizeof(g));
        if (plan.kind == EG_NT_S8P) EG_REQUIRE(eg_nt8p_geometry(p, nphase, g), "patch geometry");
        eg_launch_nt8s<T>(q, g, plan.kind == EG_NT_S8P, nphase, plan.ns, st);      // K splits are reduced inside the launch (last-arriving workgroup)
        return 0;
    }
    if (plan.kind == EG_NT_S8H) {
        eg_launch_nt8h<T>(q, nphase, plan.ns, st);
        return 0;
    }
    const size_t lds = 2 * (128 + 128) * 128;       // of the two DMA kernels below
    if (plan.kind == EG_NT_PERS) {
        nt_allow_lds<&igemm_nt_pers_kernel<T>>(lds);
        const int tm = cdiv(p.M, 128), tn = p.N / 128, ntiles = tm * tn * nphase;
        hipLaunchKernelGGL((igemm_nt_pers_kernel<T>), dim3(std::min(ntiles, 512)), dim3(256), lds, st, q, tm, tn, ntiles);
        return 0;
    }
    if (plan.kind == EG_NT_BUF128) {
        const int ns = plan.ns;
#ifdef EG_PROF
        // diagnostic build (make PROF=1): run the instrumented instantiation synchronously and print the per-wave averages of its phase
        // timers (wait+barrier / LDS-DMA issue / ds_read+MFMA / epilogue) -- how DESIGN.md section 6's round-1 breakdown was measured
        if (ns == 1) {
            const dim3 grid(cdiv(p.M, 128), p.N / 128, nphase);
            const size_t nw = (size_t)grid.x * grid.y * grid.z * 4;
            unsigned long long* dbuf = nullptr;
            (void)hipMalloc(&dbuf, nw * 64);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&igemm_nt_buf_kernel<T, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL((igemm_nt_buf_kernel<T, true>), grid, dim3(256), lds, st, q, dbuf);
            (void)hipStreamSynchronize(st);
            std::vector<unsigned long long> h(nw * 8);
            (void)hipMemcpy(h.data(), dbuf, nw * 64, hipMemcpyDeviceToHost);
            (void)hipFree(dbuf);
            double tot = 0, wt = 0, is = 0, cp = 0, ep = 0;
            for (size_t w = 0; w < nw; ++w) { tot += h[w * 8]; wt += h[w * 8 + 1]; is += h[w * 8 + 2]; cp += h[w * 8 + 3]; ep += h[w * 8 + 4]; }
            const int nk = p.ph[0].Kpad / (8 * Elt<T>::VEC);
            fprintf(stderr, "[nt_prof] grid %ux%ux%u nk %d | per wave (s_memtime ticks): total %.0f  wait+barrier %.0f (%.1f/step)  issue %.0f (%.1f/step)  compute %.0f (%.1f/step)  epilogue %.0f\n",
                    grid.x, grid.y, grid.z, nk, tot / nw, wt / nw, wt / nw / nk, is / nw, is / nw / nk, cp / nw, cp / nw / nk, ep / nw);
            return 0;
        }
#endif
        if (ns > 1) {
            nt_allow_lds<&igemm_nt_buf_kernel<T, false, true>>(lds);
            hipLaunchKernelGGL((igemm_nt_buf_kernel<T, false, true>), dim3(cdiv(p.M, 128), p.N / 128, nphase * ns), dim3(256), lds, st, q);
            launch_splitk_epilogue<T>(q, nphase, cdiv(p.M, 128) * 128, st);
        } else {
            nt_allow_lds<&igemm_nt_buf_kernel<T>>(lds);
            hipLaunchKernelGGL((igemm_nt_buf_kernel<T>), dim3(cdiv(p.M, 128), p.N / 128, nphase), dim3(256), lds, st, q);
        }
        return 0;
    }
    switch (nt_reg_bn(call)) {
        case 16: launch_nt_cfg<T, 128, 16, 4, 1>(q, nphase, st); break;
        case 32: launch_nt_cfg<T, 128, 32, 4, 1>(q, nphase, st); break;
        case 64: launch_nt_cfg<T, 128, 64, 2, 2>(q, nphase, st); break;
        default: launch_nt_cfg<T, 128, 128, 2, 2>(q, nphase, st);
    }
    return 0;
}

// eg_conv_fwd (bwd = 0: X, forward panels, Y) and eg_conv_bwd_data (bwd = 1: dY, backward panels, dX)
static int conv_nt(const eg_conv* c, int dtype, int bwd, const void* src, const void* wp, void* dst, const eg_epilogue* ep, eg_stream_t s) {
    NtCall call;
    if (int e = nt_describe(c, dtype, bwd, ep, false, call)) return e;
    EG_REQUIRE(src && wp && dst, "%s: null pointer", bwd ? "eg_conv_bwd_data" : "eg_conv_fwd");
    call.p.src = src; call.p.wp = wp; call.p.dst = dst;
    if (int e = check_stat(call.p)) return e;
    if (dtype == EG_F32) return launch_nt<float>(call, (hipStream_t)s);
    if (dtype == EG_F16) return launch_nt<f16_t>(call, (hipStream_t)s);
    return launch_nt<bf16_t>(call, (hipStream_t)s);
}

extern "C" int eg_conv_fwd(const eg_conv* c, int dtype, const void* X, const void* wp_fwd, void* Y,
                           const eg_epilogue* ep, eg_stream_t s) {
    if (int e = conv_nt(c, dtype, 0, X, wp_fwd, Y, ep, s)) return e;
    EG_LAUNCH_CHECK();
    return 0;
}

extern "C" int eg_conv_bwd_data(const eg_conv* c, int dtype, const void* dY, const void* wp_bwd, void* dX,
                                const eg_epilogue* ep, eg_stream_t s) {
    if (int e = conv_nt(c, dtype, 1, dY, wp_bwd, dX, ep, s)) return e;
    EG_LAUNCH_CHECK();
    return 0;
}

/* which igemm_nt instantiation eg_conv_fwd (bwd = 0) / eg_conv_bwd_data (bwd = 1) dispatches this problem to under the given hints
 * (profiling labels and tests; the same planner as the launches, with unlimited split-K scratch and NHWC output): nt_label's code */
extern "C" int eg_igemm_nt_tile(const eg_conv* c, int dtype, int bwd, int variant, int splitk) {
    eg_epilogue hints;
    memset(&hints, 0, sizeof(hints));       // no bias, no activation, no statistics, EG_OUT_NHWC
    hints.nt_variant = variant; hints.nt_splitk = splitk;
    NtCall call;
    if (!c || nt_describe(c, dtype, bwd, &hints, true, call)) return -1;
    return nt_label(call);
}

/* eg_igemm_nt_tile for one concrete call: the planner exactly as the launch runs it -- the epilogue's kernel hints AND its split-K scratch
 * (a launch whose scratch cannot hold the partial tiles does not split) */
extern "C" int eg_igemm_nt_tile_ep(const eg_conv* c, int dtype, int bwd, const eg_epilogue* ep) {
    NtCall call;
    if (!c || nt_describe(c, dtype, bwd, ep, false, call)) return -1;
    return nt_label(call);
}

extern "C" int eg_conv_stat_blocks(const eg_conv* c, int dtype, int bwd, const eg_epilogue* ep) {
    NtCall call;
    if (!c || nt_describe(c, dtype, bwd, ep, false, call)) return 0;
    return call.stat_nrb;
}

extern "C" size_t eg_conv_splitk_ws_bytes(const eg_conv* c, int dtype, int bwd) {
    // what the planner would split into with unlimited scratch (callers size one shared scratch from the maximum over their layers)
    NtCall call;
    if (!c || nt_describe(c, dtype, bwd, nullptr, true, call) || call.plan.ns <= 1) return 0;
    // EG_NT_S8H (= 6) works on 128-row tiles but gets the 256-row padding here too: up to 128 rows more than it needs where M % 256 is in
    // 1..128.  Kept: callers size shared buffers from this value.
    const int bm = call.plan.kind >= EG_NT_S8 ? 256 : 128;
    const NtParams& p = call.p;
    return (size_t)call.plan.ns * call.nphase * cdiv(p.M, bm) * bm * p.N * 4 + EG_SPLIT_CNT_BYTES;      // + the arrival counters at the scratch's tail
}
