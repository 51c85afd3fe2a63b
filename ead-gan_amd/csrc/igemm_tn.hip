// igemm_tn : S[n][t][c] = sum_m P[m][n] * X[pix(m,t)][c]   (weight gradients, split over m into partial slabs; fp32 or 16-bit MFMA with
// fp32 accumulate, like igemm.hip).  The per-tap kernel and its launcher; the parity-class kernel of the big 4x4 / stride-2 layers is
// igemm_tn8.hip.
#include <algorithm>
#include <type_traits>

#include "eg_common.h"
#include "igemm_nt.h"
#include "conv_geom.h"

// This file is compiled with -ffp-contract=off (Makefile), like the file it was split from.

// ------------------------------------------------------------------------------------------------
// igemm_tn : weight-gradient partial slabs
// ------------------------------------------------------------------------------------------------
struct TnParams {
    const void* P;     // [M][N]
    const void* src;   // [B,H,W,C]
    float* slab;       // [nsplit][N][ntaps][C]
    int B, H, W, C, N;
    int lOH, lOW, M;
    int TW, ntaps;
    int sy, sx, dy0, dx0, up;
    int rows_per_split;
    int ntn, ntc;
};

// swizzle of a [32][BW] element tile in units of 16 elements
__device__ __forceinline__ int tn_fsw(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }

template <typename T, int BNT, int BCT, int KR>   // KR = rows of m per K step (32, or 64: half the barriers per MFMA)
__global__ __launch_bounds__(256) void igemm_tn_kernel(const TnParams p) {
    constexpr int VEC = Elt<T>::VEC;
    constexpr int TM = BNT / 32, TN = BCT / 32;            // 2x2 waves
    constexpr int CPR_P = BNT / VEC, CPR_S = BCT / VEC;    // 16-byte chunks per row
    constexpr int LD_P = KR * CPR_P / 256 > 0 ? KR * CPR_P / 256 : 1;
    constexpr int LD_S = KR * CPR_S / 256 > 0 ? KR * CPR_S / 256 : 1;
    constexpr int MASK_P = BNT / 16 - 1, MASK_S = BCT / 16 - 1;
    constexpr int STAGE = KR * (BNT + BCT) * (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tn_i = blockIdx.x / p.ntc, tc_i = blockIdx.x % p.ntc;
    const int n0 = tn_i * BNT, c0 = tc_i * BCT;
    const int t = blockIdx.y, ty = t / p.TW, tx = t % p.TW;
    const int mbeg = blockIdx.z * p.rows_per_split;
    const int mend = min(p.M, mbeg + p.rows_per_split);
    const int nk = (mend - mbeg + KR - 1) / KR;
    const int OWm = (1 << p.lOW) - 1, OHm = (1 << p.lOH) - 1;
    const int HU = p.H << p.up, WU = p.W << p.up;
    const T* __restrict__ P = reinterpret_cast<const T*>(p.P);
    const T* __restrict__ src = reinterpret_cast<const T*>(p.src);

    uint4 rp[LD_P], rs[LD_S];
    auto gload = [&](int kt) {
        const int mb = mbeg + kt * KR;
#pragma unroll
        for (int i = 0; i < LD_P; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx / CPR_P, ch = idx % CPR_P;
            const int m = mb + row, n = n0 + ch * VEC;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (row < KR && m < mend && n < p.N) v = *reinterpret_cast<const uint4*>(P + (size_t)m * p.N + n);
            rp[i] = v;
        }
#pragma unroll
        for (int i = 0; i < LD_S; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx / CPR_S, ch = idx % CPR_S;
            const int m = mb + row, c = c0 + ch * VEC;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (row < KR && m < mend && c < p.C) {
                const int b = m >> (p.lOW + p.lOH);
                const int iy = ((m >> p.lOW) & OHm) * p.sy + p.dy0 + ty;
                const int ix = (m & OWm) * p.sx + p.dx0 + tx;
                if (iy >= 0 && iy < HU && ix >= 0 && ix < WU) {
                    const size_t pix = ((size_t)b * p.H + (iy >> p.up)) * p.W + (ix >> p.up);
                    v = *reinterpret_cast<const uint4*>(src + pix * p.C + c);
                }
            }
            rs[i] = v;
        }
    };
    auto lstore = [&](int stage) {
        T* sp = reinterpret_cast<T*>(smem + stage * STAGE);
        T* ss = sp + KR * BNT;
#pragma unroll
        for (int i = 0; i < LD_P; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx / CPR_P, e = (idx % CPR_P) * VEC;
            if (row < KR) *reinterpret_cast<uint4*>(sp + row * BNT + ((((e >> 4) ^ (tn_fsw(row) & MASK_P)) << 4) | (e & 15))) = rp[i];
        }
#pragma unroll
        for (int i = 0; i < LD_S; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx / CPR_S, e = (idx % CPR_S) * VEC;
            if (row < KR) *reinterpret_cast<uint4*>(ss + row * BCT + ((((e >> 4) ^ (tn_fsw(row) & MASK_S)) << 4) | (e & 15))) = rs[i];
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (nk > 0) {
        gload(0);
        lstore(0);
    }
    __syncthreads();
    const int g = lane >> 4, li = lane & 15;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) gload(kt + 1);
        const T* sp = reinterpret_cast<const T*>(smem + (kt & 1) * STAGE);
        const T* ss = sp + KR * BNT;
        if constexpr (std::is_same<T, float>::value) {
#pragma unroll
            for (int kg = 0; kg < KR / 4; ++kg) {
                const int row = kg * 4 + g;
                const int f = tn_fsw(row);
                float av[TM], bv[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int blk = (wm * TM + i);
                    av[i] = sp[row * BNT + (((blk ^ (f & MASK_P)) << 4) | li)];
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int blk = (wn * TN + j);
                    bv[j] = ss[row * BCT + (((blk ^ (f & MASK_S)) << 4) | li)];
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
            }
        } else {
            // transposed LDS reads: each 16-lane group g fetches k rows 8g..8g+7 (two 4-row blocks) of a 16-column block
            const int q = li >> 2, pc = li & 3;
#pragma unroll
            for (int kb = 0; kb < KR; kb += 32) {
            uint4 af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int blk = (wm * TM + i);
                s16x4 lo, hi;
                {
                    const int row = kb + 8 * g + q;
                    lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sp + row * BNT + (((blk ^ (tn_fsw(row) & MASK_P)) << 4) | (pc * 4))));
                }
                {
                    const int row = kb + 8 * g + 4 + q;
                    hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sp + row * BNT + (((blk ^ (tn_fsw(row) & MASK_P)) << 4) | (pc * 4))));
                }
                af[i] = make_uint4(((uint32_t)(uint16_t)lo[0]) | ((uint32_t)(uint16_t)lo[1] << 16), ((uint32_t)(uint16_t)lo[2]) | ((uint32_t)(uint16_t)lo[3] << 16),
                                   ((uint32_t)(uint16_t)hi[0]) | ((uint32_t)(uint16_t)hi[1] << 16), ((uint32_t)(uint16_t)hi[2]) | ((uint32_t)(uint16_t)hi[3] << 16));
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int blk = (wn * TN + j);
                s16x4 lo, hi;
                {
                    const int row = kb + 8 * g + q;
                    lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(ss + row * BCT + (((blk ^ (tn_fsw(row) & MASK_S)) << 4) | (pc * 4))));
                }
                {
                    const int row = kb + 8 * g + 4 + q;
                    hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(ss + row * BCT + (((blk ^ (tn_fsw(row) & MASK_S)) << 4) | (pc * 4))));
                }
                bfr[j] = make_uint4(((uint32_t)(uint16_t)lo[0]) | ((uint32_t)(uint16_t)lo[1] << 16), ((uint32_t)(uint16_t)lo[2]) | ((uint32_t)(uint16_t)lo[3] << 16),
                                    ((uint32_t)(uint16_t)hi[0]) | ((uint32_t)(uint16_t)hi[1] << 16), ((uint32_t)(uint16_t)hi[2]) | ((uint32_t)(uint16_t)hi[3] << 16));
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    if constexpr (std::is_same<T, f16_t>::value)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, af[i]), __builtin_bit_cast(f16x8_t, bfr[j]), acc[i][j], 0, 0, 0);
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[i]), __builtin_bit_cast(bf16x8_t, bfr[j]), acc[i][j], 0, 0, 0);
            }
        }
        if (kt + 1 < nk) lstore((kt + 1) & 1);
        __syncthreads();
    }

    float* slab = p.slab + (size_t)blockIdx.z * p.N * p.ntaps * p.C;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + (wm * TM + i) * 16 + g * 4 + r;
            if (n >= p.N) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int c = c0 + (wn * TN + j) * 16 + li;
                if (c < p.C) slab[((size_t)n * p.ntaps + t) * p.C + c] = acc[i][j][r];
            }
        }
}

static void tn_tiles(const eg_conv* c, int* bnt, int* bct) {
    *bnt = c->Cout >= 128 ? 128 : (c->Cout > 32 ? 64 : 32);
    *bct = c->Cin >= 128 ? 128 : (c->Cin > 32 ? 64 : 32);
}

void eg_tn_plan(const eg_conv* c, int wgs_target, int* nsplit, int* rps) {
    const int OH = conv_out_dim(c, c->H), OW = conv_out_dim(c, c->W);
    const int M = c->B * OH * OW;
    int bnt, bct;
    tn_tiles(c, &bnt, &bct);
    const long long base = (long long)cdiv(c->Cout, bnt) * cdiv(c->Cin, bct) * c->k * c->k;
    constexpr int target = 768;      // workgroups per launch
    long long want = base >= target ? 1 : (target + base - 1) / base;
    long long cap = M / 256 > 0 ? M / 256 : 1;
    if (want > cap) want = cap;
    // the cap binds where one output tile (x a tap or two) is all there is -- the image-side layers as GEMMs over patch rows, and there it IS
    // the grid: 128 workgroups of a 32 x 64 tile keep ~1.5 MB in flight and stream the 100-134 MB of the small networks' image-side layers at
    // ~1 TB/s; 512 of them: colored dSprites 3.08 -> 2.98 ms, dSprites 1.39 -> 1.38, MNIST neutral (profiles/r03_zv_tn_maxsplit_small.txt).
    // Big tiles (CelebA's 128-channel image-side layer, on a lane beside the main chain's GEMMs) keep 128: more took CUs from the main chain
    // (5.50 -> 5.65 ms at 512, profiles/r01_timeline_notes.md item 14).
    const int max_split = bnt * bct <= 64 * 64 ? 512 : 128;
    if (want > max_split) want = max_split;
    // a caller's own split count (eg_wgrad_img_tn, whose tests reach one-step and ragged splits with it); eg_conv_wgrad's per-tap launches
    // never had one and plan with 0
    if (wgs_target > 0) want = std::min<long long>(wgs_target, std::max(1, M / 32));
    int r = round_up((int)((M + want - 1) / want), 32);
    *rps = r;
    *nsplit = cdiv(M, r);
}

/* 2: the parity-class kernel igemm_tn8 runs this weight gradient, 1: the per-tap kernel igemm_tn (profiling labels and tests) */
extern "C" int eg_conv_wgrad_variant(const eg_conv* c, int dtype) {
    int ns;
    Tn8Params p8;
    if (!c || check_conv(c, dtype, NEED_CIN | NEED_COUT)) return -1;
    return eg_tn8_plan(c, dtype, p8, &ns, 0) ? 2 : 1;
}

extern "C" size_t eg_conv_wgrad_ws_bytes(const eg_conv* c, int dtype) {
    int ns, rps;
    Tn8Params p8;
    if (!c || check_conv(c, dtype, NEED_CIN | NEED_COUT)) return 0;      // a convolution eg_conv_wgrad refuses needs no slab
    if (eg_tn8_plan(c, dtype, p8, &ns, 0))      // the whole-chip target splits furthest
        return (size_t)ns * c->Cout * 16 * c->Cin * sizeof(float);
    eg_tn_plan(c, 0, &ns, &rps);
    return (size_t)ns * c->Cout * c->k * c->k * c->Cin * sizeof(float);
}

template <typename T, int BNT, int BCT, int KR>
static void launch_tn_kr(TnParams& p, const dim3& grid, hipStream_t st) {
    const size_t lds = 2 * KR * (BNT + BCT) * sizeof(T);
    if (lds > 65536) {
        static bool attr_set = false;
        if (!attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&igemm_tn_kernel<T, BNT, BCT, KR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            attr_set = true;
        }
    }
    hipLaunchKernelGGL((igemm_tn_kernel<T, BNT, BCT, KR>), grid, dim3(256), lds, st, p);
}

template <typename T, int BNT, int BCT>
static void launch_tn_cfg(TnParams& p, int nsplit, hipStream_t st) {
    p.ntn = cdiv(p.N, BNT); p.ntc = cdiv(p.C, BCT);
    dim3 grid(p.ntn * p.ntc, p.ntaps, nsplit);
    // 32 rows per pipeline step; 64 (half the barriers) measured 10-20 % slower on the CelebA layers.  Launches with ONE output tile (the
    // image-side layers: the grid is just the split count, <= 128 workgroups streaming the whole activation) are latency-bound on bytes in
    // flight per workgroup: those get 64 rows per step (colored dSprites B=512: 5.22 -> 5.00 ms; CelebA, dSprites, MNIST neutral to +1 %).
    if (p.ntn * p.ntc * p.ntaps == 1 && sizeof(T) == 2 && BNT + BCT <= 192)
        launch_tn_kr<T, BNT, BCT, 64>(p, grid, st);
    else
        launch_tn_kr<T, BNT, BCT, 32>(p, grid, st);
}

template <typename T>
static void launch_tn(TnParams& p, int bnt, int bct, int nsplit, hipStream_t st) {
#define EG_TN_CASE(a, b) if (bnt == a && bct == b) { launch_tn_cfg<T, a, b>(p, nsplit, st); return; }
    EG_TN_CASE(128, 128) EG_TN_CASE(128, 64) EG_TN_CASE(128, 32)
    EG_TN_CASE(64, 128) EG_TN_CASE(64, 64) EG_TN_CASE(64, 32)
    EG_TN_CASE(32, 128) EG_TN_CASE(32, 64) EG_TN_CASE(32, 32)
#undef EG_TN_CASE
}

extern "C" int eg_conv_wgrad(const eg_conv* c, int dtype, const void* X, const void* dY, float* slab, int* nsplit_out,
                             int wgs_target, eg_stream_t s) {
    if (int e = check_conv(c, dtype, NEED_CIN | NEED_COUT)) return e;
    EG_REQUIRE(X && dY && slab && nsplit_out && wgs_target >= 0, "eg_conv_wgrad: bad argument");
    const int OH = conv_out_dim(c, c->H), OW = conv_out_dim(c, c->W);
    {
        // 16-bit 4x4 / stride-2 layers with channel counts in multiples of 128: the parity-class kernel (igemm_tn8.hip), same slab layout
        Tn8Params p8;
        int ns8 = 0;
        if (eg_tn8_plan(c, dtype, p8, &ns8, wgs_target)) {
            p8.P = dY; p8.src = X; p8.slab = slab;
            if (dtype == EG_F16) eg_launch_tn8<f16_t>(p8, ns8, (hipStream_t)s);
            else eg_launch_tn8<bf16_t>(p8, ns8, (hipStream_t)s);
            *nsplit_out = ns8;
            EG_LAUNCH_CHECK();
            return 0;
        }
    }
    TnParams p;
    memset(&p, 0, sizeof(p));
    p.P = dY; p.src = X; p.slab = slab;
    p.B = c->B; p.H = c->H; p.W = c->W; p.C = c->Cin; p.N = c->Cout;
    p.lOH = ilog2_exact(OH); p.lOW = ilog2_exact(OW); p.M = c->B * OH * OW;
    p.TW = c->k; p.ntaps = c->k * c->k;
    p.sy = p.sx = c->stride; p.dy0 = p.dx0 = -c->pad; p.up = c->up;
    int ns, rps, bnt, bct;
    eg_tn_plan(c, 0, &ns, &rps);
    tn_tiles(c, &bnt, &bct);
    p.rows_per_split = rps;
    if (dtype == EG_F32) launch_tn<float>(p, bnt, bct, ns, (hipStream_t)s);
    else if (dtype == EG_F16) launch_tn<f16_t>(p, bnt, bct, ns, (hipStream_t)s);
    else launch_tn<bf16_t>(p, bnt, bct, ns, (hipStream_t)s);
    *nsplit_out = ns;
    EG_LAUNCH_CHECK();
    return 0;
}
