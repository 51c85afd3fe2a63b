// Shared pieces of the NT implicit-GEMM kernels (igemm.hip, igemm_nt8s.hip, igemm_nt8h.hip): launch parameters, LDS image of a K row,
// MFMA step, buffer-descriptor LDS-DMA helpers and the fused epilogue through LDS.  gfx950 only.
#pragma once
#include <type_traits>

#include "eg_common.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4;

// ------------------------------------------------------------------------------------------------
// geometry derived from eg_conv
// ------------------------------------------------------------------------------------------------
struct NtPhase {
    int TH, TW, dy0, dys, dx0, dxs, ooy, oox, K, Kpad;
    long long w_off;   // element offset of this phase's packed weights
};
struct NtParams {
    const void* src;
    const void* wp;
    void* dst;
    const float* bias;
    const float* sigma;
    const void* mask;
    int B, H, W, C;   // gathered source tensor (NHWC)
    int lOH, lOW;     // log2 of the output lattice
    int sy, sx, up;
    int N, bias_mod;
    int DH, DW, osy, osx;
    int act;
    float slope;
    int mask_act;
    float mask_slope;
    int out_mode;
    int sigma_rows;
    int M;
    float* part;      // split-K partial tiles [split][phase][Mpad][N] fp32 (nsplit > 1)
    int xcd_remap;    // igemm_nt_buf: 1 = every XCD gets a contiguous range of M tiles (workgroups are dispatched round robin over the 8 XCDs)
    size_t part_bytes;
    int nsplit;
    unsigned* split_cnt;   // igemm_nt8s with K splits: arrival counters, one per output tile (tail of the caller's split-K scratch; zero between launches)
    // column statistics of the stored tile (eg_epilogue.stat_*; igemm_nt8s only)
    int stat_mode, stat_nrb;
    float* stat_out;
    const void* stat_aux;
    const float* stat_p[4];
    int stat_act;
    float stat_slope;
    NtPhase ph[4];
};
// the last EG_SPLIT_CNT_BYTES of the caller-lent split-K scratch hold the arrival counters of igemm_nt8s's in-kernel reduction (at most 224
// tiles split); no planner ever places partial tiles there.  The scratch must be zero when it is first lent; every launch leaves the
// counters at zero again.
#define EG_SPLIT_CNT_BYTES 4096

// patch geometry of igemm_nt8p_kernel (igemm_nt8s.hip): filter taps grouped into classes that walk one pixel lattice
struct NtClass { int oy0, ox0, AH, AW, ty0, tys, tx0, txs; };       // source = stride * lattice + o0; tap(ay, ax) = (ty0 + ay*tys, tx0 + ax*txs)
struct Nt8pPhase { int ncls; NtClass cls[4]; };
struct Nt8pGeom {
    int nimg, OHt;                  // images per 256-row tile; output rows of one image per tile
    int PH, PW, npix, npp;          // patch lattice per image, pixels per patch, DMA pieces per wave
    unsigned inv_pw, inv_plane;     // x / PW == (x * inv_pw) >> 20, x / (PH*PW) == (x * inv_plane) >> 20  for x < 512
    Nt8pPhase ph[4];
};
#define EG_P8P_SLOTS 448

// the 8-wave NT kernels' launchers (igemm_nt8s.hip, igemm_nt8h.hip), called by the planner's dispatch in igemm.hip
bool eg_nt8p_geometry(const NtParams& p, int nphase, Nt8pGeom& g);
template <typename T> void eg_launch_nt8s(const NtParams& p, const Nt8pGeom& g, bool patch, int nphase, int ns, hipStream_t st);
template <typename T> void eg_launch_nt8h(const NtParams& p, int nphase, int ns, hipStream_t st);

// launch parameters of igemm_tn8_kernel (igemm_tn8.hip): weight gradients of the 4x4 / stride-2 layers, taps grouped by input parity
struct Tn8Params {
    const void* P;      // [M][N]
    const void* src;    // [B,H,W,C]
    float* slab;        // [nsplit][N][16][C]
    int B, H, W, C, N;
    int lOH, lOW, M;
    int rows_per_split; // multiple of 64
    int ntn, ntc, ch;   // tiles; channels per tile on both sides (128 or 64)
    int nimg, OHt, PH, PW, npix, npp;       // per 64-row K step: images, output rows per image, patch lattice, pixels, X pieces per wave
    unsigned inv_pw, inv_plane;             // x / PW, x / (PH * PW) as (x * inv) >> 20 for x < 512
};

#define EG_TN8_XSLOTS 136                   // patch pixel slots per stage (34 pieces of 4 pixels x 256 B, or 17 of 8 pixels x 128 B)

// its planner and launcher (igemm_tn8.hip), called by eg_conv_wgrad in igemm_tn.hip
bool eg_tn8_plan(const eg_conv* c, int dtype, Tn8Params& p, int* nsplit, int wgs_target);
template <typename T> void eg_launch_tn8(const Tn8Params& p, int nsplit, hipStream_t st);
// swizzle key of K row `row` of a P tile staged by LDS-DMA (igemm_tn8.hip, wgrad_img_tn.hip): source block b lands in block b ^ key
__device__ __forceinline__ int tn8_fsw(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }

// split plan of the per-tap kernel (igemm_tn.hip): splits and rows per split (a multiple of 32).  wgs_target 0: the plan of eg_conv_wgrad's
// per-tap launches; > 0: that many splits, down to one 32-row step each (eg_wgrad_img_tn, which walks the same splits)
void eg_tn_plan(const eg_conv* c, int wgs_target, int* nsplit, int* rps);

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
static inline int bk_of(int dtype) { return dtype == EG_F32 ? 32 : 64; }
static inline int vec_of(int dtype) { return dtype == EG_F32 ? 4 : 8; }

// ------------------------------------------------------------------------------------------------
// LDS helpers: rows of 128 bytes, 16-byte chunk c of row r lives at chunk (c ^ ((r>>1)&7))
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// D = B-fragment x A-fragment: the weight-panel rows (n) land on the accumulator ROW index (4 consecutive n per lane),
// the gathered rows (m) on the lane -> the epilogue packs 4 consecutive output channels per lane.
template <typename T>
__device__ __forceinline__ void mfma_step(const uint4& a, const uint4& b, f32x4& acc) {
    if constexpr (std::is_same<T, float>::value) {
        const float* af = reinterpret_cast<const float*>(&a);
        const float* bf = reinterpret_cast<const float*>(&b);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[e], af[e], acc, 0, 0, 0);
    } else if constexpr (std::is_same<T, f16_t>::value) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, b), __builtin_bit_cast(f16x8_t, a), acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, b), __builtin_bit_cast(bf16x8_t, a), acc, 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------------
// The fused epilogue.  Every NT kernel finishes a value alike -- acc * (1 / sigma), + bias, activation, optionally times the
// activation-gradient mask, rounded to T, stored at the NHWC address of row m of its phase -- and the variants are tested bit for bit
// against each other, so each step is written once:
//   nt_out_byx / nt_out_off    destination pixel / NHWC element offset of row m
//   nt_sigma_at / nt_bias_at   sigma of a row, bias of a column
//   nt_epi_finish              1/sigma, bias and activation of one accumulator value
//   nt_epi_mask                N values times the activation-gradient mask
//   nt_epi_store               N values rounded to T and stored as one vector
// The register epilogue of igemm_nt_pers, the scalar tail of igemm_nt and nt_splitk_epilogue_kernel (igemm.hip) are these pieces in
// accumulator / partial-tile layout.  Every other kernel goes through LDS: nt_epi_prefetch, then nt_epi_stage puts the finished fp32
// BM x BNW window into LDS (16-byte chunks XOR-swizzled by row: nt_tile_at) and nt_epi_rows walks its rows with 16-byte mask loads and
// stores -- nt_epilogue_lds_reg (register-staged kernel) and nt_epilogue_lds_stat (column statistics, every kernel).  The plain epilogue
// of the LDS-DMA kernels, nt_epilogue_lds_pre, is the one copy left: same steps, its own text (reason at nt_epi_prefetch).
// ------------------------------------------------------------------------------------------------
struct NtPix { int b, y, x; };
// ooy / oox: the phase's NtPhase.ooy / oox
__device__ __forceinline__ NtPix nt_out_byx(const NtParams& p, int m, int ooy, int oox) {
    const int OWm = (1 << p.lOW) - 1, OHm = (1 << p.lOH) - 1;
    return {m >> (p.lOW + p.lOH), ((m >> p.lOW) & OHm) * p.osy + ooy, (m & OWm) * p.osx + oox};
}
__device__ __forceinline__ size_t nt_pix_index(const NtParams& p, const NtPix& q) { return ((size_t)q.b * p.DH + q.y) * p.DW + q.x; }
__device__ __forceinline__ size_t nt_out_off(const NtParams& p, int m, int ooy, int oox, int n) {
    return nt_pix_index(p, nt_out_byx(p, m, ooy, oox)) * p.N + n;
}

// sigma of output row m (sigma_rows rows per tape; 0: one sigma for all) and bias of column n
__device__ __forceinline__ float nt_sigma_at(const NtParams& p, int m) { return p.sigma ? p.sigma[p.sigma_rows ? m / p.sigma_rows : 0] : 1.f; }
__device__ __forceinline__ float nt_bias_at(const NtParams& p, int n) { return p.bias ? p.bias[p.bias_mod ? n % p.bias_mod : n] : 0.f; }
__device__ __forceinline__ float nt_inv_sigma(const NtParams& p, float sigma) { return p.sigma ? 1.f / sigma : 1.f; }

// inv_sigma: nt_inv_sigma(nt_sigma_at(row)); bias: nt_bias_at(column), added when has_bias
__device__ __forceinline__ float nt_epi_finish(float acc, float inv_sigma, bool has_bias, float bias, const NtParams& p, const EgActFast& af) {
    float x = __fmul_rn(acc, inv_sigma);
    if (has_bias) x = __fadd_rn(x, bias);
    return af.special ? eg_act(x, p.act, p.slope) : eg_act_apply(x, af);
}

// me: the N stored activations (or pre-activations' signs) the gradient is taken from
template <typename T, int N>
__device__ __forceinline__ void nt_epi_mask(float* f, const T* me, const NtParams& p, const EgGradFast& gf) {
    if (!gf.special) {
#pragma unroll
        for (int q = 0; q < N; ++q) f[q] *= eg_grad_apply(Elt<T>::ld(me + q), gf);
    } else {
#pragma unroll
        for (int q = 0; q < N; ++q) f[q] *= eg_act_grad_from_out(Elt<T>::ld(me + q), p.mask_act, p.mask_slope);
    }
}

template <int BYTES> struct NtBits;
template <> struct NtBits<16> { typedef uint4 type; };
template <> struct NtBits<8> { typedef uint2 type; };
template <> struct NtBits<4> { typedef unsigned type; };
template <> struct NtBits<2> { typedef unsigned short type; };
template <typename T, int N> using NtVec = typename NtBits<N * sizeof(T)>::type;      // N elements of T as one load / store

template <typename T, int N>
__device__ __forceinline__ void nt_epi_store(T* dst, const float* f) {
    NtVec<T, N> ov;
    T* oe = reinterpret_cast<T*>(&ov);
#pragma unroll
    for (int q = 0; q < N; ++q) Elt<T>::st(oe + q, f[q]);
    *reinterpret_cast<NtVec<T, N>*>(dst) = ov;
}

// Epilogue operands fetched ahead of the last K step: sigma per accumulator row block, the bias of the lane's 4 x TN columns and the
// activation-gradient mask vectors of the first PF store iterations -- their global-load latency (the epilogue's critical path: ~40 %
// of a 16-step launch) overlaps the last MFMA block and the LDS staging.
template <typename T, int TM, int TN, int PF>
struct NtEpiPre {
    float sigma[TM];
    int m_first;      // PF = 0 (nt_epi_fetch_reg): nothing runs between fetch and use, so nt_epi_stage reads sigma where it is used (row m_first + 16 i)
    float bias[TN][4];
    uint4 mask[PF > 0 ? PF : 1];
};

// row0 / col0: first row / first window column of the calling wave's accumulators; nw0: global column of the window's first column;
// NT threads per workgroup.  Rows beyond M read the last row's sigma, columns beyond N no bias (neither is stored).
// This function and nt_epilogue_lds_pre keep the text they had before the epilogue was folded into the pieces above: the 8-wave
// kernels sit at their register limits, and with the pieces their input-patch instantiations spilled two more SGPRs and the unsplit
// bf16 launches of igemm_nt8s ran 0-2 % slower (profiles/nt_epilogue_ab.txt).
template <typename T, int BM, int BNW, int TM, int TN, int NT, int PF>
__device__ __forceinline__ void nt_epi_prefetch(NtEpiPre<T, TM, TN, PF>& e, const NtParams& p, const NtPhase& ph, int m0, int nw0, int row0, int col0,
                                                int tid, int frow, int fq) {
    constexpr int VEC = Elt<T>::VEC;
    constexpr int VPR = BNW / VEC, RPP = NT / VPR;
    const int OWm = (1 << p.lOW) - 1, OHm = (1 << p.lOH) - 1;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int mrow = min(m0 + row0 + i * 16 + frow, p.M - 1);
        e.sigma[i] = p.sigma ? p.sigma[p.sigma_rows ? mrow / p.sigma_rows : 0] : 1.f;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = nw0 + col0 + j * 16 + fq * 4 + r;
            e.bias[j][r] = (p.bias && n < p.N) ? p.bias[p.bias_mod ? n % p.bias_mod : n] : 0.f;
        }
    const T* __restrict__ mask = reinterpret_cast<const T*>(p.mask);
    const int vc = tid % VPR, vr = tid / VPR;
    const int n = nw0 + vc * VEC;
#pragma unroll
    for (int it = 0; it < PF; ++it) {
        const int m = m0 + vr + it * RPP;
        e.mask[it] = make_uint4(0, 0, 0, 0);
        if (mask && n < p.N && m < p.M) {
            const int b = m >> (p.lOW + p.lOH);
            const int y = ((m >> p.lOW) & OHm) * p.osy + ph.ooy;
            const int x = (m & OWm) * p.osx + ph.oox;
            e.mask[it] = *reinterpret_cast<const uint4*>(mask + (((size_t)b * p.DH + y) * p.DW + x) * p.N + n);
        }
    }
}

// the register-staged kernel's form (PF = 0): the lane's bias; sigma is read by nt_epi_stage.  m_first / n_first: row / column of acc[0][0][0]
template <typename T, int TM, int TN>
__device__ __forceinline__ void nt_epi_fetch_reg(NtEpiPre<T, TM, TN, 0>& e, const NtParams& p, int m_first, int n_first) {
    e.m_first = m_first;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n_first + j * 16 + r;
            e.bias[j][r] = p.bias && n < p.N ? nt_bias_at(p, n) : 0.f;
        }
}

// 16-byte chunk `chunk` of row `row` of the fp32 BM x BNW tile in LDS
template <int BNW>
__device__ __forceinline__ float* nt_tile_at(float* ct, int row, int chunk) {
    constexpr int SW = BNW / 4 < 32 ? BNW / 4 - 1 : 31;     // 16-byte fp32 chunks per tile row - 1
    return ct + row * BNW + ((chunk ^ (row & SW)) << 2);
}
// the VEC values of vector column vc of a row
template <int BNW, int VEC>
__device__ __forceinline__ void nt_tile_row(float* ct, int row, int vc, float* f) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(nt_tile_at<BNW>(ct, row, vc * (VEC / 4) + q));
        f[q * 4 + 0] = v.x; f[q * 4 + 1] = v.y; f[q * 4 + 2] = v.z; f[q * 4 + 3] = v.w;
    }
}

// the accumulators with 1/sigma, bias and activation applied go to the fp32 tile in LDS.  Callers __syncthreads() before (the K loop's
// LDS is reused) and after.
template <typename T, int BNW, int TM, int TN, int PF>
__device__ __forceinline__ void nt_epi_stage(const NtEpiPre<T, TM, TN, PF>& e, const NtParams& p, f32x4 (&acc)[TM][TN], char* smem, int nw0, int row0,
                                             int col0, int frow, int fq) {
    float* ct = reinterpret_cast<float*>(smem);
    const EgActFast af = eg_act_fast(p.act, p.slope);
    eg_if_fast(af.special, [&](auto fast) {
        EgActFast a = af;
        a.special = !decltype(fast)::value;             // a compile-time constant inside nt_epi_finish
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = row0 + i * 16 + frow;
            const float inv_sigma = nt_inv_sigma(p, PF > 0 ? e.sigma[i] : nt_sigma_at(p, min(e.m_first + i * 16, p.M - 1)));
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int nl = col0 + j * 16 + fq * 4;
                float4 v;
                float* ve = reinterpret_cast<float*>(&v);
#pragma unroll
                for (int r = 0; r < 4; ++r) ve[r] = nt_epi_finish(acc[i][j][r], inv_sigma, p.bias && nw0 + nl + r < p.N, e.bias[j][r], p, a);
                *reinterpret_cast<float4*>(nt_tile_at<BNW>(ct, row, nl >> 2)) = v;
            }
        }
    });
}

// the row walk over the staged tile: thread (vr, vc) takes columns nw0 + vc * VEC .. + VEC - 1 of rows vr, vr + RPP, ...: the row's values
// times the mask (its first PF vectors come from e), then store(o, f, mv) with o the NHWC offset, f the VEC values and mv the mask vector
// (zeros without a mask).  RAGGED: rows beyond M and columns beyond N are skipped; otherwise the tile is whole.
template <typename T, int BM, int BNW, int NT, bool RAGGED, int TM, int TN, int PF, typename F>
__device__ __forceinline__ void nt_epi_rows(const NtEpiPre<T, TM, TN, PF>& e, const NtParams& p, const NtPhase& ph, char* smem, int m0, int nw0, int tid,
                                            F&& store) {
    constexpr int VEC = Elt<T>::VEC;
    constexpr int VPR = BNW / VEC, RPP = NT / VPR, NIT = BM / RPP;
    // e.mask[it] needs the whole loop unrolled; without it (PF = 0: the register-staged kernel, its STAT instantiations too, which used to
    // unroll fully) 4 rows in flight keep the registers low
    constexpr int UNR = PF > 0 || NIT < 4 ? NIT : 4;
    float* ct = reinterpret_cast<float*>(smem);
    const EgGradFast gf = eg_grad_fast(p.mask_act, p.mask_slope);
    const int vc = tid % VPR, vr = tid / VPR;
    const T* __restrict__ mask = reinterpret_cast<const T*>(p.mask);
    const int n = nw0 + vc * VEC;
    if (RAGGED && n >= p.N) return;
#pragma unroll UNR
    for (int it = 0; it < NIT; ++it) {
        const int row = vr + it * RPP;
        const int m = m0 + row;
        if (RAGGED && m >= p.M) break;
        const size_t o = nt_out_off(p, m, ph.ooy, ph.oox, n);
        float f[VEC];
        nt_tile_row<BNW, VEC>(ct, row, vc, f);
        uint4 mv = make_uint4(0, 0, 0, 0);
        if (mask) {
            mv = it < PF ? e.mask[it < PF ? it : 0] : *reinterpret_cast<const uint4*>(mask + o);
            nt_epi_mask<T, VEC>(f, reinterpret_cast<const T*>(&mv), p, gf);
        }
        store(o, f, mv);
    }
}

// the epilogue through LDS of the register-staged kernel (PF = 0), made of the pieces
template <typename T, int BM, int BNW, int TM, int TN, int NT>
__device__ __forceinline__ void nt_epilogue_lds_reg(const NtEpiPre<T, TM, TN, 0>& e, const NtParams& p, const NtPhase& ph, f32x4 (&acc)[TM][TN], char* smem,
                                                    int m0, int nw0, int row0, int col0, int tid, int frow, int fq) {
    nt_epi_stage<T, BNW, TM, TN, 0>(e, p, acc, smem, nw0, row0, col0, frow, fq);
    __syncthreads();
    nt_epi_rows<T, BM, BNW, NT, true>(e, p, ph, smem, m0, nw0, tid, [&](size_t o, float* f, const uint4&) {
        nt_epi_store<T, Elt<T>::VEC>(reinterpret_cast<T*>(p.dst) + o, f);
    });
}

// the same for the LDS-DMA kernels (igemm_nt_buf, igemm_nt8s, igemm_nt8h; PF > 0), in its earlier text: see nt_epi_prefetch
template <typename T, int BM, int BNW, int TM, int TN, int NT, int PF>
__device__ __forceinline__ void nt_epilogue_lds_pre(const NtEpiPre<T, TM, TN, PF>& e, const NtParams& p, const NtPhase& ph, f32x4 (&acc)[TM][TN],
                                                    char* smem, int m0, int nw0, int row0, int col0, int tid, int frow, int fq) {
    constexpr int VEC = Elt<T>::VEC;
    const int OWm = (1 << p.lOW) - 1, OHm = (1 << p.lOH) - 1;
    constexpr int SW = BNW / 4 < 32 ? BNW / 4 - 1 : 31;     // 16-byte fp32 chunks per tile row - 1
    float* ct = reinterpret_cast<float*>(smem);
    const EgActFast af = eg_act_fast(p.act, p.slope);
    const EgGradFast gf = eg_grad_fast(p.mask_act, p.mask_slope);
    eg_if_fast(af.special, [&](auto fast) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = row0 + i * 16 + frow;
            const float inv_sigma = p.sigma ? 1.f / e.sigma[i] : 1.f;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int nl = col0 + j * 16 + fq * 4;
                float4 v;
                float* ve = reinterpret_cast<float*>(&v);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float x = __fmul_rn(acc[i][j][r], inv_sigma);
                    if (p.bias && nw0 + nl + r < p.N) x = __fadd_rn(x, e.bias[j][r]);
                    if constexpr (decltype(fast)::value) ve[r] = eg_act_apply(x, af);
                    else ve[r] = eg_act(x, p.act, p.slope);
                }
                *reinterpret_cast<float4*>(ct + row * BNW + (((nl >> 2) ^ (row & SW)) << 2)) = v;
            }
        }
    });
    __syncthreads();
    constexpr int VPR = BNW / VEC;
    constexpr int RPP = NT / VPR;
    constexpr int NIT = BM / RPP;
    const int vc = tid % VPR, vr = tid / VPR;
    const T* __restrict__ mask = reinterpret_cast<const T*>(p.mask);
    const int n = nw0 + vc * VEC;
    if (n < p.N) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int row = vr + it * RPP;
            const int m = m0 + row;
            if (m >= p.M) break;
            const int b = m >> (p.lOW + p.lOH);
            const int y = ((m >> p.lOW) & OHm) * p.osy + ph.ooy;
            const int x = (m & OWm) * p.osx + ph.oox;
            const size_t o = (((size_t)b * p.DH + y) * p.DW + x) * p.N + n;
            float f[VEC];
#pragma unroll
            for (int q = 0; q < VEC / 4; ++q) {
                const int chunk = (vc * (VEC / 4) + q) ^ (row & SW);
                const float4 v = *reinterpret_cast<const float4*>(ct + row * BNW + (chunk << 2));
                f[q * 4 + 0] = v.x; f[q * 4 + 1] = v.y; f[q * 4 + 2] = v.z; f[q * 4 + 3] = v.w;
            }
            if (mask) {
                const uint4 mv = it < PF ? e.mask[it < PF ? it : 0] : *reinterpret_cast<const uint4*>(mask + o);
                const T* me = reinterpret_cast<const T*>(&mv);
                if (!gf.special) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) f[q] *= eg_grad_apply(Elt<T>::ld(me + q), gf);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) f[q] *= eg_act_grad_from_out(Elt<T>::ld(me + q), p.mask_act, p.mask_slope);
                }
            }
            uint4 ov;
            T* oe = reinterpret_cast<T*>(&ov);
#pragma unroll
            for (int q = 0; q < VEC; ++q) Elt<T>::st(oe + q, f[q]);
            *reinterpret_cast<uint4*>(reinterpret_cast<T*>(p.dst) + o) = ov;
        }
    }
}

// nt_epilogue_lds_pre + column statistics of the stored tile (NtParams.stat_*, eg_epilogue.stat_mode in the ABI header): the same staging,
// the same stored values (EG_STAT_BN_BWD stores dy = da * act'(bn(z)) instead of da), plus two sums per column over the tile's BM rows,
// taken from the values as they are stored (rounded to T).  Order of the sums: a thread adds its NIT rows top down, then the RPP row
// lanes of a column are added in lane order -> deterministic.  Whole tiles only (the planner guarantees m0 + BM <= M); 16-bit types.
// rb = phase * tiles_m + m_tile: row block of the tile in stat_out; n_tile / tiles_n: for the per-tile dot of EG_STAT_SN_BIAS.
template <typename T, int BM, int BNW, int TM, int TN, int NT, int PF>
__device__ __forceinline__ void nt_epilogue_lds_stat(const NtEpiPre<T, TM, TN, PF>& e, const NtParams& p, const NtPhase& ph, f32x4 (&acc)[TM][TN],
                                                     char* smem, int m0, int nw0, int row0, int col0, int tid, int frow, int fq, int rb, int n_tile,
                                                     int tiles_n) {
    constexpr int VEC = Elt<T>::VEC;
    static_assert(VEC == 8, "16-bit element types");
    float* ct = reinterpret_cast<float*>(smem);
    nt_epi_stage<T, BNW, TM, TN, PF>(e, p, acc, smem, nw0, row0, col0, frow, fq);
    __syncthreads();
    constexpr int VPR = BNW / VEC, RPP = NT / VPR;
    const int vc = tid % VPR, vr = tid / VPR;
    const T* __restrict__ aux = reinterpret_cast<const T*>(p.stat_aux);
    const int n = nw0 + vc * VEC;
    const int mode = p.stat_mode;
    auto round_t = [](float v) { T t; Elt<T>::st(&t, v); return Elt<T>::ld(&t); };
    float s1[VEC], s2[VEC], k0[VEC], k1[VEC], k2[VEC], k3[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) { s1[q] = 0.f; s2[q] = 0.f; k0[q] = 0.f; k1[q] = 0.f; k2[q] = 0.f; k3[q] = 0.f; }
    if (mode == EG_STAT_MOMENTS) {
        // pivot = the column's value in the tile's first row (any pivot is exact; this one keeps the sums small)
#pragma unroll
        for (int q = 0; q < VEC; ++q) k0[q] = round_t(ct[vc * VEC + q]);
    } else if (mode == EG_STAT_BN_BWD) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            const float mu = p.stat_p[0][n + q], is = p.stat_p[1][n + q], g = p.stat_p[2][n + q], b = p.stat_p[3][n + q];
            k0[q] = mu; k1[q] = is; k2[q] = __fmul_rn(g, is); k3[q] = __fsub_rn(b, __fmul_rn(mu, k2[q]));
        }
    } else {
#pragma unroll
        for (int q = 0; q < VEC; ++q) k0[q] = p.stat_p[0][n + q];
    }
    const EgGradFast sgf = eg_grad_fast(p.stat_act, p.stat_slope);
    const float inv_slope = p.stat_slope != 0.f ? 1.f / p.stat_slope : 1.f;
    nt_epi_rows<T, BM, BNW, NT, false>(e, p, ph, smem, m0, nw0, tid, [&](size_t o, float* f, const uint4& mv) {
        if (mode == EG_STAT_MOMENTS) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                const float d = round_t(f[q]) - k0[q];
                s1[q] += d;
                s2[q] = fmaf(d, d, s2[q]);
            }
        } else if (mode == EG_STAT_BN_BWD) {
            const uint4 zv = *reinterpret_cast<const uint4*>(aux + o);
            const T* ze = reinterpret_cast<const T*>(&zv);
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                const float z = Elt<T>::ld(ze + q);
                const float xh = (z - k0[q]) * k1[q];
                const float dy = round_t(f[q]) * eg_grad_apply(fmaf(z, k2[q], k3[q]), sgf);      // the forward's activation input: z * (g * is) + (b - mu * g * is)
                f[q] = dy;
                s1[q] += dy;
                s2[q] = fmaf(dy, xh, s2[q]);
            }
        } else {
            const T* me = reinterpret_cast<const T*>(&mv);
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                const float g = round_t(f[q]);
                float a = Elt<T>::ld(me + q);
                a = a > 0.f ? a : a * inv_slope;
                s1[q] += g;
                s2[q] = fmaf(g, a - k0[q], s2[q]);
            }
        }
        nt_epi_store<T, VEC>(reinterpret_cast<T*>(p.dst) + o, f);
    });
    __syncthreads();                                   // every row of the tile has been read: rows 1.. become the reduction scratch
    float* red = ct + BNW;                             // [2][RPP][BNW]; row 0 of the tile (the pivots) stays
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
        *reinterpret_cast<float4*>(red + (size_t)vr * BNW + vc * VEC + q * 4) = make_float4(s1[q * 4], s1[q * 4 + 1], s1[q * 4 + 2], s1[q * 4 + 3]);
        *reinterpret_cast<float4*>(red + (size_t)(RPP + vr) * BNW + vc * VEC + q * 4) = make_float4(s2[q * 4], s2[q * 4 + 1], s2[q * 4 + 2], s2[q * 4 + 3]);
    }
    __syncthreads();
    float t2 = 0.f;
    if (tid < BNW) {
        float t1 = 0.f;
#pragma unroll 8
        for (int l = 0; l < RPP; ++l) { t1 += red[l * BNW + tid]; t2 += red[(RPP + l) * BNW + tid]; }
        const size_t nrb = (size_t)p.stat_nrb;
        float* o1 = p.stat_out + (size_t)(nw0 + tid) * nrb + rb;
        if (mode == EG_STAT_MOMENTS) {
            const float pv = round_t(ct[tid]), cnt = (float)BM;
            o1[0] = pv + t1 / cnt;
            o1[(size_t)p.N * nrb] = fmaxf(t2 - t1 * t1 / cnt, 0.f);
        } else if (mode == EG_STAT_BN_BWD) {
            o1[0] = t1;
            o1[(size_t)p.N * nrb] = t2;
        } else {
            o1[0] = t1;
        }
    }
    constexpr int NWV = (BNW + 63) / 64;               // waves that hold the column threads (2 for BNW = 128, 1 for 64 / 32)
    if (mode == EG_STAT_SN_BIAS && tid < NWV * 64) {   // the tile's dot, added in wave order (whole waves: the threads beyond BNW add zeros)
        const float w = wave_sum(tid < BNW ? t2 : 0.f);
        if ((tid & 63) == 0) red[2 * RPP * BNW + (tid >> 6)] = w;
    }
    if (mode == EG_STAT_SN_BIAS) {
        __syncthreads();
        if (tid == 0) {
            float d = red[2 * RPP * BNW];
#pragma unroll
            for (int w = 1; w < NWV; ++w) d += red[2 * RPP * BNW + w];
            p.stat_out[(size_t)p.N * p.stat_nrb + (size_t)rb * tiles_n + n_tile] = d;
        }
    }
}

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x4_t eg_make_srd(const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    u32x4_t r;
    r.x = __builtin_amdgcn_readfirstlane((unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);
    r.z = __builtin_amdgcn_readfirstlane(bytes);
    r.w = 0x00020000u;
    return r;
}

#define EG_OOB 0x80000000u

// one 1-KiB LDS-DMA piece (64 lanes x 16 B from per-lane offsets into `srd`, + the SGPR offset) to LDS [lds, lds + 1 KiB).  Issued
// through inline asm so that hipcc does not count it: the caller owns the waits (counted s_waitcnt vmcnt + s_barrier before any wave
// reads the bytes).  M0 is saved and restored inside the statement.
__device__ __forceinline__ void eg_bufdma1s(const u32x4_t srd, unsigned v0, unsigned soff, unsigned lds) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %4\n\ts_nop 0\n\t"
        "buffer_load_dwordx4 %1, %2, %3 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(v0), "s"(srd), "s"(soff), "s"(lds)
        : "memory");
}

// the same without saving M0 (three instructions): for kernels in which nothing else reads M0 -- gfx9 LDS instructions do not, and the
// kernels that use this form contain no GWS, s_movrel or s_sendmsg code.  LDS address = base + OFF.
template <int OFF>
__device__ __forceinline__ void eg_bufdma1f(const u32x4_t srd, unsigned v0, unsigned soff, unsigned lds_base) {
    asm volatile(
        "s_add_u32 m0, %3, %4\n\ts_nop 0\n\t"
        "buffer_load_dwordx4 %0, %1, %2 offen lds"
        :
        : "v"(v0), "s"(srd), "s"(soff), "s"(lds_base), "i"(OFF)
        : "memory", "scc");
}

template <int STRIDE>
__device__ __forceinline__ void eg_bufdma4s(const u32x4_t srd, unsigned v0, unsigned v1, unsigned v2, unsigned v3, unsigned soff, unsigned lds) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %7\n\ts_nop 0\n\t"
        "buffer_load_dwordx4 %1, %5, %6 offen lds\n\t"
        "s_add_u32 m0, m0, %8\n\ts_nop 0\n\t"
        "buffer_load_dwordx4 %2, %5, %6 offen lds\n\t"
        "s_add_u32 m0, m0, %8\n\ts_nop 0\n\t"
        "buffer_load_dwordx4 %3, %5, %6 offen lds\n\t"
        "s_add_u32 m0, m0, %8\n\ts_nop 0\n\t"
        "buffer_load_dwordx4 %4, %5, %6 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(srd), "s"(soff), "s"(lds), "i"(STRIDE)
        : "memory", "scc");
}
template <int STRIDE>
__device__ __forceinline__ void eg_bufdma2s(const u32x4_t srd, unsigned v0, unsigned v1, unsigned soff, unsigned lds) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %5\n\ts_nop 0\n\t"
        "buffer_load_dwordx4 %1, %3, %4 offen lds\n\t"
        "s_add_u32 m0, m0, %6\n\ts_nop 0\n\t"
        "buffer_load_dwordx4 %2, %3, %4 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(v0), "v"(v1), "s"(srd), "s"(soff), "s"(lds), "i"(STRIDE)
        : "memory", "scc");
}
