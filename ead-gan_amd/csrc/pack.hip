// Weight packing for the implicit-GEMM kernels: fp32 master weights -> the K-contiguous panels igemm_nt reads, stand-alone, fused with
// the Adam update of the master, and batched over many tensors in one launch.
#include <vector>

#include "eg_common.h"
#include "igemm_nt.h"
#include "conv_geom.h"
#include "adam.h"

// This file is compiled with -ffp-contract=off (Makefile): the Adam + pack kernels must round a parameter like the flat-arena update of
// sn_adam.hip does (adam.h), and clang contracts `a * b + c` depending on where the operands come from.

// ------------------------------------------------------------------------------------------------
// weight packing: fp32 master [Cout][Cin][k][k]  ->  K-contiguous dtype-T panels
// ------------------------------------------------------------------------------------------------
struct PackPhase { int TH, TW, kh0, kw0, K, Kpad; long long w_off; };
struct PackParams {
    const float* w;
    void* wp;
    int Nrows;           // rows of the packed panel
    int Crow;            // channels per tap in a row
    int khs, kws, k;
    long long n_stride, c_stride;   // master strides of the (row, channel) indices
    int nphase;
    PackPhase ph[4];
};

// (the pack kernels' bodies take their block coordinates as arguments: pack_multi_kernel below runs several layers' packs in one launch)
template <typename T>
__device__ __forceinline__ void pack_gather_body(const PackParams& p, int bx, int by, int gx) {
    const PackPhase ph = p.ph[by];
    const long long total = (long long)p.Nrows * ph.Kpad;
    for (long long i = (long long)bx * blockDim.x + threadIdx.x; i < total; i += (long long)gx * blockDim.x) {
        const int n = (int)(i / ph.Kpad), kk = (int)(i % ph.Kpad);
        float v = 0.f;
        if (kk < ph.K) {
            const int t = kk / p.Crow, c = kk % p.Crow;
            const int ty = t / ph.TW, tx = t % ph.TW;
            const int kh = ph.kh0 + ty * p.khs, kw = ph.kw0 + tx * p.kws;
            v = p.w[n * p.n_stride + c * p.c_stride + kh * p.k + kw];
        }
        Elt<T>::st(reinterpret_cast<T*>(p.wp) + ph.w_off + i, v);
    }
}
template <typename T>
__global__ void pack_kernel(const PackParams p) { pack_gather_body<T>(p, blockIdx.x, blockIdx.y, gridDim.x); }

struct PackTileParams;
static bool pack_record_gather(const PackParams& p, int dtype, int gx, int gy);
static bool pack_record_strided(int kind, int dtype, const float* w, void* wp, int N, int K, int Kpad, int n_div, long long s_hi, long long s_lo,
                                long long s_k, int k_div, long long s_khi, long long s_klo, int gx);
static bool pack_record_tile(const PackTileParams& p, int dtype, int gx, int gy);

static void launch_pack(const PackParams& p, int dtype, hipStream_t st) {
    long long total = 0;
    for (int i = 0; i < p.nphase; ++i) total = total > (long long)p.Nrows * p.ph[i].Kpad ? total : (long long)p.Nrows * p.ph[i].Kpad;
    const int blocks = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
    if (pack_record_gather(p, dtype, blocks, p.nphase)) return;
    if (dtype == EG_F32) hipLaunchKernelGGL(pack_kernel<float>, dim3(blocks, p.nphase), dim3(256), 0, st, p);
    else if (dtype == EG_F16) hipLaunchKernelGGL(pack_kernel<f16_t>, dim3(blocks, p.nphase), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(pack_kernel<bf16_t>, dim3(blocks, p.nphase), dim3(256), 0, st, p);
}

extern "C" size_t eg_pack_fwd_elems(const eg_conv* c, int dtype) {
    return (size_t)c->Cout * kpad_of(c->k * c->k * c->Cin, dtype);
}
extern "C" size_t eg_pack_bwd_elems(const eg_conv* c, int dtype) {
    size_t tot = 0;
    for (int ry = 0; ry < c->stride; ++ry)
        for (int rx = 0; rx < c->stride; ++rx) {
            const int K = bwd_axis(c, ry).T * bwd_axis(c, rx).T * c->Cout;
            tot += (size_t)c->Cin * kpad_of(K, dtype);
        }
    return tot;
}

extern "C" int eg_pack_fwd(const eg_conv* c, int dtype, const float* w, void* wp, eg_stream_t s) {
    EG_REQUIRE(c && w && wp, "eg_pack_fwd: null pointer");
    PackParams p;
    memset(&p, 0, sizeof(p));
    p.w = w; p.wp = wp; p.Nrows = c->Cout; p.Crow = c->Cin;
    p.khs = p.kws = 1; p.k = c->k;
    p.n_stride = (long long)c->Cin * c->k * c->k; p.c_stride = c->k * c->k;
    p.nphase = 1;
    p.ph[0].TH = p.ph[0].TW = c->k; p.ph[0].kh0 = p.ph[0].kw0 = 0;
    p.ph[0].K = c->k * c->k * c->Cin; p.ph[0].Kpad = kpad_of(p.ph[0].K, dtype); p.ph[0].w_off = 0;
    launch_pack(p, dtype, (hipStream_t)s);
    EG_LAUNCH_CHECK();
    return 0;
}

extern "C" int eg_pack_bwd(const eg_conv* c, int dtype, const float* w, void* wp, eg_stream_t s) {
    EG_REQUIRE(c && w && wp && c->stride <= 2, "eg_pack_bwd: bad argument");
    PackParams p;
    memset(&p, 0, sizeof(p));
    p.w = w; p.wp = wp; p.Nrows = c->Cin; p.Crow = c->Cout;
    p.khs = p.kws = c->stride; p.k = c->k;
    p.n_stride = c->k * c->k; p.c_stride = (long long)c->Cin * c->k * c->k;
    long long off = 0;
    int n = 0;
    for (int ry = 0; ry < c->stride; ++ry)
        for (int rx = 0; rx < c->stride; ++rx) {
            const BwdAxis ay = bwd_axis(c, ry), ax = bwd_axis(c, rx);
            PackPhase& f = p.ph[n++];
            f.TH = ay.T; f.TW = ax.T > 0 ? ax.T : 1; f.kh0 = ay.k0; f.kw0 = ax.k0;
            f.K = ay.T * ax.T * c->Cout; f.Kpad = kpad_of(f.K, dtype); f.w_off = off;
            off += (long long)c->Cin * f.Kpad;
        }
    p.nphase = n;
    launch_pack(p, dtype, (hipStream_t)s);
    EG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Both panels of a conv layer in one pass over its fp32 master [Cout][Cin][k*k] (conv view): a workgroup stages a 16 (Cout) x 32 (Cin)
// x taps tile in LDS with coalesced reads and writes it out twice as 16-byte vectors -- K-contiguous rows [n][tap][c] of the forward
// panel and [c][tap'][n] rows of every backward (sub-pixel phase) panel.  The per-element gather above reads the master with a
// 64-byte (forward) or Cin*64-byte (backward) stride and was 5-9 % of a CelebA iteration.
// ------------------------------------------------------------------------------------------------
#define EG_PACKM_TC 8       // Cin tile of the tile jobs inside pack_multi_kernel (and of the stand-alone tile kernels)
struct PackTileParams {
    const float* w;
    void* wp_fwd;          // may be null
    void* wp_bwd;          // may be null
    int Cout, Cin, T;      // T = k*k
    int nq;                // (phase, tap') combinations of the backward panels
    int t_of[16];          // master tap index of combination q
    int pitch[16];         // row pitch (Kpad) of q's phase
    long long off[16];     // element offset of (c = 0, n = 0) of combination q inside wp_bwd
    // K padding (only the Adam + pack kernel takes layers that have any): the columns [K, pitch) of every row are written as zeros
    int pad;               // any panel passed has padding (one test on the kernels' common path, where none has)
    int kfwd, pitch_fwd;   // columns and row pitch (Kpad) of the forward panel
    int nph;               // backward (sub-pixel phase) panels
    int ph_k[4], ph_pitch[4];
    long long ph_off[4];   // element offset of phase panel i inside wp_bwd
};

// TTC: taps (k*k) as a compile-time constant (16 for every 4x4 layer; 0 = run time): the index arithmetic below divides by it per element
template <typename T, int TTC, int TC>
__device__ __forceinline__ void pack_conv_tile_body(const PackTileParams& p, float* tile, int bx, int by) {
    constexpr int VEC = Elt<T>::VEC;
    constexpr int TN = 16;
    const int TT = TTC ? TTC : p.T, TP = TT + 1;
    const int n0 = bx * TN, c0 = by * TC;
    const int tid = threadIdx.x;
    for (int e = tid; e < TN * TC * TT; e += 256) {
        const int n = e / (TC * TT), rem = e - n * (TC * TT);
        const int c = rem / TT, t = rem - c * TT;
        tile[(n * TC + c) * TP + t] = p.w[((size_t)(n0 + n) * p.Cin + c0) * TT + rem];
    }
    __syncthreads();
    if (p.wp_fwd) {
        T* dst = reinterpret_cast<T*>(p.wp_fwd);
        const size_t pitch = (size_t)TT * p.Cin;
        for (int it = tid; it < TN * TT * (TC / VEC); it += 256) {
            const int cg = it % (TC / VEC), r = it / (TC / VEC);
            const int t = r % TT, n = r / TT;
            uint4 ov;
            T* oe = reinterpret_cast<T*>(&ov);
#pragma unroll
            for (int j = 0; j < VEC; ++j) Elt<T>::st(oe + j, tile[(n * TC + cg * VEC + j) * TP + t]);
            *reinterpret_cast<uint4*>(dst + (size_t)(n0 + n) * pitch + (size_t)t * p.Cin + c0 + cg * VEC) = ov;
        }
    }
    if (p.wp_bwd) {
        T* dst = reinterpret_cast<T*>(p.wp_bwd);
        for (int it = tid; it < TC * p.nq * (TN / VEC); it += 256) {
            const int ng = it % (TN / VEC), r = it / (TN / VEC);
            const int q = r % p.nq, c = r / p.nq;
            const int t = p.t_of[q];
            uint4 ov;
            T* oe = reinterpret_cast<T*>(&ov);
#pragma unroll
            for (int j = 0; j < VEC; ++j) Elt<T>::st(oe + j, tile[((ng * VEC + j) * TC + c) * TP + t]);
            *reinterpret_cast<uint4*>(dst + p.off[q] + (size_t)(c0 + c) * p.pitch[q] + n0 + ng * VEC) = ov;
        }
    }
}
template <typename T, int TTC, int TC>
__global__ __launch_bounds__(256) void pack_conv_tile_kernel(const PackTileParams p) {
    extern __shared__ float tile[];                 // [TN][TC][T + 1]
    pack_conv_tile_body<T, TTC, TC>(p, tile, blockIdx.x, blockIdx.y);
}

// tile-kernel parameters of a layer, or false where only the per-element gather kernels can pack it (ragged channel counts; K padding
// unless `allow_pad`: the kernel then zero-fills it)
static bool pack_tile_params(const eg_conv* c, int dtype, void* wp_fwd, void* wp_bwd, PackTileParams& p, bool allow_pad = false) {
    const int T = c->k * c->k, bk = bk_of(dtype);
    bool fast = (c->Cout % 16) == 0 && (c->Cin % 32) == 0 && T <= 16 && (!wp_bwd || c->stride <= 2);
    memset(&p, 0, sizeof(p));
    p.wp_fwd = wp_fwd; p.wp_bwd = wp_bwd; p.Cout = c->Cout; p.Cin = c->Cin; p.T = T;
    p.kfwd = T * c->Cin; p.pitch_fwd = kpad_of(T * c->Cin, dtype);
    p.pad = wp_fwd && p.kfwd != p.pitch_fwd;
    if (fast && wp_fwd && (T * c->Cin) % bk != 0 && !allow_pad) fast = false;          // K padding: the gather kernel zero-fills
    if (fast && wp_bwd) {
        long long off = 0;
        for (int ry = 0; ry < c->stride && fast; ++ry)
            for (int rx = 0; rx < c->stride && fast; ++rx) {
                const BwdAxis ay = bwd_axis(c, ry), ax = bwd_axis(c, rx);
                const int K = ay.T * ax.T * c->Cout;
                const int Kpad = kpad_of(K, dtype);
                if (K != Kpad && !allow_pad) { fast = false; break; }
                p.ph_k[p.nph] = K; p.ph_pitch[p.nph] = Kpad; p.ph_off[p.nph] = off;
                if (K != Kpad) p.pad = 1;
                ++p.nph;
                for (int ty = 0; ty < ay.T; ++ty)
                    for (int tx = 0; tx < ax.T; ++tx) {
                        const int kh = ay.k0 + ty * c->stride, kw = ax.k0 + tx * c->stride;
                        p.t_of[p.nq] = kh * c->k + kw;
                        p.pitch[p.nq] = Kpad;
                        p.off[p.nq] = off + (long long)(ty * ax.T + tx) * c->Cout;
                        ++p.nq;
                    }
                off += (long long)c->Cin * Kpad;
            }
    }
    return fast;
}

extern "C" int eg_pack_conv(const eg_conv* c, int dtype, const float* w, void* wp_fwd, void* wp_bwd, eg_stream_t s) {
    EG_REQUIRE(c && w && (wp_fwd || wp_bwd), "eg_pack_conv: null pointer");
    EG_REQUIRE(dtype == EG_F32 || dtype == EG_BF16 || dtype == EG_F16, "dtype must be EG_F32, EG_BF16 or EG_F16");
    const int T = c->k * c->k;
    PackTileParams p;
    const bool fast = pack_tile_params(c, dtype, wp_fwd, wp_bwd, p);
    p.w = w;
    if (!fast) {
        if (wp_fwd) if (int e = eg_pack_fwd(c, dtype, w, wp_fwd, s)) return e;
        if (wp_bwd) if (int e = eg_pack_bwd(c, dtype, w, wp_bwd, s)) return e;
        return 0;
    }
    // Cin tile 8 (16-byte panel stores, 8.5 KiB of LDS: fits on a CU beside a resident 8-wave GEMM workgroup: the re-packing on the optimizer
    // lane then runs beside the next sub-step's GEMMs), not 32 (64-byte stores, 34 KiB); A/B in profiles/r03_zm_ab_pack_tc.txt
    constexpr int tc = 8;
    const dim3 grid(c->Cout / 16, c->Cin / tc);
    const size_t lds = (size_t)16 * tc * (T + 1) * sizeof(float);
    if (pack_record_tile(p, dtype, grid.x, c->Cin / EG_PACKM_TC)) return 0;     // (the joint launch tiles Cin by EG_PACKM_TC)
#define EG_PACK_TILE(TY) do { if (T == 16) hipLaunchKernelGGL((pack_conv_tile_kernel<TY, 16, tc>), grid, dim3(256), lds, (hipStream_t)s, p); \
                              else hipLaunchKernelGGL((pack_conv_tile_kernel<TY, 0, tc>), grid, dim3(256), lds, (hipStream_t)s, p); } while (0)
    if (dtype == EG_F32) EG_PACK_TILE(float);
    else if (dtype == EG_F16) EG_PACK_TILE(f16_t);
    else EG_PACK_TILE(bf16_t);
#undef EG_PACK_TILE
    EG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Adam + re-packing in one pass (torch.optim.Adam.step() on a convolution's weight, celebA/EAD-GAN_celebA.py:344,365,400, followed by
// the panel refresh every consumer of the weight needs): the pack_conv_tile tiling with the optimizer update applied while the master
// tile is on its way into LDS -- p, g, m, v are read once, p, m, v written once, both panels written from the tile.
// Same element update as adam_kernel (adam.h), same panel bytes as eg_pack_conv of the updated master, the zeros of the K padding included.
// ------------------------------------------------------------------------------------------------
template <typename T, int TTC, bool V4, int TC>
__global__ __launch_bounds__(256) void adam_pack_conv_tile_kernel(const PackTileParams p, float* __restrict__ w, float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v, float lr, float b1, float b2,
                                                                  float eps, const int* __restrict__ step) {
    constexpr int VEC = Elt<T>::VEC;
    constexpr int TN = 16;
    extern __shared__ float tile[];                 // [TN][TC][T + 1]
    const int TT = TTC ? TTC : p.T, TP = TT + 1;
    const int n0 = blockIdx.x * TN, c0 = blockIdx.y * TC;
    const int tid = threadIdx.x;
    const AdamCoef ac = adam_coef(lr, b1, b2, eps, step);
    if (V4) {
        // 16-byte loads and stores (the four slices are 16-byte aligned and TT is a multiple of 4: a float4 stays inside one (n, c) run),
        // four vectors per thread in flight -- the scalar form below moved 1.2 TB/s, the flat-arena Adam kernel moves 5.9
        const int total4 = TN * TC * TT / 4;
        constexpr int U = TC >= 32 ? 4 : 2;           // vectors per thread in flight (the narrow tile keeps the kernel under 48 registers)
#pragma unroll 1
        for (int e0 = tid; e0 < total4; e0 += U * 256) {
            float4 pi[U], gi[U], mi[U], vi[U];
            size_t idx[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = (e0 + u * 256) * 4;
                const int n = e / (TC * TT), rem = e - n * (TC * TT);
                idx[u] = ((size_t)(n0 + n) * p.Cin + c0) * TT + rem;
                if (e0 + u * 256 < total4) {
                    pi[u] = *reinterpret_cast<const float4*>(w + idx[u]); gi[u] = *reinterpret_cast<const float4*>(g + idx[u]);
                    mi[u] = *reinterpret_cast<const float4*>(m + idx[u]); vi[u] = *reinterpret_cast<const float4*>(v + idx[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (e0 + u * 256 >= total4) continue;
                adam_elem(pi[u].x, gi[u].x, mi[u].x, vi[u].x, ac);
                adam_elem(pi[u].y, gi[u].y, mi[u].y, vi[u].y, ac);
                adam_elem(pi[u].z, gi[u].z, mi[u].z, vi[u].z, ac);
                adam_elem(pi[u].w, gi[u].w, mi[u].w, vi[u].w, ac);
                *reinterpret_cast<float4*>(w + idx[u]) = pi[u];
                *reinterpret_cast<float4*>(m + idx[u]) = mi[u];
                *reinterpret_cast<float4*>(v + idx[u]) = vi[u];
                const int e = (e0 + u * 256) * 4;
                const int n = e / (TC * TT), rem = e - n * (TC * TT);
                const int c = rem / TT, t = rem - c * TT;
                float* tp = tile + (n * TC + c) * TP + t;
                tp[0] = pi[u].x; tp[1] = pi[u].y; tp[2] = pi[u].z; tp[3] = pi[u].w;
            }
        }
    } else
    for (int e = tid; e < TN * TC * TT; e += 256) {
        const int n = e / (TC * TT), rem = e - n * (TC * TT);
        const int c = rem / TT, t = rem - c * TT;
        const size_t i = ((size_t)(n0 + n) * p.Cin + c0) * TT + rem;
        float pi = w[i], mi = m[i], vi = v[i];
        adam_elem(pi, g[i], mi, vi, ac);
        w[i] = pi; m[i] = mi; v[i] = vi;
        tile[(n * TC + c) * TP + t] = pi;
    }
    __syncthreads();
    if (p.wp_fwd) {
        T* dst = reinterpret_cast<T*>(p.wp_fwd);
        const size_t pitch = (size_t)p.pitch_fwd;
        for (int it = tid; it < TN * TT * (TC / VEC); it += 256) {
            const int cg = it % (TC / VEC), r = it / (TC / VEC);
            const int t = r % TT, n = r / TT;
            uint4 ov;
            T* oe = reinterpret_cast<T*>(&ov);
#pragma unroll
            for (int j = 0; j < VEC; ++j) Elt<T>::st(oe + j, tile[(n * TC + cg * VEC + j) * TP + t]);
            *reinterpret_cast<uint4*>(dst + (size_t)(n0 + n) * pitch + (size_t)t * p.Cin + c0 + cg * VEC) = ov;
        }
        // K padding of this tile's TN rows (the workgroups of the first Cin tile write it): K = T * Cin and the pitch are multiples of 32
        // elements, so the 16-byte stores are aligned and cover it exactly
        if (p.pad && blockIdx.y == 0 && p.kfwd < p.pitch_fwd) {
            const int nv = (p.pitch_fwd - p.kfwd) / VEC;
            for (int it = tid; it < TN * nv; it += 256) {
                const int n = it / nv, j = it - n * nv;
                *reinterpret_cast<uint4*>(dst + (size_t)(n0 + n) * pitch + p.kfwd + j * VEC) = make_uint4(0u, 0u, 0u, 0u);
            }
        }
    }
    if (p.wp_bwd) {
        T* dst = reinterpret_cast<T*>(p.wp_bwd);
        for (int it = tid; it < TC * p.nq * (TN / VEC); it += 256) {
            const int ng = it % (TN / VEC), r = it / (TN / VEC);
            const int q = r % p.nq, c = r / p.nq;
            const int t = p.t_of[q];
            uint4 ov;
            T* oe = reinterpret_cast<T*>(&ov);
#pragma unroll
            for (int j = 0; j < VEC; ++j) Elt<T>::st(oe + j, tile[((ng * VEC + j) * TC + c) * TP + t]);
            *reinterpret_cast<uint4*>(dst + p.off[q] + (size_t)(c0 + c) * p.pitch[q] + n0 + ng * VEC) = ov;
        }
        // K padding of this tile's TC rows of every phase panel (the workgroups of the first Cout tile write it): K = taps * Cout is a
        // multiple of 16 elements and the pitch one of 32
        if (p.pad && blockIdx.x == 0)
            for (int ph = 0; ph < p.nph; ++ph) {
                const int nv = (p.ph_pitch[ph] - p.ph_k[ph]) / VEC;
                for (int it = tid; it < TC * nv; it += 256) {
                    const int c = it / nv, j = it - c * nv;
                    *reinterpret_cast<uint4*>(dst + p.ph_off[ph] + (size_t)(c0 + c) * p.ph_pitch[ph] + p.ph_k[ph] + j * VEC) = make_uint4(0u, 0u, 0u, 0u);
                }
            }
    }
}

extern "C" int eg_adam_pack_conv_ok(const eg_conv* c, int dtype, int has_fwd, int has_bwd) {
    PackTileParams p;
    if (!c || (!has_fwd && !has_bwd) || c->k * c->k > 16) return 0;
    return pack_tile_params(c, dtype, has_fwd ? (void*)1 : nullptr, has_bwd ? (void*)1 : nullptr, p, true) ? 1 : 0;
}

extern "C" int eg_adam_pack_conv(const eg_conv* c, int dtype, float* w, float* g, float* m, float* v, float lr, float b1, float b2, float eps,
                                 const int* step, void* wp_fwd, void* wp_bwd, eg_stream_t s) {
    EG_REQUIRE(c && w && g && m && v && step && (wp_fwd || wp_bwd), "eg_adam_pack_conv: null pointer");
    EG_REQUIRE(dtype == EG_F32 || dtype == EG_BF16 || dtype == EG_F16, "dtype must be EG_F32, EG_BF16 or EG_F16");
    const int T = c->k * c->k;
    PackTileParams p;
    EG_REQUIRE(pack_tile_params(c, dtype, wp_fwd, wp_bwd, p, true), "eg_adam_pack_conv: this layer needs the gather kernels (eg_adam_pack_conv_ok() == 0): run eg_adam_step_zero + eg_pack_conv");
    // tile width along Cin: 8 (16-byte panel stores, 8.5 KiB of LDS: fits beside a resident 147-KiB GEMM workgroup, so the update can share
    // CUs with the main chain's convolutions like the LDS-free flat Adam kernel does), not 32 (64-byte stores, 34 KiB)
    constexpr int tc = 8;
    const dim3 grid(c->Cout / 16, c->Cin / tc);
    const size_t lds = (size_t)16 * tc * (T + 1) * sizeof(float);
    const bool v4 = T == 16 && ((((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
#define EG_AP_TILE(TY) do { if (v4) hipLaunchKernelGGL((adam_pack_conv_tile_kernel<TY, 16, true, tc>), grid, dim3(256), lds, (hipStream_t)s, p, w, g, m, v, lr, b1, b2, eps, step); \
                            else if (T == 16) hipLaunchKernelGGL((adam_pack_conv_tile_kernel<TY, 16, false, tc>), grid, dim3(256), lds, (hipStream_t)s, p, w, g, m, v, lr, b1, b2, eps, step); \
                            else hipLaunchKernelGGL((adam_pack_conv_tile_kernel<TY, 0, false, tc>), grid, dim3(256), lds, (hipStream_t)s, p, w, g, m, v, lr, b1, b2, eps, step); } while (0)
    if (dtype == EG_F32) EG_AP_TILE(float); else if (dtype == EG_F16) EG_AP_TILE(f16_t); else EG_AP_TILE(bf16_t);
#undef EG_AP_TILE
    EG_LAUNCH_CHECK();
    return 0;
}

// Adam + re-packing of a weight whose panel is a row-permuted transpose of the master: master w[K][N] (N contiguous; ConvTranspose2d on
// a 1x1 input, celebA/EAD-GAN_celebA.py:76: K = input channels, N = Cout * 16), panel wp[n'][Kpad] with n' = (n % n_mod) * n_mul + n / n_mod
// and k < K (the K padding keeps the zeros of the first eg_pack_strided).  A workgroup takes 32 master rows x 256 columns: coalesced
// reads along N, the update, 16-byte panel stores along K.
template <typename T>
__global__ __launch_bounds__(256) void adam_pack_rows_kernel(float* __restrict__ w, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                             T* __restrict__ wp, int K, int N, int Kpad, int n_mod, int n_mul, float lr, float b1,
                                                             float b2, float eps, const int* __restrict__ step) {
    constexpr int VEC = Elt<T>::VEC;
    constexpr int TK = 8, TNN = 256;                   // 8 KiB of LDS: fits beside a resident GEMM workgroup
    __shared__ float tile[TK][TNN + 1];
    const int k0 = blockIdx.y * TK, n0 = blockIdx.x * TNN;
    const int tid = threadIdx.x;
    const AdamCoef ac = adam_coef(lr, b1, b2, eps, step);
    const int n = n0 + tid;
#pragma unroll 1
    for (int kk = 0; kk < TK; kk += 4) {                 // four rows' loads in flight per thread
        float pi[4], gi[4], mi[4], vi[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + kk + u;
            pi[u] = 0.f; gi[u] = 0.f; mi[u] = 0.f; vi[u] = 0.f;
            if (k < K && n < N) {
                const size_t i = (size_t)k * N + n;
                pi[u] = w[i]; gi[u] = g[i]; mi[u] = m[i]; vi[u] = v[i];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + kk + u;
            if (k < K && n < N) {
                const size_t i = (size_t)k * N + n;
                adam_elem(pi[u], gi[u], mi[u], vi[u], ac);
                w[i] = pi[u]; m[i] = mi[u]; v[i] = vi[u];
            }
            tile[kk + u][tid] = pi[u];
        }
    }
    __syncthreads();
    // panel rows n' of this tile's columns, TK / VEC 16-byte vectors each
    for (int it = tid; it < TNN * (TK / VEC); it += 256) {
        const int kg = it % (TK / VEC), nl = it / (TK / VEC);
        const int n = n0 + nl, kb = k0 + kg * VEC;
        if (n >= N || kb >= K) continue;
        const int np = (n % n_mod) * n_mul + n / n_mod;
        T* dst = wp + (size_t)np * Kpad + kb;
        if (kb + VEC <= K) {
            uint4 ov;
            T* oe = reinterpret_cast<T*>(&ov);
#pragma unroll
            for (int j = 0; j < VEC; ++j) Elt<T>::st(oe + j, tile[kg * VEC + j][nl]);
            *reinterpret_cast<uint4*>(dst) = ov;
        } else {
            for (int j = 0; kb + j < K; ++j) Elt<T>::st(dst + j, tile[kg * VEC + j][nl]);
        }
    }
}

extern "C" int eg_adam_pack_rows(int dtype, float* w, float* g, float* m, float* v, void* wp, int K, int N, int Kpad, int n_mod, int n_mul,
                                 float lr, float b1, float b2, float eps, const int* step, eg_stream_t s) {
    EG_REQUIRE(w && g && m && v && wp && step && K > 0 && N > 0 && Kpad >= K && n_mod > 0 && n_mul > 0 && (N % n_mod) == 0, "eg_adam_pack_rows: bad argument");
    EG_REQUIRE(dtype == EG_F32 || dtype == EG_BF16 || dtype == EG_F16, "dtype must be EG_F32, EG_BF16 or EG_F16");
    EG_REQUIRE((Kpad % vec_of(dtype)) == 0, "eg_adam_pack_rows: Kpad must be a multiple of the 16-byte vector width");
    const dim3 grid(cdiv(N, 256), cdiv(K, 8));
#define EG_APR(TY) hipLaunchKernelGGL((adam_pack_rows_kernel<TY>), grid, dim3(256), 0, (hipStream_t)s, w, g, m, v, (TY*)wp, K, N, Kpad, n_mod, n_mul, lr, b1, b2, eps, step)
    if (dtype == EG_F32) EG_APR(float); else if (dtype == EG_F16) EG_APR(f16_t); else EG_APR(bf16_t);
#undef EG_APR
    EG_LAUNCH_CHECK();
    return 0;
}

// generic strided pack: wp[n][k] = w[(n / n_div) * s_hi + (n % n_div) * s_lo + k * s_k]  (k < K, else 0)
template <typename T>
__device__ __forceinline__ void pack_strided_body(const float* __restrict__ w, T* __restrict__ wp, int N, int K, int Kpad, int n_div, long long s_hi,
                                                  long long s_lo, long long s_k, int bx, int gx) {
    const long long total = (long long)N * Kpad;
    for (long long i = (long long)bx * blockDim.x + threadIdx.x; i < total; i += (long long)gx * blockDim.x) {
        const int n = (int)(i / Kpad), kk = (int)(i % Kpad);
        float v = 0.f;
        if (kk < K) v = w[(n / n_div) * s_hi + (n % n_div) * s_lo + kk * s_k];
        Elt<T>::st(wp + i, v);
    }
}
template <typename T>
__global__ void pack_strided_kernel(const float* __restrict__ w, T* __restrict__ wp, int N, int K, int Kpad, int n_div, long long s_hi,
                                    long long s_lo, long long s_k) {
    pack_strided_body<T>(w, wp, N, K, Kpad, n_div, s_hi, s_lo, s_k, blockIdx.x, gridDim.x);
}

// same with a decomposed column index: + (k / k_div) * s_khi + (k % k_div) * s_klo
template <typename T>
__device__ __forceinline__ void pack_strided2_body(const float* __restrict__ w, T* __restrict__ wp, int N, int K, int Kpad, int n_div, long long s_hi,
                                                   long long s_lo, int k_div, long long s_khi, long long s_klo, int bx, int gx) {
    const long long total = (long long)N * Kpad;
    for (long long i = (long long)bx * blockDim.x + threadIdx.x; i < total; i += (long long)gx * blockDim.x) {
        const int n = (int)(i / Kpad), kk = (int)(i % Kpad);
        float v = 0.f;
        if (kk < K) v = w[(n / n_div) * s_hi + (n % n_div) * s_lo + (kk / k_div) * s_khi + (kk % k_div) * s_klo];
        Elt<T>::st(wp + i, v);
    }
}
template <typename T>
__global__ void pack_strided2_kernel(const float* __restrict__ w, T* __restrict__ wp, int N, int K, int Kpad, int n_div, long long s_hi,
                                     long long s_lo, int k_div, long long s_khi, long long s_klo) {
    pack_strided2_body<T>(w, wp, N, K, Kpad, n_div, s_hi, s_lo, k_div, s_khi, s_klo, blockIdx.x, gridDim.x);
}
extern "C" int eg_pack_strided2(int dtype, const float* w, void* wp, int N, int K, int Kpad, int n_div, long long s_hi, long long s_lo, int k_div,
                                long long s_khi, long long s_klo, eg_stream_t s) {
    EG_REQUIRE(w && wp && N > 0 && K > 0 && Kpad >= K && n_div > 0 && k_div > 0, "eg_pack_strided2: bad argument");
    const long long total = (long long)N * Kpad;
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    if (pack_record_strided(2, dtype, w, wp, N, K, Kpad, n_div, s_hi, s_lo, 0, k_div, s_khi, s_klo, blocks)) return 0;
    if (dtype == EG_F32) hipLaunchKernelGGL(pack_strided2_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, (float*)wp, N, K, Kpad, n_div, s_hi, s_lo, k_div, s_khi, s_klo);
    else if (dtype == EG_F16) hipLaunchKernelGGL(pack_strided2_kernel<f16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, (f16_t*)wp, N, K, Kpad, n_div, s_hi, s_lo, k_div, s_khi, s_klo);
    else hipLaunchKernelGGL(pack_strided2_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, (bf16_t*)wp, N, K, Kpad, n_div, s_hi, s_lo, k_div, s_khi, s_klo);
    EG_LAUNCH_CHECK();
    return 0;
}

extern "C" int eg_pack_strided(int dtype, const float* w, void* wp, int N, int K, int Kpad, int n_div, long long s_hi, long long s_lo,
                               long long s_k, eg_stream_t s) {
    EG_REQUIRE(w && wp && N > 0 && K > 0 && Kpad >= K && n_div > 0, "eg_pack_strided: bad argument");
    const long long total = (long long)N * Kpad;
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    if (pack_record_strided(1, dtype, w, wp, N, K, Kpad, n_div, s_hi, s_lo, s_k, 1, 0, 0, blocks)) return 0;
    if (dtype == EG_F32) hipLaunchKernelGGL(pack_strided_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, (float*)wp, N, K, Kpad, n_div, s_hi, s_lo, s_k);
    else if (dtype == EG_F16) hipLaunchKernelGGL(pack_strided_kernel<f16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, (f16_t*)wp, N, K, Kpad, n_div, s_hi, s_lo, s_k);
    else hipLaunchKernelGGL(pack_strided_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, (bf16_t*)wp, N, K, Kpad, n_div, s_hi, s_lo, s_k);
    EG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Several packs in ONE launch.  The small networks re-pack 7-12 panels per optimizer update, each a 5 us launch of a few workgroups on a
// chain that is launch-bound end to end (dSprites: 46 of 290 launches per iteration).  eg_pack_record_begin() turns the pack entry points
// above into recorders (nothing is launched), eg_pack_record_end() hands the recorded jobs to the caller, who keeps them in device memory;
// eg_pack_multi() runs them: workgroup -> job by the jobs' first-workgroup table, then the SAME body the stand-alone kernel runs.
// ------------------------------------------------------------------------------------------------
struct PackStridedParams {
    const float* w;
    void* wp;
    int N, K, Kpad, n_div, k_div;
    long long s_hi, s_lo, s_k, s_khi, s_klo;
};
struct PackJob {
    int kind;           // 0 gather (pack_kernel), 1 strided, 2 strided2, 3 tile
    int dtype;
    int gx, gy;         // the stand-alone launch's grid
    int block0;         // first workgroup of this job in the joint launch
    int pad;
    union {
        PackParams g;
        PackStridedParams s;
        PackTileParams t;
    };
};
static thread_local std::vector<PackJob>* g_pack_rec = nullptr;

static bool pack_record_gather(const PackParams& p, int dtype, int gx, int gy) {
    if (!g_pack_rec) return false;
    PackJob j;
    memset(&j, 0, sizeof(j));
    j.kind = 0; j.dtype = dtype; j.gx = gx; j.gy = gy; j.g = p;
    g_pack_rec->push_back(j);
    return true;
}
static bool pack_record_strided(int kind, int dtype, const float* w, void* wp, int N, int K, int Kpad, int n_div, long long s_hi, long long s_lo,
                                long long s_k, int k_div, long long s_khi, long long s_klo, int gx) {
    if (!g_pack_rec) return false;
    PackJob j;
    memset(&j, 0, sizeof(j));
    j.kind = kind; j.dtype = dtype; j.gx = gx; j.gy = 1;
    j.s = PackStridedParams{w, wp, N, K, Kpad, n_div, k_div, s_hi, s_lo, s_k, s_khi, s_klo};
    g_pack_rec->push_back(j);
    return true;
}
static bool pack_record_tile(const PackTileParams& p, int dtype, int gx, int gy) {
    if (!g_pack_rec) return false;
    PackJob j;
    memset(&j, 0, sizeof(j));
    j.kind = 3; j.dtype = dtype; j.gx = gx; j.gy = gy; j.t = p;
    g_pack_rec->push_back(j);
    return true;
}

template <typename T>
__device__ __forceinline__ void pack_job_run(const PackJob& j, float* tile, int bx, int by) {
    switch (j.kind) {
        case 0: pack_gather_body<T>(j.g, bx, by, j.gx); break;
        case 1: pack_strided_body<T>(j.s.w, reinterpret_cast<T*>(j.s.wp), j.s.N, j.s.K, j.s.Kpad, j.s.n_div, j.s.s_hi, j.s.s_lo, j.s.s_k, bx, j.gx); break;
        case 2: pack_strided2_body<T>(j.s.w, reinterpret_cast<T*>(j.s.wp), j.s.N, j.s.K, j.s.Kpad, j.s.n_div, j.s.s_hi, j.s.s_lo, j.s.k_div, j.s.s_khi, j.s.s_klo, bx, j.gx); break;
        default:
            if (j.t.T == 16) pack_conv_tile_body<T, 16, EG_PACKM_TC>(j.t, tile, bx, by);
            else pack_conv_tile_body<T, 0, EG_PACKM_TC>(j.t, tile, bx, by);
    }
}

// (tile jobs 16 x 8 channels x taps: 8.5 KiB of LDS and 33 VGPRs -- the joint launch fits on a CU beside a resident 8-wave GEMM workgroup,
//  like the per-element pack kernels it replaces did; the stand-alone tile kernel's 16 x 32 tile needs 34 KiB)
__global__ __launch_bounds__(256) void pack_multi_kernel(const PackJob* __restrict__ jobs, int njobs) {
    __shared__ float tile[16 * EG_PACKM_TC * 17];
    int ji = 0;
    while (ji + 1 < njobs && (int)blockIdx.x >= jobs[ji + 1].block0) ++ji;      // (uniform: scalar loads)
    const PackJob& j = jobs[ji];
    const int local = blockIdx.x - j.block0, bx = local % j.gx, by = local / j.gx;
    if (j.dtype == EG_F32) pack_job_run<float>(j, tile, bx, by);
    else if (j.dtype == EG_F16) pack_job_run<f16_t>(j, tile, bx, by);
    else pack_job_run<bf16_t>(j, tile, bx, by);
}

extern "C" int eg_pack_record_begin(void) {
    EG_REQUIRE(!g_pack_rec, "eg_pack_record_begin: already recording");
    g_pack_rec = new std::vector<PackJob>();
    return 0;
}
extern "C" size_t eg_pack_job_bytes(void) { return sizeof(PackJob); }
/* ends the recording; copies the jobs (eg_pack_job_bytes() each) into host memory `jobs_out` of `cap_bytes` bytes; *njobs / *nblocks: what
 * eg_pack_multi wants back together with a DEVICE copy of jobs_out */
extern "C" int eg_pack_record_end(void* jobs_out, size_t cap_bytes, int* njobs, int* nblocks) {
    EG_REQUIRE(g_pack_rec, "eg_pack_record_end: not recording");
    std::vector<PackJob>* rec = g_pack_rec;
    g_pack_rec = nullptr;
    int nb = 0;
    for (PackJob& j : *rec) { j.block0 = nb; nb += j.gx * j.gy; }
    const size_t need = rec->size() * sizeof(PackJob);
    const bool ok = jobs_out && njobs && nblocks && need <= cap_bytes;
    if (ok) {
        memcpy(jobs_out, rec->data(), need);
        *njobs = (int)rec->size();
        *nblocks = nb;
    }
    delete rec;
    EG_REQUIRE(ok, "eg_pack_record_end: the job table does not fit (or null argument)");
    return 0;
}
extern "C" int eg_pack_multi(const void* jobs_dev, int njobs, int nblocks, eg_stream_t s) {
    EG_REQUIRE(jobs_dev && njobs > 0 && nblocks > 0, "eg_pack_multi: bad argument");
    hipLaunchKernelGGL(pack_multi_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)s, reinterpret_cast<const PackJob*>(jobs_dev), njobs);
    EG_LAUNCH_CHECK();
    return 0;
}
