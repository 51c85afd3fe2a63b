// What follows a weight-gradient launch: the reduction of igemm_tn's partial slabs into the master-layout gradient (+ the spectral-norm
// correction), and the bias-gradient column sums.
#include <algorithm>

#include "eg_common.h"
#include "conv_geom.h"

// This file is compiled with -ffp-contract=off (Makefile), like the file it was split from.

// ------------------------------------------------------------------------------------------------
// slab reduction into the master-layout gradient (+ spectral-norm correction)
// ------------------------------------------------------------------------------------------------
#define EG_SN_NPART 1024

// One block per (n, chunk of 64 gathered channels): reads the [t][c] slab rows coalesced along c, sums the splits, subtracts
// the rank-1 spectral-norm terms, transposes through LDS and read-modify-writes the master-layout gradient [n][c][t] as
// one contiguous run of 64*T floats.  MODE 0: out (+)= a; MODE 1: out = a (gtmp) + <a,W> partials; MODE 2: out (+)= a - rank1.
// `accumulate` (uniform, MODES 0 and 2): 1 = read-modify-write, 0 = store -- the first writer of a gradient slot in a backward pass stores
// the very value it would have added to a cleared slot and never reads the slot.
#define EG_RC 64
// LEAN: the instantiation for launches with < 16 splits (every big layer: 2-8 slabs): no split-group scratch (4.4 KiB of LDS instead of
// 24) and four loads in flight instead of eight (<= 48 VGPRs) -- its workgroups then fit on a CU beside a resident 8-wave GEMM workgroup
// (147 KiB of LDS, 2 x 232 VGPRs per SIMD lane), so a reduction forked beside the main chain's GEMMs no longer waits for their tiles to
// retire.  Same summation order as the eight-deep loop (one add per slab, in slab order): same bits.
template <int MODE, bool LEAN = false>
__global__ __launch_bounds__(LEAN ? 256 : 1024) void wgrad_reduce_kernel(const float* __restrict__ slab, int nsplit, int NS, int N, int C, int T,
                                                           float* __restrict__ out, int accumulate, const float* __restrict__ w_orig,
                                                           float* __restrict__ partials, int ntapes, const float* __restrict__ coef,
                                                           const float* __restrict__ u, const float* __restrict__ v, int row_div, int row_mul, int c_row) {
    extern __shared__ float tile[];      // [EG_RC][T+1]
    __shared__ float sm[16];
    const int cchunks = (C + EG_RC - 1) / EG_RC;
    const int n = blockIdx.x / cchunks, c0 = (blockIdx.x % cchunks) * EG_RC;
    const int cw = min(EG_RC, C - c0);
    const size_t split_stride = (size_t)NS * T * C;
    float un[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE == 2)
        for (int q = 0; q < ntapes; ++q) un[q] = coef[q] * u[(size_t)q * N + n];
    const int crow = c_row ? c_row : C;                 // row length of the destination (<= C when the slab is column padded)
    const int nv = T * (EG_RC / 4);                     // float4 elements of a full tile
    const int NTH = blockDim.x;                          // 256, or 1024 for the many-split form (the host picks)
    if (!LEAN && cw == EG_RC && c0 + EG_RC <= crow && (C & 3) == 0 && nv * 2 <= NTH && nsplit >= 16) {
        // many splits of a small tile (the image-side layers as 1x1 convolutions: T = 1, 128 splits; the 32- and 64-channel layers of the
        // small networks: one 64 x 16 tile per output channel, 128 splits): the loop below is a chain of nsplit loads per thread with most
        // of the chip idle.  Here blockDim / nv thread groups each take every (blockDim / nv)-th split, eight loads in flight, and the
        // groups are added in group order through LDS (deterministic).
        __shared__ float4 part[1024];
        const int G = NTH / nv, e4 = threadIdx.x % nv, sg = threadIdx.x / nv;
        const int t = e4 / (EG_RC / 4), c = (e4 % (EG_RC / 4)) * 4;
        const size_t si = ((size_t)n * T + t) * C + c0 + c;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sg < G) {
            int z = sg;
            for (; z + 7 * G < nsplit; z += 8 * G) {
                float4 x[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) x[q] = *reinterpret_cast<const float4*>(slab + (size_t)(z + q * G) * split_stride + si);
#pragma unroll
                for (int q = 0; q < 8; ++q) { a.x += x[q].x; a.y += x[q].y; a.z += x[q].z; a.w += x[q].w; }
            }
            for (; z < nsplit; z += G) {
                const float4 x = *reinterpret_cast<const float4*>(slab + (size_t)z * split_stride + si);
                a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
            }
        }
        part[threadIdx.x] = a;
        __syncthreads();
        if (threadIdx.x < nv) {
            a = part[threadIdx.x];
            for (int gq = 1; gq < G; ++gq) { const float4 x = part[gq * nv + threadIdx.x]; a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w; }
            if (MODE == 2)
                for (int q = 0; q < ntapes; ++q) {
                    const float* vq = v + (size_t)q * crow * T + (size_t)(c0 + c) * T + t;
                    a.x -= un[q] * vq[0]; a.y -= un[q] * vq[T]; a.z -= un[q] * vq[2 * T]; a.w -= un[q] * vq[3 * T];
                }
            tile[c * (T + 1) + t] = a.x; tile[(c + 1) * (T + 1) + t] = a.y; tile[(c + 2) * (T + 1) + t] = a.z; tile[(c + 3) * (T + 1) + t] = a.w;
        }
    } else if (cw == EG_RC && c0 + EG_RC <= crow && (C & 3) == 0) {
        // full 64-channel block: 16-byte loads along the channels (one float4 per thread and slab for k = 4), same summation order
        for (int e4 = threadIdx.x; e4 < T * (EG_RC / 4); e4 += NTH) {
            const int t = e4 / (EG_RC / 4), c = (e4 % (EG_RC / 4)) * 4;
            const size_t si = ((size_t)n * T + t) * C + c0 + c;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            // eight (LEAN: four) slabs' loads in flight, added in slab order (the sum's order is unchanged: bit-identical to the one-by-one
            // loop; a thread owns ONE float4 of the tile, so without this the loop is a chain of nsplit exposed HBM latencies)
            constexpr int DEPTH = LEAN ? 4 : 8;
            int z = 0;
            for (; z + DEPTH <= nsplit; z += DEPTH) {
                float4 x[DEPTH];
#pragma unroll
                for (int q = 0; q < DEPTH; ++q) x[q] = *reinterpret_cast<const float4*>(slab + (size_t)(z + q) * split_stride + si);
#pragma unroll
                for (int q = 0; q < DEPTH; ++q) { a.x += x[q].x; a.y += x[q].y; a.z += x[q].z; a.w += x[q].w; }
            }
            for (; z < nsplit; ++z) {
                const float4 x = *reinterpret_cast<const float4*>(slab + z * split_stride + si);
                a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
            }
            if (MODE == 2 && !LEAN) {
#pragma unroll 1
                for (int q = 0; q < ntapes; ++q) {
                    const float* vq = v + (size_t)q * crow * T + (size_t)(c0 + c) * T + t;
                    a.x -= un[q] * vq[0]; a.y -= un[q] * vq[T]; a.z -= un[q] * vq[2 * T]; a.w -= un[q] * vq[3 * T];
                }
            }
            tile[c * (T + 1) + t] = a.x; tile[(c + 1) * (T + 1) + t] = a.y; tile[(c + 2) * (T + 1) + t] = a.z; tile[(c + 3) * (T + 1) + t] = a.w;
        }
    } else if (!LEAN && nsplit >= 16 && T * EG_RC * 2 <= NTH) {
        // many splits of a small tile whose channel count is not a multiple of 64 (the image-side layers: 48 = 3 x 16 gathered channels,
        // 128 splits): the loop below is ONE chain of nsplit dependent loads per thread (39 us for a 6 K-parameter gradient, at the end
        // of every sub-step's backward pass).  As above: thread groups take every G-th split, eight loads in flight, added in group order.
        __shared__ float parts[1024];
        const int ne = T * EG_RC, G = min(NTH / ne, 16), e = threadIdx.x % ne, sg = threadIdx.x / ne;
        const int t = e / EG_RC, cc = e % EG_RC;
        const bool valid = cc < cw && c0 + cc < crow;
        const size_t si = ((size_t)n * T + t) * C + c0 + cc;
        float a = 0.f;
        if (sg < G && valid) {
            int z = sg;
            for (; z + 7 * G < nsplit; z += 8 * G) {
                float x[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) x[q] = slab[(size_t)(z + q * G) * split_stride + si];
#pragma unroll
                for (int q = 0; q < 8; ++q) a += x[q];
            }
            for (; z < nsplit; z += G) a += slab[(size_t)z * split_stride + si];
        }
        parts[threadIdx.x] = a;
        __syncthreads();
        if (threadIdx.x < ne && valid) {
            a = parts[threadIdx.x];
            for (int gq = 1; gq < G; ++gq) a += parts[gq * ne + threadIdx.x];
            if (MODE == 2)
                for (int q = 0; q < ntapes; ++q) a -= un[q] * v[(size_t)q * crow * T + (size_t)(c0 + cc) * T + t];
            tile[cc * (T + 1) + t] = a;
        }
    } else
    for (int e = threadIdx.x; e < T * EG_RC; e += NTH) {
        const int t = e / EG_RC, c = e % EG_RC;
        if (c < cw && c0 + c < crow) {
            const size_t si = ((size_t)n * T + t) * C + c0 + c;
            float a = 0.f;
            for (int z = 0; z < nsplit; ++z) a += slab[z * split_stride + si];
            if (MODE == 2 && !LEAN)
                for (int q = 0; q < ntapes; ++q) a -= un[q] * v[(size_t)q * crow * T + (size_t)(c0 + c) * T + t];
            tile[c * (T + 1) + t] = a;
        }
    }
    __syncthreads();
    float dot = 0.f;
    const int nout = row_div ? (n % row_div) * row_mul + n / row_div : n;
    const size_t obase = ((size_t)nout * crow + c0) * T;
    const int cwo = min(cw, crow - c0);
    for (int e = threadIdx.x; e < cwo * T; e += NTH) {
        const int c = e / T, t = e % T;
        float a = tile[c * (T + 1) + t];
        if (MODE == 2 && LEAN) {
            // the rank-1 spectral-norm terms here, on the way out: v[q][(c0 + c) * T + t] is v_q[c0 * T + e] -- contiguous along e (the
            // load phase gathers it with stride T); the same subtractions in the same order on the same values -> the same bits
#pragma unroll 1
            for (int q = 0; q < ntapes; ++q) a -= un[q] * v[(size_t)q * crow * T + (size_t)c0 * T + e];
        }
        if (MODE == 1) {
            out[obase + e] = a;
            dot += a * w_orig[obase + e];
        } else {
            out[obase + e] = accumulate ? out[obase + e] + a : a;
        }
    }
    if (MODE == 1) {
        const float tot = block_sum(dot, sm);
        if (threadIdx.x == 0) partials[blockIdx.x] = tot;
    }
}

__global__ void sn_grad_apply_kernel(const float* __restrict__ gtmp, const float* __restrict__ partials, int npart,
                                     const float* __restrict__ sigma, const float* __restrict__ u, const float* __restrict__ v,
                                     long long total, int Kdim, float* __restrict__ grad, int accumulate) {
    __shared__ float sm[16];
    float d = 0.f;
    for (int i = threadIdx.x; i < npart; i += blockDim.x) d += partials[i];
    const float dot = block_sum(d, sm);
    const float sg = sigma[0];
    const float inv = 1.f / sg, coef = dot / (sg * sg);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(i / Kdim), kk = (int)(i % Kdim);
        const float a = gtmp[i] * inv - coef * u[n] * v[kk];
        grad[i] = accumulate ? grad[i] + a : a;
    }
}

static inline int reduce_blocks(int n_rows, int C) {
    return n_rows * ((C + EG_RC - 1) / EG_RC);
}
// threads per workgroup: 1024 (several split groups per tile vector) where a launch has many splits and few, small tiles
static inline int reduce_threads(int nsplit, int n_rows, int C, int T) {
    const int nv = T * (EG_RC / 4);
    return (nsplit >= 16 && nv * 2 <= 1024 && nv * 2 > 256 && reduce_blocks(n_rows, C) <= 2048) ? 1024 : 256;
}
static inline size_t reduce_lds(int T) { return (size_t)EG_RC * (T + 1) * sizeof(float); }
static inline bool reduce_lean(int nsplit) { return nsplit < 16; }

extern "C" int eg_wgrad_reduce(const float* slab, int nsplit, int n_slab, int n_rows, int C, int T, float* grad, int accumulate, eg_stream_t s) {
    EG_REQUIRE(slab && grad && nsplit > 0 && n_rows <= n_slab && T > 0 && T <= 64, "eg_wgrad_reduce: bad argument");
    if (reduce_lean(nsplit))
        hipLaunchKernelGGL((wgrad_reduce_kernel<0, true>), dim3(reduce_blocks(n_rows, C)), dim3(256), reduce_lds(T), (hipStream_t)s, slab, nsplit, n_slab, n_rows, C, T,
                           grad, accumulate, (const float*)nullptr, (float*)nullptr, 0, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0, 0, 0);
    else
    hipLaunchKernelGGL(wgrad_reduce_kernel<0>, dim3(reduce_blocks(n_rows, C)), dim3(reduce_threads(nsplit, n_rows, C, T)), reduce_lds(T), (hipStream_t)s, slab, nsplit, n_slab, n_rows, C, T,
                       grad, accumulate, (const float*)nullptr, (float*)nullptr, 0, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0, 0, 0);
    EG_LAUNCH_CHECK();
    return 0;
}

extern "C" int eg_wgrad_reduce_perm(const float* slab, int nsplit, int n_slab, int n_rows, int C, int T, float* grad, int row_div, int row_mul, int c_row,
                                    int accumulate, eg_stream_t s) {
    EG_REQUIRE(slab && grad && nsplit > 0 && n_rows <= n_slab && T > 0 && T <= 64 && row_div >= 0 && c_row >= 0 && c_row <= C, "eg_wgrad_reduce_perm: bad argument");
    hipLaunchKernelGGL(wgrad_reduce_kernel<0>, dim3(reduce_blocks(n_rows, C)), dim3(reduce_threads(nsplit, n_rows, C, T)), reduce_lds(T), (hipStream_t)s, slab, nsplit, n_slab, n_rows, C, T,
                       grad, accumulate != 0, (const float*)nullptr, (float*)nullptr, 0, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, row_div, row_mul, c_row);
    EG_LAUNCH_CHECK();
    return 0;
}

extern "C" int eg_wgrad_reduce_rank1(const float* slab, int nsplit, int n_slab, int n_rows, int C, int T, float* grad, int ntapes,
                                     const float* coef, const float* u, const float* v, int c_row, int accumulate, eg_stream_t s) {
    EG_REQUIRE(slab && grad && nsplit > 0 && n_rows <= n_slab && ntapes >= 0 && ntapes <= 4 && (ntapes == 0 || (coef && u && v)) && T > 0 && T <= 64,
               "eg_wgrad_reduce_rank1: bad argument");
    if (reduce_lean(nsplit))
        hipLaunchKernelGGL((wgrad_reduce_kernel<2, true>), dim3(reduce_blocks(n_rows, C)), dim3(256), reduce_lds(T), (hipStream_t)s, slab, nsplit, n_slab, n_rows, C, T,
                           grad, accumulate != 0, (const float*)nullptr, (float*)nullptr, ntapes, coef, u, v, 0, 0, c_row);
    else
    hipLaunchKernelGGL(wgrad_reduce_kernel<2>, dim3(reduce_blocks(n_rows, C)), dim3(reduce_threads(nsplit, n_rows, C, T)), reduce_lds(T), (hipStream_t)s, slab, nsplit, n_slab, n_rows, C, T,
                       grad, accumulate != 0, (const float*)nullptr, (float*)nullptr, ntapes, coef, u, v, 0, 0, c_row);
    EG_LAUNCH_CHECK();
    return 0;
}

extern "C" int eg_sn_partials(void) { return 1 << 17; }

extern "C" int eg_wgrad_reduce_sn(const eg_conv* c, const float* slab, int nsplit, const float* w_orig, const float* sigma,
                                  const float* u, const float* v, float* gtmp, float* partials, float* grad, int accumulate, eg_stream_t s) {
    EG_REQUIRE(c && slab && w_orig && sigma && u && v && gtmp && partials && grad && nsplit > 0, "eg_wgrad_reduce_sn: bad argument");
    const int T = c->k * c->k;
    const int blocks = reduce_blocks(c->Cout, c->Cin);
    EG_REQUIRE(blocks <= (1 << 17), "eg_wgrad_reduce_sn: layer too large for the partials buffer");
    hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3(blocks), dim3(256), reduce_lds(T), (hipStream_t)s, slab, nsplit, c->Cout, c->Cout, c->Cin, T, gtmp, 0,
                       w_orig, partials, 0, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0, 0, 0);
    const long long total = (long long)c->Cout * c->Cin * T;
    const int blocks2 = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
    hipLaunchKernelGGL(sn_grad_apply_kernel, dim3(blocks2), dim3(256), 0, (hipStream_t)s, gtmp, partials, blocks, sigma, u, v, total,
                       c->Cin * T, grad, accumulate != 0);
    EG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// bias gradient: column sums of a [rows][N] tensor (two deterministic stages)
// ------------------------------------------------------------------------------------------------
// rows per workgroup: 256, halved (down to 16) until the launch has >= 512 workgroups -- the head layers have few rows (B*16) of
// 1024 columns, where 256-row blocks left 8-24 workgroups walking a dependent-load chain
static int bg_rpb(int rows_per_group, int ngroups, int gx) {
    int rpb = 256;
    while (rpb > 16 && (long long)gx * ngroups * cdiv(rows_per_group, rpb) < 512) rpb >>= 1;
    return rpb;
}
static int bg_gx(int N, int dtype) {
    const int cpr = N / (dtype == EG_F32 ? 4 : 8);
    return cdiv(cpr, cpr < 256 ? cpr : 256);
}

// block = 256 threads = (N/VEC chunk columns) x (row lanes); 16-byte loads; LDS combine of the row lanes
template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ x, int rows, int N, int rpb, float* __restrict__ partials) {
    constexpr int VEC = Elt<T>::VEC;
    __shared__ float sm[256 * VEC];
    const int cpr = N / VEC;                       // chunks per row (host guarantees cpr <= 256 and 256 % cpr == 0 via tiling in x)
    const int ccols = cpr < 256 ? cpr : 256;
    const int lanes = 256 / ccols;
    const int cj = threadIdx.x % ccols, rl = threadIdx.x / ccols;
    const int chunk = blockIdx.x * ccols + cj;
    const int r0 = blockIdx.y * rpb, r1 = min(rows, r0 + rpb);
    float a[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) a[j] = 0.f;
    if (chunk < cpr)
        for (int r = r0 + rl; r < r1; r += lanes) {
            const uint4 v = *reinterpret_cast<const uint4*>(x + (size_t)r * N + (size_t)chunk * VEC);
            const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) a[j] += Elt<T>::ld(e + j);
        }
#pragma unroll
    for (int j = 0; j < VEC; ++j) sm[threadIdx.x * VEC + j] = a[j];
    __syncthreads();
    if (rl == 0 && chunk < cpr) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            float t = 0.f;
            for (int l = 0; l < lanes; ++l) t += sm[(l * ccols + cj) * VEC + j];
            partials[(size_t)blockIdx.y * N + (size_t)chunk * VEC + j] = t;
        }
    }
}

// gb[j] (+)= scale * sum_{n == j mod nb} sum_r partials[r][n]; one wave per output j
__global__ void colsum_final_kernel(const float* __restrict__ partials, int nrb, int N, int nb, const float* __restrict__ scale, float* __restrict__ gb,
                                    int accumulate) {
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= nb) return;
    float a = 0.f;
    for (int n = j; n < N; n += nb)
        for (int r = lane; r < nrb; r += 64) a += partials[(size_t)r * N + n];
    a = wave_sum(a);
    if (lane == 0) {
        const float t = a * (scale ? scale[0] : 1.f);
        gb[j] = accumulate ? gb[j] + t : t;
    }
}

extern "C" size_t eg_bias_grad_ws_floats(int rows, int N) {
    // bound for every launch with <= rows rows and <= N columns, either dtype: bg_rpb stops halving once there are 512 workgroups, so
    // a launch has at most max(rows / 256, 1024) row blocks
    return (size_t)std::max(cdiv(rows, 256), 1024) * N;
}

extern "C" int eg_bias_grad(int dtype, const void* dY, int rows, int N, int bias_mod, float* partials, float* gb, int accumulate, eg_stream_t s) {
    EG_REQUIRE(dY && partials && gb && rows > 0 && N > 0, "eg_bias_grad: bad argument");
    const int vecw = dtype == EG_F32 ? 4 : 8;
    EG_REQUIRE(N % vecw == 0, "eg_bias_grad: N must be a multiple of the 16-byte vector width");
    const int cpr = N / vecw;
    const int ccols = cpr < 256 ? cpr : 256;
    EG_REQUIRE(256 % ccols == 0, "eg_bias_grad: N/vec must divide 256 or be a multiple of it");
    const int rpb = bg_rpb(rows, 1, cdiv(cpr, ccols));
    const int nrb = cdiv(rows, rpb);
    dim3 grid(cdiv(cpr, ccols), nrb);
    if (dtype == EG_F32) hipLaunchKernelGGL(colsum_partial_kernel<float>, grid, dim3(256), 0, (hipStream_t)s, (const float*)dY, rows, N, rpb, partials);
    else if (dtype == EG_F16) hipLaunchKernelGGL(colsum_partial_kernel<f16_t>, grid, dim3(256), 0, (hipStream_t)s, (const f16_t*)dY, rows, N, rpb, partials);
    else hipLaunchKernelGGL(colsum_partial_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)s, (const bf16_t*)dY, rows, N, rpb, partials);
    const int nb = bias_mod > 0 ? bias_mod : N;
    hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(nb, 4)), dim3(256), 0, (hipStream_t)s, partials, nrb, N, nb, (const float*)nullptr, gb, accumulate != 0);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- tape-segmented bias gradient + <G,W>/sigma^2 coefficient from activations (spectrally normalised layers) --------
template <typename T>
__global__ __launch_bounds__(256) void colsum_sn_partial_kernel(const T* __restrict__ x, const T* __restrict__ act, const float* __restrict__ bias,
                                                                int N, int rows_per_tape, int blocks_per_tape, int rpb, float inv_slope,
                                                                float* __restrict__ partials, float* __restrict__ dots) {
    constexpr int VEC = Elt<T>::VEC;
    __shared__ float sm[256 * VEC];
    __shared__ float smd[16];
    const int cpr = N / VEC;
    const int ccols = cpr < 256 ? cpr : 256;
    const int lanes = 256 / ccols;
    const int cj = threadIdx.x % ccols, rl = threadIdx.x / ccols;
    const int chunk = blockIdx.x * ccols + cj;
    const int tape = blockIdx.y / blocks_per_tape, blk = blockIdx.y % blocks_per_tape;
    const int r0 = tape * rows_per_tape + blk * rpb;
    const int r1 = min(tape * rows_per_tape + rows_per_tape, r0 + rpb);
    float a[VEC], bv[VEC];
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) { a[j] = 0.f; bv[j] = (chunk < cpr) ? bias[chunk * VEC + j] : 0.f; }
    if (chunk < cpr)
        for (int r = r0 + rl; r < r1; r += lanes) {
            const size_t o = (size_t)r * N + (size_t)chunk * VEC;
            const uint4 v = *reinterpret_cast<const uint4*>(x + o);
            const uint4 w = *reinterpret_cast<const uint4*>(act + o);
            const T* e = reinterpret_cast<const T*>(&v);
            const T* ae = reinterpret_cast<const T*>(&w);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float g = Elt<T>::ld(e + j);
                float z = Elt<T>::ld(ae + j);
                z = z > 0.f ? z : z * inv_slope;
                a[j] += g;
                dot += g * (z - bv[j]);
            }
        }
#pragma unroll
    for (int j = 0; j < VEC; ++j) sm[threadIdx.x * VEC + j] = a[j];
    const float dtot = block_sum(dot, smd);      // contains the __syncthreads that also publishes sm
    if (rl == 0 && chunk < cpr) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            float t = 0.f;
            for (int l = 0; l < lanes; ++l) t += sm[(l * ccols + cj) * VEC + j];
            partials[(size_t)blockIdx.y * N + (size_t)chunk * VEC + j] = t;
        }
    }
    if (threadIdx.x == 0) dots[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = dtot;
}

// gb[n] (+)= sum_rb sigma[tape(rb)] * partials[rb][n]   (one wave per n);  coef[t] = sum of the tape's dot partials (block z)
__global__ void colsum_sn_final_kernel(const float* __restrict__ partials, const float* __restrict__ dots, int nrb, int N, int blocks_per_tape,
                                       int ndot_per_rb, int ntapes, const float* __restrict__ sigma, float* __restrict__ gb, float* __restrict__ coef,
                                       int accumulate) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j < N) {
        float a = 0.f;
        for (int r = lane; r < nrb; r += 64) a += partials[(size_t)r * N + j] * sigma[r / blocks_per_tape];
        a = wave_sum(a);
        if (lane == 0) gb[j] = accumulate ? gb[j] + a : a;
    } else if (j < N + ntapes) {
        const int t = j - N;
        float a = 0.f;
        const int n = blocks_per_tape * ndot_per_rb;
        for (int r = lane; r < n; r += 64) a += dots[(size_t)t * n + r];
        a = wave_sum(a);
        if (lane == 0) coef[t] = a;
    }
}

extern "C" size_t eg_bias_grad_sn_ws_floats(int rows, int N, int rows_per_tape) {
    // same bound as eg_bias_grad_ws_floats (row blocks over all tapes), plus the per-block dot partials
    const int ntapes = rows / rows_per_tape;
    return (size_t)std::max(ntapes * cdiv(rows_per_tape, 256), 1024 + ntapes) * (N + 64);
}

extern "C" int eg_bias_grad_sn(int dtype, const void* dzs, const void* a, const float* bias, int rows, int N, int rows_per_tape,
                               const float* sigma, float slope, float* ws, float* gb, float* coef, int accumulate, eg_stream_t s) {
    EG_REQUIRE(dzs && a && bias && sigma && ws && gb && coef && rows_per_tape > 0 && rows % rows_per_tape == 0 && slope > 0.f, "eg_bias_grad_sn: bad argument");
    const int vecw = dtype == EG_F32 ? 4 : 8;
    EG_REQUIRE(N % vecw == 0, "eg_bias_grad_sn: N must be a multiple of the 16-byte vector width");
    const int cpr = N / vecw;
    const int ccols = cpr < 256 ? cpr : 256;
    EG_REQUIRE(256 % ccols == 0, "eg_bias_grad_sn: N/vec must divide 256 or be a multiple of it");
    const int ntapes = rows / rows_per_tape;
    EG_REQUIRE(ntapes <= 4, "eg_bias_grad_sn: at most 4 tapes");
    const int gx = cdiv(cpr, ccols);
    const int rpb = bg_rpb(rows_per_tape, ntapes, gx);
    const int bpt = cdiv(rows_per_tape, rpb);
    const int nrb = ntapes * bpt;
    float* partials = ws;
    float* dots = ws + (size_t)nrb * N;
    dim3 grid(gx, nrb);
    if (dtype == EG_F32) hipLaunchKernelGGL(colsum_sn_partial_kernel<float>, grid, dim3(256), 0, (hipStream_t)s, (const float*)dzs, (const float*)a, bias, N, rows_per_tape, bpt, rpb, 1.f / slope, partials, dots);
    else if (dtype == EG_F16) hipLaunchKernelGGL(colsum_sn_partial_kernel<f16_t>, grid, dim3(256), 0, (hipStream_t)s, (const f16_t*)dzs, (const f16_t*)a, bias, N, rows_per_tape, bpt, rpb, 1.f / slope, partials, dots);
    else hipLaunchKernelGGL(colsum_sn_partial_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)s, (const bf16_t*)dzs, (const bf16_t*)a, bias, N, rows_per_tape, bpt, rpb, 1.f / slope, partials, dots);
    hipLaunchKernelGGL(colsum_sn_final_kernel, dim3(cdiv(N + ntapes, 4)), dim3(256), 0, (hipStream_t)s, partials, dots, nrb, N, bpt, gx, ntapes, sigma, gb, coef, accumulate != 0);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- the same sums from the epilogue of the convolution that produced dzs (eg_epilogue.stat_mode = EG_STAT_SN_BIAS) -----------------
// stat: [N][nrb] column sums, then [nrb][tiles_n] tile dots.  gb[n] (+)= sum_rb sigma[tape(rb)] * stat[n][rb] (one wave per n, contiguous
// reads); coef[t] = sum of the dots of tape t's row blocks (waves N .. N + ntapes - 1).  tape(rb) = (rb % tiles_m) / tiles_per_tape.
// WIDE: one 256-thread workgroup per sum instead of one wave (>= 1024 row blocks: the small networks' 32 / 64-channel layers at B = 128 .. 512
// have up to 12288 of them; one wave walked 192 partials per lane with an integer division each: 25 us per launch in the colored dSprites step);
// fewer row blocks keep the wave form and its bits
template <bool WIDE>
__global__ void colsum_sn_final_t_kernel(const float* __restrict__ stat, int nrb, int N, int tiles_m, int tiles_per_tape, int tiles_n, int ntapes,
                                         const float* __restrict__ sigma, float* __restrict__ gb, float* __restrict__ coef, int accumulate) {
    __shared__ float sh[4];
    const int lane = WIDE ? threadIdx.x : threadIdx.x & 63, step = WIDE ? 256 : 64;
    const int j = WIDE ? blockIdx.x : blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    float acc = 0.f;
    if (j < N) {
        const float* __restrict__ a = stat + (size_t)j * nrb;
        for (int r = lane; r < nrb; r += step) acc += a[r] * sigma[(r % tiles_m) / tiles_per_tape];
    } else if (j < N + ntapes) {
        const int t = j - N;
        const float* __restrict__ dots = stat + (size_t)N * nrb;
        for (int r = lane; r < nrb; r += step)
            if ((r % tiles_m) / tiles_per_tape == t)
                for (int q = 0; q < tiles_n; ++q) acc += dots[(size_t)r * tiles_n + q];
    } else if (!WIDE) {
        return;
    }
    acc = wave_sum(acc);
    if (WIDE) {
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
        __syncthreads();
        acc = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    }
    if (lane != 0) return;
    if (j < N) gb[j] = accumulate ? gb[j] + acc : acc;
    else if (j < N + ntapes) coef[j - N] = acc;
}

extern "C" int eg_bias_grad_sn_fused(const float* stat, int nrb, int N, int tiles_m, int tiles_per_tape, int ntapes, const float* sigma, float* gb,
                                     float* coef, int accumulate, eg_stream_t s) {
    EG_REQUIRE(stat && sigma && gb && coef && nrb > 0 && N > 0 && ((N % 128) == 0 || N == 64 || N == 32) && tiles_m > 0 && (nrb % tiles_m) == 0 &&
               tiles_per_tape > 0 && ntapes > 0 && ntapes <= 4 && tiles_per_tape * ntapes == tiles_m, "eg_bias_grad_sn_fused: bad argument");
    // (column tiles of the producing launch: 128 wide for the 8-wave kernels, the whole row for the register-staged kernel's N = 32 / 64)
    if (nrb >= 1024)
        hipLaunchKernelGGL(colsum_sn_final_t_kernel<true>, dim3(N + ntapes), dim3(256), 0, (hipStream_t)s, stat, nrb, N, tiles_m, tiles_per_tape,
                           N >= 128 ? N / 128 : 1, ntapes, sigma, gb, coef, accumulate != 0);
    else
        hipLaunchKernelGGL(colsum_sn_final_t_kernel<false>, dim3(cdiv(N + ntapes, 4)), dim3(256), 0, (hipStream_t)s, stat, nrb, N, tiles_m, tiles_per_tape,
                           N >= 128 ? N / 128 : 1, ntapes, sigma, gb, coef, accumulate != 0);
    EG_LAUNCH_CHECK();
    return 0;
}
