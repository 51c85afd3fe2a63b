// Sliced Wasserstein distance between two image sets (Karras et al., "Progressive Growing of GANs", 2018 -- not in the reference,
// whose scripts have no image-quality number): the device side of quality.py.
//   eg_pyr_down / eg_pyr_up_sub   one level of the Laplacian pyramid: 5 x 5 binomial filter, mirror border (i < 0 -> -i, i >= n -> 2(n-1) - i)
//   eg_swd_patch_stats            per channel mean and population std of all gathered 7 x 7 patch pixels of a level (double), and the flag
//   eg_swd_unit_columns           directions made unit length
//   eg_swd_project                gather 7 x 7 x C patches and project them on D directions with the normalisation folded into the
//                                 directions; the descriptors (0.6 GB per set and level at full size) never exist
//   eg_sort_columns_f32           bitonic column sort, all compare-exchanges ascending, so that +inf padding never has to be stored
//   eg_l1_mean_f32                mean |a - b| of two sorted arrays in double
// No float atomics anywhere: every sum has a fixed order, two runs give the same bits.
#include "eg_common.h"

static inline size_t cdivz(size_t a, size_t b) { return (a + b - 1) / b; }
__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// ---- Laplacian pyramid ------------------------------------------------------------------------------------------------------------
// binomial taps in units of 1/16 per axis: the products tap_y * tap_x * pixel are accumulated with fma and scaled by an exact power of two
#define PYR_TAPS constexpr float PYR_TAP[5] = {1.f, 4.f, 6.f, 4.f, 1.f}

// out[p][y][x] = sum_ab g[a][b] in[p][mirror(2y + a - 2)][mirror(2x + b - 2)], in H x H, out H/2 x H/2
__global__ __launch_bounds__(256) void pyr_down_kernel(const float* __restrict__ in, float* __restrict__ out, int planes, int H) {
    const int h = H >> 1;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)planes * h * h) return;
    const int x = (int)(i % h), y = (int)((i / h) % h);
    const float* src = in + (i / ((size_t)h * h)) * (size_t)H * H;
    PYR_TAPS;
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const float* row = src + (size_t)mirror(2 * y + a - 2, H) * H;
#pragma unroll
        for (int b = 0; b < 5; ++b) acc = fmaf(PYR_TAP[a] * PYR_TAP[b], row[mirror(2 * x + b - 2, H)], acc);
    }
    out[i] = acc * (1.f / 256.f);
}

// fine[p][y][x] -= sum_ab 4 g[a][b] z[mirror(y + a - 2)][mirror(x + b - 2)], z = coarse written into the even positions of a zero image of
// the fine size H: only taps that land on even rows and columns contribute (at most 3 x 3)
__global__ __launch_bounds__(256) void pyr_up_sub_kernel(float* __restrict__ fine, const float* __restrict__ coarse, int planes, int H) {
    const int h = H >> 1;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)planes * H * H) return;
    const int x = (int)(i % H), y = (int)((i / H) % H);
    const float* src = coarse + (i / ((size_t)H * H)) * (size_t)h * h;
    PYR_TAPS;
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const int yy = mirror(y + a - 2, H);
        if (yy & 1) continue;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const int xx = mirror(x + b - 2, H);
            if (xx & 1) continue;
            acc = fmaf(PYR_TAP[a] * PYR_TAP[b], src[(size_t)(yy >> 1) * h + (xx >> 1)], acc);
        }
    }
    fine[i] = fine[i] - acc * (1.f / 64.f);
}

extern "C" int eg_pyr_down(const float* fine, float* coarse, int planes, int H, eg_stream_t s) {
    EG_REQUIRE(fine && coarse && planes > 0, "eg_pyr_down: bad argument");
    EG_REQUIRE(H >= 32 && ilog2_exact(H) > 0 && (size_t)planes * H * H < ((size_t)1 << 40), "eg_pyr_down: the side must be a power of two >= 32");
    const size_t n = (size_t)planes * (H / 2) * (H / 2);
    hipLaunchKernelGGL(pyr_down_kernel, dim3((unsigned)cdivz(n, 256)), dim3(256), 0, (hipStream_t)s, fine, coarse, planes, H);
    EG_LAUNCH_CHECK();
    return 0;
}

extern "C" int eg_pyr_up_sub(float* fine, const float* coarse, int planes, int H, eg_stream_t s) {
    EG_REQUIRE(fine && coarse && planes > 0, "eg_pyr_up_sub: bad argument");
    EG_REQUIRE(H >= 32 && ilog2_exact(H) > 0 && (size_t)planes * H * H < ((size_t)1 << 40), "eg_pyr_up_sub: the fine side must be a power of two >= 32");
    const size_t n = (size_t)planes * H * H;
    hipLaunchKernelGGL(pyr_up_sub_kernel, dim3((unsigned)cdivz(n, 256)), dim3(256), 0, (hipStream_t)s, fine, coarse, planes, H);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- patch statistics --------------------------------------------------------------------------------------------------------------
#define SWD_PATCH 7
#define SWD_PIX 49
#define SWD_STAT_BLOCKS 256
enum { SWD_FLAG_ZERO_STD = 1, SWD_FLAG_NONFINITE = 2, SWD_FLAG_POSITION = 4 };

// a centre outside [3, H - 3) is flagged by the statistics pass and read clamped: no launch reads outside the image
__device__ __forceinline__ int clamp_centre(int v, int H) { return v < 3 ? 3 : (v > H - 4 ? H - 4 : v); }

// fixed-order block sum of doubles (blockDim.x = 256); result in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* sm /* 256 */) {
    __syncthreads();
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    return sm[0];
}

// part[(c * nblocks + block) * 3 + {0, 1, 2}] = sum (v - pivot), sum (v - pivot)^2, number of out-of-range centres; pivot = the channel's first gathered
// pixel (a shift leaves mean and variance what they are and keeps sum of squares minus square of sum from cancelling)
__global__ __launch_bounds__(256) void patch_stats_partial_kernel(const float* __restrict__ img, const int* __restrict__ pos, int n_desc, int P, int C,
                                                                   int H, double* __restrict__ part) {
    __shared__ double sm[256];
    const int c = blockIdx.y;
    const float* first = img + ((size_t)c * H + clamp_centre(pos[0], H) - 3) * H + clamp_centre(pos[1], H) - 3;
    const double pivot = (double)first[0];
    double s1 = 0.0, s2 = 0.0, bad = 0.0;
    for (int d = blockIdx.x * 256 + threadIdx.x; d < n_desc; d += gridDim.x * 256) {
        const int py = pos[2 * d], px = pos[2 * d + 1];
        const int y = clamp_centre(py, H), x = clamp_centre(px, H);
        if (y != py || x != px) bad += 1.0;
        const float* p = img + (((size_t)(d / P) * C + c) * H + y - 3) * H + x - 3;
        for (int dy = 0; dy < SWD_PATCH; ++dy)
            for (int dx = 0; dx < SWD_PATCH; ++dx) {
                const double v = (double)p[(size_t)dy * H + dx] - pivot;
                s1 += v;
                s2 = fma(v, v, s2);
            }
    }
    s1 = block_sum_f64(s1, sm);
    s2 = block_sum_f64(s2, sm);
    bad = block_sum_f64(bad, sm);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)c * gridDim.x + blockIdx.x) * 3;
        o[0] = s1; o[1] = s2; o[2] = bad;
    }
}

__global__ __launch_bounds__(256) void patch_stats_final_kernel(const float* __restrict__ img, const int* __restrict__ pos, const double* __restrict__ part,
                                                                 int nblocks, int n_desc, int C, int H, double* __restrict__ stats, int* __restrict__ flag) {
    __shared__ double sm[256];
    const int c = blockIdx.x;
    double s1 = 0.0, s2 = 0.0, bad = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        const double* o = part + ((size_t)c * nblocks + i) * 3;
        s1 += o[0]; s2 += o[1]; bad += o[2];
    }
    s1 = block_sum_f64(s1, sm);
    s2 = block_sum_f64(s2, sm);
    bad = block_sum_f64(bad, sm);
    if (threadIdx.x == 0) {
        const float* first = img + ((size_t)c * H + clamp_centre(pos[0], H) - 3) * H + clamp_centre(pos[1], H) - 3;
        const double n = (double)n_desc * SWD_PIX, m = s1 / n;
        double var = s2 / n - m * m;
        if (var < 0.0) var = 0.0;
        const double mean = (double)first[0] + m, sd = sqrt(var);
        stats[2 * c] = mean;
        stats[2 * c + 1] = sd;
        int f = 0;
        if (!(fabs(mean) <= 1.7976931348623157e308) || !(fabs(sd) <= 1.7976931348623157e308)) f |= SWD_FLAG_NONFINITE;
        else if (sd == 0.0) f |= SWD_FLAG_ZERO_STD;
        if (bad != 0.0) f |= SWD_FLAG_POSITION;
        if (f) atomicOr(flag, f);               // integer: channels of one launch and launches of one stream may all set bits
    }
}

extern "C" size_t eg_swd_patch_stats_ws_doubles(int C) { return (size_t)(C > 0 ? C : 0) * SWD_STAT_BLOCKS * 3; }

extern "C" int eg_swd_patch_stats(const float* img, const int* pos, int n_desc, int P, int C, int H, double* ws, double* stats, int* flag, eg_stream_t s) {
    EG_REQUIRE(img && pos && ws && stats && flag, "eg_swd_patch_stats: null pointer");
    EG_REQUIRE(n_desc > 0 && P > 0 && n_desc % P == 0 && C >= 1 && C <= 4 && H >= 7, "eg_swd_patch_stats: need n_desc a positive multiple of P, 1 <= C <= 4, H >= 7");
    const int nb = (int)(cdivz(n_desc, 256) < SWD_STAT_BLOCKS ? cdivz(n_desc, 256) : SWD_STAT_BLOCKS);
    hipLaunchKernelGGL(patch_stats_partial_kernel, dim3(nb, C), dim3(256), 0, (hipStream_t)s, img, pos, n_desc, P, C, H, ws);
    hipLaunchKernelGGL(patch_stats_final_kernel, dim3(C), dim3(256), 0, (hipStream_t)s, img, pos, ws, nb, n_desc, C, H, stats, flag);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- directions ---------------------------------------------------------------------------------------------------------------------
// W [K][D]: every column divided by its Euclidean norm (formed in double, one thread per column)
__global__ void unit_columns_kernel(float* __restrict__ W, int K, int D) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    double ss = 0.0;
    for (int k = 0; k < K; ++k) ss = fma((double)W[(size_t)k * D + d], (double)W[(size_t)k * D + d], ss);
    const double inv = 1.0 / sqrt(ss);
    for (int k = 0; k < K; ++k) W[(size_t)k * D + d] = (float)((double)W[(size_t)k * D + d] * inv);
}

extern "C" int eg_swd_unit_columns(float* W, int K, int D, eg_stream_t s) {
    EG_REQUIRE(W && K > 0 && D > 0, "eg_swd_unit_columns: bad argument");
    hipLaunchKernelGGL(unit_columns_kernel, dim3(cdiv(D, 64)), dim3(64), 0, (hipStream_t)s, W, K, D);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- projection ---------------------------------------------------------------------------------------------------------------------
#define PRJ_TM 128         // descriptors per workgroup
#define PRJ_TN 128         // directions per workgroup (D <= 128: one column tile)

// wf[k][d] = W[k][d] / std[k / 49] for d < D, 0 up to PRJ_TN; wf[K][d] = sum_k (W[k][d] / std) * mean, formed in double, rounded once
__global__ void project_fold_kernel(const float* __restrict__ W, const double* __restrict__ stats, int K, int D, float* __restrict__ wf) {
    const int d = threadIdx.x;
    double cst = 0.0;
    for (int k = 0; k < K; ++k) {
        const int c = k / SWD_PIX;
        const float w = d < D ? (float)((double)W[(size_t)k * D + d] / stats[2 * c + 1]) : 0.f;
        wf[(size_t)k * PRJ_TN + d] = w;
        cst = fma((double)w, stats[2 * c], cst);
    }
    wf[(size_t)K * PRJ_TN + d] = (float)cst;
}

// out[d][i] = sum_k wf[k][d] * patch_i[k] - wf[K][d]; k = c * 49 + dy * 7 + dx.  128 x 128 tile per workgroup, 8 x 8 per thread as two 4-wide
// halves 64 apart in both directions; one channel (49 k) of patches and directions staged in LDS per step.  fp32 operands, fma chain in k order.
__global__ __launch_bounds__(256) void project_kernel(const float* __restrict__ img, const int* __restrict__ pos, int n_desc, int P, int C, int H,
                                                       const float* __restrict__ wf, int D, float* __restrict__ out, size_t ld, int vec) {
    __shared__ float As[SWD_PIX][PRJ_TM];
    __shared__ float Bs[SWD_PIX][PRJ_TN];
    __shared__ int base[PRJ_TM];              // offset of the patch's first pixel in channel 0, -1 past the end
    const int tid = threadIdx.x, ty = tid & 15, tx = tid >> 4;
    const int d0 = blockIdx.x * PRJ_TM;
    if (tid < PRJ_TM) {
        const int d = d0 + tid;
        int b = -1;
        if (d < n_desc) b = (clamp_centre(pos[2 * d], H) - 3) * H + clamp_centre(pos[2 * d + 1], H) - 3;
        base[tid] = b;
    }
    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    const size_t plane = (size_t)H * H;
    for (int c = 0; c < C; ++c) {
        __syncthreads();
        for (int e = tid; e < SWD_PIX * PRJ_TM; e += 256) {
            const int m = e & (PRJ_TM - 1), k = e >> 7;
            const int b = base[m];
            float v = 0.f;
            if (b >= 0) v = img[((size_t)((d0 + m) / P) * C + c) * plane + b + (k / SWD_PATCH) * H + (k % SWD_PATCH)];
            As[k][m] = v;
        }
        for (int e = tid; e < SWD_PIX * PRJ_TN; e += 256) Bs[e >> 7][e & (PRJ_TN - 1)] = wf[(size_t)c * SWD_PIX * PRJ_TN + e];
        __syncthreads();
#pragma unroll 7
        for (int k = 0; k < SWD_PIX; ++k) {
            const float4 a0 = *(const float4*)&As[k][ty * 4], a1 = *(const float4*)&As[k][64 + ty * 4];
            const float4 b0 = *(const float4*)&Bs[k][tx * 4], b1 = *(const float4*)&Bs[k][64 + tx * 4];
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
    }
    const float* cst = wf + (size_t)C * SWD_PIX * PRJ_TN;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int d = (j < 4 ? 0 : 64) + tx * 4 + (j & 3);
        if (d >= D) continue;
        const float k0 = cst[d];
#pragma unroll
        for (int i = 0; i < 8; i += 4) {
            const int m = d0 + (i < 4 ? 0 : 64) + ty * 4;
            float* o = out + (size_t)d * ld + m;
            if (vec && m + 3 < n_desc) {
                *(float4*)o = make_float4(acc[i][j] - k0, acc[i + 1][j] - k0, acc[i + 2][j] - k0, acc[i + 3][j] - k0);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (m + u < n_desc) o[u] = acc[i + u][j] - k0;
            }
        }
    }
}

extern "C" size_t eg_swd_project_ws_floats(int C) { return (size_t)((C > 0 ? C : 0) * SWD_PIX + 1) * PRJ_TN; }

extern "C" int eg_swd_project(const float* img, const int* pos, int n_desc, int P, int C, int H, const float* dirs, int D, const double* stats, float* ws,
                              float* out, size_t ld, eg_stream_t s) {
    EG_REQUIRE(img && pos && dirs && stats && ws && out, "eg_swd_project: null pointer");
    EG_REQUIRE(n_desc > 0 && P > 0 && n_desc % P == 0 && C >= 1 && C <= 4 && H >= 7 && H <= 16384, "eg_swd_project: need n_desc a positive multiple of P, 1 <= C <= 4, 7 <= H <= 16384");
    EG_REQUIRE(D >= 1 && D <= PRJ_TN && ld >= (size_t)n_desc, "eg_swd_project: need 1 <= D <= 128 and ld >= n_desc");
    hipLaunchKernelGGL(project_fold_kernel, dim3(1), dim3(PRJ_TN), 0, (hipStream_t)s, dirs, stats, C * SWD_PIX, D, ws);
    hipLaunchKernelGGL(project_kernel, dim3(cdiv(n_desc, PRJ_TM)), dim3(256), 0, (hipStream_t)s, img, pos, n_desc, P, C, H, ws, D, out, ld,
                       (int)(((uintptr_t)out & 15) == 0 && (ld & 3) == 0));
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- column sort --------------------------------------------------------------------------------------------------------------------
// Bitonic network in the form whose compare-exchanges all point the same way: the merge of two sorted runs of length K / 2 starts with the
// "flip" step (i against its mirror image in the block of K, i ^ (K - 1)) and goes on with the strides K / 4, K / 8 ... 1 (i against
// i ^ stride).  Every exchange leaves the smaller value at the lower index, so the +inf that pads a column to a power of two never moves
// below index n: a pair whose upper index is >= n is skipped and the padding is never stored.
//   sort_tile_kernel      all merge rounds up to K = T inside one workgroup (LDS and registers), one tile of T elements each
//   sort_global4_kernel   two consecutive steps with stride >= T in one pass (four elements per thread, closed under both steps)
//   sort_global2_kernel   one such step
//   sort_tile_kernel again, `merge` form: the strides T / 2 ... 1 of a round K > T in one LDS pass
#define SORT_T 8192
#define SORT_THREADS 512
#define SORT_E (SORT_T / SORT_THREADS)          // 16 consecutive elements per thread in the register phases

__device__ __forceinline__ void cmpx(float& a, float& b) {
    if (a > b) { const float t = a; a = b; b = t; }
}

// strides FROM, FROM / 2 ... 1 of the network on 16 values in registers (all indices are compile-time constants)
template <int FROM>
__device__ __forceinline__ void reg_strides(float (&v)[SORT_E]) {
#pragma unroll
    for (int st = FROM; st > 0; st >>= 1)
#pragma unroll
        for (int p = 0; p < SORT_E / 2; ++p) {
            const int i = ((p & ~(st - 1)) << 1) | (p & (st - 1));
            cmpx(v[i], v[i + st]);
        }
}
template <int K>
__device__ __forceinline__ void reg_round(float (&v)[SORT_E]) {          // merge round K <= 16: flip, then the strides K / 4 ... 1
#pragma unroll
    for (int p = 0; p < SORT_E / 2; ++p) {
        const int h = K >> 1, i = ((p & ~(h - 1)) << 1) | (p & (h - 1));
        cmpx(v[i], v[i ^ (K - 1)]);
    }
    if constexpr (K >= 4) reg_strides<K / 4>(v);
}
__device__ __forceinline__ void reg_load(float (&v)[SORT_E], const float* sm) {
#pragma unroll
    for (int q = 0; q < SORT_E / 4; ++q) {
        const float4 t = *(const float4*)(sm + threadIdx.x * SORT_E + 4 * q);
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
}
__device__ __forceinline__ void reg_store(const float (&v)[SORT_E], float* sm) {
#pragma unroll
    for (int q = 0; q < SORT_E / 4; ++q) *(float4*)(sm + threadIdx.x * SORT_E + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
// one compare-exchange step over the tile in LDS, stride st >= SORT_E
__device__ __forceinline__ void lds_stride(float* sm, int st) {
    for (int p = threadIdx.x; p < SORT_T / 2; p += SORT_THREADS) {
        const int i = ((p & ~(st - 1)) << 1) | (p & (st - 1));
        cmpx(sm[i], sm[i + st]);
    }
    __syncthreads();
}

// full: 1 = sort the tile (every merge round up to T); 0 = only the strides T / 2 ... 1 (the tail of a round above T).  A thread owns SORT_E = 16
// consecutive elements: the rounds up to 16 and the strides 8 ... 1 of every later round run in its registers (one LDS read and write of the
// tile instead of four), the flip steps and the strides >= 16 as compare-exchanges in LDS.  Rounds above the column's padded length only
// move +inf, so the tile is always sorted whole.
__global__ __launch_bounds__(SORT_THREADS) void sort_tile_kernel(float* __restrict__ x, int n, size_t ld, int full) {
    __shared__ __attribute__((aligned(16))) float sm[SORT_T];
    float* col = x + (size_t)blockIdx.y * ld;
    const int t0 = blockIdx.x * SORT_T;
    for (int i = threadIdx.x; i < SORT_T; i += SORT_THREADS) sm[i] = t0 + i < n ? col[t0 + i] : INFINITY;
    __syncthreads();
    float v[SORT_E];
    if (full) {
        reg_load(v, sm);
        reg_round<2>(v); reg_round<4>(v); reg_round<8>(v); reg_round<16>(v);
        reg_store(v, sm);
        __syncthreads();
        for (int K = 2 * SORT_E; K <= SORT_T; K <<= 1) {
            for (int p = threadIdx.x; p < SORT_T / 2; p += SORT_THREADS) {           // flip
                const int h = K >> 1, i = ((p & ~(h - 1)) << 1) | (p & (h - 1));
                cmpx(sm[i], sm[i ^ (K - 1)]);
            }
            __syncthreads();
            for (int st = K >> 2; st >= SORT_E; st >>= 1) lds_stride(sm, st);
            reg_load(v, sm);
            reg_strides<SORT_E / 2>(v);
            reg_store(v, sm);
            __syncthreads();
        }
    } else {
        for (int st = SORT_T >> 1; st >= SORT_E; st >>= 1) lds_stride(sm, st);
        reg_load(v, sm);
        reg_strides<SORT_E / 2>(v);
        reg_store(v, sm);
        __syncthreads();
    }
    for (int i = threadIdx.x; i < SORT_T; i += SORT_THREADS)
        if (t0 + i < n) col[t0 + i] = sm[i];
}

// one step over the whole column: flip of blocks of K (flip = 1) or stride st = K / 2 (flip = 0); pair index p < npad / 2
__global__ __launch_bounds__(256) void sort_global2_kernel(float* __restrict__ x, int n, size_t ld, int npad, int K, int flip) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (npad >> 1)) return;
    float* col = x + (size_t)blockIdx.y * ld;
    const int h = K >> 1, i = ((p & ~(h - 1)) << 1) | (p & (h - 1)), j = flip ? (i ^ (K - 1)) : i + h;
    if (j >= n) return;
    float a = col[i], b = col[j];
    if (a > b) { col[i] = b; col[j] = a; }
}

// two steps in one pass.  flip = 1: flip of blocks of K, then stride q = K / 4; flip = 0: stride K / 2, then stride q = K / 4.  The four elements
// e0 < e1 < e2 < e3 of a thread: e0 has the bits K / 2 and q clear, e1 = e0 + q; stride form e2 = e0 + K / 2, e3 = e2 + q, first step
// (e0, e2), (e1, e3); flip form e2 = mirror(e1), e3 = mirror(e0), first step (e0, e3), (e1, e2); second step (e0, e1), (e2, e3) in both
__global__ __launch_bounds__(256) void sort_global4_kernel(float* __restrict__ x, int n, size_t ld, int npad, int K, int flip) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (npad >> 2)) return;
    float* col = x + (size_t)blockIdx.y * ld;
    const int q = K >> 2;
    const int e0 = ((p & ~(q - 1)) << 2) | (p & (q - 1)), e1 = e0 + q;
    const int e2 = flip ? (e1 ^ (K - 1)) : e0 + (K >> 1), e3 = flip ? (e0 ^ (K - 1)) : e2 + q;
    if (e1 >= n) return;                    // every pair of this thread has its upper index in the padding
    float v0 = col[e0], v1 = col[e1];
    float v2 = e2 < n ? col[e2] : INFINITY, v3 = e3 < n ? col[e3] : INFINITY;
    if (flip) { cmpx(v0, v3); cmpx(v1, v2); }
    else { cmpx(v0, v2); cmpx(v1, v3); }
    cmpx(v0, v1); cmpx(v2, v3);
    col[e0] = v0; col[e1] = v1;
    if (e2 < n) col[e2] = v2;
    if (e3 < n) col[e3] = v3;
}

extern "C" int eg_sort_tile_elems(void) { return SORT_T; }

extern "C" int eg_sort_columns_f32(float* x, int n, int cols, size_t ld, eg_stream_t s) {
    EG_REQUIRE(x && n >= 1 && cols >= 1 && cols <= 65535 && ld >= (size_t)n, "eg_sort_columns_f32: need n >= 1, 1 <= cols <= 65535, ld >= n");
    EG_REQUIRE(n <= (1 << 30), "eg_sort_columns_f32: at most 2^30 elements per column");
    int npad = 1;
    while (npad < n) npad <<= 1;
    const hipStream_t st = (hipStream_t)s;
    const int tiles = cdiv(n, SORT_T);
    if (npad >= 2) hipLaunchKernelGGL(sort_tile_kernel, dim3(tiles, cols), dim3(SORT_THREADS), 0, st, x, n, ld, 1);
    for (int K = 2 * SORT_T; K <= npad && K > 0; K <<= 1) {
        // steps of this round with a stride >= T: flip(K), then strides K / 4 ... T (as the block size 2 * stride: K / 2 ... 2 T)
        int blk = K, flip = 1;
        while (blk >= 2 * SORT_T) {
            const int next = blk >> 1;                             // block size of the step after this one
            if (next >= 2 * SORT_T) {                              // this step and the next one in one pass
                hipLaunchKernelGGL(sort_global4_kernel, dim3(cdiv(npad >> 2, 256), cols), dim3(256), 0, st, x, n, ld, npad, blk, flip);
                blk = next >> 1;
            } else {
                hipLaunchKernelGGL(sort_global2_kernel, dim3(cdiv(npad >> 1, 256), cols), dim3(256), 0, st, x, n, ld, npad, blk, flip);
                blk = next;
            }
            flip = 0;
        }
        hipLaunchKernelGGL(sort_tile_kernel, dim3(tiles, cols), dim3(SORT_THREADS), 0, st, x, n, ld, 0);
    }
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- L1 distance of two sorted arrays ---------------------------------------------------------------------------------------------------
#define L1_BLOCKS 1024
__global__ __launch_bounds__(256) void l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, int cols, size_t ld,
                                                          double* __restrict__ part) {
    __shared__ double sm[256];
    const size_t total = (size_t)n * cols;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t o = (i / n) * ld + (i % n);
        acc += (double)fabsf(a[o] - b[o]);
    }
    acc = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void l1_final_kernel(const double* __restrict__ part, int nb, double count, double* __restrict__ out) {
    __shared__ double sm[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
    acc = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) out[0] = acc / count;
}

extern "C" size_t eg_l1_mean_ws_doubles(void) { return L1_BLOCKS; }

extern "C" int eg_l1_mean_f32(const float* a, const float* b, int n, int cols, size_t ld, double* ws, double* out, eg_stream_t s) {
    EG_REQUIRE(a && b && ws && out && n >= 1 && cols >= 1 && ld >= (size_t)n, "eg_l1_mean_f32: bad argument");
    const size_t total = (size_t)n * cols;
    const int nb = (int)(cdivz(total, 1024) < L1_BLOCKS ? cdivz(total, 1024) : L1_BLOCKS);
    hipLaunchKernelGGL(l1_partial_kernel, dim3(nb), dim3(256), 0, (hipStream_t)s, a, b, n, cols, ld, ws);
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, ws, nb, (double)total, out);
    EG_LAUNCH_CHECK();
    return 0;
}
