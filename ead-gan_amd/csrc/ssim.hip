// Structural similarity between PAIRS of uint8 images (not in the reference): the device half of quality.ssim, ms_ssim, psnr,
// reconstruction and diversity.  The contract, restated in tests/ssim_refs.py with plain numpy slicing, for pair p = (i, j):
//   levels   x_l[y][x] = 4^-l (integer sum of the 2^l x 2^l block of bytes), side H_l = H >> l, l = 0 .. L - 1 (exact in fp64)
//   moments  mu_a, mu_b, E_aa, E_bb, E_ab of x, y, x^2, y^2, x y:  sum_dy win[dy] sum_dx win[dx] (.)[r + dy][q + dx]  over the valid
//            positions 0 <= r, q <= n_l - 1, n_l = H_l - K + 1: rows first, then columns, every sum in index order, fp64, the products exact
//   values   cs = (2 s_ab + c2) / (s_aa + s_bb + c2), lum = (2 mu_a mu_b + c1) / (mu_a^2 + mu_b^2 + c1), ssim = lum cs
//   stats[p][l] = (mean ssim, mean cs) over channels and positions, sse[p] = sum (a - b)^2 over the bytes, an exact integer.
// The window is the caller's table: this file evaluates no exp.
//
// ssim_kernel<K>: ONE workgroup per pair.  The pair's bytes are staged once into LDS (2 C H^2 bytes; sse is summed from the staged words)
// and the coarser levels are built there as uint16 block sums (<= 255 * 4^4 < 2^16), each from the level above it.  An element becomes a
// double by one exact v_add_f64: the integer in the mantissa of 2^(52 - 2 l) minus that constant is k 4^-l, no convert and no multiply.
// A TASK is one output column q of one (level, channel), numbered level-major (l, then c, then q); thread t takes the tasks t, t + threads,
// ... (82 per channel at H = 64, K = 11, L = 3: all three levels of three channels run side by side on 246 threads).  The thread walks down
// its column: per input row the five row-filtered values of (row, q .. q + K - 1) on K taps, which it scatters into the K pending output
// rows it keeps in registers (K x 5 doubles; the row loop is unrolled K times so that every slot is a fixed register) -- a row's
// contributions reach an output in dy order -- and the row that completes is turned into (ssim, cs) and added to the thread's two sums.
// The five row-filtered planes never exist.  Summation order: a column's rows in row order in its thread; then per level the C n_l column
// sums (c, then q) by one wave, lane k adding the columns k, k + 64, ..., the 64 lane sums meeting in a fixed xor tree.  Nothing crosses
// a workgroup and there are no atomics: the bits of pair p depend on its two images, win, c1, c2, K and L alone.
// LDS at C = 3, H = 64, K = 11, L = 3: 3936 (column sums) + 32 + 24 576 (bytes) + 15 360 (levels 1, 2) = 43 904 bytes;
// the largest case (C = 4, H = 64, K = 3, L = 5) takes 61 856.
#include <math.h>

#include "eg_common.h"

#define SS_THREADS 256
#define SS_MAX_C 4
#define SS_MAX_K 11
#define SS_MAX_L 5
#define SS_FLAG_PAIR 2
#define SS_CHUNK (1 << 22)          // pairs a launch: blocks x threads stays below 2^32

// the K-tap walk down one output column of one plane: pa, pb point at element [0][q] of the two H_l x H_l planes
template <int K, typename T>
__device__ __forceinline__ void ssim_column(const T* __restrict__ pa, const T* __restrict__ pb, int Hl, int l, const double (&w)[K], double c1,
                                            double c2, double& ssim_sum, double& cs_sum) {
    const int hi = (1075 - 2 * l) << 20;                   // the exponent of 2^(52 - 2 l): its mantissa counts units of 4^-l
    const double magic = __hiloint2double(hi, 0);
    double acc[K][5];                                      // slot (r mod K): the pending moments of output row r
#pragma unroll
    for (int s = 0; s < K; ++s)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[s][m] = 0.0;
    double ss = 0.0, cs = 0.0;
    for (int y0 = 0; y0 < Hl; y0 += K) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int y = y0 + j;
            if (y < Hl) {
                const T* ra = pa + y * Hl;
                const T* rb = pb + y * Hl;
                double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;
#pragma unroll
                for (int dx = 0; dx < K; ++dx) {
                    const double u = __hiloint2double(hi, (int)ra[dx]) - magic;
                    const double v = __hiloint2double(hi, (int)rb[dx]) - magic;
                    t0 = fma(w[dx], u, t0);
                    t1 = fma(w[dx], v, t1);
                    t2 = fma(w[dx], u * u, t2);
                    t3 = fma(w[dx], v * v, t3);
                    t4 = fma(w[dx], u * v, t4);
                }
#pragma unroll
                for (int dy = 0; dy < K; ++dy) {           // row y is tap dy of output row y - dy
                    const int s = (j - dy + K) % K;
                    acc[s][0] = fma(w[dy], t0, acc[s][0]);
                    acc[s][1] = fma(w[dy], t1, acc[s][1]);
                    acc[s][2] = fma(w[dy], t2, acc[s][2]);
                    acc[s][3] = fma(w[dy], t3, acc[s][3]);
                    acc[s][4] = fma(w[dy], t4, acc[s][4]);
                }
                const int s = (j + 1) % K;                 // output row y - K + 1 has its last tap
                if (y >= K - 1) {
                    const double ma = acc[s][0], mb = acc[s][1];
                    const double saa = acc[s][2] - ma * ma, sbb = acc[s][3] - mb * mb, sab = acc[s][4] - ma * mb;
                    const double c = (2.0 * sab + c2) / (saa + sbb + c2);
                    const double lum = (2.0 * ma * mb + c1) / (ma * ma + mb * mb + c1);
                    ss += lum * c;
                    cs += c;
                }
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[s][m] = 0.0;
            }
        }
    }
    ssim_sum = ss;
    cs_sum = cs;
}

template <int K>
__global__ __launch_bounds__(SS_THREADS) void ssim_kernel(const unsigned char* __restrict__ a, int na, const unsigned char* __restrict__ b, int nb,
                                                          int C, int H, const int* __restrict__ pairs, long long p0, const double* __restrict__ win,
                                                          int L, int tasks, double c1, double c2, double* __restrict__ stats,
                                                          long long* __restrict__ sse, int* __restrict__ flag) {
    extern __shared__ double ss_lds[];
    const int t = threadIdx.x, nt = blockDim.x;
    const size_t p = (size_t)p0 + blockIdx.x;
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    if ((unsigned)i >= (unsigned)na || (unsigned)j >= (unsigned)nb) {        // uniform over the workgroup: nothing is read
        for (int k = t; k < 2 * L; k += nt) stats[p * (size_t)(2 * L) + k] = __longlong_as_double(0x7ff8000000000000ll);
        if (t == 0) {
            sse[p] = -1;
            flag[0] = SS_FLAG_PAIR;
        }
        return;
    }
    const int HW = H * H, CHW = C * HW;
    double* colsum = ss_lds;                                                 // [tasks][2]
    unsigned long long* wsse = (unsigned long long*)(colsum + 2 * tasks);    // [4]: the waves' sums of squared differences
    unsigned char* la = (unsigned char*)(wsse + 4);                          // [C][H][H]
    unsigned char* lb = la + CHW;
    uint16_t* lv = (uint16_t*)(lb + CHW);                                    // levels 1 .. L - 1: a's planes [C][H_l][H_l], then b's

    // the bytes, and sse on the way (<= 255^2 * 16384 < 2^32 per workgroup)
    const uint32_t* ga = (const uint32_t*)(a + (size_t)i * CHW);
    const uint32_t* gb = (const uint32_t*)(b + (size_t)j * CHW);
    unsigned long long sq = 0;
    for (int k = t; k < CHW / 4; k += nt) {
        const uint32_t x = ga[k], y = gb[k];
        ((uint32_t*)la)[k] = x;
        ((uint32_t*)lb)[k] = y;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = (int)((x >> (8 * q)) & 255u) - (int)((y >> (8 * q)) & 255u);
            sq += (unsigned)(d * d);
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) sq += __shfl_xor(sq, d);
    if ((t & 63) == 0) wsse[t >> 6] = sq;
    __syncthreads();

    // the coarser levels: integer 2 x 2 sums of the level above
    int off = 0, prev = 0;
    for (int l = 1; l < L; ++l) {
        const int Hl = H >> l, Hp = Hl * 2, plane = Hl * Hl, half = C * plane;
        for (int k = t; k < 2 * half; k += nt) {
            const int img = k / half, r = k - img * half, c = r / plane, yx = r - c * plane, y = yx / Hl, x = yx - y * Hl;
            unsigned v;
            if (l == 1) {
                const unsigned char* s = (img ? lb : la) + c * HW + (2 * y) * H + 2 * x;
                v = (unsigned)s[0] + s[1] + s[H] + s[H + 1];
            } else {
                const uint16_t* s = lv + prev + (img * C + c) * (Hp * Hp) + (2 * y) * Hp + 2 * x;
                v = (unsigned)s[0] + s[1] + s[Hp] + s[Hp + 1];
            }
            lv[off + k] = (uint16_t)v;
        }
        prev = off;
        off += 2 * half;
        __syncthreads();
    }

    double w[K];
#pragma unroll
    for (int d = 0; d < K; ++d) w[d] = win[d];
    for (int task = t; task < tasks; task += nt) {
        int l = 0, start = 0, lo = 0;                                        // lo: where level l's planes begin in lv (l >= 1)
        int n = H - K + 1;
        while (task >= start + C * n) {                                      // tasks < the total, so l stays below L
            start += C * n;
            if (l >= 1) lo += 2 * C * (H >> l) * (H >> l);
            ++l;
            n = (H >> l) - K + 1;
        }
        const int r = task - start, c = r / n, q = r - c * n;
        double s0, s1;
        if (l == 0) {
            ssim_column<K, unsigned char>(la + c * HW + q, lb + c * HW + q, H, 0, w, c1, c2, s0, s1);
        } else {
            const int Hl = H >> l, plane = Hl * Hl;
            const uint16_t* pa = lv + lo + c * plane + q;
            ssim_column<K, uint16_t>(pa, pa + C * plane, Hl, l, w, c1, c2, s0, s1);
        }
        colsum[2 * task] = s0;
        colsum[2 * task + 1] = s1;
    }
    __syncthreads();

    const int lane = t & 63, nw = nt >> 6;
    int start = 0;
    for (int l = 0; l < L; ++l) {
        const int n = (H >> l) - K + 1, cnt = C * n;
        if ((l % nw) == (t >> 6)) {                                          // a whole wave per level
            double s0 = 0.0, s1 = 0.0;
            for (int k = lane; k < cnt; k += 64) {
                s0 += colsum[2 * (start + k)];
                s1 += colsum[2 * (start + k) + 1];
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {                               // the same tree for every pair
                s0 += __shfl_xor(s0, d);
                s1 += __shfl_xor(s1, d);
            }
            if (lane == 0) {
                const double cells = (double)cnt * (double)n;
                stats[(p * L + l) * 2] = s0 / cells;
                stats[(p * L + l) * 2 + 1] = s1 / cells;
            }
        }
        start += cnt;
    }
    if (t == 0) {
        unsigned long long total = 0;
        for (int k = 0; k < nw; ++k) total += wsse[k];
        sse[p] = (long long)total;
    }
}

extern "C" int eg_ssim_u8(const unsigned char* a, int na, const unsigned char* b, int nb, int C, int H, const int* pairs, int P, const double* win,
                          int K, int L, double c1, double c2, double* stats, long long* sse, int* flag, eg_stream_t s) {
    EG_REQUIRE(a && b && pairs && win && stats && sse && flag, "eg_ssim_u8: null pointer");
    EG_REQUIRE(H == 16 || H == 32 || H == 64, "eg_ssim_u8: the image side must be 16, 32 or 64 (H = %d)", H);
    EG_REQUIRE(C >= 1 && C <= SS_MAX_C, "eg_ssim_u8: need 1 <= C <= %d (C = %d)", SS_MAX_C, C);
    EG_REQUIRE(na >= 1 && nb >= 1 && P >= 1, "eg_ssim_u8: need na, nb, P >= 1 (na = %d, nb = %d, P = %d)", na, nb, P);
    EG_REQUIRE(K >= 3 && K <= SS_MAX_K && (K & 1), "eg_ssim_u8: the window must have 3, 5, ... %d taps (K = %d)", SS_MAX_K, K);
    EG_REQUIRE(L >= 1 && L <= SS_MAX_L && (H >> (L - 1)) >= K, "eg_ssim_u8: need L >= 1 and H >> (L - 1) >= K (H = %d, K = %d, L = %d)", H, K, L);
    EG_REQUIRE(c1 > 0.0 && c2 > 0.0 && isfinite(c1) && isfinite(c2), "eg_ssim_u8: c1 and c2 must be positive and finite");
    EG_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)pairs | (uintptr_t)flag) & 3) == 0, "eg_ssim_u8: a, b, pairs and flag must be 4-byte aligned");
    EG_REQUIRE((((uintptr_t)win | (uintptr_t)stats | (uintptr_t)sse) & 7) == 0, "eg_ssim_u8: win, stats and sse must be 8-byte aligned");
    int tasks = 0;
    size_t levels = 0;                                                       // uint16 elements of the levels 1 .. L - 1, both images
    for (int l = 0; l < L; ++l) {
        tasks += C * ((H >> l) - K + 1);
        if (l) levels += (size_t)2 * C * (H >> l) * (H >> l);
    }
    const size_t lds = (size_t)tasks * 16 + 32 + (size_t)2 * C * H * H + levels * 2;
    const int threads = tasks >= SS_THREADS ? SS_THREADS : (tasks + 63) / 64 * 64;
    for (long long p0 = 0; p0 < P; p0 += SS_CHUNK) {
        const dim3 grid((unsigned)(P - p0 < SS_CHUNK ? P - p0 : SS_CHUNK)), block(threads);
#define SS_LAUNCH(KK)                                                                                                                          \
    hipLaunchKernelGGL((ssim_kernel<KK>), grid, block, lds, (hipStream_t)s, a, na, b, nb, C, H, pairs, p0, win, L, tasks, c1, c2, stats, sse, flag)
        switch (K) {
            case 3: SS_LAUNCH(3); break;
            case 5: SS_LAUNCH(5); break;
            case 7: SS_LAUNCH(7); break;
            case 9: SS_LAUNCH(9); break;
            default: SS_LAUNCH(11); break;
        }
#undef SS_LAUNCH
        EG_LAUNCH_CHECK();
    }
    return 0;
}
