// Exact k nearest neighbours between rows of uint8 (not in the reference, whose scripts never compare a sample with the training
// set): the device side of quality.nearest_neighbours and quality.nn_two_sample.
//   d(i, j) = sum_t (q[i][t] - x[j][t])^2 is an integer <= 255^2 * 32768 < 2^31.  With q' = q ^ 0x80 and x' = x ^ 0x80 read as int8 (v - 128; one
//   XOR per four bytes) d = |q'|^2 + |x'|^2 - 2 q'.x': the dot products on the int8 MFMA (v_mfma_i32_32x32x32_i8, int32 accumulation, exact:
//   |q'.x'| <= 2^29), the norms with v_dot4 while the operands are staged, the epilogue in uint32 (|q'|^2 + |x'|^2 <= 2^30, d <= 2^31).
//   knn_walk           THE tile loop: a workgroup owns KNN_TQ queries (two such tiles from KNN_WIDE_NQ queries on) and walks its slice of the
//                      database in tiles of KNN_TR rows; per tile the dot products go to LDS and thread (query, part of the rows) offers
//                      every distance to the selection step it was given
//   knn_tile_kernel    the search: the offers go to a sorted list of k packed keys (d << 32 | j) in LDS, after ONE compare with the list's
//                      last key; the lists of a query's parts are merged before they leave
//   knn_merge_kernel   [splits][nq][k] partial lists -> the k smallest keys of a query, unpacked
// The keys of one query are distinct and totally ordered, so the result is the same set in the same order whatever the tiling, the number
// of slices and the order in which lists are merged: two calls give the same bits.
// The ball count (quality.prdc): count[i] = #{ j != self0 + i : d(q[i], x[j]) <= rad[j] }, closed balls, over the same tile loop.
//   knn_ball_kernel      the offers add d <= rad[row] into one register per thread; the parts of a query are summed -> ws[split][query]
//   knn_ball_sum_kernel  the slices of a query -> count.  Integer sums: any order gives the same bits; nothing is zero-filled or added to.
// The kernel MMD (quality.mmd) takes two more selection steps over the same tile loop:
//   knn_ksum_kernel      the offers add exp(-d * inv_gamma[b]) into NB double registers per thread -> ws[split][query][b]
//   knn_ksum_sum_kernel  the slices of a query -> out[query][b], in a fixed order: two calls give the same bits
//   knn_hist_kernel      one pass of a radix select: the next digit of every distance that matches the prefix -> an LDS histogram
//   knn_hist_reduce_kernel, knn_hist_scan_kernel  the workgroups' histograms -> 64-bit bins -> the bin that holds the rank -> the next
//                        prefix and the rank inside it
// The Sinkhorn divergence (quality.sinkhorn) takes one more: a streaming log-sum-exp in place of the sum
//   knn_softmin_kernel        the offers go into a running (maximum, sum of exp(t - maximum)) per thread -> ws[split][query] = (m, s)
//   knn_softmin_final_kernel  the slices of a query in a fixed order -> log, count, epsilon and the average with the previous potential
#include "eg_common.h"

#define KNN_TQ 64                 // queries per workgroup tile; from KNN_WIDE_NQ queries on a workgroup owns two such tiles
#define KNN_WIDE_NQ 256
#define KNN_TR 128                // database rows per tile (32 per wave)
#define KNN_KC 128                // bytes of a row staged per step (four MFMA k steps)
#define KNN_LD (KNN_KC + 16)      // LDS row stride: 16 consecutive rows start in 16 different 16-byte bank groups
#define KNN_THREADS 256
#define KNN_KMAX 16
#define KNN_TARGET_WGS 512        // two workgroups per CU: the database is split until the launch has about this many
#define KNN_EMPTY 0xffffffffffffffffull

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int sq4(int v) {          // sum of the squares of four int8
#if __has_builtin(__builtin_amdgcn_sdot4)
    return __builtin_amdgcn_sdot4(v, v, 0, false);
#else
    int s = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int e = (int)(signed char)(v >> (8 * b));
        s += e * e;
    }
    return s;
#endif
}

// 16 bytes of row `row` (< rows, else zeros) at byte k (< K, else zeros), as int8 about 128; *norm += their squares
__device__ __forceinline__ v4i knn_load(const unsigned char* __restrict__ base, long long row, long long rows, int k, int K, int& norm) {
    v4i v = {0, 0, 0, 0};
    if (row < rows && k < K) {
        v = *(const v4i*)(base + (size_t)row * K + k);
        v ^= (int)0x80808080;
        norm += sq4(v.x) + sq4(v.y) + sq4(v.z) + sq4(v.w);
    }
    return v;
}

// sorted ascending list of k keys, slot j of thread t at list[j * KNN_THREADS + t]; key < list[k - 1] on entry
__device__ __forceinline__ void knn_insert(unsigned long long* list, int k, unsigned long long key) {
    int j = k - 1;
    while (j > 0) {
        const unsigned long long prev = list[(j - 1) * KNN_THREADS];
        if (prev < key) break;
        list[j * KNN_THREADS] = prev;
        --j;
    }
    list[j * KNN_THREADS] = key;
}

// THE tile loop of this file: the workgroup's TQ queries (blockIdx.x) against its slice of the database (blockIdx.y), a tile of KNN_TR rows
// at a time.  Per tile the exact distances d(query, row) reach thread (query sq = tid % TQ, part sp = tid / TQ of the tile's rows) one by one:
//   sel.tile(r0, n, tid)     once per tile by every thread, before the barrier that precedes the offers (LDS the offers read is written here;
//                            two barriers have passed since the previous tile's offers)
//   sel.offer(row, j, d)     row of the tile, database row j = r0 + row < n, j != the excluded row; only for queries < nq
// TQ = 64: wave w takes rows 32 w .. of the tile against all 64 queries (2 accumulators).  TQ = 128: the waves form 2 x 2, each 64 rows x 64
// queries (4 accumulators): 4 LDS fragments per 4 MFMAs instead of 3 per 2, and a third fewer operand bytes staged per multiply-add.
template <int TQ, class Sel>
__device__ __forceinline__ void knn_walk(const unsigned char* __restrict__ q, int nq, const unsigned char* __restrict__ x, int n, int K, long long self0,
                                         int tiles_per_split, Sel& sel) {
    // stage[buf]: KNN_TR rows of x, then TQ rows of q, KNN_LD bytes each; after a tile's last step the same bytes hold dots[row][query]
    __shared__ __attribute__((aligned(16))) unsigned char stage[2][(KNN_TR + TQ) * KNN_LD];
    __shared__ int xn[KNN_TR], qn[TQ];
    static_assert(sizeof(stage) >= KNN_TR * TQ * sizeof(int), "the dot products alias the staging buffers");
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int RB = TQ / 64, QP = TQ / 32, PARTS = KNN_THREADS / TQ, RP = KNN_TR / PARTS;
    const int q0 = blockIdx.x * TQ;
    const int wrow0 = TQ == 64 ? w * 32 : (w >> 1) * 64, wq0 = TQ == 64 ? 0 : (w & 1) * 64;
    const int ntiles = (int)(((long long)n + KNN_TR - 1) / KNN_TR);
    const int t_first = blockIdx.y * tiles_per_split, t_end = min(t_first + tiles_per_split, ntiles);
    const int srow = tid >> 3, sk = (tid & 7) * 16;                // staging: 8 threads per row, 32 rows per pass
    const int fr = lane & 31, fk = (lane >> 5) * 16;               // fragments: row of the 32 x 32 block, half of the k step
    const int nsteps = (K + KNN_KC - 1) / KNN_KC;

    const int sq = tid % TQ, sp = tid / TQ;                        // selection: query of the tile, part of the tile's rows
    const long long qi = (long long)q0 + sq;
    const long long excl = self0 >= 0 ? self0 + qi : -1;
    int qnorm[QP] = {};

    for (int t = t_first; t < t_end; ++t) {
        const long long r0 = (long long)t * KNN_TR;
        v16i acc[RB][2];
#pragma unroll
        for (int a = 0; a < RB; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0;
        int xnorm[4] = {0, 0, 0, 0}, qdummy[QP] = {};
        const bool first = t == t_first;
        v4i rx[4], rq[QP];
#pragma unroll
        for (int p = 0; p < 4; ++p) rx[p] = knn_load(x, r0 + p * 32 + srow, n, sk, K, xnorm[p]);
#pragma unroll
        for (int p = 0; p < QP; ++p) rq[p] = knn_load(q, (long long)q0 + p * 32 + srow, nq, sk, K, first ? qnorm[p] : qdummy[p]);
        __syncthreads();                                           // the previous tile's selection has read its dot products
#pragma unroll
        for (int p = 0; p < 4; ++p) *(v4i*)&stage[0][(p * 32 + srow) * KNN_LD + sk] = rx[p];
#pragma unroll
        for (int p = 0; p < QP; ++p) *(v4i*)&stage[0][(KNN_TR + p * 32 + srow) * KNN_LD + sk] = rq[p];
        __syncthreads();
        for (int c = 0; c < nsteps; ++c) {
            const bool more = c + 1 < nsteps;
            if (more) {
                const int kk = (c + 1) * KNN_KC + sk;
#pragma unroll
                for (int p = 0; p < 4; ++p) rx[p] = knn_load(x, r0 + p * 32 + srow, n, kk, K, xnorm[p]);
#pragma unroll
                for (int p = 0; p < QP; ++p) rq[p] = knn_load(q, (long long)q0 + p * 32 + srow, nq, kk, K, first ? qnorm[p] : qdummy[p]);
            }
            const unsigned char* sb = stage[c & 1];
#pragma unroll
            for (int s = 0; s < KNN_KC / 32; ++s) {
                // both operands take their element j from the same byte t = 32 s + fk + j of their row: the sum over t is the dot product
                v4i fa[RB], fb[2];
#pragma unroll
                for (int a = 0; a < RB; ++a) fa[a] = *(const v4i*)&sb[(wrow0 + a * 32 + fr) * KNN_LD + s * 32 + fk];
#pragma unroll
                for (int b = 0; b < 2; ++b) fb[b] = *(const v4i*)&sb[(KNN_TR + wq0 + b * 32 + fr) * KNN_LD + s * 32 + fk];
#pragma unroll
                for (int a = 0; a < RB; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
            }
            if (more) {
                unsigned char* nb = stage[(c + 1) & 1];
#pragma unroll
                for (int p = 0; p < 4; ++p) *(v4i*)&nb[(p * 32 + srow) * KNN_LD + sk] = rx[p];
#pragma unroll
                for (int p = 0; p < QP; ++p) *(v4i*)&nb[(KNN_TR + p * 32 + srow) * KNN_LD + sk] = rq[p];
            }
            __syncthreads();
        }
        // row norms: the 8 staging threads of a row are 8 consecutive lanes
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            int v = xnorm[p];
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
            if ((tid & 7) == 0) xn[p * 32 + srow] = v;
        }
        if (first) {
#pragma unroll
            for (int p = 0; p < QP; ++p) {
                int v = qnorm[p];
                v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
                if ((tid & 7) == 0) qn[p * 32 + srow] = v;
            }
        }
        sel.tile(r0, n, tid);
        // C layout of the 32 x 32 block (A = x rows, B = queries): column = lane & 31 = query, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
        int* dots = (int*)&stage[0][0];                            // [KNN_TR][TQ]: the last step's barrier has passed, nobody reads operands
#pragma unroll
        for (int a = 0; a < RB; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = wrow0 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    dots[row * TQ + wq0 + b * 32 + fr] = acc[a][b][e];
                }
        __syncthreads();
        if (qi < nq) {
            const unsigned int qnorm_u = (unsigned int)qn[sq];
            for (int r = 0; r < RP; ++r) {
                const int row = sp * RP + r;
                const long long j = r0 + row;
                if (j >= n) break;
                const unsigned int d = qnorm_u + (unsigned int)xn[row] - 2u * (unsigned int)dots[row * TQ + sq];
                if (j != excl) sel.offer(row, j, d);
            }
        }
    }
}

// selection step of the search: a sorted list of k packed keys (d << 32 | j) per thread in LDS, ONE compare with its last key per offer
struct KnnLists {
    unsigned long long* mine;                                      // slot j at mine[j * KNN_THREADS]
    unsigned long long kth;
    int k;
    __device__ __forceinline__ void tile(long long, int, int) {}
    __device__ __forceinline__ void offer(int, long long j, unsigned int d) {
        const unsigned long long key = ((unsigned long long)d << 32) | (unsigned int)j;
        if (key < kth) {
            knn_insert(mine, k, key);
            kth = mine[(k - 1) * KNN_THREADS];
        }
    }
};

// KCAP = list capacity, k <= KCAP (1, 8 or 16).
template <int TQ, int KCAP>
__global__ __launch_bounds__(KNN_THREADS) void knn_tile_kernel(const unsigned char* __restrict__ q, int nq, const unsigned char* __restrict__ x, int n,
                                                               int K, int k, long long self0, int tiles_per_split,
                                                               unsigned long long* __restrict__ part) {
    __shared__ unsigned long long lists[KCAP * KNN_THREADS];       // [k][KNN_THREADS]
    constexpr int PARTS = KNN_THREADS / TQ;
    const int tid = threadIdx.x, sq = tid % TQ, sp = tid / TQ;
    const long long qi = (long long)blockIdx.x * TQ + sq;
    KnnLists sel = {lists + tid, KNN_EMPTY, k};
    for (int j = 0; j < k; ++j) sel.mine[j * KNN_THREADS] = KNN_EMPTY;
    knn_walk<TQ>(q, nq, x, n, K, self0, tiles_per_split, sel);
    // the lists of a query's parts -> part 0's list -> part[split][query][k]
    __syncthreads();
    if (sp == 0 && qi < nq) {
        for (int o = 1; o < PARTS; ++o)
            for (int j = 0; j < k; ++j) {
                const unsigned long long key = lists[j * KNN_THREADS + o * TQ + sq];
                if (key >= sel.kth) break;                         // sorted: the rest of this list is no better
                knn_insert(sel.mine, k, key);
                sel.kth = sel.mine[(k - 1) * KNN_THREADS];
            }
        unsigned long long* o = part + ((size_t)blockIdx.y * nq + qi) * k;
        for (int j = 0; j < k; ++j) o[j] = sel.mine[j * KNN_THREADS];
    }
}

// selection step of the ball count: the radii of the tile's rows in LDS beside the norms, ONE counter per thread across all tiles.  d < 2^31,
// so the compare is signed and a negative radius is an empty ball.
struct KnnBalls {
    const int* __restrict__ rad;
    int* radl;                                                     // [KNN_TR]
    int count;
    __device__ __forceinline__ void tile(long long r0, int n, int tid) {
        if (tid < KNN_TR) radl[tid] = r0 + tid < n ? rad[r0 + tid] : -1;
    }
    __device__ __forceinline__ void offer(int row, long long, unsigned int d) { count += (int)d <= radl[row] ? 1 : 0; }
};

// count of the slice -> ws[split][query]
template <int TQ>
__global__ __launch_bounds__(KNN_THREADS) void knn_ball_kernel(const unsigned char* __restrict__ q, int nq, const unsigned char* __restrict__ x, int n,
                                                               int K, const int* __restrict__ rad, long long self0, int tiles_per_split,
                                                               int* __restrict__ ws) {
    __shared__ int radl[KNN_TR], counts[KNN_THREADS];
    constexpr int PARTS = KNN_THREADS / TQ;
    const int tid = threadIdx.x, sq = tid % TQ, sp = tid / TQ;
    const long long qi = (long long)blockIdx.x * TQ + sq;
    KnnBalls sel = {rad, radl, 0};
    knn_walk<TQ>(q, nq, x, n, K, self0, tiles_per_split, sel);
    counts[tid] = sel.count;
    __syncthreads();
    if (sp == 0 && qi < nq) {
        int c = 0;
#pragma unroll
        for (int o = 0; o < PARTS; ++o) c += counts[o * TQ + sq];
        ws[(size_t)blockIdx.y * nq + qi] = c;
    }
}

// count[i] = the sum of query i's slices: one wave per query, its lanes stride over the slices (one thread per query would walk up to
// hundreds of slices through dependent-latency loads, 50 us at 396 slices)
__global__ __launch_bounds__(256) void knn_ball_sum_kernel(const int* __restrict__ ws, int splits, int nq, int* __restrict__ count) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= nq) return;                                           // whole waves leave: the shuffles below see full waves
    int c = 0;
    for (int s = lane; s < splits; s += 64) c += ws[(size_t)s * nq + i];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) c += __shfl_xor(c, o);
    if (lane == 0) count[i] = c;
}

// one workgroup per query: round r picks the smallest key above round r - 1's (the keys of a query are distinct)
__global__ __launch_bounds__(256) void knn_merge_kernel(const unsigned long long* __restrict__ part, int splits, int nq, int k, int* __restrict__ dist,
                                                        int* __restrict__ idx) {
    __shared__ unsigned long long sm[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int total = splits * k;
    unsigned long long prev = 0;
    for (int r = 0; r < k; ++r) {
        unsigned long long best = KNN_EMPTY;
        for (int e = tid; e < total; e += 256) {
            const unsigned long long key = part[((size_t)(e / k) * nq + i) * k + (e % k)];
            if ((r == 0 || key > prev) && key < best) best = key;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other < best ? other : best;
        }
        __syncthreads();
        if ((tid & 63) == 0) sm[tid >> 6] = best;
        __syncthreads();
        best = sm[0];
#pragma unroll
        for (int o = 1; o < 4; ++o) best = sm[o] < best ? sm[o] : best;
        prev = best;
        if (tid == 0) {
            dist[(size_t)i * k + r] = (int)(unsigned int)(best >> 32);
            idx[(size_t)i * k + r] = (int)(unsigned int)best;
        }
    }
}

// ---- kernel sums and the distance select (the kernel MMD with a median bandwidth) -----------------------------------------------
// selection step of the kernel sums: acc[b] += exp(-(double)d * inv_gamma[b]) in NB double registers that live across the slice's tiles.
// The argument is ONE rounded product; the exponential is the library's (within an ulp of double).
template <int NB>
struct KnnKsum {
    double ig[NB], acc[NB];
    __device__ __forceinline__ void tile(long long, int, int) {}
    __device__ __forceinline__ void offer(int, long long, unsigned int d) {
        const double dd = (double)d;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] += exp(-(dd * ig[b]));
    }
};

// sums of the slice -> ws[split][query][b]: the parts of a query are added in the order 0, 1 .. PARTS - 1
template <int TQ, int NB>
__global__ __launch_bounds__(KNN_THREADS) void knn_ksum_kernel(const unsigned char* __restrict__ q, int nq, const unsigned char* __restrict__ x, int n,
                                                               int K, const double* __restrict__ inv_gamma, long long self0, int tiles_per_split,
                                                               double* __restrict__ ws) {
    __shared__ double sums[KNN_THREADS];
    constexpr int PARTS = KNN_THREADS / TQ;
    const int tid = threadIdx.x, sq = tid % TQ, sp = tid / TQ;
    const long long qi = (long long)blockIdx.x * TQ + sq;
    KnnKsum<NB> sel;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        sel.ig[b] = inv_gamma[b];
        sel.acc[b] = 0.0;
    }
    knn_walk<TQ>(q, nq, x, n, K, self0, tiles_per_split, sel);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        __syncthreads();                                           // the previous bandwidth's sums have been read
        sums[tid] = sel.acc[b];
        __syncthreads();
        if (sp == 0 && qi < nq) {
            double c = sums[sq];
#pragma unroll
            for (int o = 1; o < PARTS; ++o) c += sums[o * TQ + sq];
            ws[((size_t)blockIdx.y * nq + qi) * NB + b] = c;
        }
    }
}

// out[i][b] = the sum of query i's slices: one wave per query, lane l adds the slices l, l + 64 .. in that order, then a butterfly over the
// lanes -- a fixed tree, so two calls give the same bits.  Thread 0 of the launch writes the flag word: bit b <- inv_gamma[b] is not a
// finite positive number.
__global__ __launch_bounds__(256) void knn_ksum_sum_kernel(const double* __restrict__ ws, int splits, int nq, int nb, const double* __restrict__ inv_gamma,
                                                           double* __restrict__ out, int* __restrict__ flag) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int bad = 0;
        for (int b = 0; b < nb; ++b) {
            const double g = inv_gamma[b];
            if (!(g > 0.0 && g < __builtin_huge_val())) bad |= 1 << b;
        }
        flag[0] = bad;
    }
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= nq) return;                                           // whole waves leave: the shuffles below see full waves
    for (int b = 0; b < nb; ++b) {
        double c = 0.0;
        for (int s = lane; s < splits; s += 64) c += ws[((size_t)s * nq + i) * nb + b];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) c += __shfl_xor(c, o);
        if (lane == 0) out[(size_t)i * nb + b] = c;
    }
}

// ---- the soft minimum (one half-iteration of the Sinkhorn divergence) ------------------------------------------------------------
// A streaming log-sum-exp is a pair (m, s): m the largest argument so far, s = the sum of exp(t - m) over the arguments so far, so s >= 1
// once an argument has come and nothing overflows or underflows to log 0.  A part or a slice without an offer holds (-inf, 0).
// merge of two pairs: the pair with the smaller maximum is rescaled by ONE exponential; equal maxima (two empty pairs among them) take no
// exponential, so -inf - (-inf) is never formed.  The result does not depend on which of the two comes first.
__device__ __forceinline__ void softmin_merge(double& m, double& s, double m2, double s2) {
#pragma clang fp contract(off)
    if (m >= m2) {
        s = fma(s2, m2 == m ? 1.0 : exp(m2 - m), s);
    } else {
        s = fma(s, exp(m - m2), s2);
        m = m2;
    }
}

// selection step of the soft minimum: t = (g[j] - (double)d) * inv_eps, one rounded subtraction and one rounded product, into the thread's
// running pair with ONE exponential, exp(-|t - m|): it is the new term where t <= m and the rescale of s where t is the new maximum.  The
// tile's KNN_TR values of g are staged in LDS like the radii of the ball count.
struct KnnSoftmin {
    const double* __restrict__ g;
    double* gl;                                                    // [KNN_TR]
    double ie, m, s;
    __device__ __forceinline__ void tile(long long r0, int n, int tid) {
        if (tid < KNN_TR) gl[tid] = r0 + tid < n ? g[r0 + tid] : 0.0;
    }
    __device__ __forceinline__ void offer(int row, long long, unsigned int d) {
#pragma clang fp contract(off)
        const double t = (gl[row] - (double)d) * ie;
        const double up = t - m;                                   // +inf at the first offer: exp(-inf) = 0 and s = 0 * 0 + 1
        const double e = exp(-fabs(up));
        const bool keep = up <= 0.0;
        s = keep ? s + e : fma(s, e, 1.0);
        m = keep ? m : t;
    }
};

// pair of the slice -> ws[split][query] = (m, s): the parts of a query are merged in the order 0, 1 .. PARTS - 1
template <int TQ>
__global__ __launch_bounds__(KNN_THREADS) void knn_softmin_kernel(const unsigned char* __restrict__ q, int nq, const unsigned char* __restrict__ x, int n,
                                                                  int K, const double* __restrict__ g, const double* __restrict__ inv_eps, long long self0,
                                                                  int tiles_per_split, double* __restrict__ ws) {
    __shared__ double gl[KNN_TR], pm[KNN_THREADS], ps[KNN_THREADS];
    constexpr int PARTS = KNN_THREADS / TQ;
    const int tid = threadIdx.x, sq = tid % TQ, sp = tid / TQ;
    const long long qi = (long long)blockIdx.x * TQ + sq;
    KnnSoftmin sel = {g, gl, inv_eps[0], -__builtin_huge_val(), 0.0};
    knn_walk<TQ>(q, nq, x, n, K, self0, tiles_per_split, sel);
    pm[tid] = sel.m;
    ps[tid] = sel.s;
    __syncthreads();
    if (sp == 0 && qi < nq) {
        double m = pm[sq], s = ps[sq];
#pragma unroll
        for (int o = 1; o < PARTS; ++o) softmin_merge(m, s, pm[o * TQ + sq], ps[o * TQ + sq]);
        double* o = ws + ((size_t)blockIdx.y * nq + qi) * 2;
        o[0] = m;
        o[1] = s;
    }
}

// out[i] from the pairs of query i's slices: one wave per query, lane l merges the slices l, l + 64 .. in that order, then a butterfly over
// the lanes -- a fixed tree, so two calls give the same bits.  soft = -(m + (log s - log |J_i|)) / inv_eps: the small difference of the two
// logarithms first, so only one sum and the quotient round at the size of m.  prev[i] is read before out[i] is written by the same thread:
// prev and out may be one array.  Thread 0 of the launch writes the flag word: bit 0 <- inv_eps[0] is not a finite positive number.
__global__ __launch_bounds__(256) void knn_softmin_final_kernel(const double* __restrict__ ws, int splits, int nq, int n, long long self0,
                                                                const double* __restrict__ inv_eps, const double* prev, double* out,
                                                                int* __restrict__ flag) {
#pragma clang fp contract(off)
    const double ie = inv_eps[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[0] = ie > 0.0 && ie < __builtin_huge_val() ? 0 : 1;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= nq) return;                                           // whole waves leave: the shuffles below see full waves
    double m = -__builtin_huge_val(), s = 0.0;
    for (int p = lane; p < splits; p += 64) {
        const double* w = ws + ((size_t)p * nq + i) * 2;
        softmin_merge(m, s, w[0], w[1]);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        softmin_merge(m, s, m2, s2);
    }
    if (lane == 0) {
        const long long excl = self0 >= 0 ? self0 + i : -1;
        const double count = (double)(n - (excl >= 0 && excl < n ? 1 : 0));
        const double soft = -((m + (log(s) - log(count))) / ie);
        out[i] = prev ? 0.5 * prev[i] + 0.5 * soft : soft;
    }
}

// The select is a radix select over the distances, most significant digit first, KNN_HBITS bits a pass: a pass counts, among the distances
// whose higher bits equal the prefix found so far, the next digit.  (2048 bins of a first 11-bit digit would cost the wide layout its
// second workgroup per CU: its staging buffers leave 7 KB of the CU's half.  A row length above 16512 bytes, whose distances need 31 bits,
// takes a fourth pass over the one top bit instead.)
#define KNN_HBITS 10
#define KNN_HBINS (1 << KNN_HBITS)

struct KnnSelectState {                                            // device resident, written by the scan of every pass
    unsigned long long rank;                                       // rank among the distances that match the prefix
    unsigned int prefix;                                           // d >> shift of the pass that wrote it
    int beyond;                                                    // rank >= the number of pairs
};

// selection step of the select: the digit of a matching distance goes to the workgroup's LDS histogram.  Distances between natural images
// concentrate -- in the first pass a thread's run of offers (its 32 or 64 rows of every tile) falls into a handful of bins -- so a thread
// counts a run of equal digits in a register and adds it once: same-address LDS atomics serialise.
struct KnnHist {
    unsigned int* hist;                                            // [KNN_HBINS]
    unsigned int prefix;
    int shift, hshift;                                             // digit = (d >> shift) & (KNN_HBINS - 1); it counts iff d >> hshift == prefix
    unsigned int cur, run;
    __device__ __forceinline__ void tile(long long, int, int) {}
    __device__ __forceinline__ void flush() {
        if (run) atomicAdd(&hist[cur], run);
    }
    __device__ __forceinline__ void offer(int, long long, unsigned int d) {
        if ((d >> hshift) != prefix) return;
        const unsigned int bin = (d >> shift) & (KNN_HBINS - 1);
        if (bin == cur) {
            ++run;
        } else {
            flush();
            cur = bin;
            run = 1;
        }
    }
};

// histogram of the workgroup's pairs -> hist_ws[workgroup][bin], written once
template <int TQ>
__global__ __launch_bounds__(KNN_THREADS) void knn_hist_kernel(const unsigned char* __restrict__ q, int nq, const unsigned char* __restrict__ x, int n,
                                                               int K, long long self0, int tiles_per_split, int shift, int first,
                                                               const KnnSelectState* __restrict__ state, unsigned int* __restrict__ hist_ws) {
    __shared__ unsigned int hist[KNN_HBINS];
    const int tid = threadIdx.x;
    for (int b = tid; b < KNN_HBINS; b += KNN_THREADS) hist[b] = 0;
    __syncthreads();
    KnnHist sel = {hist, first ? 0u : state->prefix, shift, min(shift + KNN_HBITS, 31), 0u, 0u};      // d < 2^31: d >> 31 == 0
    knn_walk<TQ>(q, nq, x, n, K, self0, tiles_per_split, sel);
    sel.flush();
    __syncthreads();
    unsigned int* o = hist_ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * KNN_HBINS;
    for (int b = tid; b < KNN_HBINS; b += KNN_THREADS) o[b] = hist[b];
}

// thread = bin, workgroup g: the histograms of the workgroups g * per .. -> part[g][bin], 64-bit.  One workgroup walking all histograms
// of a launch (2 MB from 512 workgroups) took 160 us a pass, as long as the pass itself on 1024-byte rows; KNN_HGROUPS workgroups share it.
#define KNN_HGROUPS 32
__global__ __launch_bounds__(KNN_HBINS) void knn_hist_reduce_kernel(const unsigned int* __restrict__ hist_ws, int nwg, int per,
                                                                    unsigned long long* __restrict__ part) {
    const int tid = threadIdx.x, g0 = blockIdx.x * per, g1 = min(g0 + per, nwg);
    unsigned long long c = 0;
#pragma unroll 8
    for (int g = g0; g < g1; ++g) c += hist_ws[(size_t)g * KNN_HBINS + tid];
    part[(size_t)blockIdx.x * KNN_HBINS + tid] = c;
}

// one workgroup, thread = bin: the groups' 64-bit bins -> their sum -> its inclusive scan -> the bin that holds the rank -> the next
// prefix and the rank inside that bin.  first: the rank is the argument (no state exists yet) and the scan's total is the number of pairs;
// last: the prefix is the distance.
__global__ __launch_bounds__(KNN_HBINS) void knn_hist_scan_kernel(const unsigned long long* __restrict__ part, int groups, unsigned long long rank_arg,
                                                                  int first, int last, KnnSelectState* __restrict__ state, int* __restrict__ out) {
    __shared__ unsigned long long wsum[KNN_HBINS / 64];
    __shared__ int found;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned long long c = 0;
#pragma unroll 8
    for (int g = 0; g < groups; ++g) c += part[(size_t)g * KNN_HBINS + tid];
    unsigned long long incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (tid == 0) found = 0;
    if (lane == 63) wsum[w] = incl;
    const unsigned long long rank0 = first ? rank_arg : state->rank;
    const unsigned int prefix0 = first ? 0u : state->prefix;
    const int beyond0 = first ? 0 : state->beyond;
    __syncthreads();                                               // every thread has read the state before one of them writes it
    unsigned long long total = 0;
    for (int o = 0; o < KNN_HBINS / 64; ++o) {
        if (o == w) incl += total;
        total += wsum[o];
    }
    // a rank beyond the pairs (the first pass sees all of them) selects the largest distance and raises the mark
    const int beyond = first ? (rank0 >= total ? 1 : 0) : beyond0;
    const unsigned long long rank = first && beyond && total ? total - 1 : rank0;
    if (c && rank >= incl - c && rank < incl) {                    // at most one bin
        found = 1;
        state->rank = rank - (incl - c);
        state->prefix = (prefix0 << KNN_HBITS) | (unsigned int)tid;
        state->beyond = beyond;
        if (last) {
            out[0] = (int)((prefix0 << KNN_HBITS) | (unsigned int)tid);
            out[1] = beyond;
        }
    }
    __syncthreads();
    if (tid == 0 && !found) {                                      // no pair at all: the distance reads 0 and the mark is up
        state->rank = 0;
        state->prefix = prefix0 << KNN_HBITS;
        state->beyond = 1;
        if (last) {
            out[0] = 0;
            out[1] = 1;
        }
    }
}

// tiles of KNN_TR rows a workgroup walks for (nq, n): as few as keep about KNN_TARGET_WGS workgroups in the launch
static int knn_wg_queries(int nq) { return nq >= KNN_WIDE_NQ ? 2 * KNN_TQ : KNN_TQ; }
static int knn_tiles_per_split(int nq, int n) {
    const int tq = knn_wg_queries(nq);
    const long long qt = ((long long)nq + tq - 1) / tq, rt = ((long long)n + KNN_TR - 1) / KNN_TR;
    long long want = (KNN_TARGET_WGS + qt - 1) / qt;               // slices wanted
    if (want < 1) want = 1;
    if (want > rt) want = rt;
    return (int)((rt + want - 1) / want);
}

extern "C" int eg_knn_tile_queries(void) { return KNN_TQ; }
extern "C" int eg_knn_tile_rows(void) { return KNN_TR; }

extern "C" int eg_knn_splits(int nq, int n) {
    if (nq < 1 || n < 1) return 0;
    const int tps = knn_tiles_per_split(nq, n);
    return (int)((((long long)n + KNN_TR - 1) / KNN_TR + tps - 1) / tps);
}

extern "C" size_t eg_knn_ws_bytes(int nq, int n, int k) {
    if (nq < 1 || n < 1 || k < 1) return 0;
    return (size_t)eg_knn_splits(nq, n) * (size_t)nq * (size_t)k * sizeof(unsigned long long);
}

extern "C" int eg_knn_u8(const unsigned char* q, int nq, const unsigned char* x, int n, int K, int k, long long self0, void* ws, int* dist, int* idx,
                         eg_stream_t s) {
    EG_REQUIRE(q && x && ws && dist && idx, "eg_knn_u8: null pointer");
    EG_REQUIRE(nq >= 1 && n >= 1, "eg_knn_u8: need nq >= 1 and n >= 1");
    EG_REQUIRE(K >= 64 && K <= 32768 && K % 64 == 0, "eg_knn_u8: the row length K must be a multiple of 64 in 64 .. 32768 (K = %d)", K);
    EG_REQUIRE(k >= 1 && k <= KNN_KMAX, "eg_knn_u8: need 1 <= k <= %d (k = %d)", KNN_KMAX, k);
    const long long candidates = (long long)n - (self0 >= 0 && self0 < n ? 1 : 0);         // of query 0, which has the fewest
    EG_REQUIRE(k <= candidates, "eg_knn_u8: k = %d, but a query has only %lld candidates", k, candidates);
    EG_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)ws & 7) == 0, "eg_knn_u8: q and x must be 16-byte aligned, ws 8-byte");
    const int tps = knn_tiles_per_split(nq, n), splits = eg_knn_splits(nq, n);
    const int tq = knn_wg_queries(nq), qt = cdiv(nq, tq);
    EG_REQUIRE(splits <= 65535, "eg_knn_u8: too many slices");
#define KNN_LAUNCH(TQ, KCAP) \
    hipLaunchKernelGGL((knn_tile_kernel<TQ, KCAP>), dim3(qt, splits), dim3(KNN_THREADS), 0, (hipStream_t)s, q, nq, x, n, K, k, self0, tps, (unsigned long long*)ws)
    if (tq == KNN_TQ) {
        if (k == 1) KNN_LAUNCH(KNN_TQ, 1);
        else if (k <= 8) KNN_LAUNCH(KNN_TQ, 8);
        else KNN_LAUNCH(KNN_TQ, KNN_KMAX);
    } else {
        if (k == 1) KNN_LAUNCH(2 * KNN_TQ, 1);
        else if (k <= 8) KNN_LAUNCH(2 * KNN_TQ, 8);
        else KNN_LAUNCH(2 * KNN_TQ, KNN_KMAX);
    }
#undef KNN_LAUNCH
    hipLaunchKernelGGL(knn_merge_kernel, dim3(nq), dim3(256), 0, (hipStream_t)s, (const unsigned long long*)ws, splits, nq, k, dist, idx);
    EG_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t eg_ball_count_ws_bytes(int nq, int n) {
    if (nq < 1 || n < 1) return 0;
    return (size_t)eg_knn_splits(nq, n) * (size_t)nq * sizeof(int);
}

extern "C" int eg_ball_count_u8(const unsigned char* q, int nq, const unsigned char* x, int n, int K, const int* rad, long long self0, void* ws,
                                int* count, eg_stream_t s) {
    EG_REQUIRE(q && x && rad && ws && count, "eg_ball_count_u8: null pointer");
    EG_REQUIRE(nq >= 1 && n >= 1, "eg_ball_count_u8: need nq >= 1 and n >= 1");
    EG_REQUIRE(K >= 64 && K <= 32768 && K % 64 == 0, "eg_ball_count_u8: the row length K must be a multiple of 64 in 64 .. 32768 (K = %d)", K);
    EG_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)x & 15) == 0, "eg_ball_count_u8: q and x must be 16-byte aligned");
    EG_REQUIRE(((uintptr_t)rad & 3) == 0 && ((uintptr_t)ws & 3) == 0 && ((uintptr_t)count & 3) == 0,
               "eg_ball_count_u8: rad, ws and count must be 4-byte aligned");
    const int tps = knn_tiles_per_split(nq, n), splits = eg_knn_splits(nq, n);
    const int tq = knn_wg_queries(nq), qt = cdiv(nq, tq);
    EG_REQUIRE(splits <= 65535, "eg_ball_count_u8: too many slices");
    if (tq == KNN_TQ)
        hipLaunchKernelGGL((knn_ball_kernel<KNN_TQ>), dim3(qt, splits), dim3(KNN_THREADS), 0, (hipStream_t)s, q, nq, x, n, K, rad, self0, tps, (int*)ws);
    else
        hipLaunchKernelGGL((knn_ball_kernel<2 * KNN_TQ>), dim3(qt, splits), dim3(KNN_THREADS), 0, (hipStream_t)s, q, nq, x, n, K, rad, self0, tps, (int*)ws);
    hipLaunchKernelGGL(knn_ball_sum_kernel, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)s, (const int*)ws, splits, nq, count);
    EG_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t eg_kernel_sum_ws_bytes(int nq, int n, int nb) {
    if (nq < 1 || n < 1 || nb < 1) return 0;
    return (size_t)eg_knn_splits(nq, n) * (size_t)nq * (size_t)nb * sizeof(double);
}

extern "C" int eg_kernel_sum_u8(const unsigned char* q, int nq, const unsigned char* x, int n, int K, const double* inv_gamma, int nb, long long self0,
                                void* ws, double* out, int* flag, eg_stream_t s) {
    EG_REQUIRE(q && x && inv_gamma && ws && out && flag, "eg_kernel_sum_u8: null pointer");
    EG_REQUIRE(nq >= 1 && n >= 1, "eg_kernel_sum_u8: need nq >= 1 and n >= 1");
    EG_REQUIRE(K >= 64 && K <= 32768 && K % 64 == 0, "eg_kernel_sum_u8: the row length K must be a multiple of 64 in 64 .. 32768 (K = %d)", K);
    EG_REQUIRE(nb >= 1 && nb <= 4, "eg_kernel_sum_u8: need 1 <= nb <= 4 bandwidths (nb = %d)", nb);
    EG_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)x & 15) == 0, "eg_kernel_sum_u8: q and x must be 16-byte aligned");
    EG_REQUIRE(((uintptr_t)inv_gamma & 7) == 0 && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)flag & 3) == 0,
               "eg_kernel_sum_u8: inv_gamma, ws and out must be 8-byte aligned, flag 4-byte");
    const int tps = knn_tiles_per_split(nq, n), splits = eg_knn_splits(nq, n);
    const int tq = knn_wg_queries(nq), qt = cdiv(nq, tq);
    EG_REQUIRE(splits <= 65535, "eg_kernel_sum_u8: too many slices");
#define KSUM_LAUNCH(TQ, NB) \
    hipLaunchKernelGGL((knn_ksum_kernel<TQ, NB>), dim3(qt, splits), dim3(KNN_THREADS), 0, (hipStream_t)s, q, nq, x, n, K, inv_gamma, self0, tps, (double*)ws)
    if (tq == KNN_TQ) {
        if (nb == 1) KSUM_LAUNCH(KNN_TQ, 1);
        else if (nb == 2) KSUM_LAUNCH(KNN_TQ, 2);
        else if (nb == 3) KSUM_LAUNCH(KNN_TQ, 3);
        else KSUM_LAUNCH(KNN_TQ, 4);
    } else {
        if (nb == 1) KSUM_LAUNCH(2 * KNN_TQ, 1);
        else if (nb == 2) KSUM_LAUNCH(2 * KNN_TQ, 2);
        else if (nb == 3) KSUM_LAUNCH(2 * KNN_TQ, 3);
        else KSUM_LAUNCH(2 * KNN_TQ, 4);
    }
#undef KSUM_LAUNCH
    hipLaunchKernelGGL(knn_ksum_sum_kernel, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)s, (const double*)ws, splits, nq, nb, inv_gamma, out, flag);
    EG_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t eg_softmin_ws_bytes(int nq, int n) {
    if (nq < 1 || n < 1) return 0;
    return (size_t)eg_knn_splits(nq, n) * (size_t)nq * 2 * sizeof(double);
}

extern "C" int eg_softmin_u8(const unsigned char* q, int nq, const unsigned char* x, int n, int K, const double* g, const double* inv_eps, long long self0,
                             const double* prev, void* ws, double* out, int* flag, eg_stream_t s) {
    EG_REQUIRE(q && x && g && inv_eps && ws && out && flag, "eg_softmin_u8: null pointer");
    EG_REQUIRE(nq >= 1 && n >= 1, "eg_softmin_u8: need nq >= 1 and n >= 1");
    EG_REQUIRE(K >= 64 && K <= 32768 && K % 64 == 0, "eg_softmin_u8: the row length K must be a multiple of 64 in 64 .. 32768 (K = %d)", K);
    const long long candidates = (long long)n - (self0 >= 0 && self0 < n ? 1 : 0);         // of query 0, which has the fewest
    EG_REQUIRE(candidates >= 1, "eg_softmin_u8: a query has no candidate (n = %d, self0 = %lld): need n - 1 >= 1 where a row is excluded", n, self0);
    EG_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)x & 15) == 0, "eg_softmin_u8: q and x must be 16-byte aligned");
    EG_REQUIRE(((uintptr_t)g & 7) == 0 && ((uintptr_t)inv_eps & 7) == 0 && ((uintptr_t)prev & 7) == 0 && ((uintptr_t)ws & 7) == 0 &&
                   ((uintptr_t)out & 7) == 0 && ((uintptr_t)flag & 3) == 0,
               "eg_softmin_u8: g, inv_eps, prev, ws and out must be 8-byte aligned, flag 4-byte");
    const int tps = knn_tiles_per_split(nq, n), splits = eg_knn_splits(nq, n);
    const int tq = knn_wg_queries(nq), qt = cdiv(nq, tq);
    EG_REQUIRE(splits <= 65535, "eg_softmin_u8: too many slices");
    if (tq == KNN_TQ)
        hipLaunchKernelGGL((knn_softmin_kernel<KNN_TQ>), dim3(qt, splits), dim3(KNN_THREADS), 0, (hipStream_t)s, q, nq, x, n, K, g, inv_eps, self0, tps,
                           (double*)ws);
    else
        hipLaunchKernelGGL((knn_softmin_kernel<2 * KNN_TQ>), dim3(qt, splits), dim3(KNN_THREADS), 0, (hipStream_t)s, q, nq, x, n, K, g, inv_eps, self0, tps,
                           (double*)ws);
    hipLaunchKernelGGL(knn_softmin_final_kernel, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)s, (const double*)ws, splits, nq, n, self0, inv_eps, prev, out,
                       flag);
    EG_LAUNCH_CHECK();
    return 0;
}

// the state first (64 bytes), then KNN_HGROUPS 64-bit histograms, then one 32-bit histogram per workgroup of the tile loop's launch
extern "C" size_t eg_dist_select_ws_bytes(int nq, int n) {
    if (nq < 1 || n < 1) return 0;
    const size_t wgs = (size_t)cdiv(nq, knn_wg_queries(nq)) * (size_t)eg_knn_splits(nq, n);
    return 64 + (size_t)KNN_HGROUPS * KNN_HBINS * sizeof(unsigned long long) + wgs * KNN_HBINS * sizeof(unsigned int);
}

extern "C" int eg_dist_select_u8(const unsigned char* q, int nq, const unsigned char* x, int n, int K, long long self0, unsigned long long rank, void* ws,
                                 int* out, eg_stream_t s) {
    EG_REQUIRE(q && x && ws && out, "eg_dist_select_u8: null pointer");
    EG_REQUIRE(nq >= 1 && n >= 1, "eg_dist_select_u8: need nq >= 1 and n >= 1");
    EG_REQUIRE(K >= 64 && K <= 32768 && K % 64 == 0, "eg_dist_select_u8: the row length K must be a multiple of 64 in 64 .. 32768 (K = %d)", K);
    EG_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)x & 15) == 0, "eg_dist_select_u8: q and x must be 16-byte aligned");
    EG_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 3) == 0, "eg_dist_select_u8: ws must be 8-byte aligned, out 4-byte");
    const int tps = knn_tiles_per_split(nq, n), splits = eg_knn_splits(nq, n);
    const int tq = knn_wg_queries(nq), qt = cdiv(nq, tq);
    EG_REQUIRE(splits <= 65535, "eg_dist_select_u8: too many slices");
    EG_REQUIRE((long long)tps * KNN_TR * tq < (1ll << 32), "eg_dist_select_u8: a workgroup's pairs do not fit a 32-bit bin");
    EG_REQUIRE((long long)qt * splits < (1ll << 31), "eg_dist_select_u8: too many workgroups");
    KnnSelectState* state = (KnnSelectState*)ws;
    unsigned long long* part = (unsigned long long*)((char*)ws + 64);
    unsigned int* hist_ws = (unsigned int*)(part + (size_t)KNN_HGROUPS * KNN_HBINS);
    const int nwg = qt * splits, per = cdiv(nwg, KNN_HGROUPS), groups = cdiv(nwg, per);
    // d <= 255^2 K: three digits hold it up to K = 16512, the fourth pass takes bit 30
    const int passes = 65025ll * K >= (1ll << (3 * KNN_HBITS)) ? 4 : 3;
    for (int p = 0; p < passes; ++p) {
        const int shift = (passes - 1 - p) * KNN_HBITS, first = p == 0, last = p == passes - 1;
        if (tq == KNN_TQ)
            hipLaunchKernelGGL((knn_hist_kernel<KNN_TQ>), dim3(qt, splits), dim3(KNN_THREADS), 0, (hipStream_t)s, q, nq, x, n, K, self0, tps, shift, first,
                               (const KnnSelectState*)state, hist_ws);
        else
            hipLaunchKernelGGL((knn_hist_kernel<2 * KNN_TQ>), dim3(qt, splits), dim3(KNN_THREADS), 0, (hipStream_t)s, q, nq, x, n, K, self0, tps, shift,
                               first, (const KnnSelectState*)state, hist_ws);
        hipLaunchKernelGGL(knn_hist_reduce_kernel, dim3(groups), dim3(KNN_HBINS), 0, (hipStream_t)s, (const unsigned int*)hist_ws, nwg, per, part);
        hipLaunchKernelGGL(knn_hist_scan_kernel, dim3(1), dim3(KNN_HBINS), 0, (hipStream_t)s, (const unsigned long long*)part, groups, rank, first, last, state,
                           out);
    }
    EG_LAUNCH_CHECK();
    return 0;
}
