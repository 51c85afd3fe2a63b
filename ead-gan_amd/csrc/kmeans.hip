// k-means over rows of uint8 (not in the reference): the parts of quality.image_bins / quality.ndb that touch the whole dataset.
// The assignment is eg_knn_u8(rows, centres, 1) unchanged (knn.hip: exact integer distances, ties to the lower centre); this file holds
// what is left of Lloyd's loop and its seeding.  The contract, restated in tests/kmeans_refs.py in numpy int64:
//   centres  are BYTES: a centre is a uint8 row [K], an image like any other (K a multiple of 64 in 64 .. 32768, eg_knn_u8's limits).  The
//            rounding moves a centre by at most half a grey level per pixel, so Lloyd's inertia is not guaranteed to fall monotonically.
//   update   a cell with count > 0: centre[t] = (2 sum[t] + count) / (2 count), round half up, from exact int32 column sums
//            (n * 255 < 2^31 is an argument check); a cell with count == 0 keeps its bytes.
//   seeding  k-means++ driven by bins fp32 uniforms u in [0, 1) on the device.  Centre 0 is row min(floor((double)u[0] * n), n - 1).  For
//            j >= 1: mind[i] = the exact distance from row i to its nearest chosen centre, total = its int64 sum,
//            target = min(floor((double)u[j] * (double)total), total - 1) (n * 2^31 <= 2^53 is an argument check: total is exact in a
//            double and the product is ONE rounded multiplication); the pick is the lowest row whose inclusive prefix sum of mind
//            exceeds target, so a row at distance 0 from a chosen centre is never picked.  total == 0 (fewer than bins distinct rows)
//            raises flag bit 0 and picks row 0; a u outside [0, 1) raises bit 1 and is clamped.
// Kernels:
//   group_count_kernel, group_scan_kernel, group_scatter_kernel    eg_group_rows: a stable counting sort of the labels into cells --
//            per-workgroup LDS histograms, one workgroup that turns them into per-workgroup bases, counts and offsets, and a scatter in
//            which the lanes of a wave that hold one label find each other with ballots (rank = the peers below), the waves of a
//            workgroup taking turns: rows ascend inside a cell
//   kmeans_segbase_kernel, kmeans_partial_kernel, kmeans_divide_kernel   eg_kmeans_update_u8: the member lists are cut into segments of
//            KM_SEG rows (cells are very unequal; a segment is a workgroup's work whatever the cell); a workgroup sums KM_CC bytes of its
//            segment's rows, a wave a row at a time (64 lanes x 16 bytes, contiguous), into packed 16-bit pairs (64 rows x 255 < 2^16),
//            then int32 -> part[segment][K]; the last kernel adds a cell's segments (every fourth to one of four waves) and divides
//   kmeans_seed_dist_kernel, kmeans_seed_pick_kernel    eg_kmeans_seed_u8: per pass ONE centre against all rows on the VALU (v_dot4: the
//            MFMA tile would be 1/128 full and the pass is memory bound), d = |a|^2 + |c|^2 - 2 a.c in uint32, folded into mind, with an
//            int64 partial sum per workgroup; then one workgroup scans the partials, finds the workgroup and the row, writes idx[j] and
//            copies the row into centres[j], where the next pass reads it: nothing is read back by the host
// Integer sums throughout: any order gives the same bits, nothing is zero-filled or added to, two calls give the same bits.
#include "eg_common.h"

#define GR_BLOCK 1024             // labels per workgroup of the count and scatter kernels
#define GR_THREADS 256
#define GR_MAXBINS 1024
#define KM_SEG 256                // member rows per segment of the update
#define KM_CC 1024                // bytes of a row a workgroup of the update sums: 64 lanes x 16
#define KS_ROWS 16                // rows per workgroup of the seeding's streaming kernel: 4 waves x 4 rows in flight (64 and 32 ran 9 % and 4 %
                                  // slower on 202 599 CelebA rows, 2.2 and 1.3 times slower on 8192, whose launch has 64 x fewer workgroups)
#define KS_FLAG_DUPLICATES 1
#define KS_FLAG_U 2

typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned int udot4(unsigned int a, unsigned int b) {          // sum of the products of four uint8 pairs
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, b, 0u, false);
#else
    unsigned int s = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) s += ((a >> (8 * e)) & 255u) * ((b >> (8 * e)) & 255u);
    return s;
#endif
}
__device__ __forceinline__ unsigned int udot16(v4i a, v4i b) {
    return udot4((unsigned int)a.x, (unsigned int)b.x) + udot4((unsigned int)a.y, (unsigned int)b.y) + udot4((unsigned int)a.z, (unsigned int)b.z) +
           udot4((unsigned int)a.w, (unsigned int)b.w);
}

// inclusive scan of v over the 1024 threads of a workgroup; *total = the sum.  wsum: 16 words of LDS; all threads call it.
__device__ __forceinline__ long long block_scan_1024(long long v, long long* wsum, long long* total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    __syncthreads();                                               // the previous scan's sums have been read
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    long long t = 0;
    for (int o = 0; o < 16; ++o) {
        if (o == w) incl += t;
        t += wsum[o];
    }
    *total = t;
    return incl;
}

// ---- eg_group_rows ------------------------------------------------------------------------------------------------------------------------
// histogram of the workgroup's labels -> hist_ws[workgroup][0 .. bins - 1], and [bins] = a label outside [0, bins) was seen
__global__ __launch_bounds__(GR_THREADS) void group_count_kernel(const int* __restrict__ labels, int n, int bins, int* __restrict__ hist_ws) {
    __shared__ int hist[GR_MAXBINS];
    __shared__ int bad;
    const int tid = threadIdx.x;
    for (int b = tid; b < bins; b += GR_THREADS) hist[b] = 0;
    if (tid == 0) bad = 0;
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * GR_BLOCK;
    for (int e = tid; e < GR_BLOCK; e += GR_THREADS) {
        const long long i = r0 + e;
        if (i < n) {
            const int l = labels[i];
            if ((unsigned int)l < (unsigned int)bins) atomicAdd(&hist[l], 1);
            else bad = 1;                                          // every writer writes the same value
        }
    }
    __syncthreads();
    int* o = hist_ws + (size_t)blockIdx.x * (bins + 1);
    for (int b = tid; b < bins; b += GR_THREADS) o[b] = hist[b];
    if (tid == 0) o[bins] = bad;
}

// one workgroup, thread = cell: the workgroups' histograms -> base_ws[workgroup][cell] (the rows of the cell in earlier workgroups), counts,
// offsets (the exclusive scan of the counts; offsets[bins] = the rows that joined a cell) and the flag word
__global__ __launch_bounds__(1024) void group_scan_kernel(const int* __restrict__ hist_ws, int blocks, int bins, int* __restrict__ base_ws,
                                                          int* __restrict__ counts, int* __restrict__ offsets, int* __restrict__ flag) {
    __shared__ long long wsum[16];
    __shared__ int bad;
    const int tid = threadIdx.x;
    if (tid == 0) bad = 0;
    __syncthreads();
    int c = 0;
    if (tid < bins) {
#pragma unroll 8
        for (int g = 0; g < blocks; ++g) {
            base_ws[(size_t)g * bins + tid] = c;
            c += hist_ws[(size_t)g * (bins + 1) + tid];
        }
    }
    int f = 0;
    for (int g = tid; g < blocks; g += 1024) f |= hist_ws[(size_t)g * (bins + 1) + bins];
    if (f) bad = 1;
    long long total;
    const long long incl = block_scan_1024((long long)c, wsum, &total);
    if (tid < bins) {
        counts[tid] = c;
        offsets[tid] = (int)(incl - c);
    }
    if (tid == bins - 1) offsets[bins] = (int)incl;
    if (tid == 0) flag[0] = bad;                                   // after the scan's barriers: every `bad = 1` has landed
}

// the scatter: next[cell] = where the cell's next row of this workgroup goes.  The waves take turns (wave w owns labels 256 w .. of the
// workgroup's GR_BLOCK) and a wave takes 64 labels at a time; the lanes that hold one label find each other with one ballot per label
// bit, a lane's place is the number of its peers below it, and the highest peer moves next[cell] on.  Rows that joined no cell leave
// the tail of order, offsets[bins] .. n - 1, which is filled with -1.
__global__ __launch_bounds__(GR_THREADS) void group_scatter_kernel(const int* __restrict__ labels, int n, int bins, int nbits,
                                                                   const int* __restrict__ base_ws, const int* __restrict__ offsets,
                                                                   int* __restrict__ order) {
    __shared__ int next[GR_MAXBINS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int b = tid; b < bins; b += GR_THREADS) next[b] = offsets[b] + base_ws[(size_t)blockIdx.x * bins + b];
    const int valid = offsets[bins];
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * GR_BLOCK;
    for (int w = 0; w < GR_THREADS / 64; ++w) {
        if (wave == w) {
            for (int r = 0; r < GR_BLOCK / GR_THREADS; ++r) {
                const long long i = r0 + w * (GR_BLOCK / 4) + r * 64 + lane;
                const int l = i < n ? labels[i] : -1;
                const bool ok = (unsigned int)l < (unsigned int)bins;
                unsigned long long peers = __ballot(ok);
                for (int bit = 0; bit < nbits; ++bit) {
                    const bool one = (l >> bit) & 1;
                    const unsigned long long m = __ballot(ok && one);
                    peers &= one ? m : ~m;
                }
                int base = 0;
                if (ok) base = next[l];
                __builtin_amdgcn_wave_barrier();                   // every peer has read next[l] before the highest one moves it
                if (ok) {
                    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
                    if ((peers >> lane) == 1ull) next[l] = base + __popcll(peers);
                    const int pos = base + rank;
                    if (pos >= 0 && pos < n) order[pos] = (int)i;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < GR_BLOCK; e += GR_THREADS) {
        const long long i = r0 + e;
        if (i < n && i >= valid) order[i] = -1;
    }
}

// ---- eg_kmeans_update_u8 ------------------------------------------------------------------------------------------------------------------
// one workgroup, thread = cell: segbase[cell] = the segments of the cells before it, segbase[bins] = all segments
__global__ __launch_bounds__(1024) void kmeans_segbase_kernel(const int* __restrict__ counts, int bins, int* __restrict__ segbase) {
    __shared__ long long wsum[16];
    const int tid = threadIdx.x;
    int c = tid < bins ? counts[tid] : 0;
    c = c > 0 ? (c + KM_SEG - 1) / KM_SEG : 0;
    long long total;
    const long long incl = block_scan_1024((long long)c, wsum, &total);
    if (tid < bins) segbase[tid] = (int)(incl - c);
    if (tid == bins - 1) segbase[bins] = (int)incl;
}

// workgroup (segment, column chunk): wave w sums the segment's rows w, w + 4 .. over the chunk's KM_CC bytes, four rows in flight, the
// bytes 0 | 2 and 1 | 3 of every dword as packed 16-bit pairs; the four waves' sums are added through LDS -> part[segment][chunk]
__global__ __launch_bounds__(256) void kmeans_partial_kernel(const unsigned char* __restrict__ rows, int n, int K, const int* __restrict__ order,
                                                             const int* __restrict__ offsets, const int* __restrict__ counts,
                                                             const int* __restrict__ segbase, int bins, int* __restrict__ part) {
    __shared__ int red[4][KM_CC];
    const int seg = blockIdx.x;
    if (seg >= segbase[bins]) return;                              // the launch covers the most segments n rows in bins cells can have
    int lo = 0, hi = bins;                                         // the last cell with segbase[cell] <= seg: empty cells share a base
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (segbase[mid] <= seg) lo = mid;
        else hi = mid;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int s = seg - segbase[lo];
    const long long first = (long long)offsets[lo] + (long long)s * KM_SEG;
    int cnt = min(KM_SEG, counts[lo] - s * KM_SEG);
    if (first < 0 || first >= n) cnt = 0;
    else if (first + cnt > n) cnt = (int)(n - first);
    const int col = blockIdx.y * KM_CC + lane * 16;
    unsigned int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col < K) {
        for (int r = w; r < cnt; r += 16) {
            v4i v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] = (v4i){0, 0, 0, 0};
                if (r + 4 * q < cnt) {
                    const int row = __builtin_amdgcn_readfirstlane(order[first + r + 4 * q]);
                    if ((unsigned int)row < (unsigned int)n) v[q] = *(const v4i*)(rows + (size_t)row * K + col);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned int d = (unsigned int)v[q][e];
                    acc[2 * e] += d & 0x00ff00ffu;
                    acc[2 * e + 1] += (d >> 8) & 0x00ff00ffu;
                }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int* o = &red[w][lane * 16 + 4 * e];
        o[0] = (int)(acc[2 * e] & 0xffffu);
        o[1] = (int)(acc[2 * e + 1] & 0xffffu);
        o[2] = (int)(acc[2 * e] >> 16);
        o[3] = (int)(acc[2 * e + 1] >> 16);
    }
    __syncthreads();
    const int c0 = blockIdx.y * KM_CC + tid * 4;
    if (c0 < K) {
        v4i sum = *(const v4i*)&red[0][tid * 4];
#pragma unroll
        for (int o = 1; o < 4; ++o) sum += *(const v4i*)&red[o][tid * 4];
        *(v4i*)(part + (size_t)seg * K + c0) = sum;
    }
}

// workgroup (cell, 256 columns), lane = four columns, wave w adds the cell's segments w, w + 4 .. (a cell that holds half of 202 599 rows has
// 399 of them: one thread walking them all made the update a third slower on such cells); the waves' sums meet in LDS -> the column sums
// -> round half up -> four bytes.  Integer sums: the order does not matter.
__global__ __launch_bounds__(256) void kmeans_divide_kernel(const int* __restrict__ part, int K, const int* __restrict__ counts,
                                                            const int* __restrict__ segbase, int segs, unsigned char* __restrict__ centres) {
    __shared__ v4i red[4][64];
    const int cell = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, c0 = blockIdx.y * 256 + lane * 4;
    const int cnt = counts[cell];
    if (cnt <= 0) return;                                          // an empty cell keeps its bytes (the whole workgroup leaves)
    const int s0 = segbase[cell], s1 = min(segbase[cell + 1], segs);       // segs: the segments the launch before this one covered
    v4i sum = {0, 0, 0, 0};
    if (c0 < K) {
#pragma unroll 4
        for (int s = s0 + w; s < s1; s += 4) sum += *(const v4i*)(part + (size_t)s * K + c0);
    }
    red[w][lane] = sum;
    __syncthreads();
    if (w != 0 || c0 >= K) return;
    sum = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
    unsigned int out = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long long q = (2ll * (long long)sum[e] + cnt) / (2ll * cnt);
        out |= ((unsigned int)q & 255u) << (8 * e);
    }
    *(unsigned int*)(centres + (size_t)cell * K + c0) = out;
}

// ---- eg_kmeans_seed_u8 --------------------------------------------------------------------------------------------------------------------
// workgroup = KS_ROWS rows against ONE centre, staged in LDS with its norm.  Wave w takes the rows w, w + 4 .. four at a time (64 lanes x 16
// bytes a step, contiguous): |a|^2 - 2 a.c per lane in uint32 (exact modulo 2^32; d itself is below 2^31), summed over the wave, + |c|^2.
// Then thread = row: mind[i] = first ? d : min(mind[i], d), and the workgroup's int64 sum of the new mind -> partial[workgroup].
__global__ __launch_bounds__(256) void kmeans_seed_dist_kernel(const unsigned char* __restrict__ rows, int n, int K, const unsigned char* __restrict__ centre,
                                                               int first, unsigned int* __restrict__ mind, long long* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cl[];                 // [K]
    __shared__ unsigned int dl[KS_ROWS], cnw[4];
    __shared__ long long ps[(KS_ROWS + 63) / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned int cn = 0;
    for (int k = tid * 16; k < K; k += 256 * 16) {
        const v4i v = *(const v4i*)(centre + k);
        *(v4i*)(cl + k) = v;
        cn += udot16(v, v);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) cn += __shfl_xor(cn, o);
    if (lane == 0) cnw[w] = cn;
    __syncthreads();
    const unsigned int cnorm = cnw[0] + cnw[1] + cnw[2] + cnw[3];
    const long long r0 = (long long)blockIdx.x * KS_ROWS;
    for (int r = w; r < KS_ROWS; r += 16) {
        if (r0 + r >= n) break;                                    // wave-uniform
        unsigned int d[4] = {0, 0, 0, 0};
        for (int k = lane * 16; k < K; k += 1024) {
            const v4i c = *(const v4i*)(cl + k);
            v4i a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long i = r0 + r + 4 * q;
                a[q] = (v4i){0, 0, 0, 0};
                if (r + 4 * q < KS_ROWS && i < n) a[q] = *(const v4i*)(rows + (size_t)i * K + k);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) d[q] += udot16(a[q], a[q]) - 2u * udot16(a[q], c);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned int v = d[q];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
            if (lane == 0 && r + 4 * q < KS_ROWS) dl[r + 4 * q] = v + cnorm;
        }
    }
    __syncthreads();
    if (tid < (KS_ROWS + 63) / 64 * 64) {                          // whole waves
        const long long i = r0 + tid;
        long long v = 0;
        if (tid < KS_ROWS && i < n) {
            unsigned int d = dl[tid];
            if (!first) d = min(d, mind[i]);
            mind[i] = d;
            v = (long long)d;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
        if (lane == 0) ps[w] = v;
    }
    __syncthreads();
    if (tid == 0) {
        long long v = 0;
#pragma unroll
        for (int o = 0; o < (KS_ROWS + 63) / 64; ++o) v += ps[o];
        partial[blockIdx.x] = v;
    }
}

// one workgroup of 1024 threads: pass j's pick.  j == 0: row min(floor(u[0] n), n - 1).  j >= 1: thread t owns `per` consecutive partial
// sums; a scan of the threads' sums gives the total and the one thread whose span holds the target; it walks its span to the workgroup; a
// second scan, over that workgroup's KS_ROWS values of mind, gives the row.  The row -> idx[j] and centres[j]; the flag bits collect in
// state[0] from pass to pass and the last pass writes flag[0].
__global__ __launch_bounds__(1024) void kmeans_seed_pick_kernel(const unsigned char* __restrict__ rows, int n, int K, const float* __restrict__ u, int j,
                                                                int bins, const unsigned int* __restrict__ mind, const long long* __restrict__ partial,
                                                                int nwg, int* __restrict__ state, int* __restrict__ idx,
                                                                unsigned char* __restrict__ centres, int* __restrict__ flag) {
    __shared__ long long wsum[16];
    __shared__ long long sel_rest;
    __shared__ int sel_wg, pick;
    const int tid = threadIdx.x;
    if (tid == 0) {
        sel_wg = -1;
        sel_rest = 0;
        pick = 0;
    }
    const float uj = u[j];
    int bits = uj >= 0.f && uj < 1.f ? 0 : KS_FLAG_U;
    const double ud = uj >= 0.f ? (uj < 1.f ? (double)uj : 1.0) : 0.0;                  // NaN -> 0
    __syncthreads();
    if (j == 0) {
        if (tid == 0) {
            const long long p = (long long)floor(ud * (double)n);
            pick = (int)(p < n - 1 ? p : n - 1);
        }
    } else {
        const int per = (nwg + 1023) / 1024;
        const int g0 = min(tid * per, nwg), g1 = min(g0 + per, nwg);
        long long local = 0;
        for (int g = g0; g < g1; ++g) local += partial[g];
        long long total;
        const long long incl = block_scan_1024(local, wsum, &total);
        if (total <= 0) {
            bits |= KS_FLAG_DUPLICATES;                            // uniform: every thread sees the same total
        } else {
            long long target = (long long)floor(ud * (double)total);
            if (target > total - 1) target = total - 1;
            if (local > 0 && incl - local <= target && target < incl) {                 // exactly one thread
                long long run = incl - local;
                for (int g = g0; g < g1; ++g) {
                    const long long p = partial[g];
                    if (target < run + p) {
                        sel_wg = g;
                        sel_rest = target - run;
                        break;
                    }
                    run += p;
                }
            }
        }
        __syncthreads();
        const int g = sel_wg;
        const long long i = (long long)g * KS_ROWS + tid;
        const long long v = g >= 0 && tid < KS_ROWS && i < n ? (long long)mind[i] : 0;
        long long rows_total;
        const long long rincl = block_scan_1024(v, wsum, &rows_total);
        if (g >= 0 && v > 0 && rincl - v <= sel_rest && sel_rest < rincl) pick = (int)i;   // exactly one thread
    }
    __syncthreads();
    const int row = pick;
    if (tid == 0) {
        idx[j] = row;
        const int all = (j == 0 ? 0 : state[0]) | bits;
        state[0] = all;
        if (j == bins - 1) flag[0] = all;
    }
    for (int k = tid * 16; k < K; k += 1024 * 16) *(v4i*)(centres + (size_t)j * K + k) = *(const v4i*)(rows + (size_t)row * K + k);
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------------
extern "C" int eg_group_rows_block(void) { return GR_BLOCK; }
extern "C" int eg_kmeans_segment_rows(void) { return KM_SEG; }
extern "C" int eg_kmeans_column_chunk(void) { return KM_CC; }
extern "C" int eg_kmeans_seed_rows(void) { return KS_ROWS; }

static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// hist_ws [blocks][bins + 1], then base_ws [blocks][bins]
extern "C" size_t eg_group_rows_ws_bytes(int n, int bins) {
    if (n < 1 || bins < 1) return 0;
    const size_t blocks = ((size_t)n + GR_BLOCK - 1) / GR_BLOCK;
    return up16(blocks * (size_t)(bins + 1) * sizeof(int)) + up16(blocks * (size_t)bins * sizeof(int));
}

extern "C" int eg_group_rows(const int* labels, int n, int bins, void* ws, int* counts, int* offsets, int* order, int* flag, eg_stream_t s) {
    EG_REQUIRE(labels && ws && counts && offsets && order && flag, "eg_group_rows: null pointer");
    EG_REQUIRE(n >= 1, "eg_group_rows: need n >= 1");
    EG_REQUIRE(bins >= 1 && bins <= GR_MAXBINS, "eg_group_rows: need 1 <= bins <= %d (bins = %d)", GR_MAXBINS, bins);
    EG_REQUIRE(((uintptr_t)ws & 15) == 0, "eg_group_rows: ws must be 16-byte aligned");
    EG_REQUIRE((((uintptr_t)labels | (uintptr_t)counts | (uintptr_t)offsets | (uintptr_t)order | (uintptr_t)flag) & 3) == 0,
               "eg_group_rows: labels, counts, offsets, order and flag must be 4-byte aligned");
    const int blocks = (int)(((long long)n + GR_BLOCK - 1) / GR_BLOCK);
    int* hist_ws = (int*)ws;
    int* base_ws = (int*)((char*)ws + up16((size_t)blocks * (size_t)(bins + 1) * sizeof(int)));
    int nbits = 0;
    while ((1 << nbits) < bins) ++nbits;
    hipLaunchKernelGGL(group_count_kernel, dim3(blocks), dim3(GR_THREADS), 0, (hipStream_t)s, labels, n, bins, hist_ws);
    hipLaunchKernelGGL(group_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, (const int*)hist_ws, blocks, bins, base_ws, counts, offsets, flag);
    hipLaunchKernelGGL(group_scatter_kernel, dim3(blocks), dim3(GR_THREADS), 0, (hipStream_t)s, labels, n, bins, nbits, (const int*)base_ws,
                       (const int*)offsets, order);
    EG_LAUNCH_CHECK();
    return 0;
}

static long long kmeans_max_segments(int n, int bins) { return ((long long)n + KM_SEG - 1) / KM_SEG + bins; }

// segbase [bins + 1], then part [segments][K]: sum over the cells of ceil(count / KM_SEG) <= ceil(n / KM_SEG) + bins segments
extern "C" size_t eg_kmeans_update_ws_bytes(int n, int K, int bins) {
    if (n < 1 || K < 1 || bins < 1) return 0;
    return up16((size_t)(bins + 1) * sizeof(int)) + (size_t)kmeans_max_segments(n, bins) * (size_t)K * sizeof(int);
}

extern "C" int eg_kmeans_update_u8(const unsigned char* rows, int n, int K, const int* order, const int* offsets, const int* counts, int bins, void* ws,
                                   unsigned char* centres, eg_stream_t s) {
    EG_REQUIRE(rows && order && offsets && counts && ws && centres, "eg_kmeans_update_u8: null pointer");
    EG_REQUIRE(n >= 1 && (long long)n * 255 < (1ll << 31), "eg_kmeans_update_u8: need 1 <= n and n * 255 < 2^31: the column sums are int32 (n = %d)", n);
    EG_REQUIRE(K >= 64 && K <= 32768 && K % 64 == 0, "eg_kmeans_update_u8: the row length K must be a multiple of 64 in 64 .. 32768 (K = %d)", K);
    EG_REQUIRE(bins >= 1 && bins <= GR_MAXBINS, "eg_kmeans_update_u8: need 1 <= bins <= %d (bins = %d)", GR_MAXBINS, bins);
    EG_REQUIRE((((uintptr_t)rows | (uintptr_t)ws | (uintptr_t)centres) & 15) == 0, "eg_kmeans_update_u8: rows, ws and centres must be 16-byte aligned");
    EG_REQUIRE((((uintptr_t)order | (uintptr_t)offsets | (uintptr_t)counts) & 3) == 0, "eg_kmeans_update_u8: order, offsets and counts must be 4-byte aligned");
    const long long segs = kmeans_max_segments(n, bins);
    int* segbase = (int*)ws;
    int* part = (int*)((char*)ws + up16((size_t)(bins + 1) * sizeof(int)));
    hipLaunchKernelGGL(kmeans_segbase_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, counts, bins, segbase);
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3((unsigned int)segs, cdiv(K, KM_CC)), dim3(256), 0, (hipStream_t)s, rows, n, K, order, offsets, counts,
                       (const int*)segbase, bins, part);
    hipLaunchKernelGGL(kmeans_divide_kernel, dim3(bins, cdiv(K, 256)), dim3(256), 0, (hipStream_t)s, (const int*)part, K, counts, (const int*)segbase, (int)segs,
                       centres);
    EG_LAUNCH_CHECK();
    return 0;
}

// mind [n] uint32, then partial [workgroups] int64, then the state word
extern "C" size_t eg_kmeans_seed_ws_bytes(int n) {
    if (n < 1) return 0;
    const size_t nwg = ((size_t)n + KS_ROWS - 1) / KS_ROWS;
    return up16((size_t)n * sizeof(unsigned int)) + up16(nwg * sizeof(long long)) + 16;
}

extern "C" int eg_kmeans_seed_u8(const unsigned char* rows, int n, int K, int bins, const float* u, void* ws, int* idx, unsigned char* centres, int* flag,
                                 eg_stream_t s) {
    EG_REQUIRE(rows && u && ws && idx && centres && flag, "eg_kmeans_seed_u8: null pointer");
    EG_REQUIRE(n >= 1 && (long long)n <= (1ll << 22), "eg_kmeans_seed_u8: need 1 <= n and n * 2^31 <= 2^53: the sum of the distances is exact in a double (n = %d)", n);
    EG_REQUIRE(K >= 64 && K <= 32768 && K % 64 == 0, "eg_kmeans_seed_u8: the row length K must be a multiple of 64 in 64 .. 32768 (K = %d)", K);
    EG_REQUIRE(bins >= 1 && bins <= GR_MAXBINS, "eg_kmeans_seed_u8: need 1 <= bins <= %d (bins = %d)", GR_MAXBINS, bins);
    EG_REQUIRE((((uintptr_t)rows | (uintptr_t)ws | (uintptr_t)centres) & 15) == 0, "eg_kmeans_seed_u8: rows, ws and centres must be 16-byte aligned");
    EG_REQUIRE((((uintptr_t)u | (uintptr_t)idx | (uintptr_t)flag) & 3) == 0, "eg_kmeans_seed_u8: u, idx and flag must be 4-byte aligned");
    const int nwg = cdiv(n, KS_ROWS);
    unsigned int* mind = (unsigned int*)ws;
    long long* partial = (long long*)((char*)ws + up16((size_t)n * sizeof(unsigned int)));
    int* state = (int*)((char*)partial + up16((size_t)nwg * sizeof(long long)));
    for (int j = 0; j < bins; ++j) {
        if (j > 0)
            hipLaunchKernelGGL(kmeans_seed_dist_kernel, dim3(nwg), dim3(256), (size_t)K, (hipStream_t)s, rows, n, K, (const unsigned char*)centres + (size_t)(j - 1) * K,
                               j == 1 ? 1 : 0, mind, partial);
        hipLaunchKernelGGL(kmeans_seed_pick_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, rows, n, K, u, j, bins, (const unsigned int*)mind,
                           (const long long*)partial, nwg, state, idx, centres, flag);
    }
    EG_LAUNCH_CHECK();
    return 0;
}
