// Exponential moving average of a trainer's weights: ONE launch updates every tracked tensor -- the flat fp32 arena of each
// tracked module, its BatchNorm running statistics (lerp) and its integer / unit-vector buffers (bit copy) -- from a segment table that
// lives on the device, so the launch is a node of the captured iteration and a replay reads no host memory.  Not in the reference:
// its scripts sample from the live weights.
// Roofline class: HBM streaming (2 reads + 1 write of 4 bytes per lerp word, no reuse); no LDS.  A fixed grid of EMA_GRID workgroups
// walks the chunks grid-stride (the entry point gets no chunk total: it would have to come from the host); workgroups beyond the
// table's chunks leave at once.  Two workgroups of 8 waves per CU, every thread with 4 x 16 bytes of each operand in flight.
// Measured figures and the register count: DESIGN 6l.
#include "eg_common.h"

#define EMA_THREADS 512
#define EMA_VEC 4                                             // 16-byte groups per thread and chunk
#define EMA_CHUNK_WORDS (EMA_THREADS * 4 * EMA_VEC)           // 8192 words = 32 KiB: a multiple of 16 bytes, so a chunk starts as aligned as its segment
#define EMA_GRID 512

// the table's pointers come out of memory as generic ones: in the global address space the accesses are global_load / global_store, not flat
typedef __attribute__((address_space(1))) uint32_t g_u32;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;

// the words [0, cnt) of one chunk.  LERP: dst = fmaf(a, src - dst, dst) on fp32; else dst = src, word for word
template <bool LERP>
__device__ __forceinline__ void ema_chunk(const g_u32* __restrict__ src, g_u32* __restrict__ dst, unsigned cnt, float a) {
    const unsigned tid = threadIdx.x;
    auto one = [&](unsigned i) {
        if (LERP) {
            const float s = __uint_as_float(src[i]), d = __uint_as_float(dst[i]);
            dst[i] = __float_as_uint(fmaf(a, s - d, d));
        } else {
            dst[i] = src[i];
        }
    };
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) != 0) {      // any other 4-byte alignment: correct, not fast
        for (unsigned i = tid; i < cnt; i += EMA_THREADS) one(i);
        return;
    }
    const unsigned nv = cnt >> 2;
    const g_u32x4* s4 = (const g_u32x4*)src;
    g_u32x4* d4 = (g_u32x4*)dst;
    u32x4 s[EMA_VEC], d[EMA_VEC];
#pragma unroll
    for (int k = 0; k < EMA_VEC; ++k) {                       // every load of the chunk is issued before the first use
        const unsigned i = tid + k * EMA_THREADS;
        if (i < nv) {
            s[k] = s4[i];
            if (LERP) d[k] = d4[i];
        }
    }
#pragma unroll
    for (int k = 0; k < EMA_VEC; ++k) {
        const unsigned i = tid + k * EMA_THREADS;
        if (i < nv) {
            if (LERP) {
                const float dx = __uint_as_float(d[k].x), dy = __uint_as_float(d[k].y), dz = __uint_as_float(d[k].z), dw = __uint_as_float(d[k].w);
                s[k].x = __float_as_uint(fmaf(a, __uint_as_float(s[k].x) - dx, dx));
                s[k].y = __float_as_uint(fmaf(a, __uint_as_float(s[k].y) - dy, dy));
                s[k].z = __float_as_uint(fmaf(a, __uint_as_float(s[k].z) - dz, dz));
                s[k].w = __float_as_uint(fmaf(a, __uint_as_float(s[k].w) - dw, dw));
            }
            d4[i] = s[k];
        }
    }
    if (tid < (cnt & 3u)) one((nv << 2) + tid);               // the up to 3 words behind the last whole group of a segment
}

// updates[0] = t, the number of updates done so far (every workgroup reads it before it arrives, the last arriver writes t + 1);
// updates[1] = arrivals, zero between launches
__global__ void __launch_bounds__(EMA_THREADS) ema_update_kernel(const eg_ema_seg* __restrict__ segs, const unsigned* __restrict__ chunk_first, int nseg,
                                                                 float beta, float ramp, int* updates) {
    const unsigned total = chunk_first[nseg];
    if (blockIdx.x >= total) return;                          // a table smaller than the grid: no chunk, and not among the arrivals
    const int t = __hip_atomic_load(updates, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    float b = beta;
    if (ramp != 0.f) {
        const float tf = (float)t;
        b = fminf(beta, __fdiv_rn(1.f + tf, ramp + tf));      // engine.ema_decay: the same three fp32 operations
    }
    const float a = 1.f - b;
    for (unsigned chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
        int lo = 0, hi = nseg;                                // chunk_first[lo] <= chunk < chunk_first[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (chunk_first[mid] <= chunk) lo = mid;
            else hi = mid;
        }
        const eg_ema_seg g = segs[lo];
        const size_t off = (size_t)(chunk - chunk_first[lo]) * EMA_CHUNK_WORDS;
        const size_t left = g.n - off;
        const unsigned cnt = left < (size_t)EMA_CHUNK_WORDS ? (unsigned)left : (unsigned)EMA_CHUNK_WORDS;
        const g_u32* src = (const g_u32*)g.src + off;
        g_u32* dst = (g_u32*)g.dst + off;
        if (g.kind == 0) ema_chunk<true>(src, dst, cnt, a);
        else ema_chunk<false>(src, dst, cnt, a);
    }
    // arrival counter (protocol: igemm_nt8s.hip): every thread's load of t has returned, workgroup barrier, ONE lane adds at agent
    // scope; the last of the workgroups that had a chunk publishes t + 1 and leaves the counter at zero for the next launch
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned arrive = total < gridDim.x ? total : gridDim.x;
        const int prev = __hip_atomic_fetch_add(updates + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)prev == arrive - 1) {
            __hip_atomic_store(updates + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(updates, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

extern "C" int eg_ema_chunk_words(void) { return EMA_CHUNK_WORDS; }

// host only: the validation a device table cannot have, and the exclusive prefix of the segments' chunk counts
extern "C" int eg_ema_plan(const eg_ema_seg* segs_host, int nseg, unsigned int* chunk_first_host) {
    EG_REQUIRE(segs_host && chunk_first_host, "eg_ema_plan: null pointer");
    EG_REQUIRE(nseg >= 1 && nseg <= EG_EMA_MAX_SEGS, "eg_ema_plan: nseg must be in 1..%d, got %d", EG_EMA_MAX_SEGS, nseg);
    unsigned long long chunks = 0;
    for (int i = 0; i < nseg; ++i) {
        const eg_ema_seg& g = segs_host[i];
        EG_REQUIRE(g.src && g.dst, "eg_ema_plan: segment %d: null src or dst", i);
        EG_REQUIRE(g.n > 0, "eg_ema_plan: segment %d: n == 0", i);
        EG_REQUIRE(g.kind == 0 || g.kind == 1, "eg_ema_plan: segment %d: kind must be 0 (lerp) or 1 (copy), got %d", i, g.kind);
        EG_REQUIRE(((reinterpret_cast<uintptr_t>(g.src) | reinterpret_cast<uintptr_t>(g.dst)) & 3) == 0,
                   "eg_ema_plan: segment %d: src and dst must be 4-byte aligned", i);
        EG_REQUIRE(g.src != g.dst, "eg_ema_plan: segment %d: src == dst", i);
        chunk_first_host[i] = (unsigned int)chunks;
        chunks += (unsigned long long)(g.n / EMA_CHUNK_WORDS) + (g.n % EMA_CHUNK_WORDS != 0);
        EG_REQUIRE(chunks <= (1ull << 31), "eg_ema_plan: more than 2^31 chunks (through segment %d)", i);
    }
    chunk_first_host[nseg] = (unsigned int)chunks;
    return 0;
}

extern "C" int eg_ema_update(const eg_ema_seg* segs_dev, const unsigned int* chunk_first_dev, int nseg, float beta, float ramp, int* updates,
                             eg_stream_t s) {
    EG_REQUIRE(segs_dev && chunk_first_dev && updates, "eg_ema_update: null pointer");
    EG_REQUIRE(nseg >= 1 && nseg <= EG_EMA_MAX_SEGS, "eg_ema_update: nseg must be in 1..%d, got %d", EG_EMA_MAX_SEGS, nseg);
    EG_REQUIRE(beta >= 0.f && beta < 1.f, "eg_ema_update: beta must be in [0, 1)");
    EG_REQUIRE(ramp >= 0.f, "eg_ema_update: ramp must be >= 0");
    hipLaunchKernelGGL(ema_update_kernel, dim3(EMA_GRID), dim3(EMA_THREADS), 0, (hipStream_t)s, segs_dev, chunk_first_dev, nseg, beta, ramp, updates);
    EG_LAUNCH_CHECK();
    return 0;
}
