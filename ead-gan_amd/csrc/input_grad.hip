// Input gradient of a generator's first layer (eg_linear_dinput): the layer's output is stored in a permuted order (NHWC rows of a
// ConvTranspose2d on a 1x1 input, view-permuted Linear outputs), its weight is read from the fp32 MASTER through three strides:
//
//     dX[b][k] = sum_{i < NI} sum_{j < NJ} dH[b][i*NJ + j] * W[i*s_i + j*s_j + k*s_k]
//
// celebA/EAD-GAN_celebA.py:76 (ConvTranspose2d(cin, 1024, 4, 1, 0)), MNIST/EAD-GAN_rpqmnxy.py:77-78 (Linear + view [B,128,8,8]),
// dSprites/rp.py:142 (Linear(cin, 128)).  A skinny GEMM: M = B rows, N = K = the few input columns, a reduction of NI*NJ.
//
// The reduction is cut into chunks of 128 = IC x JC (IC = the power of two >= NI, at most 16: both real layouts have i as the faster axis
// of W, so a chunk reads whole runs of it); a workgroup takes LIN_SPLIT consecutive chunks, a 64-column block of K and a row block of B.
// Per chunk the dH tile (16-byte loads) and the W tile (rounded to the compute dtype on the way, so the values are those of the forward's
// packed panel) go to LDS with the reduction index contiguous, and every wave multiplies its 16 columns by all rows of the block on the
// MFMA units with fp32 accumulators.  More than one split: partial tiles go to the caller's workspace and a second launch adds them in split
// order.  Chunk and split sizes are constants: the result depends on the arguments only -- no atomics, every element of dX is stored,
// nothing is read before it is written.
#include "eg_common.h"

typedef __attribute__((ext_vector_type(4))) float lin_f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 lin_bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 lin_f16x8;

constexpr int LIN_RC = 128;     // reductions per chunk
constexpr int LIN_SPLIT = 4;    // chunks per workgroup
constexpr int LIN_BK = 64;      // columns of K per workgroup: 16 per wave

struct LinDinputParams {
    const void* dH;
    const float* W;
    float* out;                 // partial tiles [nsplit][B][K]; dX itself when there is one split
    int B, NI, NJ, K;
    long long ldh, s_i, s_j, s_k;
    int lic, ljc;               // log2 of IC, JC
    int njb, nchunks;           // chunk c = (i block c / njb, j block c % njb)
    // W tile loader: element e of the IC x JC x 64 tile is (x0 | x1 << a0 | x2 << (a0 + a1)) with x0 along the axis of the smallest stride;
    // pi / pj / pk = which of x0, x1, x2 is i, j, k
    int a0, a1, pi, pj, pk;
};

template <typename T>
__global__ __launch_bounds__(256) void linear_dinput_kernel(const LinDinputParams p) {
    constexpr int VEC = Elt<T>::VEC;
    constexpr int BM = sizeof(T) == 4 ? 32 : 64;          // rows of B per workgroup (both tiles within 64 KiB of LDS)
    constexpr int RT = BM / 16;
    constexpr int LDR = LIN_RC + 16 / (int)sizeof(T);     // 16 bytes of padding per row: the operand reads of 16 rows hit 64 different banks
    __shared__ __attribute__((aligned(16))) T sH[BM * LDR];
    __shared__ __attribute__((aligned(16))) T sW[LIN_BK * LDR];
    const T* __restrict__ dH = reinterpret_cast<const T*>(p.dH);
    const float* __restrict__ W = p.W;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, g = lane >> 4;
    const int k0 = blockIdx.y * LIN_BK, b0 = blockIdx.z * BM;
    const int JCm = (1 << p.ljc) - 1;
    const bool wave_has_columns = k0 + wv * 16 < p.K;

    lin_f32x4 acc[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = (lin_f32x4){0.f, 0.f, 0.f, 0.f};

    for (int cc = 0; cc < LIN_SPLIT; ++cc) {
        const int c = blockIdx.x * LIN_SPLIT + cc;
        if (c >= p.nchunks) break;
        const int i0 = (c / p.njb) << p.lic, j0 = (c % p.njb) << p.ljc;
        __syncthreads();                                   // the previous chunk's operand reads are done
        // Both tiles: all loads of a batch are issued before the first LDS store (an element outside the problem loads element 0, which
        // always exists, and stores zero: unconditional loads, so the batch is in flight together instead of one load per round trip)
        constexpr int HB = BM * (LIN_RC / VEC) / 256;      // 16-byte groups of the dH tile per thread
        uint4 hv[HB];
#pragma unroll
        for (int q = 0; q < HB; ++q) {
            const int e = q * 256 + tid;
            const int row = e / (LIN_RC / VEC), rl = (e % (LIN_RC / VEC)) * VEC;
            const int b = b0 + row, i = i0 + (rl >> p.ljc), j = j0 + (rl & JCm);
            const bool ok = b < p.B && i < p.NI && j < p.NJ;
            const uint4 v = *reinterpret_cast<const uint4*>(dH + (ok ? (size_t)b * p.ldh + (size_t)i * p.NJ + j : 0));
            hv[q] = ok ? v : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < HB; ++q) {
            const int e = q * 256 + tid;
            *reinterpret_cast<uint4*>(sH + (e / (LIN_RC / VEC)) * LDR + (e % (LIN_RC / VEC)) * VEC) = hv[q];
        }
        constexpr int WB = 16;                              // W elements per thread and batch (LIN_RC * LIN_BK / 256 = 32 per chunk)
#pragma unroll 1
        for (int e0 = tid; e0 < LIN_RC * LIN_BK; e0 += 256 * WB) {
            float wv[WB];
            int wo[WB];
#pragma unroll
            for (int q = 0; q < WB; ++q) {
                const int e = e0 + q * 256;
                const int x0 = e & ((1 << p.a0) - 1), x1 = (e >> p.a0) & ((1 << p.a1) - 1), x2 = e >> (p.a0 + p.a1);
                const int il = p.pi == 0 ? x0 : (p.pi == 1 ? x1 : x2);
                const int jl = p.pj == 0 ? x0 : (p.pj == 1 ? x1 : x2);
                const int kl = p.pk == 0 ? x0 : (p.pk == 1 ? x1 : x2);
                const int i = i0 + il, j = j0 + jl, k = k0 + kl;
                const bool ok = i < p.NI && j < p.NJ && k < p.K;
                const float w = W[ok ? i * p.s_i + j * p.s_j + k * p.s_k : 0];
                wv[q] = ok ? w : 0.f;
                wo[q] = kl * LDR + (il << p.ljc) + jl;
            }
#pragma unroll
            for (int q = 0; q < WB; ++q) Elt<T>::st(sW + wo[q], wv[q]);
        }
        __syncthreads();
        if (wave_has_columns) {
            // fragments (C = A B with A = dH rows, B = W columns): lane holds A[row li][k = KS g + e] and B[k = KS g + e][column li]
            const T* wrow = sW + (wv * 16 + li) * LDR;
            if constexpr (sizeof(T) == 4) {
#pragma unroll 8
                for (int s = 0; s < LIN_RC / 4; ++s) {
                    const float bw = wrow[4 * s + g];
#pragma unroll
                    for (int r = 0; r < RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(sH[(r * 16 + li) * LDR + 4 * s + g], bw, acc[r], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int s = 0; s < LIN_RC / 32; ++s) {
                    const uint4 bw = *reinterpret_cast<const uint4*>(wrow + 32 * s + 8 * g);
#pragma unroll
                    for (int r = 0; r < RT; ++r) {
                        const uint4 a = *reinterpret_cast<const uint4*>(sH + (r * 16 + li) * LDR + 32 * s + 8 * g);
                        if constexpr (std::is_same<T, f16_t>::value)
                            acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(lin_f16x8, a), __builtin_bit_cast(lin_f16x8, bw), acc[r], 0, 0, 0);
                        else
                            acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(lin_bf16x8, a), __builtin_bit_cast(lin_bf16x8, bw), acc[r], 0, 0, 0);
                    }
                }
            }
        }
    }
    // accumulator element e of lane (li, g): row 4 g + e, column li of the 16 x 16 tile
    float* out = p.out + (size_t)blockIdx.x * p.B * p.K;
    const int k = k0 + wv * 16 + li;
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int b = b0 + r * 16 + g * 4 + e;
            if (b < p.B && k < p.K) out[(size_t)b * p.K + k] = acc[r][e];
        }
}

__global__ void linear_dinput_reduce_kernel(const float* __restrict__ part, int nsplit, size_t n, float* __restrict__ dX) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    float s = part[idx];
    for (int sp = 1; sp < nsplit; ++sp) s += part[(size_t)sp * n + idx];
    dX[idx] = s;
}

static void lin_chunk_shape(int NI, int* lic, int* ljc) {
    int l = 0;
    while ((1 << l) < NI && l < 4) ++l;
    *lic = l;
    *ljc = 7 - l;                                           // IC * JC == LIN_RC, JC >= 8
}

static int lin_nchunks(int NI, int NJ, int* njb_out) {
    int lic, ljc;
    lin_chunk_shape(NI, &lic, &ljc);
    const int nib = cdiv(NI, 1 << lic), njb = cdiv(NJ, 1 << ljc);
    if (njb_out) *njb_out = njb;
    return nib * njb;
}

static bool lin_shape_ok(int B, int NI, int NJ, int K) {
    return B > 0 && NI > 0 && NJ > 0 && K > 0 && NJ % 8 == 0 && (long long)NI * NJ < (1ll << 31) && (long long)cdiv(NI, 16) * cdiv(NJ, 8) < (1ll << 24);
}

extern "C" size_t eg_linear_dinput_ws_floats(int B, int NI, int NJ, int K) {
    if (!lin_shape_ok(B, NI, NJ, K)) return 0;
    const int nsplit = cdiv(lin_nchunks(NI, NJ, nullptr), LIN_SPLIT);
    return nsplit > 1 ? (size_t)nsplit * B * K : 0;
}

extern "C" int eg_linear_dinput(int dtype, const void* dH, long long ldh, const float* W, float* dX, int B, int NI, int NJ, int K, long long s_i,
                                long long s_j, long long s_k, float* ws, size_t ws_floats, eg_stream_t s) {
    EG_REQUIRE(dH && W && dX, "eg_linear_dinput: null pointer");
    EG_REQUIRE(dtype == EG_F32 || dtype == EG_BF16 || dtype == EG_F16, "dtype must be EG_F32, EG_BF16 or EG_F16");
    EG_REQUIRE(B > 0 && NI > 0 && NJ > 0 && K > 0, "eg_linear_dinput: B, NI, NJ and K must be positive");
    EG_REQUIRE(NJ % 8 == 0, "eg_linear_dinput: NJ must be a multiple of 8 (the vector loads of dH run along j)");
    EG_REQUIRE(lin_shape_ok(B, NI, NJ, K), "eg_linear_dinput: reduction too long");
    EG_REQUIRE(s_i >= 0 && s_j >= 0 && s_k >= 0, "eg_linear_dinput: strides must not be negative");
    EG_REQUIRE(ldh >= (long long)NI * NJ && ldh % 8 == 0 && ((uintptr_t)dH & 15) == 0,
               "eg_linear_dinput: dH rows must be 16-byte aligned (ldh a multiple of 8, at least NI*NJ)");
    LinDinputParams p;
    p.dH = dH; p.W = W; p.B = B; p.NI = NI; p.NJ = NJ; p.K = K; p.ldh = ldh; p.s_i = s_i; p.s_j = s_j; p.s_k = s_k;
    lin_chunk_shape(NI, &p.lic, &p.ljc);
    p.nchunks = lin_nchunks(NI, NJ, &p.njb);
    const int nsplit = cdiv(p.nchunks, LIN_SPLIT);
    const size_t n = (size_t)B * K;
    if (nsplit > 1) {
        EG_REQUIRE(ws, "eg_linear_dinput: null pointer (workspace)");
        EG_REQUIRE(ws_floats >= (size_t)nsplit * n, "eg_linear_dinput: workspace smaller than eg_linear_dinput_ws_floats()");
    }
    p.out = nsplit > 1 ? ws : dX;
    // loader order of the W tile: the axis of the smallest stride runs fastest over the threads (stride 0 -- an axis of extent 1 -- last)
    const long long big = 0x7fffffffffffffffll;
    long long st[3] = {s_i ? s_i : big, s_j ? s_j : big, s_k ? s_k : big};
    const int lg[3] = {p.lic, p.ljc, 6};
    int ord[3] = {0, 1, 2};
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (st[ord[b]] < st[ord[a]]) { const int t = ord[a]; ord[a] = ord[b]; ord[b] = t; }
    int pos[3];
    for (int a = 0; a < 3; ++a) pos[ord[a]] = a;
    p.a0 = lg[ord[0]]; p.a1 = lg[ord[1]];
    p.pi = pos[0]; p.pj = pos[1]; p.pk = pos[2];
    hipStream_t stream = (hipStream_t)s;
    const int bm = dtype == EG_F32 ? 32 : 64;
    const dim3 grid(nsplit, cdiv(K, LIN_BK), cdiv(B, bm));
    EG_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "eg_linear_dinput: B or K too large");
    if (dtype == EG_F32) hipLaunchKernelGGL(linear_dinput_kernel<float>, grid, dim3(256), 0, stream, p);
    else if (dtype == EG_F16) hipLaunchKernelGGL(linear_dinput_kernel<f16_t>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(linear_dinput_kernel<bf16_t>, grid, dim3(256), 0, stream, p);
    if (nsplit > 1) hipLaunchKernelGGL(linear_dinput_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws, nsplit, n, dX);
    EG_LAUNCH_CHECK();
    return 0;
}
