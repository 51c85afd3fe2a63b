// Azimuthally averaged power spectrum of uint8 images (not in the reference): the device half of quality.spectrum.
// The contract, restated in tests/spectrum_refs.py with np.fft.rfft2:
//   X[ky][kx] = sum_y sum_x u[y][x] exp(-2 pi i (ky y + kx x) / H) over the bytes as they are, P = |X|^2 / H^2 (Parseval: sum_k P = sum u^2),
//   on the half spectrum kx = 0 .. H/2; a cell of column kx weighs w = 1 for kx in {0, H/2} and 2 otherwise;
//   profile[n][b] = sum_{cells of ring b} w sum_c P / (C ring_count[b]),  full[n][ky][kx] = sum_c P / C.
// The rings are the caller's integer tables: this file forms no radius and evaluates no sine or cosine; the twiddles are the caller's
// cos_sin table, indexed by (k x) mod H in integers.  float64 throughout.
//
// spectrum_kernel: ONE workgroup per image (grid.x = N), looping over its channels.  Per channel the direct matrix DFT in two stages, each
// a small matrix product on fp64 VALU FMAs with a TY x TX register tile per thread:
//   rows     R[y][kx] = sum_x u[y][x] W^(kx x)        bytes (LDS, 4 per word) x twiddles (LDS) -> H x (H/2 + 1) complex in LDS
//   columns  X[ky][kx] = sum_y W^(ky y) R[y][kx]      complex x complex; |X|^2 / H^2 is added to the thread's own cells in registers
// so the channel sum of a cell is formed by one thread in channel order.  After the last channel the cells go to LDS (over R), `full` is
// written from there, and a wave takes every third ring: lane l adds the ring's cells l, l + 64, ... in the order of ring_cells, then the
// 64 lane sums meet in a fixed xor tree.  No atomics, nothing crosses a workgroup: the bits of image n depend on nothing but its bytes.
// LDS at H = 64: 33 792 (R) + 4096 (bytes) + 1024 (twiddles) = 38 912 bytes.
#include "eg_common.h"

#define SP_THREADS 192
#define SP_MAX_C 4

static int spectrum_rings(int H) { return H == 16 ? 12 : H == 32 ? 24 : H == 64 ? 46 : 0; }

template <int H, int TY, int TX>
__global__ __launch_bounds__(SP_THREADS) void spectrum_kernel(const unsigned char* __restrict__ images, int C, const double* __restrict__ cos_sin,
                                                             const int* __restrict__ ring_start, const int* __restrict__ ring_cells,
                                                             const int* __restrict__ ring_count, int B, double* __restrict__ profile,
                                                             double* __restrict__ full) {
    constexpr int KX = H / 2 + 1, KXG = KX / TX, ACTIVE = KXG * (H / TY), CELLS = H * KX;
    static_assert(KX % TX == 0 && H % TY == 0 && ACTIVE <= SP_THREADS, "the register tiles must cover the half spectrum exactly");
    __shared__ double2 tw[H];                        // (cos, sin)(2 pi k / H)
    __shared__ double2 R[CELLS];                     // stage 1's result; at the end the cells' channel sums (as doubles)
    __shared__ uint32_t img[H * H / 4];              // one channel's bytes
    const int t = threadIdx.x;
    const size_t n = blockIdx.x;
    for (int i = t; i < H; i += SP_THREADS) tw[i] = make_double2(cos_sin[i], cos_sin[H + i]);
    const bool active = t < ACTIVE;
    const int kx0 = (t % KXG) * TX, r0 = (t / KXG) * TY;      // r0: the tile's first y in stage 1, its first ky in stage 2
    const uint32_t* src = (const uint32_t*)(images + n * (size_t)C * (H * H));
    double acc[TY][TX];
#pragma unroll
    for (int j = 0; j < TY; ++j)
#pragma unroll
        for (int i = 0; i < TX; ++i) acc[j][i] = 0.0;

    for (int c = 0; c < C; ++c) {
        __syncthreads();                             // the twiddles are there; the last channel's readers of img and R are done
        for (int i = t; i < H * H / 4; i += SP_THREADS) img[i] = src[(size_t)c * (H * H / 4) + i];
        __syncthreads();
        if (active) {
            double re[TY][TX], im[TY][TX];
#pragma unroll
            for (int j = 0; j < TY; ++j)
#pragma unroll
                for (int i = 0; i < TX; ++i) re[j][i] = im[j][i] = 0.0;
            for (int x4 = 0; x4 < H / 4; ++x4) {
                uint32_t w[TY];
#pragma unroll
                for (int j = 0; j < TY; ++j) w[j] = img[(r0 + j) * (H / 4) + x4];
#pragma unroll
                for (int xx = 0; xx < 4; ++xx) {
                    const int x = x4 * 4 + xx;
                    double2 k[TX];
#pragma unroll
                    for (int i = 0; i < TX; ++i) k[i] = tw[((kx0 + i) * x) & (H - 1)];
#pragma unroll
                    for (int j = 0; j < TY; ++j) {
                        const double u = (double)((w[j] >> (8 * xx)) & 255u);
#pragma unroll
                        for (int i = 0; i < TX; ++i) {
                            re[j][i] = fma(u, k[i].x, re[j][i]);
                            im[j][i] = fma(-u, k[i].y, im[j][i]);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < TY; ++j)
#pragma unroll
                for (int i = 0; i < TX; ++i) R[(r0 + j) * KX + kx0 + i] = make_double2(re[j][i], im[j][i]);
        }
        __syncthreads();
        if (active) {
            double xr[TY][TX], xi[TY][TX];
#pragma unroll
            for (int j = 0; j < TY; ++j)
#pragma unroll
                for (int i = 0; i < TX; ++i) xr[j][i] = xi[j][i] = 0.0;
#pragma unroll 2
            for (int y = 0; y < H; ++y) {
                double2 r[TX];
#pragma unroll
                for (int i = 0; i < TX; ++i) r[i] = R[y * KX + kx0 + i];
#pragma unroll
                for (int j = 0; j < TY; ++j) {
                    const double2 k = tw[((r0 + j) * y) & (H - 1)];
#pragma unroll
                    for (int i = 0; i < TX; ++i) {                       // (r.x + i r.y)(k.x - i k.y)
                        xr[j][i] = fma(r[i].x, k.x, xr[j][i]);
                        xr[j][i] = fma(r[i].y, k.y, xr[j][i]);
                        xi[j][i] = fma(r[i].y, k.x, xi[j][i]);
                        xi[j][i] = fma(-r[i].x, k.y, xi[j][i]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < TY; ++j)
#pragma unroll
                for (int i = 0; i < TX; ++i) acc[j][i] += fma(xr[j][i], xr[j][i], xi[j][i] * xi[j][i]) * (1.0 / (H * H));      // the scale is a power of two
        }
    }

    __syncthreads();
    double* P = (double*)R;                          // [H][KX]: sum over the channels of P
    if (active) {
#pragma unroll
        for (int j = 0; j < TY; ++j)
#pragma unroll
            for (int i = 0; i < TX; ++i) P[(r0 + j) * KX + kx0 + i] = acc[j][i];
    }
    __syncthreads();
    if (full)
        for (int i = t; i < CELLS; i += SP_THREADS) full[n * CELLS + i] = P[i] / (double)C;
    const int lane = t & 63;
    for (int b = t >> 6; b < B; b += SP_THREADS / 64) {
        const int end = min(ring_start[b + 1], CELLS);
        double s = 0.0;
        for (int i = max(ring_start[b], 0) + lane; i < end; i += 64) {
            const int cell = ring_cells[i];
            if ((unsigned)cell < (unsigned)CELLS) {
                const int kx = cell % KX;
                s = fma(kx == 0 || kx == H / 2 ? 1.0 : 2.0, P[cell], s);
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);           // the same tree for every image
        if (lane == 0) profile[n * (size_t)B + b] = s / ((double)C * (double)ring_count[b]);
    }
}

extern "C" int eg_spectrum_u8(const unsigned char* images, int N, int C, int H, const double* cos_sin, const int* cell_ring, const int* ring_start,
                              const int* ring_cells, const int* ring_count, double* profile, double* full, eg_stream_t s) {
    EG_REQUIRE(images && cos_sin && cell_ring && ring_start && ring_cells && ring_count && profile, "eg_spectrum_u8: null pointer");
    EG_REQUIRE(H == 16 || H == 32 || H == 64, "eg_spectrum_u8: the image side must be 16, 32 or 64 (H = %d)", H);
    EG_REQUIRE(C >= 1 && C <= SP_MAX_C, "eg_spectrum_u8: need 1 <= C <= %d (C = %d)", SP_MAX_C, C);
    EG_REQUIRE(N >= 1, "eg_spectrum_u8: need N >= 1");
    EG_REQUIRE(((uintptr_t)images & 3) == 0, "eg_spectrum_u8: images must be 4-byte aligned");
    EG_REQUIRE((((uintptr_t)cell_ring | (uintptr_t)ring_start | (uintptr_t)ring_cells | (uintptr_t)ring_count) & 3) == 0,
               "eg_spectrum_u8: the ring tables must be 4-byte aligned");
    EG_REQUIRE((((uintptr_t)cos_sin | (uintptr_t)profile | (uintptr_t)full) & 7) == 0, "eg_spectrum_u8: cos_sin, profile and full must be 8-byte aligned");
    const int B = spectrum_rings(H);
    const dim3 grid((unsigned)N), block(SP_THREADS);
    if (H == 64)
        hipLaunchKernelGGL((spectrum_kernel<64, 4, 3>), grid, block, 0, (hipStream_t)s, images, C, cos_sin, ring_start, ring_cells, ring_count, B, profile, full);
    else if (H == 32)
        hipLaunchKernelGGL((spectrum_kernel<32, 4, 1>), grid, block, 0, (hipStream_t)s, images, C, cos_sin, ring_start, ring_cells, ring_count, B, profile, full);
    else
        hipLaunchKernelGGL((spectrum_kernel<16, 1, 1>), grid, block, 0, (hipStream_t)s, images, C, cos_sin, ring_start, ring_cells, ring_count, B, profile, full);
    EG_LAUNCH_CHECK();
    return 0;
}
