// wgrad_img_tn: weight gradient of the image-side 4x4 / stride-2 / pad-1 layers of the CelebA networks (D's first Conv2d(C -> 128), G's last
// ConvTranspose2d(128 -> C) in conv view) straight from the fp32 images, 16-bit types, 64 x 64 images, N = 128:
//
//     S[n][c*16 + ky*4 + kx] = sum over m = (tape, b, oy, ox) of P[m][n] * img[tape][b][c][2 oy - 1 + ky][2 ox - 1 + kx]
//
// split over m into fp32 slabs [split][128][16 C].  It replaces eg_im2col_img (fp32 image -> 16-bit patch rows in HBM, 16.8 MB per tape
// written and read back) + the per-tap kernel igemm_tn_kernel<T,128,64,64> over those rows, and writes the SAME BITS: one workgroup is one K
// split of that kernel's plan (eg_tn_plan), walks its rows in ascending 32-row MFMA steps (the per-tap kernel's 64-row step is two of them,
// lower half first) and feeds every MFMA the operands the per-tap kernel feeds it -- P as the A operand from transposed LDS reads, the
// patch values as the B operand, K value e of lane group g = row 8 g + e of the step.
//
// A 32-row step is one output row oy of one image (OW = 32):
//   * its P operand is 8 KiB contiguous in memory: eight 1 KiB LDS-DMA pieces, two per wave, 256-byte rows with the 32-byte blocks
//     XOR-swizzled on the source side and read back with ds_read_b64_tr_b16 (the staging of igemm_tn8.hip);
//   * its image operand is rows 2 oy - 1 .. 2 oy + 2 of every channel: ONE 1 KiB piece per channel (4 rows x 256 B of fp32), issued by
//     wave c for channel c; rows -1 and 64 are out-of-range lanes of the piece and land as zeros.  The piece rides in the same ring stage
//     as P, so every byte of a step is behind one counted vmcnt.  (Register loads of the image rows would retire in order with the DMA
//     pieces: waiting for them one step ahead drains the ring.)  Two of the four rows were in the previous step's piece too: the second
//     fetch of a row is an L2 hit, 6 MB per tape beside the 33.5 MB of P.
//   * one step ahead of its use every lane of wave c converts the 16 bytes IT staged to T (Elt<T>::st, the rounding of eg_im2col_img) and
//     writes them to a 16-bit window [2][channel][4 rows][72] whose columns 0 and 65 (x = -1 and 64) stay zero;
//   * the X fragment of column tile j (= channel j; lane column li = (ky, kx) = (li >> 2, li & 3)) is eight stride-2 elements of window row
//     ky starting at column 16 g + kx: nine aligned dwords, a dword shift for kx >= 2 and a byte permute that keeps the low or the high
//     halves.  No patch row exists, in LDS or in HBM.
//   * wave w owns output channels 32 w .. 32 w + 31 and all 16 C columns: 2 C MFMAs per step, every wave walks every step.
//
// Ring of EG_TNI_RING = 7 stages of 12 KiB (8 KiB of P + 4 x 1 KiB of image rows), one barrier per step:
//
//     iteration t:  s_waitcnt vmcnt(pieces of steps t+2 .. t+5) lgkmcnt(0) ; s_barrier
//                   DMA of step t+6 into the stage of step t-1
//                   fragment reads of step t (P from its stage, X from window t & 1) | this lane's image bytes of step t+1 -> window (t+1) & 1
//                   MFMAs of step t
//
// so five steps (40 KiB of P) are in flight per workgroup behind the one being multiplied and the one being converted.
// Hazards.  RAW: the wait in front of barrier t has this wave's pieces of steps <= t+1 landed, the barrier those of every wave: P of step t
// is read behind barrier t (landed by barrier t-1 already), the image bytes of step t+1 are read only by the lane that staged them.  The
// window writes of iteration t-1 are retired by the lgkmcnt(0) in front of barrier t, behind which iteration t reads them.
// WAR: the stage of step t-1 was last read in iteration t-1 (P) and t-2 (image bytes), window (t+1) & 1 in iteration t-1; every wave's
// reads are retired by its lgkmcnt(0) in front of barrier t, and the DMA into that stage and the window writes follow the barrier.
// The compiler issues no VMEM instruction inside the loop, so vmcnt counts the DMA pieces alone.
#include <string.h>

#include "eg_common.h"
#include "igemm_nt.h"

#ifndef EG_TNI_RING
#define EG_TNI_RING 7          // stages of the LDS ring (12 KiB each; 12 is what 160 KiB of LDS hold)
#endif

struct ImgTnParams {
    const float* img[4];      // per tape: [B][C][64][64] fp32
    const void* P;            // [M][128] dtype T, tape-major rows
    float* slab;              // [nsplit][128][16 C]
    int B, M;                 // images per tape; rows = ntapes * B * 1024
    int rows_per_split;       // multiple of 32
};

// vmcnt(pieces) lgkmcnt(0) for `ahead` steps of DMA allowed in flight, 3 pieces per step and wave (`three`: the wave also stages an image
// piece) or 2; vmcnt is six bits wide, its upper two sit in bits 15:14 of the immediate
__device__ __forceinline__ void tni_wait(int ahead, bool three) {
#define EG_TNI_ENC(n) ((((n) & 15) | (7 << 4) | (((n) >> 4) << 14)))
#define EG_TNI_W(a) case a: if (three) __builtin_amdgcn_s_waitcnt(EG_TNI_ENC(3 * a)); else __builtin_amdgcn_s_waitcnt(EG_TNI_ENC(2 * a)); break;
    switch (ahead) {
        EG_TNI_W(1) EG_TNI_W(2) EG_TNI_W(3) EG_TNI_W(4) EG_TNI_W(5) EG_TNI_W(6) EG_TNI_W(7) EG_TNI_W(8) EG_TNI_W(9) EG_TNI_W(10)
        default: __builtin_amdgcn_s_waitcnt(EG_TNI_ENC(0)); break;
    }
#undef EG_TNI_W
#undef EG_TNI_ENC
}

template <typename T, int C>
__global__ __launch_bounds__(256) void wgrad_img_tn_kernel(const ImgTnParams p) {
    constexpr int D = EG_TNI_RING;
    constexpr int ROWB = 256;                            // bytes per K row of P
    constexpr int STAGE_P = 32 * ROWB, STAGE = STAGE_P + 4 * 1024;
    constexpr int WROW = 144, WBUF = 4 * 4 * WROW;       // window: [2][channel][row of the step's four][72 x 16 bit], image column x at x + 1
    constexpr int KC = 16 * C;
    static_assert(D >= 3 && D - 2 <= 10, "cases of tni_wait");
    extern __shared__ __attribute__((aligned(256))) char smem[];
    typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
    typedef __attribute__((address_space(3))) u32x4_t* lds_u4;
    typedef __attribute__((address_space(3))) f32x4* lds_f4;
    typedef __attribute__((address_space(3))) unsigned* lds_u1;
    typedef __attribute__((address_space(3))) unsigned short* lds_h1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15, q = li >> 2, pc = li & 3;
    const int mbeg = blockIdx.x * p.rows_per_split;
    const int mend = min(p.M, mbeg + p.rows_per_split);
    const int nk = (mend - mbeg) >> 5;                   // 32-row steps of this split
    const int s0 = mbeg >> 5;                            // its first step: step s is output row s & 31 of image s >> 5 (over all tapes)
    const unsigned sm0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned win0 = sm0 + D * STAGE;

    for (int i = tid; i < 2 * WBUF / 4; i += 256) *(lds_u1)(size_t)(win0 + 4 * i) = 0u;      // halo columns stay zero
    __syncthreads();

    // ---- P fragment addresses: K rows 8 g + q and + 4 (one swizzle key), 16-channel blocks 2 wave + i ----
    int pk[2];
    {
        const int r = 8 * g + q, key = tn8_fsw(r) & 7;
#pragma unroll
        for (int i = 0; i < 2; ++i) pk[i] = r * ROWB + ((((wave * 2 + i) ^ key) << 5) | (pc << 3));
    }
    // ---- DMA source offsets: lane -> (row rsub of the piece's four, 16-byte chunk c16) ----
    const int c16 = lane & 15, rsub = lane >> 4;
    const u32x4_t srdP = eg_make_srd(p.P, (unsigned)((size_t)p.M * ROWB));
    const unsigned img_bytes = (unsigned)p.B * C * 64u * 256u;
    const u32x4_t srdI0 = eg_make_srd(p.img[0], img_bytes), srdI1 = eg_make_srd(p.img[1], img_bytes), srdI2 = eg_make_srd(p.img[2], img_bytes);
    unsigned vP[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = 4 * (wave + 4 * j) + rsub;
        const int src16 = (((c16 >> 1) ^ (tn8_fsw(r) & 7)) << 1) | (c16 & 1);
        vP[j] = (unsigned)r * ROWB + (unsigned)src16 * 16u;
    }
    const int vI = (wave * 64 + rsub - 1) * 256 + c16 * 16;      // channel `wave`, image row 2 oy - 1 + rsub relative to (image b, channel 0, row 2 oy)
    const unsigned lds0 = sm0 + (unsigned)wave * 1024u;

    auto issue = [&](int s, int stage) {                 // the DMA of step s of this split
        const unsigned base = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)stage * STAGE);
        const unsigned soffP = (unsigned)(mbeg + (s << 5)) * (unsigned)ROWB;
        eg_bufdma1f<0>(srdP, vP[0], soffP, base);
        eg_bufdma1f<0x1000>(srdP, vP[1], soffP, base);
        if (wave < C) {
            const int gs = s0 + s, ib = gs >> 5, oy = gs & 31;
            const int tape = (ib >= p.B ? 1 : 0) + (ib >= 2 * p.B ? 1 : 0), b = ib - tape * p.B;
            const unsigned v = (unsigned)(2 * oy - 1 + rsub) < 64u ? (unsigned)(vI + (b * C * 64 + 2 * oy) * 256) : EG_OOB;
            if (tape == 0) eg_bufdma1f<STAGE_P>(srdI0, v, 0u, base);
            else if (tape == 1) eg_bufdma1f<STAGE_P>(srdI1, v, 0u, base);
            else eg_bufdma1f<STAGE_P>(srdI2, v, 0u, base);
        }
    };
    // this lane's 16 image bytes of the step in `stage` -> T -> window `buf` (waves < C)
    auto convert = [&](int stage, int buf) {
        const f32x4 v = *(lds_f4)(size_t)(lds0 + (unsigned)stage * STAGE + STAGE_P + (unsigned)lane * 16u);
        T h0, h1, h2, h3;
        Elt<T>::st(&h0, v[0]); Elt<T>::st(&h1, v[1]); Elt<T>::st(&h2, v[2]); Elt<T>::st(&h3, v[3]);
        const unsigned w = win0 + (unsigned)(buf * WBUF + (wave * 4 + rsub) * WROW + (1 + 4 * c16) * 2);
        *(lds_h1)(size_t)w = __builtin_bit_cast(unsigned short, h0);
        *(lds_u1)(size_t)(w + 2) = (unsigned)__builtin_bit_cast(unsigned short, h1) | ((unsigned)__builtin_bit_cast(unsigned short, h2) << 16);
        *(lds_h1)(size_t)(w + 6) = __builtin_bit_cast(unsigned short, h3);
    };
    auto tr2 = [&](unsigned a_lo, unsigned a_hi) {       // 8 K-consecutive 16-bit elements of one column: two transposed reads
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(size_t)a_lo);
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(size_t)a_hi);
        return make_uint4(((uint32_t)(uint16_t)lo[0]) | ((uint32_t)(uint16_t)lo[1] << 16), ((uint32_t)(uint16_t)lo[2]) | ((uint32_t)(uint16_t)lo[3] << 16),
                          ((uint32_t)(uint16_t)hi[0]) | ((uint32_t)(uint16_t)hi[1] << 16), ((uint32_t)(uint16_t)hi[2]) | ((uint32_t)(uint16_t)hi[3] << 16));
    };
    // X fragment of channel j: window row ky = q, elements 16 g + kx + 2 e (e = 0..7, kx = pc) = dword 8 g + (kx >> 1) + e, half kx & 1
    const bool xshift = (pc & 2) != 0;
    const unsigned xsel = (pc & 1) ? 0x07060302u : 0x05040100u;
    auto xfrag = [&](int buf, int j) {
        const unsigned a = win0 + (unsigned)(buf * WBUF + (j * 4 + q) * WROW + g * 32);
        const u32x4_t d0 = *(lds_u4)(size_t)a, d1 = *(lds_u4)(size_t)(a + 16);
        const unsigned d8 = *(lds_u1)(size_t)(a + 32);
        const unsigned e0 = xshift ? d0[1] : d0[0], e1 = xshift ? d0[2] : d0[1], e2 = xshift ? d0[3] : d0[2], e3 = xshift ? d1[0] : d0[3];
        const unsigned e4 = xshift ? d1[1] : d1[0], e5 = xshift ? d1[2] : d1[1], e6 = xshift ? d1[3] : d1[2], e7 = xshift ? d8 : d1[3];
        return make_uint4(__builtin_amdgcn_perm(e1, e0, xsel), __builtin_amdgcn_perm(e3, e2, xsel),
                          __builtin_amdgcn_perm(e5, e4, xsel), __builtin_amdgcn_perm(e7, e6, xsel));
    };
    // counted wait (+ barrier): the empty asm statements and sched_barrier(0) keep LDS accesses on their side (see igemm_tn8.hip)
    auto publish = [&](int ahead, bool barrier) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        tni_wait(ahead, wave < C);
        if (barrier) __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    f32x4 acc[2][C];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < C; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ring: step s lives in stage s % D.  Prologue: steps 0 .. D-2 in flight, this wave's pieces of step 0 landed, its image bytes in window 0.
    const int npro = min(nk, D - 1);
    for (int s = 0; s < npro; ++s) issue(s, s);
    publish(max(npro - 1, 0), false);
    if (wave < C && nk > 0) convert(0, 0);
    int st = 0, buf = 0;
    for (int t = 0; t < nk; ++t) {
        const int st1 = st + 1 == D ? 0 : st + 1;        // stage of step t + 1
        const int stp = st == 0 ? D - 1 : st - 1;        // stage of step t - 1 = that of step t + D - 1
        publish(min(max(nk - 2 - t, 0), D - 3), true);
        if (t + D - 1 < nk) issue(t + D - 1, stp);
        const unsigned sb = sm0 + (unsigned)st * STAGE;
        uint4 af[2], xf[C];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = tr2(sb + (unsigned)pk[i], sb + (unsigned)pk[i] + 4 * ROWB);
#pragma unroll
        for (int j = 0; j < C; ++j) xf[j] = xfrag(buf, j);
        if (wave < C && t + 1 < nk) convert(st1, buf ^ 1);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < C; ++j) {
                if constexpr (std::is_same<T, f16_t>::value)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, af[i]), __builtin_bit_cast(f16x8_t, xf[j]), acc[i][j], 0, 0, 0);
                else
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[i]), __builtin_bit_cast(bf16x8_t, xf[j]), acc[i][j], 0, 0, 0);
            }
        st = st1;
        buf ^= 1;
    }

    // ---- slab[split][n][16 C]: acc[i][j][r] = S[n = 32 wave + 16 i + 4 g + r][16 j + li], 64-byte runs ----
    float* slab = p.slab + (size_t)blockIdx.x * 128 * KC;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* row = slab + (size_t)(wave * 32 + i * 16 + g * 4 + r) * KC + li;
#pragma unroll
            for (int j = 0; j < C; ++j) row[j * 16] = acc[i][j][r];
        }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int eg_wgrad_img_tn_ok(int dtype, int C, int H, int W, int N, int k, int stride, int pad) {
    return dtype != EG_F32 && C >= 1 && C <= 4 && N == 128 && k == 4 && stride == 2 && pad == 1 && H == 64 && W == 64;
}

// the per-tap kernel's plan for the patch rows of `images` 64 x 64 images: a 1x1 convolution of 16 C -> 128 channels over 32 x 32 pixels
static void tni_plan(int images, int C, int wgs_target, int* nsplit, int* rps) {
    eg_conv c;
    memset(&c, 0, sizeof(c));
    c.B = images; c.H = 32; c.W = 32; c.Cin = 16 * C; c.Cout = 128; c.k = 1; c.stride = 1;
    eg_tn_plan(&c, wgs_target, nsplit, rps);
}

extern "C" int eg_wgrad_img_tn_plan(int images, int C, int wgs_target, int* rows_per_split) {
    int ns = 0, rps = 0;
    if (images <= 0 || C < 1 || C > 4 || wgs_target < 0) return -1;
    tni_plan(images, C, wgs_target, &ns, &rps);
    if (rows_per_split) *rows_per_split = rps;
    return ns;
}

template <typename T, int C>
static void launch_tni(const ImgTnParams& p, int nsplit, hipStream_t st) {
    constexpr size_t lds = (size_t)EG_TNI_RING * (32 * 256 + 4 * 1024) + 2 * 4 * 4 * 144;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_img_tn_kernel<T, C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((wgrad_img_tn_kernel<T, C>), dim3(nsplit), dim3(256), lds, st, p);
}

template <typename T>
static void launch_tni_c(const ImgTnParams& p, int C, int nsplit, hipStream_t st) {
    if (C == 1) launch_tni<T, 1>(p, nsplit, st);
    else if (C == 2) launch_tni<T, 2>(p, nsplit, st);
    else if (C == 3) launch_tni<T, 3>(p, nsplit, st);
    else launch_tni<T, 4>(p, nsplit, st);
}

extern "C" int eg_wgrad_img_tn(int dtype, const float* img0, const float* img1, const float* img2, int ntapes, const void* P, float* slab, int B, int C,
                               int H, int W, int N, int wgs_target, int* nsplit_out, eg_stream_t s) {
    EG_REQUIRE(img0 && P && slab && nsplit_out && ntapes >= 1 && ntapes <= 3 && B > 0 && wgs_target >= 0, "eg_wgrad_img_tn: bad argument");
    EG_REQUIRE((ntapes < 2 || img1) && (ntapes < 3 || img2), "eg_wgrad_img_tn: one image pointer per tape");
    EG_REQUIRE(eg_wgrad_img_tn_ok(dtype, C, H, W, N, 4, 2, 1), "eg_wgrad_img_tn: 16-bit types, C <= 4, N = 128, 64 x 64 images, 4x4 / stride 2 / pad 1 only (use eg_im2col_img + eg_conv_wgrad)");
    EG_REQUIRE((long long)ntapes * B * 1024 * 256 < 0x7fffffffLL, "eg_wgrad_img_tn: P beyond the 2 GiB a buffer descriptor addresses");
    ImgTnParams p;
    memset(&p, 0, sizeof(p));
    p.img[0] = img0; p.img[1] = ntapes > 1 ? img1 : img0; p.img[2] = ntapes > 2 ? img2 : img0;
    p.P = P; p.slab = slab; p.B = B; p.M = ntapes * B * 1024;
    int ns = 0;
    tni_plan(ntapes * B, C, wgs_target, &ns, &p.rows_per_split);
    if (dtype == EG_F16) launch_tni_c<f16_t>(p, C, ns, (hipStream_t)s);
    else launch_tni_c<bf16_t>(p, C, ns, (hipStream_t)s);
    *nsplit_out = ns;
    EG_LAUNCH_CHECK();
    return 0;
}
