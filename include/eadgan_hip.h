/* libeadgan_hip.so -- C ABI of the MI355X-native EAD-GAN training hot path (gfx950 / CDNA4).
 *
 * The reference (letao1991/EAD-GAN) is pure PyTorch: it has no FFI of its own.  Its hot path calls the
 * torch operators listed per entry point below (file:line relative to the reference root); each entry
 * point here is the hand-written HIP replacement that the Python host layer (ead-gan_amd/) binds with
 * ctypes.  INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (tensor.data_ptr()); nothing is allocated,
 *     freed or retained by the library; workspaces are passed in explicitly;
 *   - every call is an asynchronous enqueue on `stream` (hipStream_t passed as void*), no device sync,
 *     graph-capturable;
 *   - return value: 0 ok, <0 argument error, >0 hipError_t; eg_last_error() gives the text;
 *   - activations are NHWC ("pixel-major") in dtype T (EG_F32, EG_BF16 or EG_F16); images at the module boundary
 *     are NCHW fp32 like the reference's tensors; master weights / gradients / optimizer state are fp32
 *     in the reference's own layouts ([Cout][Cin][kh][kw] for Conv2d, [Cin][Cout][kh][kw] for
 *     ConvTranspose2d);
 *   - "conv view": a ConvTranspose2d(Ci->Co,k,s,p) layer is described as the Conv2d(Co->Ci,k,s,p) whose
 *     backward-data it is; its forward is eg_conv_bwd_data, its input gradient eg_conv_fwd.
 */
#ifndef EADGAN_HIP_H
#define EADGAN_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* eg_stream_t;

enum { EG_F32 = 0, EG_BF16 = 1, EG_F16 = 2 };   /* compute / activation dtype T; masters, statistics, losses and Adam are always fp32 */
enum { EG_ACT_NONE = 0, EG_ACT_LRELU = 1, EG_ACT_RELU = 2, EG_ACT_TANH = 3, EG_ACT_SIGMOID = 4 };
enum { EG_OUT_NHWC = 0, EG_OUT_NCHW_F32 = 1 };

int eg_version(void);
const char* eg_last_error(void);
/* drain HIP's sticky last-error slot after a failed hipGraph capture (returns the number of pending errors) */
int eg_clear_errors(void);

/* One square 2-D convolution in conv view.  X is [B,H,W,Cin] (NHWC); if up==1 the conv reads the
 * nearest-2x-upsampled X (nn.Upsample fused, MNIST/EAD-GAN_rpqmnxy.py:81,85).  Y is [B,OH,OW,Cout],
 * OH = ((H<<up) + 2*pad - k)/stride + 1.  All spatial extents must be powers of two.
 * Refused (-1, before anything is launched; the queries answer -1 / 0): B, k, stride, Cin, Cout, H or W <= 0, pad < 0, up outside 0 / 1,
 * B * OH * OW >= 2^31, a gathered channel count that is no multiple of the 16-byte vector (4 fp32 / 8 16-bit elements); for the
 * backward-data pass also stride > 2, OH != (H<<up)/stride and k < stride (a sub-pixel phase without a tap). */
typedef struct eg_conv {
    int B, H, W, Cin, Cout, k, stride, pad, up;
} eg_conv;

/* Fused epilogue of the implicit-GEMM kernels:  v = acc [/ sigma[tape]] [+ bias[n % bias_mod]] ;
 * v = act(v) ; [v *= act'(mask)] ; store.  `mask` holds the activation OUTPUT of the layer whose
 * gradient is being formed (same dtype and layout as dst), so LeakyReLU/ReLU backward never needs a
 * separate pass.  Several forwards of one network ("tapes", each with its own spectral-norm sigma) can be
 * batched along M: tape = lattice_row / sigma_rows (sigma_rows == 0: one sigma for the whole launch).
 * Contract, checked in one place before any launch (eg_conv_fwd / eg_conv_bwd_data return -1; eg_igemm_nt_tile_ep answers -1,
 * eg_conv_stat_blocks 0): act, mask_act and (with a stat_mode) stat_act are EG_ACT_* codes, out_mode is an EG_OUT_* code, bias_mod >= 0
 * (0: bias[n]) and sigma_rows >= 0.  EG_OUT_NCHW_F32 stores fp32 [B][N][DH][DW] and reads `mask` in that layout and type; only the
 * register-staged kernel writes it (a forced DMA variant is refused). */
typedef struct eg_epilogue {
    const float* bias;
    int bias_mod;
    const float* sigma;
    int act;
    float slope;
    const void* mask;
    int mask_act;
    float mask_slope;
    int out_mode;
    int sigma_rows;
    void* splitk_ws;          /* optional caller-owned scratch: lets small-M / deep-K launches split K across workgroups (fp32 partial */
    size_t splitk_ws_bytes;   /* tiles, summed in split order -- inside the launch by the last-arriving workgroup, or by a second launch); */
                              /* NULL / 0 = never split.  ZERO it once before the first use: its last 4 KiB hold arrival counters that */
                              /* every launch leaves at zero.  One scratch must not be lent to two launches that may run concurrently. */
    int nt_variant;           /* EG_NT_AUTO (0): the planner picks the kernel; otherwise force one (the call fails if it cannot run the problem) */
    int nt_splitk;            /* 0: the planner picks the K split; n >= 1: at most n splits (1 = never) */
    /* Column statistics of the stored tile, fused into the epilogue (EG_STAT_*; 0 = none): the reductions that follow a convolution in the
     * reference's graph -- BatchNorm batch statistics (celebA/EAD-GAN_celebA.py:79,83,87), the two sums of the BatchNorm backward, the bias
     * gradient + spectral-norm coefficient of a spectrally normalised layer (:110-122) -- taken from the tile while it is in LDS instead of
     * by a kernel that re-reads the whole tensor.  Only launches that eg_conv_stat_blocks() answers > 0 for may set it (the 8-wave kernel
     * on whole 256-row tiles); such a launch fails otherwise.  Per row block rb = phase * tiles_m + m_tile (256 lattice rows) and column n:
     *   stat_out[(0 * N + n) * nrb + rb], stat_out[(1 * N + n) * nrb + rb]     (nrb = eg_conv_stat_blocks())
     * deterministic (fixed order inside a tile; the consumers eg_bn_fwd_train_fused / eg_bn_bwd_fused / eg_bias_grad_sn_fused sum the row
     * blocks in a fixed order).
     *   EG_STAT_MOMENTS : (mean, M2) of the 256 stored values of the column
     *   EG_STAT_BN_BWD  : the launch computes da = the gradient w.r.t. a BatchNorm layer's activation output.  stat_aux = z (the BatchNorm
     *                     input, layout of dst), stat_p0..p3 = save_mean, save_invstd, gamma, beta, stat_act / stat_slope = the activation
     *                     behind the BatchNorm.  STORES dy = da * act'(bn(z)) instead of da; sums (sum dy, sum dy * xhat)
     *   EG_STAT_SN_BIAS : the launch computes dzs = dz / sigma of a spectrally normalised LeakyReLU layer (mask = its activation output a,
     *                     mask_act = EG_ACT_LRELU); stat_p0 = the layer's bias.  Sums (sum dzs, sum dzs * (lrelu^-1(a) - bias)); the second
     *                     sum is further reduced over the tile's 128 columns: stat_out[N * nrb + rb * (N / 128) + n_tile] */
    int stat_mode;
    float* stat_out;
    const void* stat_aux;
    const float* stat_p0;
    const float* stat_p1;
    const float* stat_p2;
    const float* stat_p3;
    int stat_act;
    float stat_slope;
} eg_epilogue;
enum { EG_STAT_NONE = 0, EG_STAT_MOMENTS = 1, EG_STAT_BN_BWD = 2, EG_STAT_SN_BIAS = 3 };

/* kernels behind eg_conv_fwd / eg_conv_bwd_data.  The choice is a pure function of the problem and of these two per-call fields:
 * the library holds no tuning state.  All variants accumulate K in the same order: without a K split they are bit-identical. */
#define EG_NT_AUTO 0
#define EG_NT_REG 1      /* register-staged 128 x {16,32,64,128} tiles: every problem; the reference of the others */
#define EG_NT_BUF128 2   /* 128 x 128, 4 waves (two workgroups per CU), 2-stage buffer-descriptor LDS-DMA ring */
#define EG_NT_PERS 3     /* persistent 128 x 128 pipeline (1-2-step image-side layers) */
#define EG_NT_S8 4       /* 256 x 128, 8 waves, 3-K-tile LDS-DMA ring, one barrier per K tile, fragments double-buffered in registers */
#define EG_NT_S8H 6      /* the 8-wave design on 128 x 128 tiles (waves 4 x 2, wave tile 32 x 64), ring of four K tiles: launches with too few 256-row tiles */
#define EG_NT_S8P 5      /* the same with the A operand held in LDS as an input patch shared by the filter taps of a class: 2.6-3.5x
                          * fewer A bytes through the LDS-DMA path; K is accumulated class by class (deterministic, not bit-identical
                          * to the tap-major variants) */

/* --- implicit-GEMM convolution family (MFMA) ---------------------------------------------------
 * replaces torch.nn.functional.conv2d / conv_transpose2d / linear and their autograd backward:
 *   celebA/EAD-GAN_celebA.py:76-90,110-122   dSprites/rp.py:95-110,129-146
 *   MNIST/EAD-GAN_rpqmnxy.py:77-90,107-124,143-163 */
size_t eg_pack_fwd_elems(const eg_conv* c, int dtype);                 /* elements of Wp_fwd */
size_t eg_pack_bwd_elems(const eg_conv* c, int dtype);                 /* elements of Wp_bwd */
int eg_pack_fwd(const eg_conv* c, int dtype, const float* w_master, void* wp, eg_stream_t s);
int eg_pack_bwd(const eg_conv* c, int dtype, const float* w_master, void* wp, eg_stream_t s);
/* both panels in one pass over the master (either destination may be NULL); same bytes as eg_pack_fwd + eg_pack_bwd */
int eg_pack_conv(const eg_conv* c, int dtype, const float* w_master, void* wp_fwd, void* wp_bwd, eg_stream_t s);
/* Y = conv(X, W) */
int eg_conv_fwd(const eg_conv* c, int dtype, const void* X, const void* wp_fwd, void* Y,
                const eg_epilogue* ep, eg_stream_t s);
/* dX = conv^T(dY, W)  (== ConvTranspose2d forward); dX has spatial dims (H<<up, W<<up) */
int eg_conv_bwd_data(const eg_conv* c, int dtype, const void* dY, const void* wp_bwd, void* dX,
                     const eg_epilogue* ep, eg_stream_t s);
/* which kernel eg_conv_fwd (bwd = 0) / eg_conv_bwd_data (bwd = 1) runs this problem on under the given hints (same planner as the
 * launches, unlimited split-K scratch): BM * 1000 + code; code = BN of the register-staged kernels, 131 / 132 = 128 x 128
 * buffer-descriptor kernel (plain / split-K), 135 = persistent pipeline, 147 / 148 = igemm_nt8s (plain / split-K), 149 / 150 =
 * igemm_nt8s with the input patch, 151 / 152 = igemm_nt8h (plain / split-K); -1 = the forced variant cannot run the problem.  Profiling labels and tests. */
int eg_igemm_nt_tile(const eg_conv* c, int dtype, int bwd, int variant, int splitk);
/* the same for ONE concrete call: the epilogue's kernel hints and ITS split-K scratch (what the launch itself will do) */
int eg_igemm_nt_tile_ep(const eg_conv* c, int dtype, int bwd, const eg_epilogue* ep);
/* row blocks (nrb) of the column statistics that THIS call -- eg_conv_fwd (bwd = 0) / eg_conv_bwd_data (bwd = 1) with this epilogue, its
 * kernel hints and its split-K scratch -- would write if stat_mode were set; 0 = the launch cannot fuse them (another kernel than the
 * 8-wave one, ragged row tiles, splits reduced by a second launch): the caller then runs the stand-alone reduction kernels. */
int eg_conv_stat_blocks(const eg_conv* c, int dtype, int bwd, const eg_epilogue* ep);
/* bytes of eg_epilogue.splitk_ws that let eg_conv_fwd (bwd = 0) / eg_conv_bwd_data (bwd = 1) split as far as the policy wants */
size_t eg_conv_splitk_ws_bytes(const eg_conv* c, int dtype, int bwd);
/* dW partial slabs: slab[split][Cout][k*k][Cin] fp32.  Returns the split count through *nsplit.  16-bit 4x4 / stride-2 / pad-1 layers
 * whose channel counts are multiples of 128 run on the parity-class kernel (igemm_tn8.hip: the four taps of an input-parity class share
 * one input patch and one tile of dY per K step), everything else on the per-tap kernel; eg_conv_wgrad_variant tells which (2 / 1). */
int eg_conv_wgrad_variant(const eg_conv* c, int dtype);
size_t eg_conv_wgrad_ws_bytes(const eg_conv* c, int dtype);
/* wgs_target: the caller's share of the chip = workgroups the parity-class kernel should aim for (0 = one per CU).  A launch forked onto
 * a side stream beside the main chain's GEMMs passes 128 (half the slab to write and reduce, the other CUs stay with the main chain);
 * never more splits than eg_conv_wgrad_ws_bytes provides for. */
int eg_conv_wgrad(const eg_conv* c, int dtype, const void* X, const void* dY, float* slab, int* nsplit,
                  int wgs_target, eg_stream_t s);
/* Gradient writers.  Every entry point from here on that writes a parameter gradient ("(+)=" below) takes `accumulate` in front of the
 * stream: accumulate != 0 adds to the slot (autograd's .grad contract), accumulate == 0 stores the same sum without reading the slot
 * (what accumulating into a cleared slot gives, up to the sign of a zero). */
/* grad[n][c][t] (+)= sum_split slab[split][n][t][c]  for n < n_rows (slab rows: n_slab >= n_rows);
 * C = gathered channels, T = taps.  Master layouts [Cout][Cin][k][k] / [Cin_T][Cout_T][k][k] are both [n][c][t]. */
int eg_wgrad_reduce(const float* slab, int nsplit, int n_slab, int n_rows, int C, int T, float* grad,
                    int accumulate, eg_stream_t s);
/* same with a row permutation: slab row n lands in gradient row (n % row_div) * row_mul + n / row_div
 * (Linear whose output is viewed [B,C,H,W] and kept NHWC on device: MNIST/EAD-GAN_rpqmnxy.py:77,95-96) */
int eg_wgrad_reduce_perm(const float* slab, int nsplit, int n_slab, int n_rows, int C, int T, float* grad,
                         int row_div, int row_mul, int c_row /* destination row length in channels, 0 = C */, int accumulate, eg_stream_t s);
/* out[i] += src[(i / div) * s_div + (i % div) * s_mod]   (un-permute a bias gradient) */
int eg_gather_add(float* out, const float* src, int n, int div, int s_div, int s_mod, eg_stream_t s);
/* y[B,H,W,C] = 2x2 sum-pool of x[B,2H,2W,C]  (backward of nn.Upsample(scale_factor=2), MNIST/EAD-GAN_rpqmnxy.py:81,85) */
int eg_sumpool2x2(int dtype, const void* x, void* y, int B, int H, int W, int C, eg_stream_t s);
/* weight gradient of Conv2d(64, 1, 3, 1, 1) -- the MNIST generator's last layer (MNIST/EAD-GAN_rpqmnxy.py:88) -- with the activation read ONCE
 * (lane = input channel, nine per-lane accumulators, dy [B][H][W] fp32 broadcast from LDS after a pass through the compute dtype): x
 * [B][H][W][64] dtype T; writes slab[split][9][64] for eg_wgrad_reduce(slab, *nsplit_out, 1, 1, 64, 9, grad); the slab must hold
 * eg_wgrad_c1_splits(B, H) * 576 floats.  Replaces eg_cast_pad + the per-tap eg_conv_wgrad over the output padded to 8 channels. */
int eg_wgrad_c1_ok(int dtype, int C, int H, int W, int Cout, int k, int stride, int pad);
int eg_wgrad_c1_splits(int B, int H);
int eg_wgrad_c1(int dtype, const void* x, const float* dy, float* slab, int B, int H, int W, int C, int* nsplit_out, eg_stream_t s);
/* nn.Upsample(scale_factor=2) + Conv2d(Cin -> Cout, 3, 1, 1) run as ConvTranspose2d(Cin -> Cout, 4, 2, 1) with summed taps
 * (MNIST/EAD-GAN_rpqmnxy.py:81-82, 85-86): eg_up3_expand writes the effective master w4t[Cin][Cout][4][4] (W4[kh] = sum of the 3x3 taps
 * t in [max(0, 2-kh), min(2, 3-kh)], rows and columns alike) from w3[Cout][Cin][3][3]; eg_up3_contract takes the weight gradient of the
 * transposed convolution back through the transpose of that map: dw3 (+)= E^T dw4t E.  fp32 masters / gradients only. */
int eg_up3_expand(const float* w3, float* w4t, int Cout, int Cin, eg_stream_t s);
int eg_up3_contract(const float* dw4t, float* dw3, int Cout, int Cin, int accumulate, eg_stream_t s);
/* spectral-norm variant (torch.nn.utils.spectral_norm backward, celebA/EAD-GAN_celebA.py:110-120):
 * G = sum slab ;  grad (+)= G/sigma - (<G,W_orig>/sigma^2) u v^T.  gtmp: Cout*Cin*k*k floats,
 * partials: >= eg_sn_partials() floats. */
int eg_sn_partials(void);
int eg_wgrad_reduce_sn(const eg_conv* c, const float* slab, int nsplit, const float* w_orig,
                       const float* sigma, const float* u, const float* v, float* gtmp, float* partials,
                       float* grad, int accumulate, eg_stream_t s);
/* per-output-channel bias gradient: gb[n % bias_mod] (+)= sum_rows dY[row][n]  (dY is [rows][N] dtype T) */
size_t eg_bias_grad_ws_floats(int rows, int N);
int eg_bias_grad(int dtype, const void* dY, int rows, int N, int bias_mod, float* partials, float* gb,
                 int accumulate, eg_stream_t s);
/* Batched-tape form for spectrally normalised layers.  dzs holds dL/dz ALREADY divided by the tape's sigma
 * (dzs = dz / sigma[tape]); a = activation output (LeakyReLU), bias = the layer's bias.  Computes
 *   gb[n]  (+)= sum_tape sigma[tape] * sum_{rows of tape} dzs[row][n]
 *   coef[t]  = sum_{rows of tape t, n} dzs[row][n] * (lrelu^-1(a[row][n]) - bias[n])      (== <G_t, W_orig> / sigma_t^2)
 * ws: eg_bias_grad_sn_ws_floats(rows, N, rows_per_tape) floats. */
size_t eg_bias_grad_sn_ws_floats(int rows, int N, int rows_per_tape);
int eg_bias_grad_sn(int dtype, const void* dzs, const void* a, const float* bias, int rows, int N, int rows_per_tape,
                    const float* sigma, float slope, float* ws, float* gb, float* coef, int accumulate, eg_stream_t s);
/* eg_bias_grad_sn with the per-tile sums taken from the epilogue of the convolution that produced dzs (EG_STAT_SN_BIAS): stat = its
 * stat_out (nrb = nphase * tiles_m row blocks of 256 lattice rows; tape of a row block = (rb % tiles_m) / tiles_per_tape) */
int eg_bias_grad_sn_fused(const float* stat, int nrb, int N, int tiles_m, int tiles_per_tape, int ntapes, const float* sigma, float* gb,
                          float* coef, int accumulate, eg_stream_t s);
/* grad[n][c][t] (+)= sum_split slab[split][n][t][c] - sum_tape coef[tape] * u[tape][n] * v[tape][c*T + t]
 * (u: [ntapes][n_rows], v: [ntapes][c_row*T]); single pass, deterministic.  c_row: destination row length in channels
 * (0 = C; < C when the gathered operand was zero padded, e.g. 9 of 16 im2col columns). */
int eg_wgrad_reduce_rank1(const float* slab, int nsplit, int n_slab, int n_rows, int C, int T, float* grad,
                          int ntapes, const float* coef, const float* u, const float* v, int c_row, int accumulate, eg_stream_t s);
/* wp[n][k] = w[(n / n_div) * s_hi + (n % n_div) * s_lo + k * s_k], zero for K <= k < Kpad
 * (ConvTranspose2d on a 1x1 input as a GEMM: celebA/EAD-GAN_celebA.py:76; view-permuted Linear outputs) */
int eg_pack_strided(int dtype, const float* w, void* wp, int N, int K, int Kpad, int n_div, long long s_hi,
                    long long s_lo, long long s_k, eg_stream_t s);

/* Input gradient of a first layer whose output is stored in a permuted order (the layers eg_pack_strided packs: celebA/EAD-GAN_celebA.py:76,
 * MNIST/EAD-GAN_rpqmnxy.py:77-78, dSprites/rp.py:142):
 *     dX[b][k] = sum_{i < NI} sum_{j < NJ} dH[b][i*NJ + j] * W[i*s_i + j*s_j + k*s_k]        b < B, k < K
 * dH: dtype T, row stride ldh elements (16-byte aligned rows); W: the fp32 MASTER, rounded to T in registers (the values the forward's
 * packed panel holds -- there is no panel of its own to re-pack); dX: fp32 [B][K], exactly K columns; fp32 accumulation (MFMA).  NJ must
 * be a multiple of 8.  The reduction is split over workgroups in fixed chunks; with more than one split the partial tiles go to ws
 * (eg_linear_dinput_ws_floats(B, NI, NJ, K) floats, 0 = not needed, ws may be NULL) and are added in split order by a second launch of
 * the same call: no atomics, every element of dX is stored, nothing needs zeroing, bitwise reproducible.
 *   CelebA   conv_blocks.0.weight [cin][1024][4][4], dh0 NHWC (n' = t*1024 + co):  NI, NJ = 16, 1024;  s_i, s_j, s_k = 1, 16, 16384
 *   MNIST    l1.0.weight [8192][cin], dh (n' = hw*128 + c, row f = c*64 + hw):     NI, NJ = 64, 128;   s_i, s_j, s_k = cin, 64*cin, 1
 *   dSprites fc1.0.weight [128][cin], dz1:                                         NI, NJ = 1, 128;    s_i, s_j, s_k = 0, cin, 1 */
size_t eg_linear_dinput_ws_floats(int B, int NI, int NJ, int K);
int eg_linear_dinput(int dtype, const void* dH, long long ldh, const float* W, float* dX, int B, int NI, int NJ, int K, long long s_i,
                     long long s_j, long long s_k, float* ws, size_t ws_floats, eg_stream_t s);

/* wp[n][k] = w[(n / n_div) * s_hi + (n % n_div) * s_lo + (k / k_div) * s_khi + (k % k_div) * s_klo]  (row AND column permuted) */
int eg_pack_strided2(int dtype, const float* w, void* wp, int N, int K, int Kpad, int n_div, long long s_hi, long long s_lo,
                     int k_div, long long s_khi, long long s_klo, eg_stream_t s);

/* --- image-side (1..4 channel, NCHW fp32) convolution and its weight gradient ---------------------
 * first Discriminator/Encoder conv (celebA/EAD-GAN_celebA.py:110, dSprites/rp.py:95, MNIST/EAD-GAN_rpqmnxy.py:107)
 * and input gradient / weight gradient of the Generator's last ConvTranspose2d (celebA/EAD-GAN_celebA.py:90) */
int eg_conv_img_fwd(int dtype, const float* img, const float* w_master, void* out, int B, int CI, int H, int W,
                    int N, int k, int stride, int pad, const eg_epilogue* ep, eg_stream_t s);
size_t eg_conv_img_wgrad_ws_bytes(int B, int CI, int N, int k);
int eg_conv_img_wgrad(int dtype, const void* dz, const float* img, float* slab, int B, int CI, int H, int W,
                      int N, int k, int stride, int pad, eg_stream_t s);
/* patch rows [B*OH*OW][Kp] (dtype T, K = CI*k*k in master weight order, zero padded to Kp): lets the image-side layers
 * run on the MFMA kernels as 1x1 convolutions over Kp channels */
int eg_im2col_img(int dtype, const float* img, void* out, int B, int CI, int H, int W, int k, int stride, int pad, int Kp,
                  eg_stream_t s);
/* the same convolution WITHOUT patch rows in HBM, 16-bit types: Conv2d(C <= 4 -> 128, 4, 2, 1) of up to three fp32 NCHW image tensors
 * ("tapes": independent forwards batched into one launch, each with its own spectral-norm sigma -- ep->sigma[tape]) straight on the MFMA
 * units; out [ntapes*B][H/2][W/2][128] dtype T.  wp: the [128][64] panel of eg_pack_strided (K order = master weight order).  gate_t != NULL:
 * the convolution's input is img_t * act'(gate_t) (the input gradient of the Generator's last ConvTranspose2d + Tanh, celebA.py:90-91: img =
 * d(loss)/d(image), gate = the image).  ep: bias, sigma, act / slope only.  Bit-identical to eg_im2col_img + eg_conv_fwd on the patch rows. */
int eg_conv_img_mfma_ok(int dtype, int C, int H, int W, int N, int k, int stride, int pad);
/* ep->stat_mode == EG_STAT_BN_BWD is honoured too (the output feeds a BatchNorm backward: dy stored, the two sums per tile of 64 pixels
 * to ep->stat_out[(which * 128 + n) * nrb + tile]); nrb = eg_conv_img_mfma_stat_blocks() */
int eg_conv_img_mfma_stat_blocks(int B, int H, int W, int ntapes);
/* N = 32, 64 or 128 output channels (wp: the [N][64] panel; out [ntapes*B][H/2][W/2][N]): 32 is the first trunk layer of the dSprites
 * networks, Conv2d(C -> 32, 4, 2, 1) (dSprites/rp.py:95-97, 165-167; rp_color.py likewise).  EG_STAT_BN_BWD: N = 128 only. */
int eg_conv_img_mfma(int dtype, const float* img0, const float* img1, const float* img2, const float* gate0, const float* gate1,
                     const float* gate2, int ntapes, const void* wp, void* out, int B, int C, int H, int W, int N, const eg_epilogue* ep,
                     int gate_act, float gate_slope, eg_stream_t s);
/* weight gradient of the image-side 4x4 / stride-2 / pad-1 layers of the dSprites networks WITHOUT patch rows in HBM (16-bit types, 64 x 64
 * images, C <= 4): S[n][c*16 + ky*4 + kx] = sum over output pixels of P[pixel][n] * img[b][c][2 oy - 1 + ky][2 ox - 1 + kx] for up to three
 * tapes (img_t fp32 NCHW; P [ntapes*B*1024][N] dtype T, tape-major rows) -- Conv2d(C -> 32, 4, 2, 1) of the trunks (dSprites/rp.py:95-97,
 * 165-167; N = 32, P = d(loss)/d(pre-activation)) and ConvTranspose2d(64 -> C, 4, 2, 1) of the generator (:139-140; N = 64, img = the image
 * gradient, P = the layer's input).  Writes *nsplit_out = eg_wgrad_img_splits(ntapes * B, N) slabs [N][16 C] (the per-tap kernel's layout over
 * patch rows: finish with eg_wgrad_reduce / _rank1 / _perm as after eg_im2col_img + eg_conv_wgrad, which this replaces). */
int eg_wgrad_img_ok(int dtype, int C, int H, int W, int N, int k, int stride, int pad);
int eg_wgrad_img_splits(int images, int N);          /* N = 32 / 64, and 128: the first Discriminator layer of the CelebA script (celebA/EAD-GAN_celebA.py:110) */
int eg_wgrad_img(int dtype, const float* img0, const float* img1, const float* img2, int ntapes, const void* P, float* slab, int B, int C,
                 int H, int W, int N, int* nsplit_out, eg_stream_t s);
/* The same sum for the CelebA layers (N = 128: Conv2d(C -> 128, 4, 2, 1), celebA/EAD-GAN_celebA.py:110, and ConvTranspose2d(128 -> C, 4, 2, 1),
 * :90-91, in conv view) as a streaming kernel whose slabs are BIT-IDENTICAL to eg_im2col_img (Kp = 16 C) + eg_conv_wgrad over the patch rows:
 * one workgroup per K split of the per-tap kernel's plan for those rows, P staged by LDS-DMA, the patch values picked from the staged image
 * rows; no patch rows in HBM.  wgs_target: 0 = the plan eg_conv_wgrad uses for the patch rows (its per-tap launches take no target), > 0 =
 * that many splits, down to one 32-row step each.  eg_wgrad_img_tn_plan returns the split count for `images` = ntapes * B images and
 * stores the rows per split; the slab holds nsplit * 128 * 16 C floats. */
int eg_wgrad_img_tn_ok(int dtype, int C, int H, int W, int N, int k, int stride, int pad);
int eg_wgrad_img_tn_plan(int images, int C, int wgs_target, int* rows_per_split);
int eg_wgrad_img_tn(int dtype, const float* img0, const float* img1, const float* img2, int ntapes, const void* P, float* slab, int B, int C,
                    int H, int W, int N, int wgs_target, int* nsplit_out, eg_stream_t s);
/* ConvTranspose2d(128 -> C <= 3, 4, 2, 1) from 16-bit NHWC activations a [B][Hin][Win][128] to an fp32 NCHW image [B][C][2 Hin][2 Win] in ONE
 * launch (the GEMM's columns stay in LDS): out = act(bias + transposed convolution); wp = the [16 * C][128] panel (row t * C + c) of
 * eg_pack_strided.  The Generator's last layer + Tanh (celebA.py:90-91) and the backward-to-image of the first Discriminator layer (:110).
 * Bit-identical to eg_conv_fwd (N = 16 C columns) + eg_col2im_img. */
int eg_convt_img_mfma_ok(int dtype, int C, int Hin, int Win, int K, int k, int stride, int pad);
/* K = 64 or 128 input channels (a [B][Hin][Win][K], wp [16 * C][K]): 64 is the dSprites generators' last layer ConvTranspose2d(64 -> C, 4, 2, 1) +
 * Sigmoid (dSprites/rp.py:139-141) */
int eg_convt_img_mfma(int dtype, const void* a, const void* wp, const float* bias, float* out, int B, int C, int Hin, int Win, int K, int act,
                      float slope, eg_stream_t s);
int eg_cast_pad(int dtype, const float* src, void* dst, int rows, int n, int npad, eg_stream_t s);
/* col2im of a transposed convolution with C = 1 or 3 output channels (ConvTranspose2d(128 -> 3, 4, 2, 1): celebA/EAD-GAN_celebA.py:90-91; the
 * backward-to-image of Conv2d(3 -> 128, 4, 2, 1): :110).  cols [B*Hin*Win][k*k*C] (dtype T; column t*C + c, t = kh*k + kw) is the output of
 * ONE GEMM over the input pixels (eg_conv_fwd on a 1x1 geometry with Cout = k*k*C), so every activation is read once:
 *   out[b][c][oy][ox] = act(bias[c] + sum of cols[(b,iy,ix)][t*C + c] over the taps with oy = iy*stride - pad + kh, ox = ix*stride - pad + kw)
 * out: fp32 NCHW [B][C][(Hin-1)*stride - 2*pad + k][(Win-1)*stride - 2*pad + k]; bias may be NULL. */
int eg_col2im_img(int dtype, const void* cols, int B, int C, int Hin, int Win, int k, int stride, int pad, const float* bias, int act,
                  float slope, float* out, eg_stream_t s);
/* out = g * act'(a) over an NCHW fp32 tensor and gb[c] (+)= sum_{b,hw} out  (partial: B*C floats) */
int eg_act_grad_mul_bias_nchw(const float* g, const float* a, float* out, int B, int C, int HW, int act, float slope,
                              float* partial, float* gb, int accumulate, eg_stream_t s);
int eg_flat_reduce(const float* slab, int nslab, size_t total, float* grad, int accumulate, eg_stream_t s);

/* --- small-N dense heads (celebA/EAD-GAN_celebA.py:122; MNIST/EAD-GAN_rpqmnxy.py:124,161-163; dSprites/rp.py:109-110,180-183)
 * y[b][n] = sum_k x[b][k] Wp[n][k] + bias[n];  x dtype T [B][K]; Wp dtype T [N][Kpad] (eg_pack_fwd order);  y fp32
 * ws (optional, ws_floats >= 16*B*N lets the planner go as far as it wants): scratch for splitting K over workgroups when B/4 row groups
 * do not fill the GPU; the slices are added in a fixed order by a second launch. */
int eg_dense_small_fwd(int dtype, const void* x, const void* wp, const float* bias, float* y, int B, int K,
                       int Kpad, int N, float* ws, size_t ws_floats, eg_stream_t s);
/* spectrally normalised variant: y = (x Wp^T) / sigma[b / sigma_rows] + bias */
int eg_dense_small_fwd_sn(int dtype, const void* x, const void* wp, const float* bias, float* y, int B, int K,
                          int Kpad, int N, const float* sigma, int sigma_rows, float* ws, size_t ws_floats, eg_stream_t s);
/* gradient prep of a dense head: dys = dy / sigma[tape] (sigma == NULL: plain head) written as dtype T at column col0 of a
 * [rows][npad] buffer and, if dys32 != NULL, as fp32 at column col0 of a [rows][ld32] buffer; gb[n] += sum_rows dy;
 * coef[tape] = sum dys * (y - bias)  (== <G_t,W>/sigma_t^2, the spectral-norm rank-1 coefficient) */
int eg_head_prep_sn(int dtype, const float* dy, int ldy, const float* y, int ldyy, const float* bias, int rows, int N,
                    const float* sigma, int rows_per_tape, void* dys, int npad, int col0, float* gb, float* coef,
                    float* dys32, int ld32, eg_stream_t s);
/* Several weight packs in ONE launch (the small networks re-pack 7-12 panels per optimizer update, each a launch of a few workgroups on
 * a launch-bound chain).  Between eg_pack_record_begin() and eg_pack_record_end() the calling thread's eg_pack_fwd / eg_pack_bwd /
 * eg_pack_conv / eg_pack_strided / eg_pack_strided2 calls launch nothing and are recorded as jobs; _end copies the jobs (eg_pack_job_bytes()
 * bytes each) to host memory jobs_out and returns their count and the joint launch's workgroup count; eg_pack_multi runs a DEVICE copy of the
 * job table: the same panel bytes as the recorded calls launched one by one. */
int eg_pack_record_begin(void);
size_t eg_pack_job_bytes(void);
int eg_pack_record_end(void* jobs_out, size_t cap_bytes, int* njobs, int* nblocks);
int eg_pack_multi(const void* jobs_dev, int njobs, int nblocks, eg_stream_t s);
/* the K-slice sums of eg_dense_small_fwd without the combine launch: partials[slice][b][n] (ws_floats >= 16 * B * N), *nslice_out slices;
 * eg_head_fused adds them (slice order, + bias) */
int eg_dense_small_fwd_slices(int dtype, const void* x, const void* wp, int B, int K, int Kpad, int N, float* partials, size_t ws_floats,
                              int* nslice_out, eg_stream_t s);
/* dx[b] = (dy[b] Wp) * act'(mask[b]) [/ sigma[b / sigma_rows]] */
int eg_dense_small_bwd(int dtype, const float* dy, const void* wp, const void* mask, void* dx, int B, int K,
                       int Kpad, int N, int mask_act, float mask_slope, const float* sigma, int sigma_rows,
                       eg_stream_t s);
int eg_dense_small_wgrad(int dtype, const float* dy, const void* x, float* gw, float* gb, int B, int K, int N,
                         int Cin, int taps, eg_stream_t s);
int eg_dense_small_bgrad(const float* dy, float* gb, int B, int N, int accumulate, eg_stream_t s);   /* gb[n] (+)= sum_b dy[b][n] */

/* --- BatchNorm2d, training mode (celebA/EAD-GAN_celebA.py:79,83,87; MNIST/EAD-GAN_rpqmnxy.py:80,83,87,145) ----
 * x,y: [M][C] dtype T; updates running stats (momentum, unbiased var: M2 / (M - 1), M2 / M for M = 1) and num_batches_tracked; fused
 * activation.
 * Argument contract of EVERY eg_bn_* entry point below (checked before anything is computed from C or launched; a call that breaks it
 * returns a negative value and leaves its reason, with the entry point's name, in eg_last_error()):
 *   - dtype is EG_F32, EG_BF16 or EG_F16;
 *   - M > 0 (M_local > 0 for the data-parallel pair, which also needs M_global >= M_local, and nranks > 0 in the forward);
 *   - C > 0 and C % 4 == 0 in fp32, C % 8 == 0 in the 16-bit types (rows are walked in 16-byte vectors);
 *   - act is EG_ACT_NONE, EG_ACT_RELU or EG_ACT_LRELU, in the forwards too: the backwards have no derivative for another one;
 *   - post_act of eg_bn_bwd_post is any EG_ACT_* code and nothing else;
 *   - the fused pair needs nrb > 0, the forward also nrb * rows_per_block == M;
 *   - pointers are non-null except where a comment says otherwise: running_mean, running_var and num_batches_tracked of the training
 *     forwards, dgamma and dbeta of the backwards and post_sigma may each be NULL (that output is skipped; post_sigma: no division).
 * y is formed as x * A[c] + B[c] from the two fp32 coefficients A = gamma * invstd, B = beta - mean * A, and the backwards decide act'(y)
 * on that very expression; dz = A * dy - Bz * z - Cc with Bz = A * invstd * sum(dy * xhat) / M and
 * Cc = A * (sum(dy) / M - mean * invstd * sum(dy * xhat) / M). */
size_t eg_bn_ws_floats(int M, int C);
int eg_bn_fwd_train(int dtype, const void* x, void* y, int M, int C, const float* gamma, const float* beta, float eps,
                    float momentum, float* running_mean, float* running_var, long long* num_batches_tracked,
                    float* save_mean, float* save_invstd, float* ws, int act, float slope, eg_stream_t s);
/* the same with the batch statistics taken from the producing convolution's epilogue (eg_epilogue.stat_mode = EG_STAT_MOMENTS):
 * stat = its stat_out, nrb row blocks of rows_per_block rows each.  Two launches (statistics + running stats, apply) instead of three,
 * and x is read once instead of twice.  ws: 2*C floats. */
int eg_bn_fwd_train_fused(int dtype, const void* x, void* y, int M, int C, const float* stat, int nrb, int rows_per_block,
                          const float* gamma, const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                          long long* num_batches_tracked, float* save_mean, float* save_invstd, float* ws, int act, float slope,
                          eg_stream_t s);
/* backward with the two sums taken from the epilogue of the convolution that produced dy (EG_STAT_BN_BWD: dy already carries the
 * activation gradient): dz = gamma * invstd * (dy - sum(dy)/M - xhat * sum(dy*xhat)/M); dgamma / dbeta (+)= their sums.  ws: 5*C floats. */
int eg_bn_bwd_fused(int dtype, const void* z, const void* dy, void* dz, int M, int C, const float* stat, int nrb,
                    const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta,
                    float* sums, float* ws, int accumulate, eg_stream_t s);
/* synchronised BatchNorm for data parallel runs (statistics over the global batch: N ranks x B/N images == 1 rank x B images).
 * Forward: eg_bn_stats_local writes this rank's (count, mean, M2) per channel to stats[3*C]; the host gathers every rank's block
 * (stats_all[nranks][3*C]); eg_bn_fwd_from_stats combines them (Chan, fp64), updates the running statistics with the GLOBAL
 * batch (M_global rows) and normalises the local rows.  Backward: eg_bn_bwd_sums_local writes the local sum(dy), sum(dy*xhat)
 * to sums[2*C] and dbeta / dgamma (+)= them (parameter gradients stay local; the gradient all-reduce averages them); the host
 * all-reduces sums; eg_bn_bwd_from_sums produces dz of the local rows.  ws: eg_bn_ws_floats(M, C) floats. */
int eg_bn_stats_local(int dtype, const void* x, int M, int C, float* ws, float* stats, eg_stream_t s);
int eg_bn_fwd_from_stats(int dtype, const void* x, void* y, int M_local, int C, const float* stats_all, int nranks, int M_global,
                         const float* gamma, const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                         long long* num_batches_tracked, float* save_mean, float* save_invstd, float* ws, int act, float slope,
                         eg_stream_t s);
int eg_bn_bwd_sums_local(int dtype, const void* z, const void* da, int M, int C, const float* gamma, const float* beta,
                         const float* save_mean, const float* save_invstd, int act, float slope, float* dgamma, float* dbeta,
                         float* sums, float* ws, int accumulate, eg_stream_t s);
int eg_bn_bwd_from_sums(int dtype, const void* z, const void* da, void* dz, int M_local, int C, const float* sums_global, int M_global,
                        const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, int act, float slope,
                        float* ws, eg_stream_t s);
/* eval mode (module.eval(): generate_image.py:146-154, gen_imgs.py:106-120 of the reference): y = act((x - running_mean) /
 * sqrt(running_var + eps) * gamma + beta); nothing is updated; ws: 2*C floats */
int eg_bn_fwd_eval(int dtype, const void* x, void* y, int M, int C, const float* gamma, const float* beta, float eps,
                   const float* running_mean, const float* running_var, float* ws, int act, float slope, eg_stream_t s);
/* backward of eg_bn_fwd_eval with respect to its input (the statistics are constants, so the layer is elementwise and has no batch
 * coupling): dz = da * act'(y) * gamma / sqrt(running_var + eps), y recomputed in fp32 from z by the forward's own expression and
 * coefficients.  act: EG_ACT_NONE, EG_ACT_RELU or EG_ACT_LRELU.  No parameter gradients; ws: 2*C floats */
int eg_bn_bwd_eval(int dtype, const void* z, const void* da, void* dz, int M, int C, const float* gamma, const float* beta, float eps,
                   const float* running_mean, const float* running_var, float* ws, int act, float slope, eg_stream_t s);
/* dz from da (gradient w.r.t. the activation output); dgamma / dbeta (+)= their sums; sums: 2*C floats scratch */
int eg_bn_bwd(int dtype, const void* z, const void* da, void* dz, int M, int C, const float* gamma, const float* beta,
              const float* save_mean, const float* save_invstd, int act, float slope, float* dgamma, float* dbeta,
              float* sums, float* ws, int accumulate, eg_stream_t s);
/* as eg_bn_bwd, then dz *= act'(z as an activation OUTPUT) / post_sigma  -- for blocks ordered conv -> LeakyReLU -> BN
 * (MNIST/EAD-GAN_rpqmnxy.py:143-146): the BN input IS the LeakyReLU output, so its backward mask is fused here */
int eg_bn_bwd_post(int dtype, const void* z, const void* da, void* dz, int M, int C, const float* gamma, const float* beta,
                   const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta, float* sums, float* ws,
                   int post_act, float post_slope, const float* post_sigma, eg_stream_t s);

/* --- spectral norm power iteration (torch.nn.utils.spectral_norm, celebA/EAD-GAN_celebA.py:110-120) -------- */
size_t eg_sn_ws_floats(int R, int Kd);
int eg_sn_power_iter(const float* w_orig, int R, int Kd, float* u, float* v, float* sigma, float* u_snap,
                     float* v_snap, float* ws, int training, float eps, eg_stream_t s);

/* all spectrally-normalised layers of a network in one launch per stage (4 launches per forward instead of 4 per layer) */
typedef struct eg_sn_layer {
    const float* w;
    float* u;
    float* v;
    float* sigma;
    float* u_snap;
    float* v_snap;
    int R, Kd;
} eg_sn_layer;
size_t eg_sn_multi_ws_floats(const eg_sn_layer* layers, int nlayers);
int eg_sn_power_iter_multi(const eg_sn_layer* layers, int nlayers, float* ws, int training, float eps, eg_stream_t s);

/* --- Adam (torch.optim.Adam, celebA/EAD-GAN_celebA.py:211-217) over a flat fp32 arena ----------------------- */
/* tick: step[0] += 1 before the update (the bias correction reads the counter after the tick).  n == 0 (an empty slice) is valid for
 * both entry points: with `tick` the counter still advances, no element kernel is launched, the call returns 0. */
int eg_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps,
                 int* step, int tick, eg_stream_t s);
/* the same update on a slice of the arena (one gradient bucket); zero_grad: the gradient slice is cleared in the same pass
 * (optimizer.step() + optimizer.zero_grad(), celebA/EAD-GAN_celebA.py:344-345,365-366,400-401) */
int eg_adam_step_zero(float* p, float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps,
                      int* step, int tick, int zero_grad, eg_stream_t s);
/* optimizer.step() on ONE convolution weight (conv view master [Cout][Cin][k][k]) fused with the refresh of its packed panels: the update
 * of eg_adam_step_zero (same bits) applied on the way through the tile transpose of eg_pack_conv (same panel bytes); p / g / m / v are
 * the parameter's slices of the four arenas; `step` is the optimizer's device step counter, already ticked (eg_adam_tick).  Only layers
 * eg_adam_pack_conv_ok() accepts (Cout a multiple of 16, Cin of 32, at most 16 taps, stride <= 2 with a backward panel; where a panel's K
 * is no multiple of the K block its padding columns are written as zeros, as eg_pack_conv writes them); either panel may be NULL. */
int eg_adam_pack_conv_ok(const eg_conv* c, int dtype, int has_fwd, int has_bwd);
int eg_adam_pack_conv(const eg_conv* c, int dtype, float* p, float* g, float* m, float* v, float lr, float b1, float b2, float eps,
                      const int* step, void* wp_fwd, void* wp_bwd, eg_stream_t s);
/* the same for a weight whose panel is a row-permuted transpose of the master: master p[K][N] (N contiguous; the ConvTranspose2d on a
 * 1x1 input, celebA/EAD-GAN_celebA.py:76), panel wp[n'][Kpad], n' = (n % n_mod) * n_mul + n / n_mod, columns k < K (the padding keeps
 * the zeros eg_pack_strided wrote once) */
int eg_adam_pack_rows(int dtype, float* p, float* g, float* m, float* v, void* wp, int K, int N, int Kpad, int n_mod, int n_mul,
                      float lr, float b1, float b2, float eps, const int* step, eg_stream_t s);
int eg_adam_tick(int* step, eg_stream_t s);            /* step[0] += 1 (once per optimizer.step(), before its slice-wise updates) */
int eg_fill_f32(float* p, size_t n, float val, eg_stream_t s);

/* --- utility: generator input concat+cast ---------------------------------------------------------------- */
int eg_concat_cast(int dtype, const float* a, int wa, const float* b, int wb, const float* c, int wc, int B,
                   int Cpad, void* out, eg_stream_t s);

/* --- affine codes, warp and loss heads ---------------------------------------------------------------------
 * eg_theta_rpqxy : celebA/utils_rpqxy.py:59-80 (rows 0,1 of R*Z*T) ;  eg_warp_affine : transformation_2D,
 * celebA/EAD-GAN_celebA.py:146-152 ;  losses : celebA/EAD-GAN_celebA.py:161-169,342,355-362,383-395 */
int eg_theta_rpqxy(const float* code, int ldc, int B, float* theta, eg_stream_t s);
int eg_warp_affine(const float* img, const float* theta, float* out, int B, int C, int H, int W, eg_stream_t s);
/* eg_theta_rpqxy + eg_warp_affine in one launch (same arithmetic; H * W a multiple of 256); theta_out optional; zero / zero_n: floats the
 * launch clears first (the iteration's loss accumulators) */
int eg_warp_affine_rpqxy(const float* img, const float* code, int ldc, float* theta_out, float* out, int B, int C, int H, int W,
                         float* zero, int zero_n, eg_stream_t s);
int eg_loss_bce_sigmoid(const float* o, int ld, int col, int B, float target, float scale, float* loss, float* dout,
                        int zero_rows, eg_stream_t s);
int eg_loss_mse(const float* o, int ld, int col0, int n, int B, const float* tgt, int ldt, float tconst, float scale,
                float* loss, float* dout, int zero_rows, eg_stream_t s);
int eg_loss_ce_softmaxed(const float* o, int ld, int c0, int n, int B, const long long* labels, float scale,
                         float* loss, float* dout, eg_stream_t s);
/* MNIST variant, 7 codes (theta,p,q,m,n,x,y): MNIST/utils_rpqmnxy.py:46-134.  eg_theta_rpqmnxy = rows 0,1 of R Z S T.
 * eg_loss_affine_rpqmnxy: MSE(latent(MLP(flat(rel))), code) * scale with the frozen 6-256-256-256-256-7 LeakyReLU(0.01)
 * approximator; mlp = eg_mlp_rpqmnxy_floats() floats: W1[256][6] b1 W2[256][256] b2 W3 b3 W4 b4 W5[7][256] b5, then the
 * transposes W2t W3t W4t ([in][out]) for the forward sweep. */
size_t eg_mlp_rpqmnxy_floats(void);
int eg_theta_rpqmnxy(const float* code, int ldc, int B, float* theta, eg_stream_t s);
int eg_loss_affine_rpqmnxy(const float* o_real, const float* o_trans, int ld, int c0, int B, const float* code, int ldc,
                           const float* mlp, float scale, float* loss, float* d_real, float* d_trans, float* pred_out,
                           float* ws /* B floats */, eg_stream_t s);
/* dSprites variants (dSprites/utils_rp.py:38-59,94-147, utils_pxy.py:69-87, rp.py:225-232,375-377) */
int eg_theta_rp(const float* code, int ldc, int B, float* theta, eg_stream_t s);                 /* rows 0,1 of R Z(p,p) T */
int eg_theta_pxy_align_inv(const float* code, int ldc, int B, float* theta, eg_stream_t s);      /* rows 0,1 of inverse(T(x,y)) */
int eg_loss_affine_rp(const float* o_real, const float* o_trans, int ld, int c0, int B, const float* code, int ldc, float scale,
                      float* loss, float* d_real, float* d_trans, float* pred_out, eg_stream_t s);
int eg_loss_mutual_info(const float* o, int ld, int c0, int n, int B, const float* tgt, int ldt, int t0, int target_logits,
                        float scale, float* loss, float* dout, eg_stream_t s);
/* colored dSprites (colored_dSprites/rp_color.py:368-394,415-424; utils_rp_color.py:38-75,100-139) */
int eg_u8_colorize(const unsigned char* sprites, const float* gain, float* out, int B, int C, int HW, eg_stream_t s);
int eg_color_scale(const float* in, const float* code, int ldc, int c0, float factor, int divide, float* out, int B, int C, int HW,
                   eg_stream_t s);
int eg_loss_affine_rp_color(const float* o_real, const float* o_trans, int ld, int c0, int B, const float* code, int ldc, float scale,
                            float* loss, float* d_real, float* d_trans, float* pred_out, eg_stream_t s);
int eg_add_f32(float* out, const float* a, const float* b, size_t n, eg_stream_t s);
int eg_u8_to_f32(const unsigned char* x, float* y, size_t n, eg_stream_t s);            /* uint8 sprites -> float (rp.py:369-370) */
int eg_loss_affine_rpqxy(const float* o_real, const float* o_trans, int ld, int c0, int B, const float* code, int ldc,
                         float scale, float* loss, float* d_real, float* d_trans, float* pred_out, eg_stream_t s);
/* the info step's three losses in one launch (celebA.py:390-396): lcon * MSE(o_gen[:, c_cont : c_cont+n_cont], code) + lcat *
 * CE(softmax(o_gen[:, c_cont+n_cont : +n_cat]), labels) into d_gen (rows zeroed first), laff * MSE(affine_regularzier(o_real, o_trans),
 * code[:, :5]) into d_real / d_trans; all three add to loss[0] in that order -- the same numbers as eg_loss_mse, eg_loss_ce_softmaxed and
 * eg_loss_affine_rpqxy launched one after the other */
int eg_loss_info_rpqxy(const float* o_gen, const float* o_trans, const float* o_real, int ld, int c_cont, int n_cont, int n_cat, int B,
                       const float* code, int ldc, const long long* labels, float lcat, float lcon, float laff, float* loss, float* d_gen,
                       float* d_trans, float* d_real, eg_stream_t s);

/* The tail of the discriminator's head in ONE launch behind eg_dense_small_fwd_slices (celebA.py:110-122 the 4x4 head convolution as a
 * dense layer; :334-345, :353-366 the adversarial BCE terms; :375-401 the info step's three losses): the workgroups of sample index b work
 * on the T rows t*B + b (the tapes of that sample):
 *   y[t*B+b][n]  = sum_slices partials[slice][t*B+b][n] + bias[n]                               (= the slice combine of eg_dense_small_fwd)
 *   dout rows    = d(loss)/d(y) of the rows, other columns zero                                 (= eg_loss_bce_sigmoid / eg_loss_info_rpqxy)
 *   dx[t*B+b][k] = (sum_n dout[t*B+b][n] * wp[n][k]) * act'(x[t*B+b][k]) / sigma[t]              (= eg_dense_small_bwd with mask = x)
 * and the last workgroup to finish adds the batch's loss terms to loss[0] in the order of the stand-alone loss kernels: the same bits as
 * the four launches it replaces (combine, loss, dense backward; the loss sums for B <= 256, affine term B <= 128 -- beyond, the same
 * terms added in another order).  mode 0: tape t carries BCE(sigmoid(y[:, 0]), target[t]) * scale[t] (T <= 3).  mode 1 (T = 3, tapes:
 * generated, transformed, real): lcon * MSE(y_gen[:, c_cont : +n_cont], code) + lcat * CE(softmax(y_gen[:, c_cont+n_cont : +n_cat]),
 * labels) + laff * MSE(affine_regularzier(y_real, y_trans), code[:, :5]).  terms: >= 3*B floats of scratch, counter: one zeroed unsigned
 * (left zero).  Supported heads: N = 19 (CelebA), K a multiple of 8 elements (4 for fp32). */
typedef struct eg_head {
    const void* x;
    const void* wp;
    const float* bias;
    const float* partials;
    int nslice;
    float* y;
    float* dout;
    void* dx;
    const float* sigma;
    int B, T, K, Kpad, N, mode;
    float target[3], scale[3];
    int c_cont, n_cont, n_cat;
    const float* code;
    int ldc;
    const long long* labels;
    float lcat, lcon, laff;
    float* loss;
    float* terms;
    unsigned int* counter;
    int mask_act;
    float mask_slope;
} eg_head;
int eg_head_fused(int dtype, const eg_head* h, eg_stream_t s);
int eg_head_fused_ok(int dtype, int T, int K, int N);

/* regression target of the approximator fit (MNIST/approximate_rpqmnxy.py:43-60,119-136): affine parameters of a code */
int eg_affine_para_rpqmnxy(const float* code, int ldc, int B, float* para, eg_stream_t s);

/* stage-1 trainer of Encoder_pxy (dSprites/pxy.py:156-191, dSprites/utils_pxy.py:24-66,107-126): theta = rows 0,1 of
 * get_matrix_pxy(code); affine_regularzier_pxy + MSE with fused gradients w.r.t. both codes */
int eg_theta_pxy(const float* code, int ldc, int B, float* theta, eg_stream_t s);
/* ncol = 3: three colour-gain entries follow (p, x, y) (colored_dSprites/utils_pxy.py:150-176, pxy_color.py:185-213) */
int eg_loss_affine_pxy(const float* o_real, const float* o_trans, int ld, int c0, int B, const float* code, int ldc, int ncol, float scale,
                       float* loss, float* d_real, float* d_trans, float* pred_out, eg_stream_t s);
/* transformation_2D with grid_sample(padding_mode='zeros') (colored_dSprites/pxy_color.py:86-92) */
int eg_warp_affine_zeros(const float* img, const float* theta, float* out, int B, int C, int H, int W, eg_stream_t s);
/* backward of eg_warp_affine (zeros = 0, 'border') / eg_warp_affine_zeros (zeros = 1): dimg [B,C,H,W] and dtheta [B,6]; either may be
 * null.  Every element of a non-null output is WRITTEN (no pre-zeroed buffer needed, nothing is accumulated into it).  grid_sample's
 * derivative rules: 'border' has no coordinate gradient where the unclamped coordinate is <= 0 or >= size - 1, 'zeros' counts inside
 * taps only.  dtheta is bitwise reproducible (fixed-order sums); dimg is summed by LDS float adds in arrival order and is not (nor is
 * torch's).  One image plane is kept in LDS: H * W <= 16384. */
int eg_warp_affine_bwd(const float* img, const float* theta, const float* dout, float* dimg, float* dtheta,
                       int B, int C, int H, int W, int zeros, eg_stream_t s);
/* dcode = J^T dtheta for the code -> theta maps; kind: 0 rpqxy (5 codes), 1 rpqmnxy (7), 2 rp (4), 3 pxy (3), 4 pxy_align_inv (3).
 * dcode [B][ldc]: the kind's columns get the gradient, every other column of the row is written 0 (as d_real / d_trans are). */
int eg_theta_bwd(int kind, const float* code, int ldc, int B, const float* dtheta, float* dcode, eg_stream_t s);

/* --- image grids of the sampling tools: torchvision.utils.make_grid / save_image (0.8.2, not vendored) as the reference
 * calls them -- MNIST/EAD-GAN_rpqmnxy.py:281-330, MNIST/generate_image.py:122-138, celebA/EAD-GAN_celebA.py:238-287,
 * celebA/gen_imgs.py:183-199, dSprites/rp.py:299-353, colored_dSprites/rp_color.py:297-353.
 * eg_make_grid : img [B,C,H,W] fp32 -> grid [Cg][ymaps*(H+padding)+padding][xmaps*(W+padding)+padding] fp32, xmaps = min(nrow,B),
 *   ymaps = ceil(B/xmaps), Cg = 3 when C == 1 (replicated) else C; gaps and unused cells = pad_value.  range != NULL ({lo, hi} on the
 *   device, e.g. from eg_minmax_f32): image pixels are normalised like eg_quantize_u8 does while tiling (make_grid(normalize=True)).
 * eg_minmax_f32: out2 = {min, max} of x[0..n) (the normalize=True range); ws: eg_minmax_ws_floats() floats.
 * eg_quantize_u8: x [C][H][W] fp32 -> out [H][W][C] uint8 = clamp(v' * 255 + 0.5, 0, 255) truncated, v' = v or, with range = {lo, hi}
 *   on the device, (clamp(v, lo, hi) - lo) / (hi - lo + 1e-5).  Every step separately rounded: bytes equal the CPU restatement's. */
int eg_make_grid(const float* img, int B, int C, int H, int W, int nrow, int padding, float pad_value, const float* range,
                 float* grid, eg_stream_t s);
size_t eg_minmax_ws_floats(void);
int eg_minmax_f32(const float* x, size_t n, float* ws, float* out2, eg_stream_t s);
int eg_quantize_u8(const float* x, int C, int H, int W, const float* range, unsigned char* out, eg_stream_t s);

/* --- device-side input pipeline: replaces the per-iteration host work of the reference loops -- DataLoader + PIL
 * RandomHorizontalFlip / ToTensor / Normalize (celebA/EAD-GAN_celebA.py:194-206, MNIST/EAD-GAN_rpqmnxy.py:235-246) and the numpy draws
 * of z / code / labels (:308-317; :351-357) -- so that a captured hipGraph feeds itself.  Philox4x32-10, counter = (element, *step,
 * stream_id), key = seed: reproducible per (seed, step), same distributions as the reference, NOT numpy's stream.
 * kind 0: uniform [a,b) fp32; 1: normal(a, b) fp32; 2: integers in [a,b) as int64; 3: Bernoulli(a) as uint8;
 * 4: epoch permutation (DataLoader(shuffle=True), celebA.py:204-206): int64 dataset indices in [0, N = a) for the stream positions
 *    *step * total + elem0 + i -- a keyed bijection per epoch (position / N), every index exactly once per epoch, nothing stored;
 *    N <= 2^24
 * Sharded draws (data parallel): the call writes the n LOCAL elements [elem0, elem0 + n) of a global draw of `total` elements
 * (elem0 + n <= total is required).  Kinds 0-3: local element i is element g = elem0 + i of that draw -- lane g % 4 of the Philox block
 * with counter (g / 4 lo, g / 4 hi, *step, stream_id); for kind 1 the Box-Muller output of that lane, so a shard may begin or end inside a
 * pair or a quad.  Kind 4: the batch stride of the stream is the GLOBAL batch `total`, *step counts global iterations.  The ranks'
 * outputs, concatenated in rank order, are bit for bit the one call with elem0 = 0, total = n_global; elem0 = 0, total = n is the
 * unsharded draw.  out (and the fused one-hot rows) are indexed locally. */
int eg_rng_fill(int kind, void* out, size_t n, float a, float b, unsigned long long seed, const int* step, unsigned int stream_id,
                size_t elem0, size_t total, eg_stream_t s);
/* several draws in ONE launch (the same values as one eg_rng_fill per draw).  onehot != NULL (kind 2 only): row i of onehot[n][onehot_n] is
 * the one-hot code of draw i (to_categorical fused). */
typedef struct eg_rng_seg {
    int kind;
    void* out;
    size_t n;
    float a, b;
    unsigned int stream_id;
    float* onehot;
    int onehot_n;
    size_t elem0, total;            /* the shard [elem0, elem0 + n) of a global draw of `total` elements, as in eg_rng_fill */
} eg_rng_seg;
int eg_rng_fill_multi(const eg_rng_seg* segs, int nseg, unsigned long long seed, const int* step, eg_stream_t s);
int eg_counter_add(int* counter, int v, eg_stream_t s);
/* out[b] = data[idx[b]] (uint8 NCHW dataset in HBM), mirrored along x where flip[b], * scale + shift  -> fp32 NCHW */
int eg_gather_u8_images(const unsigned char* data, const long long* idx, const unsigned char* flip, float* out, int B, int C, int H,
                        int W, float scale, float shift, eg_stream_t s);
/* the same, and step_tick[0] += 1 afterwards (NULL: no tick): the iteration's draws -- earlier launches on the stream -- have read the counter */
int eg_gather_u8_images_tick(const unsigned char* data, const long long* idx, const unsigned char* flip, float* out, int B, int C, int H,
                             int W, float scale, float shift, int* step_tick, eg_stream_t s);
int eg_onehot(const long long* labels, float* out, int B, int n, eg_stream_t s);          /* to_categorical (celebA.py:59-64) */
/* transforms.Resize (PIL bilinear, antialiased) + CenterCrop of the uint8 dataset on its way into HBM (celebA.py:194-196): ONE separable
 * pass along y (axis 0) or x (axis 1) of `planes` planar uint8 images [in_h][in_w] with PIL's 8-bit fixed-point coefficient tables
 * (bounds[2*o] = first tap, bounds[2*o+1] = tap count, kk[o*ksize + t], 22 fractional bits; the host builds them as PIL does); produces
 * outputs o0 .. o0+on-1 along the axis and copies columns / rows c0 .. c0+cn-1 of the other axis: dst is [planes][on][cn] (axis 0) or
 * [planes][cn][on] (axis 1).  Horizontal pass first, then vertical, reproduces Image.resize(..., BILINEAR) bit for bit. */
int eg_resample_u8(const unsigned char* src, unsigned char* dst, int planes, int in_h, int in_w, int axis, const int* bounds,
                   const int* kk, int ksize, int o0, int on, int c0, int cn, eg_stream_t s);

/* Disentanglement scores of a trained encoder pair (dSprites/score/MIG.py, FactorVAE.py, BetVAE.py, SAP.py, F_score.py, DCI.py; colored_dSprites/score/ likewise).
 * Staging: out[b][c] = data[idx[b]] * gain[b][c] (uint8 [N][HW] sprites, gain [B][C] fp32 or NULL = 1) -> fp32 NCHW; the reference's
 * imgs[select_index] + add_color_2_img (colored MIG.py:169-184,204; FactorVAE.py:236-254,270,315). */
int eg_score_stage_u8(const unsigned char* data, const int* idx, const float* gain, float* out, int B, int C, int HW, eg_stream_t s);
/* out[b] = [argmax softmax(cat[b]) (first index on ties), cont[b][0], cont[b][1], pxy[b][1], pxy[b][2]] as float64 [B][5]: the
 * np.concatenate((cat, cont[:,0:2], align_code[:,1:3]), axis=1) row of MIG.py:233-243 / FactorVAE.py:263-266,300-303 */
int eg_score_rows(const float* cat, int ldcat, int ncat, const float* cont, int ldcont, const float* pxy, int ldpxy, int B, double* out,
                  eg_stream_t s);
/* make_discretizer(codes.T, nbins) (MIG.py:270-275): per column of codes [n][ncode] float64 np.digitize(x, np.histogram(x, nbins)[1][:-1])
 * with numpy's edge arithmetic -> bins [ncode][n] int32 in 1..nbins; lohi [ncode][2] (optional) receives the (widened) range */
int eg_score_digitize(const double* codes, int n, int ncode, int nbins, int* bins, double* lohi, eg_stream_t s);
/* discrete_mutual_info + discrete_entropy (MIG.py:278-294) with sklearn.metrics.mutual_info_score: mi[i*nf + j] = MI(ys[j], bins[i]),
 * mi[ncode*nf + j] = MI(ys[j], ys[j]).  ys [nf][n] int32 class ids in 0..kmax-1; bins [ncode][n] in 1..nbins.  ws: eg_score_mig_ws_ints ints */
size_t eg_score_mig_ws_ints(int ncode, int nf, int kmax, int nbins);
int eg_score_mig(const int* bins, int ncode, const int* ys, int nf, int n, int kmax, int nbins, int* ws, double* mi, eg_stream_t s);
/* np.std(x, axis=0) of x [n][ncol] float64, bit for bit (numpy's row-sequential axis-0 reduction) (FactorVAE.py:269) */
int eg_score_col_std(const double* x, int n, int ncol, double* out, eg_stream_t s);
/* FactorVAEMetric.evaluate's vote loop (FactorVAE.py:273-312): for group g (rows g*L.. of x [M*L][ncol]) predict[g] = argmin of
 * np.std(x_g / eval_std, axis=0) (numpy's rule: first NaN, else first minimum); votes [ncol][nlab] int64 (zeroed here) [predict][labels[g]] += 1 */
int eg_score_fvae_votes(const double* x, int L, int M, int ncol, const double* eval_std, const int* labels, int nlab, int* predict,
                        long long* votes, eg_stream_t s);
/* BetaVAEMetric.evaluate's features (BetVAE.py:256-257): for group g (rows g*L.. of x [M*L][ncol] float64)
 * feat[g] = np.mean(np.abs(x_g[0::2] - x_g[1::2]), axis=0), bit for bit (numpy's row-sequential axis-0 reduction).  L must be even. */
int eg_score_pair_absdiff_mean(const double* x, int L, int M, int ncol, double* feat, eg_stream_t s);
/* classifier.score's two parts (BetVAE.py:268) at the W [K][d+1] of eg_score_softmax_fit (K >= 3: one weight row per class):
 * predict[i] = np.argmax of the logits W [x_i, 1] (first index on ties), correct[0] = #{i: predict[i] == y[i]} (int64, zeroed here) */
int eg_score_logreg_accuracy(const double* X, const int* y, int n, int d, int K, const double* W, int* predict, long long* correct,
                             eg_stream_t s);
/* SAP (dSprites/score/SAP.py:283-309, colored :304-330).  R [k][nf] float64: R[i][j] = cov(i, j)^2 / var(i) / var(j) of code column i of
 * codes [n][k] and factor column j of fv [n][nf] (float64) as np.cov(x, y, ddof=1) gives them: the means first, then the centred sums.
 * One workgroup per (i, j), fixed summation order; a zero variance gives IEEE's NaN as the reference's division does.  n >= 2. */
int eg_score_sq_corr(const double* codes, int n, int k, const double* fv, int nf, double* R, eg_stream_t s);
/* classifier.fit of SAP.py:303-304 for P one-feature columns X [n][P] float64 that share the class ids y [n] int32 in 0..K-1: the optimum
 * of LinearSVC(C, class_weight="balanced") with sklearn's defaults (L2 penalty, squared hinge, one-vs-rest, the intercept a regularised
 * weight).  Problem (p, k) minimises  (w^2 + b^2) / 2 + sum_i c_i max(0, 1 - s_i (w x_ip + b))^2,  s_i = +1 where y_i = k and -1
 * elsewhere, c_i = C n / (K count_k) where y_i = k and C elsewhere -- strictly convex, one optimum.  One workgroup per (p, k): float64
 * generalised Newton from (0, 0) with the 2 x 2 Hessian solved in closed form and eg_score_softmax_fit's Armijo backtracking (1e-4,
 * halving, 40 trials, the n eps |f| slack); counts and weights come from y on the device; fixed summation order, two runs give the
 * same bits.  3 <= K <= 64, C > 0.  Stops when the gradient's inf-norm is <= gtol or after max_iter steps.  W [P][K][2] = (w, b); info [P][K][4] float64 = (iterations, final |g|inf,
 * objective, status: 0 converged, 1 max_iter reached, 2 line search failed, 4 a label outside 0..K-1 or a class without a sample (W = 0,
 * nothing computed), 5 non-finite).  No workspace. */
int eg_score_svc1_fit(const double* X, const int* y, int n, int P, int K, double C, int max_iter, double gtol, double* W, double* info,
                      eg_stream_t s);
/* classifier.predict of SAP.py:305-306 per column: predict [P][n] int32 = np.argmax_k (w_pk x_ip + b_pk) (first index on ties),
 * correct [P] int64 (zeroed here) = #{i: predict[p][i] == y[i]} */
int eg_score_svc1_accuracy(const double* X, const int* y, int n, int P, int K, const double* W, int* predict, long long* correct,
                           eg_stream_t s);
/* The logistic fit of the fitted scores: classifier.fit of F-stat's explicitness half (dSprites/score/F_score.py:327-338, colored
 * :345-356) and of the BetaVAE score (BetVAE.py:265-266).  The optimum of sklearn's LogisticRegression(C = 1 / inv_C) on X [n][d] float64
 * with class ids y [n] int32 in 0..K-1.  K >= 3: the multinomial objective
 * sum_i CE(softmax(W [x_i, 1]), y_i) + inv_C / 2 * |coefficients|^2  (sklearn's objective times n; intercepts unpenalised), W [K][d+1]
 * (coefficients | intercept) with zero-sum intercepts.  K = 2: the binomial form sklearn fits for two classes,
 * sum_i [log(1 + exp(z_i)) - y_i z_i] + inv_C / 2 |w|^2 with z_i = w . x_i + b, W [1][d+1] (not the two-class softmax: its penalty
 * differs).  2 <= K <= 64, K (d + 1) <= 256, inv_C > 0; everything else is refused.  Float64 damped Newton from W = 0: the Hessian (for
 * K >= 3 plus v v^T on the intercept block, v = 1 / sqrt(K), the one null direction; the mean of the step's intercepts, rounding only, is
 * taken out), Cholesky, and Armijo backtracking t = 1, 1/2, ... for 40 trials at most until
 * f(W + t s) <= f(W) + 1e-4 t g.s + n eps |f(W)|  (the last term is the rounding bound of the row sum).  Stops when the gradient's
 * inf-norm is <= gtol or after max_iter steps.  The row sums run over many workgroups, each a launch of its own in stream
 * order: probabilities and objective partials, Armijo's test, gradient partials per row slice of an accepted trial, the P x P Hessian
 * as per-slice partial slabs in ws and their reduction in ascending order; Cholesky and the triangular solves run on the Hessian in
 * global memory in one workgroup.  No workgroup waits on another, no float atomics: two calls give the same bits.
 * THE ONE BLOCKING ENTRY POINT OF THIS HEADER: the loop over Newton iterations and backtracking trials runs on the host inside the call.
 * Every decision (accept, backtrack, converged, failed) is taken on the device in float64 and written to a small record in ws; after
 * each trial the host copies that record back (a stream synchronisation) only to choose the next launch.  A stream that is capturing
 * is refused.  info [4] float64 = (iterations, final |g|inf, objective, status: 0 converged, 1 max_iter reached, 2 line search failed,
 * 3 Hessian not positive definite, 4 a label outside 0..K-1, 5 non-finite gradient (a non-finite input ends here), 6 a class without a
 * sample; 4 and 6 leave W = 0).  ws: eg_score_softmax_ws_bytes bytes. */
size_t eg_score_softmax_ws_bytes(int n, int d, int K);
int eg_score_softmax_fit(const double* X, const int* y, int n, int d, int K, double inv_C, int max_iter, double gtol, void* ws, double* W,
                         double* info, eg_stream_t s);
/* classifier.predict_proba at W (F_score.py:332): proba [n][K] float64 = softmax of the logits, or [1 - p, p] with p = sigmoid(z) for
 * K = 2 (W [1][d+1]).  The limits of eg_score_softmax_fit. */
int eg_score_softmax_proba(const double* X, int n, int d, int K, const double* W, double* proba, eg_stream_t s);
/* roc_auc_score's one-vs-rest pair counts (F_score.py:334-336), exact: for class k over all pairs (positive i: y_i = k, negative j:
 * y_j != k) of scores [n][K] float64, less[k] = #{s_jk < s_ik} and equal[k] = #{s_jk == s_ik} (uint64, zeroed here; integer atomics).
 * order [n] int32: the rows grouped by class; offsets [K+1] int32: class k's rows are order[offsets[k] .. offsets[k+1]); max_class_rows:
 * the largest offsets[k+1] - offsets[k], which sizes the grid (a smaller value would leave positives out).  The host forms
 * AUC_k = (2 less + equal) / (2 n_pos n_neg), the Mann-Whitney form of the trapezoid roc_auc_score integrates (ties count one half).
 * Positives sit in registers, negatives stream through LDS in tiles; no sort.  An order entry outside 0..n-1 is skipped, not read. */
int eg_score_auc_ovr(const double* scores, const int* order, const int* offsets, int n, int K, int max_class_rows,
                     unsigned long long* less, unsigned long long* equal, eg_stream_t s);

/* DCI with the script's default regressor, Lasso(alpha = 0.02) (dSprites/score/DCI.py:304-309,354-374; colored :323-328,381-401).
 * DCIMetric.normalize of codes [n][k] and fv [n][nf] (float64) as moments and one matrix: mean [k+nf], stddev [k+nf] (np.std: ddof = 0, two
 * passes) and G [(k+nf)][(k+nf)] = Z^T Z / n of the normalised columns Z = (X - mean) / stddev of [codes | fv], symmetric bit for bit; each
 * fit of the script depends on the data through G alone (G[:k][:k] its Gram matrix, G[:k][k+j] factor j's right-hand side).  The rows
 * are spread over up to 1024 workgroups (512 rows each at least); slice sums, then centred cross products per slice, then one
 * workgroup adds the slices in ascending order: no float atomics, two calls give the same bits.  n >= 2, k >= 1, nf >= 1, k + nf <= 32.
 * status [2] int32: [0] = 0, or bit 0: a column whose minimum equals its maximum (no variance; its mean is that value, its stddev 0),
 * bit 1: a column whose sum or centred square sum is not finite; [1] = the lowest such column, or -1.  A flagged column's entries of G
 * hold what IEEE's 0 / 0 gives; the status word is how the caller learns of it.  ws: eg_score_norm_gram_ws_bytes bytes. */
size_t eg_score_norm_gram_ws_bytes(int n, int k, int nf);
int eg_score_norm_gram(const double* codes, const double* fv, int n, int k, int nf, void* ws, double* mean, double* stddev, double* G,
                       int* status, eg_stream_t s);
/* regressor.fit of DCI.py:361-364 for every factor at once, on G [(k+nf)][(k+nf)] of eg_score_norm_gram: for factor j, with A = G[:k][:k],
 * c = G[:k][k+j], the optimum of  f(w) = (G[k+j][k+j] - 2 c.w + w.A w) / 2 + alpha |w|_1,  which is sklearn's Lasso objective
 * (1 / 2n) |y - X w - b|^2 + alpha |w|_1 on the normalised columns (their intercept b is zero); convex, one optimum when A is definite.
 * One wave per factor, w and g in registers: cyclic coordinate descent with soft thresholding from w = 0; before the first sweep and after each one the KKT
 * residual  max_i ( w_i != 0 ? |g_i - alpha sign(w_i)| : max(|g_i| - alpha, 0) ),  g = c - A w formed afresh, ends the fit when it is
 * <= tol, max_sweeps ends it otherwise.  W [nf][k]; info [nf][4] float64 = (sweeps, final KKT residual, objective, status: 0 converged,
 * 1 max_sweeps reached, 2 a non-finite entry or residual, 3 a diagonal entry of A that is not positive; 2 and 3 found in G leave W = 0).
 * k >= 1, nf >= 1, k + nf <= 32, alpha >= 0.  No workspace. */
int eg_score_lasso_gram_fit(const double* G, int k, int nf, double alpha, int max_sweeps, double tol, double* W, double* info,
                            eg_stream_t s);

/* --- device loss log of a training run: replaces the `.item()` calls of the reference's progress lines --
 * celebA/EAD-GAN_celebA.py:404-408, MNIST/EAD-GAN_rpqmnxy.py:453-457, dSprites/rp.py:491-496, colored_dSprites/rp_color.py:523-528,
 * dSprites/pxy.py:194-198, colored_dSprites/pxy_color.py:223-227 -- with one small launch inside the (captured) iteration:
 * row head[0] % capacity of ring[capacity][n] <- losses[0..n), then head[0] += 1 (head counts the iterations ever logged); if a value is
 * NaN or +-Inf and first_nonfinite[0] == 0, first_nonfinite[0] <- the 1-based iteration (sticky).  1 <= n <= 64.  No allocation, no sync. */
int eg_runlog_append(const float* losses, int n, float* ring, int capacity, int* head, int* first_nonfinite, eg_stream_t s);

/* --- exponential moving average of a trainer's weights (not in the reference, whose scripts sample from the live weights):
 * ONE launch over a segment table that lives on the device, so the launch can be captured and a replay reads no host memory.
 * A segment is n 32-bit words.  kind 0 (lerp, fp32): dst = fmaf(1 - b_t, src - dst, dst); kind 1 (copy): dst = src, bit for bit (integer
 * counters -- an int64 is two words -- and unit vectors, whose average is no unit vector).  b_t = beta when ramp == 0, else
 * min(beta, (1 + t) / (ramp + t)) in fp32 in this order of operations, t = updates[0] = the number of updates done so far: every
 * workgroup of a launch uses the same t, and the launch leaves updates[0] = t + 1.  updates[1] counts the arriving workgroups and is zero
 * between launches (the caller zeroes it once).  src is never written and nothing outside [dst, dst + n) is; the result is elementwise
 * (no float atomics): two launches from the same state give the same bits.  16-byte accesses where src and dst of a chunk are both
 * 16-byte aligned, word accesses otherwise.
 * eg_ema_plan (host only, touches no device): validates a table -- 1 <= nseg <= EG_EMA_MAX_SEGS, src / dst non-null, distinct and 4-byte
 * aligned, n > 0, kind 0 or 1, at most 2^31 chunks -- and fills chunk_first[nseg + 1], the exclusive prefix of ceil(n / chunk) with
 * chunk = eg_ema_chunk_words() words.  eg_ema_update takes DEVICE copies of the validated table and of chunk_first; 0 <= beta < 1,
 * ramp >= 0.  No allocation, no sync. */
#define EG_EMA_MAX_SEGS 256
typedef struct eg_ema_seg {
    const void* src;
    void* dst;
    size_t n;                       /* 32-bit words */
    int kind;
} eg_ema_seg;
int eg_ema_chunk_words(void);
int eg_ema_plan(const eg_ema_seg* segs_host, int nseg, unsigned int* chunk_first_host);
int eg_ema_update(const eg_ema_seg* segs_dev, const unsigned int* chunk_first_dev, int nseg, float beta, float ramp, int* updates,
                  eg_stream_t s);

/* --- sliced Wasserstein distance between two image sets (Karras et al., "Progressive Growing of GANs", 2018; not in the
 * reference, whose scripts have no image-quality number).  Images are planar fp32 [N][C][H][H]; every entry point enqueues eager launches
 * and never synchronises; no float atomics, fixed summation orders: two calls give the same bits.
 * Laplacian pyramid, g = outer([1,4,6,4,1], [1,4,6,4,1]) / 256, border i < 0 -> -i, i >= n -> 2(n-1) - i (scipy 'mirror'):
 * eg_pyr_down   : coarse [planes][H/2][H/2] = the 5 x 5 correlation of fine [planes][H][H] with g at the even rows and columns
 * eg_pyr_up_sub : fine -= (coarse written into the even positions of a zero image of side H) filtered with 4 g, in place
 * H is the FINE side in both: a power of two >= 32. */
int eg_pyr_down(const float* fine, float* coarse, int planes, int H, eg_stream_t s);
int eg_pyr_up_sub(float* fine, const float* coarse, int planes, int H, eg_stream_t s);
/* Descriptor i < n_desc is the 7 x 7 x C patch of image i / P around the centre (pos[i][0], pos[i][1]) = (y, x), int32 [n_desc][2], legal
 * in [3, H - 3); its entry k = c * 49 + dy * 7 + dx is the pixel (c, y - 3 + dy, x - 3 + dx).
 * eg_swd_patch_stats: stats [C][2] float64 = (mean, population standard deviation) of all n_desc * 49 gathered pixels of the channel,
 * summed in double about the channel's first gathered pixel.  flag[0] |= 1: a standard deviation is 0; 2: a mean or standard deviation is
 * not finite (any NaN or infinity among the gathered pixels); 4: a centre outside [3, H - 3) -- such a centre is read clamped into the
 * range by this call and by eg_swd_project, never outside the image.  The caller zeroes the flag.  ws: eg_swd_patch_stats_ws_doubles(C). */
size_t eg_swd_patch_stats_ws_doubles(int C);
int eg_swd_patch_stats(const float* img, const int* pos, int n_desc, int P, int C, int H, double* ws, double* stats, int* flag, eg_stream_t s);
/* dirs [K][D] fp32: every column divided by its Euclidean norm (the norm formed in double) */
int eg_swd_unit_columns(float* dirs, int K, int D, eg_stream_t s);
/* out[d][i] = sum_k w'[k][d] * descriptor_i[k] - sum_k w'[k][d] * mean[c(k)],  w'[k][d] = dirs[k][d] / std[c(k)],  c(k) = k / 49: the
 * projections of the per-channel normalised descriptors on the D <= 128 columns of dirs [49 C][D], written transposed (row d of out, row
 * stride ld >= n_desc) so that a direction's column is contiguous; the descriptors are gathered from img in the kernel and never stored.
 * fp32 operands and fp32 fma accumulation in k order; w' and the constant are formed in double and rounded once.
 * stats: eg_swd_patch_stats's [C][2]; ws: eg_swd_project_ws_floats(C) floats (w' and the constants). */
size_t eg_swd_project_ws_floats(int C);
int eg_swd_project(const float* img, const int* pos, int n_desc, int P, int C, int H, const float* dirs, int D, const double* stats, float* ws,
                   float* out, size_t ld, eg_stream_t s);
/* x [cols][ld] fp32: each row's first n elements sorted ascending in place (n >= 1, ld >= n, cols <= 65535, n <= 2^30); +-inf are
 * ordered as values, -0.0 and +0.0 compare equal, the result for NaN inputs is unspecified.  A bitonic network whose compare-exchanges
 * all leave the smaller value at the lower index, padded to a power of two with +inf that is never stored: tiles of
 * eg_sort_tile_elems() elements are sorted in LDS, every merge round above the tile takes one global pass per two strides >= the tile and
 * one LDS pass for all smaller strides.  No workspace. */
int eg_sort_tile_elems(void);
int eg_sort_columns_f32(float* x, int n, int cols, size_t ld, eg_stream_t s);
/* out[0] (float64) = sum |a - b| / (cols * n) over the first n elements of the rows of a, b [cols][ld]; per-element fp32 difference,
 * summed in double in a fixed order.  ws: eg_l1_mean_ws_doubles() doubles. */
size_t eg_l1_mean_ws_doubles(void);
int eg_l1_mean_f32(const float* a, const float* b, int n, int cols, size_t ld, double* ws, double* out, eg_stream_t s);

/* --- exact k nearest neighbours between rows of uint8 (not in the reference, whose scripts never compare a sample with the
 * training set).  q [nq][K] and x [n][K] contiguous uint8, 16-byte aligned; d(i, j) = sum_t (q[i][t] - x[j][t])^2 as an exact integer
 * (<= 255^2 * 32768 < 2^31).  dist [nq][k] and idx [nq][k] (int32) receive, per query, the k smallest pairs in ascending lexicographic
 * order of (d, j): equal distances go to the lower index.  The order is total, so the result does not depend on the tiling, on the number
 * of database slices or on the order of any reduction, and two calls give the same bits.  self0 >= 0 excludes the pair j == self0 + i
 * (leave-one-out: the queries are the rows self0 ... of the database; queries with self0 + i >= n exclude nothing); self0 < 0 excludes
 * nothing.  64 <= K <= 32768 with K % 64 == 0; 1 <= k <= 16 and k <= the candidates of every query (n, or n - 1 where a row is excluded).
 * The dot products run on the int8 MFMA over q ^ 0x80 and x ^ 0x80 (v - 128; distances do not change under the common shift) with int32
 * accumulation, d = |q'|^2 + |x'|^2 - 2 q'.x' in unsigned 32-bit arithmetic.  A workgroup owns eg_knn_tile_queries() queries (two such tiles from
 * 4 * eg_knn_tile_queries() queries on: another wave layout) and walks a slice of the database in tiles of eg_knn_tile_rows() rows; the database is cut into eg_knn_splits(nq, n) slices whose partial lists
 * ([splits][nq][k] packed keys d << 32 | j in ws, eg_knn_ws_bytes(nq, n, k) bytes) a second kernel merges.  No allocation, no sync. */
int eg_knn_tile_queries(void);
int eg_knn_tile_rows(void);
int eg_knn_splits(int nq, int n);
size_t eg_knn_ws_bytes(int nq, int n, int k);
int eg_knn_u8(const unsigned char* q, int nq, const unsigned char* x, int n, int K, int k, long long self0, void* ws, int* dist, int* idx,
              eg_stream_t s);
/* --- how many balls contain a row (precision, recall, density and coverage).  count[i] (int32, i < nq) = the number of rows
 * j in [0, n), j != self0 + i, with d(q[i], x[j]) <= rad[j]: q, x, d, K and self0 as for eg_knn_u8, rad [n] int32.  The balls are CLOSED
 * (a row at exactly the radius is inside).  d < 2^31 and the compare is signed: a negative rad[j] is an empty ball, which makes rad a mask.
 * The tile loop, the slices (eg_knn_splits) and the wave layouts are eg_knn_u8's; ws: eg_ball_count_ws_bytes(nq, n) = splits * nq * 4 bytes
 * of per-slice counts a second kernel sums.  count and ws are written exactly once (no atomic, no zero-fill); integer sums, so two calls
 * give the same bits.  q and x 16-byte aligned, rad, ws and count 4-byte.  Two launches, no allocation, no sync. */
size_t eg_ball_count_ws_bytes(int nq, int n);
int eg_ball_count_u8(const unsigned char* q, int nq, const unsigned char* x, int n, int K, const int* rad, long long self0,
                     void* ws, int* count, eg_stream_t s);
/* --- kernel sums and the distance select (the kernel MMD with an exact median bandwidth).  q, x, d, K, self0, the limits, the
 * alignment of q and x, the tile loop, the slices (eg_knn_splits) and the wave layouts are eg_knn_u8's.
 * eg_kernel_sum_u8: out[i][b] (double [nq][nb]) = sum over j != self0 + i of exp(-((double)d(q[i], x[j]) * inv_gamma[b])): the argument is
 * one rounded product, the exponential the device library's.  inv_gamma: a DEVICE pointer to nb doubles, 1 <= nb <= 4.  flag[0] (device
 * int32) is WRITTEN, not or-ed: bit b says inv_gamma[b] is not a finite positive number (out[.][b] then holds what the arithmetic gives).
 * ws: eg_kernel_sum_ws_bytes(nq, n, nb) = splits * nq * nb * 8 bytes of per-slice sums; the parts of a query, then its slices, are added
 * in a fixed order, everything is written exactly once (no atomic, no zero-fill): two calls with the same shapes give the same bits.
 * inv_gamma, ws and out 8-byte aligned.  Two launches, no allocation, no sync.
 * eg_dist_select_u8: out[0] (int32) = the element of 0-based rank `rank` of the multiset { d(q[i], x[j]) : j != self0 + i } in ascending
 * order; out[1] = 1 if rank >= the number of pairs (out[0] is then the largest distance, or 0 if there is no pair), else 0.  A radix
 * select, 10 bits a pass from the top: three passes of the tile loop (four where 255^2 K >= 2^30), each followed by a sum of the
 * workgroups' histograms and a one-workgroup scan that leaves the prefix and the remaining rank in ws for the next; all enqueued at once,
 * no host read.  ws: eg_dist_select_ws_bytes(nq, n) = 64 + 32 * 8192 + workgroups * 4096 bytes, 8-byte aligned. */
size_t eg_kernel_sum_ws_bytes(int nq, int n, int nb);
int eg_kernel_sum_u8(const unsigned char* q, int nq, const unsigned char* x, int n, int K, const double* inv_gamma, int nb, long long self0,
                     void* ws, double* out, int* flag, eg_stream_t s);
size_t eg_dist_select_ws_bytes(int nq, int n);
int eg_dist_select_u8(const unsigned char* q, int nq, const unsigned char* x, int n, int K, long long self0, unsigned long long rank,
                      void* ws, int* out, eg_stream_t s);
/* --- the soft minimum (one half-iteration of the debiased Sinkhorn divergence).  q, x, d, K, self0, the limits, the alignment of
 * q and x, the tile loop, the slices (eg_knn_splits) and the wave layouts are eg_knn_u8's.  g: [n] doubles on the device; inv_eps: a
 * DEVICE pointer to one double, so a whole epsilon schedule is enqueued without a host read.  With J_i = { j in [0, n) : j != self0 + i }
 * and t_ij = (g[j] - (double)d(q[i], x[j])) * inv_eps[0] (one rounded subtraction, one rounded product):
 *     soft[i] = -(log sum_{j in J_i} exp(t_ij) - log |J_i|) / inv_eps[0]
 *     out[i]  = prev ? 0.5 * prev[i] + 0.5 * soft[i] : soft[i]
 * as a streaming log-sum-exp: a running pair (m, s), m the maximum and s = sum exp(t - m), one exponential per pair of rows; two pairs
 * are merged by rescaling the one with the smaller maximum (equal maxima, two empty pairs (-inf, 0) among them, take no exponential), and
 * soft = -(m + (log s - log |J_i|)) / inv_eps[0].  |J_i| >= 1 is an argument check: n - 1 >= 1 where a row is excluded.
 * ws: eg_softmin_ws_bytes(nq, n) = splits * nq * 16 bytes of per-slice pairs; the parts of a query, then its slices, are merged in a
 * fixed order and everything is written exactly once (no atomic, no zero-fill): two calls with the same shapes give the same bits.
 * prev may be NULL; prev, g and out may alias one another: the tile kernel only reads g and writes ws, the second kernel reads prev[i]
 * before the same thread writes out[i].  flag[0] (device int32) is WRITTEN, not or-ed: bit 0 says inv_eps[0] is not a finite positive
 * number (out then holds what the arithmetic gives).  g, inv_eps, prev, ws and out 8-byte aligned.  Two launches, no allocation, no
 * sync. */
size_t eg_softmin_ws_bytes(int nq, int n);
int eg_softmin_u8(const unsigned char* q, int nq, const unsigned char* x, int n, int K, const double* g, const double* inv_eps, long long self0,
                  const double* prev, void* ws, double* out, int* flag, eg_stream_t s);

/* --- k-means over rows of uint8 (the bins of the NDB score; not in the reference).  rows [n][K] contiguous uint8, 16-byte
 * aligned, K a multiple of 64 in 64 .. 32768 (eg_knn_u8's limits); 1 <= bins <= 1024.  The contract:
 *   centres  are BYTES, [bins][K] uint8: a centre is an image, it can be shown and passed to every *_u8 entry point.  The rounding moves a
 *            centre by at most half a grey level per pixel; Lloyd's inertia is therefore not guaranteed to be monotone.
 *   assign   label[i] = the nearest centre by the exact squared L2 distance, ties to the lower index: eg_knn_u8(rows, centres, 1).
 *   update   a cell with count > 0: centre[t] = (2 sum[t] + count) / (2 count) in integers (round half up) from exact int32 column sums
 *            (n * 255 < 2^31 is an argument check); a cell with count == 0 keeps its bytes.
 *   seeding  k-means++ driven by u, bins fp32 uniforms in [0, 1) on the device: centre 0 is row min(floor((double)u[0] * n), n - 1); for
 *            j >= 1, with mind[i] the exact distance from row i to its nearest chosen centre and total its int64 sum,
 *            target = min(floor((double)u[j] * (double)total), total - 1) and the pick is the lowest row whose inclusive prefix sum of
 *            mind exceeds target: a row at distance 0 from a chosen centre is never picked.  n * 2^31 <= 2^53 is an argument check, so
 *            total is exact in a double and the product is one rounded multiplication.
 * No allocation, no sync; every output and workspace word is written once per launch that owns it, nothing is zero-filled or added to,
 * results do not depend on earlier workspace contents, all sums are integers: two calls give the same bits.
 * eg_group_rows: a stable counting sort of labels [n] (int32) into cells.  counts [bins], offsets [bins + 1] (the exclusive scan of the
 * counts; offsets[bins] = the rows that joined a cell), order [n]: the rows of cell c are order[offsets[c] .. offsets[c + 1]), ascending.
 * A label outside [0, bins) raises flag[0] bit 0 (flag is WRITTEN, not or-ed) and its row joins no cell; order[offsets[bins] .. n) = -1.
 * The count and scatter kernels give a workgroup eg_group_rows_block() labels.  ws: eg_group_rows_ws_bytes(n, bins), 16-byte aligned.
 * eg_kmeans_update_u8: rows, order, offsets, counts (eg_group_rows' outputs) -> centres [bins][K] in place under the update rule.  Every
 * member row is read once, contiguously; the member lists are cut into segments of eg_kmeans_segment_rows() rows, a workgroup sums
 * eg_kmeans_column_chunk() bytes of its segment's rows into int32 partial sums, a second kernel adds a cell's segments and
 * divides.  ws: eg_kmeans_update_ws_bytes(n, K, bins) = the segment table and (ceil(n / segment) + bins) * K * 4 bytes of partial sums.
 * eg_kmeans_seed_u8: the seeding above -> idx [bins] (int32, the picked rows), centres [bins][K] (their bytes) and flag[0] (WRITTEN):
 * bit 0 = some total was 0 (fewer than bins distinct rows; that pass picks row 0), bit 1 = a u outside [0, 1) (clamped).  All passes are
 * enqueued by this one call: per pass a streaming kernel (one centre against all rows with v_dot4, a workgroup per eg_kmeans_seed_rows()
 * rows, mind folded and an int64 partial sum per workgroup) and a one-workgroup kernel that scans the partial sums, finds the row and
 * copies it into centres, where the next pass reads it; nothing is read back.  ws: eg_kmeans_seed_ws_bytes(n), 16-byte aligned. */
int eg_group_rows_block(void);
size_t eg_group_rows_ws_bytes(int n, int bins);
int eg_group_rows(const int* labels, int n, int bins, void* ws, int* counts, int* offsets, int* order, int* flag, eg_stream_t s);
int eg_kmeans_segment_rows(void);
int eg_kmeans_column_chunk(void);
size_t eg_kmeans_update_ws_bytes(int n, int K, int bins);
int eg_kmeans_update_u8(const unsigned char* rows, int n, int K, const int* order, const int* offsets, const int* counts, int bins, void* ws,
                        unsigned char* centres, eg_stream_t s);
int eg_kmeans_seed_rows(void);
size_t eg_kmeans_seed_ws_bytes(int n);
int eg_kmeans_seed_u8(const unsigned char* rows, int n, int K, int bins, const float* u, void* ws, int* idx, unsigned char* centres, int* flag,
                      eg_stream_t s);

/* --- the azimuthally averaged power spectrum of uint8 images (not in the reference).  images [N][C][H][H] contiguous uint8,
 * 4-byte aligned, H = 16, 32 or 64, 1 <= C <= 4, N >= 1.  The contract, for image n and channel c:
 *   X[ky][kx] = sum_y sum_x u[y][x] exp(-2 pi i (ky y + kx x) / H) over the bytes as they are (nothing is subtracted),
 *   P[ky][kx] = |X|^2 / H^2 (Parseval: sum_k P = sum u^2), on the half spectrum kx = 0 .. H/2; a cell of column kx weighs w = 1 for
 *   kx in {0, H/2} and w = 2 otherwise.
 *   rings    with fy = min(ky, H - ky), q = fy^2 + kx^2 the ring of a cell is the integer b with (b - 1/2)^2 <= q < (b + 1/2)^2, i.e.
 *            s = isqrt(q), b = s if q <= s^2 + s, else s + 1: B = 12, 24, 46 rings for H = 16, 32, 64.  The CALLER builds the tables in
 *            integers, on the device: cell_ring [H][H/2 + 1] (the ring of every cell; part of the table set, not read by the launch),
 *            ring_start [B + 1] and ring_cells [H (H/2 + 1)] (the cells ky (H/2 + 1) + kx of every ring, ascending), ring_count [B] =
 *            the sum of w over the ring (they sum to H^2).  The library forms no radius.
 *   twiddles cos_sin [2][H] = cos(2 pi k / H), sin(2 pi k / H) in doubles from the caller, indexed by (k x) mod H in integers: the
 *            library evaluates no sine or cosine.
 *   profile [N][B]          = sum_{cells of ring b} w sum_c P / (C ring_count[b])
 *   full    [N][H][H/2 + 1] = sum_c P / C, written when full is not NULL.
 * float64 throughout; the direct matrix DFT in two stages (rows, then columns), every sum of H terms in index order, a cell's channels in
 * channel order, a ring's cells in ring_cells order (lane l of a wave takes the cells l, l + 64, ...; the lane sums meet in a fixed
 * tree).  One workgroup per image, no atomics, no allocation, no sync: the bits of image n depend on its bytes alone, not on N, its
 * position or the run.  |profile - exact| <= 4 H 2^-53 S^2 / H^2 with S the image's largest per-channel byte sum. */
int eg_spectrum_u8(const unsigned char* images, int N, int C, int H, const double* cos_sin, const int* cell_ring, const int* ring_start,
                   const int* ring_cells, const int* ring_count, double* profile, double* full, eg_stream_t s);

/* --- structural similarity between PAIRS of uint8 images (not in the reference): SSIM, its contrast-structure term per level
 * of a 2 x 2 mean pyramid (MS-SSIM is a product of their powers), and the squared error (PSNR).  a [na][C][H][H] and b [nb][C][H][H]
 * contiguous uint8, 4-byte aligned, a == b is allowed; H = 16, 32 or 64, 1 <= C <= 4; pairs [P][2] int32 on the device = (row of a, row of
 * b), 1 <= P < 2^31; win [K] doubles on the device, the one-dimensional window, normalised by the CALLER (the library evaluates no exp), K
 * odd, 3 <= K <= 11; 1 <= L and H >> (L - 1) >= K; c1, c2 positive and finite.  Anything else returns non-zero and launches nothing.
 * The contract, for pair p = (i, j):
 *   levels   x_l[y][x] = 4^-l (integer sum of the 2^l x 2^l block of bytes), l = 0 .. L - 1: l-fold 2 x 2 mean pooling, exact in fp64,
 *            every value <= 255.  Side H_l = H >> l; the valid window positions are 0 <= r, q <= n_l - 1 with n_l = H_l - K + 1 (Wang's
 *            "valid" form, no padding).
 *   moments  per level, channel and position mu_a, mu_b, E_aa, E_bb, E_ab of x, y, x^2, y^2, x y, each
 *            sum_dy win[dy] sum_dx win[dx] (.)[r + dy][q + dx]: rows first, then columns, every sum in index order, fp64 throughout (the
 *            products are exact in fp64).
 *   values   s_aa = E_aa - mu_a^2, s_bb = E_bb - mu_b^2, s_ab = E_ab - mu_a mu_b,
 *            cs = (2 s_ab + c2) / (s_aa + s_bb + c2), lum = (2 mu_a mu_b + c1) / (mu_a^2 + mu_b^2 + c1), ssim = lum cs.
 *   stats [P][L][2]: stats[p][l][0] = the mean of ssim, stats[p][l][1] = the mean of cs over channels and positions, summed in a fixed
 *            order: an output column's rows in row order (one thread), then per level the C n_l column sums, channel then column, lane k of
 *            a wave taking the columns k, k + 64, ..., the lane sums meeting in a fixed tree.
 *   sse [P]: sum (a - b)^2 over all bytes of the pair, an exact integer.
 *   A pair with an index outside [0, na) x [0, nb): nothing is read, stats[p] = NaN, sse[p] = -1, and *flag (int32, ZEROED BY THE CALLER)
 *   is set to 2 (bit 1) by a plain store of that constant; all other pairs are unaffected.
 * One workgroup per pair, no atomics, no allocation, no sync: the bits of pair p depend on its two images, win, c1, c2, K and L alone, not
 * on P, its place in the table, other pairs or the run.  |ssim - exact| <= (8 / k1^2 + 12 / k2^2) (2 K + 2) 2^-53 with c1 = (255 k1)^2,
 * c2 = (255 k2)^2 (2.5e-10 at K = 11 and the usual k1 = 0.01, k2 = 0.03); the means inherit it. */
int eg_ssim_u8(const unsigned char* a, int na, const unsigned char* b, int nb, int C, int H, const int* pairs, int P, const double* win, int K,
               int L, double c1, double c2, double* stats, long long* sse, int* flag, eg_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* EADGAN_HIP_H */
