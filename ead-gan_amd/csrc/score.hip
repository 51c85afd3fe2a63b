// Disentanglement scores of a trained dSprites / colored-dSprites encoder pair: MIG and FactorVAE (dSprites/score/MIG.py,
// FactorVAE.py; colored_dSprites/score/MIG.py, FactorVAE.py).  The encoder passes themselves run on the existing engines
// (Encoder_pxy forward, eg_theta_pxy_align_inv, eg_warp_affine_zeros, eg_color_scale, the eval-mode trunk); this file holds the
// staging gather in front of them, the representation rows behind them and the metric arithmetic.
//
// Built with -ffp-contract=off: the histogram edges, the FactorVAE moments and the MI terms reproduce numpy's / sklearn's float64
// operation sequence, which a fused multiply-add would change.
#include "eg_common.h"

// ---- staging: out[b][c][p] = float(data[idx[b]][p]) * gain[b][c]  (gain NULL: 1) ------------------------------------------------
// The reference's colouring (add_color_2_img) multiplies the {0,1} sprite by a float64 gain and casts to float32: every pixel is
// float32(gain) or 0, which is what the float32 gain the host uploads gives here.
__global__ void score_stage_kernel(const unsigned char* __restrict__ data, const int* __restrict__ idx, const float* __restrict__ gain,
                                   float* __restrict__ out, int B, int C, int HW4) {
    const size_t total = (size_t)B * C * HW4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int p4 = (int)(e % HW4);
        const int bc = (int)(e / HW4);
        const int b = bc / C, c = bc - b * C;
        const uchar4 v = reinterpret_cast<const uchar4*>(data + (size_t)idx[b] * HW4 * 4)[p4];
        const float g = gain ? gain[(size_t)b * C + c] : 1.f;
        reinterpret_cast<float4*>(out)[e] = make_float4((float)v.x * g, (float)v.y * g, (float)v.z * g, (float)v.w * g);
    }
}

extern "C" int eg_score_stage_u8(const unsigned char* data, const int* idx, const float* gain, float* out, int B, int C, int HW, eg_stream_t s) {
    EG_REQUIRE(data && idx && out && B > 0 && C > 0 && HW > 0 && HW % 4 == 0, "eg_score_stage_u8: bad argument");
    const size_t total = (size_t)B * C * (HW / 4);
    const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    hipLaunchKernelGGL(score_stage_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, data, idx, gain, out, B, C, HW / 4);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- representation rows: [argmax softmax(cat), cont0, cont1, pxy1, pxy2] as float64 ---------------------------------------------
__global__ void score_rows_kernel(const float* __restrict__ cat, int ldcat, int ncat, const float* __restrict__ cont, int ldcont,
                                  const float* __restrict__ pxy, int ldpxy, int B, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* l = cat + (size_t)b * ldcat;
    float m = l[0];
    for (int j = 1; j < ncat; ++j) m = fmaxf(m, l[j]);
    float sum = 0.f;
    for (int j = 0; j < ncat; ++j) sum += expf(l[j] - m);
    int arg = 0;
    float best = expf(l[0] - m) / sum;
    for (int j = 1; j < ncat; ++j) {             // np.argmax over the probabilities: the first index on ties
        const float p = expf(l[j] - m) / sum;
        if (p > best) best = p, arg = j;
    }
    double* o = out + (size_t)b * 5;
    o[0] = (double)arg;
    o[1] = (double)cont[(size_t)b * ldcont + 0];
    o[2] = (double)cont[(size_t)b * ldcont + 1];
    o[3] = (double)pxy[(size_t)b * ldpxy + 1];
    o[4] = (double)pxy[(size_t)b * ldpxy + 2];
}

extern "C" int eg_score_rows(const float* cat, int ldcat, int ncat, const float* cont, int ldcont, const float* pxy, int ldpxy, int B,
                             double* out, eg_stream_t s) {
    EG_REQUIRE(cat && cont && pxy && out && B > 0 && ncat >= 1 && ncat <= ldcat && ldcont >= 2 && ldpxy >= 3, "eg_score_rows: bad argument");
    hipLaunchKernelGGL(score_rows_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)s, cat, ldcat, ncat, cont, ldcont, pxy, ldpxy, B, out);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- MIG: per-column histogram discretisation -------------------------------------------------------------------------------------
// One block per code column: min / max over the n rows, numpy's edges (np.histogram -> np.linspace: lo, hi widened by 0.5 when equal,
// step = (hi - lo) / nbins, edge_k = k * step + lo, unfused), bin = number of edges <= x (np.digitize on the first nbins edges), 1..nbins.
__device__ __forceinline__ double dmin_wave(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double dmax_wave(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

__global__ void score_digitize_kernel(const double* __restrict__ codes, int n, int ncode, int nbins, int* __restrict__ bins,
                                      double* __restrict__ lohi) {
    __shared__ double smin[16], smax[16];
    __shared__ double edges[64];
    const int c = blockIdx.x;
    double lo = INFINITY, hi = -INFINITY;
    for (int r = threadIdx.x; r < n; r += blockDim.x) {
        const double x = codes[(size_t)r * ncode + c];
        lo = fmin(lo, x);
        hi = fmax(hi, x);
    }
    lo = dmin_wave(lo);
    hi = dmax_wave(hi);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) smin[w] = lo, smax[w] = hi;
    __syncthreads();
    lo = smin[0], hi = smax[0];
    for (int i = 1; i < nw; ++i) lo = fmin(lo, smin[i]), hi = fmax(hi, smax[i]);
    if (lo == hi) lo = lo - 0.5, hi = hi + 0.5;
    const double step = (hi - lo) / (double)nbins;
    if (threadIdx.x < nbins) {
        const double t = (double)threadIdx.x * step;
        edges[threadIdx.x] = t + lo;
    }
    if (threadIdx.x == 0 && lohi) lohi[2 * c] = lo, lohi[2 * c + 1] = hi;
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += blockDim.x) {
        const double x = codes[(size_t)r * ncode + c];
        int k = 0;
        for (int e = 0; e < nbins; ++e) k += edges[e] <= x ? 1 : 0;
        bins[(size_t)c * n + r] = k;
    }
}

extern "C" int eg_score_digitize(const double* codes, int n, int ncode, int nbins, int* bins, double* lohi, eg_stream_t s) {
    EG_REQUIRE(codes && bins && n > 0 && ncode > 0 && nbins >= 1 && nbins <= 64, "eg_score_digitize: bad argument");
    hipLaunchKernelGGL(score_digitize_kernel, dim3(ncode), dim3(1024), 0, (hipStream_t)s, codes, n, ncode, nbins, bins, lohi);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- MIG: contingency tables and sklearn.metrics.mutual_info_score ---------------------------------------------------------------
// Table t < ncode * nf is (factor j = t % nf, code i = t / nf): rows = factor class ids (labels_true), columns = bins - 1
// (labels_pred).  Table ncode * nf + j is (factor j, factor j).  Every table is [kmax][cmax] int32 in `ws`.
__global__ void score_contingency_kernel(const int* __restrict__ bins, int ncode, const int* __restrict__ ys, int nf, int n, int kmax,
                                         int cmax, int* __restrict__ ws) {
    const int t = blockIdx.y;
    const int* rowl;
    const int* coll;
    int coff;
    if (t < ncode * nf) {
        rowl = ys + (size_t)(t % nf) * n;
        coll = bins + (size_t)(t / nf) * n;
        coff = -1;
    } else {
        rowl = ys + (size_t)(t - ncode * nf) * n;
        coll = rowl;
        coff = 0;
    }
    int* tab = ws + (size_t)t * kmax * cmax;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
    {
        const int a = rowl[r], b = coll[r] + coff;
        if (a >= 0 && a < kmax && b >= 0 && b < cmax) atomicAdd(tab + (size_t)a * cmax + b, 1);     // ids outside the table are dropped
    }
}

// One block per table.  The sum over the non-zero cells of
//   nm * (log(c) - log(N)) + nm * (-log(pi * pj) + log(N) + log(N)),   nm = c / N,
// terms with |term| < DBL_EPSILON set to 0, the total clipped at 0; 0 when either labelling has a single cluster (sklearn 1.x).
__global__ void score_mi_kernel(const int* __restrict__ ws, int kmax, int cmax, double* __restrict__ mi) {
    extern __shared__ long long sh[];
    long long* pi = sh;
    long long* pj = sh + kmax;
    __shared__ int nzi[16], nzj[16];
    __shared__ double sm[16];
    const int t = blockIdx.x;
    const int* tab = ws + (size_t)t * kmax * cmax;
    for (int r = threadIdx.x; r < kmax; r += blockDim.x) {
        long long a = 0;
        for (int c = 0; c < cmax; ++c) a += tab[(size_t)r * cmax + c];
        pi[r] = a;
    }
    for (int c = threadIdx.x; c < cmax; c += blockDim.x) {
        long long a = 0;
        for (int r = 0; r < kmax; ++r) a += tab[(size_t)r * cmax + c];
        pj[c] = a;
    }
    __syncthreads();
    int ci = 0, cj = 0;
    long long part = 0;
    for (int r = threadIdx.x; r < kmax; r += blockDim.x) ci += pi[r] != 0, part += pi[r];
    for (int c = threadIdx.x; c < cmax; c += blockDim.x) cj += pj[c] != 0;
    // counts of non-empty clusters and N: integer sums, order free
    for (int o = 32; o > 0; o >>= 1) {
        ci += __shfl_xor(ci, o);
        cj += __shfl_xor(cj, o);
        part += __shfl_xor(part, o);
    }
    __shared__ long long sN[16];
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) nzi[w] = ci, nzj[w] = cj, sN[w] = part;
    __syncthreads();
    int nci = 0, ncj = 0;
    long long N = 0;
    for (int i = 0; i < nw; ++i) nci += nzi[i], ncj += nzj[i], N += sN[i];
    if (nci <= 1 || ncj <= 1) {
        if (threadIdx.x == 0) mi[t] = 0.0;
        return;
    }
    const double dN = (double)N, logN = log(dN);
    double acc = 0.0;
    for (int e = threadIdx.x; e < kmax * cmax; e += blockDim.x) {
        const int v = tab[e];
        if (v == 0) continue;
        const int r = e / cmax, c = e - r * cmax;
        const double nm = (double)v / dN;
        const double lc = log((double)v);
        const double log_outer = (-log((double)(pi[r] * pj[c])) + logN) + logN;
        const double a = nm * (lc - logN);
        const double b = nm * log_outer;
        double term = a + b;
        if (fabs(term) < 2.220446049250313e-16) term = 0.0;
        acc += term;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < nw; ++i) tot += sm[i];
        mi[t] = tot > 0.0 ? tot : 0.0;
    }
}

extern "C" size_t eg_score_mig_ws_ints(int ncode, int nf, int kmax, int nbins) {
    const size_t cmax = (size_t)(kmax > nbins ? kmax : nbins);
    return (size_t)(ncode * nf + nf) * kmax * cmax;
}

extern "C" int eg_score_mig(const int* bins, int ncode, const int* ys, int nf, int n, int kmax, int nbins, int* ws, double* mi, eg_stream_t s) {
    EG_REQUIRE(bins && ys && ws && mi && n > 0 && ncode > 0 && nf > 0 && kmax > 0 && nbins > 0, "eg_score_mig: bad argument");
    const int cmax = kmax > nbins ? kmax : nbins;
    EG_REQUIRE((size_t)(kmax + cmax) * sizeof(long long) <= 48 * 1024, "eg_score_mig: %d factor classes exceed the shared-memory marginals", kmax);
    const int ntab = ncode * nf + nf;
    hipError_t e = hipMemsetAsync(ws, 0, eg_score_mig_ws_ints(ncode, nf, kmax, nbins) * sizeof(int), (hipStream_t)s);
    if (e != hipSuccess) EG_FAIL((int)e, "eg_score_mig: %s", hipGetErrorString(e));
    const int gx = cdiv(n, 256) < 64 ? cdiv(n, 256) : 64;
    hipLaunchKernelGGL(score_contingency_kernel, dim3(gx, ntab), dim3(256), 0, (hipStream_t)s, bins, ncode, ys, nf, n, kmax, cmax, ws);
    EG_LAUNCH_CHECK();
    hipLaunchKernelGGL(score_mi_kernel, dim3(ntab), dim3(256), (size_t)(kmax + cmax) * sizeof(long long), (hipStream_t)s, ws, kmax, cmax, mi);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- FactorVAE ----------------------------------------------------------------------------------------------------------------------
// np.std(x, axis=0) of a C-contiguous [n][ncol] float64 array: numpy reduces axis 0 by adding the rows one after the other into the
// accumulator row (no pairwise summation across rows), mean = sum / n, then the same over (x - mean)^2, / n, sqrt.  One thread per
// column reproduces that sequence exactly.
__global__ void score_col_std_kernel(const double* __restrict__ x, int n, int ncol, double* __restrict__ out) {
    const int c = threadIdx.x;
    if (c >= ncol) return;
    double s = 0.0;
    for (int r = 0; r < n; ++r) s = r == 0 ? x[(size_t)r * ncol + c] : s + x[(size_t)r * ncol + c];
    const double mean = s / (double)n;
    double q = 0.0;
    for (int r = 0; r < n; ++r) {
        const double d = x[(size_t)r * ncol + c] - mean;
        const double d2 = d * d;
        q = r == 0 ? d2 : q + d2;
    }
    out[c] = sqrt(q / (double)n);
}

extern "C" int eg_score_col_std(const double* x, int n, int ncol, double* out, eg_stream_t s) {
    EG_REQUIRE(x && out && n > 0 && ncol > 0 && ncol <= 64, "eg_score_col_std: bad argument");
    hipLaunchKernelGGL(score_col_std_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, x, n, ncol, out);
    EG_LAUNCH_CHECK();
    return 0;
}

// Group g holds rows [g*L, (g+1)*L) of `x`.  Its prediction is argmin over the columns of std(x_g / eval_std) with numpy's rule (the
// first NaN when there is one, else the first minimum); votes[predict][labels[g]] += 1.  The column values x / 0 are +-inf or NaN
// exactly as in numpy (IEEE division), and their std is NaN.
__global__ void score_fvae_kernel(const double* __restrict__ x, int L, int M, int ncol, const double* __restrict__ eval_std,
                                  const int* __restrict__ labels, int nlab, int* __restrict__ predict, unsigned long long* __restrict__ votes) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= M) return;
    const double* xg = x + (size_t)g * L * ncol;
    int arg = 0;
    double best = 0.0;
    bool nan = false;
    for (int c = 0; c < ncol; ++c) {
        const double sd = eval_std[c];
        double s = 0.0;
        for (int r = 0; r < L; ++r) {
            const double v = xg[(size_t)r * ncol + c] / sd;
            s = r == 0 ? v : s + v;
        }
        const double mean = s / (double)L;
        double q = 0.0;
        for (int r = 0; r < L; ++r) {
            const double d = xg[(size_t)r * ncol + c] / sd - mean;
            const double d2 = d * d;
            q = r == 0 ? d2 : q + d2;
        }
        const double v = sqrt(q / (double)L);
        if (nan) continue;
        if (v != v) {
            nan = true, arg = c;
        } else if (c == 0 || v < best) {
            best = v, arg = c;
        }
    }
    if (predict) predict[g] = arg;
    const int lab = labels[g];
    if (lab >= 0 && lab < nlab) atomicAdd(votes + (size_t)arg * nlab + lab, 1ull);
}

extern "C" int eg_score_fvae_votes(const double* x, int L, int M, int ncol, const double* eval_std, const int* labels, int nlab, int* predict,
                                   long long* votes, eg_stream_t s) {
    EG_REQUIRE(x && eval_std && labels && votes && L > 0 && M > 0 && ncol > 0 && nlab > 0, "eg_score_fvae_votes: bad argument");
    hipError_t e = hipMemsetAsync(votes, 0, (size_t)ncol * nlab * sizeof(long long), (hipStream_t)s);
    if (e != hipSuccess) EG_FAIL((int)e, "eg_score_fvae_votes: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(score_fvae_kernel, dim3(cdiv(M, 64)), dim3(64), 0, (hipStream_t)s, x, L, M, ncol, eval_std, labels, nlab, predict,
                       reinterpret_cast<unsigned long long*>(votes));
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- BetaVAE ------------------------------------------------------------------------------------------------------------------------
// feat[g] = np.mean(np.abs(x_g[0::2] - x_g[1::2]), axis=0) (BetVAE.py:256-257): numpy adds the L/2 rows of |differences| one after the
// other into the accumulator row, then divides by L/2.  One thread per (group, column) reproduces that sequence exactly.
__global__ void score_pair_absdiff_mean_kernel(const double* __restrict__ x, int L, int M, int ncol, double* __restrict__ feat) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)M * ncol) return;
    const size_t g = e / ncol;
    const int c = (int)(e - g * ncol);
    const double* xg = x + g * (size_t)L * ncol + c;
    double s = 0.0;
    for (int r = 0; r < L; r += 2) {
        const double v = fabs(xg[(size_t)r * ncol] - xg[(size_t)(r + 1) * ncol]);
        s = r == 0 ? v : s + v;
    }
    feat[e] = s / (double)(L / 2);
}

extern "C" int eg_score_pair_absdiff_mean(const double* x, int L, int M, int ncol, double* feat, eg_stream_t s) {
    EG_REQUIRE(x && feat && L > 0 && M > 0 && ncol > 0, "eg_score_pair_absdiff_mean: bad argument");
    EG_REQUIRE(L % 2 == 0, "eg_score_pair_absdiff_mean: L = %d is odd, the rows of a group are paired", L);
    const size_t total = (size_t)M * ncol;
    hipLaunchKernelGGL(score_pair_absdiff_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s, x, L, M, ncol, feat);
    EG_LAUNCH_CHECK();
    return 0;
}

// The fit itself (classifier.fit of BetVAE.py:265-266) is eg_score_softmax_fit (score_fstat.hip); its training predictions:
// predict[i] = np.argmax of the logits of row i (first index on ties); correct[0] = #{predict == y} (zeroed here; integer atomics)
__global__ void score_logreg_accuracy_kernel(const double* __restrict__ X, const int* __restrict__ y, int n, int d, int K,
                                             const double* __restrict__ W, int* __restrict__ predict, unsigned long long* __restrict__ correct) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int arg = 0;
    double best = 0.0;
    for (int k = 0; k < K; ++k) {
        double a = 0.0;
        for (int c = 0; c < d; ++c) a += W[k * (d + 1) + c] * X[(size_t)i * d + c];
        a += W[k * (d + 1) + d];
        if (k == 0 || a > best) best = a, arg = k;
    }
    predict[i] = arg;
    if (arg == y[i]) atomicAdd(correct, 1ull);
}

extern "C" int eg_score_logreg_accuracy(const double* X, const int* y, int n, int d, int K, const double* W, int* predict, long long* correct,
                                        eg_stream_t s) {
    EG_REQUIRE(X && y && W && predict && correct && n > 0 && d > 0 && K > 0, "eg_score_logreg_accuracy: bad argument");
    hipError_t e = hipMemsetAsync(correct, 0, sizeof(long long), (hipStream_t)s);
    if (e != hipSuccess) EG_FAIL((int)e, "eg_score_logreg_accuracy: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(score_logreg_accuracy_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, X, y, n, d, K, W, predict,
                       reinterpret_cast<unsigned long long*>(correct));
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- SAP ----------------------------------------------------------------------------------------------------------------------------
// All float64.  Every row sum below has one order: thread t adds rows t, t + SVC_THREADS, ... ascending, a 64-lane butterfly combines
// the lanes of a wave, and the four wave sums are added as (w0 + w1) + (w2 + w3).  No float atomics and no hand-off between workgroups:
// two runs give the same bits.
#define SVC_THREADS 256
#define SVC_KMAX 64

// sums of NV per-thread values over the workgroup; every thread receives the same totals.  red: [4 * NV] doubles of LDS.
template <int NV>
__device__ __forceinline__ void score_block_sum(double (&a)[NV], double* red) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
        for (int o = 32; o > 0; o >>= 1) a[j] += __shfl_xor(a[j], o);
    __syncthreads();                           // the previous call's readers are done with red
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) red[w * NV + j] = a[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) a[j] = (red[j] + red[NV + j]) + (red[2 * NV + j] + red[3 * NV + j]);
}

// R[i][j] = cov(i, j)^2 / var(i) / var(j) of code column i and factor column j as np.cov(x, y, ddof=1) gives them (SAP.py:295-300): the
// means first, then the centred sums times 1 / (n - 1).  One workgroup per (i, j).  A zero variance divides 0 by 0: NaN, as in numpy.
__global__ void __launch_bounds__(SVC_THREADS) score_sq_corr_kernel(const double* __restrict__ codes, int k, const double* __restrict__ fv,
                                                                    int nf, int n, double* __restrict__ R) {
    __shared__ double red[4 * 3];
    const int i = blockIdx.x / nf, j = blockIdx.x - i * nf;
    const double* x = codes + i;
    const double* y = fv + j;
    double s[2] = {0.0, 0.0};
    for (int r = threadIdx.x; r < n; r += SVC_THREADS) s[0] += x[(size_t)r * k], s[1] += y[(size_t)r * nf];
    score_block_sum<2>(s, red);
    const double mx = s[0] / (double)n, my = s[1] / (double)n;
    double c[3] = {0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < n; r += SVC_THREADS) {
        const double dx = x[(size_t)r * k] - mx, dy = y[(size_t)r * nf] - my;
        c[0] += dx * dx, c[1] += dy * dy, c[2] += dx * dy;
    }
    score_block_sum<3>(c, red);
    if (threadIdx.x == 0) {
        const double f = 1.0 / (double)(n - 1);
        const double vx = c[0] * f, vy = c[1] * f, cxy = c[2] * f;
        R[blockIdx.x] = cxy * cxy / vx / vy;
    }
}

extern "C" int eg_score_sq_corr(const double* codes, int n, int k, const double* fv, int nf, double* R, eg_stream_t s) {
    EG_REQUIRE(codes && fv && R && k > 0 && nf > 0, "eg_score_sq_corr: bad argument");
    EG_REQUIRE(n >= 2, "eg_score_sq_corr: n = %d rows, the covariance with ddof = 1 needs at least 2", n);
    hipLaunchKernelGGL(score_sq_corr_kernel, dim3(k * nf), dim3(SVC_THREADS), 0, (hipStream_t)s, codes, k, fv, nf, n, R);
    EG_LAUNCH_CHECK();
    return 0;
}

// One-feature LinearSVC(C, class_weight="balanced") with sklearn's defaults (SAP.py:303-304): L2 penalty, squared hinge, one-vs-rest,
// the intercept a regularised weight on a constant feature 1.  For class k, s_i = +1 where y_i = k and -1 elsewhere,
//   f(w, b) = (w^2 + b^2) / 2 + sum_i c_i max(0, 1 - s_i (w x_i + b))^2,   c_i = C n / (K count_k) where y_i = k, C elsewhere
// (liblinear weights only the positive side of a one-vs-rest problem).  f is strictly convex: one optimum, whatever liblinear's
// randomised dual coordinate descent stops at.  Generalised Newton from (0, 0): one pass over the rows gives f, the gradient and the
// 2 x 2 generalised Hessian I + 2 sum_{active} c_i [x_i, 1][x_i, 1]^T, which is solved in closed form; Armijo backtracking with
// eg_score_softmax_fit's constants (1e-4, halving, 40 trials, the n eps |f| slack).  The sums at an accepted trial point are the next
// iteration's.
struct SvcPoint {
    double f, gw, gb, hww, hwb, hbb;
};

__device__ SvcPoint svc1_eval(const double* __restrict__ x, int P, const int* __restrict__ y, int n, int k, double cpos, double C, double w,
                              double b, double* red) {
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += SVC_THREADS) {
        const double xi = x[(size_t)i * P];
        const bool pos = y[i] == k;
        const double sg = pos ? 1.0 : -1.0, c = pos ? cpos : C;
        const double m = 1.0 - sg * (w * xi + b);
        if (!(m <= 0.0)) {                     // active; a NaN margin enters the sums and surfaces as status 5
            const double cm = c * m, t = sg * cm, cx = c * xi;
            a[0] += cm * m;
            a[1] += t * xi;
            a[2] += t;
            a[3] += cx * xi;
            a[4] += cx;
            a[5] += c;
        }
    }
    score_block_sum<6>(a, red);
    SvcPoint p;
    p.f = 0.5 * (w * w + b * b) + a[0];
    p.gw = w - 2.0 * a[1];
    p.gb = b - 2.0 * a[2];
    p.hww = 1.0 + 2.0 * a[3];
    p.hwb = 2.0 * a[4];
    p.hbb = 1.0 + 2.0 * a[5];
    return p;
}

// workgroup blockIdx.x = column p * K + class k
__global__ void __launch_bounds__(SVC_THREADS) score_svc1_fit_kernel(const double* __restrict__ X, const int* __restrict__ y, int n, int P,
                                                                     int K, double C, int max_iter, double gtol, double* __restrict__ Wout,
                                                                     double* __restrict__ info) {
    __shared__ double red[4 * 6];
    __shared__ int cnt[SVC_KMAX];
    const int tid = threadIdx.x;
    const int p = blockIdx.x / K, k = blockIdx.x - p * K;
    double* wo = Wout + (size_t)blockIdx.x * 2;
    double* io = info + (size_t)blockIdx.x * 4;
    if (tid < SVC_KMAX) cnt[tid] = 0;
    __syncthreads();
    int bad = 0;
    for (int i = tid; i < n; i += SVC_THREADS) {
        const int yi = y[i];
        if (yi < 0 || yi >= K) bad = 1;
        else atomicAdd(&cnt[yi], 1);           // integer counts: order free
    }
    bad = __syncthreads_or(bad);
    for (int j = 0; j < K; ++j) bad |= cnt[j] == 0 ? 1 : 0;
    if (bad) {                                 // a label outside 0..K-1 or a class without a sample: nothing is fitted
        if (tid == 0) wo[0] = 0.0, wo[1] = 0.0, io[0] = 0.0, io[1] = INFINITY, io[2] = INFINITY, io[3] = 4.0;
        return;
    }
    const double cpos = C * ((double)n / (double)((long long)K * cnt[k]));     // sklearn's balanced weight n / (K count_k), times C
    const double* x = X + p;
    double w = 0.0, b = 0.0;
    SvcPoint cur = svc1_eval(x, P, y, n, k, cpos, C, w, b, red);
    double gmax = INFINITY;
    int it = 0, status = 1;
    for (;;) {
        gmax = fmax(fabs(cur.gw), fabs(cur.gb));
        if (!(gmax > gtol)) {
            status = gmax <= gtol ? 0 : 5;     // 5: the gradient is NaN
            break;
        }
        if (it >= max_iter) break;             // status 1
        const double det = cur.hww * cur.hbb - cur.hwb * cur.hwb;
        const double sw = -(cur.hbb * cur.gw - cur.hwb * cur.gb) / det;
        const double sb = -(cur.hww * cur.gb - cur.hwb * cur.gw) / det;
        const double gs = cur.gw * sw + cur.gb * sb;
        if (!(det > 0.0) || !(gs < 0.0)) {     // H >= I in exact arithmetic: only an overflow or a NaN comes here
            status = 5;
            break;
        }
        const double slack = (double)n * 2.220446049250313e-16 * fabs(cur.f);
        double t = 1.0, wt = w, bt = b;
        SvcPoint trial = cur;
        bool ok = false;
        for (int h = 0; h < 40; ++h) {
            wt = w + t * sw, bt = b + t * sb;
            trial = svc1_eval(x, P, y, n, k, cpos, C, wt, bt, red);
            if (trial.f <= cur.f + 1e-4 * t * gs + slack) {
                ok = true;
                break;
            }
            t *= 0.5;
        }
        if (!ok) {
            status = 2;
            break;
        }
        w = wt, b = bt, cur = trial;
        ++it;
    }
    if (tid == 0) wo[0] = w, wo[1] = b, io[0] = (double)it, io[1] = gmax, io[2] = cur.f, io[3] = (double)status;
}

extern "C" int eg_score_svc1_fit(const double* X, const int* y, int n, int P, int K, double C, int max_iter, double gtol, double* W,
                                 double* info, eg_stream_t s) {
    EG_REQUIRE(X && y && W && info && n > 0 && P > 0 && max_iter >= 0 && gtol >= 0.0, "eg_score_svc1_fit: bad argument");
    EG_REQUIRE(K >= 3 && K <= SVC_KMAX, "eg_score_svc1_fit: K = %d classes, 3..%d supported (liblinear fits K = 2 as one problem)", K, SVC_KMAX);
    EG_REQUIRE(C > 0.0, "eg_score_svc1_fit: C must be positive");
    EG_REQUIRE((long long)P * K <= 65535, "eg_score_svc1_fit: P K = %lld problems exceed one launch", (long long)P * K);
    hipLaunchKernelGGL(score_svc1_fit_kernel, dim3(P * K), dim3(SVC_THREADS), 0, (hipStream_t)s, X, y, n, P, K, C, max_iter, gtol, W, info);
    EG_LAUNCH_CHECK();
    return 0;
}

// predict[p][i] = np.argmax_k (w_pk x_ip + b_pk), the first index on ties (LinearSVC.predict over decision_function, SAP.py:305);
// correct[p] = #{i: predict[p][i] == y[i]} (zeroed here; one integer atomic per workgroup).  blockIdx.y = column p.
__global__ void __launch_bounds__(SVC_THREADS) score_svc1_accuracy_kernel(const double* __restrict__ X, const int* __restrict__ y, int n,
                                                                          int P, int K, const double* __restrict__ W,
                                                                          int* __restrict__ predict, unsigned long long* __restrict__ correct) {
    const int p = blockIdx.y;
    const int i = blockIdx.x * SVC_THREADS + threadIdx.x;
    const double* wp = W + (size_t)p * K * 2;
    int hit = 0;
    if (i < n) {
        const double xi = X[(size_t)i * P + p];
        int arg = 0;
        double best = 0.0;
        for (int k = 0; k < K; ++k) {
            const double a = wp[2 * k] * xi + wp[2 * k + 1];
            if (k == 0 || a > best) best = a, arg = k;
        }
        predict[(size_t)p * n + i] = arg;
        hit = arg == y[i] ? 1 : 0;
    }
    const int hits = __syncthreads_count(hit);
    if (threadIdx.x == 0 && hits) atomicAdd(correct + p, (unsigned long long)hits);
}

extern "C" int eg_score_svc1_accuracy(const double* X, const int* y, int n, int P, int K, const double* W, int* predict, long long* correct,
                                      eg_stream_t s) {
    EG_REQUIRE(X && y && W && predict && correct && n > 0 && P > 0 && K > 0 && P <= 65535, "eg_score_svc1_accuracy: bad argument");
    hipError_t e = hipMemsetAsync(correct, 0, (size_t)P * sizeof(long long), (hipStream_t)s);
    if (e != hipSuccess) EG_FAIL((int)e, "eg_score_svc1_accuracy: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(score_svc1_accuracy_kernel, dim3(cdiv(n, SVC_THREADS), P), dim3(SVC_THREADS), 0, (hipStream_t)s, X, y, n, P, K, W,
                       predict, reinterpret_cast<unsigned long long*>(correct));
    EG_LAUNCH_CHECK();
    return 0;
}
