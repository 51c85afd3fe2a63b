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
