// The DCI (Lasso) score (dSprites/score/DCI.py, colored_dSprites/score/DCI.py) on the device.
//   eg_score_norm_gram       DCIMetric.normalize of the code and factor columns, as their moments and the correlation matrix
//                            G = Z^T Z / n of the normalised columns Z = (X - mean) / std: every Lasso fit of the script depends on
//                            the data through G alone
//   eg_score_lasso_gram_fit  the optimum of sklearn's Lasso(alpha) for every factor, by cyclic coordinate descent on G
// All float64.  No float atomics, no hand-off between workgroups inside a launch: every sum has one order (inside a row slice each
// row group adds its rows, tiles and rows ascending, then the groups are added in ascending order; then the slices ascending), so two
// calls give the same bits.
#include <math.h>

#include "eg_common.h"

#define NG_THREADS 256
#define NG_MMAX 32             // columns k + nf
#define NG_TILE 128            // rows of a slice staged in LDS at a time
#define NG_SLICE_ROWS 512      // rows per slice at least (below NG_SLICES slices)
#define NG_SLICES 1024         // row slices = workgroups at most
#define NG_ZERO_VAR 1          // status bits
#define NG_NONFINITE 2

struct NgDims {
    int n, k, nf, m;           // m = k + nf columns
    int NS, RS;                // row slices, rows per slice
};

static NgDims ng_dims(int n, int k, int nf) {
    NgDims d;
    d.n = n, d.k = k, d.nf = nf, d.m = k + nf;
    const long long want = ((long long)n + NG_SLICE_ROWS - 1) / NG_SLICE_ROWS;
    d.NS = want < NG_SLICES ? (int)want : NG_SLICES;
    d.RS = (int)(((long long)n + d.NS - 1) / d.NS);
    return d;
}

struct NgWs {
    double *psum, *pmin, *pmax;    // [NS][m] each
    double* pcross;                // [NS][m][m]
};

static size_t ng_layout(const NgDims& d, void* base, NgWs* w) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? (char*)base + off : nullptr;
        off += (bytes + 255) / 256 * 256;
        return p;
    };
    NgWs l;
    l.psum = (double*)take((size_t)d.NS * d.m * sizeof(double));
    l.pmin = (double*)take((size_t)d.NS * d.m * sizeof(double));
    l.pmax = (double*)take((size_t)d.NS * d.m * sizeof(double));
    l.pcross = (double*)take((size_t)d.NS * d.m * d.m * sizeof(double));
    if (w) *w = l;
    return off;
}

// rows [r0, r0 + nr) of [codes | fv] into tile [nr][m]: both arrays are read as the contiguous runs they are
__device__ __forceinline__ void ng_load_tile(const double* __restrict__ codes, const double* __restrict__ fv, const NgDims& d, size_t r0,
                                             int nr, double* tile) {
    const int k = d.k, nf = d.nf, m = d.m;
    const double* c = codes + r0 * k;
    for (int e = threadIdx.x; e < nr * k; e += NG_THREADS) {
        const int r = e / k;
        tile[r * m + (e - r * k)] = c[e];
    }
    const double* f = fv + r0 * nf;
    for (int e = threadIdx.x; e < nr * nf; e += NG_THREADS) {
        const int r = e / nf;
        tile[r * m + k + (e - r * nf)] = f[e];
    }
}

// the slice of workgroup b: rows [i0, i1), empty past the end
__device__ __forceinline__ void ng_slice(const NgDims& d, size_t* i0, size_t* i1) {
    const size_t n = (size_t)d.n;
    const size_t a = (size_t)blockIdx.x * d.RS;
    *i0 = a < n ? a : n;
    *i1 = *i0 + d.RS < n ? *i0 + d.RS : n;
}

// ---- pass 1: per slice the column sums, minima and maxima --------------------------------------------------------------------------
// thread (q = tid / 32, c = tid % 32) takes rows q, q + 8, ... of each tile of column c; the 8 groups are added in ascending order.
// min == max is the exact test for a column without variance (a rounded mean of equal values need not be that value).
__global__ void __launch_bounds__(NG_THREADS) ng_sum_kernel(const double* __restrict__ codes, const double* __restrict__ fv, NgDims d, NgWs w) {
    __shared__ double tile[NG_TILE * NG_MMAX];
    __shared__ double red[3][NG_THREADS];
    const int tid = threadIdx.x, q = tid >> 5, c = tid & 31, m = d.m;
    size_t i0, i1;
    ng_slice(d, &i0, &i1);
    double s = 0.0, lo = INFINITY, hi = -INFINITY;
    for (size_t r0 = i0; r0 < i1; r0 += NG_TILE) {
        const int nr = i1 - r0 < NG_TILE ? (int)(i1 - r0) : NG_TILE;
        __syncthreads();
        ng_load_tile(codes, fv, d, r0, nr, tile);
        __syncthreads();
        if (c < m)
            for (int r = q; r < nr; r += NG_THREADS / 32) {
                const double x = tile[r * m + c];
                s += x;
                lo = fmin(lo, x), hi = fmax(hi, x);
            }
    }
    red[0][tid] = s, red[1][tid] = lo, red[2][tid] = hi;
    __syncthreads();
    if (tid < m) {
        s = red[0][tid], lo = red[1][tid], hi = red[2][tid];
        for (int g = 1; g < NG_THREADS / 32; ++g) {
            s += red[0][g * 32 + tid];
            lo = fmin(lo, red[1][g * 32 + tid]), hi = fmax(hi, red[2][g * 32 + tid]);
        }
        const size_t o = (size_t)blockIdx.x * m + tid;
        w.psum[o] = s, w.pmin[o] = lo, w.pmax[o] = hi;
    }
}

// acc[e] = op over the slices b = 0 .. NS-1, ascending, of part[b][e], e < width <= NG_BUF: the partials come through LDS in chunks of
// NG_BUF / width slices, loaded by every thread at once, because a thread that walks the slices in global memory waits out one
// load's latency per slice.  OP 0: sum, 1: min, 2: max.  buf: NG_BUF doubles of LDS; acc: LDS, valid after the call in every thread.
#define NG_BUF (NG_TILE * NG_MMAX)
template <int OP>
__device__ __forceinline__ void ng_reduce_slices(const double* __restrict__ part, int NS, int width, double* buf, double* acc) {
    const int chunk = NG_BUF / width;
    for (int e = threadIdx.x; e < width; e += NG_THREADS) acc[e] = OP == 0 ? 0.0 : (OP == 1 ? INFINITY : -INFINITY);
    for (int b0 = 0; b0 < NS; b0 += chunk) {
        const int nb = NS - b0 < chunk ? NS - b0 : chunk;
        __syncthreads();
        for (int e = threadIdx.x; e < nb * width; e += NG_THREADS) buf[e] = part[(size_t)b0 * width + e];
        __syncthreads();
        for (int e = threadIdx.x; e < width; e += NG_THREADS) {
            double v = acc[e];
            for (int b = 0; b < nb; ++b) {
                const double x = buf[b * width + e];
                v = OP == 0 ? v + x : (OP == 1 ? fmin(v, x) : fmax(v, x));
            }
            acc[e] = v;
        }
    }
    __syncthreads();
}

// ---- pass 2: per slice the centred cross products sum_r (x_ra - mean_a)(x_rb - mean_b), the full m x m matrix -----------------------
// The tile is centred in LDS.  Entry e = a m + b sits in slot e % nslot; the 256 / nslot row groups take rows q, q + Q, ... of each
// tile and are added in ascending order.  x y and y x are the same product, so the matrix is symmetric bit for bit.
__global__ void __launch_bounds__(NG_THREADS) ng_cross_kernel(const double* __restrict__ codes, const double* __restrict__ fv, NgDims d, NgWs w,
                                                              double* __restrict__ mean_out) {
    __shared__ double tile[NG_TILE * NG_MMAX];
    __shared__ double mean[NG_MMAX];
    __shared__ double part[NG_MMAX * NG_MMAX];
    const int tid = threadIdx.x, m = d.m, mm = m * m;
    ng_reduce_slices<0>(w.psum, d.NS, m, tile, mean);          // every workgroup forms the same bits
    if (tid < m) {
        mean[tid] = mean[tid] / (double)d.n;
        if (blockIdx.x == 0) mean_out[tid] = mean[tid];
    }
    const int nslot = mm <= 64 ? 64 : (mm <= 128 ? 128 : NG_THREADS);
    const int Q = NG_THREADS / nslot, q = tid / nslot, slot = tid - q * nslot;
    constexpr int PER = NG_MMAX * NG_MMAX / NG_THREADS;        // entries per thread at most
    double acc[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) acc[u] = 0.0;
    size_t i0, i1;
    ng_slice(d, &i0, &i1);
    for (size_t r0 = i0; r0 < i1; r0 += NG_TILE) {
        const int nr = i1 - r0 < NG_TILE ? (int)(i1 - r0) : NG_TILE;
        __syncthreads();
        ng_load_tile(codes, fv, d, r0, nr, tile);
        __syncthreads();
        for (int e = tid; e < nr * m; e += NG_THREADS) tile[e] -= mean[e % m];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = slot + u * nslot;
            if (e < mm) {
                const int a = e / m, b = e - a * m;
                double s = acc[u];
                for (int r = q; r < nr; r += Q) s = fma(tile[r * m + a], tile[r * m + b], s);
                acc[u] = s;
            }
        }
    }
    double* out = w.pcross + (size_t)blockIdx.x * mm;
    for (int g = 0; g < Q; ++g) {                              // group 0 stores, the others add in ascending order
        __syncthreads();
        if (q == g) {
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int e = slot + u * nslot;
                if (e < mm) part[e] = g == 0 ? acc[u] : part[e] + acc[u];
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < mm; e += NG_THREADS) out[e] = part[e];
}

// ---- finish: slices ascending, std = sqrt(sum (x - mean)^2 / n) (np.std's two passes, ddof = 0), G, the status word ----------------
__global__ void __launch_bounds__(NG_THREADS) ng_finish_kernel(NgDims d, NgWs w, double* __restrict__ mean_out, double* __restrict__ std_out,
                                                               double* __restrict__ G, int* __restrict__ status) {
    __shared__ double buf[NG_BUF];
    __shared__ double C[NG_MMAX * NG_MMAX];
    __shared__ double sum[NG_MMAX], mn[NG_MMAX], mx[NG_MMAX], sd[NG_MMAX];
    __shared__ int flag[NG_MMAX];
    const int tid = threadIdx.x, m = d.m, mm = m * m;
    ng_reduce_slices<0>(w.pcross, d.NS, mm, buf, C);
    ng_reduce_slices<0>(w.psum, d.NS, m, buf, sum);
    ng_reduce_slices<1>(w.pmin, d.NS, m, buf, mn);
    ng_reduce_slices<2>(w.pmax, d.NS, m, buf, mx);
    if (tid < m) {
        const double lo = mn[tid], hi = mx[tid], s = sum[tid];
        const double var = C[tid * m + tid] / (double)d.n;
        int f = 0;
        if (!(s - s == 0.0) || !(var - var == 0.0)) f = NG_NONFINITE;
        else if (lo == hi) f = NG_ZERO_VAR;
        if (f == NG_ZERO_VAR) {                                // the column's one value and no spread, whatever the sums rounded to
            mean_out[tid] = lo;
            sd[tid] = 0.0;
        } else sd[tid] = sqrt(var);
        std_out[tid] = sd[tid];
        flag[tid] = f;
    }
    __syncthreads();
    for (int e = tid; e < mm; e += NG_THREADS) {
        const int a = e / m, b = e - a * m;
        G[e] = C[e] / (sd[a] * sd[b]) / (double)d.n;           // a flagged column leaves IEEE's NaN / Inf here, next to the status word
    }
    if (tid == 0) {
        int all = 0, first = -1;
        for (int c = m - 1; c >= 0; --c)
            if (flag[c]) all |= flag[c], first = c;
        status[0] = all, status[1] = first;
    }
}

static int ng_check_shape(const char* who, int n, int k, int nf) {
    EG_REQUIRE(n >= 2, "%s: n = %d rows, a standard deviation needs at least 2", who, n);
    EG_REQUIRE(k >= 1 && nf >= 1 && k + nf <= NG_MMAX, "%s: k = %d code and nf = %d factor columns, 1 <= k, 1 <= nf, k + nf <= %d supported", who,
               k, nf, NG_MMAX);
    return 0;
}

extern "C" size_t eg_score_norm_gram_ws_bytes(int n, int k, int nf) {
    if (n < 2 || k < 1 || nf < 1 || k + nf > NG_MMAX) return 0;
    return ng_layout(ng_dims(n, k, nf), nullptr, nullptr);
}

extern "C" int eg_score_norm_gram(const double* codes, const double* fv, int n, int k, int nf, void* ws, double* mean, double* stddev, double* G,
                                  int* status, eg_stream_t s) {
    EG_REQUIRE(codes && fv && ws && mean && stddev && G && status, "eg_score_norm_gram: bad argument");
    if (ng_check_shape("eg_score_norm_gram", n, k, nf)) return -1;
    const NgDims d = ng_dims(n, k, nf);
    NgWs w;
    ng_layout(d, ws, &w);
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(ng_sum_kernel, dim3(d.NS), dim3(NG_THREADS), 0, st, codes, fv, d, w);
    hipLaunchKernelGGL(ng_cross_kernel, dim3(d.NS), dim3(NG_THREADS), 0, st, codes, fv, d, w, mean);
    hipLaunchKernelGGL(ng_finish_kernel, dim3(1), dim3(NG_THREADS), 0, st, d, w, mean, stddev, G, status);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- Lasso on the Gram matrix -------------------------------------------------------------------------------------------------------------
// Target j of G [(k+nf)][(k+nf)]: A = G[:k, :k], c = G[:k, k + j], minimise  f(w) = (G_yy - 2 c.w + w.A w) / 2 + alpha |w|_1  with
// G_yy = G[k+j][k+j] -- sklearn's (1 / 2n) |y - X w|^2 + alpha |w|_1 on the normalised columns, whose intercept is zero.  Cyclic
// coordinate descent from w = 0:  w_i <- soft(c_i - sum_{l != i} A_il w_l, alpha) / A_ii,  i = 0 .. k-1 per sweep; a step that changes
// w_i by delta takes A_li delta off every g_l.  Before the first sweep and after each one lane i forms g_i = c_i - (A w)_i afresh (l ascending) and the
// KKT residual  max_i ( w_i != 0 ? |g_i - alpha sign(w_i)| : max(|g_i| - alpha, 0) );  the fit stops when it is <= tol or after max_sweeps.
// One wave per target.
#define LS_KMAX 31
#define LS_LD 33               // LDS row stride of A: lanes read one column without a bank conflict

// lane l's value in every lane; l is uniform over the wave
__device__ __forceinline__ double ls_lane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

__global__ void __launch_bounds__(64) lasso_gram_fit_kernel(const double* __restrict__ G, int k, int nf, double alpha, int max_sweeps,
                                                            double tol, double* __restrict__ Wout, double* __restrict__ info) {
    __shared__ double A[LS_KMAX * LS_LD];
    const int lane = threadIdx.x, j = blockIdx.x, m = k + nf;
    const bool on = lane < k;
    for (int e = lane; e < k * k; e += 64) {
        const int a = e / k, b = e - a * k;
        A[a * LS_LD + b] = G[(size_t)a * m + b];
    }
    __syncthreads();
    const double* arow = A + (on ? lane : 0) * LS_LD;          // A is symmetric: lane l's row is column l
    const double c = on ? G[(size_t)lane * m + k + j] : 0.0;
    const double diag = on ? arow[lane] : 1.0;
    double* wo = Wout + (size_t)j * k;
    double* io = info + (size_t)j * 4;
    const double gyy = G[(size_t)(k + j) * m + k + j];
    int bad = 0;                                               // 2: a non-finite entry, 3: a diagonal entry that is not positive
    if (on) {
        double t = c;
        for (int l = 0; l < k; ++l) t += arow[l];
        if (!(t - t == 0.0)) bad = 2;
        else if (!(diag > 0.0)) bad = 3;
    }
    if (!(gyy - gyy == 0.0)) bad = 2;
    const int any2 = __any(bad == 2), any3 = __any(bad == 3);
    if (any2 || any3) {
        if (on) wo[lane] = 0.0;
        if (lane == 0) io[0] = 0.0, io[1] = INFINITY, io[2] = INFINITY, io[3] = any2 ? 2.0 : 3.0;
        return;
    }
    // Lane l holds w_l and g_l = c_l - (A w)_l in registers; what a coordinate step needs of another lane comes through readlane, not
    // LDS.  1 / A_ii is formed once: the last bit of the quotient is not what the stopping test measures.
    const double inv = 1.0 / diag;
    double w = 0.0, g = 0.0, kkt = INFINITY;
    int sweeps = 0, status = 1;
    for (;;) {
        g = c;                                                 // afresh after every sweep: the updates below do not accumulate rounding
        for (int l = 0; l < k; ++l) g = fma(-(on ? arow[l] : 0.0), ls_lane(w, l), g);
        const double r = w > 0.0 ? fabs(g - alpha) : (w < 0.0 ? fabs(g + alpha) : fmax(fabs(g) - alpha, 0.0));
        bool finite = true;
        kkt = 0.0;
        for (int l = 0; l < k; ++l) {
            const double rl = ls_lane(r, l);
            finite = finite && rl - rl == 0.0;
            kkt = fmax(kkt, rl);
        }
        if (!finite) {
            kkt = NAN, status = 2;
            break;
        }
        if (kkt <= tol) {
            status = 0;
            break;
        }
        if (sweeps >= max_sweeps) break;                       // status 1
        for (int i = 0; i < k; ++i) {
            const double wi = ls_lane(w, i);
            const double rho = fma(ls_lane(diag, i), wi, ls_lane(g, i));       // c_i - sum_{l != i} A_il w_l
            const double sft = rho > alpha ? rho - alpha : (rho < -alpha ? rho + alpha : 0.0);
            const double wn = sft * ls_lane(inv, i);
            const double delta = wn - wi;
            g = fma(-(on ? arow[i] : 0.0), delta, g);
            if (lane == i) w = wn;
        }
        ++sweeps;
    }
    if (on) wo[lane] = w;
    double cw = 0.0, l1 = 0.0;                                 // w.A w = w.(c - g):  f = G_yy / 2 - w.(c + g) / 2 + alpha |w|_1
    for (int i = 0; i < k; ++i) cw = fma(ls_lane(w, i), ls_lane(c + g, i), cw), l1 += fabs(ls_lane(w, i));
    if (lane == 0) io[0] = (double)sweeps, io[1] = kkt, io[2] = 0.5 * gyy - 0.5 * cw + alpha * l1, io[3] = (double)status;
}

extern "C" int eg_score_lasso_gram_fit(const double* G, int k, int nf, double alpha, int max_sweeps, double tol, double* W, double* info,
                                       eg_stream_t s) {
    EG_REQUIRE(G && W && info && max_sweeps >= 0 && tol >= 0.0, "eg_score_lasso_gram_fit: bad argument");
    EG_REQUIRE(k >= 1 && nf >= 1 && k + nf <= NG_MMAX, "eg_score_lasso_gram_fit: k = %d code and nf = %d factor columns, 1 <= k, 1 <= nf, k + nf <= %d supported",
               k, nf, NG_MMAX);
    EG_REQUIRE(alpha >= 0.0, "eg_score_lasso_gram_fit: alpha must not be negative");
    hipLaunchKernelGGL(lasso_gram_fit_kernel, dim3(nf), dim3(64), 0, (hipStream_t)s, G, k, nf, alpha, max_sweeps, tol, W, info);
    EG_LAUNCH_CHECK();
    return 0;
}
