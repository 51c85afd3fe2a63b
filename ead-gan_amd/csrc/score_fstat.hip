// The logistic solver of the fitted scores and the explicitness half of F-stat (dSprites/score/F_score.py, BetVAE.py;
// colored_dSprites/score/ likewise) on the device.
//   eg_score_softmax_fit    the optimum of sklearn's LogisticRegression(C), K = 2 .. 64 classes, K (d + 1) <= 256: F-stat's fit on all
//                           code columns and the BetaVAE score's classifier
//   eg_score_softmax_proba  predict_proba at that optimum
//   eg_score_auc_ovr        exact one-vs-rest pair counts of roc_auc_score (Mann-Whitney form)
// The objective, K >= 3 (sklearn minimises f / n, the same point):
//   f(W) = sum_i [ logsumexp_k z_ik - z_i,y_i ] + inv_C / 2 * sum_{k, a < d} W_ka^2,   z_ik = sum_{a<d} W_ka x_ia + W_kd
// and for K = 2 the binomial form with one weight row, sum_i [ log(1 + exp(z_i)) - y_i z_i ] + inv_C / 2 * |w|^2.  Damped Newton from
// W = 0: s = -H^-1 g by Cholesky, then Armijo backtracking t = 1, 1/2, ... (SM_TRIALS trials at most) until
//   f(W + t s) <= f(W) + 1e-4 t g.s + n eps |f(W)|
// where the last term is the rounding bound of the row sum: once the decrease falls below what f resolves, the full Newton step is taken
// as it is.  The iteration stops when |g|inf <= gtol or after max_iter steps.  info[3]: 0 converged, 1 max_iter reached, 2 line search
// failed, 3 Hessian not positive definite, 4 a label outside 0..K-1, 5 non-finite gradient, 6 a class without a sample.
// All float64.  No float atomics, no hand-off between workgroups inside a launch: every row sum has one order (rows ascending inside a
// slice, slices ascending), so two calls give the same bits.
#include <math.h>

#include "eg_common.h"

#define SM_THREADS 256
#define SM_PMAX 256            // parameters K (d + 1) (K = 2: d + 1)
#define SM_KMAX 64
#define SM_SLICES 64           // row slices of the gradient / Hessian sums at most
#define SM_SLICE_ROWS 1024     // rows per slice at least (below SM_SLICES slices)
#define SM_TRIALS 40           // Armijo halvings of one Newton step at most
#define SM_EPS 2.220446049250313e-16

// The decision record of the Newton iteration: written by the kernels below in float64, read by the host after each trial only to choose
// the next launch.
struct SmState {
    double f;                  // objective at W
    double ft;                 // objective at the last trial point W + t s
    double gmax;               // |g|inf at W
    double gs;                 // g . s of the current Newton step
    double t;                  // step length of the current / next trial
    long long it;              // accepted Newton steps
    long long status;          // info[3] once action == SM_DONE
    long long action;          // what the host launches next
    long long trials;          // halvings of the current step
    long long init;            // 1 until the first evaluation (at W = 0) has been taken
};
enum { SM_DONE = 0, SM_NEWTON = 1, SM_TRIAL = 2, SM_GRAD = 3 };     // SM_GRAD: a trial was accepted, its gradient is due (device only)

struct SmDims {
    int n, d, K, Kw, D, P;     // Kw weight rows (K, or 1 in the binomial form), D = d + 1, P = Kw D
    int NS, RS;                // row slices, rows per slice
    int NB;                    // objective partials: workgroups of SM_THREADS rows
};

struct SmWs {
    SmState* st;
    int* counts;               // [SM_KMAX] samples per class, [SM_KMAX] = a label outside 0..K-1 was seen
    double *W, *s, *g;         // [SM_PMAX] each
    double* fpart;             // [NB]
    double* gpart;             // [NS][P]
    double* prob;              // [n][Kw]
    double* H;                 // [P][P], lower triangle used
    double* slab;              // [NS][P][P]
};

static SmDims sm_dims(int n, int d, int K) {
    SmDims m;
    m.n = n, m.d = d, m.K = K, m.Kw = K == 2 ? 1 : K, m.D = d + 1, m.P = m.Kw * m.D;
    m.NS = cdiv(n, SM_SLICE_ROWS) < SM_SLICES ? cdiv(n, SM_SLICE_ROWS) : SM_SLICES;
    m.RS = cdiv(n, m.NS);
    m.NB = cdiv(n, SM_THREADS);
    return m;
}

static size_t sm_layout(const SmDims& m, void* base, SmWs* w) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? (char*)base + off : nullptr;
        off += (bytes + 255) / 256 * 256;
        return p;
    };
    SmWs l;
    l.st = (SmState*)take(sizeof(SmState));
    l.counts = (int*)take((SM_KMAX + 1) * sizeof(int));
    l.W = (double*)take(SM_PMAX * sizeof(double));
    l.s = (double*)take(SM_PMAX * sizeof(double));
    l.g = (double*)take(SM_PMAX * sizeof(double));
    l.fpart = (double*)take((size_t)m.NB * sizeof(double));
    l.gpart = (double*)take((size_t)m.NS * m.P * sizeof(double));
    l.prob = (double*)take((size_t)m.n * m.Kw * sizeof(double));
    l.H = (double*)take((size_t)m.P * m.P * sizeof(double));
    l.slab = (double*)take((size_t)m.NS * m.P * m.P * sizeof(double));
    if (w) *w = l;
    return off;
}

// sum of one value per thread over a workgroup of SM_THREADS by a halving tree in LDS; every thread receives the total
__device__ __forceinline__ double sm_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = SM_THREADS / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// the trial point: one expression, so that every kernel forms the same bits
__device__ __forceinline__ double sm_trial_w(const double* W, const double* s, double t, int j) { return fma(t, s[j], W[j]); }

// ---- labels: counts per class, and whether a label lies outside 0..K-1 (integer atomics: order free) --------------------------------
__global__ void __launch_bounds__(SM_THREADS) sm_count_kernel(const int* __restrict__ y, int n, int K, int* counts) {
    const int i = blockIdx.x * SM_THREADS + threadIdx.x;
    if (i >= n) return;
    const int yi = y[i];
    if (yi < 0 || yi >= K) atomicOr(&counts[SM_KMAX], 1);
    else atomicAdd(&counts[yi], 1);
}

// W = 0, s = 0, the record; status 4 (a label outside 0..K-1) or 6 (a class without a sample) ends the fit before anything is indexed
// with a label
__global__ void __launch_bounds__(SM_THREADS) sm_init_kernel(SmWs w, int K) {
    const int tid = threadIdx.x;
    w.W[tid] = 0.0, w.s[tid] = 0.0, w.g[tid] = 0.0;
    if (tid == 0) {
        long long status = 1;
        if (w.counts[SM_KMAX]) status = 4;
        else
            for (int k = 0; k < K; ++k)
                if (w.counts[k] == 0) status = 6;
        SmState s;
        s.f = INFINITY, s.ft = INFINITY, s.gmax = INFINITY, s.gs = 0.0, s.t = 0.0;
        s.it = 0, s.status = status, s.action = status == 1 ? SM_TRIAL : SM_DONE, s.trials = 0, s.init = 1;
        *w.st = s;
    }
}

// ---- probabilities of one row at weights Wl (LDS) -> p [Kw] (global), and the row's loss -----------------------------------------------
// K >= 3: p = softmax(z), loss = logsumexp_k z_k - z_y.  K = 2: p[0] = sigmoid(z), loss = log(1 + exp(z)) - y z.
__device__ __forceinline__ double sm_row(const double* Wl, const double* __restrict__ x, int yi, int d, int K, double* p) {
    const int D = d + 1;
    if (K == 2) {
        double z = 0.0;
        for (int c = 0; c < d; ++c) z += Wl[c] * x[c];
        z += Wl[d];
        const double e = exp(-fabs(z));                        // in (0, 1]
        const double q = 1.0 / (1.0 + e);                      // sigmoid(|z|)
        p[0] = z >= 0.0 ? q : e * q;
        return fmax(z, 0.0) + log1p(e) - (yi == 1 ? z : 0.0);
    }
    double m = -INFINITY, zy = 0.0;
    for (int k = 0; k < K; ++k) {
        double a = 0.0;
        for (int c = 0; c < d; ++c) a += Wl[k * D + c] * x[c];
        a += Wl[k * D + d];
        p[k] = a;
        m = fmax(m, a);
        if (k == yi) zy = a;
    }
    double se = 0.0;
    for (int k = 0; k < K; ++k) {
        const double e = exp(p[k] - m);
        p[k] = e;
        se += e;
    }
    for (int k = 0; k < K; ++k) p[k] = p[k] / se;
    return log(se) - (zy - m);
}

// one trial: probabilities of every row at W + t s into prob, the objective's partial sum of this workgroup's rows into fpart
__global__ void __launch_bounds__(SM_THREADS) sm_eval_kernel(SmWs w, const double* __restrict__ X, const int* __restrict__ y, SmDims m) {
    __shared__ double Wl[SM_PMAX];
    __shared__ double red[SM_THREADS];
    if (w.st->action != SM_TRIAL) return;                      // the step could not be formed (status 3): nothing to try
    const double t = w.st->t;
    if (threadIdx.x < m.P) Wl[threadIdx.x] = sm_trial_w(w.W, w.s, t, threadIdx.x);
    __syncthreads();
    const int i = blockIdx.x * SM_THREADS + threadIdx.x;
    double loss = 0.0;
    if (i < m.n) loss = sm_row(Wl, X + (size_t)i * m.d, y[i], m.d, m.K, w.prob + (size_t)i * m.Kw);
    const double tot = sm_block_sum(loss, red);
    if (threadIdx.x == 0) w.fpart[blockIdx.x] = tot;
}

// gradient partials of row slice blockIdx.x at the probabilities of the accepted trial in prob: gpart[slice][k D + a] = sum_i (p_ik - [y_i = k]) x_ia
#define SM_GTILE 32
__global__ void __launch_bounds__(SM_THREADS) sm_grad_kernel(SmWs w, const double* __restrict__ X, const int* __restrict__ y, SmDims m) {
    __shared__ double pt[SM_GTILE * SM_KMAX];
    __shared__ double xt[SM_GTILE * (SM_PMAX / 2)];
    __shared__ int yt[SM_GTILE];
    if (w.st->action != SM_GRAD) return;                       // the trial was not accepted: its gradient is never used
    const int tid = threadIdx.x;
    const int D = m.D, d = m.d, Kw = m.Kw;
    const int i0 = blockIdx.x * m.RS, i1 = i0 + m.RS < m.n ? i0 + m.RS : m.n;
    const int k = tid / D, a = tid - k * D;
    const int cls = m.K == 2 ? 1 : k;                          // the class whose indicator this parameter's residual carries
    double acc = 0.0, comp = 0.0;                              // compensated (Kahan): a 1e3-scaled column's partial sums would otherwise
                                                               // carry n eps of their own size into a gradient that has to reach gtol
    for (int r0 = i0; r0 < i1; r0 += SM_GTILE) {
        const int nr = i1 - r0 < SM_GTILE ? i1 - r0 : SM_GTILE;
        __syncthreads();
        for (int e = tid; e < nr * Kw; e += SM_THREADS) pt[e] = w.prob[(size_t)r0 * Kw + e];
        for (int e = tid; e < nr * D; e += SM_THREADS) {
            const int r = e / D, c = e - r * D;
            xt[e] = c < d ? X[(size_t)(r0 + r) * d + c] : 1.0;
        }
        if (tid < nr) yt[tid] = y[r0 + tid];
        __syncthreads();
        if (tid < m.P)
            for (int r = 0; r < nr; ++r) {
                const double term = (pt[r * Kw + k] - (yt[r] == cls ? 1.0 : 0.0)) * xt[r * D + a] - comp;
                const double t = acc + term;
                comp = (t - acc) - term;
                acc = t;
            }
    }
    if (tid < m.P) w.gpart[(size_t)blockIdx.x * m.P + tid] = acc;
}

// The decision after a trial, one workgroup: f(W + t s) from the partials in a fixed order and Armijo's test with the constants and
// rounding slack of the file header.  A rejected trial halves t (or ends the fit with status 2); an accepted one becomes the new W and asks for
// its gradient (SM_GRAD), which sm_grad_kernel and sm_converge_kernel supply behind this launch.
__global__ void __launch_bounds__(SM_THREADS) sm_decide_kernel(SmWs w, SmDims m, double inv_C) {
    __shared__ double red[SM_THREADS];
    const int tid = threadIdx.x;
    SmState st = *w.st;
    if (st.action != SM_TRIAL) return;
    const bool coef = tid < m.P && (tid % m.D) < m.d;
    const double wt = tid < m.P ? sm_trial_w(w.W, w.s, st.t, tid) : 0.0;
    double part = 0.0;
    for (int b = tid; b < m.NB; b += SM_THREADS) part += w.fpart[b];
    const double rows = sm_block_sum(part, red);
    const double pen = sm_block_sum(coef ? wt * wt : 0.0, red);
    const double ft = rows + 0.5 * inv_C * pen;
    st.ft = ft;
    const double slack = (double)m.n * SM_EPS * fabs(st.f);
    if (!st.init && !(ft <= st.f + 1e-4 * st.t * st.gs + slack)) {
        st.trials += 1;
        st.t *= 0.5;
        if (st.trials >= SM_TRIALS) st.status = 2, st.action = SM_DONE;
        if (tid == 0) *w.st = st;
        return;
    }
    if (tid < m.P) w.W[tid] = wt;
    st.f = ft;
    if (!st.init) st.it += 1;
    st.init = 0, st.trials = 0, st.action = SM_GRAD;
    if (tid == 0) *w.st = st;
}

// The gradient at the accepted point (slices ascending, then the penalty), |g|inf and the stopping tests; one workgroup.
__global__ void __launch_bounds__(SM_THREADS) sm_converge_kernel(SmWs w, SmDims m, double inv_C, int max_iter, double gtol) {
    __shared__ double gl[SM_PMAX];
    const int tid = threadIdx.x;
    SmState st = *w.st;
    if (st.action != SM_GRAD) return;
    double g = 0.0;
    if (tid < m.P) {
        for (int s = 0; s < m.NS; ++s) g += w.gpart[(size_t)s * m.P + tid];
        if ((tid % m.D) < m.d) g += inv_C * w.W[tid];
        w.g[tid] = g;
    }
    gl[tid] = g;
    __syncthreads();
    double gmax = 0.0;
    bool finite = st.f - st.f == 0.0;
    for (int j = 0; j < m.P; ++j) {
        const double a = fabs(gl[j]);
        finite = finite && a - a == 0.0;
        gmax = fmax(gmax, a);
    }
    st.gmax = finite ? gmax : NAN;
    if (!finite) st.status = 5, st.action = SM_DONE;
    else if (gmax <= gtol) st.status = 0, st.action = SM_DONE;
    else if (st.it >= max_iter) st.status = 1, st.action = SM_DONE;
    else st.action = SM_NEWTON;
    if (tid == 0) *w.st = st;
}

// ---- Hessian: per row slice the partial slab of a 16 x 16 tile of H (tiles of the lower triangle) --------------------------------------
// H[(k,a)][(l,b)] = sum_i p_ik ([k = l] - p_il) x_ia x_ib; the binomial form has the one block p (1 - p).  blockIdx.x = tile, .y = slice.
#define SM_HT 16
#define SM_HROWS 64
__global__ void __launch_bounds__(SM_THREADS) sm_hess_kernel(SmWs w, const double* __restrict__ X, SmDims m) {
    __shared__ double pr[SM_HROWS * SM_HT], pc[SM_HROWS * SM_HT], xr[SM_HROWS * SM_HT], xc[SM_HROWS * SM_HT];
    if (w.st->action != SM_NEWTON) return;
    int tr = 0, tc = blockIdx.x;                               // tile index -> (tr, tc), tc <= tr
    while (tc > tr) tc -= tr + 1, ++tr;
    const int tid = threadIdx.x, ty = tid / SM_HT, tx = tid - ty * SM_HT;
    const int row = tr * SM_HT + ty, col = tc * SM_HT + tx;
    const int D = m.D, d = m.d, Kw = m.Kw, P = m.P;
    const bool same = row / D == col / D;
    const int i0 = blockIdx.y * m.RS, i1 = i0 + m.RS < m.n ? i0 + m.RS : m.n;
    double acc = 0.0;
    for (int r0 = i0; r0 < i1; r0 += SM_HROWS) {
        const int nr = i1 - r0 < SM_HROWS ? i1 - r0 : SM_HROWS;
        __syncthreads();
        for (int e = tid; e < nr * SM_HT; e += SM_THREADS) {
            const int r = e / SM_HT, q = e - r * SM_HT;
            const size_t i = (size_t)(r0 + r);
            const int hr = tr * SM_HT + q, hc = tc * SM_HT + q;
            if (hr < P) {
                const int k = hr / D, a = hr - k * D;
                pr[e] = w.prob[i * Kw + k];
                xr[e] = a < d ? X[i * d + a] : 1.0;
            } else pr[e] = 0.0, xr[e] = 0.0;
            if (hc < P) {
                const int l = hc / D, b = hc - l * D;
                pc[e] = w.prob[i * Kw + l];
                xc[e] = b < d ? X[i * d + b] : 1.0;
            } else pc[e] = 0.0, xc[e] = 0.0;
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const double pk = pr[r * SM_HT + ty], pl = pc[r * SM_HT + tx];
            const double wgt = same ? pk * (1.0 - pk) : -(pk * pl);
            acc += wgt * (xr[r * SM_HT + ty] * xc[r * SM_HT + tx]);
        }
    }
    if (row < P && col <= row) w.slab[((size_t)blockIdx.y * P + row) * P + col] = acc;
}

// H = slabs in ascending order + inv_C on the coefficient diagonal + (K >= 3) 1 / K on the intercept block: v v^T with v = 1 / sqrt(K) on
// each intercept, the one null direction (a constant added to every intercept), which the gradient is orthogonal to -- the step is the
// minimum-norm one and the intercepts stay zero-sum.  Lower triangle only.
__global__ void __launch_bounds__(SM_THREADS) sm_hess_reduce_kernel(SmWs w, SmDims m, double inv_C) {
    if (w.st->action != SM_NEWTON) return;
    const int P = m.P;
    const int e = blockIdx.x * SM_THREADS + threadIdx.x;
    if (e >= P * P) return;
    const int row = e / P, col = e - row * P;
    if (col > row) return;
    double h = 0.0;
    for (int s = 0; s < m.NS; ++s) h += w.slab[((size_t)s * P + row) * P + col];
    const int a = row % m.D, b = col % m.D;
    if (row == col && a < m.d) h += inv_C;
    if (m.K >= 3 && a == m.d && b == m.d) h += 1.0 / (double)m.K;
    w.H[(size_t)row * P + col] = h;
}

// Cholesky H = L L^T in place in global memory (lower triangle), s = -H^-1 g, the step's intercept mean (rounding only) taken out, g . s;
// one workgroup.  A pivot that is not positive ends the fit with status 3.
#define SM_CHOL_THREADS 1024
__global__ void __launch_bounds__(SM_CHOL_THREADS) sm_solve_kernel(SmWs w, SmDims m) {
    __shared__ double colj[SM_PMAX];
    __shared__ double sv[SM_PMAX];
    __shared__ double gl[SM_PMAX];
    if (w.st->action != SM_NEWTON) return;
    const int tid = threadIdx.x, P = m.P;
    const int ty = tid >> 5, tx = tid & 31;
    double* H = w.H;
    bool spd = true;
    for (int j = 0; j < P; ++j) {
        const double djj = H[(size_t)j * P + j];               // read by every thread before anyone writes column j: uniform
        if (!(djj > 0.0)) {
            spd = false;
            break;
        }
        const double ljj = sqrt(djj);
        __syncthreads();
        for (int i = j + tid; i < P; i += SM_CHOL_THREADS) {
            const double v = i == j ? ljj : H[(size_t)i * P + j] / ljj;
            H[(size_t)i * P + j] = v;
            colj[i] = v;
        }
        __syncthreads();
        for (int i = j + 1 + ty; i < P; i += SM_CHOL_THREADS / 32) {
            const double lij = colj[i];
            for (int c = j + 1 + tx; c <= i; c += 32) H[(size_t)i * P + c] -= lij * colj[c];
        }
        __syncthreads();
    }
    if (!spd) {
        if (tid == 0) w.st->status = 3, w.st->action = SM_DONE;
        return;
    }
    if (tid < P) gl[tid] = w.g[tid], sv[tid] = -gl[tid];
    __syncthreads();
    for (int j = 0; j < P; ++j) {                              // L u = -g
        const double uj = sv[j] / H[(size_t)j * P + j];
        __syncthreads();
        if (tid == j) sv[j] = uj;
        if (tid > j && tid < P) sv[tid] -= H[(size_t)tid * P + j] * uj;
        __syncthreads();
    }
    for (int j = P - 1; j >= 0; --j) {                         // L^T s = u
        const double sj = sv[j] / H[(size_t)j * P + j];
        __syncthreads();
        if (tid == j) sv[j] = sj;
        if (tid < j) sv[tid] -= H[(size_t)j * P + tid] * sj;
        __syncthreads();
    }
    if (m.K >= 3) {
        double sb = 0.0;
        for (int k = 0; k < m.K; ++k) sb += sv[k * m.D + m.d];
        sb /= (double)m.K;
        __syncthreads();
        if (tid < m.K) sv[tid * m.D + m.d] -= sb;
        __syncthreads();
    }
    if (tid < P) w.s[tid] = sv[tid];
    if (tid == 0) {
        double gs = 0.0;
        for (int j = 0; j < P; ++j) gs += gl[j] * sv[j];
        w.st->gs = gs, w.st->t = 1.0, w.st->trials = 0, w.st->action = SM_TRIAL;
    }
}

__global__ void __launch_bounds__(SM_THREADS) sm_finish_kernel(SmWs w, int P, double* Wout, double* info) {
    const int tid = threadIdx.x;
    if (tid < P) Wout[tid] = w.W[tid];
    if (tid == 0) info[0] = (double)w.st->it, info[1] = w.st->gmax, info[2] = w.st->f, info[3] = (double)w.st->status;
}

static int sm_check_shape(const char* who, int n, int d, int K) {
    EG_REQUIRE(n > 0 && d > 0, "%s: bad argument", who);
    EG_REQUIRE(K >= 2 && K <= SM_KMAX, "%s: K = %d classes, 2..%d supported", who, K, SM_KMAX);
    EG_REQUIRE((long long)K * (d + 1) <= SM_PMAX, "%s: K (d + 1) = %lld parameters exceed %d", who, (long long)K * (d + 1), SM_PMAX);
    return 0;
}

extern "C" size_t eg_score_softmax_ws_bytes(int n, int d, int K) {
    if (n <= 0 || d <= 0 || K < 2 || K > SM_KMAX || (long long)K * (d + 1) > SM_PMAX) return 0;
    return sm_layout(sm_dims(n, d, K), nullptr, nullptr);
}

extern "C" int eg_score_softmax_fit(const double* X, const int* y, int n, int d, int K, double inv_C, int max_iter, double gtol, void* ws,
                                    double* W, double* info, eg_stream_t s) {
    EG_REQUIRE(X && y && ws && W && info && max_iter >= 0 && gtol >= 0.0, "eg_score_softmax_fit: bad argument");
    if (sm_check_shape("eg_score_softmax_fit", n, d, K)) return -1;
    EG_REQUIRE(inv_C > 0.0, "eg_score_softmax_fit: inv_C must be positive (the penalty makes the Hessian definite)");
    hipStream_t st = (hipStream_t)s;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(st, &cap);
    if (e != hipSuccess) EG_FAIL((int)e, "eg_score_softmax_fit: %s", hipGetErrorString(e));
    EG_REQUIRE(cap == hipStreamCaptureStatusNone, "eg_score_softmax_fit: the stream is capturing; this entry point blocks on the device "
                                                  "between launches and cannot be recorded into a graph");
    const SmDims m = sm_dims(n, d, K);
    SmWs w;
    sm_layout(m, ws, &w);
    e = hipMemsetAsync(w.counts, 0, (SM_KMAX + 1) * sizeof(int), st);
    if (e != hipSuccess) EG_FAIL((int)e, "eg_score_softmax_fit: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(sm_count_kernel, dim3(cdiv(n, SM_THREADS)), dim3(SM_THREADS), 0, st, y, n, K, w.counts);
    hipLaunchKernelGGL(sm_init_kernel, dim3(1), dim3(SM_THREADS), 0, st, w, K);
    EG_LAUNCH_CHECK();
    const int nt = cdiv(m.P, SM_HT), ntile = nt * (nt + 1) / 2;
    // every trial costs one read of the record; the count of trials is bounded by the iteration's own limits
    const long long max_trials = ((long long)max_iter + 1) * SM_TRIALS + 1;
    SmState rec;
    for (long long trial = 0; trial < max_trials; ++trial) {
        hipLaunchKernelGGL(sm_eval_kernel, dim3(m.NB), dim3(SM_THREADS), 0, st, w, X, y, m);
        hipLaunchKernelGGL(sm_decide_kernel, dim3(1), dim3(SM_THREADS), 0, st, w, m, inv_C);
        hipLaunchKernelGGL(sm_grad_kernel, dim3(m.NS), dim3(SM_THREADS), 0, st, w, X, y, m);
        hipLaunchKernelGGL(sm_converge_kernel, dim3(1), dim3(SM_THREADS), 0, st, w, m, inv_C, max_iter, gtol);
        EG_LAUNCH_CHECK();
        e = hipMemcpyAsync(&rec, w.st, sizeof(SmState), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) EG_FAIL((int)e, "eg_score_softmax_fit: %s", hipGetErrorString(e));
        if (rec.action == SM_DONE) break;
        if (rec.action == SM_NEWTON) {
            hipLaunchKernelGGL(sm_hess_kernel, dim3(ntile, m.NS), dim3(SM_THREADS), 0, st, w, X, m);
            hipLaunchKernelGGL(sm_hess_reduce_kernel, dim3(cdiv(m.P * m.P, SM_THREADS)), dim3(SM_THREADS), 0, st, w, m, inv_C);
            hipLaunchKernelGGL(sm_solve_kernel, dim3(1), dim3(SM_CHOL_THREADS), 0, st, w, m);
            EG_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(sm_finish_kernel, dim3(1), dim3(SM_THREADS), 0, st, w, m.P, W, info);
    EG_LAUNCH_CHECK();
    return 0;
}

// predict_proba at W: softmax of the logits [n][K], or [1 - p, p] with p = sigmoid(z) for K = 2 (W [1][d+1])
__global__ void __launch_bounds__(SM_THREADS) sm_proba_kernel(const double* __restrict__ X, int n, int d, int K, const double* __restrict__ W,
                                                              double* __restrict__ proba) {
    __shared__ double Wl[SM_PMAX];
    const int P = (K == 2 ? 1 : K) * (d + 1);
    if (threadIdx.x < P) Wl[threadIdx.x] = W[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * SM_THREADS + threadIdx.x;
    if (i >= n) return;
    double* p = proba + (size_t)i * K;
    sm_row(Wl, X + (size_t)i * d, 0, d, K, p);
    if (K == 2) {
        const double q = p[0];
        p[0] = 1.0 - q, p[1] = q;
    }
}

extern "C" int eg_score_softmax_proba(const double* X, int n, int d, int K, const double* W, double* proba, eg_stream_t s) {
    EG_REQUIRE(X && W && proba, "eg_score_softmax_proba: bad argument");
    if (sm_check_shape("eg_score_softmax_proba", n, d, K)) return -1;
    hipLaunchKernelGGL(sm_proba_kernel, dim3(cdiv(n, SM_THREADS)), dim3(SM_THREADS), 0, (hipStream_t)s, X, n, d, K, W, proba);
    EG_LAUNCH_CHECK();
    return 0;
}

// ---- one-vs-rest ROC AUC as exact pair counts ------------------------------------------------------------------------------------------
// order [n]: the rows grouped by class, offsets [K+1]: class k's rows are order[offsets[k] .. offsets[k+1]).  For class k, over all pairs
// (positive i, negative j): less[k] = #{s_jk < s_ik}, equal[k] = #{s_jk == s_ik}.  AUC_k = (2 less + equal) / (2 n_pos n_neg).
// Workgroup (x, y = class, z): AUC_PPT positives per thread in registers (chunk x of the class; the grid's x extent covers the largest
// class, whose row count the host passes as max_class_rows next to the offsets it built), the negatives of range z of the grouped
// order stream through LDS in tiles of AUC_THREADS; every lane reads the same LDS word (a broadcast).  A slot without a sample holds NaN,
// which is neither less than nor equal to anything.  Counts are integers: one 64-bit atomic add per workgroup and count.
#define AUC_THREADS 256
#define AUC_PPT 4
#define AUC_NEG 4096           // negatives per workgroup

__device__ __forceinline__ double auc_score(const double* __restrict__ sc, const int* __restrict__ order, int n, int K, int k, int pos) {
    const int row = order[pos];
    return (unsigned)row < (unsigned)n ? sc[(size_t)row * K + k] : NAN;
}

__global__ void __launch_bounds__(AUC_THREADS) auc_ovr_kernel(const double* __restrict__ sc, const int* __restrict__ order,
                                                              const int* __restrict__ offsets, int n, int K, unsigned long long* less,
                                                              unsigned long long* equal) {
    __shared__ double tile[AUC_THREADS];
    __shared__ unsigned long long red[2 * AUC_THREADS / 64];
    const int k = blockIdx.y, tid = threadIdx.x;
    int lo = offsets[k], hi = offsets[k + 1];
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < lo ? lo : (hi > n ? n : hi);
    const int p0 = lo + blockIdx.x * (AUC_THREADS * AUC_PPT);
    if (p0 >= hi) return;                                      // uniform: this class has no such chunk of positives
    double p[AUC_PPT];
#pragma unroll
    for (int r = 0; r < AUC_PPT; ++r) {
        const int pos = p0 + r * AUC_THREADS + tid;
        p[r] = pos < hi ? auc_score(sc, order, n, K, k, pos) : NAN;
    }
    unsigned cl[AUC_PPT], ce[AUC_PPT];
#pragma unroll
    for (int r = 0; r < AUC_PPT; ++r) cl[r] = 0, ce[r] = 0;
    const int q0 = blockIdx.z * AUC_NEG, q1 = q0 + AUC_NEG < n ? q0 + AUC_NEG : n;
    for (int t0 = q0; t0 < q1; t0 += AUC_THREADS) {
        const int pos = t0 + tid;
        __syncthreads();
        tile[tid] = pos < q1 && (pos < lo || pos >= hi) ? auc_score(sc, order, n, K, k, pos) : NAN;
        __syncthreads();
        for (int j = 0; j < AUC_THREADS; ++j) {
            const double v = tile[j];
#pragma unroll
            for (int r = 0; r < AUC_PPT; ++r) cl[r] += v < p[r] ? 1u : 0u, ce[r] += v == p[r] ? 1u : 0u;
        }
    }
    unsigned long long tl = 0, te = 0;
#pragma unroll
    for (int r = 0; r < AUC_PPT; ++r) tl += cl[r], te += ce[r];
    for (int o = 32; o > 0; o >>= 1) tl += __shfl_xor(tl, o), te += __shfl_xor(te, o);
    if ((tid & 63) == 0) red[2 * (tid >> 6)] = tl, red[2 * (tid >> 6) + 1] = te;
    __syncthreads();
    if (tid == 0) {
        tl = 0, te = 0;
        for (int wv = 0; wv < AUC_THREADS / 64; ++wv) tl += red[2 * wv], te += red[2 * wv + 1];
        if (tl) atomicAdd(less + k, tl);
        if (te) atomicAdd(equal + k, te);
    }
}

extern "C" int eg_score_auc_ovr(const double* scores, const int* order, const int* offsets, int n, int K, int max_class_rows,
                                unsigned long long* less, unsigned long long* equal, eg_stream_t s) {
    EG_REQUIRE(scores && order && offsets && less && equal && n > 0, "eg_score_auc_ovr: bad argument");
    EG_REQUIRE(max_class_rows >= 1 && max_class_rows <= n, "eg_score_auc_ovr: max_class_rows = %d outside 1..n", max_class_rows);
    EG_REQUIRE(K >= 1 && K <= 65535, "eg_score_auc_ovr: K = %d classes, 1..65535 supported", K);
    hipStream_t st = (hipStream_t)s;
    hipError_t e = hipMemsetAsync(less, 0, (size_t)K * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(equal, 0, (size_t)K * sizeof(unsigned long long), st);
    if (e != hipSuccess) EG_FAIL((int)e, "eg_score_auc_ovr: %s", hipGetErrorString(e));
    const int chunks = cdiv(max_class_rows, AUC_THREADS * AUC_PPT), ranges = cdiv(n, AUC_NEG);     // x: the largest class's positives
    EG_REQUIRE(ranges <= 65535, "eg_score_auc_ovr: n = %d rows exceed one launch", n);
    hipLaunchKernelGGL(auc_ovr_kernel, dim3(chunks, K, ranges), dim3(AUC_THREADS), 0, st, scores, order, offsets, n, K, less, equal);
    EG_LAUNCH_CHECK();
    return 0;
}
