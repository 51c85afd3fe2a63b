// Convolution geometry shared by the host code of the implicit-GEMM translation units (igemm.hip, pack.hip, igemm_tn.hip, grad_reduce.hip):
// argument checks, output extents and the NT launch geometry of the forward and the backward-data pass, which the packed weight panels
// must follow tap for tap.  Host only.
#pragma once
#include "eg_common.h"
#include "igemm_nt.h"

// K extent of a packed weight panel row: K rounded up to the K tile.  (Skewing pitches that are multiples of 2 KiB by one extra tile
// was tried against L2 channel aliasing of the 128-byte column slices: no effect on MI355X.)
static inline int kpad_of(int K, int dtype) {
    return round_up(K > 0 ? K : 1, bk_of(dtype));
}

static inline int conv_out_dim(const eg_conv* c, int in) { return ((in << c->up) + 2 * c->pad - c->k) / c->stride + 1; }

enum { NEED_CIN = 1, NEED_COUT = 2 };
static inline int check_conv(const eg_conv* c, int dtype, int need) {
    EG_REQUIRE(c && c->B > 0 && c->k > 0 && c->stride > 0 && c->pad >= 0 && (c->up == 0 || c->up == 1), "eg_conv: bad field");
    EG_REQUIRE(dtype == EG_F32 || dtype == EG_BF16 || dtype == EG_F16, "dtype must be EG_F32, EG_BF16 or EG_F16");
    // zero channels pass every `% vec` test below, and the kernels' tap walks (`while (kc >= C) kc -= C`) never end on C == 0
    EG_REQUIRE(c->Cin > 0 && c->Cout > 0 && c->H > 0 && c->W > 0, "eg_conv: Cin, Cout, H and W must be positive (Cin=%d Cout=%d H=%d W=%d)",
               c->Cin, c->Cout, c->H, c->W);
    const int OH = conv_out_dim(c, c->H), OW = conv_out_dim(c, c->W);
    EG_REQUIRE(ilog2_exact(c->H) >= 0 && ilog2_exact(c->W) >= 0 && ilog2_exact(OH) >= 0 && ilog2_exact(OW) >= 0,
               "spatial extents must be powers of two (H=%d W=%d OH=%d OW=%d)", c->H, c->W, OH, OW);
    // the kernels index the B * OH * OW lattice rows with an int
    EG_REQUIRE((long long)c->B * OH * OW < (1LL << 31), "eg_conv: B * OH * OW must be below 2^31 (B=%d OH=%d OW=%d)", c->B, OH, OW);
    EG_REQUIRE((!(need & NEED_CIN) || c->Cin % vec_of(dtype) == 0) && (!(need & NEED_COUT) || c->Cout % vec_of(dtype) == 0),
               "gathered channel count must be a multiple of %d for this dtype (Cin=%d Cout=%d); pad the tensor", vec_of(dtype), c->Cin, c->Cout);
    return 0;
}

// forward: one phase, taps = k x k, source = X
static inline void geom_fwd(const eg_conv* c, int dtype, NtParams& p) {
    const int OH = conv_out_dim(c, c->H), OW = conv_out_dim(c, c->W);
    p.B = c->B; p.H = c->H; p.W = c->W; p.C = c->Cin;
    p.lOH = ilog2_exact(OH); p.lOW = ilog2_exact(OW);
    p.sy = p.sx = c->stride; p.up = c->up;
    p.N = c->Cout;
    p.DH = OH; p.DW = OW; p.osy = p.osx = 1;
    p.M = c->B * OH * OW;
    NtPhase& f = p.ph[0];
    f.TH = f.TW = c->k; f.dy0 = f.dx0 = -c->pad; f.dys = f.dxs = 1; f.ooy = f.oox = 0;
    f.K = c->k * c->k * c->Cin; f.Kpad = kpad_of(f.K, dtype); f.w_off = 0;
}

struct BwdAxis { int k0, T, d0; };   // first kernel index, tap count, source offset for tap 0 (then -1 per tap)
static inline BwdAxis bwd_axis(const eg_conv* c, int r) {
    BwdAxis a;
    a.k0 = (r + c->pad) % c->stride;
    a.T = a.k0 < c->k ? (c->k - a.k0 + c->stride - 1) / c->stride : 0;
    a.d0 = (r + c->pad - a.k0) / c->stride;
    return a;
}

// backward-data: stride*stride phases; source = dY (lattice == dY's grid), dst = dX interleaved
static inline int geom_bwd(const eg_conv* c, int dtype, NtParams& p, int* nphase) {
    const int OH = conv_out_dim(c, c->H), OW = conv_out_dim(c, c->W);
    const int s = c->stride;
    EG_REQUIRE(s == 1 || s == 2, "stride must be 1 or 2");
    // k < stride leaves sub-pixel phases without a tap (TH or TW == 0): the kernels divide by TW and walk taps until ty reaches TH
    EG_REQUIRE(c->k >= s, "backward-data needs k >= stride (k=%d s=%d)", c->k, s);
    const int XH = c->H << c->up, XW = c->W << c->up;   // dX is produced at the (upsampled) conv-input resolution
    EG_REQUIRE(XH % s == 0 && XW % s == 0 && XH / s == OH && XW / s == OW,
               "backward-data needs OH == H/stride (k=%d s=%d p=%d)", c->k, s, c->pad);
    p.B = c->B; p.H = OH; p.W = OW; p.C = c->Cout;
    p.lOH = ilog2_exact(OH); p.lOW = ilog2_exact(OW);
    p.sy = p.sx = 1; p.up = 0;
    p.N = c->Cin;
    p.DH = XH; p.DW = XW; p.osy = p.osx = s;
    p.M = c->B * OH * OW;
    long long off = 0;
    int n = 0;
    for (int ry = 0; ry < s; ++ry)
        for (int rx = 0; rx < s; ++rx) {
            const BwdAxis ay = bwd_axis(c, ry), ax = bwd_axis(c, rx);
            NtPhase& f = p.ph[n++];
            f.TH = ay.T; f.TW = ax.T; f.dy0 = ay.d0; f.dx0 = ax.d0; f.dys = f.dxs = -1; f.ooy = ry; f.oox = rx;
            f.K = ay.T * ax.T * c->Cout; f.Kpad = kpad_of(f.K, dtype); f.w_off = off;
            off += (long long)c->Cin * f.Kpad;
        }
    *nphase = n;
    return 0;
}
