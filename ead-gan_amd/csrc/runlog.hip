// Device loss log of a training run: one row of the iteration's losses appended to a ring in HBM by a launch that is part of the
// iteration (captured into its hipGraph), so that watching a run needs no host wait on the hot path.  Replaces the `.item()` calls of the
// reference's progress lines (celebA/EAD-GAN_celebA.py:404-408, MNIST/EAD-GAN_rpqmnxy.py:453-457, dSprites/rp.py:491-496,
// colored_dSprites/rp_color.py:523-528, dSprites/pxy.py:194-198, colored_dSprites/pxy_color.py:223-227).
// Roofline class: latency (one wave, a few dozen bytes); no LDS, a handful of VGPRs -- co-resident with anything.
#include "eg_common.h"

#define EG_RUNLOG_MAX_N 64

// one wave: lane j < n copies losses[j] into row head % capacity; lane 0 then advances head and latches the first non-finite iteration
__global__ void __launch_bounds__(64) runlog_append_kernel(const float* __restrict__ losses, int n, float* __restrict__ ring, int capacity,
                                                           int* __restrict__ head, int* __restrict__ first_nonfinite) {
    const int lane = threadIdx.x;
    const int h = head[0];                                  // every lane reads it before lane 0 writes it (the ballot below orders them)
    const int row = (int)((unsigned)h % (unsigned)capacity);
    bool bad = false;
    if (lane < n) {
        const float v = losses[lane];
        ring[(size_t)row * n + lane] = v;
        bad = (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;      // NaN or +-Inf: exponent all ones
    }
    const unsigned long long any_bad = __ballot(bad);
    if (lane == 0) {
        if (any_bad != 0ull && first_nonfinite[0] == 0) first_nonfinite[0] = h + 1;      // 1-based iteration, sticky
        head[0] = h + 1;
    }
}

extern "C" int eg_runlog_append(const float* losses, int n, float* ring, int capacity, int* head, int* first_nonfinite, eg_stream_t s) {
    EG_REQUIRE(losses && ring && head && first_nonfinite, "eg_runlog_append: null pointer");
    EG_REQUIRE(n > 0 && n <= EG_RUNLOG_MAX_N && capacity > 0, "eg_runlog_append: n must be in 1..64 and capacity positive");
    hipLaunchKernelGGL(runlog_append_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, losses, n, ring, capacity, head, first_nonfinite);
    EG_LAUNCH_CHECK();
    return 0;
}
