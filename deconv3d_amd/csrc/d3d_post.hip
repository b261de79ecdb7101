// Posterior moments on the device (d3d_post_*): running mean and sum of squared deviations of
// the chain's samples -- clean cube, LSF (x) FSF convolved cube, (a, c, w, F) map -- updated
// between sweeps without a host round trip.  gfx950 only.
#include "d3d_ctx.h"

namespace d3d {

struct PostArgs {
    int D, Dp, HL;
    long nspax;
    double n;               // number of this sample, counted from 1
    double flux_k;          // sqrt(2 pi) * sum_k ratio[k]: F = a w flux_k
    const double *params;   // (H,W,3) chain state
    const uint8_t *mask;
    const double *sim;      // the sample's convolved cube (SLOT_SIM)
    double *clean_mean, *clean_m2;  // NULL: that moment is off
    double *conv_mean, *conv_m2;
    double *map_mean, *map_m2;      // (H,W,4)
    LineShape line;
};

typedef double post_v2d __attribute__((ext_vector_type(2)));

template <bool NTV>
__device__ __forceinline__ double2 post_load(const double *p) {
    if constexpr (NTV) {
        const post_v2d t = __builtin_nontemporal_load(reinterpret_cast<const post_v2d *>(p));
        return make_double2(t.x, t.y);
    } else {
        return *reinterpret_cast<const double2 *>(p);
    }
}

template <bool NTV>
__device__ __forceinline__ void post_store(double *p, double2 v) {
    if constexpr (NTV) {
        post_v2d t;
        t.x = v.x;
        t.y = v.y;
        __builtin_nontemporal_store(t, reinterpret_cast<post_v2d *>(p));
    } else {
        *reinterpret_cast<double2 *>(p) = v;
    }
}

// Welford's update of (mean, M2) with sample m, the n-th: plain IEEE operations in this order
// (no contraction: the moments do not depend on what the compiler fuses).
__device__ __forceinline__ void welford(double &mean, double &m2, double m, double n) {
#pragma clang fp contract(off)
    const double delta = m - mean;
    mean += delta / n;
    m2 += delta * (m - mean);
}

template <bool NTV>
__device__ __forceinline__ void welford_pair(double *mean, double *m2, double2 m, double n) {
    double2 mu = post_load<NTV>(mean), s = post_load<NTV>(m2);
    welford(mu.x, s.x, m.x, n);
    welford(mu.y, s.y, m.y, n);
    post_store<NTV>(mean, mu);
    post_store<NTV>(m2, s);
}

// One wavefront per spaxel, lanes along z in double2 pairs, the spectrum in steps of 64 lanes
// (k_chi2_map's mapping: one form for every depth; the pad channel of an odd depth stays 0).
// The clean sample is k_lines' expression, so that the mean of one sample is d3d_build_clean's
// cube bit for bit; the convolved sample is read from SLOT_SIM.  Lane 0 updates the map.
// Streaming: reads and writes four cubes, reads a fifth -- 72 bytes per voxel.
template <bool MULTI, bool NTV>
static __global__ __launch_bounds__(256) void k_post_accum(PostArgs A) {
    const int lane = threadIdx.x & 63;
    const long sp = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sp >= A.nspax) return;
    const double a = A.params[sp * 3 + 0], c = A.params[sp * 3 + 1], w = A.params[sp * 3 + 2];
    const bool live = A.mask[sp] != 0;
    for (int zl = lane; zl < A.HL; zl += 64) {
        const long at = sp * A.Dp + 2 * zl;
        if (A.clean_mean) {
            const int z = 2 * zl;
            double2 m = make_double2(0.0, 0.0);
            if (live) {
                m.x = (z < A.D) ? a * unit_line<MULTI>(A.line, (double)z, c, w) : 0.0;
                m.y = (z + 1 < A.D) ? a * unit_line<MULTI>(A.line, (double)(z + 1), c, w) : 0.0;
            }
            welford_pair<NTV>(A.clean_mean + at, A.clean_m2 + at, m, A.n);
        }
        if (A.conv_mean)
            welford_pair<NTV>(A.conv_mean + at, A.conv_m2 + at, post_load<NTV>(A.sim + at), A.n);
    }
    if (lane == 0) {
        const double v[4] = {a, c, w, a * w * A.flux_k};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double mu = A.map_mean[sp * 4 + k], s = A.map_m2[sp * 4 + k];
            welford(mu, s, v[k], A.n);
            A.map_mean[sp * 4 + k] = mu;
            A.map_m2[sp * 4 + k] = s;
        }
    }
}

}  // namespace d3d

namespace d3dh {

template <bool MULTI, bool NTV>
static int launch_post_t(d3d_ctx *c, const d3d::PostArgs &A) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(d3d::k_post_accum<MULTI, NTV>), dim3((unsigned)((c->HW + 3) / 4)),
                       dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_post_accum(d3d_ctx *c) {
    d3d::PostArgs A;
    A.D = c->D;
    A.Dp = c->Dp;
    A.HL = c->HL;
    A.nspax = c->HW;
    A.n = (double)(c->post_n + 1);
    double ratios = 0.0;
    for (int k = 0; k < c->line.K; ++k) ratios += c->line.ratio[k];
    A.flux_k = std::sqrt(2.0 * M_PI) * ratios;
    A.params = c->params;
    A.mask = c->mask;
    A.sim = c->slot[D3D_SLOT_SIM];
    A.clean_mean = c->post_cube[0];
    A.clean_m2 = c->post_cube[1];
    A.conv_mean = c->post_cube[2];
    A.conv_m2 = c->post_cube[3];
    A.map_mean = c->post_map;
    A.map_m2 = c->post_map + (size_t)c->HW * 4;
    A.line = c->line;
    // MULTI only for K > 1, as every other line kernel
    if (c->line.K > 1)
        return c->post_nt ? launch_post_t<true, true>(c, A) : launch_post_t<true, false>(c, A);
    return c->post_nt ? launch_post_t<false, true>(c, A) : launch_post_t<false, false>(c, A);
}

}  // namespace d3dh
