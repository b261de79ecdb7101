// Pointwise predictive accuracy (d3d_pred_*): for every voxel v the log pointwise predictive density
// lppd_v = log mean_s p(y_v | theta_s) and the WAIC penalty p_v = var_s log p(y_v | theta_s) over the
// samples of the posterior moments.  log p = k_v + q_sv with k_v constant over the chain, so one
// streaming kernel between sweeps folds q alone into four accumulator cubes -- a running maximum M,
// S = sum exp(q - M), Welford's mean and M2 -- and k_v joins at extraction.
// gfx950 only.
#include "d3d_ctx.h"

// every floating-point operation below is the one written: tests/predictive_oracle.py restates the
// update and the extraction operation for operation (as k_robust_step in d3d_robust.hip)
#pragma clang fp contract(off)

namespace d3d {

struct PredArgs {
    long HW;
    int HL;
    double n;               // number of this sample, counted from 1 (extraction: the samples held)
    double nu, half;        // Student-t: degrees of freedom and (nu + 1) / 2
    double kc;              // extraction: the part of k_v that no voxel changes
    const double *err, *i0; // residual; base 1/variance (rescale_base)
    double *M, *S, *mean, *m2;
};

// q of one voxel: Gaussian -1/2 r^2 i0; Student-t (the weight integrated out) -(nu + 1)/2
// log1p(r^2 i0 / nu)
template <bool T>
__device__ __forceinline__ double pred_q(const PredArgs &A, double r, double i0) {
    const double x = (r * r) * i0;
    if constexpr (T) return -(A.half * log1p(x / A.nu));
    return -0.5 * x;
}

// One sample into one voxel's accumulators.  S never holds a term above 1: whichever of q and M is
// the smaller one is rescaled by exp(-|q - M|), so no order of good and bad samples overflows.
template <bool T>
__device__ __forceinline__ void pred_update(const PredArgs &A, double r, double i0, double &M, double &S,
                                            double &mean, double &m2) {
    if (i0 == 0.0) return;  // a voxel without information is not counted: its accumulators stay 0
    const double q = pred_q<T>(A, r, i0);
    if (A.n == 1.0) {
        M = q;
        S = 1.0;
    } else {
        const double d = q - M;
        const double e = exp(-fabs(d));
        S = (d <= 0.0) ? S + e : S * e + 1.0;
        M = (d <= 0.0) ? M : q;
    }
    welford(mean, m2, q, A.n);
}

// One wavefront per spaxel, lanes along z in double2 cells of the [HW][Dp] layout, the spectrum in
// steps of 64 lanes (k_post_accum's and k_robust_step's mapping: no index division).  Reads the
// residual and the base 1/variance (16 bytes per voxel, cached: the next sweep reads them again),
// reads and writes the four accumulators (32 + 32 bytes, NTV: past the caches) -- 80 bytes per voxel.
template <bool T, bool NTV>
static __global__ __launch_bounds__(256) void k_pred_accum(PredArgs A) {
    const int lane = threadIdx.x & 63;
    const long sp = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sp >= A.HW) return;
    for (int zl = lane; zl < A.HL; zl += 64) {
        const long at = (sp * A.HL + zl) * 2;
        const double2 r = *reinterpret_cast<const double2 *>(A.err + at);
        const double2 b = *reinterpret_cast<const double2 *>(A.i0 + at);
        double2 M = post_load<NTV>(A.M + at), S = post_load<NTV>(A.S + at);
        double2 mu = post_load<NTV>(A.mean + at), s2 = post_load<NTV>(A.m2 + at);
        pred_update<T>(A, r.x, b.x, M.x, S.x, mu.x, s2.x);
        pred_update<T>(A, r.y, b.y, M.y, S.y, mu.y, s2.y);
        post_store<NTV>(A.M + at, M);
        post_store<NTV>(A.S + at, S);
        post_store<NTV>(A.mean + at, mu);
        post_store<NTV>(A.m2 + at, s2);
    }
}

// lppd_v and p_v of a counted voxel from its accumulators; p is NaN below two samples
__device__ __forceinline__ void pred_point(const PredArgs &A, double i0, double M, double S, double m2, double &lp,
                                           double &p) {
    const double k = 0.5 * log(i0) + A.kc;
    lp = (k + M) + log(S / A.n);
    p = A.n < 2.0 ? __builtin_nan("") : m2 / (A.n - 1.0);
}

struct PredSums {
    double lp, p, cnt, sq;
};

__device__ __forceinline__ void pred_add(const PredArgs &A, PredSums &s, double i0, double M, double S, double m2) {
    if (i0 == 0.0) return;
    double lp, p;
    pred_point(A, i0, M, S, m2, lp, p);
    const double e = lp - p;
    s.lp = s.lp + lp;
    s.p = s.p + p;
    s.cnt = s.cnt + 1.0;
    s.sq = s.sq + e * e;
}

// One wavefront per spaxel: the counted voxels of its spectrum into out[sp][4] = {sum lppd_v, sum
// p_v, their number, sum (lppd_v - p_v)^2}.  A fixed order -- lane l takes the cells l, l + 64, ...,
// each cell's even channel first, then the 64 lanes fold by halves (32, 16, .. 1) -- so that the sums
// are the same bits on every run.
static __global__ __launch_bounds__(256) void k_pred_maps(PredArgs A, double *out) {
    const int lane = threadIdx.x & 63;
    const long sp = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sp >= A.HW) return;  // (a whole wavefront: the shuffles below see all 64 lanes)
    PredSums s = {0.0, 0.0, 0.0, 0.0};
    for (int zl = lane; zl < A.HL; zl += 64) {
        const long at = (sp * A.HL + zl) * 2;
        const double2 b = *reinterpret_cast<const double2 *>(A.i0 + at);
        const double2 M = *reinterpret_cast<const double2 *>(A.M + at);
        const double2 S = *reinterpret_cast<const double2 *>(A.S + at);
        const double2 s2 = *reinterpret_cast<const double2 *>(A.m2 + at);
        pred_add(A, s, b.x, M.x, S.x, s2.x);
        pred_add(A, s, b.y, M.y, S.y, s2.y);
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        s.lp = s.lp + __shfl_xor(s.lp, d);
        s.p = s.p + __shfl_xor(s.p, d);
        s.cnt = s.cnt + __shfl_xor(s.cnt, d);
        s.sq = s.sq + __shfl_xor(s.sq, d);
    }
    if (lane == 0) {
        out[sp * 4 + 0] = s.lp;
        out[sp * 4 + 1] = s.p;
        out[sp * 4 + 2] = s.cnt;
        out[sp * 4 + 3] = s.sq;
    }
}

// out = lppd_v (which 0) or p_v (1) in the device layout, NaN where the voxel is not counted: what
// d3d_pred_cubes hands out
static __global__ __launch_bounds__(256) void k_pred_view(PredArgs A, long n, int which, double *out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double b = A.i0[i];
    double lp = __builtin_nan(""), p = lp;
    if (b != 0.0) pred_point(A, b, A.M[i], A.S[i], A.m2[i], lp, p);
    out[i] = which == 0 ? lp : p;
}

}  // namespace d3d

namespace d3dh {

// the base 1/variance: SLOT_IVAR is d3d_set_data's cube whether or not it is uniform (the uniform
// fast path only skips reading it), and the weights' copy of it while they rewrite the slot
static d3d::PredArgs pred_args(const d3d_ctx *c) {
    d3d::PredArgs A;
    A.HW = c->HW;
    A.HL = c->HL;
    A.n = (double)c->post.n;
    A.nu = (double)c->pred.nu;
    A.half = 0.5 * ((double)c->pred.nu + 1.0);
    // lgamma((nu + 1) / 2) - lgamma(nu / 2) - 1/2 log(nu pi), or -1/2 log(2 pi): on the host
    A.kc = c->pred.nu ? std::lgamma(A.half) - std::lgamma(0.5 * A.nu) - 0.5 * std::log(A.nu * M_PI)
                      : -0.5 * std::log(2.0 * M_PI);
    A.err = c->slot[D3D_SLOT_ERR];
    A.i0 = rescale_base(c);
    A.M = c->pred.cube[0];
    A.S = c->pred.cube[1];
    A.mean = c->pred.cube[2];
    A.m2 = c->pred.cube[3];
    return A;
}

template <bool T>
static int launch_pred_t(d3d_ctx *c, const d3d::PredArgs &A) {
    const dim3 grid((unsigned)((c->HW + 3) / 4));
    if (c->post_nt)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(d3d::k_pred_accum<T, true>), grid, dim3(256), 0, c->stream, A);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(d3d::k_pred_accum<T, false>), grid, dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pred_sample(d3d_ctx *c) {
    NEED(c->have_data && c->have_taps, D3D_ERR_STATE, "taps/data not set: the predictive density is the residual's");
    NEED((c->robust.on ? c->robust.nu : 0) == c->pred.nu, D3D_ERR_STATE,
         "the robust weights were armed, disarmed or given another nu after d3d_pred_begin: the samples of "
         "one predictive density share a likelihood (d3d_pred_begin again)");
    if (!c->err_valid)
        if (int rc = d3d_residual(c, nullptr)) return rc;
    if (int rc = flush_pending(c)) return rc;  // the residual is stored only every second colour
    d3d::PredArgs A = pred_args(c);
    A.n = (double)(c->post.n + 1);
    return c->pred.nu ? launch_pred_t<true>(c, A) : launch_pred_t<false>(c, A);
}

}  // namespace d3dh

using namespace d3dh;

extern "C" {

int d3d_pred_begin(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED,
         "predictive accuracy on a tile: the voxels of its frame belong to other ranks");
    NEED(c->post.on, D3D_ERR_STATE, "posterior moments not begun (d3d_post_begin)");
    NEED(!c->noise.on, D3D_ERR_UNSUPPORTED,
         "noise scales are armed (d3d_noise_begin): the density's normaliser 1/2 log i0 would change with every sample");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pred = {};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = c->pred.cube[k].alloc(c->cube_elems);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the context stays usable for the chain and the moments
        c->pred = {};
        return fail(D3D_ERR_HIP, "predictive accumulators (4 cubes of %zu bytes): %s", c->cube_elems * sizeof(double),
                    hipGetErrorString(e));
    }
    c->pred.on = true;
    c->pred.nu = c->robust.on ? c->robust.nu : 0;
    return post_reset(c);  // its samples are the moments', from the first one
}

int d3d_pred_count(d3d_ctx *c, int64_t *n) {
    NEED(c && n, D3D_ERR_INVALID, "NULL argument");
    *n = c->pred.on ? c->post.n : 0;
    return D3D_OK;
}

int d3d_pred_get(d3d_ctx *c, double *M, double *S, double *mean, double *m2) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->pred.on, D3D_ERR_STATE, "predictive accuracy not begun (d3d_pred_begin)");
    HIP_TRY(hipSetDevice(c->device));
    double *const out[4] = {M, S, mean, m2};
    for (int k = 0; k < 4; ++k)
        if (out[k])
            if (int rc = download_device_cube(c, c->pred.cube[k], out[k])) return rc;
    return D3D_OK;
}

int d3d_pred_maps(d3d_ctx *c, double *maps) {
    NEED(c && maps, D3D_ERR_INVALID, "NULL argument");
    NEED(c->pred.on, D3D_ERR_STATE, "predictive accuracy not begun (d3d_pred_begin)");
    NEED(c->have_data, D3D_ERR_STATE, "data not set");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<double> buf;  // [HW][4]
    HIP_TRY(buf.alloc((size_t)c->HW * 4));
    hipLaunchKernelGGL(d3d::k_pred_maps, dim3((unsigned)((c->HW + 3) / 4)), dim3(256), 0, c->stream, pred_args(c),
                       buf.get());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(maps, buf, (size_t)c->HW * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);  // (before buf goes)
    HIP_TRY(e);
    HIP_TRY(es);
    return D3D_OK;
}

int d3d_pred_cubes(d3d_ctx *c, double *lppd, double *p) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->pred.on, D3D_ERR_STATE, "predictive accuracy not begun (d3d_pred_begin)");
    NEED(c->have_data, D3D_ERR_STATE, "data not set");
    HIP_TRY(hipSetDevice(c->device));
    const unsigned grid = (unsigned)((c->cube_elems + 255) / 256);
    double *const scratch = c->slot[D3D_SLOT_TMP0];
    for (int k = 0; k < 2; ++k) {
        double *const out = k == 0 ? lppd : p;
        if (!out) continue;
        hipLaunchKernelGGL(d3d::k_pred_view, dim3(grid), dim3(256), 0, c->stream, pred_args(c), (long)c->cube_elems, k,
                           scratch);
        HIP_TRY(hipGetLastError());
        if (int rc = download_device_cube(c, scratch, out)) return rc;
    }
    return D3D_OK;
}

int d3d_pred_end(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pred = {};
    return D3D_OK;
}

}  // extern "C"
