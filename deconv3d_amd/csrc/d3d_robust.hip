// Student-t likelihood (d3d_robust_*): a Student-t error with nu degrees of freedom is a Gaussian
// whose variance is divided by a latent weight lambda_v ~ Gamma(nu/2, rate nu/2) per voxel.  Given
// the weights the model is the per-voxel-variance model the sweep kernels run; given the residual
// the weights are independent Gamma((nu+1)/2, rate (nu + r^2 i0)/2) variables.  One streaming
// kernel between sweeps redraws them and rewrites SLOT_IVAR = lambda * i0 from the residual and
// the base 1/variance.  gfx950 only.
#include "d3d_ctx.h"
#include "d3d_rng.h"

// every floating-point operation below is the one written: tests/robust_oracle.py restates the
// draw operation for operation (as k_hist_* in d3d_post.hip)
#pragma clang fp contract(off)

namespace d3d {

// fourth Philox counter word of the weights' streams; the sweep's own blocks have 0 there
// (philox_pair), so the two never share a counter
constexpr uint32_t ROBUST_TAG = 0x52425354u;

struct RobustArgs {
    long HW;
    int HL;
    int nu, m, nblk;        // m = (nu + 1) / 2 uniforms in the product; Philox blocks per voxel
    int even;               // nu even: one Box-Muller pair after the product's uniforms
    uint32_t sweep;         // the run's numbering
    uint32_t k0, k1;        // seed
    double n;               // number of this draw in the running mean, counted from 1; 0: not accumulated
    const double *err, *i0;
    double *ivar, *mean;
};

// Gamma((nu + 1) / 2, 1) from a fixed number of uniforms: -log of a product of m of them, plus
// -log(u_a) cos^2(2 pi u_b) -- half the square of a Box-Muller normal, a Gamma(1/2) -- when nu is
// even.  Block b gives uniforms 2b and 2b + 1; the product takes uniforms 0 .. m-1, u_a = m,
// u_b = m + 1.  No rejection: the trip count is the launch's, not the voxel's.
__device__ __forceinline__ double robust_gamma(const RobustArgs &A, uint32_t voxel) {
    double prod = 1.0, ua = 0.5, ub = 0.25;
    for (int b = 0; b < A.nblk; ++b) {
        uint32_t r[4];
        philox4x32_10(voxel, A.sweep, (uint32_t)b, ROBUST_TAG, A.k0, A.k1, r);
        const double ux = u64_to_unit(((uint64_t)r[1] << 32) | r[0]);
        const double uy = u64_to_unit(((uint64_t)r[3] << 32) | r[2]);
        const int j = 2 * b;
        // (an odd m + 2 leaves the last block's second uniform unused)
        if (j < A.m) prod = prod * ux;
        else if (j == A.m) ua = ux;
        else if (j == A.m + 1) ub = ux;
        if (j + 1 < A.m) prod = prod * uy;
        else if (j + 1 == A.m) ua = uy;
        else if (j + 1 == A.m + 1) ub = uy;
    }
    double g = -log(prod);
    if (A.even) {
        const double t = cos(6.283185307179586 * ub);
        g = g + (-log(ua)) * (t * t);
    }
    return g;
}

__device__ __forceinline__ double robust_weight(const RobustArgs &A, uint32_t voxel, double r, double i0) {
    const double g = robust_gamma(A, voxel);
    return (2.0 * g) / ((double)A.nu + (r * r) * i0);
}

// One wavefront per spaxel, lanes along z in double2 cells of the [HW][Dp] layout (16-byte loads and
// stores), the spectrum in steps of 64 lanes (k_post_accum's mapping: no index division): reads the
// residual and the base 1/variance, writes 1/variance; ACC also reads and writes the running mean
// of the weights.  24 / 40 bytes per voxel.  A voxel without information (i0 == 0: NaN voxels, the
// pad channel of an odd depth) gets 0 and keeps a mean of 0.  voxel = z * HW + spaxel, the cube's
// own (D,H,W) order, so that a draw does not depend on the layout.
template <bool ACC>
static __global__ __launch_bounds__(256) void k_robust_step(RobustArgs A) {
    const int lane = threadIdx.x & 63;
    const long sp = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sp >= A.HW) return;
    const uint32_t hw = (uint32_t)A.HW;
    for (int zl = lane; zl < A.HL; zl += 64) {
        const long at = (sp * A.HL + zl) * 2;
        const double2 r = *reinterpret_cast<const double2 *>(A.err + at);
        const double2 b = *reinterpret_cast<const double2 *>(A.i0 + at);
        // (the pad channel's index may wrap: its draw is discarded, i0 == 0 there)
        const uint32_t v0 = (uint32_t)(2 * zl) * hw + (uint32_t)sp;
        const uint32_t v1 = v0 + hw;
        const double l0 = robust_weight(A, v0, r.x, b.x), l1 = robust_weight(A, v1, r.y, b.y);
        double2 out;
        out.x = b.x == 0.0 ? 0.0 : l0 * b.x;
        out.y = b.y == 0.0 ? 0.0 : l1 * b.y;
        *reinterpret_cast<double2 *>(A.ivar + at) = out;
        if constexpr (ACC) {
            double2 mu = *reinterpret_cast<const double2 *>(A.mean + at);
            if (b.x != 0.0) mu.x = mu.x + (l0 - mu.x) / A.n;
            if (b.y != 0.0) mu.y = mu.y + (l1 - mu.y) / A.n;
            *reinterpret_cast<double2 *>(A.mean + at) = mu;
        }
    }
}

// out = num / i0 (ratio) or num, NaN where i0 == 0: what d3d_robust_get hands out
static __global__ __launch_bounds__(256) void k_robust_view(long n, const double *num, const double *i0, int ratio,
                                                            double *out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double b = i0[i];
    out[i] = b == 0.0 ? __builtin_nan("") : (ratio ? num[i] / b : num[i]);
}

}  // namespace d3d

namespace d3dh {

int robust_draw(d3d_ctx *c, int64_t rs) {
    if (int rc = flush_pending(c)) return rc;  // the residual is stored only every second colour
    d3d::RobustArgs A;
    A.HW = c->HW;
    A.HL = c->HL;
    A.nu = c->robust.nu;
    A.m = (c->robust.nu + 1) / 2;
    A.even = (c->robust.nu & 1) ? 0 : 1;
    A.nblk = (A.m + (A.even ? 2 : 0) + 1) / 2;
    A.sweep = (uint32_t)rs;
    A.k0 = (uint32_t)c->seed;
    A.k1 = (uint32_t)(c->seed >> 32);
    const bool acc = rs >= c->robust.accum_from;
    A.n = acc ? (double)(c->robust.count + 1) : 0.0;
    A.err = c->slot[D3D_SLOT_ERR];
    A.i0 = rescale_base(c);
    A.ivar = c->slot[D3D_SLOT_IVAR];
    A.mean = c->robust.mean;
    const dim3 grid((unsigned)((c->HW + 3) / 4));
    if (acc)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(d3d::k_robust_step<true>), grid, dim3(256), 0, c->stream, A);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(d3d::k_robust_step<false>), grid, dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    if (acc) ++c->robust.count;
    return 0;
}

// the base cube back into the slot, the buffers freed (the caller has drained the stream)
static void robust_free(d3d_ctx *c) {
    rescale_disarm(c, d3d_ctx::Rescale::ROBUST);
    c->robust = {};
}

}  // namespace d3dh

using namespace d3dh;

extern "C" {

int d3d_robust_begin(d3d_ctx *c, int nu, int every, int64_t start, int64_t accumulate_from) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(nu >= 1 && nu <= 30, D3D_ERR_INVALID,
         "nu = %d: the degrees of freedom are an integer from 1 to 30 (the draw takes (nu + 1) / 2 uniforms)", nu);
    NEED(every >= 1, D3D_ERR_INVALID, "every = %d: redraw after one sweep in how many (>= 1)", every);
    NEED(start >= 0 && accumulate_from >= 0, D3D_ERR_INVALID, "start = %lld / accumulate_from = %lld is negative",
         (long long)start, (long long)accumulate_from);
    NEED(c->have_data, D3D_ERR_STATE, "data not set: the base 1/variance is d3d_set_data's");
    if (int rc = rescale_free_for(c, d3d_ctx::Rescale::ROBUST)) return rc;
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED,
         "robust weights on a tile: the voxels of its frame belong to other ranks");
    NEED((double)c->D * (double)c->HW < 4294967296.0, D3D_ERR_UNSUPPORTED,
         "robust weights key their random numbers by a 32-bit voxel index: D*H*W must be < 2^32");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->robust = {};  // (armed already: rescale_arm first puts the base cube back)
    if (int rc = rescale_arm(c, d3d_ctx::Rescale::ROBUST, every, start)) return rc;
    const size_t bytes = c->cube_elems * sizeof(double);
    hipError_t e = c->robust.mean.alloc(c->cube_elems);
    if (e == hipSuccess) e = hipMemsetAsync(c->robust.mean, 0, bytes, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the context stays usable for the Gaussian chain
        robust_free(c);
        return fail(D3D_ERR_HIP, "robust weights (a cube of %zu bytes): %s", bytes, hipGetErrorString(e));
    }
    c->robust.on = true;
    c->robust.nu = nu;
    c->robust.accum_from = accumulate_from;
    return D3D_OK;
}

int d3d_robust_step(d3d_ctx *c, int64_t sweep_number) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->robust.on, D3D_ERR_STATE, "robust weights not begun (d3d_robust_begin)");
    NEED(sweep_number >= 0, D3D_ERR_INVALID, "sweep_number = %lld is negative", (long long)sweep_number);
    NEED(c->have_taps && c->have_params && c->have_cfg, D3D_ERR_STATE,
         "taps/parameters/mh_config not set: the draw needs the residual and the seed");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->err_valid)
        if (int rc = d3d_residual(c, nullptr)) return rc;
    if (int rc = robust_draw(c, sweep_number)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_robust_get(d3d_ctx *c, double *weights, double *weight_mean, int64_t *count) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->robust.on, D3D_ERR_STATE, "robust weights not begun (d3d_robust_begin)");
    HIP_TRY(hipSetDevice(c->device));
    if (count) *count = c->robust.count;
    const unsigned grid = (unsigned)((c->cube_elems + 255) / 256);
    double *const scratch = c->slot[D3D_SLOT_TMP0];
    for (int k = 0; k < 2; ++k) {
        double *const out = k == 0 ? weights : weight_mean;
        if (!out) continue;
        hipLaunchKernelGGL(d3d::k_robust_view, dim3(grid), dim3(256), 0, c->stream, (long)c->cube_elems,
                           (const double *)(k == 0 ? c->slot[D3D_SLOT_IVAR] : c->robust.mean), rescale_base(c),
                           k == 0 ? 1 : 0, scratch);
        HIP_TRY(hipGetLastError());
        if (int rc = download_device_cube(c, scratch, out)) return rc;
    }
    return D3D_OK;
}

int d3d_robust_end(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    robust_free(c);
    return D3D_OK;
}

}  // extern "C"
