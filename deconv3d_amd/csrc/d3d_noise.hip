// Noise-scale inference (d3d_noise_*): the likelihood's variance is s_g * variance_v for every voxel
// of a channel of group g, with s_g ~ InvGamma(shape a0, rate b0).  Given the residual the precision
// factors tau_g = 1 / s_g are independent Gamma(a0 + N_g / 2, rate b0 + Q_g / 2) variables, N_g the
// counted voxels of the group and Q_g = sum r^2 i0 over them; given the factors the model is the
// per-voxel-variance model the sweep kernels run.  Between sweeps one reduction (k_noise_sums, folded
// by k_noise_fold), one draw (k_noise_draw) and one streaming rewrite SLOT_IVAR = i0 * tau[z] (k_noise_apply) are the whole
// device side.  gfx950 only.
//
// The order of every sum is fixed, whatever the chip, the grid, the options and the padding of Dp:
//   1. stream j of NOISE_STREAMS = 1024 adds, per channel, the terms (r * r) * i0 of the counted voxels
//      of the spaxels j, j + 1024, j + 2048, ... one after the other, from 0;
//   2. the 1024 partials of a channel are added in index order, from 0;
//   3. the channels of a group are added in increasing z, from 0.
// tests/noise_oracle.py restates the three steps; the sums agree bit for bit.
#include "d3d_ctx.h"
#include "d3d_rng.h"

// every floating-point operation below is the one written: tests/noise_oracle.py restates the
// sums and the draw operation for operation (as k_robust_step in d3d_robust.hip)
#pragma clang fp contract(off)

namespace d3d {

// fourth Philox counter word of the scales' streams: the sweep's own blocks have 0 there
// (philox_pair) and the Student-t weights ROBUST_TAG, so none of them share a counter
constexpr uint32_t NOISE_TAG = 0x4E4F4953u;
constexpr int NOISE_S = d3dh::NOISE_STREAMS;
constexpr int NOISE_ATTEMPTS = 16;  // Marsaglia-Tsang attempts before the fall-back g = d

struct NoiseArgs {
    long HW;
    int HL, Dp, D, G;
    int nchunk;             // steps of 64 double2 cells along a spectrum: (HL + 63) / 64
    uint32_t sweep;         // the run's numbering
    uint32_t k0, k1;        // seed
    double shape, rate;     // a0, b0
    long row;               // row of the series this draw writes
    const double *err, *i0;
    const uint8_t *spaxels; // NULL: every spaxel
    const int *group;
    double *part_q;
    unsigned *part_n;
    double *chan, *tau, *tau_g, *series, *ivar;
};

// One wavefront per (stream j, step k of 64 cells along z): lanes run along z in double2 cells of the
// [HW][Dp] layout (k_robust_step's and k_pred_accum's mapping: 16-byte loads, no index division), the
// wavefront walks the spaxels j, j + S, ... of its stream in turn and every lane keeps the sums and
// counts of its two channels in registers.  Four spaxels' loads are issued before their terms are
// added, in the stream's order.  16 bytes per voxel read; [S][Dp] partials written, zeros included.
static __global__ __launch_bounds__(256) void k_noise_sums(NoiseArgs A) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long)NOISE_S * A.nchunk) return;
    const int j = (int)(w / A.nchunk);
    const int zl = (int)(w % A.nchunk) * 64 + lane;
    if (zl >= A.HL) return;
    double q0 = 0.0, q1 = 0.0;
    unsigned n0 = 0, n1 = 0;
    for (long sp = j; sp < A.HW; sp += 4L * NOISE_S) {
        double2 r[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long s = sp + (long)u * NOISE_S;
            const bool counted = s < A.HW && (!A.spaxels || A.spaxels[s]);
            r[u] = b[u] = make_double2(0.0, 0.0);
            if (counted) {
                const long at = (s * A.HL + zl) * 2;
                r[u] = *reinterpret_cast<const double2 *>(A.err + at);
                b[u] = *reinterpret_cast<const double2 *>(A.i0 + at);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (b[u].x != 0.0) {
                q0 = q0 + (r[u].x * r[u].x) * b[u].x;
                ++n0;
            }
            if (b[u].y != 0.0) {
                q1 = q1 + (r[u].y * r[u].y) * b[u].y;
                ++n1;
            }
        }
    }
    const long at = (long)j * A.Dp + 2 * zl;
    *reinterpret_cast<double2 *>(A.part_q + at) = make_double2(q0, q1);
    *reinterpret_cast<uint2 *>(A.part_n + at) = make_uint2(n0, n1);
}

// g ~ Gamma(alpha, 1), alpha >= 1, by Marsaglia and Tsang (2000): attempt t takes Philox block 2t for
// the Box-Muller pair (u1, u2) and block 2t + 1 (its first uniform) for u3.  No acceptance in
// NOISE_ATTEMPTS attempts gives g = d, the mode of d v: an attempt is rejected with probability below
// 0.05 for alpha >= 1, sixteen in a row below 1e-20.
__device__ __forceinline__ double noise_gamma(const NoiseArgs &A, uint32_t g_index, double alpha) {
    const double d = alpha - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    for (int t = 0; t < NOISE_ATTEMPTS; ++t) {
        uint32_t r[4];
        philox4x32_10(g_index, A.sweep, (uint32_t)(2 * t), NOISE_TAG, A.k0, A.k1, r);
        const double u1 = u64_to_unit(((uint64_t)r[1] << 32) | r[0]);
        const double u2 = u64_to_unit(((uint64_t)r[3] << 32) | r[2]);
        philox4x32_10(g_index, A.sweep, (uint32_t)(2 * t + 1), NOISE_TAG, A.k0, A.k1, r);
        const double u3 = u64_to_unit(((uint64_t)r[1] << 32) | r[0]);
        const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        if (log(u3) < 0.5 * x * x + d - d * v + d * log(v)) return d * v;
    }
    return d;
}

// One workgroup per channel: its 1024 partials in index order into chan[0][z] (the sum) and chan[1][z]
// (the count).  The workgroup fetches the partials into LDS in one round of loads; one thread then adds
// them in order.  (As the first step of k_noise_draw -- a thread per channel walking the 1024 partials
// in global memory, sixteen loads in flight -- the fold took 240 us at 128 channels, eight times the
// streaming kernel it follows: profiles/noise_time.txt.)
static __global__ __launch_bounds__(256) void k_noise_fold(NoiseArgs A) {
    __shared__ double sq[NOISE_S];
    __shared__ unsigned sn[NOISE_S];
    const int z = blockIdx.x;  // (the grid is Dp workgroups)
    for (int j = threadIdx.x; j < NOISE_S; j += 256) {
        sq[j] = A.part_q[(long)j * A.Dp + z];
        sn[j] = A.part_n[(long)j * A.Dp + z];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double q = 0.0;
    unsigned long long n = 0;
#pragma unroll 8
    for (int j = 0; j < NOISE_S; ++j) {
        q = q + sq[j];
        n += sn[j];
    }
    A.chan[z] = q;
    A.chan[A.Dp + z] = (double)n;
}

// One workgroup.  (1) every group's channels in increasing z: a thread per group, 256 groups at a time,
// the channels' sums, counts and labels passing through LDS in tiles of 256; (2) tau_g ~ Gamma(a0 +
// N_g / 2, rate b0 + Q_g / 2) -- a group of fewer than 2 counted voxels keeps tau = 1 and is reported as
// NaN, a rate of exactly 0 keeps the previous tau; the scale 1 / tau_g into the series' row; (3) tau[z]
// of every channel: its group's, 1 for group -1 and the pad channel.
static __global__ __launch_bounds__(256) void k_noise_draw(NoiseArgs A) {
    __shared__ double s_q[256], s_n[256];
    __shared__ int s_g[256];
    for (int gb = 0; gb < A.G; gb += 256) {
        const int g = gb + (int)threadIdx.x;
        double q = 0.0, n = 0.0;
        for (int z0 = 0; z0 < A.D; z0 += 256) {
            const int zt = z0 + (int)threadIdx.x;
            __syncthreads();  // (the tile before has been read)
            if (zt < A.D) {
                s_q[threadIdx.x] = A.chan[zt];
                s_n[threadIdx.x] = A.chan[A.Dp + zt];
                s_g[threadIdx.x] = A.group[zt];
            }
            __syncthreads();
            const int nz = min(256, A.D - z0);
            for (int k = 0; k < nz; ++k)
                if (s_g[k] == g) {
                    q = q + s_q[k];
                    n = n + s_n[k];
                }
        }
        if (g >= A.G) continue;
        double tau = A.tau_g[g];
        double scale = __builtin_nan("");
        if (n >= 2.0) {
            const double rate = A.rate + 0.5 * q;
            if (rate != 0.0) tau = noise_gamma(A, (uint32_t)g, A.shape + 0.5 * n) / rate;
            scale = 1.0 / tau;
        } else {
            tau = 1.0;
        }
        A.tau_g[g] = tau;
        A.tau_g[A.G + g] = n;
        A.tau_g[2 * A.G + g] = q;
        A.series[A.row * A.G + g] = scale;
    }
    __syncthreads();  // (tau_g: global memory written and read by this workgroup alone)
    for (int z = threadIdx.x; z < A.Dp; z += 256) {
        const int g = z < A.D ? A.group[z] : -1;
        A.tau[z] = g >= 0 ? A.tau_g[g] : 1.0;
    }
}

// One wavefront per spaxel, lanes along z in double2 cells, the spectrum in steps of 64 lanes
// (k_robust_step's mapping): SLOT_IVAR = i0 * tau[z], 0 where i0 == 0.  16 bytes per voxel.
static __global__ __launch_bounds__(256) void k_noise_apply(NoiseArgs A) {
    const int lane = threadIdx.x & 63;
    const long sp = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sp >= A.HW) return;
    for (int zl = lane; zl < A.HL; zl += 64) {
        const long at = (sp * A.HL + zl) * 2;
        const double2 b = *reinterpret_cast<const double2 *>(A.i0 + at);
        const double2 t = *reinterpret_cast<const double2 *>(A.tau + 2 * zl);
        double2 out;
        out.x = b.x == 0.0 ? 0.0 : b.x * t.x;
        out.y = b.y == 0.0 ? 0.0 : b.y * t.y;
        *reinterpret_cast<double2 *>(A.ivar + at) = out;
    }
}

}  // namespace d3d

namespace d3dh {

static void noise_args(const d3d_ctx *c, int64_t rs, d3d::NoiseArgs &A) {
    A.HW = c->HW;
    A.HL = c->HL;
    A.Dp = c->Dp;
    A.D = c->D;
    A.G = c->noise.G;
    A.nchunk = (c->HL + 63) / 64;
    A.sweep = (uint32_t)rs;
    A.k0 = (uint32_t)c->seed;
    A.k1 = (uint32_t)(c->seed >> 32);
    A.shape = c->noise.shape;
    A.rate = c->noise.rate;
    A.row = (long)c->noise.draws;
    A.err = c->slot[D3D_SLOT_ERR];
    A.i0 = rescale_base(c);
    A.spaxels = c->noise.has_spaxels ? c->noise.spaxels.get() : nullptr;
    A.group = c->noise.group;
    A.part_q = c->noise.part_q;
    A.part_n = c->noise.part_n;
    A.chan = c->noise.chan;
    A.tau = c->noise.tau;
    A.tau_g = c->noise.tau_g;
    A.series = c->noise.series;
    A.ivar = c->slot[D3D_SLOT_IVAR];
}

// four launches on the context's stream, nothing but device memory between them
int noise_draw(d3d_ctx *c, int64_t rs, hipEvent_t *ev) {
    NEED(c->noise.draws < c->noise.capacity, D3D_ERR_STATE,
         "the series of noise scales is full (%lld draws): d3d_noise_begin with a larger capacity",
         (long long)c->noise.capacity);
    if (int rc = flush_pending(c)) return rc;  // the residual is stored only every second colour
    d3d::NoiseArgs A;
    noise_args(c, rs, A);
    const unsigned waves = (unsigned)(d3d::NOISE_S * A.nchunk);
    if (ev) HIP_TRY(hipEventRecord(ev[0], c->stream));
    hipLaunchKernelGGL(d3d::k_noise_sums, dim3((waves + 3) / 4), dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    if (ev) HIP_TRY(hipEventRecord(ev[1], c->stream));
    hipLaunchKernelGGL(d3d::k_noise_fold, dim3((unsigned)c->Dp), dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(d3d::k_noise_draw, dim3(1), dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    if (ev) HIP_TRY(hipEventRecord(ev[2], c->stream));
    hipLaunchKernelGGL(d3d::k_noise_apply, dim3((unsigned)((c->HW + 3) / 4)), dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    if (ev) HIP_TRY(hipEventRecord(ev[3], c->stream));
    c->noise.sweeps.push_back(rs);
    ++c->noise.draws;
    return 0;
}

// the base cube back into the slot, the buffers freed (the caller has drained the stream)
static void noise_free(d3d_ctx *c) {
    rescale_disarm(c, d3d_ctx::Rescale::NOISE);
    c->noise = {};
}

}  // namespace d3dh

using namespace d3dh;

extern "C" {

int d3d_noise_begin(d3d_ctx *c, const int32_t *group, int G, const uint8_t *spaxels, double shape, double rate,
                    int every, int64_t start, int64_t capacity) {
    NEED(c && group, D3D_ERR_INVALID, "NULL argument");
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED,
         "noise scales on a tile: the sums of a channel run over the voxels of every rank");
    if (int rc = rescale_free_for(c, d3d_ctx::Rescale::NOISE)) return rc;
    NEED(!c->pred.on, D3D_ERR_UNSUPPORTED,
         "predictive accuracy is armed (d3d_pred_begin): its normaliser 1/2 log i0 would change with every "
         "sample; d3d_pred_end first");
    NEED(!ctx_is_tempered(c), D3D_ERR_UNSUPPORTED,
         "noise scales on a tempered context: a rung's variance / beta is not rescaled with them");
    NEED(G >= 1, D3D_ERR_INVALID, "G = %d: the number of groups is >= 1", G);
    for (int z = 0; z < c->D; ++z)
        NEED(group[z] >= -1 && group[z] < G, D3D_ERR_INVALID,
             "group[%d] = %d: a label is -1 (never rescaled) or in 0 .. %d", z, (int)group[z], G - 1);
    NEED(shape >= 0.0 && rate >= 0.0, D3D_ERR_INVALID,
         "shape = %g / rate = %g: the inverse-gamma prior's are >= 0 (0, 0: Jeffreys' 1/s)", shape, rate);
    NEED(every >= 1, D3D_ERR_INVALID, "every = %d: redraw after one sweep in how many (>= 1)", every);
    NEED(start >= 0, D3D_ERR_INVALID, "start = %lld is negative", (long long)start);
    NEED(capacity >= 1, D3D_ERR_INVALID, "capacity = %lld: rows of the series (>= 1)", (long long)capacity);
    NEED(c->have_data, D3D_ERR_STATE, "data not set: the base 1/variance is d3d_set_data's");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->noise = {};  // (armed already: rescale_arm first puts the base cube back)
    if (int rc = rescale_arm(c, d3d_ctx::Rescale::NOISE, every, start)) return rc;
    d3d_ctx::Noise &N = c->noise;
    const size_t Dp = (size_t)c->Dp, S = (size_t)NOISE_STREAMS;
    std::vector<double> one(std::max(Dp, (size_t)3 * G), 0.0);
    hipError_t e = N.group.alloc((size_t)c->D);
    if (e == hipSuccess && spaxels) e = N.spaxels.alloc((size_t)c->HW);
    if (e == hipSuccess) e = N.part_q.alloc(S * Dp);
    if (e == hipSuccess) e = N.part_n.alloc(S * Dp);
    if (e == hipSuccess) e = N.chan.alloc(2 * Dp);
    if (e == hipSuccess) e = N.tau.alloc(Dp);
    if (e == hipSuccess) e = N.tau_g.alloc((size_t)3 * G);
    if (e == hipSuccess) e = N.series.alloc((size_t)capacity * G);
    if (e == hipSuccess) e = hipMemcpyAsync(N.group, group, (size_t)c->D * sizeof(int), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && spaxels)
        e = hipMemcpyAsync(N.spaxels, spaxels, (size_t)c->HW, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (the host arrays are the caller's)
    // tau = 1 everywhere; tau_g = 1 | no voxels | no sum
    std::fill(one.begin(), one.begin() + Dp, 1.0);
    if (e == hipSuccess) e = hipMemcpy(N.tau, one.data(), Dp * sizeof(double), hipMemcpyHostToDevice);
    std::fill(one.begin(), one.end(), 0.0);
    std::fill(one.begin(), one.begin() + G, 1.0);
    if (e == hipSuccess) e = hipMemcpy(N.tau_g, one.data(), (size_t)3 * G * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the context stays usable for the chain of known variance
        noise_free(c);
        return fail(D3D_ERR_HIP, "noise scales (%d x %zu partials, %lld x %d scales): %s", NOISE_STREAMS, Dp,
                    (long long)capacity, G, hipGetErrorString(e));
    }
    N.on = true;
    N.has_spaxels = spaxels != nullptr;
    N.G = G;
    N.shape = shape;
    N.rate = rate;
    N.capacity = capacity;
    return D3D_OK;
}

int d3d_noise_step(d3d_ctx *c, int64_t sweep_number) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->noise.on, D3D_ERR_STATE, "noise scales not begun (d3d_noise_begin)");
    NEED(sweep_number >= 0, D3D_ERR_INVALID, "sweep_number = %lld is negative", (long long)sweep_number);
    NEED(c->have_taps && c->have_params && c->have_cfg, D3D_ERR_STATE,
         "taps/parameters/mh_config not set: the draw needs the residual and the seed");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->err_valid)
        if (int rc = d3d_residual(c, nullptr)) return rc;
    if (!c->noise_timing) {
        if (int rc = noise_draw(c, sweep_number)) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        return D3D_OK;
    }
    // option noise_timing: the device time of k_noise_sums, of k_noise_fold and k_noise_draw together and
    // of k_noise_apply (read-only options noise_sums_ns / noise_draw_ns / noise_apply_ns), by HIP events
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
    int rc = e == hipSuccess ? noise_draw(c, sweep_number, ev) : fail(D3D_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e));
    if (!rc) {
        e = hipStreamSynchronize(c->stream);
        for (int k = 0; k < 3 && e == hipSuccess; ++k) {
            float ms = 0.f;
            e = hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
            c->noise_ns[k] = (long)(ms * 1e6f);
        }
        if (e != hipSuccess) rc = fail(D3D_ERR_HIP, "timing the noise kernels: %s", hipGetErrorString(e));
    }
    for (int k = 0; k < 4; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    return rc;
}

int d3d_noise_count(d3d_ctx *c, int64_t *draws) {
    NEED(c && draws, D3D_ERR_INVALID, "NULL argument");
    NEED(c->noise.on, D3D_ERR_STATE, "noise scales not begun (d3d_noise_begin)");
    *draws = c->noise.draws;
    return D3D_OK;
}

int d3d_noise_get(d3d_ctx *c, double *series, int64_t *sweeps, double *voxels, double *last_sum, double *tau) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->noise.on, D3D_ERR_STATE, "noise scales not begun (d3d_noise_begin)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const d3d_ctx::Noise &N = c->noise;
    const size_t G = (size_t)N.G;
    if (series && N.draws > 0)
        HIP_TRY(hipMemcpy(series, N.series, (size_t)N.draws * G * sizeof(double), hipMemcpyDeviceToHost));
    if (sweeps) std::copy(N.sweeps.begin(), N.sweeps.end(), sweeps);
    if (voxels) HIP_TRY(hipMemcpy(voxels, N.tau_g + G, G * sizeof(double), hipMemcpyDeviceToHost));
    if (last_sum) HIP_TRY(hipMemcpy(last_sum, N.tau_g + 2 * G, G * sizeof(double), hipMemcpyDeviceToHost));
    if (tau) HIP_TRY(hipMemcpy(tau, N.tau, (size_t)c->D * sizeof(double), hipMemcpyDeviceToHost));
    return D3D_OK;
}

int d3d_noise_end(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    noise_free(c);
    return D3D_OK;
}

}  // extern "C"
