// Posterior moments on the device (d3d_post_*): running mean and sum of squared deviations of
// the chain's samples -- clean cube, LSF (x) FSF convolved cube, (a, c, w, F) map -- updated
// between sweeps without a host round trip.  Posterior histograms (d3d_hist_*): per spaxel and per
// quantity of the map 64 equal bins over a range frozen from a pilot, filled between sweeps, and
// their quantile / mode / outside maps.  The lifecycle and the C entry points of both follow the
// kernels.  gfx950 only.
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

// ---- posterior histograms -----------------------------------------------
// A SERIES is one (spaxel, quantity) pair, i = spaxel * 4 + k, k over (a, c, w, F) as in the map.
constexpr int HIST_BINS = 64;  // one bin per lane of a wavefront (k_hist_quantiles)

struct HistArgs {
    long nser;              // HW * 4
    double pilot_m1;        // pilot - 1
    double span;
    double flux_k;
    double L[4], U[4];      // bounds of (a, c, w, F)
    const double *params;
    const uint8_t *mask;
    const double *map_mean, *map_m2;
    double *range;          // [nser][2]
    uint32_t *bins;         // [nser][64]
    uint32_t *tails;        // [nser][2]
};

// One thread per series: lo = max(mean - span sd, L), hi = min(mean + span sd, U) of the pilot's
// moments; a pilot that did not move (or moved to one side of a bound only) takes the whole of
// [L, U].  Masked spaxels keep NaN, which k_hist_accum never counts.  Plain IEEE operations in
// this order, as welford.
static __global__ __launch_bounds__(256) void k_hist_freeze(HistArgs A) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nser) return;
    const int k = (int)(i & 3);
    const double L = k == 0 ? A.L[0] : k == 1 ? A.L[1] : k == 2 ? A.L[2] : A.L[3];
    const double U = k == 0 ? A.U[0] : k == 1 ? A.U[1] : k == 2 ? A.U[2] : A.U[3];
    double lo = __builtin_nan(""), hi = __builtin_nan("");
    if (A.mask[i >> 2]) {
        const double mean = A.map_mean[i];
        const double sd = sqrt(A.map_m2[i] / A.pilot_m1);
        const double half = A.span * sd;
        lo = mean - half;
        hi = mean + half;
        lo = lo > L ? lo : L;
        hi = hi < U ? hi : U;
        if (!(sd > 0.0) || !(hi > lo)) {
            lo = L;
            hi = U;
        }
    }
    A.range[2 * i] = lo;
    A.range[2 * i + 1] = hi;
}

// One thread per series: the sample's bin, and a plain read-modify-write of that one counter -- the
// series is this thread's alone and the launches of a stream are ordered, so no atomics.  F is
// k_post_accum's expression.
static __global__ __launch_bounds__(256) void k_hist_accum(HistArgs A) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nser) return;
    const double lo = A.range[2 * i], hi = A.range[2 * i + 1];
    if (!(hi > lo)) return;  // masked (NaN), or bounds that coincide
    const long sp = i >> 2;
    const int k = (int)(i & 3);
    const double a = A.params[sp * 3 + 0], c = A.params[sp * 3 + 1], w = A.params[sp * 3 + 2];
    const double v = k == 0 ? a : k == 1 ? c : k == 2 ? w : a * w * A.flux_k;
    const double b = floor((v - lo) * ((double)HIST_BINS / (hi - lo)));
    uint32_t *p;
    if (b < 0.0)
        p = A.tails + 2 * i;
    else if (b >= (double)HIST_BINS)
        p = A.tails + 2 * i + 1;
    else if (b >= 0.0)
        p = A.bins + (size_t)HIST_BINS * i + (int)b;
    else
        return;  // a NaN sample is not counted
    *p += 1u;
}

struct HistQArgs {
    long nser;
    int n_q;
    double q[8];
    const double *range;
    const uint32_t *bins, *tails;
    double *quantiles, *mode, *outside;  // [nser][n_q], [nser], [nser]; NULL: not wanted
};

// One wavefront per series, lane = bin: the 64 counters in one coalesced 256-byte load, an
// inclusive scan by shuffles, the crossing bin of each quantile from the 64-bit ballot of
// "below + cum >= q n", the mode by a butterfly arg-max (ties to the lower bin).  Every value the
// branches test is the same in all lanes, so the shuffles inside them see the whole wavefront.
static __global__ __launch_bounds__(256) void k_hist_quantiles(HistQArgs A) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= A.nser) return;
    const uint32_t cnt = A.bins[(size_t)HIST_BINS * i + lane];
    uint32_t cum = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(cum, d);
        if (lane >= d) cum += up;
    }
    const uint32_t inside = __shfl(cum, 63);
    const uint64_t below = A.tails[2 * i], above = A.tails[2 * i + 1];
    const uint64_t n = below + inside + above;
    const double lo = A.range[2 * i], hi = A.range[2 * i + 1];
    const double width = (hi - lo) / (double)HIST_BINS;
    const double nan = __builtin_nan("");
    for (int j = 0; j < A.n_q; ++j) {
        double r = nan;
        if (n) {
            const double t = A.q[j] * (double)n;
            if (t <= (double)below) {
                r = lo;
            } else if (t > (double)(n - above)) {
                r = hi;
            } else {
                const unsigned long long crossed = __ballot((double)(below + cum) >= t);
                const int b = __ffsll(crossed) - 1;
                const uint32_t cum_b = __shfl(cum, b), cnt_b = __shfl(cnt, b);
                r = lo + ((double)b + (t - (double)(below + cum_b - cnt_b)) / (double)cnt_b) * width;
            }
        }
        if (A.quantiles && lane == j) A.quantiles[i * A.n_q + j] = r;
    }
    uint32_t best = cnt;
    int best_bin = lane;
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const uint32_t oc = __shfl_xor(best, d);
        const int ob = __shfl_xor(best_bin, d);
        if (oc > best || (oc == best && ob < best_bin)) {
            best = oc;
            best_bin = ob;
        }
    }
    if (lane == 0) {
        if (A.mode) A.mode[i] = inside ? lo + ((double)best_bin + 0.5) * width : nan;
        if (A.outside) A.outside[i] = n ? (double)(below + above) / (double)n : nan;
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

// F = a w flux_k
double flux_factor(const d3d_ctx *c) {
    double ratios = 0.0;
    for (int k = 0; k < c->line.K; ++k) ratios += c->line.ratio[k];
    if (c->line.tab) return c->line_tab_flux * ratios;  // (the table's own integral: d3d_set_line_table)
    return std::sqrt(2.0 * M_PI) * ratios;
}

int launch_post_accum(d3d_ctx *c) {
    d3d::PostArgs A;
    A.D = c->D;
    A.Dp = c->Dp;
    A.HL = c->HL;
    A.nspax = c->HW;
    A.n = (double)(c->post.n + 1);
    A.flux_k = flux_factor(c);
    A.params = c->params;
    A.mask = c->mask;
    A.sim = c->slot[D3D_SLOT_SIM];
    A.clean_mean = c->post.cube[0];
    A.clean_m2 = c->post.cube[1];
    A.conv_mean = c->post.cube[2];
    A.conv_m2 = c->post.cube[3];
    A.map_mean = c->post.map;
    A.map_m2 = c->post.map + (size_t)c->HW * 4;
    A.line = c->line;
    // MULTI only for K > 1 or a table, as every other line kernel
    if (d3d::line_multi(c->line))
        return c->post_nt ? launch_post_t<true, true>(c, A) : launch_post_t<true, false>(c, A);
    return c->post_nt ? launch_post_t<false, true>(c, A) : launch_post_t<false, false>(c, A);
}

static d3d::HistArgs hist_args(const d3d_ctx *c) {
    d3d::HistArgs A;
    A.nser = c->HW * 4;
    A.pilot_m1 = (double)(c->hist.pilot - 1);
    A.span = c->hist.span;
    A.flux_k = flux_factor(c);
    for (int k = 0; k < 3; ++k) {
        A.L[k] = c->min_b[k];
        A.U[k] = c->max_b[k];
    }
    A.L[3] = c->min_b[0] * c->min_b[2] * A.flux_k;
    A.U[3] = c->max_b[0] * c->max_b[2] * A.flux_k;
    A.params = c->params;
    A.mask = c->mask;
    A.map_mean = c->post.map;
    A.map_m2 = c->post.map + (size_t)c->HW * 4;
    A.range = c->hist.range;
    A.bins = c->hist.bins;
    A.tails = c->hist.tails;
    return A;
}

int launch_hist_freeze(d3d_ctx *c) {
    const d3d::HistArgs A = hist_args(c);
    hipLaunchKernelGGL(d3d::k_hist_freeze, dim3((unsigned)((A.nser + 255) / 256)), dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_hist_accum(d3d_ctx *c) {
    const d3d::HistArgs A = hist_args(c);
    hipLaunchKernelGGL(d3d::k_hist_accum, dim3((unsigned)((A.nser + 255) / 256)), dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_hist_quantiles(d3d_ctx *c, int n_q, const double *q, double *quantiles, double *mode, double *outside) {
    d3d::HistQArgs A;
    A.nser = c->HW * 4;
    A.n_q = n_q;
    for (int j = 0; j < 8; ++j) A.q[j] = j < n_q ? q[j] : 0.5;
    A.range = c->hist.range;
    A.bins = c->hist.bins;
    A.tails = c->hist.tails;
    A.quantiles = quantiles;
    A.mode = mode;
    A.outside = outside;
    hipLaunchKernelGGL(d3d::k_hist_quantiles, dim3((unsigned)((A.nser + 3) / 4)), dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- lifecycle: moments, with the histograms and regions that hang on them ---------------
// (the caller has drained the stream)
static void post_free(d3d_ctx *c) {
    c->hist = {};
    c->reg = {};
    c->pred = {};
    c->post = {};
}

// count 0, accumulators zero (Welford's first sample starts from mean = M2 = 0)
int post_reset(d3d_ctx *c) {
    if (!c->post.on) return 0;
    c->post.n = 0;
    for (double *p : c->post.cube)
        if (p) HIP_TRY(hipMemsetAsync(p, 0, c->cube_elems * sizeof(double), c->stream));
    HIP_TRY(hipMemsetAsync(c->post.map, 0, (size_t)c->HW * 8 * sizeof(double), c->stream));
    if (c->hist.on) {  // counters zero, ranges not frozen (all bits set: NaN)
        const size_t nser = (size_t)c->HW * 4;
        c->hist.frozen = false;
        HIP_TRY(hipMemsetAsync(c->hist.bins, 0, nser * 64 * sizeof(uint32_t), c->stream));
        HIP_TRY(hipMemsetAsync(c->hist.tails, 0, nser * 2 * sizeof(uint32_t), c->stream));
        HIP_TRY(hipMemsetAsync(c->hist.range, 0xff, nser * 2 * sizeof(double), c->stream));
    }
    if (c->reg.on) {  // series and spectra zero; the count is the moments'
        if (c->reg.series)
            HIP_TRY(hipMemsetAsync(c->reg.series, 0, (size_t)c->reg.rows * c->reg.K * 3 * sizeof(double), c->stream));
        if (c->reg.spec)
            HIP_TRY(hipMemsetAsync(c->reg.spec, 0, (size_t)2 * c->reg.K * c->Dp * sizeof(double), c->stream));
    }
    if (c->pred.on)  // the first sample overwrites M and S; Welford's starts from zero
        for (double *p : c->pred.cube) HIP_TRY(hipMemsetAsync(p, 0, c->cube_elems * sizeof(double), c->stream));
    return 0;
}

int post_sample(d3d_ctx *c) {
    NEED(c->post.on, D3D_ERR_STATE, "posterior moments not begun (d3d_post_begin)");
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED,
         "posterior moments on a tile: the parameters of its frame belong to other ranks");
    NEED(c->have_params, D3D_ERR_STATE, "parameters not set");
    if (c->post.what & 2) {
        NEED(c->have_taps, D3D_ERR_STATE, "taps not set");
        if (int rc = forward_into(c, c->slot[D3D_SLOT_SIM], false)) return rc;
    }
    if (int rc = launch_post_accum(c)) return rc;
    if (c->pred.on)  // d3d_pred_begin: the same sample, the same number
        if (int rc = pred_sample(c)) return rc;
    if (c->reg.on)  // d3d_region_begin: the same sample, the same number
        if (int rc = launch_region_sample(c)) return rc;
    ++c->post.n;
    if (c->hist.on) {  // d3d_hist_begin: the pilot's last sample freezes the ranges, later ones are binned
        if (c->post.n == c->hist.pilot) {
            if (int rc = launch_hist_freeze(c)) return rc;
            c->hist.frozen = true;
        } else if (c->hist.frozen) {
            if (int rc = launch_hist_accum(c)) return rc;
        }
    }
    return 0;
}

bool post_due(const d3d_ctx *c, int s) {
    return c->post.on && c->post.every > 0 && s >= c->post.first &&
           (s - c->post.first) % c->post.every == 0;
}

}  // namespace d3dh

using namespace d3dh;

extern "C" {

int d3d_post_begin(d3d_ctx *c, int what) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(what >= 0 && what <= 3, D3D_ERR_INVALID,
         "what = %d: bit 0 the clean cube, bit 1 the convolved cube (0..3)", what);
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED,
         "posterior moments on a tile: the parameters of its frame belong to other ranks");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    post_free(c);
    hipError_t e = c->post.map.alloc((size_t)c->HW * 8);
    for (int k = 0; k < 4 && e == hipSuccess; ++k)
        if (what & (1 << (k / 2))) e = c->post.cube[k].alloc(c->cube_elems);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the context stays usable for the chain
        post_free(c);
        return fail(D3D_ERR_HIP, "posterior accumulators (%d cubes of %zu bytes): %s",
                    2 * ((what & 1) + (what >> 1)), c->cube_elems * sizeof(double), hipGetErrorString(e));
    }
    c->post.on = true;
    c->post.what = what;
    return post_reset(c);
}

int d3d_post_schedule(d3d_ctx *c, int first_sweep, int every) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(first_sweep >= 0, D3D_ERR_INVALID, "first_sweep = %d is negative", first_sweep);
    NEED(every >= 1, D3D_ERR_INVALID, "every = %d: accumulate one sweep in how many (>= 1)", every);
    NEED(c->post.on, D3D_ERR_STATE, "posterior moments not begun (d3d_post_begin)");
    c->post.first = first_sweep;
    c->post.every = every;
    return D3D_OK;
}

int d3d_post_accumulate(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return post_sample(c);
}

int d3d_post_count(d3d_ctx *c, int64_t *n) {
    NEED(c && n, D3D_ERR_INVALID, "NULL argument");
    *n = c->post.on ? c->post.n : 0;
    return D3D_OK;
}

int d3d_post_get(d3d_ctx *c, int which, double *mean, double *m2) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(which >= 0 && which <= 2, D3D_ERR_INVALID,
         "which = %d: 0 the parameter map, 1 the clean cube, 2 the convolved cube", which);
    NEED(c->post.on, D3D_ERR_STATE, "posterior moments not begun (d3d_post_begin)");
    NEED(which == 0 || (c->post.what & which), D3D_ERR_STATE,
         "the %s cube's moments were not begun (d3d_post_begin what = %d)",
         which == 1 ? "clean" : "convolved", c->post.what);
    HIP_TRY(hipSetDevice(c->device));
    if (which == 0) {
        const size_t bytes = (size_t)c->HW * 4 * sizeof(double);
        if (mean) HIP_TRY(hipMemcpyAsync(mean, c->post.map, bytes, hipMemcpyDeviceToHost, c->stream));
        if (m2)
            HIP_TRY(hipMemcpyAsync(m2, c->post.map + (size_t)c->HW * 4, bytes, hipMemcpyDeviceToHost,
                                   c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return D3D_OK;
    }
    if (mean)
        if (int rc = download_device_cube(c, c->post.cube[2 * (which - 1)], mean)) return rc;
    if (m2)
        if (int rc = download_device_cube(c, c->post.cube[2 * (which - 1) + 1], m2)) return rc;
    return D3D_OK;
}

int d3d_post_end(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    post_free(c);
    return D3D_OK;
}

int d3d_hist_begin(d3d_ctx *c, int64_t pilot, double span) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(pilot >= 2, D3D_ERR_INVALID, "pilot = %lld: the range needs a standard deviation (>= 2 samples)",
         (long long)pilot);
    NEED(std::isfinite(span) && span > 0.0, D3D_ERR_INVALID, "span = %g is not a positive number", span);
    NEED(c->post.on, D3D_ERR_STATE, "posterior moments not begun (d3d_post_begin)");
    NEED(c->have_cfg, D3D_ERR_STATE, "bounds not set (d3d_mh_config)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->hist = {};
    const size_t nser = (size_t)c->HW * 4;
    hipError_t e = c->hist.bins.alloc(nser * 64);
    if (e == hipSuccess) e = c->hist.tails.alloc(nser * 2);
    if (e == hipSuccess) e = c->hist.range.alloc(nser * 2);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the context stays usable for the chain and the moments
        c->hist = {};
        return fail(D3D_ERR_HIP, "posterior histograms (%zu bytes): %s", nser * (66 * sizeof(uint32_t) + 16),
                    hipGetErrorString(e));
    }
    c->hist.on = true;
    c->hist.pilot = pilot;
    c->hist.span = span;
    return post_reset(c);  // the pilot is the moments' first samples
}

int d3d_hist_count(d3d_ctx *c, int64_t *n) {
    NEED(c && n, D3D_ERR_INVALID, "NULL argument");
    *n = c->hist.on ? std::max<int64_t>(c->post.n - c->hist.pilot, 0) : 0;
    return D3D_OK;
}

int d3d_hist_get(d3d_ctx *c, uint32_t *bins, uint32_t *tails, double *range) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->hist.on, D3D_ERR_STATE, "posterior histograms not begun (d3d_hist_begin)");
    HIP_TRY(hipSetDevice(c->device));
    const size_t nser = (size_t)c->HW * 4;
    if (bins)
        HIP_TRY(hipMemcpyAsync(bins, c->hist.bins, nser * 64 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (tails)
        HIP_TRY(hipMemcpyAsync(tails, c->hist.tails, nser * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (range)
        HIP_TRY(hipMemcpyAsync(range, c->hist.range, nser * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_hist_quantiles(d3d_ctx *c, int n_q, const double *q, double *quantiles, double *mode, double *outside) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(n_q >= 1 && n_q <= 8, D3D_ERR_INVALID, "n_q = %d: 1 to 8 quantiles a call", n_q);
    NEED(q, D3D_ERR_INVALID, "q is NULL");
    for (int j = 0; j < n_q; ++j)
        NEED(q[j] > 0.0 && q[j] < 1.0, D3D_ERR_INVALID, "q[%d] = %g lies outside (0, 1)", j, q[j]);
    NEED(c->hist.on, D3D_ERR_STATE, "posterior histograms not begun (d3d_hist_begin)");
    HIP_TRY(hipSetDevice(c->device));
    const size_t nser = (size_t)c->HW * 4;
    DevBuf<double> buf;  // quantiles [nser][n_q] | mode [nser] | outside [nser]
    HIP_TRY(buf.alloc(nser * (size_t)(n_q + 2)));
    double *d_mode = buf + nser * (size_t)n_q, *d_out = d_mode + nser;
    int rc = launch_hist_quantiles(c, n_q, q, quantiles ? buf.get() : nullptr, mode ? d_mode : nullptr,
                                   outside ? d_out : nullptr);
    hipError_t e = hipSuccess;
    if (!rc && quantiles)
        e = hipMemcpyAsync(quantiles, buf, nser * (size_t)n_q * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (!rc && e == hipSuccess && mode)
        e = hipMemcpyAsync(mode, d_mode, nser * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (!rc && e == hipSuccess && outside)
        e = hipMemcpyAsync(outside, d_out, nser * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);  // (before buf goes)
    if (rc) return rc;
    HIP_TRY(e);
    HIP_TRY(es);
    return D3D_OK;
}

int d3d_hist_end(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->hist = {};
    return D3D_OK;
}

}  // extern "C"
