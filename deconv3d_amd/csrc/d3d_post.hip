// Posterior moments on the device (d3d_post_*): running mean and sum of squared deviations of
// the chain's samples -- clean cube, LSF (x) FSF convolved cube, (a, c, w, F) map -- updated
// between sweeps without a host round trip.  Posterior histograms (d3d_hist_*): per spaxel and per
// quantity of the map 64 equal bins over a range frozen from a pilot, filled between sweeps, and
// their quantile / mode / outside maps.  gfx950 only.
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
    A.n = (double)(c->post_n + 1);
    A.flux_k = flux_factor(c);
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
    // MULTI only for K > 1 or a table, as every other line kernel
    if (d3d::line_multi(c->line))
        return c->post_nt ? launch_post_t<true, true>(c, A) : launch_post_t<true, false>(c, A);
    return c->post_nt ? launch_post_t<false, true>(c, A) : launch_post_t<false, false>(c, A);
}

static d3d::HistArgs hist_args(const d3d_ctx *c) {
    d3d::HistArgs A;
    A.nser = c->HW * 4;
    A.pilot_m1 = (double)(c->hist_pilot - 1);
    A.span = c->hist_span;
    A.flux_k = flux_factor(c);
    for (int k = 0; k < 3; ++k) {
        A.L[k] = c->min_b[k];
        A.U[k] = c->max_b[k];
    }
    A.L[3] = c->min_b[0] * c->min_b[2] * A.flux_k;
    A.U[3] = c->max_b[0] * c->max_b[2] * A.flux_k;
    A.params = c->params;
    A.mask = c->mask;
    A.map_mean = c->post_map;
    A.map_m2 = c->post_map + (size_t)c->HW * 4;
    A.range = c->hist_range;
    A.bins = c->hist_bins;
    A.tails = c->hist_tails;
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
    A.range = c->hist_range;
    A.bins = c->hist_bins;
    A.tails = c->hist_tails;
    A.quantiles = quantiles;
    A.mode = mode;
    A.outside = outside;
    hipLaunchKernelGGL(d3d::k_hist_quantiles, dim3((unsigned)((A.nser + 3) / 4)), dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace d3dh
