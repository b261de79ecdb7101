// Preparation of a raw cube on the device (d3d_running_median, d3d_channel_stats, d3d_prepare):
// a running median along every spectrum as the continuum, and the median / MAD of every channel
// plane of the residual as the channel noise.  Both are exact selections: the only arithmetic is
// one subtraction, one * 0.5 and one * 1.4826.  gfx950 only.
#include "d3d_ctx.h"

namespace d3d {

constexpr int PREP_NT = 256;       // threads of a running-median workgroup
constexpr int PREP_CB = 4;         // candidates a thread ranks per pass over its window
constexpr int PREP_LDS = 48 * 1024;  // spectra of a running-median workgroup (one spectrum may take more)
constexpr int PREP_SPEC_MAX = 32;  // most spectra per workgroup
constexpr int STATS_NT = 1024;     // threads of a channel-statistics workgroup
constexpr int PREP_TILE = 32;      // transposition tile

__device__ __forceinline__ bool prep_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// (D,HW) -> (HW,Dp): v where the voxel is valid (valid == NULL: where it is finite; a NaN is never
// valid), NaN elsewhere; the pad channel of an odd depth gets NaN and is never read.
static __global__ __launch_bounds__(256) void k_prep_to_device(const double *__restrict__ in,
                                                                const uint8_t *__restrict__ valid,
                                                                double *__restrict__ out, int D, int Dp,
                                                                long HW) {
    __shared__ double tile[PREP_TILE][PREP_TILE + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long s0 = (long)blockIdx.x * PREP_TILE;
    const int z0 = blockIdx.y * PREP_TILE;
    const double nan = __builtin_nan("");
    for (int r = ty; r < PREP_TILE; r += 8) {
        const int z = z0 + r;
        const long s = s0 + tx;
        double v = nan;
        if (z < D && s < HW) {
            const size_t i = (size_t)z * HW + s;
            const double x = in[i];
            const bool ok = valid ? (valid[i] != 0 && x == x) : prep_finite(x);
            v = ok ? x : nan;
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < PREP_TILE; r += 8) {
        const long s = s0 + r;
        const int z = z0 + tx;
        if (s < HW && z < Dp) out[(size_t)s * Dp + z] = tile[tx][r];
    }
}

// continuum (HW,Dp) -> (D,HW), and residual = cube - continuum beside it (both in the host layout)
static __global__ __launch_bounds__(256) void k_prep_to_host(const double *__restrict__ cont_d,
                                                              const double *__restrict__ cube,
                                                              double *__restrict__ cont,
                                                              double *__restrict__ res, int D, int Dp,
                                                              long HW) {
    __shared__ double tile[PREP_TILE][PREP_TILE + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long s0 = (long)blockIdx.x * PREP_TILE;
    const int z0 = blockIdx.y * PREP_TILE;
    for (int r = ty; r < PREP_TILE; r += 8) {
        const long s = s0 + r;
        const int z = z0 + tx;
        tile[r][tx] = (s < HW && z < D) ? cont_d[(size_t)s * Dp + z] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < PREP_TILE; r += 8) {
        const int z = z0 + r;
        const long s = s0 + tx;
        if (z < D && s < HW) {
            const size_t i = (size_t)z * HW + s;
            const double c = tile[tx][r];
            cont[i] = c;
            if (res) res[i] = cube[i] - c;
        }
    }
}

// the rejection pass: a valid voxel stays valid where |v - continuum| <= reject * sigma_z, and
// everywhere in a channel whose sigma is NaN (device layout, NaN = invalid)
static __global__ __launch_bounds__(256) void k_prep_reject(const double *__restrict__ vals,
                                                             const double *__restrict__ cont_d,
                                                             const double *__restrict__ sigma, double reject,
                                                             double *__restrict__ out, int D, int Dp,
                                                             size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int z = (int)(i % (size_t)Dp);
    double v = vals[i];
    if (z < D) {
        const double sg = sigma[z];
        const bool keep = (sg != sg) || (fabs(v - cont_d[i]) <= reject * sg);
        v = keep ? v : __builtin_nan("");
    }
    out[i] = v;
}

// Running median by counting ranks.  A workgroup holds `nspec` consecutive spectra in LDS, each in
// a row of D + 2 h + PREP_CB - 1 doubles with h NaNs in front and h + PREP_CB - 1 behind: an invalid
// voxel is a NaN too, and a NaN compares false with everything, so the window of every voxel is
// the same 2 h + 1 row entries with no test of the ends or of validity.  Lanes run along z (items
// spectrum * D + z): neighbouring lanes read neighbouring LDS addresses.  A thread ranks
// PREP_CB candidates at a time against its window -- one LDS read serves 2 PREP_CB comparisons --
// and candidate v_i is the k-th order statistic iff  #{v_j < v_i} <= k < #{v_j < v_i} + #{v_j == v_i}.
// No branch depends on the data; O((2 h + 1)^2) comparisons per voxel.
static __global__ __launch_bounds__(PREP_NT) void k_running_median(const double *__restrict__ vals,
                                                                    double *__restrict__ out, int D, int Dp,
                                                                    long HW, int h, int nspec, int row) {
    extern __shared__ double smem[];  // [nspec][row]
    const int tid = threadIdx.x;
    const long sp0 = (long)blockIdx.x * nspec;
    const double nan = __builtin_nan("");
    for (int i = tid; i < nspec * row; i += PREP_NT) {
        const int s = i / row, p = i - s * row;
        const int z = p - h;
        const long sp = sp0 + s;
        smem[i] = (z >= 0 && z < D && sp < HW) ? vals[(size_t)sp * Dp + z] : nan;
    }
    __syncthreads();
    const int w = 2 * h + 1;
    for (int it = tid; it < nspec * D; it += PREP_NT) {
        const int s = it / D, z = it - s * D;
        const long sp = sp0 + s;
        if (sp >= HW) break;  // (items ascend: everything after belongs to spectra beyond the cube)
        const double *win = smem + (size_t)s * row + z;  // win[0 .. w-1] is the window of channel z
        int n = 0;
        for (int j = 0; j < w; ++j) {
            const double vj = win[j];
            n += (vj == vj) ? 1 : 0;
        }
        const int k_lo = (n - 1) >> 1, k_hi = n >> 1;  // (n = 0: nothing is selected)
        double r_lo = nan, r_hi = nan;
        for (int i0 = 0; i0 < w; i0 += PREP_CB) {
            double vi[PREP_CB];
            int less[PREP_CB], eq[PREP_CB];
#pragma unroll
            for (int c = 0; c < PREP_CB; ++c) {
                // (the row has PREP_CB - 1 spare entries: the read stays inside it)
                const double x = win[i0 + c];
                vi[c] = (i0 + c < w) ? x : nan;
                less[c] = 0;
                eq[c] = 0;
            }
            for (int j = 0; j < w; ++j) {
                const double vj = win[j];
#pragma unroll
                for (int c = 0; c < PREP_CB; ++c) {
                    less[c] += (vj < vi[c]) ? 1 : 0;
                    eq[c] += (vj == vi[c]) ? 1 : 0;
                }
            }
#pragma unroll
            for (int c = 0; c < PREP_CB; ++c) {
                const bool hit_lo = less[c] <= k_lo && k_lo < less[c] + eq[c];
                const bool hit_hi = less[c] <= k_hi && k_hi < less[c] + eq[c];
                r_lo = hit_lo ? vi[c] : r_lo;
                r_hi = hit_hi ? vi[c] : r_hi;
            }
        }
        out[(size_t)sp * Dp + z] = (n & 1) ? r_lo : (r_lo + r_hi) * 0.5;
    }
}

// order-preserving 64-bit key of a double that is not NaN, and back
__device__ __forceinline__ unsigned long long prep_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double prep_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

struct StatsShared {
    unsigned hist[256];
    unsigned wave_sum[4];
    unsigned long long prefix;
    unsigned k;
    unsigned count;
};

// the k-th (from 0) smallest of the plane's selected values -- x itself (dev == false) or
// |x - centre| -- by a radix select on the order-preserving key, 8 bits a pass from the top: a
// histogram of the digit among the values that share the digits found so far, a scan of its 256
// counts, the digit that holds rank k.  Every thread of the workgroup calls it; all get the result.
__device__ double prep_select(const double *__restrict__ plane, const uint8_t *__restrict__ select, long HW,
                              bool dev, double centre, unsigned k, StatsShared &S) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        S.prefix = 0;
        S.k = k;
    }
    for (int pass = 7; pass >= 0; --pass) {
        const int shift = pass * 8;
        const unsigned long long himask = pass == 7 ? 0ull : (~0ull << (shift + 8));
        if (tid < 256) S.hist[tid] = 0;
        __syncthreads();
        const unsigned long long prefix = S.prefix;
        for (long s = tid; s < HW; s += STATS_NT) {
            const double x = plane[s];
            if ((select == nullptr || select[s] != 0) && prep_finite(x)) {
                const unsigned long long key = prep_key(dev ? fabs(x - centre) : x);
                if (((key ^ prefix) & himask) == 0) atomicAdd(&S.hist[(unsigned)(key >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        // exclusive scan of the 256 counts by the first four wavefronts
        unsigned cnt = 0, incl = 0;
        if (tid < 256) {
            cnt = S.hist[tid];
            incl = cnt;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const unsigned o = __shfl_up(incl, m);
                if ((tid & 63) >= m) incl += o;
            }
            if ((tid & 63) == 63) S.wave_sum[tid >> 6] = incl;
        }
        __syncthreads();
        const unsigned kk = S.k;
        __syncthreads();  // (everyone has read S.k and S.prefix before the owner of the digit writes them)
        if (tid < 256) {
            unsigned base = 0;
            for (int q = 0; q < (tid >> 6); ++q) base += S.wave_sum[q];
            const unsigned excl = base + incl - cnt;
            if (excl <= kk && kk < excl + cnt) {  // (exactly one digit: k is below the number of values)
                S.k = kk - excl;
                S.prefix = prefix | ((unsigned long long)tid << shift);
            }
        }
        __syncthreads();
    }
    const double v = prep_unkey(S.prefix);
    __syncthreads();  // (before the next call's thread 0 resets the prefix)
    return v;
}

// One workgroup per channel plane (contiguous in the host layout): the count n of the selected
// finite values, their median m and the median of |x - m|; out[z] = {m, mad, n}, NaN NaN 0 for n = 0.
static __global__ __launch_bounds__(STATS_NT) void k_channel_stats(const double *__restrict__ cube,
                                                                    const uint8_t *__restrict__ select, long HW,
                                                                    double *__restrict__ out) {
    __shared__ StatsShared S;
    const int tid = threadIdx.x;
    const double *plane = cube + (size_t)blockIdx.x * HW;
    if (tid == 0) S.count = 0;
    __syncthreads();
    unsigned mine = 0;
    for (long s = tid; s < HW; s += STATS_NT)
        mine += ((select == nullptr || select[s] != 0) && prep_finite(plane[s])) ? 1u : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m);
    if ((tid & 63) == 0) atomicAdd(&S.count, mine);
    __syncthreads();
    const unsigned n = S.count;
    __syncthreads();
    double med = __builtin_nan(""), mad = __builtin_nan("");
    if (n > 0) {  // (uniform over the workgroup)
        const unsigned k_lo = (n - 1) >> 1, k_hi = n >> 1;
        const double a = prep_select(plane, select, HW, false, 0.0, k_lo, S);
        med = a;
        if (k_hi != k_lo) med = (a + prep_select(plane, select, HW, false, 0.0, k_hi, S)) * 0.5;
        const double b = prep_select(plane, select, HW, true, med, k_lo, S);
        mad = b;
        if (k_hi != k_lo) mad = (b + prep_select(plane, select, HW, true, med, k_hi, S)) * 0.5;
    }
    if (tid == 0) {
        double *o = out + (size_t)blockIdx.x * 3;
        o[0] = med;
        o[1] = mad;
        o[2] = (double)n;
    }
}

}  // namespace d3d

namespace d3dh {

namespace {

// everything a call allocates, freed on every return path
struct PrepBuffers {
    DevBuf<double> cube;         // (D,HW) the caller's cube
    DevBuf<double> vals;         // (HW,Dp) valid voxels, NaN elsewhere
    DevBuf<double> vals2;        // ... after the rejection pass
    DevBuf<double> cont_d;       // (HW,Dp) running median
    DevBuf<double> cont;         // (D,HW)
    DevBuf<double> res;          // (D,HW)
    DevBuf<double> stats;        // [D][3]
    DevBuf<double> sigma;        // [D]
    DevBuf<uint8_t> valid;       // (D,HW)
    DevBuf<uint8_t> select;      // [HW]
    hipEvent_t ev[4] = {};       // around the running-median kernel, around the statistics kernel
    ~PrepBuffers() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

dim3 tile_grid(const d3d_ctx *c, int depth) {
    return dim3((unsigned)((c->HW + d3d::PREP_TILE - 1) / d3d::PREP_TILE),
                (unsigned)((depth + d3d::PREP_TILE - 1) / d3d::PREP_TILE));
}

int launch_to_device(d3d_ctx *c, const double *cube, const uint8_t *valid, double *vals) {
    hipLaunchKernelGGL(d3d::k_prep_to_device, tile_grid(c, c->Dp), dim3(256), 0, c->stream, cube, valid, vals,
                       c->D, c->Dp, c->HW);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_to_host(d3d_ctx *c, const double *cont_d, const double *cube, double *cont, double *res) {
    hipLaunchKernelGGL(d3d::k_prep_to_host, tile_grid(c, c->D), dim3(256), 0, c->stream, cont_d, cube, cont, res,
                       c->D, c->Dp, c->HW);
    HIP_TRY(hipGetLastError());
    return 0;
}

// vals (HW,Dp), NaN = invalid -> out (HW,Dp); the events B.ev[0], B.ev[1] around the kernel
int launch_running_median(d3d_ctx *c, PrepBuffers &B, const double *vals, double *out, int half_window) {
    // (a half window of D - 1 already spans the whole spectrum from every channel)
    const int h = std::min(half_window, std::max(c->D - 1, 1));
    const int row = c->D + 2 * h + d3d::PREP_CB - 1;
    const size_t row_bytes = (size_t)row * sizeof(double);
    // spectra per workgroup: enough for two passes of the workgroup's threads, within the LDS
    // budget; the deepest cube's single spectrum takes (3682 + 259) * 8 = 31.5 KB
    int nspec = (2 * d3d::PREP_NT + c->D - 1) / c->D;
    nspec = std::min(nspec, (int)(d3d::PREP_LDS / row_bytes));
    nspec = std::max(1, std::min(nspec, d3d::PREP_SPEC_MAX));
    const size_t lds = (size_t)nspec * row_bytes;
    NEED(lds <= 160 * 1024 - 1024, D3D_ERR_UNSUPPORTED,
         "running median: one spectrum of %d channels with half window %d takes %zu bytes of LDS", c->D, h, lds);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&d3d::k_running_median),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned grid = (unsigned)((c->HW + nspec - 1) / nspec);
    HIP_TRY(hipEventRecord(B.ev[0], c->stream));
    hipLaunchKernelGGL(d3d::k_running_median, dim3(grid), dim3(d3d::PREP_NT), lds, c->stream, vals, out, c->D,
                       c->Dp, c->HW, h, nspec, row);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(B.ev[1], c->stream));
    return 0;
}

// cube (D,HW) on the device -> stats [D][3]; the events B.ev[2], B.ev[3] around the kernel
int launch_channel_stats(d3d_ctx *c, PrepBuffers &B, const double *cube, const uint8_t *select, double *stats) {
    HIP_TRY(hipEventRecord(B.ev[2], c->stream));
    hipLaunchKernelGGL(d3d::k_channel_stats, dim3((unsigned)c->D), dim3(d3d::STATS_NT), 0, c->stream, cube, select,
                       c->HW, stats);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(B.ev[3], c->stream));
    return 0;
}

int elapsed_ns(hipEvent_t a, hipEvent_t b, long *ns) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    *ns = (long)(ms * 1e6);
    return 0;
}

int make_events(PrepBuffers &B) {
    for (hipEvent_t &e : B.ev) HIP_TRY(hipEventCreate(&e));
    return 0;
}

}  // namespace

int prep_running_median(d3d_ctx *c, const double *cube, const uint8_t *valid, int half_window, double *out) {
    const size_t n_host = (size_t)c->D * c->HW, n_dev = (size_t)c->HW * c->Dp;
    HIP_TRY(hipSetDevice(c->device));
    PrepBuffers B;
    if (int rc = make_events(B)) return rc;
    HIP_TRY(B.cube.alloc(n_host));
    HIP_TRY(B.vals.alloc(n_dev));
    HIP_TRY(B.cont_d.alloc(n_dev));
    HIP_TRY(B.cont.alloc(n_host));
    HIP_TRY(hipMemcpyAsync(B.cube, cube, n_host * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (valid) {
        HIP_TRY(B.valid.alloc(n_host));
        HIP_TRY(hipMemcpyAsync(B.valid, valid, n_host, hipMemcpyHostToDevice, c->stream));
    }
    if (int rc = launch_to_device(c, B.cube, B.valid, B.vals)) return rc;
    if (int rc = launch_running_median(c, B, B.vals, B.cont_d, half_window)) return rc;
    if (int rc = launch_to_host(c, B.cont_d, nullptr, B.cont, nullptr)) return rc;
    HIP_TRY(hipMemcpyAsync(out, B.cont, n_host * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return elapsed_ns(B.ev[0], B.ev[1], &c->prep_median_ns);
}

int prep_channel_stats(d3d_ctx *c, const double *cube, const uint8_t *select, double *m_out, double *mad_out,
                       int64_t *n_out) {
    const size_t n_host = (size_t)c->D * c->HW;
    HIP_TRY(hipSetDevice(c->device));
    PrepBuffers B;
    if (int rc = make_events(B)) return rc;
    HIP_TRY(B.cube.alloc(n_host));
    HIP_TRY(B.stats.alloc((size_t)c->D * 3));
    HIP_TRY(hipMemcpyAsync(B.cube, cube, n_host * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (select) {
        HIP_TRY(B.select.alloc((size_t)c->HW));
        HIP_TRY(hipMemcpyAsync(B.select, select, (size_t)c->HW, hipMemcpyHostToDevice, c->stream));
    }
    if (int rc = launch_channel_stats(c, B, B.cube, B.select, B.stats)) return rc;
    std::vector<double> st((size_t)c->D * 3);
    HIP_TRY(hipMemcpyAsync(st.data(), B.stats, st.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int z = 0; z < c->D; ++z) {
        m_out[z] = st[(size_t)z * 3];
        mad_out[z] = st[(size_t)z * 3 + 1];
        n_out[z] = (int64_t)st[(size_t)z * 3 + 2];
    }
    return elapsed_ns(B.ev[2], B.ev[3], &c->prep_stats_ns);
}

int prep_prepare(d3d_ctx *c, const double *cube, const uint8_t *select, int half_window, double reject,
                 double *continuum_out, double *residual_out, double *chan_out) {
    const size_t n_host = (size_t)c->D * c->HW, n_dev = (size_t)c->HW * c->Dp;
    const bool rejecting = reject == reject;
    HIP_TRY(hipSetDevice(c->device));
    PrepBuffers B;
    if (int rc = make_events(B)) return rc;
    HIP_TRY(B.cube.alloc(n_host));
    HIP_TRY(B.vals.alloc(n_dev));
    HIP_TRY(B.cont_d.alloc(n_dev));
    HIP_TRY(B.cont.alloc(n_host));
    HIP_TRY(B.res.alloc(n_host));
    HIP_TRY(B.stats.alloc((size_t)c->D * 3));
    if (rejecting) {
        HIP_TRY(B.vals2.alloc(n_dev));
        HIP_TRY(B.sigma.alloc((size_t)c->D));
    }
    HIP_TRY(hipMemcpyAsync(B.cube, cube, n_host * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (select) {
        HIP_TRY(B.select.alloc((size_t)c->HW));
        HIP_TRY(hipMemcpyAsync(B.select, select, (size_t)c->HW, hipMemcpyHostToDevice, c->stream));
    }
    std::vector<double> st((size_t)c->D * 3), sigma((size_t)c->D);
    long median_ns = 0, stats_ns = 0;
    if (int rc = launch_to_device(c, B.cube, nullptr, B.vals)) return rc;
    const double *vals = B.vals;
    for (int pass = 0; pass < (rejecting ? 2 : 1); ++pass) {
        if (int rc = launch_running_median(c, B, vals, B.cont_d, half_window)) return rc;
        if (int rc = launch_to_host(c, B.cont_d, B.cube, B.cont, B.res)) return rc;
        if (int rc = launch_channel_stats(c, B, B.res, B.select, B.stats)) return rc;
        // only the [D][3] statistics cross to the host: sigma_z = 1.4826 mad_z, NaN for n_z < 2 or mad_z = 0
        HIP_TRY(hipMemcpyAsync(st.data(), B.stats, st.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        long a = 0, b = 0;
        if (int rc = elapsed_ns(B.ev[0], B.ev[1], &a)) return rc;
        if (int rc = elapsed_ns(B.ev[2], B.ev[3], &b)) return rc;
        median_ns += a;
        stats_ns += b;
        for (int z = 0; z < c->D; ++z) {
            const double mad = st[(size_t)z * 3 + 1], n = st[(size_t)z * 3 + 2];
            sigma[z] = (n < 2.0 || mad == 0.0) ? std::nan("") : 1.4826 * mad;
        }
        if (pass == 0 && rejecting) {
            HIP_TRY(hipMemcpyAsync(B.sigma, sigma.data(), sigma.size() * sizeof(double), hipMemcpyHostToDevice,
                                   c->stream));
            hipLaunchKernelGGL(d3d::k_prep_reject, dim3((unsigned)((n_dev + 255) / 256)), dim3(256), 0, c->stream,
                               (const double *)B.vals, (const double *)B.cont_d, (const double *)B.sigma, reject,
                               B.vals2, c->D, c->Dp, n_dev);
            HIP_TRY(hipGetLastError());
            vals = B.vals2;
        }
    }
    HIP_TRY(hipMemcpyAsync(continuum_out, B.cont, n_host * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(residual_out, B.res, n_host * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int z = 0; z < c->D; ++z) {
        chan_out[(size_t)z * 3] = st[(size_t)z * 3];
        chan_out[(size_t)z * 3 + 1] = sigma[z];
        chan_out[(size_t)z * 3 + 2] = st[(size_t)z * 3 + 2];
    }
    c->prep_median_ns = median_ns;
    c->prep_stats_ns = stats_ns;
    return 0;
}

}  // namespace d3dh
