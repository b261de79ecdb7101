// Region posteriors on the device (d3d_region_*): per sample of the posterior moments the flux F,
// the flux-weighted centre C and width S of every labelled set of spaxels into a series, and the
// set's summed clean spectrum into a running mean and M2.  A segmented reduction over the label
// map in a FIXED order (include/deconv3d_hip.h states it): no atomics, and nothing that depends on
// the grid, the options or the number of regions.  gfx950 only.
#include "d3d_ctx.h"

namespace d3d {

constexpr int REGION_CHUNK = 64;  // members per chunk: one per lane of a wavefront

struct RegionArgs {
    int K, D, Dp, steps, n_chunks;
    double n;               // number of this sample, counted from 1 (k_post_accum's)
    double flux_k;          // F = (a w) flux_k, as k_post_accum has it
    const double *params;   // (H,W,3) chain state
    const int *member;      // [members] spaxel of every member, region after region, row-major inside
    const int4 *chunk;      // [n_chunks] {first member, members (1..64), region, -}
    const int *first;       // [K + 1] first chunk of every region
    double *part;           // [n_chunks][4]: sum F | sum F c | sum F (w^2 + (c - C)^2) | -
    double *fc;             // [K][2]: F_k | C_k between the two passes
    double *row;            // [K][3] this sample's row of the series; NULL: the series is full
    double *spart;          // [n_chunks][Dp] spectrum partials; NULL: spectra off
    double *spec_mean, *spec_m2;  // [K][Dp]
    LineShape line;
};

// The fold of a wavefront's 64 terms by halves, v = v[:32] + v[32:], then 16, ... 1: an
// xor-butterfly, after which every lane holds the sum (a + b == b + a bit for bit).
__device__ __forceinline__ double region_fold(double v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// Lane j's value in every lane (j a constant after unrolling: two v_readlane, no LDS round trip).
__device__ __forceinline__ double region_lane(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j),
                            __builtin_amdgcn_readlane(__double2loint(v), j));
}

// Sums of the elements col and (TWO) col + 1 of the chunk partials c0 .. c1 - 1 in ascending order
// from +0.0, the same in every lane: 64 partials in one coalesced load, then lane after lane.
// Lanes beyond c1 hold +0.0, and adding +0.0 to a sum that started from +0.0 never changes it (such
// a sum is never -0.0), so all 64 are added: the order does not depend on where a region ends.
template <bool TWO>
__device__ __forceinline__ void region_chunk_sums(const double *part, int col, int c0, int c1, int lane, double &s0,
                                                  double &s1) {
    s0 = 0.0;
    s1 = 0.0;
    for (int base = c0; base < c1; base += 64) {
        const bool have = base + lane < c1;
        const double *p = part + (size_t)(base + lane) * 4 + col;
        const double v0 = have ? p[0] : 0.0;
        const double v1 = (TWO && have) ? p[1] : 0.0;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            s0 += region_lane(v0, j);
            if (TWO) s1 += region_lane(v1, j);
        }
    }
}

// Stage one of the scalars, one wavefront per chunk, lane = member (absent lanes contribute +0.0).
// PASS 0: sum F_i and sum F_i c_i.  PASS 1, after k_region_reduce<0> has left the region's C:
// sum F_i (w_i^2 + (c_i - C)^2) -- two passes, so nothing cancels.
template <int PASS>
static __global__ __launch_bounds__(256) void k_region_chunks(RegionArgs A) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int ci = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ci >= A.n_chunks) return;
    const int4 ch = A.chunk[ci];
    double t0 = 0.0, t1 = 0.0;
    if (lane < ch.y) {
        const long sp = A.member[ch.x + lane];
        const double a = A.params[sp * 3 + 0], c = A.params[sp * 3 + 1], w = A.params[sp * 3 + 2];
        const double F = (a * w) * A.flux_k;
        if (PASS == 0) {
            t0 = F;
            t1 = F * c;
        } else {
            const double d = c - A.fc[2 * ch.z + 1];
            t0 = F * (w * w + d * d);
        }
    }
    t0 = region_fold(t0);
    if (PASS == 0) t1 = region_fold(t1);
    if (lane == 0) {
        if (PASS == 0) {
            A.part[(size_t)ci * 4 + 0] = t0;
            A.part[(size_t)ci * 4 + 1] = t1;
        } else {
            A.part[(size_t)ci * 4 + 2] = t0;
        }
    }
}

// Stage two of the scalars, one wavefront per region: the chunk partials in ascending order.
// PASS 0 leaves F_k and C_k = (sum F c) / F_k; PASS 1 writes the sample's (F, C, S) with
// S = sqrt((sum F (w^2 + (c - C)^2)) / F_k).  F_k == 0 -- no member, or no flux -- is (0, NaN, NaN).
template <int PASS>
static __global__ __launch_bounds__(256) void k_region_reduce(RegionArgs A) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= A.K) return;
    const int c0 = A.first[k], c1 = A.first[k + 1];
    const double nan = __builtin_nan("");
    if (PASS == 0) {
        double F, Fc;
        region_chunk_sums<true>(A.part, 0, c0, c1, lane, F, Fc);
        if (lane == 0) {
            A.fc[2 * k + 0] = F;
            A.fc[2 * k + 1] = (F == 0.0) ? nan : Fc / F;
        }
    } else {
        double ss, unused;
        region_chunk_sums<false>(A.part, 2, c0, c1, lane, ss, unused);
        if (lane == 0) {
            const double F = A.fc[2 * k + 0];
            const bool none = F == 0.0;
            A.row[3 * k + 0] = none ? 0.0 : F;
            A.row[3 * k + 1] = A.fc[2 * k + 1];
            A.row[3 * k + 2] = none ? nan : sqrt(ss / F);
        }
    }
}

// Stage one of the spectra, one wavefront per (chunk, step of 64 channels), lane = channel: the
// chunk's members one after the other in ascending order from +0.0, each a k_post_accum's clean
// sample a unit_line(z, c, w).  The chunk comes from the block index, so a member's spaxel and
// parameters are the same in every lane (scalar loads), and the store is one coalesced 512 bytes.
// The pad channel of an odd depth is written 0.
template <bool MULTI>
static __global__ __launch_bounds__(64) void k_region_spectra(RegionArgs A) {
#pragma clang fp contract(off)
    const int ci = blockIdx.x / A.steps;
    const int z = (blockIdx.x - ci * A.steps) * 64 + threadIdx.x;
    if (z >= A.Dp) return;
    const int4 ch = A.chunk[ci];
    double acc = 0.0;
    if (z < A.D) {
        for (int m = 0; m < ch.y; ++m) {
            const long sp = A.member[ch.x + m];
            const double a = A.params[sp * 3 + 0], c = A.params[sp * 3 + 1], w = A.params[sp * 3 + 2];
            const double v = a * unit_line<MULTI>(A.line, (double)z, c, w);
            acc += v;
        }
    }
    A.spart[(size_t)ci * A.Dp + z] = acc;
}

// Stage two of the spectra, one wavefront per (region, step of 64 channels), lane = channel: the
// chunk partials in ascending order from +0.0 (coalesced rows, 32 independent loads in flight), then
// Welford.
static __global__ __launch_bounds__(64) void k_region_spectra_fold(RegionArgs A) {
#pragma clang fp contract(off)
    const int k = blockIdx.x / A.steps;
    const int z = (blockIdx.x - k * A.steps) * 64 + threadIdx.x;
    if (z >= A.Dp) return;
    const int c0 = A.first[k], c1 = A.first[k + 1];
    double s = 0.0;
#pragma unroll 32
    for (int ci = c0; ci < c1; ++ci) s += A.spart[(size_t)ci * A.Dp + z];
    const size_t at = (size_t)k * A.Dp + z;
    double mu = A.spec_mean[at], m2 = A.spec_m2[at];
    welford(mu, m2, s, A.n);
    A.spec_mean[at] = mu;
    A.spec_m2[at] = m2;
}

}  // namespace d3d

namespace d3dh {

// The members of the regions from the label map and the mask in force: region after region, its
// unmasked spaxels in row-major order, cut into chunks of 64 (the last of a region may be short).
void region_layout(const d3d_ctx *c, std::vector<int> &member, std::vector<int4> &chunk, std::vector<int> &first,
                   std::vector<int32_t> &sizes) {
    const int K = c->reg.K;
    sizes.assign((size_t)K, 0);
    for (long s = 0; s < c->HW; ++s) {
        const int l = c->reg.h_labels[(size_t)s];
        if (l > 0 && c->h_mask[(size_t)s]) ++sizes[(size_t)l - 1];
    }
    std::vector<size_t> at((size_t)K + 1, 0);
    for (int k = 0; k < K; ++k) at[(size_t)k + 1] = at[(size_t)k] + (size_t)sizes[(size_t)k];
    member.assign(at[(size_t)K], 0);
    std::vector<size_t> next(at.begin(), at.end() - 1);
    for (long s = 0; s < c->HW; ++s) {
        const int l = c->reg.h_labels[(size_t)s];
        if (l > 0 && c->h_mask[(size_t)s]) member[next[(size_t)l - 1]++] = (int)s;
    }
    chunk.clear();
    first.assign((size_t)K + 1, 0);
    for (int k = 0; k < K; ++k) {
        first[(size_t)k] = (int)chunk.size();
        for (int m = 0; m < sizes[(size_t)k]; m += d3d::REGION_CHUNK)
            chunk.push_back(make_int4((int)at[(size_t)k] + m, std::min(d3d::REGION_CHUNK, sizes[(size_t)k] - m), k, 0));
    }
    first[(size_t)K] = (int)chunk.size();
}

template <bool MULTI>
static void launch_region_spectra_t(d3d_ctx *c, const d3d::RegionArgs &A) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(d3d::k_region_spectra<MULTI>), dim3((unsigned)A.n_chunks * (unsigned)A.steps),
                       dim3(64), 0, c->stream, A);
}

int launch_region_sample(d3d_ctx *c) {
    d3d::RegionArgs A;
    A.K = c->reg.K;
    A.D = c->D;
    A.Dp = c->Dp;
    A.steps = (c->Dp + 63) / 64;
    A.n_chunks = c->reg.nchunks;
    A.n = (double)(c->post.n + 1);
    A.flux_k = flux_factor(c);
    A.params = c->params;
    A.member = c->reg.member;
    A.chunk = c->reg.chunk;
    A.first = c->reg.first;
    A.part = c->reg.part;
    A.fc = c->reg.fc;
    A.row = c->post.n < c->reg.rows ? c->reg.series + (size_t)c->post.n * (size_t)c->reg.K * 3 : nullptr;
    A.spart = c->reg.spart;
    A.spec_mean = c->reg.spec;
    A.spec_m2 = c->reg.spec ? c->reg.spec + (size_t)c->reg.K * c->Dp : nullptr;
    A.line = c->line;
    const unsigned chunk_grid = (unsigned)((A.n_chunks + 3) / 4), region_grid = (unsigned)((A.K + 3) / 4);
    if (A.row) {  // (past the capacity the series stops, the spectra go on)
        if (A.n_chunks)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(d3d::k_region_chunks<0>), dim3(chunk_grid), dim3(256), 0, c->stream, A);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(d3d::k_region_reduce<0>), dim3(region_grid), dim3(256), 0, c->stream, A);
        if (A.n_chunks)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(d3d::k_region_chunks<1>), dim3(chunk_grid), dim3(256), 0, c->stream, A);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(d3d::k_region_reduce<1>), dim3(region_grid), dim3(256), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
    }
    if (A.spart) {
        if (A.n_chunks) {
            // MULTI only for K > 1 or a table, as every other line kernel
            if (d3d::line_multi(c->line))
                launch_region_spectra_t<true>(c, A);
            else
                launch_region_spectra_t<false>(c, A);
        }
        hipLaunchKernelGGL(d3d::k_region_spectra_fold, dim3((unsigned)A.K * (unsigned)A.steps), dim3(64), 0,
                           c->stream, A);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// The members of the regions under the mask in force, on the device (d3d_region_begin, and
// d3d_set_data on a context with regions: its mask may have changed).  The tables that depend on
// the number of chunks are allocated here; on failure the regions are freed.
int region_members(d3d_ctx *c) {
    std::vector<int> member, first;
    std::vector<int4> chunk;
    region_layout(c, member, chunk, first, c->reg.h_sizes);
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->reg.spart.reset();
    c->reg.nchunks = (int)chunk.size();
    const size_t nm = std::max<size_t>(member.size(), 1), nc = std::max<size_t>(chunk.size(), 1);
    hipError_t e = c->reg.member.alloc(nm);
    if (e == hipSuccess) e = c->reg.chunk.alloc(nc);
    if (e == hipSuccess) e = c->reg.first.alloc(first.size());
    if (e == hipSuccess) e = c->reg.part.alloc(nc * 4);
    if (e == hipSuccess && (c->reg.what & 1)) e = c->reg.spart.alloc(nc * c->Dp);
    if (e == hipSuccess && !member.empty())
        e = hipMemcpyAsync(c->reg.member, member.data(), member.size() * sizeof(int), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && !chunk.empty())
        e = hipMemcpyAsync(c->reg.chunk, chunk.data(), chunk.size() * sizeof(int4), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->reg.first, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the host vectors go out of scope
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the context stays usable for the chain and the moments
        c->reg = {};
        return fail(D3D_ERR_HIP, "region posteriors (%zu members in %zu chunks): %s", member.size(), chunk.size(),
                    hipGetErrorString(e));
    }
    return 0;
}

}  // namespace d3dh

using namespace d3dh;

extern "C" {

int d3d_region_begin(d3d_ctx *c, const int32_t *labels, int K, int64_t capacity, int what) {
    NEED(c && labels, D3D_ERR_INVALID, "NULL argument");
    NEED(K >= 1, D3D_ERR_INVALID, "K = %d: at least one region", K);
    NEED(capacity >= 0, D3D_ERR_INVALID, "capacity = %lld is negative", (long long)capacity);
    NEED(what >= 0 && what <= 1, D3D_ERR_INVALID, "what = %d: bit 0 the spectra (0..1)", what);
    for (long s = 0; s < c->HW; ++s)
        NEED(labels[s] >= 0 && labels[s] <= K, D3D_ERR_INVALID, "labels[%ld] = %d lies outside 0 .. K = %d", s,
             (int)labels[s], K);
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED,
         "region posteriors on a tile: the parameters of its frame belong to other ranks");
    NEED(c->post.on, D3D_ERR_STATE, "posterior moments not begun (d3d_post_begin)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->reg = {};
    c->reg.K = K;
    c->reg.what = what;
    c->reg.rows = capacity;
    c->reg.h_labels.assign(labels, labels + c->HW);
    const size_t series_elems = (size_t)capacity * K * 3;
    const size_t spec_elems = (what & 1) ? (size_t)2 * K * c->Dp : 0;
    hipError_t e = c->reg.fc.alloc((size_t)K * 2);
    if (e == hipSuccess && series_elems) e = c->reg.series.alloc(series_elems);
    if (e == hipSuccess && spec_elems) e = c->reg.spec.alloc(spec_elems);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the context stays usable for the chain and the moments
        c->reg = {};
        return fail(D3D_ERR_HIP, "region posteriors (%zu bytes): %s", (series_elems + spec_elems) * sizeof(double),
                    hipGetErrorString(e));
    }
    if (int rc = region_members(c)) return rc;
    c->reg.on = true;
    return post_reset(c);  // the series' rows are the moments' samples
}

int d3d_region_count(d3d_ctx *c, int64_t *n, int64_t *stored) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    if (n) *n = c->reg.on ? c->post.n : 0;
    if (stored) *stored = c->reg.on ? std::min<int64_t>(c->post.n, c->reg.rows) : 0;
    return D3D_OK;
}

int d3d_region_get(d3d_ctx *c, double *series, double *spec_mean, double *spec_m2, int32_t *sizes) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->reg.on, D3D_ERR_STATE, "region posteriors not begun (d3d_region_begin)");
    NEED(c->reg.spec || (!spec_mean && !spec_m2), D3D_ERR_STATE,
         "the regions' spectra were not begun (d3d_region_begin what = %d)", c->reg.what);
    HIP_TRY(hipSetDevice(c->device));
    const size_t stored = (size_t)std::min<int64_t>(c->post.n, c->reg.rows);
    if (series && stored)
        HIP_TRY(hipMemcpyAsync(series, c->reg.series, stored * c->reg.K * 3 * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream));
    // (K, Dp) on the device, (K, D) for the caller: the pad channel of an odd depth stays behind
    const size_t row = (size_t)c->D * sizeof(double), pitch = (size_t)c->Dp * sizeof(double);
    if (spec_mean)
        HIP_TRY(hipMemcpy2DAsync(spec_mean, row, c->reg.spec, pitch, row, (size_t)c->reg.K, hipMemcpyDeviceToHost,
                                 c->stream));
    if (spec_m2)
        HIP_TRY(hipMemcpy2DAsync(spec_m2, row, c->reg.spec + (size_t)c->reg.K * c->Dp, pitch, row, (size_t)c->reg.K,
                                 hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (sizes) std::copy(c->reg.h_sizes.begin(), c->reg.h_sizes.end(), sizes);
    return D3D_OK;
}

int d3d_region_end(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->reg = {};
    return D3D_OK;
}

}  // extern "C"
