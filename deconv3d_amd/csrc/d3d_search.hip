// Matched-filter line search on the device (d3d_line_search): every spaxel's data against a bank
// of LSF-convolved unit lines over a grid of centres and widths -- detection S/N, best candidate
// and its two centre neighbours, with no (candidates x spaxels) array in memory.  gfx950 only.
#include "d3d_ctx.h"

namespace d3d {

// threads of a search workgroup, candidates a thread owns per pass, candidates per pass
constexpr int SEARCH_NT = 256;
constexpr int SEARCH_KC = 4;
constexpr int SEARCH_PASS = SEARCH_NT * SEARCH_KC;

struct SearchArgs {
    int D, Dp;
    int n_c, n_cand;
    int ncp;               // row length of the transposed bank: n_cand rounded up to even
    long nspax;
    const double *bt;      // [D][ncp] transposed bank, zero beyond n_cand
    const double *data;    // SLOT_DATA [nspax][Dp]
    const double *ivar;    // SLOT_IVAR
    const uint8_t *mask;   // the caller's mask (d3d_set_data), not the NaN rule
    int *best;             // [nspax]
    double *stat;          // [nspax][4]
};

// bank [n_cand][Dp] -> bt [D][ncp] (lanes along the candidates: the search reads rows of bt
// coalesced); the columns n_cand .. ncp are zero
static __global__ __launch_bounds__(256) void k_search_transpose(const double *__restrict__ bank,
                                                                  double *__restrict__ bt, int D, int Dp,
                                                                  int n_cand, int ncp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)D * ncp) return;
    const int z = (int)(i / ncp), k = (int)(i - (long)z * ncp);
    bt[i] = k < n_cand ? bank[(long)k * Dp + z] : 0.0;
}

__device__ __forceinline__ double search_snr(double N, double Q) { return Q > 0.0 ? N / sqrt(Q) : 0.0; }

// (s, k) of a better candidate: a larger statistic, or the same one at a lower index
__device__ __forceinline__ bool search_better(double s, int k, double bs, int bk) {
    return k >= 0 && (bk < 0 || s > bs || (s == bs && k < bk));
}

// One workgroup per SPX consecutive spaxels, whose d iv and iv spectra sit in LDS as rows
// [z][x_0 .. x_SPX-1 | v_0 .. v_SPX-1]: every thread reads the same row (a broadcast, 16-byte
// reads).  A thread owns the candidates {k0, k0 + 1, k1, k1 + 1}, k0 = pass * 1024 + 2 tid,
// k1 = k0 + 512, per pass and streams their bank values from the transposed bank (a wavefront
// reads 1 KiB of one row per load; the bank stays in L2): per channel 2 global and SPX / 2 LDS
// 16-byte reads for 8 SPX fp64 FMAs.  The epilogue of a pass folds its 4 SPX statistics into the
// thread's running (s, k) per spaxel; the workgroup then reduces them (lowest k on a tie) and a
// second, small phase recomputes N and Q of the winner and of its two centre neighbours, a
// wavefront per (spaxel, candidate) with lanes along z.
template <int SPX>
static __global__ __launch_bounds__(SEARCH_NT) void k_line_search(SearchArgs A) {
    extern __shared__ double smem[];  // [D][2 SPX]
    __shared__ double red_s[SEARCH_NT / 64][SPX];
    __shared__ int red_k[SEARCH_NT / 64][SPX];
    __shared__ int win[SPX];
    __shared__ double res[SPX][3][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long sp0 = (long)blockIdx.x * SPX;
    for (int i = tid; i < SPX * A.D; i += SEARCH_NT) {
        const int s = i / A.D, z = i - s * A.D;
        const long sp = sp0 + s;
        double d = 0.0, iv = 0.0;
        if (sp < A.nspax) {
            d = A.data[sp * A.Dp + z];
            iv = A.ivar[sp * A.Dp + z];
        }
        smem[(size_t)z * 2 * SPX + s] = d * iv;
        smem[(size_t)z * 2 * SPX + SPX + s] = iv;
    }
    __syncthreads();

    double bs[SPX];
    int bk[SPX];
#pragma unroll
    for (int s = 0; s < SPX; ++s) {
        bs[s] = 0.0;
        bk[s] = -1;
    }
    for (int base = 0; base < A.ncp; base += SEARCH_PASS) {
        const int k0 = base + 2 * tid, k1 = k0 + SEARCH_PASS / 2;
        if (k0 >= A.ncp) continue;  // (k1 > k0: nothing of this pass is the thread's)
        const bool h1 = k1 < A.ncp;
        // (ncp and k0, k1 are even: the pair k, k + 1 lies inside the row)
        const double *p0 = A.bt + k0, *p1 = A.bt + (h1 ? k1 : k0);
        double aN[SEARCH_KC][SPX], aQ[SEARCH_KC][SPX];
#pragma unroll
        for (int c = 0; c < SEARCH_KC; ++c)
#pragma unroll
            for (int s = 0; s < SPX; ++s) {
                aN[c][s] = 0.0;
                aQ[c][s] = 0.0;
            }
        double2 n0 = *reinterpret_cast<const double2 *>(p0);
        double2 n1 = *reinterpret_cast<const double2 *>(p1);
#pragma unroll 2
        for (int z = 0; z < A.D; ++z) {
            const double t[SEARCH_KC] = {n0.x, n0.y, n1.x, n1.y};
            const int zn = z + 1 < A.D ? z + 1 : z;  // the next channel's values, in flight over this one's FMAs
            n0 = *reinterpret_cast<const double2 *>(p0 + (size_t)zn * A.ncp);
            n1 = *reinterpret_cast<const double2 *>(p1 + (size_t)zn * A.ncp);
            const double2 *row = reinterpret_cast<const double2 *>(smem + (size_t)z * 2 * SPX);
            double rv[2 * SPX];
#pragma unroll
            for (int j = 0; j < SPX; ++j) {
                const double2 p = row[j];
                rv[2 * j] = p.x;
                rv[2 * j + 1] = p.y;
            }
#pragma unroll
            for (int c = 0; c < SEARCH_KC; ++c) {
                const double tq = t[c] * t[c];
#pragma unroll
                for (int s = 0; s < SPX; ++s) {
                    aN[c][s] = fma(t[c], rv[s], aN[c][s]);
                    aQ[c][s] = fma(tq, rv[SPX + s], aQ[c][s]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < SEARCH_KC; ++c) {
            const int k = (c < 2 ? k0 : k1) + (c & 1);
            if (k >= A.n_cand || (c >= 2 && !h1)) continue;
#pragma unroll
            for (int s = 0; s < SPX; ++s) {
                if (aQ[c][s] > 0.0 && aN[c][s] > 0.0) {
                    const double sv = aN[c][s] / sqrt(aQ[c][s]);
                    if (search_better(sv, k, bs[s], bk[s])) {
                        bs[s] = sv;
                        bk[s] = k;
                    }
                }
            }
        }
    }
    // the workgroup's winner per spaxel
#pragma unroll
    for (int s = 0; s < SPX; ++s) {
        double vs = bs[s];
        int vk = bk[s];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double os = __shfl_xor(vs, m);
            const int ok = __shfl_xor(vk, m);
            if (search_better(os, ok, vs, vk)) {
                vs = os;
                vk = ok;
            }
        }
        if (lane == 0) {
            red_s[wave][s] = vs;
            red_k[wave][s] = vk;
        }
    }
    __syncthreads();
    if (tid < SPX) {
        double vs = red_s[0][tid];
        int vk = red_k[0][tid];
        for (int w = 1; w < SEARCH_NT / 64; ++w)
            if (search_better(red_s[w][tid], red_k[w][tid], vs, vk)) {
                vs = red_s[w][tid];
                vk = red_k[w][tid];
            }
        win[tid] = vk;
    }
    __syncthreads();
    // N and Q of the winner and of its centre neighbours (same width), lanes along z
    for (int item = wave; item < 3 * SPX; item += SEARCH_NT / 64) {
        const int s = item / 3, j = item - 3 * s;
        const int k = win[s];  // (wave-uniform)
        if (k < 0) continue;
        const int ic = k % A.n_c + (j - 1);
        if (ic < 0 || ic >= A.n_c) continue;
        const int cand = k + (j - 1);
        double N = 0.0, Q = 0.0;
        for (int z = lane; z < A.D; z += 64) {
            const double t = A.bt[(size_t)z * A.ncp + cand];
            N = fma(t, smem[(size_t)z * 2 * SPX + s], N);
            Q = fma(t * t, smem[(size_t)z * 2 * SPX + SPX + s], Q);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            N += __shfl_xor(N, m);
            Q += __shfl_xor(Q, m);
        }
        if (lane == 0) {
            res[s][j][0] = N;
            res[s][j][1] = Q;
        }
    }
    __syncthreads();
    if (tid < SPX && sp0 + tid < A.nspax) {
        const long sp = sp0 + tid;
        const int k = A.mask[sp] != 0 ? win[tid] : -1;
        double o[4] = {0.0, 0.0, 0.0, 0.0};
        if (k >= 0) {
            const int ic = k % A.n_c;
            const double nan = __builtin_nan("");
            o[0] = res[tid][1][0];
            o[1] = res[tid][1][1];
            o[2] = ic > 0 ? search_snr(res[tid][0][0], res[tid][0][1]) : nan;
            o[3] = ic + 1 < A.n_c ? search_snr(res[tid][2][0], res[tid][2][1]) : nan;
        }
        A.best[sp] = k;
#pragma unroll
        for (int q = 0; q < 4; ++q) A.stat[sp * 4 + q] = o[q];
    }
}

}  // namespace d3d

namespace d3dh {

namespace {

// everything the call allocates, freed on every return path
struct SearchBuffers {
    DevBuf<double> bank, bt, pmap, stat;
    DevBuf<uint8_t> ones, umask;
    DevBuf<int> best;
    hipEvent_t ev[4] = {};  // around the bank build, around the search kernel
    ~SearchBuffers() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

template <int SPX>
int launch_search_t(d3d_ctx *c, const d3d::SearchArgs &A) {
    const size_t lds = (size_t)A.D * 2 * SPX * sizeof(double);
    auto kern = &d3d::k_line_search<SPX>;
    // (up to 48 KiB for 8, 4 or 2 spaxels, up to 128 KiB for one spaxel of the deepest cube)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    const unsigned grid = (unsigned)((A.nspax + SPX - 1) / SPX);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(d3d::SEARCH_NT), lds, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

int line_search(d3d_ctx *c, int n_c, const double *centres, int n_w, const double *widths,
                const double *host_bank, int *best_out, double *stat_out) {
    const long n_cand = (long)n_c * n_w;
    const size_t bank_bytes = (size_t)n_cand * c->Dp * sizeof(double);
    NEED(bank_bytes <= SEARCH_BANK_BUDGET, D3D_ERR_UNSUPPORTED,
         "line search: the template bank of %d widths x %d centres x %d channels takes %zu bytes, above the "
         "budget of %zu: search fewer centres at a time (a sub-range of the channels) or fewer widths",
         n_w, n_c, c->Dp, bank_bytes, SEARCH_BANK_BUDGET);
    const int ncp = (int)((n_cand + 1) & ~1L);
    HIP_TRY(hipSetDevice(c->device));
    SearchBuffers B;
    HIP_TRY(B.bank.alloc((size_t)n_cand * c->Dp));
    HIP_TRY(B.bt.alloc((size_t)c->D * ncp));
    HIP_TRY(B.umask.alloc((size_t)c->HW));
    HIP_TRY(B.best.alloc((size_t)c->HW));
    HIP_TRY(B.stat.alloc((size_t)c->HW * 4));
    for (hipEvent_t &e : B.ev) HIP_TRY(hipEventCreate(&e));
    if (host_bank) {
        HIP_TRY(hipEventRecord(B.ev[0], c->stream));
        // rows of D channels into rows of Dp (the pad channel of an odd depth stays 0)
        HIP_TRY(hipMemsetAsync(B.bank, 0, bank_bytes, c->stream));
        HIP_TRY(hipMemcpy2DAsync(B.bank, (size_t)c->Dp * sizeof(double), host_bank, (size_t)c->D * sizeof(double),
                                 (size_t)c->D * sizeof(double), (size_t)n_cand, hipMemcpyHostToDevice, c->stream));
    } else {
        // the forward model's own line kernels on a map of (1, c, w) rows: the bank is what a
        // spaxel with these parameters contributes before the FSF, bit for bit
        std::vector<double> rows((size_t)n_cand * 3);
        for (int iw = 0; iw < n_w; ++iw)
            for (int ic = 0; ic < n_c; ++ic) {
                double *r = rows.data() + ((size_t)iw * n_c + ic) * 3;
                r[0] = 1.0;
                r[1] = centres[ic];
                r[2] = widths[iw];
            }
        HIP_TRY(B.pmap.alloc(rows.size()));
        HIP_TRY(B.ones.alloc((size_t)n_cand));
        HIP_TRY(hipMemcpyAsync(B.pmap, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice,
                               c->stream));
        HIP_TRY(hipMemsetAsync(B.ones, 1, (size_t)n_cand, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (rows leaves scope)
        HIP_TRY(hipEventRecord(B.ev[0], c->stream));
        // the line launchers take their spectrum count and mask from the context
        const long HW = c->HW;
        c->HW = n_cand;
        std::swap(c->mask, B.ones);
        const int rc = launch_lines(c, B.bank, 1, B.pmap);
        c->HW = HW;
        std::swap(c->mask, B.ones);
        if (rc) return rc;
    }
    {
        const long n = (long)c->D * ncp;
        hipLaunchKernelGGL(d3d::k_search_transpose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                           (const double *)B.bank, B.bt, c->D, c->Dp, (int)n_cand, ncp);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(B.ev[1], c->stream));
    HIP_TRY(hipMemcpyAsync(B.umask, c->h_user_mask.data(), (size_t)c->HW, hipMemcpyHostToDevice, c->stream));
    d3d::SearchArgs A;
    A.D = c->D;
    A.Dp = c->Dp;
    A.n_c = n_c;
    A.n_cand = (int)n_cand;
    A.ncp = ncp;
    A.nspax = c->HW;
    A.bt = B.bt;
    A.data = c->slot[D3D_SLOT_DATA];
    A.ivar = c->slot[D3D_SLOT_IVAR];
    A.mask = B.umask;
    A.best = B.best;
    A.stat = B.stat;
    // spaxels per workgroup: as many of 8, 4, 2, 1 as keep the spectra within 48 KiB of LDS (two
    // workgroups per CU); one spaxel of a deeper cube takes up to 128 KiB
    const size_t per_spaxel = (size_t)c->D * 2 * sizeof(double);
    HIP_TRY(hipEventRecord(B.ev[2], c->stream));
    int rc;
    if (8 * per_spaxel <= 48 * 1024) rc = launch_search_t<8>(c, A);
    else if (4 * per_spaxel <= 48 * 1024) rc = launch_search_t<4>(c, A);
    else if (2 * per_spaxel <= 48 * 1024) rc = launch_search_t<2>(c, A);
    else rc = launch_search_t<1>(c, A);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(B.ev[3], c->stream));
    HIP_TRY(hipMemcpyAsync(best_out, B.best, (size_t)c->HW * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(stat_out, B.stat, (size_t)c->HW * 4 * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms_bank = 0.f, ms_kernel = 0.f;  // (options search_bank_ns / search_kernel_ns: tools/search_time.py)
    HIP_TRY(hipEventElapsedTime(&ms_bank, B.ev[0], B.ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms_kernel, B.ev[2], B.ev[3]));
    c->search_bank_ns = (long)(ms_bank * 1e6);
    c->search_kernel_ns = (long)(ms_kernel * 1e6);
    return 0;
}

}  // namespace d3dh
