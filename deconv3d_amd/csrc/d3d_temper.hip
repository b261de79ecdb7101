// Replica exchange between tempered chains (d3d_temper_*): n contexts of one geometry sample
// L^beta_r x prior -- the same model with the variance divided by beta_r, so no sweep kernel
// knows about it -- and adjacent rungs trade their STATES (residual + parameters) by the
// Metropolis rule of parallel tempering.  One round is three launches on the leader's stream
// with nothing but device memory between them: the chains' energies (k_temper_energy), the
// decisions (k_temper_decide), the swaps (k_temper_exchange).  gfx950 only.
#include "d3d_ctx.h"

namespace d3d {

constexpr int TEMPER_MAX = 64;  // rungs of a group at most (the chains' pointers travel as kernel arguments)
constexpr int TEMPER_NT = 256;

// What the kernels need of every chain, by value (2.5 KiB of kernel arguments).
struct TemperChains {
    double *err[TEMPER_MAX];         // SLOT_ERR, (HW, Dp): pad channels hold zero residual
    const double *ivar[TEMPER_MAX];  // SLOT_IVAR, or NULL: one constant 1/variance
    double ivar_uniform[TEMPER_MAX];
    double *params[TEMPER_MAX];      // (HW, 3)
    double beta[TEMPER_MAX];
};

struct TemperBlock {
    double *partials;   // [n][nblk] block partials of k_temper_energy
    double *energy;     // [n] E_r of the last round
    double *u, *logu;   // [n-1] of the last round (NaN: pair not proposed)
    double *e_mean, *e_m2;  // [n] Welford moments of the energy at every rung
    long long *attempts, *accepts;  // [n-1]
    long long *e_n;     // [n]
    int *decided;       // [n-1] of the last round: 1, 0, -1 = not proposed
    int *labels;        // [n] which start's state sits at rung r
};

// total_r = sum_v 0.5 err^2 / var of chain r = blockIdx.y, as gridDim.x block partials.  Fixed
// order: every lane walks the cube in double2 steps of the whole grid, the wavefront adds its 64
// lanes by shuffles, the workgroup its four wavefronts through LDS.  The padded channels of the
// (HW, Dp) layout are read like the others: they hold zero residual, as k_chi2_map relies on.
// (elems = HW * Dp and Dp is always even, so the odd-element branches below cannot be reached
// through the C ABI and no test runs them; they keep the kernel right for any span.)
static __global__ __launch_bounds__(TEMPER_NT) void k_temper_energy(TemperChains C, size_t elems,
                                                                    double *__restrict__ partials) {
    __shared__ double part[TEMPER_NT / 64];
    const int r = blockIdx.y;
    const double *__restrict__ err = C.err[r];
    const double *__restrict__ ivar = C.ivar[r];
    const size_t nvec = elems >> 1;
    const size_t stride = (size_t)gridDim.x * TEMPER_NT;
    double a0 = 0.0, a1 = 0.0;
    if (ivar) {
        for (size_t i = (size_t)blockIdx.x * TEMPER_NT + threadIdx.x; i < nvec; i += stride) {
            const double2 e = *reinterpret_cast<const double2 *>(err + 2 * i);
            const double2 v = *reinterpret_cast<const double2 *>(ivar + 2 * i);
            a0 = fma(e.x * e.x, v.x, a0);
            a1 = fma(e.y * e.y, v.y, a1);
        }
        if ((elems & 1) && blockIdx.x == 0 && threadIdx.x == 0)
            a0 = fma(err[elems - 1] * err[elems - 1], ivar[elems - 1], a0);
    } else {
        for (size_t i = (size_t)blockIdx.x * TEMPER_NT + threadIdx.x; i < nvec; i += stride) {
            const double2 e = *reinterpret_cast<const double2 *>(err + 2 * i);
            a0 = fma(e.x, e.x, a0);
            a1 = fma(e.y, e.y, a1);
        }
        if ((elems & 1) && blockIdx.x == 0 && threadIdx.x == 0) a0 = fma(err[elems - 1], err[elems - 1], a0);
        a0 *= C.ivar_uniform[r];
        a1 *= C.ivar_uniform[r];
    }
    const double w = wave_sum(a0 + a1);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < TEMPER_NT / 64; ++k) t += part[k];
        partials[(size_t)r * gridDim.x + blockIdx.x] = 0.5 * t;
    }
}

// One workgroup.  Prologue: the block partials of every chain in a fixed order (lane-strided,
// shuffles), E_r = total_r / beta_r -- minus log L of state r under the untempered variance.  Then
// thread i decides pair (i, i + 1) where i has the round's parity, and thread r folds E_r -- of the
// state at rung r BEFORE the exchange -- into that rung's moments.
static __global__ __launch_bounds__(TEMPER_NT) void k_temper_decide(TemperChains C, TemperBlock T, int n, int nblk,
                                                                    long long round, uint64_t seed) {
#pragma clang fp contract(off)
    __shared__ double E[TEMPER_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < n; r += TEMPER_NT / 64) {
        double acc = 0.0;
        for (int b = lane; b < nblk; b += 64) acc += T.partials[(size_t)r * nblk + b];
        acc = wave_sum(acc);
        if (lane == 0) {
            const double e = acc / C.beta[r];
            E[r] = e;
            T.energy[r] = e;
        }
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i < n) {  // Welford, plain IEEE operations in this order
        const long long cnt = T.e_n[i] + 1;
        double mean = T.e_mean[i], m2 = T.e_m2[i];
        const double delta = E[i] - mean;
        mean += delta / (double)cnt;
        m2 += delta * (E[i] - mean);
        T.e_n[i] = cnt;
        T.e_mean[i] = mean;
        T.e_m2[i] = m2;
    }
    if (i < n - 1) {
        const int p = (int)(round & 1);
        if ((i & 1) != p) {
            T.decided[i] = -1;
            T.u[i] = __longlong_as_double(0x7ff8000000000000LL);
            T.logu[i] = __longlong_as_double(0x7ff8000000000000LL);
            return;
        }
        // the chains' streams always have a last counter word of 0: these never collide
        uint32_t w[4];
        philox4x32_10(0xFFFFFFFFu, (uint32_t)round, (uint32_t)i, 1u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        const double u = u64_to_unit(((uint64_t)w[1] << 32) | w[0]);
        const double logu = log(u);
        const double db = C.beta[i] - C.beta[i + 1];
        const double de = E[i] - E[i + 1];
        const double delta = db * de;
        const int ok = logu < delta ? 1 : 0;
        T.u[i] = u;
        T.logu[i] = logu;
        T.decided[i] = ok;
        T.attempts[i] += 1;
        if (ok) {
            T.accepts[i] += 1;
            const int l = T.labels[i];
            T.labels[i] = T.labels[i + 1];
            T.labels[i + 1] = l;
        }
    }
}

// a[0..n) <-> b[0..n) in 16-byte steps of the whole grid; an odd last element by one thread (the
// parameter map of an odd number of spaxels: HW * 3 odd; never the cube, whose Dp is even)
__device__ __forceinline__ void swap_span(double *__restrict__ a, double *__restrict__ b, size_t n, size_t tid,
                                          size_t stride) {
    const size_t nvec = n >> 1;
    for (size_t i = tid; i < nvec; i += stride) {
        const double2 x = *reinterpret_cast<const double2 *>(a + 2 * i);
        const double2 y = *reinterpret_cast<const double2 *>(b + 2 * i);
        *reinterpret_cast<double2 *>(a + 2 * i) = y;
        *reinterpret_cast<double2 *>(b + 2 * i) = x;
    }
    if ((n & 1) && tid == 0) {
        const double x = a[n - 1];
        a[n - 1] = b[n - 1];
        b[n - 1] = x;
    }
}

// blockIdx.y = ordinal of a proposed pair (i, i + 1), i = parity + 2 blockIdx.y.  An accepted pair
// trades the raw padded residual buffers and the parameter maps, nothing else: streaming, two
// cubes read and two written.
static __global__ __launch_bounds__(TEMPER_NT) void k_temper_exchange(TemperChains C, const int *__restrict__ decided,
                                                                      int parity, size_t cube_elems,
                                                                      size_t par_elems) {
    const int i = parity + 2 * (int)blockIdx.y;
    if (decided[i] != 1) return;
    const size_t tid = (size_t)blockIdx.x * TEMPER_NT + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * TEMPER_NT;
    swap_span(C.err[i], C.err[i + 1], cube_elems, tid, stride);
    swap_span(C.params[i], C.params[i + 1], par_elems, tid, stride);
}

}  // namespace d3d

struct d3d_temper {
    int n = 0, device = 0;
    std::vector<d3d_ctx *> ctxs;
    std::vector<double> betas;
    uint64_t seed = 0;
    int64_t rounds = 0;
    size_t cube_elems = 0, par_elems = 0;
    int nblk = 0;     // workgroups per chain of k_temper_energy
    int xblk = 0;     // workgroups per pair of k_temper_exchange
    void *dev = nullptr;  // the group's one device block
    d3d::TemperBlock T = {};
    hipEvent_t done = nullptr;  // end of the last round on the leader's stream
};

namespace {

// For the duration of a round every context runs on the leader's stream (flush_pending launches
// on c->stream); on every way out each is back on its own.
struct StreamScope {
    d3d_temper *t;
    std::vector<hipStream_t> own;
    ~StreamScope() {
        for (size_t r = 0; r < own.size(); ++r) t->ctxs[r]->stream = own[r];
    }
};

void fill_chains(const d3d_temper *t, d3d::TemperChains &C) {
    memset(&C, 0, sizeof C);
    for (int r = 0; r < t->n; ++r) {
        const d3d_ctx *c = t->ctxs[r];
        C.err[r] = c->slot[D3D_SLOT_ERR];
        C.ivar[r] = c->ivar_is_uniform ? nullptr : c->slot[D3D_SLOT_IVAR];
        C.ivar_uniform[r] = c->ivar_uniform;
        C.params[r] = c->params;
        C.beta[r] = t->betas[r];
    }
}

}  // namespace

// The three launches of one round on the leader's stream (d3d_temper_swap has validated the group
// and written the pending layers back).
int d3dh::temper_round(d3d_temper *t, int64_t round) {
    d3d_ctx *L = t->ctxs[0];
    d3d::TemperChains C;
    fill_chains(t, C);
    hipLaunchKernelGGL(d3d::k_temper_energy, dim3((unsigned)t->nblk, (unsigned)t->n), dim3(d3d::TEMPER_NT), 0,
                       L->stream, C, t->cube_elems, t->T.partials);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(d3d::k_temper_decide, dim3(1), dim3(d3d::TEMPER_NT), 0, L->stream, C, t->T, t->n, t->nblk,
                       (long long)round, t->seed);
    HIP_TRY(hipGetLastError());
    const int parity = (int)(round & 1);
    const int pairs = (t->n - parity) / 2;  // pairs (i, i + 1), i = parity, parity + 2, ..., i + 1 < n
    if (pairs > 0) {
        hipLaunchKernelGGL(d3d::k_temper_exchange, dim3((unsigned)t->xblk, (unsigned)pairs), dim3(d3d::TEMPER_NT), 0,
                           L->stream, C, (const int *)t->T.decided, parity, t->cube_elems, t->par_elems);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" {

int d3d_temper_create(d3d_temper **out, d3d_ctx **ctxs, int n, const double *betas, uint64_t seed) {
    NEED(out && ctxs && betas, D3D_ERR_INVALID, "NULL argument");
    *out = nullptr;
    NEED(n >= 2 && n <= d3d::TEMPER_MAX, D3D_ERR_INVALID, "a tempering group has 2 to %d rungs, got %d",
         d3d::TEMPER_MAX, n);
    NEED(betas[0] == 1.0, D3D_ERR_INVALID, "betas[0] must be 1 (rung 0 samples the posterior), got %g", betas[0]);
    for (int r = 0; r < n; ++r) {
        NEED(std::isfinite(betas[r]) && betas[r] > 0.0, D3D_ERR_INVALID, "betas[%d] = %g must be finite and > 0", r,
             betas[r]);
        NEED(r == 0 || betas[r] < betas[r - 1], D3D_ERR_INVALID,
             "betas must be strictly decreasing (betas[%d] = %g after %g)", r, betas[r], betas[r - 1]);
    }
    d3d_ctx *L = ctxs[0];
    for (int r = 0; r < n; ++r) {
        d3d_ctx *c = ctxs[r];
        NEED(c, D3D_ERR_INVALID, "ctx %d is NULL", r);
        for (int q = 0; q < r; ++q) NEED(ctxs[q] != c, D3D_ERR_INVALID, "ctx %d appears twice", r);
        NEED(c->have_taps && c->have_data, D3D_ERR_STATE, "ctx %d: taps/data not set", r);
        NEED(!c->tiled && c->parts.size() == 1 && !c->comm, D3D_ERR_UNSUPPORTED,
             "ctx %d is tiled or partitioned: tempered chains are whole cubes", r);
        NEED(c->ext_cap == 0, D3D_ERR_UNSUPPORTED,
             "ctx %d is driven by d3d_mh_colour_lines: its lines live on the host, tempering swaps device state", r);
        NEED(c->device == L->device && c->D == L->D && c->H == L->H && c->W == L->W && c->fh == L->fh &&
                 c->fw == L->fw,
             D3D_ERR_INVALID, "ctx %d: another device or shape than ctx 0", r);
        NEED(c->h_mask == L->h_mask && c->h_fsf == L->h_fsf && c->h_has_lsf == L->h_has_lsf &&
                 (!c->h_has_lsf || c->h_lsf == L->h_lsf) && c->h_thr == L->h_thr,
             D3D_ERR_INVALID, "ctx %d: another mask, FSF or LSF than ctx 0 (the rungs trade residuals)", r);
        bool same_line = c->line.K == L->line.K;
        for (int k = 0; k < d3d::LINE_KMAX; ++k)
            same_line = same_line && c->line.off[k] == L->line.off[k] && c->line.ratio[k] == L->line.ratio[k];
        same_line = same_line && c->line.n == L->line.n && c->line.support == L->line.support &&
                    c->h_line_tab == L->h_line_tab;
        NEED(same_line, D3D_ERR_INVALID, "ctx %d: another line shape than ctx 0 (the rungs trade parameters)", r);
    }
    HIP_TRY(hipSetDevice(L->device));
    d3d_temper *t = new (std::nothrow) d3d_temper;
    NEED(t, D3D_ERR_HIP, "out of host memory");
    t->n = n;
    t->device = L->device;
    t->ctxs.assign(ctxs, ctxs + n);
    t->betas.assign(betas, betas + n);
    t->seed = seed;
    t->cube_elems = L->cube_elems;
    t->par_elems = (size_t)L->HW * 3;
    // a lane takes at least four 16-byte loads per buffer; 1024 workgroups fill the chip
    const size_t vecs = (t->cube_elems / 2 + d3d::TEMPER_NT * 4 - 1) / (d3d::TEMPER_NT * 4);
    t->nblk = (int)std::min<size_t>(std::max<size_t>(vecs, 1), 1024);
    t->xblk = (int)std::min<size_t>(std::max<size_t>(vecs, 1), 2048);
    // the device block, in 8-byte words: doubles | 64-bit counters | 32-bit flags and labels
    const size_t nd = (size_t)n * t->nblk + n + 2 * (size_t)(n - 1) + 2 * (size_t)n;
    const size_t nl = 2 * (size_t)(n - 1) + n;
    const size_t ni = (size_t)(n - 1) + n;
    const size_t bytes = (nd + nl) * 8 + ni * 4;
    hipError_t e = hipMalloc(&t->dev, bytes);
    if (e == hipSuccess) e = hipMemset(t->dev, 0, bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->done, hipEventDisableTiming);
    double *d = static_cast<double *>(t->dev);
    t->T.partials = d;
    d += (size_t)n * t->nblk;
    t->T.energy = d;
    d += n;
    t->T.u = d;
    d += n - 1;
    t->T.logu = d;
    d += n - 1;
    t->T.e_mean = d;
    d += n;
    t->T.e_m2 = d;
    d += n;
    long long *l = reinterpret_cast<long long *>(d);
    t->T.attempts = l;
    l += n - 1;
    t->T.accepts = l;
    l += n - 1;
    t->T.e_n = l;
    l += n;
    int *w = reinterpret_cast<int *>(l);
    t->T.decided = w;
    w += n - 1;
    t->T.labels = w;
    if (e == hipSuccess) {
        std::vector<int> init(ni, -1);
        for (int r = 0; r < n; ++r) init[(n - 1) + r] = r;
        e = hipMemcpy(t->T.decided, init.data(), ni * sizeof(int), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        if (t->done) (void)hipEventDestroy(t->done);
        if (t->dev) (void)hipFree(t->dev);
        delete t;
        HIP_TRY(e);
    }
    *out = t;
    return D3D_OK;
}

int d3d_temper_swap(d3d_temper *t, int64_t round) {
    NEED(t, D3D_ERR_INVALID, "group is NULL");
    NEED(round >= 0, D3D_ERR_INVALID, "negative round %lld", (long long)round);
    d3d_ctx *L = t->ctxs[0];
    for (int r = 0; r < t->n; ++r) {
        const d3d_ctx *c = t->ctxs[r];
        NEED(c->have_taps && c->have_data && c->have_params, D3D_ERR_STATE, "ctx %d: taps/data/parameters not set", r);
        NEED(c->err_valid, D3D_ERR_STATE,
             "ctx %d has no valid carried residual (d3d_residual, or a sweep, makes one): nothing to exchange", r);
        NEED(c->cube_elems == t->cube_elems && (size_t)c->HW * 3 == t->par_elems, D3D_ERR_STATE,
             "ctx %d changed shape since the group was made", r);
    }
    HIP_TRY(hipSetDevice(t->device));
    StreamScope scope = {t};
    for (int r = 0; r < t->n; ++r) {
        d3d_ctx *c = t->ctxs[r];
        HIP_TRY(hipStreamSynchronize(c->stream));
        scope.own.push_back(c->stream);
        c->stream = L->stream;
    }
    for (int r = 0; r < t->n; ++r)
        if (int rc = d3dh::flush_pending(t->ctxs[r])) return rc;
    if (int rc = d3dh::temper_round(t, round)) return rc;
    // what the other contexts enqueue next on their own streams waits for the exchange (on the
    // device: the host goes on)
    HIP_TRY(hipEventRecord(t->done, L->stream));
    for (int r = 1; r < t->n; ++r)
        if (scope.own[r] != L->stream) HIP_TRY(hipStreamWaitEvent(scope.own[r], t->done, 0));
    // as d3d_set_params: the proposal table was made from the parameters a rung held before
    for (int r = 0; r < t->n; ++r) t->ctxs[r]->props_sweep = -1;
    ++t->rounds;
    return D3D_OK;
}

int d3d_temper_get(d3d_temper *t, int64_t *rounds, int64_t *attempts, int64_t *accepts, int64_t *energy_n,
                   double *energy_mean, double *energy_m2, int32_t *labels) {
    NEED(t, D3D_ERR_INVALID, "group is NULL");
    HIP_TRY(hipSetDevice(t->device));
    hipStream_t s = t->ctxs[0]->stream;
    const size_t n = (size_t)t->n;
    if (attempts) HIP_TRY(hipMemcpyAsync(attempts, t->T.attempts, (n - 1) * 8, hipMemcpyDeviceToHost, s));
    if (accepts) HIP_TRY(hipMemcpyAsync(accepts, t->T.accepts, (n - 1) * 8, hipMemcpyDeviceToHost, s));
    if (energy_n) HIP_TRY(hipMemcpyAsync(energy_n, t->T.e_n, n * 8, hipMemcpyDeviceToHost, s));
    if (energy_mean) HIP_TRY(hipMemcpyAsync(energy_mean, t->T.e_mean, n * 8, hipMemcpyDeviceToHost, s));
    if (energy_m2) HIP_TRY(hipMemcpyAsync(energy_m2, t->T.e_m2, n * 8, hipMemcpyDeviceToHost, s));
    if (labels) HIP_TRY(hipMemcpyAsync(labels, t->T.labels, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (rounds) *rounds = t->rounds;
    return D3D_OK;
}

int d3d_temper_last(d3d_temper *t, double *energy, double *u, double *logu, int32_t *decided) {
    NEED(t, D3D_ERR_INVALID, "group is NULL");
    NEED(t->rounds > 0, D3D_ERR_STATE, "no exchange round yet");
    HIP_TRY(hipSetDevice(t->device));
    hipStream_t s = t->ctxs[0]->stream;
    const size_t n = (size_t)t->n;
    if (energy) HIP_TRY(hipMemcpyAsync(energy, t->T.energy, n * 8, hipMemcpyDeviceToHost, s));
    if (u) HIP_TRY(hipMemcpyAsync(u, t->T.u, (n - 1) * 8, hipMemcpyDeviceToHost, s));
    if (logu) HIP_TRY(hipMemcpyAsync(logu, t->T.logu, (n - 1) * 8, hipMemcpyDeviceToHost, s));
    if (decided) HIP_TRY(hipMemcpyAsync(decided, t->T.decided, (n - 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return D3D_OK;
}

int d3d_temper_destroy(d3d_temper *t) {
    if (!t) return D3D_OK;
    (void)hipSetDevice(t->device);
    (void)hipEventSynchronize(t->done);  // (a round may still be running)
    if (t->done) (void)hipEventDestroy(t->done);
    if (t->dev) (void)hipFree(t->dev);
    delete t;
    return D3D_OK;
}

}  // extern "C"
