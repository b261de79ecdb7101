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
// whole == 0 (patch exchange, d3d_temper_set_patch): the energies and their moments only; every pair's
// whole-cube record reads "not proposed".
static __global__ __launch_bounds__(TEMPER_NT) void k_temper_decide(TemperChains C, TemperBlock T, int n, int nblk,
                                                                    long long round, uint64_t seed, int whole) {
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
        if ((i & 1) != p || !whole) {
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


// ---- exchange of PATCHES of spaxels (d3d_temper_set_patch) ------------------------------------
// The field is cut into tiles of p x p spaxels from a per-round origin; a tile's unmasked spaxels
// are one patch.  Rungs i and j = i + 1 propose to trade the parameters of the patch; with
// delta = sum_{s in P} [contribution(s, x_i[s]) - contribution(s, x_j[s])] (supported on the tile
// dilated by the FSF) the residuals become e_i + delta and e_j - delta, and the log ratio is local.

// The LSF-convolved lines of every rung of a proposed pair, (HW, Dp), zero at masked spaxels:
// launch_lines into the rung's SLOT_TMP0 once per round (a spaxel lies in one tile, a tile in one
// colour, so the lines of a round's start serve all of its colours).
struct PatchLines {
    const double *lines[TEMPER_MAX];
};

struct PatchBlock {
    double *terms;   // [n-1][ntiles][5]
    double *u, *logu;  // [n-1][ntiles]
    int *decided;    // [n-1][ntiles]
    unsigned long long *attempts, *accepts;  // [n-1] patch totals
};

struct PatchArgs {
    int D, Dp, H, W, fh, fw;
    int p, oy, ox, nty, ntx, my, mx;
    int cy, cx, nkx;  // the launch's colour; tiles of that colour along x
    int parity, prior;
    double lam[3];
    long long round;
    uint64_t seed;
    const double *fsf;
    const uint8_t *mask;
    PatchBlock B;
};

static __global__ __launch_bounds__(TEMPER_NT) void k_patch_clear(PatchBlock B, long nrec) {
    const long r = (long)blockIdx.x * TEMPER_NT + threadIdx.x;
    if (r >= nrec) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int k = 0; k < 5; ++k) B.terms[r * 5 + k] = nan;
    B.u[r] = nan;
    B.logu[r] = nan;
    B.decided[r] = -1;
}

struct PatchTile {
    int ty0, ty1, tx0, tx1;  // the tile, clipped to the field
    int fy0, fy1, fx0, fx1;  // its footprint: dilated by the FSF's half sizes, clipped
};

// Eight wavefronts per tile, two per SIMD (a colour of 300 x 300 spaxels at p = 10 is 240 workgroups,
// one per CU at most).  Sixteen leave 64 architectural registers a lane and spill 43.
constexpr int PATCH_NT = 512;
// The staged form: the tile's line differences of one z-block in LDS, a wavefront along z.  Tiles of
// up to PATCH_LDS_SPAXELS spaxels (60 KiB of static LDS beside the reduction's) take it; larger ones
// read the two line cubes through the caches.
constexpr int PATCH_ZB = 64;
constexpr int PATCH_UNROLL = 4;
constexpr int PATCH_LDS_SPAXELS = 120;

// delta at voxel (y, x, z): the tile's line differences through the FSF, sources row-major.  A
// contribution at (sy + dy, sx + dx) carries fsf[fhh + dy, fhw + dx].  One IEEE operation per step,
// and the staged difference is the same subtraction: the deciding pass, the updating pass and both
// forms get the same bits.
template <bool STAGED>
__device__ __forceinline__ double patch_delta(const PatchArgs &A, const PatchTile &T, const double *__restrict__ Li,
                                              const double *__restrict__ Lj, const double *dl, int y, int x, int z,
                                              int zz) {
#pragma clang fp contract(off)
    const int fhh = (A.fh - 1) / 2, fhw = (A.fw - 1) / 2;
    const int sy0 = max(T.ty0, y - fhh), sy1 = min(T.ty1, y + fhh + 1);
    const int sx0 = max(T.tx0, x - fhw), sx1 = min(T.tx1, x + fhw + 1);
    const int tw = T.tx1 - T.tx0;
    double d = 0.0;
    for (int sy = sy0; sy < sy1; ++sy) {
        const double *__restrict__ frow = A.fsf + (size_t)(fhh + y - sy) * A.fw + (fhw + x);
        for (int sx = sx0; sx < sx1; ++sx) {
            double v;
            if constexpr (STAGED) {
                v = dl[((sy - T.ty0) * tw + (sx - T.tx0)) * PATCH_ZB + zz];
            } else {
                const size_t o = ((size_t)sy * A.W + sx) * A.Dp + z;
                v = Li[o] - Lj[o];
            }
            d += frow[-sx] * v;
        }
    }
    return d;
}

// One walk over the footprint in z-blocks of PATCH_ZB channels: a wavefront takes one footprint
// spaxel at a time with its lanes along z, so every load of residual, 1/variance and lines is
// coalesced and the spaxel -- with it the FSF taps and the bounds of the source loop -- is the
// same in all lanes (scalar loads, no divergence).  UPDATE = false: the four sums into acc, per
// thread in the order of its spaxels.  UPDATE = true: delta into both residuals.  (The caller has a
// barrier between two walks: the staging of the second does not overtake the first's reads.)
template <bool STAGED, bool UPDATE>
__device__ __forceinline__ void patch_walk(const PatchArgs &A, const PatchTile &T, double *__restrict__ ei,
                                           double *__restrict__ ej, const double *__restrict__ vi,
                                           const double *__restrict__ vj, const double *__restrict__ Li,
                                           const double *__restrict__ Lj, double *dl, double acc[5]) {
#pragma clang fp contract(off)
    const int tw = T.tx1 - T.tx0, nsp = (T.ty1 - T.ty0) * tw;
    const int fwid = T.fx1 - T.fx0, nf = (T.fy1 - T.fy0) * fwid;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nzb = (A.D + PATCH_ZB - 1) / PATCH_ZB;
    for (int zb = 0; zb < nzb; ++zb) {
        const int z0 = zb * PATCH_ZB;
        const int zn = min(PATCH_ZB, A.D - z0);
        if constexpr (STAGED) {
            if (zb) __syncthreads();
            for (int q = threadIdx.x; q < nsp * PATCH_ZB; q += PATCH_NT) {
                const int s = q / PATCH_ZB, zz = q - s * PATCH_ZB;
                const size_t o = ((size_t)(T.ty0 + s / tw) * A.W + T.tx0 + s % tw) * A.Dp + z0 + zz;
                dl[q] = (zz < zn) ? Li[o] - Lj[o] : 0.0;
            }
            __syncthreads();
        }
        // PATCH_UNROLL spaxels per step, their loads first: a tile's workgroup has a CU to itself, and
        // one spaxel's loads per wavefront in flight leave the walk waiting for memory
        for (int f0 = wave; f0 < nf; f0 += PATCH_UNROLL * (PATCH_NT / 64)) {
            double e_i[PATCH_UNROLL], e_j[PATCH_UNROLL], w_i[PATCH_UNROLL], w_j[PATCH_UNROLL];
#pragma unroll
            for (int k = 0; k < PATCH_UNROLL; ++k) {
                const int f = f0 + k * (PATCH_NT / 64);
                if (f < nf && lane < zn) {
                    const size_t o = ((size_t)(T.fy0 + f / fwid) * A.W + T.fx0 + f % fwid) * A.Dp + z0 + lane;
                    e_i[k] = ei[o];
                    e_j[k] = ej[o];
                    if constexpr (!UPDATE) {
                        w_i[k] = vi ? vi[o] : 1.0;
                        w_j[k] = vj ? vj[o] : 1.0;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < PATCH_UNROLL; ++k) {
                const int f = f0 + k * (PATCH_NT / 64);
                if (f < nf && lane < zn) {
                    const int y = T.fy0 + f / fwid, x = T.fx0 + f % fwid, z = z0 + lane;
                    const double d = patch_delta<STAGED>(A, T, Li, Lj, dl, y, x, z, lane);
                    if constexpr (UPDATE) {
                        const size_t o = ((size_t)y * A.W + x) * A.Dp + z;
                        ei[o] = e_i[k] + d;
                        ej[o] = e_j[k] - d;
                    } else {
                        acc[0] += w_i[k] * (e_i[k] * d);
                        acc[1] += w_j[k] * (e_j[k] * d);
                        acc[2] += w_i[k] * (d * d);
                        acc[3] += w_j[k] * (d * d);
                    }
                }
            }
        }
    }
}

// One workgroup per (tile of the launch's colour, proposed pair): blockIdx.x = the tile's ordinal
// among those of its colour, blockIdx.y = the pair's.  Pass 1 walks the footprint and sums e_i delta,
// e_j delta and the two delta^2 per thread, per wavefront by shuffles, per workgroup through LDS: a
// fixed order.  Thread 0 adds the prior's term, draws u and decides.  Pass 2, accepted tiles only:
// delta again into both residuals, then the patch's parameters trade places.  Footprints of one
// colour are disjoint and, with a prior on (FSFs of three spaxels and more), the tiles not adjacent.
template <bool STAGED>
static __global__ __launch_bounds__(PATCH_NT) void k_temper_patch(TemperChains C, PatchLines Ls, PatchArgs A) {
#pragma clang fp contract(off)
    __shared__ double dl[STAGED ? PATCH_LDS_SPAXELS * PATCH_ZB : 1];
    __shared__ double red[PATCH_NT / 64][5];
    __shared__ int s_ok;
    const int ky = (int)blockIdx.x / A.nkx, kx = (int)blockIdx.x - ky * A.nkx;
    const int ty = A.cy + ky * A.my, tx = A.cx + kx * A.mx;
    const int i = A.parity + 2 * (int)blockIdx.y, j = i + 1;
    const int fhh = (A.fh - 1) / 2, fhw = (A.fw - 1) / 2;
    PatchTile T;
    T.ty0 = max(0, ty * A.p - A.p + A.oy);
    T.ty1 = min(A.H, ty * A.p + A.oy);
    T.tx0 = max(0, tx * A.p - A.p + A.ox);
    T.tx1 = min(A.W, tx * A.p + A.ox);
    if (T.ty0 >= T.ty1 || T.tx0 >= T.tx1) return;  // (the first row or column of tiles under a zero shift)
    T.fy0 = max(0, T.ty0 - fhh);
    T.fy1 = min(A.H, T.ty1 + fhh);
    T.fx0 = max(0, T.tx0 - fhw);
    T.fx1 = min(A.W, T.tx1 + fhw);
    const int tw = T.tx1 - T.tx0, nsp = (T.ty1 - T.ty0) * tw;
    if (STAGED && nsp > PATCH_LDS_SPAXELS) return;  // (the host picks the form from the largest tile: never taken)
    int live = 0;
    for (int s = threadIdx.x; s < nsp; s += PATCH_NT)
        live |= A.mask[(size_t)(T.ty0 + s / tw) * A.W + T.tx0 + s % tw] != 0;
    if (!__syncthreads_or(live)) return;  // no unmasked spaxel: not proposed (k_patch_clear's record stands)

    double *__restrict__ ei = C.err[i], *__restrict__ ej = C.err[j];
    const double *__restrict__ vi = C.ivar[i], *__restrict__ vj = C.ivar[j];
    const double *__restrict__ Li = Ls.lines[i], *__restrict__ Lj = Ls.lines[j];
    double *__restrict__ pi = C.params[i], *__restrict__ pj = C.params[j];
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    patch_walk<STAGED, false>(A, T, ei, ej, vi, vj, Li, Lj, dl, acc);
    if (A.prior) {  // the pairs <s, t> with s in the patch, t an unmasked 4-neighbour outside the tile
        for (int q = threadIdx.x; q < 4 * nsp; q += PATCH_NT) {
            const int s = q >> 2, dir = q & 3;
            const int sy = T.ty0 + s / tw, sx = T.tx0 + s % tw;
            const int ny = sy + (dir == 0 ? -1 : dir == 1 ? 1 : 0), nx = sx + (dir == 2 ? -1 : dir == 3 ? 1 : 0);
            if (ny < 0 || ny >= A.H || nx < 0 || nx >= A.W) continue;
            if (ny >= T.ty0 && ny < T.ty1 && nx >= T.tx0 && nx < T.tx1) continue;
            const size_t so = (size_t)sy * A.W + sx, to = (size_t)ny * A.W + nx;
            if (!A.mask[so] || !A.mask[to]) continue;
            for (int k = 0; k < 3; ++k) {
                const double xis = pi[so * 3 + k], xjs = pj[so * 3 + k];
                const double xit = pi[to * 3 + k], xjt = pj[to * 3 + k];
                const double a = xjs - xit, b = xis - xit, c = xis - xjt, e = xjs - xjt;
                acc[4] += A.lam[k] * (((a * a - b * b) + c * c) - e * e);
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double w = wave_sum(acc[k]);
        if (lane == 0) red[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double v = 0.0;
            for (int w = 0; w < PATCH_NT / 64; ++w) v += red[w][k];
            t[k] = v;
        }
        const double si = vi ? 1.0 : C.ivar_uniform[i], sj = vj ? 1.0 : C.ivar_uniform[j];
        t[0] = si * t[0];
        t[1] = sj * t[1];
        t[2] = 0.5 * (si * t[2]);
        t[3] = 0.5 * (sj * t[3]);
        t[4] = -0.5 * t[4];
        const int tile = ty * A.ntx + tx;
        uint32_t w[4];
        philox4x32_10(0xFFFFFFFFu, (uint32_t)A.round, (uint32_t)i, 2u + (uint32_t)tile, (uint32_t)A.seed,
                      (uint32_t)(A.seed >> 32), w);
        const double u = u64_to_unit(((uint64_t)w[1] << 32) | w[0]);
        const double logu = log(u);
        const double delta = (-(t[0] + t[2]) - (t[3] - t[1])) + t[4];
        const int ok = logu < delta ? 1 : 0;
        const size_t rec = (size_t)i * A.nty * A.ntx + tile;
#pragma unroll
        for (int k = 0; k < 5; ++k) A.B.terms[rec * 5 + k] = t[k];
        A.B.u[rec] = u;
        A.B.logu[rec] = logu;
        A.B.decided[rec] = ok;
        atomicAdd(A.B.attempts + i, 1ull);  // (integer totals: any order gives the same)
        if (ok) atomicAdd(A.B.accepts + i, 1ull);
        s_ok = ok;
    }
    __syncthreads();
    if (!s_ok) return;
    patch_walk<STAGED, true>(A, T, ei, ej, vi, vj, Li, Lj, dl, acc);
    for (int q = threadIdx.x; q < 3 * nsp; q += PATCH_NT) {
        const int s = q / 3, k = q - 3 * s;
        const size_t so = (size_t)(T.ty0 + s / tw) * A.W + T.tx0 + s % tw;
        if (!A.mask[so]) continue;
        const double a = pi[so * 3 + k];
        pi[so * 3 + k] = pj[so * 3 + k];
        pj[so * 3 + k] = a;
    }
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
    DevBuf<char> dev;     // the group's one device block
    d3d::TemperBlock T = {};
    hipEvent_t done = nullptr;  // end of the last round on the leader's stream
    // exchange of patches (d3d_temper_set_patch): nothing allocated before the first such round
    int patch = 0;               // 0: whole cubes
    DevBuf<unsigned long long> pcount;  // [2][n-1] patch attempts | accepts
    DevBuf<char> prec;           // the per-tile record of the last round, 7 * 8 + 4 bytes per pair and tile
    d3d::PatchBlock P = {};
    int pgeom[6] = {0, 0, 0, 0, 0, 0};  // oy, ox, nty, ntx, my, mx of the last patch round
    bool plast = false;          // the last round was a patch round
};

namespace {
// the live groups (d3d_temper_create .. d3d_temper_destroy): ctx_is_tempered looks a context up
std::mutex live_mutex;
std::vector<const d3d_temper *> live_groups;
}  // namespace

namespace d3dh {
bool ctx_is_tempered(const d3d_ctx *c) {
    std::lock_guard<std::mutex> lock(live_mutex);
    for (const d3d_temper *t : live_groups)
        if (std::find(t->ctxs.begin(), t->ctxs.end(), c) != t->ctxs.end()) return true;
    return false;
}
}  // namespace d3dh

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

// Philox4x32-10 on the host (the round's origin shift is launch geometry): d3d_rng.h's function.
void philox_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)m1;
        c3 = (uint32_t)m0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// The patch block for `nrec` records per pair (grown, never shrunk); the counters once.
int ensure_patch_block(d3d_temper *t, size_t nrec) {
    const size_t np = (size_t)t->n - 1;
    if (!t->pcount) {
        HIP_TRY(t->pcount.alloc(2 * np));
        HIP_TRY(hipMemsetAsync(t->pcount, 0, 2 * np * 8, t->ctxs[0]->stream));
        t->P.attempts = t->pcount;
        t->P.accepts = t->P.attempts + np;
    }
    const size_t bytes = np * nrec * (7 * 8 + 4);
    if (bytes > t->prec.size() && t->prec) HIP_TRY(hipStreamSynchronize(t->ctxs[0]->stream));
    HIP_TRY(t->prec.reserve(bytes));
    // (laid out for this round's record count: d3d_temper_last_patches reads it the same way)
    double *d = reinterpret_cast<double *>(t->prec.get());
    t->P.terms = d;
    d += np * nrec * 5;
    t->P.u = d;
    d += np * nrec;
    t->P.logu = d;
    d += np * nrec;
    t->P.decided = reinterpret_cast<int *>(d);
    return 0;
}

// One patch round on the leader's stream: the energies and their moments (no whole-cube decision),
// the lines of the rungs of the proposed pairs, the cleared record, one launch per tile colour.
int patch_round(d3d_temper *t, int64_t round) {
    d3d_ctx *L = t->ctxs[0];
    const int n = t->n, p = t->patch, H = L->H, W = L->W;
    d3d::TemperChains C;
    fill_chains(t, C);
    hipLaunchKernelGGL(d3d::k_temper_energy, dim3((unsigned)t->nblk, (unsigned)n), dim3(d3d::TEMPER_NT), 0, L->stream,
                       C, t->cube_elems, t->T.partials);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(d3d::k_temper_decide, dim3(1), dim3(d3d::TEMPER_NT), 0, L->stream, C, t->T, n, t->nblk,
                       (long long)round, t->seed, 0);
    HIP_TRY(hipGetLastError());
    uint32_t w[4];
    philox_host(0xFFFFFFFEu, (uint32_t)round, 0u, 1u, (uint32_t)t->seed, (uint32_t)(t->seed >> 32), w);
    const int oy = (int)(w[0] % (uint32_t)p), ox = (int)(w[1] % (uint32_t)p);
    const int nty = (H - 1 + p - oy) / p + 1, ntx = (W - 1 + p - ox) / p + 1;
    const int my = 1 + (L->fh - 1 + p - 1) / p, mx = 1 + (L->fw - 1 + p - 1) / p;
    const int g[6] = {oy, ox, nty, ntx, my, mx};
    memcpy(t->pgeom, g, sizeof g);
    const size_t nrec = (size_t)nty * ntx;
    if (int rc = ensure_patch_block(t, nrec)) return rc;
    const long all = (long)((size_t)(n - 1) * nrec);
    hipLaunchKernelGGL(d3d::k_patch_clear, dim3((unsigned)((all + d3d::TEMPER_NT - 1) / d3d::TEMPER_NT)),
                       dim3(d3d::TEMPER_NT), 0, L->stream, t->P, all);
    HIP_TRY(hipGetLastError());
    const int parity = (int)(round & 1);
    const int pairs = (n - parity) / 2;
    if (pairs <= 0) return 0;
    d3d::PatchLines Ls;
    memset(&Ls, 0, sizeof Ls);
    for (int r = parity; r < parity + 2 * pairs; ++r) {
        d3d_ctx *c = t->ctxs[r];
        if (int rc = d3dh::launch_lines(c, c->slot[D3D_SLOT_TMP0], 1)) return rc;
        Ls.lines[r] = c->slot[D3D_SLOT_TMP0];
    }
    d3d::PatchArgs A;
    memset(&A, 0, sizeof A);
    A.D = L->D;
    A.Dp = L->Dp;
    A.H = H;
    A.W = W;
    A.fh = L->fh;
    A.fw = L->fw;
    A.p = p;
    A.oy = oy;
    A.ox = ox;
    A.nty = nty;
    A.ntx = ntx;
    A.my = my;
    A.mx = mx;
    A.parity = parity;
    A.prior = L->prior.on && (L->prior.lam[0] != 0.0 || L->prior.lam[1] != 0.0 || L->prior.lam[2] != 0.0);
    for (int k = 0; k < 3; ++k) A.lam[k] = L->prior.on ? L->prior.lam[k] : 0.0;
    A.round = (long long)round;
    A.seed = t->seed;
    A.fsf = L->fsf;
    A.mask = L->mask;
    A.B = t->P;
    // the staged form where the largest tile's line differences of a z-block fit its LDS
    const bool staged = std::min(p, H) * (long)std::min(p, W) <= d3d::PATCH_LDS_SPAXELS;
    for (int cy = 0; cy < my; ++cy)
        for (int cx = 0; cx < mx; ++cx) {
            const int nky = (nty - cy + my - 1) / my, nkx = (ntx - cx + mx - 1) / mx;
            if (nky <= 0 || nkx <= 0) continue;
            A.cy = cy;
            A.cx = cx;
            A.nkx = nkx;
            if (staged)
                hipLaunchKernelGGL(d3d::k_temper_patch<true>, dim3((unsigned)(nky * nkx), (unsigned)pairs),
                                   dim3(d3d::PATCH_NT), 0, L->stream, C, Ls, A);
            else
                hipLaunchKernelGGL(d3d::k_temper_patch<false>, dim3((unsigned)(nky * nkx), (unsigned)pairs),
                                   dim3(d3d::PATCH_NT), 0, L->stream, C, Ls, A);
            HIP_TRY(hipGetLastError());
        }
    return 0;
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
                       (long long)round, t->seed, 1);
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
        NEED(!c->noise.on, D3D_ERR_UNSUPPORTED,
             "ctx %d: noise scales are armed (d3d_noise_begin): a rung's variance / beta is not rescaled with them", r);
        NEED(!c->extbuf, D3D_ERR_UNSUPPORTED,
             "ctx %d is driven by d3d_mh_colour_lines: its lines live on the host, tempering swaps device state", r);
        const char *const differs = d3dh::setup_differs(c, L);
        NEED(!differs, D3D_ERR_INVALID, "ctx %d: another %s than ctx 0 (the rungs trade residuals and parameters)", r,
             differs);
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
    hipError_t e = t->dev.alloc(bytes);
    if (e == hipSuccess) e = hipMemset(t->dev, 0, bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->done, hipEventDisableTiming);
    double *d = reinterpret_cast<double *>(t->dev.get());
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
        delete t;
        HIP_TRY(e);
    }
    {
        std::lock_guard<std::mutex> lock(live_mutex);
        live_groups.push_back(t);
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
    if (t->patch > 0) {
        for (int r = 1; r < t->n; ++r) {
            const d3d_ctx *c = t->ctxs[r];
            bool same = c->prior.on == L->prior.on;
            for (int k = 0; k < 3; ++k) same = same && (!c->prior.on || c->prior.lam[k] == L->prior.lam[k]);
            NEED(same, D3D_ERR_INVALID,
                 "ctx %d: another smoothness prior than ctx 0 (the prior's term of a patch exchange cancels "
                 "only between rungs of one prior)", r);
        }
        if (int rc = patch_round(t, round)) return rc;
    } else if (int rc = d3dh::temper_round(t, round)) {
        return rc;
    }
    t->plast = t->patch > 0;
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

int d3d_temper_set_patch(d3d_temper *t, int p) {
    NEED(t, D3D_ERR_INVALID, "group is NULL");
    NEED(p >= 0 && p <= (1 << 24), D3D_ERR_INVALID,
         "patch size %d: 0 (whole cubes) or the side of a tile in spaxels, 2^24 at most", p);
    t->patch = p;
    return D3D_OK;
}

int d3d_temper_last_patches(d3d_temper *t, int32_t geometry[6], double *terms, double *u, double *logu,
                            int32_t *decided) {
    NEED(t, D3D_ERR_INVALID, "group is NULL");
    NEED(t->rounds > 0 && t->plast, D3D_ERR_STATE, "the last round (if any) exchanged no patches");
    HIP_TRY(hipSetDevice(t->device));
    hipStream_t s = t->ctxs[0]->stream;
    if (geometry)
        for (int k = 0; k < 6; ++k) geometry[k] = t->pgeom[k];
    const size_t nrec = (size_t)(t->n - 1) * t->pgeom[2] * t->pgeom[3];
    if (terms) HIP_TRY(hipMemcpyAsync(terms, t->P.terms, nrec * 5 * 8, hipMemcpyDeviceToHost, s));
    if (u) HIP_TRY(hipMemcpyAsync(u, t->P.u, nrec * 8, hipMemcpyDeviceToHost, s));
    if (logu) HIP_TRY(hipMemcpyAsync(logu, t->P.logu, nrec * 8, hipMemcpyDeviceToHost, s));
    if (decided) HIP_TRY(hipMemcpyAsync(decided, t->P.decided, nrec * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return D3D_OK;
}

int d3d_temper_get_patches(d3d_temper *t, int64_t *attempts, int64_t *accepts) {
    NEED(t, D3D_ERR_INVALID, "group is NULL");
    const size_t np = (size_t)t->n - 1;
    if (!t->pcount) {  // no patch round yet
        if (attempts) memset(attempts, 0, np * 8);
        if (accepts) memset(accepts, 0, np * 8);
        return D3D_OK;
    }
    HIP_TRY(hipSetDevice(t->device));
    hipStream_t s = t->ctxs[0]->stream;
    if (attempts) HIP_TRY(hipMemcpyAsync(attempts, t->P.attempts, np * 8, hipMemcpyDeviceToHost, s));
    if (accepts) HIP_TRY(hipMemcpyAsync(accepts, t->P.accepts, np * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return D3D_OK;
}

int d3d_temper_destroy(d3d_temper *t) {
    if (!t) return D3D_OK;
    (void)hipSetDevice(t->device);
    (void)hipEventSynchronize(t->done);  // (a round may still be running)
    if (t->done) (void)hipEventDestroy(t->done);
    {
        std::lock_guard<std::mutex> lock(live_mutex);
        live_groups.erase(std::remove(live_groups.begin(), live_groups.end(), t), live_groups.end());
    }
    delete t;  // every DevBuf of the group
    return D3D_OK;
}

}  // extern "C"
