// C ABI of libdeconv3d_hip.so -- see include/deconv3d_hip.h.
// Host-side context, device memory, options, halo exchange.  What can be decided without a device is
// decided in host-only headers, each proved by a stand-alone program on the CPU, and only executed
// here: the work lists and every part's launch forms (d3d_worklists.h -> build_colour_lists), the
// forms of the taps (d3d_taps.h -> set_taps_impl).  gfx950 only.
#include "d3d_ctx.h"

#include <dlfcn.h>

#define D3D_VERSION 300  // 0.3.0
#ifndef D3D_SOURCE_HASH
#define D3D_SOURCE_HASH "unknown"
#endif

namespace {
thread_local std::string g_err;
}

namespace d3dh {
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

d3d_worklists::Input worklist_input(const d3d_ctx *c) {
    d3d_worklists::Input in;
    in.H = c->H;
    in.W = c->W;
    in.Dp = c->Dp;
    in.fh = c->fh;
    in.fw = c->fw;
    in.gy0 = c->gy0;
    in.gx0 = c->gx0;
    in.owned = {c->oy0, c->oy1, c->ox0, c->ox1};
    in.tiled = c->tiled;
    in.part_rects = c->part_rects.data();
    in.part_phase = c->part_phase.data();
    in.n_part_rects = (int)c->part_rects.size();
    in.mask = c->h_mask.data();
    in.flow_grid = c->flow_grid;
    in.cube_elems = c->cube_elems;
    in.ws_max_dp = d3d::MH_WS_MAX_DP;
    in.mh_zb = c->mh_zb;
    in.deep = c->deep;
    in.mh_defer = c->mh_defer;
    in.mh_layers_cfg = c->mh_layers_cfg;
    in.mh_layers_forced = c->mh_layers_forced;
    in.mh_zigzag = c->mh_zigzag;
    in.mh_wide = c->mh_wide;
    in.mh_small = c->mh_small;
    in.mh_props = c->mh_props;
    in.strips_opt = c->mh_strips_opt;
    in.strip_order_opt = c->mh_strip_order_opt;
    in.chain_opt = c->mh_chain_opt != 0;
    in.flow = c->mh_flow != 0;
    in.pair = c->mh_pair != 0;
    in.uniform = c->ivar_is_uniform && c->uniform_fast_path;
    return in;
}
}  // namespace d3dh

using d3dh::fail;
using namespace d3dh;

namespace {
// RCCL is loaded at run time (the library stays loadable without it, and a process
// that already holds an RCCL -- torch's -- shares that one: same soname).
struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;

int next_pow2_ref(int depth) {
    // lib/convolution.py:137-141: 2 ** len(bin(depth-1)[:-1] + '0')
    unsigned v = (unsigned)(depth - 1);
    int bits = 0;
    do {
        ++bits;
        v >>= 1;
    } while (v);
    return 1 << bits;
}

}  // namespace

namespace {

using namespace d3d;

int to_device_layout(d3d_ctx *c, const double *src_stage, double *dst) {
    dim3 grid((unsigned)((c->HW + 31) / 32), (unsigned)((c->Dp + 31) / 32));
    hipLaunchKernelGGL(d3d::k_to_device_layout, grid, dim3(256), 0, c->stream, src_stage, dst, c->D,
                       c->Dp, c->HW);
    HIP_TRY(hipGetLastError());
    return 0;
}

int to_host_layout(d3d_ctx *c, const double *src, double *dst_stage) {
    dim3 grid((unsigned)((c->HW + 31) / 32), (unsigned)((c->Dp + 31) / 32));
    hipLaunchKernelGGL(d3d::k_to_host_layout, grid, dim3(256), 0, c->stream, src, dst_stage, c->D,
                       c->Dp, c->HW);
    HIP_TRY(hipGetLastError());
    return 0;
}

int upload_cube(d3d_ctx *c, const double *host, double *dst) {
    const size_t bytes = (size_t)c->D * c->HW * sizeof(double);
    HIP_TRY(hipMemcpyAsync(c->stage, host, bytes, hipMemcpyHostToDevice, c->stream));
    return to_device_layout(c, c->stage, dst);
}

int download_cube(d3d_ctx *c, const double *src, double *host) {
    const size_t bytes = (size_t)c->D * c->HW * sizeof(double);
    int rc = to_host_layout(c, src, c->stage);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(host, c->stage, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// Choose the MH workgroup: NT threads, window kept in MAXIT double2 registers
// per thread (0 = window re-read from memory in pass 2).
void pick_mh_geometry(d3d_ctx *c) {
    const int npos = c->fh * c->fw;
    int need = c->N > c->Dp ? c->N : c->Dp;
    const int nt_env = c->mh_nt_opt, mi_env = c->mh_maxit_opt;
    // Measured on MI355X (300x300x128, 11x11): small workgroups that re-read
    // the err window in pass 2 (MAXIT = 0) beat register-resident windows --
    // 6 workgroups per CU overlap each other's load / reduce / store phases.
    const int cands[3] = {256, 512, 1024};
    int nt = 1024;
    for (int k = 0; k < 3; ++k)
        if (cands[k] >= need && cands[k] / c->HL >= 1) {
            nt = cands[k];
            break;
        }
    if ((nt_env == 128 || nt_env == 256 || nt_env == 512 || nt_env == 1024) && nt_env >= need)
        nt = nt_env;
    const int G = nt / c->HL;
    const int iters = (npos + G - 1) / G;
    int maxit = 0;
    if ((mi_env == 4 || mi_env == 8 || mi_env == 16 || mi_env == 32) && mi_env >= iters)
        maxit = mi_env;
    c->mh_nt = nt;
    c->mh_maxit = maxit;
    // (mh_defer -- 0: immediate write-back, 1: deferred + wave-specialised, 2: deferred, plain)
    // measured crossover on MI355X (256 MiB Infinity Cache): 276 / 323 MB +1 %, 369 MB +6 %,
    // 230 MB -7 % (tools/mh_sizes.py)
    // The write-through residual stores of that variant address the residual through a raw
    // buffer of the WINDOW (32-bit byte offsets from its first cell: (fh + 1) rows of the cube
    // must span < 2 GiB -- every cube this library takes; round 3 used one buffer over the whole
    // slot and switched the policy off for residuals >= 2 GiB, e.g. a full MUSE cube).
    const bool fits_raw = 8.0 * (double)c->Dp * (double)(c->fh + 1) * (double)c->W < 2147483648.0;
    c->mh_nt_ivar = 16.0 * (double)c->Dp * (double)c->H * (double)c->W >= 350e6;
    if (c->mh_nt_ivar_opt >= 0) c->mh_nt_ivar = c->mh_nt_ivar_opt != 0;
    c->mh_nt_ivar = c->mh_nt_ivar && fits_raw;
    // pending layers of k_mh_ws: the 3-layer kernel stages 4*Dp G values per layer in
    // two registers per thread (Dp <= 160), the 2-layer one in four (Dp <= 256); the
    // other MH kernels keep one layer
    c->mh_layers_forced = c->mh_layers_opt > 0;
    c->mh_layers_cfg = c->mh_layers_forced ? c->mh_layers_opt : 2;
    if (c->mh_layers_cfg < 1) c->mh_layers_cfg = 1;
    if (c->mh_layers_cfg > d3d::MH_LAYERS) c->mh_layers_cfg = d3d::MH_LAYERS;
    if (c->Dp > 160 && c->mh_layers_cfg > 2) c->mh_layers_cfg = 2;
    // cubes deeper than k_mh_ws takes: its z-blocked form, when the LSF taps lie within +-8
    // channels (every Gaussian / MUSE-like LSF; unknown before d3d_set_taps: assumed)
    c->mh_defer = c->mh_defer_opt;
    c->mh_zb = c->mh_zblocks && c->Dp > d3d::MH_WS_MAX_DP && c->mh_defer == 1 && !c->mh_flow &&
               (!c->have_taps || c->ntaps == 0 || c->lsf_dense_any);
    if (c->mh_defer != 1 || c->mh_flow || (c->Dp > d3d::MH_WS_MAX_DP && !c->mh_zb)) c->mh_layers_cfg = 1;
    if (c->deep && !c->mh_zb) c->mh_defer = 0;  // k_mh_deep writes the residual back at once
    c->mh_layers = c->mh_layers_cfg;
}

// The kernels read a list entry as an int4 {y, x, real, -}: the upload is one copy of the vector.
static_assert(sizeof(d3d_worklists::Entry) == sizeof(int4) && offsetof(d3d_worklists::Entry, y) == offsetof(int4, x) &&
                  offsetof(d3d_worklists::Entry, x) == offsetof(int4, y) &&
                  offsetof(d3d_worklists::Entry, real) == offsetof(int4, z),
              "d3d_worklists::Entry is not laid out as an int4");

#ifdef D3D_EXPERIMENTS
// k_mh_chain: whole sweeps of a part in one launch of persistent workgroups, one per lattice slot
// -- where every slot is resident at once (one workgroup per CU) and a thread can hold its share of
// the window in registers.  The slot grid of every part, and the device tables of those that take it.
int chain_tables(d3d_ctx *c, const d3d_worklists::Input &in) {
    const int ncol = c->fh * c->fw;
    const int fhw = (c->fw - 1) / 2;
    size_t need_slots = 0, need_G = 0;
    std::vector<int2> cols((size_t)c->parts.size() * ncol, make_int2(0, 0));
    bool any = false;
    for (size_t pi = 0; pi < c->parts.size(); ++pi) {
        d3d_ctx::Part &pt = c->parts[pi];
        if (pt.y1 <= pt.y0 || pt.x1 <= pt.x0 || pt.K <= 0) continue;
        const int cus = c->flow_grid / 4;
        // slot grid over the window centres [dy0 - fhh, dy1 + fhh) x [.., dx1 + fhw), its
        // columns aligned with the colour order: slot column boundaries at the local
        // residue of colour cx = 0, so that a slot's window moves right by one column
        // per colour class along a row of colours
        int ly0, lx0;
        d3d_worklists::local_residue(in, 0, &ly0, &lx0);
        pt.chain_sx0 = (pt.dx0 - fhw) - ((((pt.dx0 - fhw) - lx0) % c->fw + c->fw) % c->fw);
        pt.n_sy = (pt.dy1 - pt.dy0 + 2 * c->fh - 2) / c->fh;
        pt.n_sx = (pt.dx1 + fhw - 1 - pt.chain_sx0) / c->fw + 1;
        // fw thread groups of HL threads hold the window's columns; + one deciding wavefront
        pt.chain_ns = c->fw * c->HL;
        const int nt = (pt.chain_ns + 63) / 64 * 64 + 64;
        const bool fh_ok = c->fh == 3 || c->fh == 5 || c->fh == 7 || c->fh == 9 || c->fh == 11;
        const double g_bytes = 4.0 * pt.K * pt.n_sy * pt.n_sx * c->Dp * 8.0;
        const size_t lds = d3d::mh_chain_lds_doubles(c->fw, c->Dp, c->N, ncol, pt.K, nt / 64 - 1) * 8;
        pt.chain = c->mh_chain_opt == 1 && c->mh_defer == 1 && c->Dp <= 256 && pt.layers == 1 &&
                   (long)pt.n_sy * pt.n_sx <= cus && fh_ok && c->fw >= 3 && nt <= MH_CHAIN_NT &&
                   c->Dp <= pt.chain_ns && lds <= (size_t)160 * 1024 && g_bytes <= 512e6 &&
                   c->cube_elems * sizeof(double) < (size_t(1) << 31);
        if (!pt.chain) continue;
        any = true;
        need_slots = std::max(need_slots, (size_t)pt.n_sy * pt.n_sx);
        need_G = std::max(need_G, (size_t)4 * pt.K * pt.n_sy * pt.n_sx * c->Dp);  // G rows | lines
        int k = 0;
        for (int col = 0; col < ncol; ++col)
            if (pt.real[col] > 0) {  // local residues of the (global) colour class
                int2 &r = cols[pi * ncol + k++];
                d3d_worklists::local_residue(in, col, &r.x, &r.y);
            }
    }
    if (any) {
        HIP_TRY(c->chain_cols.reserve(cols.size()));
        HIP_TRY(hipMemcpyAsync(c->chain_cols, cols.data(), cols.size() * sizeof(int2),
                               hipMemcpyHostToDevice, c->stream));
        if (2 * need_slots > c->chain_flags.size()) {
            HIP_TRY(c->chain_flags.alloc(2 * need_slots));
            HIP_TRY(hipMemsetAsync(c->chain_flags, 0, 2 * need_slots * sizeof(unsigned), c->stream));
            c->chain_base = 0;
        }
        HIP_TRY(c->chain_G.reserve(need_G));
        HIP_TRY(hipStreamSynchronize(c->stream));  // `cols` goes out of scope
    }
    return 0;
}

// tables of the dataflow kernel (unpartitioned contexts only): active colours in
// order, their ticket ranges, and per colour the map lattice point -> index in its list
int flow_tables(d3d_ctx *c, const std::vector<d3d_worklists::Entry> &list) {
    const int ncol = c->fh * c->fw;
    if (c->tiled || c->parts.size() != 1 || list.size() > c->flow_cap_items) return 0;
    const d3d_ctx::Part &pt = c->parts[0];
    std::vector<int4> ents, cols;
    std::vector<int> lat((size_t)ncol * c->flow_LY * c->flow_LX, -1);
    for (int col = 0; col < ncol; ++col) {
        if (pt.real[col] <= 0) continue;
        const int cy = col / c->fw, cx = col % c->fw;  // == local residues (not tiled)
        const int n_all = pt.off[col + 1] - pt.off[col];
        const int k = (int)cols.size();
        cols.push_back(make_int4((int)ents.size(), cy, cx, 0));
        for (int i = 0; i < n_all; ++i) {
            const d3d_worklists::Entry e = list[(size_t)pt.off[col] + i];
            const int iy = (e.y - cy) / c->fh + 1, ix = (e.x - cx) / c->fw + 1;
            if (iy < 0 || iy >= c->flow_LY || ix < 0 || ix >= c->flow_LX)
                return fail(D3D_ERR_HIP, "internal: lattice index out of range");
            lat[((size_t)k * c->flow_LY + iy) * c->flow_LX + ix] = i;
            ents.push_back(make_int4(e.y, e.x, e.real, k));
        }
        c->flow_last_cy = cy;
        c->flow_last_cx = cx;
    }
    c->flow_K = (int)cols.size();
    c->flow_items = (int)ents.size();
    c->flow_first.clear();
    c->flow_colour.clear();
    for (const int4 &cc : cols) {
        c->flow_first.push_back(cc.x);
        c->flow_colour.push_back(cc.y * c->fw + cc.z);
    }
    c->flow_first.push_back(c->flow_items);
    if (c->flow_K > 0) {
        HIP_TRY(hipMemcpyAsync(c->flow_ent, ents.data(), ents.size() * sizeof(int4),
                               hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->flow_col, cols.data(), cols.size() * sizeof(int4),
                               hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->flow_lat, lat.data(),
                               (size_t)c->flow_K * c->flow_LY * c->flow_LX * sizeof(int),
                               hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // the host vectors go out of scope
    }
    return 0;
}
#endif

// The work lists of every (part, colour class) and what every part's colour launches run as:
// d3d_worklists.h builds and decides; here they go to the device, with the tables of the
// experimental kernels, which read the finished lists.
int build_colour_lists(d3d_ctx *c) {
    const d3d_worklists::Input in = worklist_input(c);
    std::vector<d3d_worklists::Entry> list;
    list.reserve(c->spx.size());
    if (d3d_worklists::build(in, &c->parts, &list, &c->colour_real, &c->n_phases))
        return fail(D3D_ERR_HIP, "internal: lattice row outside the strips");
#ifdef D3D_EXPERIMENTS
    if (int rc = chain_tables(c, in)) return rc;
#endif
    c->mh_layers = 1;
    for (const d3d_ctx::Part &pt : c->parts) c->mh_layers = std::max(c->mh_layers, pt.layers);
    HIP_TRY(c->spx.reserve(list.size()));
    c->flow_K = 0;
    c->flow_items = 0;
    c->flow_last_cy = c->flow_last_cx = -1;
#ifdef D3D_EXPERIMENTS
    if (int rc = flow_tables(c, list)) return rc;
#endif
    if (!list.empty())
        HIP_TRY(hipMemcpyAsync(c->spx, list.data(), list.size() * sizeof(int4),
                               hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    pend_clear(c);
    c->props_sweep = -1;
    return 0;
}

// ---- per-spaxel jump scales (d3d_adapt_*) and the smoothness prior (d3d_prior_*) ----------
void adapt_free(d3d_ctx *c) {
    c->adapt = {};
    c->props_sweep = -1;  // (a table made with the scales)
}

// The kernels that make proposals from parameters they keep to themselves across sweeps
// (EXPERIMENTS builds) never see a scale map change: refused with adaptation on.
int adapt_kernels_ok(const d3d_ctx *c) {
    NEED(!c->mh_chain_opt && !c->mh_flow && !c->mh_pair, D3D_ERR_UNSUPPORTED,
         "per-spaxel jump scales (d3d_adapt_begin) with option %s: k_mh_chain, k_mh_flow and k_mh_pair "
         "keep their proposals' inputs across sweeps",
         c->mh_chain_opt ? "mh_chain" : c->mh_flow ? "mh_flow" : "mh_pair");
    return 0;
}

// The smoothness prior reads a spaxel's neighbours as they are when it is decided.  That holds
// where a launch decides ONE colour class from the parameters in memory: the kernels that decide
// several classes in a launch, or keep parameters on chip across colours (EXPERIMENTS builds),
// and the contexts whose parts or tiles run beside each other are refused, never ignored.
int prior_kernels_ok(const d3d_ctx *c) {
    NEED(!c->mh_chain_opt && !c->mh_flow && !c->mh_pair, D3D_ERR_UNSUPPORTED,
         "smoothness prior (d3d_prior_begin) with option %s: k_mh_chain, k_mh_flow and k_mh_pair decide "
         "more than one colour class in a launch",
         c->mh_chain_opt ? "mh_chain" : c->mh_flow ? "mh_flow" : "mh_pair");
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED,
         "smoothness prior on a tile: the neighbours across its edge belong to other ranks");
    NEED(c->part_rects.size() <= 1 && c->parts.size() <= 1, D3D_ERR_UNSUPPORTED,
         "smoothness prior on a context cut into %zu parts (d3d_set_parts): parts of one phase are "
         "not ordered against each other", std::max(c->part_rects.size(), c->parts.size()));
    return 0;
}

}  // namespace

int d3dh::download_device_cube(d3d_ctx *c, const double *src, double *host) { return download_cube(c, src, host); }

const char *d3dh::setup_differs(const d3d_ctx *c, const d3d_ctx *L) {
    if (!(c->device == L->device && c->D == L->D && c->H == L->H && c->W == L->W && c->fh == L->fh && c->fw == L->fw))
        return "device or shape";
    if (!(c->h_mask == L->h_mask && c->h_fsf == L->h_fsf && c->h_has_lsf == L->h_has_lsf &&
          (!c->h_has_lsf || c->h_lsf == L->h_lsf) && c->h_thr == L->h_thr))
        return "mask, FSF or LSF";
    bool same_line = c->line.K == L->line.K;
    for (int k = 0; k < d3d::LINE_KMAX; ++k)
        same_line = same_line && c->line.off[k] == L->line.off[k] && c->line.ratio[k] == L->line.ratio[k];
    // (and the table: where chains share a launch the leader's device copy serves every one)
    same_line = same_line && c->line.n == L->line.n && c->line.support == L->line.support && c->h_line_tab == L->h_line_tab;
    return same_line ? nullptr : "line shape";
}

// ---- variance rescaling (d3d_ctx::Rescale) ----------------------------------------------------
d3dh::RescaleName d3dh::rescale_name(const d3d_ctx *c) {
    static const RescaleName names[] = {{"no rescalers", "none"}, {"robust weights", "robust"}, {"noise scales", "noise"}};
    return names[c->rescale.who];
}

int d3dh::rescale_free_for(const d3d_ctx *c, d3d_ctx::Rescale::Who who) {
    NEED(!c->rescale.who || c->rescale.who == who, D3D_ERR_UNSUPPORTED,
         "%s are armed (d3d_%s_begin): both rewrite SLOT_IVAR from the base cube; d3d_%s_end first", rescale_name(c).what,
         rescale_name(c).api, rescale_name(c).api);
    return 0;
}

int d3dh::rescale_arm(d3d_ctx *c, d3d_ctx::Rescale::Who who, int every, int64_t start) {
    if (int rc = rescale_free_for(c, who)) return rc;
    rescale_disarm(c, who);  // (held already: the base cube first goes back)
    const size_t bytes = c->cube_elems * sizeof(double);
    hipError_t e = c->rescale.i0.alloc(c->cube_elems);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->rescale.i0, c->slot[D3D_SLOT_IVAR], bytes, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the context stays usable for the chain of known variance
        c->rescale = {};
        return fail(D3D_ERR_HIP, "the base 1/variance (a cube of %zu bytes): %s", bytes, hipGetErrorString(e));
    }
    c->rescale.who = who;
    c->rescale.every = every;
    c->rescale.start = start;
    c->rescale.was_uniform = c->ivar_is_uniform;
    c->ivar_is_uniform = false;  // the slot is read from now on (bit-identical while it holds the base cube)
    return 0;
}

void d3dh::rescale_disarm(d3d_ctx *c, d3d_ctx::Rescale::Who who) {
    if (!who || c->rescale.who != who) return;
    (void)hipMemcpyAsync(c->slot[D3D_SLOT_IVAR], c->rescale.i0, c->cube_elems * sizeof(double), hipMemcpyDeviceToDevice,
                         c->stream);
    (void)hipStreamSynchronize(c->stream);
    c->ivar_is_uniform = c->rescale.was_uniform;
    c->rescale = {};
}

bool d3dh::rescale_due(const d3d_ctx *c, int s) {
    if (!c->rescale.who) return false;
    const int64_t rs = (int64_t)s + (int64_t)c->sweep_origin;
    return rs >= c->rescale.start && (rs - c->rescale.start) % c->rescale.every == 0;
}

int d3dh::rescale_after_sweep(d3d_ctx *c, int s) {
    if (!rescale_due(c, s)) return 0;
    const int64_t rs = (int64_t)s + (int64_t)c->sweep_origin;
    return c->rescale.who == d3d_ctx::Rescale::ROBUST ? robust_draw(c, rs) : noise_draw(c, rs);
}

namespace {

// ---- per-context options (d3d_ctx_set_option) -----------------------------------------
// Every switch of the library is a field of the context.  The environment is only the
// source of a new context's DEFAULTS (D3D_<KEY>, read once in d3d_ctx_create), so two
// contexts of one process can run with different settings.  kind: what has to be
// re-derived when the option changes.
enum OptKind { OPT_LAUNCH = 0, OPT_MH = 1, OPT_TAPS = 2 };
struct OptDesc {
    const char *key, *env;
    int d3d_ctx::*field;
    OptKind kind;
    int lo, hi;
};
const OptDesc g_opts[] = {
    {"mh_defer", "D3D_MH_DEFER", &d3d_ctx::mh_defer_opt, OPT_MH, 0, 2},
    {"mh_zblocks", "D3D_MH_ZBLOCKS", &d3d_ctx::mh_zblocks, OPT_MH, 0, 1},
    {"mh_layers", "D3D_MH_LAYERS", &d3d_ctx::mh_layers_opt, OPT_MH, 0, d3d::MH_LAYERS},
    {"mh_wide", "D3D_MH_WIDE", &d3d_ctx::mh_wide, OPT_MH, 0, 1},
    {"mh_props", "D3D_MH_PROPS", &d3d_ctx::mh_props, OPT_LAUNCH, 0, 1},
    {"mh_small", "D3D_MH_SMALL", &d3d_ctx::mh_small, OPT_MH, 0, 2},
    {"halo_timing", "D3D_HALO_TIMING", &d3d_ctx::halo_timing, OPT_LAUNCH, 0, 1},
    {"mh_zigzag", "D3D_MH_ZIGZAG", &d3d_ctx::mh_zigzag, OPT_MH, 0, 1},
    {"mh_nt_ivar", "D3D_MH_NT_IVAR", &d3d_ctx::mh_nt_ivar_opt, OPT_MH, -1, 1},
    {"mh_strips", "D3D_MH_STRIPS", &d3d_ctx::mh_strips_opt, OPT_MH, 0, d3d_strips::MAX_STRIPS},
    {"mh_strip_order", "D3D_MH_STRIP_ORDER", &d3d_ctx::mh_strip_order_opt, OPT_MH, 0, 2},
    {"mh_strip_lag", "D3D_MH_STRIP_LAG", &d3d_ctx::mh_strip_lag, OPT_LAUNCH, 0, d3d_strips::MAX_STRIPS},
    {"mh_nt", "D3D_MH_NT", &d3d_ctx::mh_nt_opt, OPT_MH, 0, 1024},
    {"uniform_ivar", "D3D_UNIFORM_IVAR", &d3d_ctx::uniform_fast_path, OPT_MH, 0, 1},
    {"conv_rows", "D3D_CONV_ROWS", &d3d_ctx::conv_rows, OPT_LAUNCH, 0, 1},
    {"conv_zb", "D3D_CONV_ZB", &d3d_ctx::conv_zb, OPT_LAUNCH, 0, 1},
    {"conv_hy", "D3D_CONV_HY", &d3d_ctx::conv_hy_opt, OPT_LAUNCH, 0, 1 << 20},
    {"spatial_sep", "D3D_SPATIAL_SEP", &d3d_ctx::spatial_sep, OPT_TAPS, 0, 1},
    {"sep_fuse", "D3D_SEP_FUSE", &d3d_ctx::sep_fuse, OPT_LAUNCH, 0, 1},
    {"spatial_mode", "D3D_SPATIAL_MODE", &d3d_ctx::march_mode, OPT_LAUNCH, 0, 3},
    {"march_hy", "D3D_MARCH_HY", &d3d_ctx::march_hy_opt, OPT_TAPS, 0, 1 << 20},
    {"zmajor", "D3D_ZMAJOR", &d3d_ctx::zmajor, OPT_LAUNCH, 0, 1},
    {"zmajor_hy", "D3D_ZMAJOR_HY", &d3d_ctx::zmajor_hy, OPT_LAUNCH, 0, 1 << 20},
    {"spectral_dense", "D3D_SPECTRAL_DENSE", &d3d_ctx::spectral_dense, OPT_LAUNCH, 0, 1},
    {"spectral_blocks", "D3D_SPECTRAL_BLOCKS", &d3d_ctx::spectral_blocks, OPT_LAUNCH, 0, 1},
    {"lines_dense", "D3D_LINES_DENSE", &d3d_ctx::lines_dense, OPT_LAUNCH, 0, 3},
    {"lines_rounds", "D3D_LINES_ROUNDS", &d3d_ctx::lines_rounds, OPT_LAUNCH, 0, 64},
    {"spatial_nt", "D3D_SPATIAL_NT", &d3d_ctx::sp_nt_opt, OPT_LAUNCH, 0, 1024},
    {"xcd_remap", "D3D_XCD_REMAP", &d3d_ctx::xcd_remap, OPT_LAUNCH, 0, 1},
    {"alt_dir", "D3D_ALT_DIR", &d3d_ctx::alt_dir, OPT_LAUNCH, 0, 1},
    {"stagger", "D3D_STAGGER", &d3d_ctx::stagger, OPT_LAUNCH, 0, 1 << 20},
    {"post_nt", "D3D_POST_NT", &d3d_ctx::post_nt, OPT_LAUNCH, 0, 1},
    {"noise_timing", "D3D_NOISE_TIMING", &d3d_ctx::noise_timing, OPT_LAUNCH, 0, 1},
#ifdef D3D_EXPERIMENTS
    // measured-but-not-faster variants of DESIGN.md section 3 (make EXPERIMENTS=1)
    {"mh_chain", "D3D_MH_CHAIN", &d3d_ctx::mh_chain_opt, OPT_MH, 0, 1},
    {"mh_prio", "D3D_MH_PRIO", &d3d_ctx::mh_prio, OPT_LAUNCH, 0, 255},
    {"mh_maxit", "D3D_MH_MAXIT", &d3d_ctx::mh_maxit_opt, OPT_MH, -1, 32},
    {"mh_flow", "D3D_MH_FLOW", &d3d_ctx::mh_flow, OPT_MH, 0, 1},
    {"mh_pair", "D3D_MH_PAIR", &d3d_ctx::mh_pair, OPT_MH, 0, 1},
    {"spectral_shfl", "D3D_SPECTRAL_SHFL", &d3d_ctx::spectral_shfl, OPT_LAUNCH, 0, 1},
    {"fuse_lsf", "D3D_FUSE_LSF", &d3d_ctx::fuse_lsf, OPT_TAPS, 0, 1},
    {"march_pf", "D3D_MARCH_PF", &d3d_ctx::march_pf, OPT_LAUNCH, 0, 3},
    {"march_one", "D3D_MARCH_ONE", &d3d_ctx::march_one, OPT_LAUNCH, 0, 3},
    {"march_stamp", "D3D_STAMP", &d3d_ctx::march_stamp, OPT_LAUNCH, 0, 1},
#endif
};

const OptDesc *find_opt(const char *key) {
    for (const OptDesc &o : g_opts)
        if (!strcmp(o.key, key)) return &o;
    return nullptr;
}

bool opt_value_ok(const OptDesc &o, long v) {
    if (v < o.lo || v > o.hi) return false;
    if (!strcmp(o.key, "mh_nt")) return v == 0 || v == 128 || v == 256 || v == 512 || v == 1024;
    if (!strcmp(o.key, "spatial_nt")) return v == 0 || v == 256 || v == 512 || v == 1024;
    if (!strcmp(o.key, "mh_maxit")) return v == -1 || v == 0 || v == 4 || v == 8 || v == 16 || v == 32;
    return true;
}

// defaults of a new context from the environment (out-of-range values are ignored)
void options_from_env(d3d_ctx *c) {
    for (const OptDesc &o : g_opts)
        if (const char *e = getenv(o.env)) {
            const long v = atol(e);
            if (opt_value_ok(o, v)) c->*(o.field) = (int)v;
        }
    if (getenv("D3D_NO_ZMAJOR")) c->zmajor = 0;  // (the round-1 spelling)
}

}  // namespace

extern "C" {

int d3d_version(void) { return D3D_VERSION; }

const char *d3d_source_hash(void) { return D3D_SOURCE_HASH; }

const char *d3d_last_error(void) { return g_err.c_str(); }

int d3d_device_count(int *count) {
    NEED(count, D3D_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return D3D_OK;
}

int d3d_ctx_create(d3d_ctx **out, int device, int D, int H, int W, int fh, int fw) {
    NEED(out, D3D_ERR_INVALID, "ctx is NULL");
    *out = nullptr;
    NEED(D >= 1 && H >= 1 && W >= 1, D3D_ERR_INVALID, "cube shape (%d,%d,%d) must be positive", D,
         H, W);
    // lib/run.py:210-211
    NEED(fh >= 1 && fw >= 1 && (fh & 1) && (fw & 1), D3D_ERR_INVALID,
         "FSF *must* be of odd dimensions, got (%d,%d)", fh, fw);
    NEED((long)H * W < (1L << 31) - 1, D3D_ERR_UNSUPPORTED, "too many spaxels");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(D3D_ERR_NO_DEVICE,
                    "no HIP device available: libdeconv3d_hip has no CPU fallback");
    }
    NEED(device >= 0 && device < n, D3D_ERR_INVALID, "device %d out of range (%d visible)", device,
         n);
    HIP_TRY(hipSetDevice(device));

    d3d_ctx *c = new (std::nothrow) d3d_ctx();
    NEED(c, D3D_ERR_HIP, "out of host memory");
    c->device = device;
    c->D = D;
    c->H = H;
    c->W = W;
    c->fh = fh;
    c->fw = fw;
    c->Dp = (D + 1) & ~1;
    c->HL = c->Dp / 2;
    c->N = next_pow2_ref(D);
    c->HW = (long)H * W;
    c->cube_elems = (size_t)c->HW * c->Dp;
    if (c->N > d3d::MH_DEEP_MAX || c->Dp > d3d::MH_DEEP_MAX) {
        delete c;
        return fail(D3D_ERR_UNSUPPORTED, "spectral depth %d exceeds the kernels' limit of %d", D,
                    d3d::MH_DEEP_MAX);
    }
    c->deep = c->N > 1024 || c->Dp > 1024;
    c->sp_nt = pick_nt(c->HL);
    options_from_env(c);
    pick_mh_geometry(c);

#define CTX_TRY(expr)                                                                 \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                       \
            d3d_ctx_destroy(c);                                                       \
            return fail(D3D_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));  \
        }                                                                             \
    } while (0)
    CTX_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    CTX_TRY(hipEventCreate(&c->ev0));
    CTX_TRY(hipEventCreate(&c->ev1));
    for (int s = 0; s < D3D_SLOT_COUNT; ++s) {
        CTX_TRY(c->slot[s].alloc(c->cube_elems));
        CTX_TRY(hipMemsetAsync(c->slot[s], 0, c->cube_elems * sizeof(double), c->stream));
    }
    CTX_TRY(c->stage.alloc((size_t)D * c->HW));
    CTX_TRY(c->stage2.alloc((size_t)D * c->HW));
    CTX_TRY(c->params.alloc((size_t)c->HW * 3));
    CTX_TRY(c->params_alt.alloc((size_t)c->HW * 3));
    CTX_TRY(c->mask.alloc((size_t)c->HW));
    CTX_TRY(c->fsf.alloc((size_t)fh * fw));
    CTX_TRY(c->sep_uv.alloc((size_t)(fh + fw)));
    CTX_TRY(c->fsf_quad.alloc((size_t)fh * fw));
    CTX_TRY(c->fsf_quad_sep.alloc((size_t)fh * fw));
    CTX_TRY(c->lsf_shift.alloc((size_t)c->N));
    CTX_TRY(c->lsf_weight.alloc((size_t)c->N));
    CTX_TRY(c->lsf_dense.alloc((2 * d3d::LSF_RL + 1)));
    CTX_TRY(c->dlog.alloc((size_t)c->HW));
    CTX_TRY(c->hwbuf.alloc((size_t)c->HW));
    CTX_TRY(c->scal.alloc(16));
    CTX_TRY(c->accepted.alloc(1));
    CTX_TRY(c->acc_map.alloc((size_t)c->HW));
    CTX_TRY(c->spx.alloc((size_t)(H + 2 * fh) * (W + 2 * fw)));
    c->slots_x = (W + fw - 1) / fw;
    c->slots = c->slots_x * ((H + fh - 1) / fh);
    c->Wg = W;
    c->oy1 = H;
    c->ox1 = W;
    CTX_TRY(c->prev.alloc((size_t)c->HW * 3));
    CTX_TRY(c->recbuf.alloc((size_t)c->HW * 8));
    CTX_TRY(c->idxbuf.alloc((size_t)c->HW));
    for (int b = 0; b < 4; ++b) {
        CTX_TRY(c->gbuf[b].alloc((size_t)c->slots * c->Dp));
        CTX_TRY(hipMemsetAsync(c->gbuf[b], 0, (size_t)c->slots * c->Dp * sizeof(double), c->stream));
    }
    {
#ifdef D3D_EXPERIMENTS
        const size_t ncol = (size_t)fh * fw;
        c->flow_LY = H / fh + 3;
        c->flow_LX = W / fw + 3;
        c->flow_cap_K = ncol;
        c->flow_cap_items = c->spx.size();
        CTX_TRY(c->flow_ent.alloc(c->spx.size()));
        CTX_TRY(c->flow_col.alloc(ncol));
        CTX_TRY(c->flow_lat.alloc(ncol * c->flow_LY * c->flow_LX));
        c->flow_state_bytes = ((4 + ncol + c->spx.size()) * sizeof(unsigned) + 15) / 16 * 16;
        CTX_TRY(c->flow_state.alloc(c->flow_state_bytes / sizeof(unsigned)));
        CTX_TRY(c->pair_state.alloc((4 + c->spx.size())));
        CTX_TRY(hipMemsetAsync(c->pair_state, 0, (4 + c->spx.size()) * sizeof(unsigned), c->stream));
#endif
        CTX_TRY(c->flow_err.alloc(4));
        CTX_TRY(hipMemsetAsync(c->flow_err, 0, 16, c->stream));
        int cus = 0;
        CTX_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        c->flow_grid = 4 * (cus > 0 ? cus : 256);
    }
    CTX_TRY(hipMemsetAsync(c->dlog, 0, (size_t)c->HW * sizeof(double), c->stream));
    CTX_TRY(hipMemsetAsync(c->accepted, 0, sizeof(unsigned long long), c->stream));
    CTX_TRY(hipMemsetAsync(c->acc_map, 0, (size_t)c->HW * sizeof(unsigned), c->stream));
    CTX_TRY(hipMemsetAsync(c->mask, 1, (size_t)c->HW, c->stream));
    CTX_TRY(hipStreamSynchronize(c->stream));
#undef CTX_TRY
    c->h_mask.assign((size_t)c->HW, 1);
    c->h_user_mask.assign((size_t)c->HW, 1);
    *out = c;
    return D3D_OK;
}

int d3d_ctx_destroy(d3d_ctx *c) {
    if (!c) return D3D_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    c->comm = nullptr;
    for (int b = 0; b < d3d_ctx::STREAM_NB; ++b) {
        if (c->snap_host[b]) (void)hipHostFree(c->snap_host[b]);
        if (c->snap_ready[b]) (void)hipEventDestroy(c->snap_ready[b]);
        if (c->snap_done[b]) (void)hipEventDestroy(c->snap_done[b]);
    }
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (int a = 0; a < d3d_ctx::STRIP_AUX; ++a) {
        if (c->strip_stream[a]) (void)hipStreamDestroy(c->strip_stream[a]);
        if (c->strip_join[a]) (void)hipEventDestroy(c->strip_join[a]);
    }
    if (c->strip_fork) (void)hipEventDestroy(c->strip_fork);
    for (hipEvent_t e : c->strip_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->halo_ev) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;  // every DevBuf of the context
    return D3D_OK;
}

int d3d_ctx_set_stream(d3d_ctx *c, void *hip_stream) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return D3D_OK;
}

int d3d_sync(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_timer_start(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    return D3D_OK;
}

int d3d_timer_stop(d3d_ctx *c, double *ms) {
    NEED(c && ms, D3D_ERR_INVALID, "NULL argument");
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, c->ev0, c->ev1));
    *ms = (double)f;
    return D3D_OK;
}

static int set_taps_impl(d3d_ctx *c, const double *fsf, const double *lsf, double thr);

int d3d_set_taps(d3d_ctx *c, const double *fsf, const double *lsf, double thr) {
    NEED(c && fsf, D3D_ERR_INVALID, "NULL argument");
    // host copies: an option that changes the analysis of the taps redoes it from these
    c->h_fsf.assign(fsf, fsf + (size_t)c->fh * c->fw);
    c->h_has_lsf = lsf != nullptr;
    if (lsf) c->h_lsf.assign(lsf, lsf + c->D);
    c->h_thr = thr;
    if (int rc = set_taps_impl(c, c->h_fsf.data(), c->h_has_lsf ? c->h_lsf.data() : nullptr, thr)) return rc;
    return post_reset(c);  // moments over two instrument models mean nothing
}

int d3d_ctx_set_option(d3d_ctx *c, const char *key, long value) {
    NEED(c && key, D3D_ERR_INVALID, "NULL argument");
    const OptDesc *o = find_opt(key);
    NEED(o, D3D_ERR_INVALID, "unknown option '%s'", key);
    NEED(opt_value_ok(*o, value), D3D_ERR_INVALID, "option %s: value %ld out of range", key, value);
    if (c->*(o->field) == (int)value) return D3D_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (c->adapt.on && value != 0 &&
        (!strcmp(key, "mh_chain") || !strcmp(key, "mh_flow") || !strcmp(key, "mh_pair")))
        return fail(D3D_ERR_UNSUPPORTED,
                    "option %s with per-spaxel jump scales on (d3d_adapt_begin): the kernel keeps its "
                    "proposals' inputs across sweeps", key);
    if (c->prior.on && value != 0 &&
        (!strcmp(key, "mh_chain") || !strcmp(key, "mh_flow") || !strcmp(key, "mh_pair")))
        return fail(D3D_ERR_UNSUPPORTED,
                    "option %s with the smoothness prior on (d3d_prior_begin): the kernel decides more "
                    "than one colour class in a launch", key);
    if (o->kind == OPT_MH)  // pending layers belong to the old kernel selection
        if (int rc = flush_pending(c)) return rc;
    c->*(o->field) = (int)value;
    if (o->kind == OPT_MH) {
        pick_mh_geometry(c);
        if (c->have_data) return build_colour_lists(c);
    } else if (o->kind == OPT_TAPS && c->have_taps) {
        return set_taps_impl(c, c->h_fsf.data(), c->h_has_lsf ? c->h_lsf.data() : nullptr, c->h_thr);
    }
    return D3D_OK;
}

int d3d_ctx_get_option(d3d_ctx *c, const char *key, long *value) {
    NEED(c && key && value, D3D_ERR_INVALID, "NULL argument");
    if (!strcmp(key, "chain_parts")) {  // read-only: parts whose sweeps run as ONE launch (k_mh_chain)
        long n = 0;
        for (const d3d_ctx::Part &pt : c->parts) n += pt.chain ? 1 : 0;
        *value = c->have_data ? n : 0;
        return D3D_OK;
    }
    if (!strcmp(key, "search_bank_ns") || !strcmp(key, "search_kernel_ns")) {  // read-only: the last d3d_line_search
        *value = key[7] == 'b' ? c->search_bank_ns : c->search_kernel_ns;
        return D3D_OK;
    }
    if (!strcmp(key, "prep_median_ns") || !strcmp(key, "prep_stats_ns")) {  // read-only: the last d3d_prepare etc.
        *value = key[5] == 'm' ? c->prep_median_ns : c->prep_stats_ns;
        return D3D_OK;
    }
    if (!strcmp(key, "noise_sums_ns") || !strcmp(key, "noise_draw_ns") || !strcmp(key, "noise_apply_ns")) {
        *value = c->noise_ns[key[6] == 's' ? 0 : key[6] == 'd' ? 1 : 2];  // read-only: the last timed d3d_noise_step
        return D3D_OK;
    }
    if (!strcmp(key, "device_bytes")) {  // read-only: device memory the library holds, all contexts of the process
        *value = (long)d3dh::dev_bytes.load();
        return D3D_OK;
    }
    // read-only, derived: what the context actually runs
    if (!strcmp(key, "mh_nt_ivar_on")) {  // the beyond-the-Infinity-Cache policy of k_mh_ws is in effect
        *value = c->mh_nt_ivar ? 1 : 0;
        return D3D_OK;
    }
    if (!strcmp(key, "mh_strips_on")) {   // lattice-row strips the colour rows of d3d_mh_sweeps run in (0: none)
        *value = (c->have_data && c->parts.size() == 1 && c->parts[0].strips > 1) ? c->parts[0].strips : 0;
        return D3D_OK;
    }
    if (!strcmp(key, "mh_strip_order_on")) {  // how those strips are ordered: 0 no strips, 1 joined per colour row, 2 chained
        const bool strips = c->have_data && c->parts.size() == 1 && c->parts[0].strips > 1;
        *value = !strips ? 0 : c->parts[0].order.S > 1 ? 2 : 1;
        return D3D_OK;
    }
    // read-only: what the launchers of d3d_mh.hip launched since the record was last cleared (D3D_MH_*)
    if (!strcmp(key, "mh_path")) {           // the packed code of the last sweep-kernel launch
        *value = c->mh_path.code;
        return D3D_OK;
    }
    if (!strcmp(key, "mh_path_layers")) {    // bit n: a launch found n layers pending
        *value = (long)c->mh_path.layers;
        return D3D_OK;
    }
    if (!strcmp(key, "mh_path_launches")) {  // the launches counted; this read clears the record
        *value = c->mh_path.launches;
        c->mh_path = {};
        return D3D_OK;
    }
    if (!strcmp(key, "device_cus")) {        // compute units of the ctx's device: a colour launch of fewer than
        *value = c->flow_grid / 4;           // 2 workgroups per CU "does not fill the chip" (launch_mh_ws: few)
        return D3D_OK;
    }
    if (!strcmp(key, "batch_layers")) {   // pending layers of the last d3d_mh_sweeps_batch: 2 = its joint launches filled the chip
        *value = c->batch_layers;
        return D3D_OK;
    }
    if (!strcmp(key, "lsf_fits")) {       // the LSF taps lie within +-LSF_RL channels: fused / z-blocked kernels
        *value = (c->have_taps && (c->ntaps == 0 || c->lsf_dense_any)) ? 1 : 0;
        return D3D_OK;
    }
    if (!strcmp(key, "lsf_taps")) {
        *value = c->ntaps;
        return D3D_OK;
    }
    if (!strcmp(key, "spatial_path") || !strcmp(key, "spectral_path") || !strcmp(key, "stage_path")) {
        // read-only: the kernel family the dispatcher took last (D3D_SPATIAL_* / D3D_SPECTRAL_* / D3D_STAGE_*)
        *value = key[2] == 'a' ? (key[3] == 't' ? c->spatial_path : c->stage_path) : c->spectral_path;
        return D3D_OK;
    }
    if (!strcmp(key, "small_parts")) {    // parts whose colour launches run k_mh_small
        long n = 0;
        for (const d3d_ctx::Part &pt : c->parts) n += d3dh::mh_part_uses_tables(c, pt) ? 1 : 0;
        *value = c->have_data ? n : 0;
        return D3D_OK;
    }
    const OptDesc *o = find_opt(key);
    NEED(o, D3D_ERR_INVALID, "unknown option '%s'", key);
    *value = c->*(o->field);
    return D3D_OK;
}

int d3d_has_experiments(void) {
#ifdef D3D_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

// d3d_taps.h analyses the taps; here what its flags say goes to the device.
static int set_taps_impl(d3d_ctx *c, const double *fsf, const double *lsf, double thr) {
    HIP_TRY(hipSetDevice(c->device));
    const d3d_taps::Result r = d3d_taps::analyse(c->fh, c->fw, c->D, c->N, c->H, c->W, c->HL, c->flow_grid, d3d::LSF_RL,
                                                 fsf, lsf, thr, c->spatial_sep, c->march_hy_opt);
    NEED(!r.lsf_empty, D3D_ERR_INVALID, "LSF has no non-zero tap");
    c->ptab_valid = false;  // (the position tables of k_mh_small hold tap values)
    auto upload = [c](auto &dst, const auto &v) {
        return hipMemcpyAsync(dst, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, c->stream);
    };
    HIP_TRY(hipMemcpyAsync(c->fsf, fsf, (size_t)c->fh * c->fw * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->fsf_symx = r.symx;
    c->fsf_symy = r.symy;
    c->fsf_sep = r.sep;
    c->fsf_symt = r.symt;
    if (r.sep) HIP_TRY(upload(c->sep_uv, r.uv));
    if (!r.quad.empty()) HIP_TRY(upload(c->fsf_quad, r.quad));
    if (!r.quad_sep.empty()) HIP_TRY(upload(c->fsf_quad_sep, r.quad_sep));
    c->march_hy = r.march_hy;
    c->ntaps = (int)r.shift.size();
    // dense form for the fused epilogue: out[k] = sum_j wl[j] v[(k + j - RL) mod N]
    c->lsf_dense_any = r.dense_any;
    c->lsf_dense_ok = r.dense_ok;
    c->lsf_dense_sym = r.dense_sym;
    c->lsf_fusable = r.fusable;
    if (r.dense_any) HIP_TRY(upload(c->lsf_dense, r.dense));
    if (c->ntaps) {
        HIP_TRY(upload(c->lsf_shift, r.shift));
        HIP_TRY(upload(c->lsf_weight, r.weight));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));  // `r` goes out of scope
    c->have_taps = true;
    c->err_valid = false;
    pend_clear(c);
    if (c->Dp > d3d::MH_WS_MAX_DP) {  // the taps decide whether the z-blocked sweep kernels run
        const bool was = c->mh_zb;
        pick_mh_geometry(c);
        if (c->mh_zb != was && c->have_data) return build_colour_lists(c);
    }
    return D3D_OK;
}

int d3d_set_data(d3d_ctx *c, const double *data, const double *var, double var_scalar,
                 const uint8_t *mask) {
    NEED(c && data, D3D_ERR_INVALID, "NULL argument");
    NEED(!c->rescale.who, D3D_ERR_STATE, "%s are armed on the old variance: d3d_%s_end first",
         rescale_name(c).what, rescale_name(c).api);
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)c->D * c->HW;
    // mask: user mask AND no NaN anywhere in the spectrum (lib/run.py:153-162)
    for (long s = 0; s < c->HW; ++s) c->h_mask[s] = mask ? (mask[s] == 1) : 1;
    c->h_user_mask = c->h_mask;
    bool any_nan = false;
    for (int z = 0; z < c->D; ++z) {
        const double *pl = data + (size_t)z * c->HW;
        for (long s = 0; s < c->HW; ++s)
            if (pl[s] != pl[s]) {
                c->h_mask[s] = 0;
                any_nan = true;
            }
    }
    // one constant 1/variance everywhere (scalar variance, or a cube of equal
    // values as the reference builds when none is given, lib/run.py:171-178) and
    // no NaN voxel (those get 1/var = 0): the MH kernel need not read SLOT_IVAR.
    {
        const double v0 = var ? var[0] : var_scalar;
        bool uni = !any_nan && v0 == v0;
        if (uni && var)
            for (size_t i = 1; i < n; ++i)
                if (var[i] != v0) {
                    uni = false;
                    break;
                }
        c->ivar_is_uniform = uni;
        c->ivar_uniform = uni ? 1.0 / (v0 == 0.0 ? 1e12 : v0) : 0.0;
    }
    HIP_TRY(hipMemcpyAsync(c->mask, c->h_mask.data(), (size_t)c->HW, hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(c->stage, data, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    double *dvar = nullptr;
    if (var) {
        // the 1/var staging reuses TMP1's storage when it is large enough; use
        // a dedicated upload through stage2 to keep things simple.
        HIP_TRY(hipMemcpyAsync(c->stage2, var, n * sizeof(double), hipMemcpyHostToDevice,
                               c->stream));
        dvar = c->stage2;
    }
    const unsigned grid = (unsigned)((n + 255) / 256);
    // in place: stage <- cleaned data, stage2 <- 1/var
    hipLaunchKernelGGL(d3d::k_prepare_data, dim3(grid), dim3(256), 0, c->stream, c->stage,
                       c->stage2, (const double *)dvar, var_scalar, (long)n);
    HIP_TRY(hipGetLastError());
    int rc = to_device_layout(c, c->stage, c->slot[D3D_SLOT_DATA]);
    if (rc) return rc;
    rc = to_device_layout(c, c->stage2, c->slot[D3D_SLOT_IVAR]);
    if (rc) return rc;
    rc = build_colour_lists(c);
    if (rc) return rc;
    c->have_data = true;
    c->err_valid = false;
    pend_clear(c);
    if (c->reg.on)  // the members of a region are its unmasked spaxels
        if (int rc2 = region_members(c)) return rc2;
    return post_reset(c);  // moments over two data sets mean nothing
}

int d3d_set_params(d3d_ctx *c, const double *params) {
    NEED(c && params, D3D_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->params, params, (size_t)c->HW * 3 * sizeof(double),
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_params = true;
    c->err_valid = false;
    c->props_sweep = -1;
    pend_clear(c);
    return D3D_OK;
}

int d3d_set_line_shape(d3d_ctx *c, int K, const double *offsets, const double *ratios) {
    NEED(c && offsets && ratios, D3D_ERR_INVALID, "NULL argument");
    NEED(K >= 1 && K <= d3d::LINE_KMAX, D3D_ERR_INVALID, "a line shape has 1 to %d components, got %d",
         d3d::LINE_KMAX, K);
    for (int k = 0; k < K; ++k)
        NEED(std::isfinite(offsets[k]) && std::isfinite(ratios[k]), D3D_ERR_INVALID,
             "line shape: offsets and ratios must be finite (component %d)", k);
    NEED(offsets[0] == 0.0 && ratios[0] == 1.0, D3D_ERR_INVALID,
         "line shape: offsets[0] must be 0 and ratios[0] must be 1 (c and a are the first line's)");
    for (int k = 0; k < K; ++k) {
        NEED(ratios[k] >= 0.0, D3D_ERR_INVALID, "line shape: ratios must be >= 0 (component %d)", k);
        for (int j = 0; j < k; ++j)
            NEED(offsets[j] != offsets[k], D3D_ERR_INVALID,
                 "line shape: offsets must be distinct (components %d and %d)", j, k);
    }
    HIP_TRY(hipSetDevice(c->device));
    // the pending updates were made with the old line: written back with it, then everything
    // built from the line -- the residual, the sweep's proposal and line tables -- is stale
    if (int rc = flush_pending(c)) return rc;
    d3d::LineShape L = c->line;  // (the table, if any, stays: d3d_set_line_table)
    L.K = K;
    for (int k = 0; k < d3d::LINE_KMAX; ++k) {
        L.off[k] = k < K ? offsets[k] : 0.0;
        L.ratio[k] = k < K ? ratios[k] : 0.0;
    }
    c->line = L;
    c->err_valid = false;
    c->props_sweep = -1;
    return post_reset(c);  // moments over two line models mean nothing
}

int d3d_set_line_table(d3d_ctx *c, int n, double support, const double *table, double flux_factor) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    if (n != 0) {
        NEED(table, D3D_ERR_INVALID, "NULL argument");
        NEED(n >= 8 && n <= 65537, D3D_ERR_INVALID, "a line table has 8 to 65537 samples, got %d", n);
        NEED(std::isfinite(support) && support > 0.0, D3D_ERR_INVALID,
             "line table: the support must be finite and > 0");
        NEED(std::isfinite(flux_factor), D3D_ERR_INVALID, "line table: the flux factor must be finite");
        double peak = 0.0;
        for (int j = 0; j < n; ++j) {
            NEED(std::isfinite(table[j]), D3D_ERR_INVALID, "line table: sample %d is not finite", j);
            if (std::fabs(table[j]) > std::fabs(peak)) peak = table[j];
        }
        NEED(peak == 1.0, D3D_ERR_INVALID,
             "line table: the sample of largest magnitude must be 1 (a is the peak amplitude), got %g", peak);
    }
    HIP_TRY(hipSetDevice(c->device));
    // the new table first (a failure keeps the old one), then as d3d_set_line_shape: the pending
    // updates were made with the old line
    DevBuf<double> dev;
    if (n != 0) {
        std::vector<double> padded((size_t)n + 2, 0.0);
        std::copy(table, table + n, padded.begin() + 1);
        HIP_TRY(dev.alloc(padded.size()));
        HIP_TRY(hipMemcpy(dev, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (int rc = flush_pending(c)) return rc;
    if (c->line_tab) HIP_TRY(hipStreamSynchronize(c->stream));  // (launches that read the old table may still be queued)
    c->line_tab = std::move(dev);
    c->line.tab = c->line_tab;
    c->line.n = n;
    c->line.support = n ? support : 0.0;
    c->line.inv_h = n ? (double)(n - 1) / (2.0 * support) : 0.0;
    c->line_tab_flux = n ? flux_factor : 0.0;
    if (n)
        c->h_line_tab.assign(table, table + n);
    else
        c->h_line_tab.clear();
    c->err_valid = false;
    c->props_sweep = -1;
    return post_reset(c);  // moments over two line models mean nothing
}

int d3d_get_params(d3d_ctx *c, double *params) {
    NEED(c && params, D3D_ERR_INVALID, "NULL argument");
    NEED(c->have_params, D3D_ERR_STATE, "parameters not set");
    HIP_TRY(hipMemcpyAsync(params, c->params, (size_t)c->HW * 3 * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_build_clean(d3d_ctx *c, double *out) {
    NEED(c && out, D3D_ERR_INVALID, "NULL argument");
    NEED(c->have_params, D3D_ERR_STATE, "parameters not set");
    HIP_TRY(hipSetDevice(c->device));
    int rc = launch_lines(c, c->slot[D3D_SLOT_TMP0], 0);
    if (rc) return rc;
    return download_cube(c, c->slot[D3D_SLOT_TMP0], out);
}

int d3d_convolve_slots(d3d_ctx *c, int src, int dst) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(src >= 0 && src < D3D_SLOT_COUNT && dst >= 0 && dst < D3D_SLOT_COUNT && src != dst,
         D3D_ERR_INVALID, "bad slots %d -> %d", src, dst);
    NEED(c->have_taps, D3D_ERR_STATE, "taps not set");
    NEED(dst != D3D_SLOT_TMP1 && src != D3D_SLOT_TMP1, D3D_ERR_INVALID,
         "SLOT_TMP1 is the convolution's intermediate");
    NEED(dst != D3D_SLOT_IVAR || !c->rescale.who, D3D_ERR_STATE, "SLOT_IVAR is rewritten by the %s: d3d_%s_end first",
         rescale_name(c).what, rescale_name(c).api);
    HIP_TRY(hipSetDevice(c->device));
    if (src == D3D_SLOT_ERR)
        if (int rc = flush_pending(c)) return rc;
    if (dst == D3D_SLOT_IVAR) c->ivar_is_uniform = false;
    const double *in = c->slot[src];
    if (c->ntaps > 0) {
        // FSF and LSF act on different axes and commute: when possible the LSF is
        // applied in the spatial kernel's epilogue (one pass over the cube)
        if (can_fuse_lsf(c)) return launch_spatial(c, in, c->slot[dst], nullptr, true);
        int rc = launch_spectral(c, in, c->slot[D3D_SLOT_TMP1]);
        if (rc) return rc;
        in = c->slot[D3D_SLOT_TMP1];
    }
    return launch_spatial(c, in, c->slot[dst], nullptr);
}

int d3d_upload_slot(d3d_ctx *c, int slot, const double *cube) {
    NEED(c && cube, D3D_ERR_INVALID, "NULL argument");
    NEED(slot >= 0 && slot < D3D_SLOT_COUNT, D3D_ERR_INVALID, "bad slot %d", slot);
    NEED(slot != D3D_SLOT_IVAR || !c->rescale.who, D3D_ERR_STATE, "SLOT_IVAR is rewritten by the %s: d3d_%s_end first",
         rescale_name(c).what, rescale_name(c).api);
    HIP_TRY(hipSetDevice(c->device));
    int rc = upload_cube(c, cube, c->slot[slot]);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (slot == D3D_SLOT_ERR) {
        c->err_valid = true;
        pend_clear(c);
    }
    if (slot == D3D_SLOT_IVAR) c->ivar_is_uniform = false;
    return D3D_OK;
}

int d3d_download_slot(d3d_ctx *c, int slot, double *cube) {
    NEED(c && cube, D3D_ERR_INVALID, "NULL argument");
    NEED(slot >= 0 && slot < D3D_SLOT_COUNT, D3D_ERR_INVALID, "bad slot %d", slot);
    HIP_TRY(hipSetDevice(c->device));
    if (slot == D3D_SLOT_ERR)
        if (int rc = flush_pending(c)) return rc;
    return download_cube(c, c->slot[slot], cube);
}

// ---- convolution in the reference layout (staging buffers, z-major) --------

int d3d_stage_upload(d3d_ctx *c, const double *cube) {
    NEED(c && cube, D3D_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->stage, cube, (size_t)c->D * c->HW * sizeof(double),
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_stage_download(d3d_ctx *c, double *cube) {
    NEED(c && cube, D3D_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(cube, c->stage, (size_t)c->D * c->HW * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_stage_convolve(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->have_taps, D3D_ERR_STATE, "taps not set");
    HIP_TRY(hipSetDevice(c->device));
    c->stage_path = zmajor_ok(c) ? D3D_STAGE_ZMAJOR : D3D_STAGE_TRANSPOSE;
    if (zmajor_ok(c)) return launch_zmajor_convolve(c);
    // general taps: through the spectrum-contiguous slot kernels
    int rc = to_device_layout(c, c->stage, c->slot[D3D_SLOT_TMP0]);
    if (rc) return rc;
    rc = d3d_convolve_slots(c, D3D_SLOT_TMP0, D3D_SLOT_SIM);
    if (rc) return rc;
    return to_host_layout(c, c->slot[D3D_SLOT_SIM], c->stage);
}

int d3d_convolve(d3d_ctx *c, const double *in, double *out) {
    NEED(c && in && out, D3D_ERR_INVALID, "NULL argument");
    int rc = d3d_stage_upload(c, in);
    if (rc) return rc;
    rc = d3d_stage_convolve(c);
    if (rc) return rc;
    return d3d_stage_download(c, out);
}

int d3d_forward(d3d_ctx *c, double *out_sim) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->have_taps && c->have_params, D3D_ERR_STATE, "taps/parameters not set");
    HIP_TRY(hipSetDevice(c->device));
    int rc = forward_into(c, c->slot[D3D_SLOT_SIM], false);
    if (rc) return rc;
    if (out_sim) return download_cube(c, c->slot[D3D_SLOT_SIM], out_sim);
    return D3D_OK;
}

int d3d_simulate(d3d_ctx *c, const double *params, int convolved, double *out) {
    NEED(c && params && out, D3D_ERR_INVALID, "NULL argument");
    NEED(c->have_taps || !convolved, D3D_ERR_STATE, "taps not set");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->params_alt, params, (size_t)c->HW * 3 * sizeof(double),
                           hipMemcpyHostToDevice, c->stream));
    const bool fuse = convolved && c->ntaps > 0 && can_fuse_lsf(c);  // as forward_into
    int rc = launch_lines(c, c->slot[D3D_SLOT_TMP0], (convolved && !fuse) ? 1 : 0, c->params_alt);
    if (rc) return rc;
    if (!convolved) return download_cube(c, c->slot[D3D_SLOT_TMP0], out);
    rc = launch_spatial(c, c->slot[D3D_SLOT_TMP0], c->slot[D3D_SLOT_SIM], nullptr, fuse);
    if (rc) return rc;
    return download_cube(c, c->slot[D3D_SLOT_SIM], out);
}

int d3d_residual(d3d_ctx *c, double *out_err) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->have_taps && c->have_params && c->have_data, D3D_ERR_STATE,
         "taps/data/parameters not set");
    HIP_TRY(hipSetDevice(c->device));
    int rc = forward_into(c, c->slot[D3D_SLOT_ERR], true);
    if (rc) return rc;
    c->err_valid = true;
    if (out_err) return download_cube(c, c->slot[D3D_SLOT_ERR], out_err);
    return D3D_OK;
}

int d3d_chi2_map(d3d_ctx *c, double *out_hw, double *total) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->have_data && c->err_valid, D3D_ERR_STATE, "residual not available");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = flush_pending(c)) return rc;
    const unsigned grid = (unsigned)((c->HW + 3) / 4);
    hipLaunchKernelGGL(d3d::k_chi2_map, dim3(grid), dim3(256), 0, c->stream,
                       (const double *)c->slot[D3D_SLOT_ERR], (const double *)c->slot[D3D_SLOT_IVAR],
                       c->hwbuf, c->HL, c->Dp, c->HW);
    HIP_TRY(hipGetLastError());
    if (total) {
        hipLaunchKernelGGL(d3d::k_sum, dim3(1), dim3(1024), 0, c->stream, (const double *)c->hwbuf,
                           c->HW, c->scal + 8);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(total, c->scal + 8, sizeof(double), hipMemcpyDeviceToHost,
                               c->stream));
    }
    if (out_hw)
        HIP_TRY(hipMemcpyAsync(out_hw, c->hwbuf, (size_t)c->HW * sizeof(double),
                               hipMemcpyDeviceToHost, c->stream));
    // (nothing for the host: the map stays on the device and the call does not wait -- bench.py
    // times the kernel that way)
    if (out_hw || total) HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_mh_config(d3d_ctx *c, const double min_b[3], const double max_b[3],
                  const double jump_amp[3], double ra, uint64_t seed, int refresh_every) {
    NEED(c && min_b && max_b && jump_amp, D3D_ERR_INVALID, "NULL argument");
    for (int k = 0; k < 3; ++k)  // lib/run.py:244-245
        NEED(!(min_b[k] > max_b[k]), D3D_ERR_INVALID, "Boundaries are inconsistent: min > max.");
    NEED(ra > 0.0, D3D_ERR_INVALID, "gibbs_apriori_variance must be positive");
    NEED(refresh_every >= 0, D3D_ERR_INVALID, "refresh_every must be >= 0");
    for (int k = 0; k < 3; ++k) {
        c->min_b[k] = min_b[k];
        c->max_b[k] = max_b[k];
        c->amp[k] = jump_amp[k];
    }
    c->amp[0] = 0.0;  // lib/run.py:261-262
    c->ra = ra;
    c->seed = seed;
    c->refresh_every = refresh_every;
    c->have_cfg = true;
    c->props_sweep = -1;
    c->mh_path = {};  // (read-only options mh_path*: the record of a chain starts with its configuration)
    return D3D_OK;
}

int d3d_mh_set_sweep_origin(d3d_ctx *c, int64_t origin) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(origin >= 0 && origin < (int64_t(1) << 31), D3D_ERR_INVALID, "sweep origin out of range");
    c->sweep_origin = (uint32_t)origin;
    c->props_sweep = -1;
    return D3D_OK;
}

int d3d_window_stats(d3d_ctx *c, int y, int x, const double p_new[3], double out[5]) {
    NEED(c && p_new && out, D3D_ERR_INVALID, "NULL argument");
    NEED(c->have_taps && c->have_data && c->have_params, D3D_ERR_STATE,
         "taps/data/parameters not set");
    NEED(y >= 0 && y < c->H && x >= 0 && x < c->W, D3D_ERR_INVALID, "spaxel (%d,%d) out of range",
         y, x);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->err_valid) {
        int rc = d3d_residual(c, nullptr);
        if (rc) return rc;
    }
    if (int rc = flush_pending(c)) return rc;
    d3d::MHArgs P;
    fill_mh_args(c, P);
    P.probe = 1;
    P.probe_sp = y * c->W + x;
    P.probe_p[0] = p_new[0];
    P.probe_p[1] = p_new[1];
    P.probe_p[2] = p_new[2];
    int rc = launch_mh(c, P, 1, 0);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->scal, 5 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_mh_accepted(d3d_ctx *c, int64_t *count, int reset) {
    NEED(c && count, D3D_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long acc = 0;
    if (int rc = accepted_collect(c)) return rc;
    HIP_TRY(hipMemcpyAsync(&acc, c->accepted, sizeof acc, hipMemcpyDeviceToHost, c->stream));
    if (reset) HIP_TRY(hipMemsetAsync(c->accepted, 0, sizeof(unsigned long long), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *count = (int64_t)acc;
    return D3D_OK;
}

int d3d_flush(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return flush_pending(c);
}

int d3d_line_search(d3d_ctx *c, int n_c, const double *centres, int n_w, const double *widths,
                    const double *host_bank, int32_t *best_out, double *stat_out) {
    NEED(c && centres && widths && best_out && stat_out, D3D_ERR_INVALID, "NULL argument");
    NEED(n_c >= 1 && n_w >= 1, D3D_ERR_INVALID, "line search: %d centres and %d widths (at least one of each)",
         n_c, n_w);
    for (int i = 0; i < n_c; ++i)
        NEED(std::isfinite(centres[i]), D3D_ERR_INVALID, "line search: centres[%d] is not finite", i);
    for (int i = 0; i < n_w; ++i)
        NEED(std::isfinite(widths[i]) && widths[i] > 0.0, D3D_ERR_INVALID,
             "line search: widths[%d] = %g is not a positive number", i, widths[i]);
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED,
         "line search on a tile: search the whole cube on one context and cut the map");
    NEED(c->have_taps && c->have_data, D3D_ERR_STATE, "taps/data not set");
    return line_search(c, n_c, centres, n_w, widths, host_bank, best_out, stat_out);
}

int d3d_running_median(d3d_ctx *c, const double *cube, const uint8_t *valid, int half_window, double *out) {
    NEED(c && cube && out, D3D_ERR_INVALID, "NULL argument");
    NEED(half_window >= 1 && half_window <= 128, D3D_ERR_INVALID,
         "running median: half_window = %d is outside 1 .. 128", half_window);
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED, "running median on a tile: prepare the whole cube on one context");
    return prep_running_median(c, cube, valid, half_window, out);
}

int d3d_channel_stats(d3d_ctx *c, const double *cube, const uint8_t *select, double *m_out, double *mad_out,
                      int64_t *n_out) {
    NEED(c && cube && m_out && mad_out && n_out, D3D_ERR_INVALID, "NULL argument");
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED, "channel statistics on a tile: prepare the whole cube on one context");
    return prep_channel_stats(c, cube, select, m_out, mad_out, n_out);
}

int d3d_prepare(d3d_ctx *c, const double *cube, const uint8_t *select, int half_window, double reject,
                double *continuum_out, double *residual_out, double *chan_out) {
    NEED(c && cube && continuum_out && residual_out && chan_out, D3D_ERR_INVALID, "NULL argument");
    NEED(half_window >= 1 && half_window <= 128, D3D_ERR_INVALID,
         "prepare: half_window = %d is outside 1 .. 128", half_window);
    NEED(reject != reject || reject > 0.0, D3D_ERR_INVALID,
         "prepare: reject = %g is not a positive number of sigmas (NaN: no rejection pass)", reject);
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED, "prepare on a tile: prepare the whole cube on one context and cut it");
    return prep_prepare(c, cube, select, half_window, reject, continuum_out, residual_out, chan_out);
}

int d3d_adapt_begin(d3d_ctx *c, double target, int window, int64_t last_sweep, double gain,
                    double scale_min, double scale_max) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(target > 0.0 && target < 1.0, D3D_ERR_INVALID, "target = %g: an acceptance rate inside (0, 1)", target);
    NEED(window >= 0, D3D_ERR_INVALID, "window = %d is negative (0: a fixed map that never adapts)", window);
    NEED(gain > 0.0 && std::isfinite(gain), D3D_ERR_INVALID, "gain = %g: a positive number", gain);
    NEED(std::isfinite(scale_min) && std::isfinite(scale_max) && scale_min > 0.0 && scale_max > 0.0,
         D3D_ERR_INVALID, "scale range (%g, %g): finite, positive numbers", scale_min, scale_max);
    NEED(scale_min <= scale_max, D3D_ERR_INVALID, "scale range: min %g > max %g", scale_min, scale_max);
    NEED(!c->tiled, D3D_ERR_UNSUPPORTED,
         "per-spaxel jump scales on a tile: a window's scale steps would have to follow the ranks' phases");
    if (int rc = adapt_kernels_ok(c)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    adapt_free(c);
    hipError_t e = c->adapt.jscale.alloc((size_t)c->HW);
    if (e == hipSuccess) e = c->adapt.jacc.alloc((size_t)c->HW);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the context stays usable for the chain
        adapt_free(c);
        return fail(D3D_ERR_HIP, "jump scale map (%ld spaxels): %s", c->HW, hipGetErrorString(e));
    }
    std::vector<double> ones((size_t)c->HW, 1.0);
    HIP_TRY(hipMemcpy(c->adapt.jscale, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->adapt.jacc, 0, (size_t)c->HW * sizeof(unsigned)));
    c->adapt.target = target;
    c->adapt.window = window;
    c->adapt.last = last_sweep;
    c->adapt.gain = gain;
    c->adapt.min = scale_min;
    c->adapt.max = scale_max;
    c->adapt.n_win = c->adapt.k = 0;
    c->adapt.on = true;
    c->props_sweep = -1;
    return D3D_OK;
}

int d3d_adapt_get(d3d_ctx *c, double *scale_hw, uint32_t *accepted_hw, int64_t *n_win, int64_t *k) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->adapt.on, D3D_ERR_STATE, "per-spaxel jump scales not begun (d3d_adapt_begin)");
    HIP_TRY(hipSetDevice(c->device));
    if (scale_hw)
        HIP_TRY(hipMemcpyAsync(scale_hw, c->adapt.jscale, (size_t)c->HW * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (accepted_hw)
        HIP_TRY(hipMemcpyAsync(accepted_hw, c->adapt.jacc, (size_t)c->HW * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n_win) *n_win = c->adapt.n_win;
    if (k) *k = c->adapt.k;
    return D3D_OK;
}

int d3d_adapt_set(d3d_ctx *c, const double *scale_hw, const uint32_t *accepted_hw, int64_t n_win, int64_t k) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(c->adapt.on, D3D_ERR_STATE, "per-spaxel jump scales not begun (d3d_adapt_begin)");
    NEED(n_win >= 0 && k >= 0, D3D_ERR_INVALID, "n_win = %lld / k = %lld is negative", (long long)n_win, (long long)k);
    if (scale_hw)
        for (long i = 0; i < c->HW; ++i)
            NEED(std::isfinite(scale_hw[i]) && scale_hw[i] > 0.0, D3D_ERR_INVALID,
                 "jump scale of spaxel (%ld, %ld) is %g: finite, positive numbers", i / c->W, i % c->W, scale_hw[i]);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (scale_hw) HIP_TRY(hipMemcpy(c->adapt.jscale, scale_hw, (size_t)c->HW * sizeof(double), hipMemcpyHostToDevice));
    if (accepted_hw)
        HIP_TRY(hipMemcpy(c->adapt.jacc, accepted_hw, (size_t)c->HW * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->adapt.n_win = n_win;
    c->adapt.k = k;
    c->props_sweep = -1;  // (a table made from the old scales)
    return D3D_OK;
}

int d3d_adapt_end(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    adapt_free(c);
    return D3D_OK;
}

int d3d_prior_begin(d3d_ctx *c, const double lam[3]) {
    NEED(c && lam, D3D_ERR_INVALID, "NULL argument");
    for (int k = 0; k < 3; ++k)
        NEED(std::isfinite(lam[k]) && lam[k] >= 0.0, D3D_ERR_INVALID,
             "lam[%d] = %g: finite and >= 0 (1 / sigma^2 of the neighbour differences)", k, lam[k]);
    NEED(c->fh > 1 && c->fw > 1, D3D_ERR_INVALID,
         "smoothness prior with a %d x %d FSF: adjacent spaxels would share a colour class", c->fh, c->fw);
    if (int rc = prior_kernels_ok(c)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; ++k) c->prior.lam[k] = lam[k];
    c->prior.on = true;
    c->props_sweep = -1;
    return D3D_OK;
}

int d3d_prior_get(d3d_ctx *c, double lam[3], int *on) {
    NEED(c && lam && on, D3D_ERR_INVALID, "NULL argument");
    for (int k = 0; k < 3; ++k) lam[k] = c->prior.on ? c->prior.lam[k] : 0.0;
    *on = c->prior.on ? 1 : 0;
    return D3D_OK;
}

int d3d_prior_end(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->prior.on = false;
    c->prior.lam[0] = c->prior.lam[1] = c->prior.lam[2] = 0.0;
    c->props_sweep = -1;
    return D3D_OK;
}

int d3d_prior_energy(d3d_ctx *c, const double *params, double energy[3], int64_t *pairs) {
    NEED(c && energy && pairs, D3D_ERR_INVALID, "NULL argument");
    NEED(params || c->have_params, D3D_ERR_STATE, "parameters not set");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<double> tmp;
    if (params) {
        HIP_TRY(tmp.alloc((size_t)c->HW * 3));
        HIP_TRY(hipMemcpyAsync(tmp, params, (size_t)c->HW * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    double out4[4] = {0.0, 0.0, 0.0, 0.0};
    const int rc = d3dh::prior_energy(c, params ? tmp.get() : c->params.get(), out4);
    if (tmp) (void)hipStreamSynchronize(c->stream);
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) energy[k] = out4[k];
    *pairs = (int64_t)out4[3];
    return D3D_OK;
}

int d3d_get_dlog(d3d_ctx *c, double *out_hw) {
    NEED(c && out_hw, D3D_ERR_INVALID, "NULL argument");
    HIP_TRY(hipMemcpyAsync(out_hw, c->dlog, (size_t)c->HW * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

#ifdef D3D_EXPERIMENTS
// Phase stamps of the next `launches` colour launches of d3d_mh_sweeps
// (tools/mh_phases.py).  d3d_x_stamps_read copies launch `i`'s n*8 stamps out.
int d3d_x_stamps_arm(d3d_ctx *c, int launches) {
    NEED(c && launches > 0, D3D_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    c->stampbuf.reset();
    NEED(c->have_data, D3D_ERR_STATE, "data not set");
    size_t most = 0;
    for (const d3d_ctx::Part &pt : c->parts)
        for (size_t k = 0; k + 1 < pt.off.size(); ++k)
            most = std::max(most, (size_t)(pt.off[k + 1] - pt.off[k]));
    c->stamp_stride = most * 8;
    c->stamp_launches = (size_t)launches;
    c->stamp_next = 0;
    const size_t bytes = c->stamp_launches * c->stamp_stride * sizeof(unsigned long long);
    HIP_TRY(c->stampbuf.alloc(c->stamp_launches * c->stamp_stride));
    HIP_TRY(hipMemset(c->stampbuf, 0, bytes));
    return D3D_OK;
}

int d3d_x_stamps_read(d3d_ctx *c, int launch, int n, unsigned long long *out) {
    NEED(c && out && c->stampbuf && launch >= 0 && (size_t)launch < c->stamp_launches && n > 0,
         D3D_ERR_INVALID, "bad argument");
    if ((size_t)n * 8 > c->stamp_stride) n = (int)(c->stamp_stride / 8);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->stampbuf + (size_t)launch * c->stamp_stride,
                      (size_t)n * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return D3D_OK;
}

// the whole stamp buffer from word `first` on (k_mh_chain: [slot][colour][8], tools/chain_phases.py)
int d3d_x_stamps_raw(d3d_ctx *c, long first, long nwords, unsigned long long *out) {
    NEED(c && out && c->stampbuf && first >= 0 && nwords > 0 &&
             (size_t)(first + nwords) <= c->stamp_launches * c->stamp_stride,
         D3D_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->stampbuf + first, (size_t)nwords * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
    return D3D_OK;
}
#endif

int d3d_mh_layers(d3d_ctx *c, int *out) {
    NEED(c && out, D3D_ERR_INVALID, "NULL argument");
    NEED(c->have_data, D3D_ERR_STATE, "data not set");
    const bool partitioned = partitioned_sweep(c);
    const bool deferred =
        c->mh_defer &&
        (!partitioned || (c->mh_defer == 1 && (c->Dp <= d3d::MH_WS_MAX_DP || c->mh_zb)));
    *out = deferred ? c->mh_layers : 0;
    return D3D_OK;
}

int d3d_variance_is_uniform(d3d_ctx *c, int *out) {
    NEED(c && out, D3D_ERR_INVALID, "NULL argument");
    NEED(c->have_data, D3D_ERR_STATE, "data not set");
    *out = (c->ivar_is_uniform && c->uniform_fast_path) ? 1 : 0;
    return D3D_OK;
}

int d3d_set_tile(d3d_ctx *c, int gy0, int gx0, int Wg, int oy0, int oy1, int ox0, int ox1) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(gy0 >= 0 && gx0 >= 0 && Wg >= gx0 + c->W, D3D_ERR_INVALID,
         "tile origin (%d,%d) / global width %d inconsistent with local width %d", gy0, gx0, Wg,
         c->W);
    NEED(0 <= oy0 && oy0 <= oy1 && oy1 <= c->H && 0 <= ox0 && ox0 <= ox1 && ox1 <= c->W,
         D3D_ERR_INVALID, "owned rectangle [%d,%d)x[%d,%d) outside the tile", oy0, oy1, ox0, ox1);
    NEED(!c->adapt.on, D3D_ERR_UNSUPPORTED,
         "per-spaxel jump scales are on (d3d_adapt_begin): not on a tile; call d3d_adapt_end first");
    NEED(!c->prior.on, D3D_ERR_UNSUPPORTED,
         "the smoothness prior is on (d3d_prior_begin): not on a tile; call d3d_prior_end first");
    NEED(!c->rescale.who, D3D_ERR_UNSUPPORTED, "%s are armed (d3d_%s_begin): not on a tile; call d3d_%s_end first",
         rescale_name(c).what, rescale_name(c).api, rescale_name(c).api);
    c->gy0 = gy0;
    c->gx0 = gx0;
    c->Wg = Wg;
    c->oy0 = oy0;
    c->oy1 = oy1;
    c->ox0 = ox0;
    c->ox1 = ox1;
    c->tiled = true;
    c->part_rects.clear();  // one part: the owned rectangle (d3d_set_parts refines it)
    c->part_phase.clear();
    pend_clear(c);
    if (c->have_data) return build_colour_lists(c);
    return D3D_OK;
}

int d3d_set_parts(d3d_ctx *c, int nparts, const int *rects, const int *phases) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(nparts >= 0 && nparts <= 4096 && (nparts == 0 || (rects && phases)), D3D_ERR_INVALID,
         "bad part list");
    NEED(!c->prior.on || nparts <= 1, D3D_ERR_UNSUPPORTED,
         "the smoothness prior is on (d3d_prior_begin): not on a context cut into parts; call "
         "d3d_prior_end first");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = flush_pending(c)) return rc;
    std::vector<d3d_worklists::Rect> rr;
    std::vector<int> ph;
    for (int i = 0; i < nparts; ++i) {
        const int y0 = rects[4 * i], y1 = rects[4 * i + 1], x0 = rects[4 * i + 2],
                  x1 = rects[4 * i + 3];
        NEED(c->oy0 <= y0 && y0 <= y1 && y1 <= c->oy1 && c->ox0 <= x0 && x0 <= x1 && x1 <= c->ox1,
             D3D_ERR_INVALID, "part %d [%d,%d)x[%d,%d) is not inside the owned rectangle", i, y0, y1,
             x0, x1);
        NEED(phases[i] >= 0 && phases[i] < D3D_PLAN_PARAMS, D3D_ERR_INVALID,
             "phase %d of part %d out of range", phases[i], i);
        for (size_t j = 0; j < rr.size(); ++j)  // parts must not overlap
            NEED(y1 <= rr[j].y0 || rr[j].y1 <= y0 || x1 <= rr[j].x0 || rr[j].x1 <= x0 || y0 == y1 ||
                     x0 == x1 || rr[j].y0 == rr[j].y1 || rr[j].x0 == rr[j].x1,
                 D3D_ERR_INVALID, "parts %d and %zu overlap", i, j);
        rr.push_back({y0, y1, x0, x1});
        ph.push_back(phases[i]);
    }
    c->part_rects = rr;
    c->part_phase = ph;
    if (c->have_data) return build_colour_lists(c);
    return D3D_OK;
}

int d3d_export_updates(d3d_ctx *c, int n, const int *spaxels, double *out) {
    NEED(c && (n == 0 || (spaxels && out)), D3D_ERR_INVALID, "NULL argument");
    NEED(n >= 0 && n <= c->HW, D3D_ERR_INVALID, "bad record count %d", n);
    if (n == 0) return D3D_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->idxbuf, spaxels, (size_t)n * sizeof(int), hipMemcpyHostToDevice,
                           c->stream));
    d3d::MHArgs P;
    fill_mh_args(c, P);
    hipLaunchKernelGGL(d3d::k_gather_updates, dim3((n + 255) / 256), dim3(256), 0, c->stream, P,
                       (const int *)c->idxbuf, n, c->recbuf);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->recbuf, (size_t)n * 8 * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_apply_updates(d3d_ctx *c, int n, const double *records) {
    NEED(c && (n == 0 || records), D3D_ERR_INVALID, "NULL argument");
    NEED(n >= 0 && n <= c->HW, D3D_ERR_INVALID, "bad record count %d", n);
    NEED(c->have_taps && c->have_data, D3D_ERR_STATE, "taps/data not set");
    NEED(!c->deep, D3D_ERR_UNSUPPORTED, "update records are not replayed on cubes deeper than 1024 channels");
    if (n == 0) return D3D_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->err_valid) {
        int rc = d3d_residual(c, nullptr);
        if (rc) return rc;
    }
    if (int rc = flush_pending(c)) return rc;
    HIP_TRY(hipMemcpyAsync(c->recbuf, records, (size_t)n * 8 * sizeof(double),
                           hipMemcpyHostToDevice, c->stream));
    d3d::MHArgs P;
    fill_mh_args(c, P);
    if (int rc = launch_apply_updates(c, P, (const double *)c->recbuf, n)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_mh_colour_lines(d3d_ctx *c, int sweep, int n, const int *spaxels, const double *in3,
                        const double *lines, int gibbs, double *out3) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(n >= 0 && sweep >= 0, D3D_ERR_INVALID, "bad count / sweep");
    if (n == 0) return D3D_OK;
    NEED(spaxels && in3 && lines && out3, D3D_ERR_INVALID, "NULL argument");
    NEED(!c->prior.on, D3D_ERR_UNSUPPORTED,
         "the smoothness prior is on (d3d_prior_begin): a host-evaluated model's parameters are not the "
         "context's (a, c, w); call d3d_prior_end first");
    NEED(c->have_taps && c->have_data && c->have_cfg && c->err_valid, D3D_ERR_STATE,
         "taps/data/mh_config/residual not set");
    NEED(n <= c->HW, D3D_ERR_INVALID, "too many spaxels");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = flush_pending(c)) return rc;
    const size_t per = 6 + 2 * (size_t)c->D;
    HIP_TRY(c->extbuf.reserve((size_t)n * per));
    double *d_in = c->extbuf;                      // [n*3]
    double *d_out = d_in + (size_t)n * 3;          // [n*3]
    double *d_lines = d_out + (size_t)n * 3;       // [n*2*D]
    HIP_TRY(hipMemcpyAsync(c->idxbuf, spaxels, (size_t)n * sizeof(int), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(d_in, in3, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(d_lines, lines, (size_t)n * 2 * c->D * sizeof(double),
                           hipMemcpyHostToDevice, c->stream));
    d3d::MHArgs P;
    fill_mh_args(c, P);
    P.ext_idx = c->idxbuf;
    P.ext_in = d_in;
    P.ext_lines = d_lines;
    P.ext_out = d_out;
    P.ext_gibbs = gibbs ? 1 : 0;
    P.prev = nullptr;
    const int saved_maxit = c->mh_maxit;
    c->mh_maxit = 0;  // re-read variant: any window size
    int rc = launch_mh(c, P, (unsigned)n, (uint32_t)sweep);
    c->mh_maxit = saved_maxit;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out3, d_out, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

}  // extern "C"

// ---- halo exchange of the tiled chain ------------------------------------------

namespace {

int load_rccl() {
    if (g_rccl.handle) return 0;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    for (const char *n : names) {
        h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) return fail(D3D_ERR_UNSUPPORTED, "cannot load RCCL (librccl.so.1): %s", dlerror());
    RcclApi a;
    a.handle = h;
#define D3D_SYM(field, name)                                                        \
    do {                                                                            \
        *(void **)(&a.field) = dlsym(h, name);                                      \
        if (!a.field) return fail(D3D_ERR_UNSUPPORTED, "RCCL lacks symbol %s", name); \
    } while (0)
    D3D_SYM(GetUniqueId, "ncclGetUniqueId");
    D3D_SYM(CommInitRank, "ncclCommInitRank");
    D3D_SYM(CommDestroy, "ncclCommDestroy");
    D3D_SYM(Send, "ncclSend");
    D3D_SYM(Recv, "ncclRecv");
    D3D_SYM(GroupStart, "ncclGroupStart");
    D3D_SYM(GroupEnd, "ncclGroupEnd");
    D3D_SYM(CommCount, "ncclCommCount");
    D3D_SYM(CommUserRank, "ncclCommUserRank");
    D3D_SYM(GetErrorString, "ncclGetErrorString");
#undef D3D_SYM
    g_rccl = a;
    return 0;
}

#define RCCL_TRY(expr)                                                                  \
    do {                                                                                \
        ncclResult_t r_ = (expr);                                                       \
        if (r_ != ncclSuccess)                                                          \
            return fail(D3D_ERR_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(r_)); \
    } while (0)

int rect_copy(d3d_ctx *c, int what, int y0, int y1, int x0, int x1, double *packed, int unpack) {
    const int ny = y1 - y0, nx = x1 - x0;
    if (ny <= 0 || nx <= 0) return 0;
    double *arr = what == 0 ? c->slot[D3D_SLOT_ERR] : c->params;
    const int E = what == 0 ? c->Dp : 3;
    const long total = (long)ny * nx * E;
    const unsigned grid = (unsigned)std::min<long>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(d3d::k_rect_copy, dim3(grid), dim3(256), 0, c->stream, arr, c->W, E, y0, x0,
                       ny, nx, packed, unpack);
    HIP_TRY(hipGetLastError());
    return 0;
}

int halo_pack(d3d_ctx *c, int plan) {
    bool err_cells = false;
    for (const d3d_ctx::HaloEntry &e : c->plans[plan]) err_cells = err_cells || (e.what == 0 && e.send_n);
    // pending updates are part of the residual a neighbour must see
    if (err_cells)
        if (int rc = flush_pending(c)) return rc;
    for (const d3d_ctx::HaloEntry &e : c->plans[plan])
        if (e.send_n)
            if (int rc = rect_copy(c, e.what, e.sy0, e.sy1, e.sx0, e.sx1, c->halo_send + e.send_off, 0))
                return rc;
    return 0;
}

int halo_unpack(d3d_ctx *c, int plan) {
    bool err_cells = false;
    for (const d3d_ctx::HaloEntry &e : c->plans[plan]) err_cells = err_cells || (e.what == 0 && e.recv_n);
    if (err_cells)
        if (int rc = flush_pending(c)) return rc;
    for (const d3d_ctx::HaloEntry &e : c->plans[plan])
        if (e.recv_n)
            if (int rc = rect_copy(c, e.what, e.ry0, e.ry1, e.rx0, e.rx1, c->halo_recv + e.recv_off, 1))
                return rc;
    return 0;
}

}  // namespace

bool d3dh::plan_has_entries(const d3d_ctx *c, int plan) {
    return plan >= 0 && plan < (int)c->plans.size() && !c->plans[plan].empty();
}

// pack -> grouped point-to-point RCCL send/recv -> unpack, all queued on the ctx
// stream: no host synchronisation, no staging through host memory.
int d3dh::halo_exchange(d3d_ctx *c, int plan) {
    if (!plan_has_entries(c, plan)) return 0;
    if (!c->comm) return fail(D3D_ERR_STATE, "d3d_comm_init has not been called");
    if (int rc = halo_pack(c, plan)) return rc;
    RCCL_TRY(g_rccl.GroupStart());
    for (const d3d_ctx::HaloEntry &e : c->plans[plan]) {
        if (e.recv_n)
            RCCL_TRY(g_rccl.Recv(c->halo_recv + e.recv_off, e.recv_n, ncclFloat64, e.peer, c->comm,
                                 c->stream));
        if (e.send_n)
            RCCL_TRY(g_rccl.Send(c->halo_send + e.send_off, e.send_n, ncclFloat64, e.peer, c->comm,
                                 c->stream));
    }
    RCCL_TRY(g_rccl.GroupEnd());
    return halo_unpack(c, plan);
}

namespace {

bool plan_ok(const d3d_ctx *c, int plan) { return plan >= 0 && plan < (int)c->plans.size(); }

}  // namespace

extern "C" {

int d3d_halo_plan(d3d_ctx *c, int plan, int n, const int *entries) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(plan >= 0 && plan <= D3D_PLAN_PARAMS, D3D_ERR_INVALID, "plan %d out of range", plan);
    NEED(n >= 0 && n <= 64 && (n == 0 || entries), D3D_ERR_INVALID, "bad entry list");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<d3d_ctx::HaloEntry> v;
    size_t so = 0, ro = 0;
    for (int i = 0; i < n; ++i) {
        const int *q = entries + 10 * i;
        d3d_ctx::HaloEntry e;
        e.peer = q[0];
        e.what = q[1];
        e.sy0 = q[2]; e.sy1 = q[3]; e.sx0 = q[4]; e.sx1 = q[5];
        e.ry0 = q[6]; e.ry1 = q[7]; e.rx0 = q[8]; e.rx1 = q[9];
        NEED(e.peer >= 0 && (e.what == 0 || e.what == 1), D3D_ERR_INVALID, "entry %d: bad peer/kind", i);
        const bool s_empty = e.sy1 <= e.sy0 || e.sx1 <= e.sx0;
        const bool r_empty = e.ry1 <= e.ry0 || e.rx1 <= e.rx0;
        NEED(s_empty || (e.sy0 >= 0 && e.sy1 <= c->H && e.sx0 >= 0 && e.sx1 <= c->W), D3D_ERR_INVALID,
             "entry %d: send rectangle outside the cube", i);
        NEED(r_empty || (e.ry0 >= 0 && e.ry1 <= c->H && e.rx0 >= 0 && e.rx1 <= c->W), D3D_ERR_INVALID,
             "entry %d: receive rectangle outside the cube", i);
        const size_t E = e.what == 0 ? (size_t)c->Dp : 3;
        e.send_n = s_empty ? 0 : (size_t)(e.sy1 - e.sy0) * (e.sx1 - e.sx0) * E;
        e.recv_n = r_empty ? 0 : (size_t)(e.ry1 - e.ry0) * (e.rx1 - e.rx0) * E;
        e.send_off = so;
        e.recv_off = ro;
        so += e.send_n;
        ro += e.recv_n;
        v.push_back(e);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));  // nobody may still use the old buffers
    // Grow the buffers FIRST; the plan goes live only when both exist, so that a failed
    // allocation leaves the old plan and the old buffers as they were.
    DevBuf<double> ns, nr;
    if (so > c->halo_send.size()) HIP_TRY(ns.alloc(so));
    if (ro > c->halo_recv.size()) {
        const hipError_t e = nr.alloc(ro);
        if (e != hipSuccess)
            return fail(D3D_ERR_HIP, "hipMalloc of the halo receive buffer failed: %s", hipGetErrorString(e));
    }
    if (ns) c->halo_send = std::move(ns);
    if (nr) c->halo_recv = std::move(nr);
    if ((int)c->plans.size() <= plan) c->plans.resize(plan + 1);
    c->plans[plan] = v;
    return D3D_OK;
}

int d3d_halo_pack(d3d_ctx *c, int plan) {
    NEED(c && plan_ok(c, plan), D3D_ERR_INVALID, "bad ctx / plan");
    HIP_TRY(hipSetDevice(c->device));
    return halo_pack(c, plan);
}

int d3d_halo_unpack(d3d_ctx *c, int plan) {
    NEED(c && plan_ok(c, plan), D3D_ERR_INVALID, "bad ctx / plan");
    HIP_TRY(hipSetDevice(c->device));
    return halo_unpack(c, plan);
}

int d3d_halo_buffers(d3d_ctx *c, int plan, int entry, void **send_ptr, size_t *send_bytes,
                     void **recv_ptr, size_t *recv_bytes) {
    NEED(c && plan_ok(c, plan), D3D_ERR_INVALID, "bad ctx / plan");
    NEED(entry >= 0 && entry < (int)c->plans[plan].size(), D3D_ERR_INVALID, "bad entry %d", entry);
    const d3d_ctx::HaloEntry &e = c->plans[plan][entry];
    if (send_ptr) *send_ptr = e.send_n ? (void *)(c->halo_send + e.send_off) : nullptr;
    if (send_bytes) *send_bytes = e.send_n * sizeof(double);
    if (recv_ptr) *recv_ptr = e.recv_n ? (void *)(c->halo_recv + e.recv_off) : nullptr;
    if (recv_bytes) *recv_bytes = e.recv_n * sizeof(double);
    return D3D_OK;
}

int d3d_halo_download(d3d_ctx *c, int plan, int entry, double *host) {
    NEED(c && plan_ok(c, plan) && host, D3D_ERR_INVALID, "bad ctx / plan / buffer");
    NEED(entry >= 0 && entry < (int)c->plans[plan].size(), D3D_ERR_INVALID, "bad entry %d", entry);
    const d3d_ctx::HaloEntry &e = c->plans[plan][entry];
    HIP_TRY(hipSetDevice(c->device));
    if (e.send_n)
        HIP_TRY(hipMemcpyAsync(host, c->halo_send + e.send_off, e.send_n * sizeof(double),
                               hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_halo_upload(d3d_ctx *c, int plan, int entry, const double *host) {
    NEED(c && plan_ok(c, plan) && host, D3D_ERR_INVALID, "bad ctx / plan / buffer");
    NEED(entry >= 0 && entry < (int)c->plans[plan].size(), D3D_ERR_INVALID, "bad entry %d", entry);
    const d3d_ctx::HaloEntry &e = c->plans[plan][entry];
    HIP_TRY(hipSetDevice(c->device));
    if (e.recv_n)
        HIP_TRY(hipMemcpyAsync(c->halo_recv + e.recv_off, host, e.recv_n * sizeof(double),
                               hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_device_copy(d3d_ctx *c, void *dst, const void *src, size_t bytes) {
    NEED(c && (bytes == 0 || (dst && src)), D3D_ERR_INVALID, "NULL argument");
    if (bytes == 0) return D3D_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_comm_unique_id(void *uid) {
    NEED(uid, D3D_ERR_INVALID, "uid is NULL");
    if (int rc = load_rccl()) return rc;
    static_assert(sizeof(ncclUniqueId) == D3D_COMM_UID_BYTES, "unexpected ncclUniqueId size");
    ncclUniqueId id;
    RCCL_TRY(g_rccl.GetUniqueId(&id));
    memcpy(uid, &id, sizeof id);
    return D3D_OK;
}

int d3d_comm_init(d3d_ctx *c, int nranks, int rank, const void *uid) {
    NEED(c && uid, D3D_ERR_INVALID, "NULL argument");
    NEED(nranks >= 1 && rank >= 0 && rank < nranks, D3D_ERR_INVALID, "rank %d of %d", rank, nranks);
    NEED(!c->comm, D3D_ERR_STATE, "communicator already initialised");
    if (int rc = load_rccl()) return rc;
    HIP_TRY(hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(&id, uid, sizeof id);
    RCCL_TRY(g_rccl.CommInitRank(&c->comm, nranks, id, rank));
    c->comm_rank = rank;
    c->comm_size = nranks;
    return D3D_OK;
}

int d3d_comm_destroy(d3d_ctx *c) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    if (!c->comm) return D3D_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ncclComm_t comm = c->comm;
    c->comm = nullptr;
    RCCL_TRY(g_rccl.CommDestroy(comm));
    return D3D_OK;
}

int d3d_halo_time(d3d_ctx *c, double *ms, long *count, int reset) {
    NEED(c && ms, D3D_ERR_INVALID, "NULL argument");
    *ms = c->halo_ms;
    if (count) *count = c->halo_count;
    if (reset) {
        c->halo_ms = 0.0;
        c->halo_count = 0;
    }
    return D3D_OK;
}

int d3d_comm_info(d3d_ctx *c, int *nranks, int *rank) {
    NEED(c && nranks && rank, D3D_ERR_INVALID, "NULL argument");
    NEED(c->comm, D3D_ERR_STATE, "d3d_comm_init has not been called");
    RCCL_TRY(g_rccl.CommCount(c->comm, nranks));
    RCCL_TRY(g_rccl.CommUserRank(c->comm, rank));
    return D3D_OK;
}

int d3d_halo_exchange(d3d_ctx *c, int plan) {
    NEED(c && plan_ok(c, plan), D3D_ERR_INVALID, "bad ctx / plan");
    for (const d3d_ctx::HaloEntry &e : c->plans[plan])
        NEED(e.peer < c->comm_size, D3D_ERR_INVALID, "plan %d names peer %d of %d ranks", plan, e.peer,
             c->comm_size);
    HIP_TRY(hipSetDevice(c->device));
    return halo_exchange(c, plan);
}

int d3d_rtnorm(d3d_ctx *c, long n, double lo, double hi, double mu, double sigma, uint64_t seed,
               int wave_mode, double *out) {
    NEED(c && out, D3D_ERR_INVALID, "NULL argument");
    NEED(n >= 0 && n <= (1L << 24), D3D_ERR_INVALID, "sample count %ld out of range", n);
    // lib/rtnorm.py:66-71
    NEED(lo < hi, D3D_ERR_INVALID, "For a truncated normal, b must be greater than a.");
    NEED(sigma > 0.0, D3D_ERR_INVALID, "sigma must be positive");
    if (n == 0) return D3D_OK;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<double> buf;
    HIP_TRY(buf.alloc((size_t)n));
    if (int rc = launch_rtnorm(c, n, lo, hi, mu, sigma, seed, wave_mode, buf)) return rc;
    HIP_TRY(hipMemcpyAsync(out, buf, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D3D_OK;
}

int d3d_philox(d3d_ctx *c, long n, const uint32_t *counters, const uint32_t *keys, uint32_t *out_words,
               double *out_pairs) {
    NEED(c && counters && keys && out_words && out_pairs, D3D_ERR_INVALID, "NULL argument");
    NEED(n >= 0 && n <= (1L << 24), D3D_ERR_INVALID, "block count %ld out of range", n);
    if (n == 0) return D3D_OK;
    HIP_TRY(hipSetDevice(c->device));
    // one allocation: pairs [2n] doubles | counters [4n] | keys [2n] | words [4n]
    const size_t nn = (size_t)n;
    DevBuf<char> buf;
    HIP_TRY(buf.alloc(nn * (2 * sizeof(double) + 10 * sizeof(uint32_t))));
    double *d_pairs = reinterpret_cast<double *>(buf.get());
    uint32_t *d_counters = reinterpret_cast<uint32_t *>(buf + nn * 2 * sizeof(double));
    uint32_t *d_keys = d_counters + 4 * nn;
    uint32_t *d_words = d_keys + 2 * nn;
    hipError_t e = hipMemcpyAsync(d_counters, counters, nn * 4 * sizeof(uint32_t), hipMemcpyHostToDevice,
                                  c->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_keys, keys, nn * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        HIP_TRY(e);
    }
    if (int rc = launch_philox(c, n, d_counters, d_keys, d_words, d_pairs)) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    e = hipMemcpyAsync(out_words, d_words, nn * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(out_pairs, d_pairs, nn * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    HIP_TRY(e);
    HIP_TRY(es);
    return D3D_OK;
}

int d3d_colour_count(d3d_ctx *c, int colour, int *count) {
    NEED(c && count, D3D_ERR_INVALID, "NULL argument");
    NEED(c->have_data, D3D_ERR_STATE, "data not set");
    NEED(colour >= 0 && colour < c->fh * c->fw, D3D_ERR_INVALID, "colour %d out of range", colour);
    *count = c->colour_real[colour];
    return D3D_OK;
}

}  // extern "C"

