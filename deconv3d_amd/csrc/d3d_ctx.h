// Internal header of libdeconv3d_hip.so: the context struct and the launch
// functions shared by the library's translation units (d3d_api.hip: C ABI and host
// logic; d3d_spatial.hip: line / LSF / FSF kernels; d3d_mh.hip: the MH-within-Gibbs
// kernels; d3d_sweep.hip: the sweep driver; d3d_post.hip: posterior moments and histograms;
// d3d_region.hip: region posteriors; d3d_search.hip: the matched-filter line search; d3d_prep.hip:
// continuum removal and channel noise of a raw cube; d3d_temper.hip: replica exchange between
// tempered chains; d3d_robust.hip: the per-voxel weights of a Student-t likelihood; d3d_pred.hip:
// lppd and WAIC per voxel; d3d_noise.hip: the variance factors of channel groups).
// Ownership: every device allocation is a DevBuf, freed by whoever holds it -- the context or group
// it is a member of (their `delete`), or the call it is a local of.  An optional feature's state is
// one sub-struct of the context, and its *_end is `c->feature = {}`: buffers freed, fields back at
// their defaults (Post, Hist, Regions, Adapt, Prior, Robust, Pred, Noise; and Rescale, which whichever of
// Robust and Noise rewrites SLOT_IVAR holds: rescale_disarm is its `c->rescale = {}`, the base cube put
// back first).  A DevBuf never synchronises: whoever frees one has drained the stream that uses it.
// Not installed: the public interface is include/deconv3d_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is dlopen()ed by d3d_comm_init

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/deconv3d_hip.h"
#include "d3d_kernels.h"
#include "d3d_strip_order.h"
#include "d3d_strips.h"
#include "d3d_taps.h"
#include "d3d_worklists.h"

// The WIDE form of a small colour launch at 128 channels: eleven
// streaming wavefronts per window instead of four -- one per window row of an 11 x 11 FSF
// -- in workgroups of 768 threads.
// (round 4, same-box A/B with k_mh_small through tools/build_variant.sh -DD3D_WIDE_NS=512: eight
// wavefronts, two per SIMD, 11.95 us per launch of an 8x1 strip against 11.79 with eleven)
#ifndef D3D_WIDE_NS
#define D3D_WIDE_NS 704
#endif
constexpr int MH_WIDE_NS = D3D_WIDE_NS;
// k_mh_chain: at most this many threads per workgroup (three wavefronts per SIMD: 168
// registers each, of which a thread's column of an 11-row window takes 88)
constexpr int MH_CHAIN_NT = 768;
// (MH_STRIPS_AUTO, MH_STRIP_ORDER_AUTO: d3d_worklists.h)

namespace d3dh {
// sets the thread-local message d3d_last_error() returns; returns `code`
int fail(int code, const char *fmt, ...);
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return d3dh::fail(D3D_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                              __FILE__, __LINE__);                                      \
    } while (0)

#define NEED(cond, code, ...) \
    do {                      \
        if (!(cond)) return d3dh::fail(code, __VA_ARGS__); \
    } while (0)

namespace d3dh {
// bytes of device memory the DevBufs of this process hold (read-only option device_bytes)
inline std::atomic<size_t> dev_bytes{0};
}

// One device allocation of n elements, owned (move-only).  No contents survive alloc / reserve.
template <typename T>
class DevBuf {
    T *p_ = nullptr;
    size_t n_ = 0;

   public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
        o.reset();
        return *this;
    }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t n) {  // on failure it holds nothing
        reset();
        const hipError_t e = hipMalloc(&p_, n * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            return e;
        }
        n_ = n;
        d3dh::dev_bytes += n * sizeof(T);
        return e;
    }
    hipError_t reserve(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }  // grow-only
    void reset() {
        if (p_) (void)hipFree(p_);
        d3dh::dev_bytes -= n_ * sizeof(T);
        p_ = nullptr;
        n_ = 0;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t size() const { return n_; }
};

struct d3d_ctx {
    int device = 0;
    int D = 0, H = 0, W = 0, fh = 0, fw = 0;
    int Dp = 0, HL = 0, N = 0;
    bool deep = false;  // more than 1024 channels: the z-blocked kernel forms (k_*_deep)
    long HW = 0;
    size_t cube_elems = 0;  // HW * Dp
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    DevBuf<double> slot[D3D_SLOT_COUNT];
    DevBuf<double> stage;   // D*HW doubles, host-layout staging
    DevBuf<double> stage2;  // second staging (variance)
    DevBuf<double> params;  // HW*3
    DevBuf<double> params_alt;  // HW*3: parameter map of d3d_simulate (not the chain state)
    DevBuf<uint8_t> mask;   // HW
    DevBuf<double> fsf;     // fh*fw
    DevBuf<int> lsf_shift;
    DevBuf<double> lsf_weight;
    int ntaps = 0;
    DevBuf<double> dlog;  // HW
    DevBuf<double> hwbuf; // HW scratch (chi2 map)
    DevBuf<double> scal;  // small device scalars (8 doubles)
    DevBuf<unsigned long long> accepted;
    DevBuf<unsigned> acc_map;  // [HW] accepted moves per spaxel since the last accepted_collect (MHArgs::acc_map)
    DevBuf<int4> spx;  // work lists per (part, colour): real spaxels first, then virtual ones
    std::vector<int> colour_real;  // fh*fw: number of real spaxels of each colour (all parts)
    // the parts of a sweep and their work lists (d3d_worklists.h decides them, build_colour_lists uploads)
    using Part = d3d_worklists::Part;
    std::vector<Part> parts;
    std::vector<d3d_worklists::Rect> part_rects;  // as given to d3d_set_parts (.phase apart)
    std::vector<int> part_phase;
    int n_phases = 1;
    int pend_part = -1;            // part the pending layers belong to
    // halo plans (tiled chains): per plan a list of rectangle copies to / from peers
    struct HaloEntry {
        int peer = 0, what = 0;                   // what: 0 = SLOT_ERR cells, 1 = parameter map
        int sy0 = 0, sy1 = 0, sx0 = 0, sx1 = 0;  // rectangle sent (local), empty when sy1 <= sy0
        int ry0 = 0, ry1 = 0, rx0 = 0, rx1 = 0;  // rectangle received (local)
        size_t send_off = 0, send_n = 0, recv_off = 0, recv_n = 0;  // in doubles
    };
    std::vector<std::vector<HaloEntry>> plans;
    DevBuf<double> halo_send, halo_recv;
    // asynchronous chain streaming (lib/run.py:447-451 chain[i] = parameters, :428-432):
    // at a saved sweep the compute stream snapshots parameters + log ratios device to
    // device (microseconds), a COPY stream moves the snapshot to a pinned host buffer,
    // and the host thread copies it into the caller's (pageable) chain while the GPU
    // runs on -- STREAM_NB snapshots may be in flight
    static constexpr int STREAM_NB = 4;
    hipStream_t copy_stream = nullptr;
    DevBuf<double> snap_dev[STREAM_NB]; // [HW*4]: params (HW*3) | dlog (HW)
    double *snap_host[STREAM_NB] = {};  // pinned
    hipEvent_t snap_ready[STREAM_NB] = {}, snap_done[STREAM_NB] = {};
    // lattice-row strips of a colour row (Part::strips): strip 0 runs on `stream`, strip s > 0 on
    // strip_stream[s - 1]; one fork and one join per colour row, or -- chained -- per sweep (run_part).
    // Created on first use.
    static constexpr int STRIP_AUX = 3;
    hipStream_t strip_stream[STRIP_AUX] = {};
    hipEvent_t strip_fork = nullptr, strip_join[STRIP_AUX] = {};
    int mh_strips_opt = 0;        // option mh_strips: 0 automatic, 1 off, 2..4 that many strips (forced: also
                                  // where the colour launches do not fill the chip)
    // the chained order (d3d_strip_order.h): its events; the G buffer behind every slot the schedule names
    // (the pending layers always lie in the pool the sweep's first row does not write); the pool that row takes
    hipEvent_t strip_ev[d3d_strip_order::NEV] = {};
    int strip_gbuf[d3d_strip_order::GSLOTS] = {0, 1, 2, 3, 4, 5, 6, 7};
    int strip_pool = 0;
    int mh_strip_order_opt = 0;   // option mh_strip_order: 0 automatic, 1 joined after every colour row, 2 chained
    int mh_strip_lag = 0;         // test option mh_strip_lag: s + 1 delays strip s at the start of every colour row
    // RCCL communicator of the tiled chain (d3d_comm_init)
    ncclComm_t comm = nullptr;
    int comm_rank = -1, comm_size = 0;
    // option halo_timing = 1: HIP events around every halo exchange of d3d_mh_sweeps
    int halo_timing = 0;
    static constexpr size_t HALO_RING = 64;  // event pairs in flight at most
    std::vector<hipEvent_t> halo_ev;   // ring of pairs (start, stop), recorded on the ctx stream
    size_t halo_ev_used = 0, halo_ev_head = 0;  // pairs in flight, oldest pair
    double halo_ms = 0.0;              // summed at the end of each d3d_mh_sweeps call
    long halo_count = 0;
    std::vector<uint8_t> h_mask;
    std::vector<uint8_t> h_user_mask;  // the caller's mask alone, without the NaN rule (d3d_line_search)

    d3d::LineShape line = {1, {0.0, 0.0, 0.0, 0.0}, {1.0, 0.0, 0.0, 0.0}, nullptr, 0, 0.0, 0.0};  // d3d_set_line_shape
    // d3d_set_line_table: line_tab owns the device copy (n + 2 doubles) that line.tab points to, h_line_tab
    // holds the n samples on the host (d3d_mh_sweeps_batch compares them), line_tab_flux the integral of phi
    DevBuf<double> line_tab;
    std::vector<double> h_line_tab;
    double line_tab_flux = 0.0;
    bool have_taps = false, have_data = false, have_params = false, have_cfg = false;
    bool err_valid = false;
    double min_b[3] = {}, max_b[3] = {}, amp[3] = {};
    double ra = 0;
    uint64_t seed = 0;
    int refresh_every = 1000;
    uint32_t sweep_origin = 0;  // Philox sweep index of sweep s is s + sweep_origin (resumed runs)

    int mh_nt = 0, mh_maxit = 0;  // MH kernel geometry (derived: apply_mh_options)
    int mh_nt_opt = 0, mh_maxit_opt = -1;  // options mh_nt / mh_maxit (0 / -1: chosen per shape)
    int mh_defer = 1;             // deferred residual write-back in effect (pick_mh_geometry: mh_defer_opt,
                                  // 0 for deep cubes that cannot take the z-blocked kernels)
    int mh_defer_opt = 1;         // option mh_defer
    int mh_zblocks = 1;           // option mh_zblocks = 0: cubes deeper than 512 channels keep k_mh_defer / k_mh_deep
    bool mh_zb = false;           // the z-blocked kernels run (k_mh_ws<..., ZBK> + k_mh_zdecide)
    DevBuf<double> z_part;        // [strip][items of a launch][blocks][4 waves][8] wave sums (launch_mh_zb)
    DevBuf<double> z_E;           // [2][slots][Dp] lines of the updates of the last colour class
#ifdef D3D_EXPERIMENTS
    DevBuf<unsigned long long> stampbuf; // D3D_MH_STAMP=1: [launch][workgroup][8]
    size_t stamp_launches = 0, stamp_next = 0, stamp_stride = 0;
#endif
    bool ivar_is_uniform = false; // SLOT_IVAR holds one constant (k_mh_ws<.., true> skips reading it)
    double ivar_uniform = 0.0;
    int uniform_fast_path = 1;    // option uniform_ivar = 0 turns the variant off
    static constexpr int GBUFS = 8;
    DevBuf<double> gbuf[GBUFS];  // update coefficients [slots][Dp]; 4 .. 7 only where colour rows run in strips
    // pending layers, oldest first: colour class and G buffer of each update that has
    // not been written into SLOT_ERR yet (k_mh_ws applies up to mh_layers of them)
    int lay_n = 0, lay_cy[3] = {-1, -1, -1}, lay_cx[3] = {-1, -1, -1}, lay_g[3] = {0, 0, 0};
    int mh_layers = 2;            // most pending layers any part uses (d3d_mh_layers)
    int batch_layers = 0;         // pending layers of the last d3d_mh_sweeps_batch this context was in (0: none yet)
    bool mh_nt_ivar = false;      // 1/variance loads non-temporal: residual + 1/variance exceed the Infinity Cache
    int mh_nt_ivar_opt = -1;      // option mh_nt_ivar: -1 by working set, 0 / 1 forced (within the raw buffer's 2 GiB)
    int mh_zigzag = 1;            // option mh_zigzag: odd colour ordinals walk windows / work lists backwards (MHArgs::rev)
    int mh_layers_opt = 0;        // option mh_layers: 0 chosen per part, 1..3 forced
    int mh_layers_cfg = 2;        // derived: layers of a part whose launches fill the chip
    bool mh_layers_forced = false;
    // dataflow kernel (k_mh_flow): one launch per sweep
    int mh_flow = 0;              // D3D_MH_FLOW=1: one launch per sweep (k_mh_flow; measured
                                  // slower than one k_mh_ws launch per colour: DESIGN.md)
    int flow_K = 0, flow_LY = 0, flow_LX = 0, flow_items = 0, flow_grid = 0;
    int flow_last_cy = -1, flow_last_cx = -1;  // colour class of the last active colour
    // k_mh_pair (two colour classes per launch): per-item flags with epochs and a
    // monotonic ticket counter, so that nothing needs clearing between launches
    int mh_chain_opt = 0;          // option mh_chain (EXPERIMENTS builds): 1 = k_mh_chain wherever a part's
                                   // slots are all resident; measured no faster than the colour launches
                                   // (profiles/r03_chain_phases.txt)
    DevBuf<int2> chain_cols;       // [parts][fh*fw] local residues of each part's active colours
    DevBuf<unsigned> chain_flags;  // [2][size() / 2]: flag1 | flag2 (monotonic epochs)
    DevBuf<double> chain_G;        // [2][K][slots][Dp] G rows | [slots][K][2][Dp] unit lines of a sweep
    unsigned chain_base = 0;       // the epoch every flag of a finished launch holds
    bool chain_used = false;       // a chain launch ran since the error word was last read
    int mh_props = 1;              // option mh_props: the proposals of a sweep in one launch before its colours
    DevBuf<d3d::MHProposal> props; // [HW]
    long props_sweep = -1;         // the sweep (Philox number) the table holds, -1 = none
    int mh_prio = 0;               // option mh_prio: staggered completion by wave priority (MHArgs::prio)
    int mh_small = 1;              // option mh_small = 0: small colour launches keep round 3's k_mh_ws variants instead of k_mh_small
    DevBuf<double> ptab;           // [(fh fw + 1)][fh fw][4] relative position tables of k_mh_small (ensure_proposals)
    bool ptab_valid = false;       // (d3d_set_taps invalidates them)
    DevBuf<double> ltab;           // [HW][2][Dp] line table of the current sweep (k_mh_line_table), allocated on first use
    int mh_wide = 1;               // option mh_wide = 0: never the wide form for the small launches of a partitioned context
    int mh_pair = 0;               // D3D_MH_PAIR=1: two colour classes per launch (k_mh_pair;
                                   // measured 43.0 vs 42.0 us per colour: opt-in)
    DevBuf<unsigned> pair_state; // [0] ticket counter | [4 ..] done flags per item
    unsigned pair_epoch = 0, pair_tickets = 0;
    std::vector<int> flow_first;   // first item of every active colour (+ total)
    std::vector<int> flow_colour;  // colour class index of every active colour
    DevBuf<int4> flow_ent;        // [items] {y, x, real, colour ordinal}
    DevBuf<int4> flow_col;        // [K] {first ticket, cy, cx, -}
    DevBuf<int> flow_lat;         // [K][LY*LX]
    DevBuf<unsigned> flow_state; // one block, zeroed per launch: ctl[4] | cnt[K] | done[items]
    DevBuf<unsigned> flow_err;   // sticky error word of k_mh_flow
    size_t flow_state_bytes = 0, flow_cap_items = 0, flow_cap_K = 0;
    int slots_x = 0, slots = 0;
    int gy0 = 0, gx0 = 0, Wg = 0;    // tile origin / global width (RNG keys)
    bool tiled = false;              // d3d_set_tile was called
    int oy0 = 0, oy1 = 0, ox0 = 0, ox1 = 0;  // owned local rectangle
    DevBuf<double> prev;          // [HW*3] parameters before each spaxel's last update
    DevBuf<double> recbuf;        // [HW*8] staging of update records
    DevBuf<int> idxbuf;           // [HW] staging of spaxel lists
    DevBuf<double> extbuf;           // external-lines staging of d3d_mh_colour_lines: [spaxels][6 + 2D] doubles
    bool fsf_sep = false;         // fsf == u v^T to rounding (k_spatial_sep); D3D_SPATIAL_SEP=0 disables
    int sep_fuse = 1;             // LSF in the same pass (k_spatial_sep_lsf); option sep_fuse = 0 disables
    int spatial_sep = 1;          // option spatial_sep = 0: treat an outer-product FSF as a general one
    DevBuf<double> sep_uv;        // [fh + fw] on the device
    bool fsf_symx = false;        // fsf[k][i] == fsf[k][fw-1-i] bit for bit
    bool fsf_symy = false;        // fsf[k][i] == fsf[fh-1-k][i] bit for bit
    DevBuf<double> fsf_quad;      // [(fhh+1)^2] quadrant taps of an x/y-symmetric square FSF (k_conv_rows)
    DevBuf<double> fsf_quad_sep; // the same table for an outer-product FSF: row 0 = v, row 1 = u
    bool fsf_symt = false;        // ... and fsf[k][i] == fsf[i][k] bit for bit (radial FSFs)
    bool lsf_dense_sym = false;   // dense LSF weights mirror-symmetric bit for bit
    int conv_rows = 1;            // D3D_CONV_ROWS=0: never use the one-pass kernel k_conv_rows
    int conv_zb = 1;              // option conv_zb = 0: depths above 128 keep the march kernels (no z-blocks)
    DevBuf<double> lsf_dense;     // [2*LSF_RL+1] dense LSF weights for the fused epilogue
    bool lsf_dense_ok = false;    // taps within +-LSF_RL and power-of-two depth (z-major spectral kernel)
    bool lsf_dense_any = false;   // taps within +-LSF_RL channels at ANY depth (k_spectral_blocks)
    int spectral_blocks = 1;      // option spectral_blocks = 0: never use k_spectral_blocks
    int lines_dense = 1;          // option lines_dense: 0 the line cube by the tap-list kernel (k_lines); 1 by
                                  // k_lines_dense where the LSF is applied with it (k_lines' bits); 2 always,
                                  // with its own exp (within 2 ulp; measured 7-10 % faster: not the default);
                                  // 3 always, with the library's exp (tests)
    int lines_rounds = 0;         // option lines_rounds: spaxel rounds per wavefront of k_lines_dense (0: by size)
    bool lsf_fusable = false;     // taps within +-LSF_RL, power-of-two depth, strip within a wave
    int spectral_dense = 1;       // D3D_SPECTRAL_DENSE=0: always the general tap-list kernel
    int spectral_shfl = 0;        // D3D_SPECTRAL_SHFL=1: wavefront shuffles instead of the LDS window
    int fuse_lsf = 0;             // D3D_FUSE_LSF=1: LSF in the march epilogue (correct; slower today: register spills)
    int march_hy = 16;            // output rows per strip of the march kernel (derived in d3d_set_taps)
    int march_hy_opt = 0;         // option march_hy (0: chosen per shape)
    int conv_hy_opt = 0;          // option conv_hy: rows per strip of k_conv_rows (0: one strip per CU)
    int zmajor = 1;               // option zmajor = 0: d3d_convolve never uses the reference-layout kernels
    int zmajor_hy = 0;            // output rows per strip of the z-major spatial kernel (0: by shape)
    int sp_nt_opt = 0;            // option spatial_nt: workgroup size of the spatial kernels (0: by depth)
    int xcd_remap = 1, alt_dir = 1, stagger = 0;  // march kernels: workgroup -> XCD mapping, strip direction
    // host copies of the taps, so that an option that changes their analysis can redo it
    std::vector<double> h_fsf, h_lsf;
    bool h_has_lsf = false;
    double h_thr = 0.0;
    int march_one = 0;            // D3D_MARCH_ONE=2|3: one-channel-per-lane variant, TX columns
    int march_pf = 0;             // D3D_MARCH_PF=2|3: software-pipelined variant, TX columns
    // 0: tile kernel; 1: march; 2: march + the mirror symmetries the FSF has (x, and y on
    // top of x); 3: march + x symmetry only
    int march_mode = 2;
    int sp_nt = 256;              // spectral / spatial block size
    int march_stamp = 0;          // option march_stamp (EXPERIMENTS builds): phase stamps of the march kernel
    int post_nt = 0;               // option post_nt = 1: the moments' accumulators' loads and stores non-temporal
    // The optional features, one sub-struct each: nothing is allocated before its d3d_*_begin, and
    // `c->feature = {}` frees it and puts every field back (the caller has drained the stream).
    // posterior moments (d3d_post_*): running mean and M2 = sum of squared deviations of the
    // samples' clean cube, convolved cube and (a, c, w, F) map, updated on the device after the
    // scheduled sweeps (k_post_accum)
    struct Post {
        bool on = false;
        int what = 0;             // bit 0 clean cube, bit 1 convolved cube
        DevBuf<double> cube[4];   // clean mean | clean M2 | convolved mean | convolved M2, device layout
        DevBuf<double> map;       // [2][HW*4]: mean | M2 of (a, c, w, F)
        int64_t n = 0;            // samples accumulated
        int first = 0, every = 0; // d3d_post_schedule (every == 0: none)
    } post;
    // posterior histograms (d3d_hist_*): per spaxel and per quantity of post.map 64 equal bins and
    // two tail counters over a range frozen from the moments of the first `pilot` samples
    // (k_hist_freeze); every later sample is binned (k_hist_accum)
    struct Hist {
        bool on = false, frozen = false;
        int64_t pilot = 0;        // samples that feed the moments only
        double span = 0.0;        // the range is mean +- span * sd of the pilot, clipped to the bounds
        DevBuf<uint32_t> bins;    // [HW*4][64]
        DevBuf<uint32_t> tails;   // [HW*4][2]: below | above
        DevBuf<double> range;     // [HW*4][2]: lo | hi (NaN: not frozen yet, or masked)
    } hist;
    // region posteriors (d3d_region_*): per sample of the moments the (F, C, S) of every labelled set
    // of spaxels into a series, and its summed clean spectrum into a mean and M2 (d3d_region.hip)
    struct Regions {
        bool on = false;
        int K = 0, what = 0;      // regions 1..K; bit 0 of what: the spectra
        int64_t rows = 0;         // rows of the series (the caller's capacity)
        int nchunks = 0;
        std::vector<int32_t> h_labels;  // the caller's (H,W) map: d3d_set_data lays the members out again
        std::vector<int32_t> h_sizes;   // [K] members of every region
        DevBuf<int> member;       // [members] spaxels, region after region
        DevBuf<int4> chunk;       // [chunks] {first member, members, region, -}
        DevBuf<int> first;        // [K + 1] first chunk of every region
        DevBuf<double> part;      // [chunks][4] scalar partials
        DevBuf<double> fc;        // [K][2] F and C between the passes
        DevBuf<double> series;    // [rows][K][3]
        DevBuf<double> spart;     // [chunks][Dp] spectrum partials (spectra on)
        DevBuf<double> spec;      // [2][K][Dp] mean | M2 (spectra on)
    } reg;
    // per-spaxel jump scales (d3d_adapt_*): every `window` sweeps of d3d_mh_sweeps each spaxel's
    // scale moves towards the target acceptance rate (k_mh_adapt), up to sweep `last`; the counters
    // then go on counting
    struct Adapt {
        bool on = false;
        DevBuf<double> jscale;    // [HW] multiplicative jump scale of every spaxel
        DevBuf<unsigned> jacc;    // [HW] accepted proposals since the counters were last cleared
        double target = 0.0, gain = 0.0, min = 0.0, max = 0.0;
        int window = 0;           // sweeps per adaptation step (0: a fixed map that never adapts)
        int64_t last = 0;         // no step after this sweep (the run's numbering: s + sweep_origin)
        int64_t n_win = 0;        // sweeps counted since the counters were last cleared
        int64_t k = 0;            // adaptation steps taken
    } adapt;
    // smoothness prior between 4-neighbours (d3d_prior_*): lam[k] = 1 / sigma_k^2 of (a, c, w), read by
    // every MH decision (MHArgs::lam).  `part` is allocated by the first d3d_prior_energy and kept.
    struct Prior {
        bool on = false;
        double lam[3] = {0.0, 0.0, 0.0};
        DevBuf<double> part;      // [PRIOR_BLOCKS + 1][4] block partials | totals of k_prior_energy
    } prior;
    // variance rescaling (d3dh::rescale_*): at most one feature -- the holder -- rewrites SLOT_IVAR from the
    // base 1/variance after the due sweeps.  Every other writer of SLOT_IVAR refuses while it is held.
    struct Rescale {
        enum Who { NONE, ROBUST, NOISE } who = NONE;  // the holder (d3d_robust_begin / d3d_noise_begin)
        bool was_uniform = false; // ivar_is_uniform before arming (false while armed)
        int every = 1;
        int64_t start = 0;        // due: s >= start and (s - start) % every == 0, the run's numbering
        DevBuf<double> i0;        // the base 1/variance d3d_set_data left in SLOT_IVAR, device layout
    } rescale;
    // Student-t likelihood (d3d_robust_*): after the due sweeps k_robust_step redraws one weight per
    // voxel from the residual and writes SLOT_IVAR = weight * base 1/variance (holds `rescale`)
    struct Robust {
        bool on = false;
        int nu = 0;
        int64_t accum_from = 0;   // draws of the sweeps from this one on enter the weight mean
        int64_t count = 0;        // draws in the weight mean
        DevBuf<double> mean;      // running mean of the weights, device layout (0 where i0 == 0)
    } robust;
    // pointwise predictive accuracy (d3d_pred_*): per voxel and per sample of the moments the
    // chain-varying part q of the log density of the residual -- its running maximum M, S = sum
    // exp(q - M), and Welford's mean and M2 (k_pred_accum); lppd and the WAIC penalty at extraction
    struct Pred {
        bool on = false;
        int nu = 0;               // the likelihood of every sample: 0 Gaussian, else the armed robust.nu
        DevBuf<double> cube[4];   // M | S | mean | M2, device layout (0 where the voxel is not counted)
    } pred;
    // noise-scale inference (d3d_noise_*): every group of channels has a variance factor s_g with an
    // inverse-gamma prior; after the due sweeps k_noise_sums / k_noise_draw redraw tau_g = 1 / s_g from
    // the residual and k_noise_apply writes SLOT_IVAR = base 1/variance * tau of the channel's group
    // (holds `rescale`)
    struct Noise {
        bool on = false;
        bool has_spaxels = false; // a map of counted spaxels was given (else every spaxel)
        int G = 0;
        double shape = 0.0, rate = 0.0;  // the prior InvGamma(shape, rate) of every s_g
        int64_t capacity = 0, draws = 0; // rows of the series, rows written
        std::vector<int64_t> sweeps;     // the sweep (the run's numbering) of every row
        DevBuf<int> group;        // [D] group of every channel, -1: never rescaled
        DevBuf<uint8_t> spaxels;  // [HW] 0/1 counted spaxels (has_spaxels)
        DevBuf<double> part_q;    // [NOISE_STREAMS][Dp] partial sums of r^2 i0
        DevBuf<unsigned> part_n;  // [NOISE_STREAMS][Dp] partial counts
        DevBuf<double> chan;      // [2][Dp] sum | count of every channel
        DevBuf<double> tau;       // [Dp] precision factor of every channel (1: not rescaled; the pad channel)
        DevBuf<double> tau_g;     // [3][G] tau | counted voxels | last sum of every group
        DevBuf<double> series;    // [capacity][G] the scales s_g = 1 / tau_g (NaN: a group of fewer than 2 voxels)
    } noise;
    // option noise_timing = 1: d3d_noise_step records HIP events around its three kernels; their device
    // time in the last such call (read-only options noise_sums_ns / noise_draw_ns / noise_apply_ns)
    int noise_timing = 0;
    long noise_ns[3] = {0, 0, 0};
    // d3d_line_search: device time of the last call's bank build (lines + transpose, or the transpose
    // of a host bank) and of its search kernel, by HIP events (read-only options search_bank_ns /
    // search_kernel_ns)
    long search_bank_ns = 0, search_kernel_ns = 0;
    // d3d_running_median / d3d_channel_stats / d3d_prepare: device time of the last call's
    // running-median and channel-statistics kernels (both passes of a rejecting d3d_prepare summed),
    // by HIP events (read-only options prep_median_ns / prep_stats_ns)
    long prep_median_ns = 0, prep_stats_ns = 0;
    // kernel family the last launch_spatial / launch_spectral / d3d_stage_convolve took (read-only
    // options spatial_path / spectral_path / stage_path: D3D_SPATIAL_*, D3D_SPECTRAL_*, D3D_STAGE_*)
    int spatial_path = 0, spectral_path = 0, stage_path = 0;
    // what the launchers of d3d_mh.hip launched (read-only options mh_path / mh_path_layers /
    // mh_path_launches): the D3D_MH_* code of the last sweep-kernel launch, the pending-layer counts
    // the launches found (bit n: n layers), the launches -- since d3d_mh_config or the last read of
    // mh_path_launches.  Written by the host thread that launches, strips included.
    struct MHPath {
        int code = 0;
        unsigned layers = 0;
        long launches = 0;
    } mh_path;
};

namespace d3dh {

// ---- d3d_spatial.hip: line build, LSF and FSF passes ---------------------------------
int pick_nt(int HL);  // block size of the group-per-spaxel kernels: at least HL threads
// params: (H,W,3) map on the device (NULL: the chain state c->params)
int launch_lines(d3d_ctx *c, double *out, int convolved, const double *params = nullptr);
int launch_spectral(d3d_ctx *c, const double *in, double *out);
bool conv_rows_usable(const d3d_ctx *c, bool with_lsf);
bool can_fuse_lsf(const d3d_ctx *c);
// out = FSF (*) in, or data - FSF (*) in when data != NULL.  in != out.
// fuse_lsf: also apply the LSF along z (only when can_fuse_lsf()).
int launch_spatial(d3d_ctx *c, const double *in, double *out, const double *data,
                   bool fuse_lsf = false);
// params -> SLOT_TMP0 (LSF lines) -> dst (sim, or residual when resid)
int forward_into(d3d_ctx *c, double *dst, bool resid);
// d3d_post.hip: one sample (the chain state; SLOT_SIM holds its convolved cube when that moment
// is on) into the running moments, as sample number c->post.n + 1
int launch_post_accum(d3d_ctx *c);
// d3d_post.hip, posterior histograms: the ranges from the moments as they are (c->post.n samples);
// the chain state into its bins; quantiles, mode and outside share of every histogram into device
// buffers [HW*4][n_q], [HW*4], [HW*4] (any may be NULL)
int launch_hist_freeze(d3d_ctx *c);
int launch_hist_accum(d3d_ctx *c);
int launch_hist_quantiles(d3d_ctx *c, int n_q, const double *q, double *quantiles, double *mode, double *outside);
// d3d_post.hip: F = a w flux_factor(c)
double flux_factor(const d3d_ctx *c);
// d3d_region.hip: the members, chunks and chunk offsets of c->reg.h_labels under c->h_mask; one
// sample (the chain state) into the series and the spectra, as sample number c->post_n + 1
void region_layout(const d3d_ctx *c, std::vector<int> &member, std::vector<int4> &chunk, std::vector<int> &first,
                   std::vector<int32_t> &sizes);
int launch_region_sample(d3d_ctx *c);
// d3d_mh.hip: after sweep `s` of a d3d_mh_sweeps call (d3d_adapt_begin): the sweep is counted and,
// where it fills a window at or before the last adapted sweep, the jump scales take a step
int adapt_after_sweep(d3d_ctx *c, int s);
// d3d_mh.hip: the accepted moves the decisions left in c->acc_map, added to *c->accepted (on the
// context's stream); every read of the counter is preceded by it
int accepted_collect(d3d_ctx *c);
// d3d_mh.hip: sums of squared neighbour differences of a parameter map on the device over the
// adjacent pairs of unmasked spaxels, {E_a, E_c, E_w, pairs} (k_prior_energy)
int prior_energy(d3d_ctx *c, const double *params_dev, double out4[4]);
// d3d_search.hip: the matched-filter search of d3d_line_search (arguments already validated).  The
// template bank is refused above this many bytes of device memory.
constexpr size_t SEARCH_BANK_BUDGET = (size_t)256 << 20;
int line_search(d3d_ctx *c, int n_c, const double *centres, int n_w, const double *widths,
                const double *host_bank, int *best_out, double *stat_out);
// d3d_prep.hip: d3d_running_median, d3d_channel_stats and d3d_prepare (arguments already validated);
// every buffer lives inside the call
int prep_running_median(d3d_ctx *c, const double *cube, const uint8_t *valid, int half_window, double *out);
int prep_channel_stats(d3d_ctx *c, const double *cube, const uint8_t *select, double *m_out, double *mad_out,
                       int64_t *n_out);
int prep_prepare(d3d_ctx *c, const double *cube, const uint8_t *select, int half_window, double reject,
                 double *continuum_out, double *residual_out, double *chan_out);
bool zmajor_ok(const d3d_ctx *c);
// LSF (x) FSF of c->stage in the reference layout (D,H,W), in place (zmajor_ok())
int launch_zmajor_convolve(d3d_ctx *c);

// ---- d3d_post.hip: what the sweep driver runs between and after the sweeps; what the setters call
int post_sample(d3d_ctx *c);               // the chain state as one more sample of the posterior moments
bool post_due(const d3d_ctx *c, int s);    // sweep s (the caller's numbering) is one d3d_post_schedule asked for
int post_reset(d3d_ctx *c);                // count 0, every accumulator of moments, histograms and regions zero
// d3d_region.hip: the members of the regions under the mask in force, on the device (d3d_set_data:
// the mask may have changed); on failure the regions are freed
int region_members(d3d_ctx *c);
// ---- d3d_api.hip ---------------------------------------------------------------------------
bool plan_has_entries(const d3d_ctx *c, int plan);
int halo_exchange(d3d_ctx *c, int plan);
// a cube in the device layout into a host array (D,H,W), synchronously (through c->stage)
int download_device_cube(d3d_ctx *c, const double *src, double *host);

// `c` and `L` can share a launch or trade state: same device and shape, same mask, FSF and LSF, same line
// shape and table.  NULL, or what differs (d3d_mh_sweeps_batch, d3d_temper_create).
const char *setup_differs(const d3d_ctx *c, const d3d_ctx *L);

// ---- variance rescaling (d3d_ctx::Rescale; defined in d3d_api.hip) ------------------------------
// the wording of a refusal: what the context's holder is called, and its <api> in d3d_<api>_begin / _end
struct RescaleName {
    const char *what, *api;
};
RescaleName rescale_name(const d3d_ctx *c);
// 0, or the refusal of `who`: another feature holds the rescale (d3d_*_begin, ahead of their other checks)
int rescale_free_for(const d3d_ctx *c, d3d_ctx::Rescale::Who who);
// `who` takes the rescale (the caller has drained the stream): the base cube copied out of SLOT_IVAR and
// waited for, ivar_is_uniform saved and cleared.  Refused while another feature holds it; where `who`
// holds it already, the base cube first goes back.  On failure nothing is held and the context stays usable.
int rescale_arm(d3d_ctx *c, d3d_ctx::Rescale::Who who, int every, int64_t start);
// where `who` holds it: the base cube back into the slot (on the context's stream, waited for),
// ivar_is_uniform restored, c->rescale = {}.  Nothing otherwise.
void rescale_disarm(d3d_ctx *c, d3d_ctx::Rescale::Who who);
bool rescale_due(const d3d_ctx *c, int s);   // sweep s (the caller's numbering) is followed by the holder's draw
int rescale_after_sweep(d3d_ctx *c, int s);  // where due: the pending layers written back, then the draw
// the base 1/variance: the saved cube while the rescale is held, else SLOT_IVAR
inline const double *rescale_base(const d3d_ctx *c) {
    return c->rescale.who ? c->rescale.i0.get() : c->slot[D3D_SLOT_IVAR].get();
}

// ---- d3d_robust.hip: the weights of a Student-t likelihood --------------------------------
// the draw of sweep `rs` (the run's numbering) from the residual, its pending layers written back first
int robust_draw(d3d_ctx *c, int64_t rs);

// ---- d3d_noise.hip: the variance factors of channel groups --------------------------------
// streams of the reduction of k_noise_sums: stream j adds the spaxels j, j + NOISE_STREAMS, ... in turn
constexpr int NOISE_STREAMS = 1024;
// the draw of sweep `rs` likewise (ev: four events recorded around the launches, or NULL -- option
// noise_timing of d3d_noise_step)
int noise_draw(d3d_ctx *c, int64_t rs, hipEvent_t *ev = nullptr);

// ---- d3d_pred.hip: pointwise predictive accuracy ------------------------------------------
// the chain state's residual (made valid, pending layers written back) as sample number
// c->post.n + 1 of the four accumulators
int pred_sample(d3d_ctx *c);

// ---- d3d_api.hip: what the work lists and their decisions are a function of (d3d_worklists.h); valid
// while the context's mask and part rectangles stay as they are
d3d_worklists::Input worklist_input(const d3d_ctx *c);
// The context is cut up as far as the SWEEP's kernels go (run_part, d3d_mh_layers): a tile, or more
// than one part.  Not d3d_worklists::partitioned_lists, which also counts a single given part
// rectangle: such a context gets no strips and maybe the wide form from the lists, and runs the
// unpartitioned kernels here.  Unifying the two would change which kernel it runs.
inline bool partitioned_sweep(const d3d_ctx *c) { return c->tiled || c->parts.size() > 1; }
// local colour residues of colour class `col` (a tile's origin shifts them)
inline void colour_residue(const d3d_ctx *c, int col, int *cy, int *cx) {
    d3d_worklists::local_residue(c->fh, c->fw, c->gy0, c->gx0, col, cy, cx);
}

// ---- d3d_mh.hip: the MH-within-Gibbs kernels ---------------------------------------------
void pend_clear(d3d_ctx *c);
int pend_free_buf(const d3d_ctx *c);
void pend_push(d3d_ctx *c, int cy, int cx, int g);
void fill_mh_args(d3d_ctx *c, d3d::MHArgs &P);
int launch_mh(d3d_ctx *c, const d3d::MHArgs &P, unsigned grid, uint32_t sweep);
// (total: the windows of the whole colour where the launch is one strip of it -- the kernel variant
// follows the colour, not the strip; 0: the launch is the colour.  strip: which strip of the colour row
// the launch is -- every strip keeps its blocks' wave sums in a region of its own)
int launch_mh_zb(d3d_ctx *c, d3d::MHArgs &P, unsigned n_items, uint32_t sweep, int layers, unsigned total = 0,
                 unsigned strip = 0);
// a colour launch of R chains together (MHArgs::batch; d3d_mh_sweeps_batch), grid = R x windows
int launch_mh_batch(d3d_ctx *c, const d3d::MHArgs &P, unsigned grid, uint32_t sweep, int layers);
// what differs between the chains of a joint launch; tables: with the chain's sweep tables
void fill_chain_args(const d3d_ctx *c, d3d::MHChainArgs &B, bool tables);
int launch_mh_defer(d3d_ctx *c, const d3d::MHArgs &P, unsigned grid, uint32_t sweep, int layers,
                    bool wide, unsigned total = 0);
int flush_pending(d3d_ctx *c);
// the proposals of sweep `sweep` for every owned spaxel (MHArgs::props), once per sweep
int ensure_proposals(d3d_ctx *c, uint32_t sweep);
// the proposal table and (lines) the line table, allocated on first use; the position tables
int ensure_tables(d3d_ctx *c, bool lines);
int ensure_ptab(d3d_ctx *c);
// proposals and line table of sweep `sweep` (k_mh_line_table): the context's, or those of the R
// chains of a batch in one launch
int launch_line_table(d3d_ctx *c, const d3d::MHArgs &P, uint32_t sweep, const d3d::MHChainArgs *chains, int R);
// k_mh_small can take this context's small parts (depth, tap count, options)
bool mh_small_usable(const d3d_ctx *c);
// row of the position tables for a launch of local colour residues (ly, lx) over the pending layer
int mh_ptab_row(const d3d_ctx *c, int ly, int lx, int layer = 0);
// the part's colour launches run k_mh_small (its small form, or -- option mh_small = 2 -- the chip-filling one)
bool mh_part_uses_tables(const d3d_ctx *c, const d3d_ctx::Part &pt);
// n_sweeps whole sweeps (Philox numbers sweep0 ..) of part pi in one launch (Part::chain)
#ifdef D3D_EXPERIMENTS
int launch_mh_chain(d3d_ctx *c, int pi, uint32_t sweep0, int n_sweeps);
#endif
int launch_apply_updates(d3d_ctx *c, const d3d::MHArgs &P, const double *rec, int n);
int launch_rtnorm(d3d_ctx *c, long n, double lo, double hi, double mu, double sigma, uint64_t seed,
                  int wave_mode, double *buf);
int launch_philox(d3d_ctx *c, long n, const uint32_t *counters, const uint32_t *keys, uint32_t *words,
                  double *pairs);
#ifdef D3D_EXPERIMENTS
int launch_mh_flow(d3d_ctx *c, uint32_t sweep);
int launch_mh_pair(d3d_ctx *c, int ka, uint32_t sweep);
#endif

// ---- d3d_temper.hip: replica exchange between tempered chains -----------------------------
// One round of a group on its leader's stream: the chains' energies, the decisions of the pairs of
// the round's parity, the exchange of the accepted pairs' residuals and parameters (three launches,
// nothing but device memory between them).  The caller has written the pending layers back.
int temper_round(d3d_temper *t, int64_t round);
// the context is a member of a live group (d3d_temper_create .. d3d_temper_destroy)
bool ctx_is_tempered(const d3d_ctx *c);

}  // namespace d3dh
