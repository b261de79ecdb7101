// The sweep driver of the MH-within-Gibbs chain: the colour loop of a part, what follows every
// sweep and the snapshot ring of a streamed chain -- once, for one context (d3d_mh_sweeps,
// d3d_mh_phase, d3d_mh_colour) and for R contexts that share every colour launch
// (d3d_mh_sweeps_batch).  gfx950 only.
#include "d3d_ctx.h"

using namespace d3dh;

namespace {

// ---- asynchronous chain streaming ------------------------------------------------
struct SnapQueue {
    int slot[d3d_ctx::STREAM_NB];  // chain slot each in-flight buffer belongs to
    int head = 0, count = 0;       // ring of in-flight buffers, oldest first
};

int snap_setup(d3d_ctx *c) {
    if (c->copy_stream) return 0;
    HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    const size_t bytes = (size_t)c->HW * 4 * sizeof(double);
    for (int b = 0; b < d3d_ctx::STREAM_NB; ++b) {
        HIP_TRY(c->snap_dev[b].alloc((size_t)c->HW * 4));
        HIP_TRY(hipHostMalloc((void **)&c->snap_host[b], bytes, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&c->snap_ready[b], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->snap_done[b], hipEventDisableTiming));
    }
    return 0;
}

// The oldest snapshot in flight: wait for its copy, hand it to the caller's arrays.
int snap_drain_one(d3d_ctx *c, SnapQueue &q, double *chain_out, double *dlog_out) {
    const int b = q.head;
    HIP_TRY(hipEventSynchronize(c->snap_done[b]));
    const size_t slot = (size_t)q.slot[b];
    if (chain_out)
        memcpy(chain_out + slot * c->HW * 3, c->snap_host[b], (size_t)c->HW * 3 * sizeof(double));
    if (dlog_out)
        memcpy(dlog_out + slot * c->HW, c->snap_host[b] + (size_t)c->HW * 3,
               (size_t)c->HW * sizeof(double));
    q.head = (q.head + 1) % d3d_ctx::STREAM_NB;
    --q.count;
    return 0;
}

// Snapshot the current parameters / log ratios for chain slot `slot`.
int snap_push(d3d_ctx *c, SnapQueue &q, int slot, double *chain_out, double *dlog_out) {
    if (q.count == d3d_ctx::STREAM_NB)
        if (int rc = snap_drain_one(c, q, chain_out, dlog_out)) return rc;
    const int b = (q.head + q.count) % d3d_ctx::STREAM_NB;
    HIP_TRY(hipMemcpyAsync(c->snap_dev[b], c->params, (size_t)c->HW * 3 * sizeof(double),
                           hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->snap_dev[b] + (size_t)c->HW * 3, c->dlog, (size_t)c->HW * sizeof(double),
                           hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->snap_ready[b], c->stream));
    HIP_TRY(hipStreamWaitEvent(c->copy_stream, c->snap_ready[b], 0));
    HIP_TRY(hipMemcpyAsync(c->snap_host[b], c->snap_dev[b], (size_t)c->HW * 4 * sizeof(double),
                           hipMemcpyDeviceToHost, c->copy_stream));
    HIP_TRY(hipEventRecord(c->snap_done[b], c->copy_stream));
    q.slot[b] = slot;
    ++q.count;
    return 0;
}

// ---- one colour launch ---------------------------------------------------------------
bool chain_ready(const d3d_ctx *c) { return c->have_taps && c->have_data && c->have_params && c->have_cfg; }

// What every call that advances the chain starts with: the device, a residual if none is valid,
// the accepted counter from zero where the call reports one, no proposal table from an earlier
// call (recomputed per call: the spaxels not yet updated get the same proposals).
int begin_sweeps(d3d_ctx *c, bool zero_accepted) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->err_valid)
        if (int rc = d3d_residual(c, nullptr)) return rc;
    if (zero_accepted) {
        HIP_TRY(hipMemsetAsync(c->accepted, 0, sizeof(unsigned long long), c->stream));
        HIP_TRY(hipMemsetAsync(c->acc_map, 0, (size_t)c->HW * sizeof(unsigned), c->stream));
    }
    c->props_sweep = -1;
    return 0;
}

// ordinal of colour `col` among the part's active ones: odd ones walk backwards (MHArgs::rev)
int active_ordinal(const d3d_ctx::Part &pt, int col) {
    int ord = 0;
    for (int k = 0; k < col; ++k) ord += pt.real[k] > 0;
    return ord;
}

// The arguments of the launch of colour `col`, the ka-th active one, of part `pt`.  layers: the
// pending layers its kernel keeps (0: it writes the residual itself; else the caller has set
// c->pend_part, fill_mh_args takes the domain from it).  tables: 0 none, 1 the sweep's
// proposals, 2 also the line table and the position tables k_mh_small reads.
void fill_colour_args(d3d_ctx *c, const d3d_ctx::Part &pt, int col, int ka, int layers, int tables,
                      d3d::MHArgs &P) {
    fill_mh_args(c, P);
    P.spx = c->spx + pt.off[col];
    P.rev = (c->mh_zigzag && (ka & 1)) ? 1 : 0;
    if (tables) P.props = c->props;
    if (tables > 1) {
        P.ltab = c->ltab;
        P.ptab = c->ptab;
        int ly, lx;
        colour_residue(c, col, &ly, &lx);
        for (int j = 0; j < 2; ++j) P.ptab_row[j] = mh_ptab_row(c, ly, lx, j);
    }
    // the launch that finds `layers` layers pending applies them for good
    if (layers) P.write_back = (c->lay_n >= layers) ? 1 : 0;
}

// The launch's updates, in G buffer g, are the newest pending layer (local residues) -- the
// only one after a launch that wrote the older ones back.
void push_colour_layer(d3d_ctx *c, int pi, int col, int g, bool wrote_back) {
    if (wrote_back) c->lay_n = 0;
    int cy, cx;
    colour_residue(c, col, &cy, &cx);
    pend_push(c, cy, cx, g);
    c->pend_part = pi;
}

// The real spaxels of colour `col` through the kernels that write the residual at once (k_mh): the
// head of the colour's list, or -- a part whose lists are strip-major -- the head of every strip's.
int launch_real(d3d_ctx *c, const d3d_ctx::Part &pt, int col, const d3d::MHArgs &P, uint32_t sweep) {
    if (pt.strips <= 1) return launch_mh(c, P, (unsigned)pt.real[col], sweep);
    for (int s = 0; s < pt.strips; ++s) {
        const int n = pt.sreal[(size_t)col * pt.strips + s];
        if (n <= 0) continue;
        d3d::MHArgs Ps = P;
        Ps.spx = P.spx + pt.soff[(size_t)col * (pt.strips + 1) + s];
        if (int rc = launch_mh(c, Ps, (unsigned)n, sweep)) return rc;
    }
    return 0;
}

// Lattice-row strips of a colour row (Part::strips, d3d_strips.h).  The launches of the colours
// (cy, 0 .. fw - 1) on a strip of lattice rows touch only that strip's bands of the residual, its
// spaxels and its slot rows of the G buffers, so the strips run on streams of their own, free of each
// other, between ONE fork before the row's first active colour and ONE join after its last:
// strip 0 on the context's stream, strip s on strip_stream[s - 1].  On every way out of run_part:
// joined, the context back on its stream.
//
// Chained (Part::order, option mh_strip_order): ONE fork per sweep and ONE join at its end; between
// them the strips of consecutive colour rows are ordered by the events of d3d_strip_order.h, and the
// colours write the G buffers its schedule names.
static_assert(d3d_ctx::GBUFS == d3d_strip_order::GSLOTS, "a G buffer behind every slot of the schedule");

// Test option mh_strip_lag: one wavefront that ends once the constant 100 MHz counter has advanced by
// 100 us -- or after 40 sleeps of some 3 us, whichever comes first.  It reads and writes no memory.
__global__ __launch_bounds__(64) void k_strip_lag() {
    const uint64_t t0 = wall_clock64();
    for (int i = 0; i < 40 && wall_clock64() - t0 < 10000; ++i) __builtin_amdgcn_s_sleep(127);
}

struct StripScope {
    d3d_ctx *c;
    hipStream_t main;
    int S = 1, row = -1;  // strips in flight (1: none), their colour row
    unsigned locked = 0;  // G buffers of the layers of other colour rows that were pending at the fork
    int setup() {
        if (c->strip_fork) return 0;
        // (G buffers beyond the four of whole launches: up to three locked, three pending, one to write)
        for (int b = 4; b < d3d_ctx::GBUFS; ++b) {
            HIP_TRY(c->gbuf[b].alloc((size_t)c->slots * c->Dp));
            HIP_TRY(hipMemsetAsync(c->gbuf[b], 0, (size_t)c->slots * c->Dp * sizeof(double), main));
        }
        HIP_TRY(hipEventCreateWithFlags(&c->strip_fork, hipEventDisableTiming));
        for (int a = 0; a < d3d_ctx::STRIP_AUX; ++a) {
            HIP_TRY(hipStreamCreateWithFlags(&c->strip_stream[a], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&c->strip_join[a], hipEventDisableTiming));
        }
        return 0;
    }
    // a G buffer that holds no pending layer and is not locked
    int free_buf() const {
        for (int b = 0; b < d3d_ctx::GBUFS; ++b) {
            bool used = (locked >> b) & 1;
            for (int j = 0; j < c->lay_n; ++j) used = used || c->lay_g[j] == b;
            if (!used) return b;
        }
        return 0;  // unreachable: at most 3 locked and 3 pending of GBUFS = 8
    }
    int fork(int strips, int colour_row, unsigned locked_bufs) {
        if (int rc = setup()) return rc;
        locked = locked_bufs;
        HIP_TRY(hipEventRecord(c->strip_fork, main));
        for (int a = 0; a + 1 < strips; ++a) HIP_TRY(hipStreamWaitEvent(c->strip_stream[a], c->strip_fork, 0));
        S = strips;
        row = colour_row;
        return 0;
    }
    // ---- the chained order (d3d_strip_order.h): the schedule's steps, nothing else ----
    const d3d_strip_order::Schedule *sched = nullptr;  // the sweep's schedule once its first step has run
    int pool0 = 0;                                     // pool of the sweep's first active row
    hipStream_t stream_of(int s) const { return s ? c->strip_stream[s - 1] : main; }
    int record(unsigned mask, int s) {
        for (int e = 0; e < d3d_strip_order::NEV; ++e)
            if ((mask >> e) & 1) HIP_TRY(hipEventRecord(c->strip_ev[e], stream_of(s)));
        return 0;
    }
    int wait(unsigned mask, int s) {
        for (int e = 0; e < d3d_strip_order::NEV; ++e)
            if ((mask >> e) & 1) HIP_TRY(hipStreamWaitEvent(stream_of(s), c->strip_ev[e], 0));
        return 0;
    }
    // Before the launches of step k: its records, its waits.  The first step of a sweep also sees to the G
    // buffers: every layer pending from before must lie in the pool this sweep's first row does NOT write
    // (its last reader in another strip runs in that row).  Layers the chained sweep before left do; others
    // (whole launches, joined strips) get the slots of that pool, the free buffers the rest.
    int enter(const d3d_strip_order::Schedule &sd, int k) {
        namespace so = d3d_strip_order;
        const so::Step &st = sd.steps[(size_t)k];
        if (k == 0) {
            if (int rc = setup()) return rc;
            for (int e = 0; e < so::NEV; ++e)
                if (!c->strip_ev[e]) HIP_TRY(hipEventCreateWithFlags(&c->strip_ev[e], hipEventDisableTiming));
            pool0 = c->strip_pool & 1;
            const int other = (1 - pool0) * (sd.M + 1);
            bool placed = true;
            for (int j = 0; j < c->lay_n; ++j) {
                bool in = false;
                for (int q = 0; q <= sd.M; ++q) in = in || c->strip_gbuf[other + q] == c->lay_g[j];
                placed = placed && in;
            }
            if (!placed) {
                int order[d3d_ctx::GBUFS], n = 0;
                for (int j = 0; j < c->lay_n; ++j) order[n++] = c->lay_g[j];
                for (int b = 0; b < d3d_ctx::GBUFS; ++b) {
                    bool pending = false;
                    for (int j = 0; j < c->lay_n; ++j) pending = pending || c->lay_g[j] == b;
                    if (!pending) order[n++] = b;
                }
                n = 0;
                for (int q = 0; q <= sd.M; ++q) c->strip_gbuf[other + q] = order[n++];
                for (int q = 0; q <= sd.M; ++q) c->strip_gbuf[pool0 * (sd.M + 1) + q] = order[n++];
                for (int q = 2 * (sd.M + 1); q < so::GSLOTS; ++q) c->strip_gbuf[q] = order[n++];  // (stays a permutation)
            }
            c->strip_pool = so::pool_after(sd, pool0);
            S = sd.S;
            sched = &sd;
        }
        for (int s = 0; s < sd.S; ++s)
            if (int rc = record(st.pre[s], s)) return rc;
        for (int s = 0; s < sd.S; ++s)
            if (int rc = wait(st.wait[s], s)) return rc;
        // test option mh_strip_lag: one strip late at every colour row -- the chain must not notice
        if (st.first_of_row && c->mh_strip_lag >= 1 && c->mh_strip_lag <= sd.S) {
            hipLaunchKernelGGL(k_strip_lag, dim3(1), dim3(64), 0, stream_of(c->mh_strip_lag - 1));
            HIP_TRY(hipGetLastError());
        }
        return 0;
    }
    int buf_of(int k) const { return c->strip_gbuf[d3d_strip_order::gslot(*sched, sched->steps[(size_t)k], pool0)]; }
    int leave(int k) {
        for (int s = 0; s < sched->S; ++s)
            if (int rc = record(sched->steps[(size_t)k].post[s], s)) return rc;
        return 0;
    }
    int join() {
        c->stream = main;
        if (sched) {  // the sweep-end join of the schedule
            const d3d_strip_order::Schedule &sd = *sched;
            sched = nullptr;
            S = 1;
            for (int s = 0; s < sd.S; ++s)
                if (int rc = record(sd.tail_post[s], s)) return rc;
            for (int s = 0; s < sd.S; ++s)
                if (int rc = wait(sd.tail_wait[s], s)) return rc;
            return 0;
        }
        const int n = S;
        S = 1;
        row = -1;
        locked = 0;
        for (int a = 0; a + 1 < n; ++a) {
            HIP_TRY(hipEventRecord(c->strip_join[a], c->strip_stream[a]));
            HIP_TRY(hipStreamWaitEvent(main, c->strip_join[a], 0));
        }
        return 0;
    }
    ~StripScope() { (void)join(); }
};

// d3d_mh_sweeps_batch: R contexts of one geometry share every colour launch.  The leader -- the
// context run_part is called on -- carries what they share: work lists, taps, pending layers.
struct Batch {
    d3d_ctx **cs;
    int R, layers;  // pending layers of the joint launches
    bool small;     // a joint launch does not fill the chip: k_mh_small with the chains' sweep tables
    const d3d::MHChainArgs *dev;
};

// Every colour class of one part, for one sweep (lib/run.py:367-519 restricted to
// the part, in colour order).
// strips: the colour rows may run in the part's lattice-row strips (d3d_mh_sweeps; stepping by phase
// keeps whole colour launches).
int run_part(d3d_ctx *c, int pi, uint32_t sweep, const Batch *b = nullptr, bool strips_allowed = false) {
    d3d_ctx::Part &pt = c->parts[pi];
    const int ncol = c->fh * c->fw;
    const int layers = b ? b->layers : pt.layers;
    d3d_ctx *const self[1] = {c};
    d3d_ctx *const *cs = b ? b->cs : self;
    // deferred write-back with pending layers: the wave-specialised kernel (D <= 256);
    // an unpartitioned context may also use the plain deferred kernel
    const bool partitioned = partitioned_sweep(c);
    const bool deferred =
        c->mh_defer &&
        (!partitioned || (c->mh_defer == 1 && (c->Dp <= d3d::MH_WS_MAX_DP || c->mh_zb)));
    // (more layers pending than this part's kernels take: a batched launch that filled the chip
    // left two, the context alone keeps one)
    if (c->lay_n && (c->pend_part != pi || !deferred || c->lay_n > layers))
        if (int rc = flush_pending(c)) return rc;
#ifdef D3D_EXPERIMENTS
    if (deferred && pt.chain && !b) return launch_mh_chain(c, pi, sweep, 1);  // all colours in one launch
#endif
    // two colour classes per launch (k_mh_pair) where the N/W alternation of two pending
    // layers allows it: an unpartitioned context, a launch that fills the chip
    const bool pairs = !b && deferred && c->mh_pair && !partitioned && c->mh_defer == 1 && c->Dp <= 256 &&
                       pt.layers == 2 && c->flow_K > 1 && !c->flow_first.empty();
    // small colour launches: the sweep's proposals come from one launch before them
    // (and the z-blocked kernels: every block's prepare wavefront and k_mh_zdecide need it;
    // and every part that runs k_mh_small, which also reads the sweep's line table, built with
    // the proposals).  The chains of a batch made theirs in one launch before the sweep.
    const bool small = deferred && c->mh_defer == 1 && !c->mh_zb && d3dh::mh_part_uses_tables(c, pt);
    const int tables = b ? (b->small ? 2 : 0)
                         : (c->mh_props && deferred && (c->mh_zb || (pt.layers == 1 && !c->deep) || small))
                               ? (small ? 2 : 1) : 0;
    // lattice-row strips: this context alone, the wave-specialised deferred kernels
    bool strips_ok = strips_allowed && !b && pt.strips > 1 && deferred && !partitioned && c->mh_defer == 1 && tables < 2 &&
                     (c->mh_zb || c->Dp <= d3d::MH_WS_MAX_DP);
#ifdef D3D_EXPERIMENTS
    strips_ok = strips_ok && !c->stampbuf && !pairs;  // (phase stamps are per colour launch)
#endif
    StripScope strips = {c, c->stream};
    int ord = 0;  // ordinal of `col` among the active colours
    for (int col = 0; col < ncol; ++col) {
        const int n_real = pt.real[col];
        if (n_real <= 0) continue;
        const int ka = ord++;
        if (deferred) c->pend_part = pi;  // fill_mh_args takes the domain from it
#ifdef D3D_EXPERIMENTS
        if (pairs && c->lay_n == 1 && ka + 1 < c->flow_K) {
            if (c->stampbuf) goto single;  // phase stamps are per colour launch
            int rc = launch_mh_pair(c, ka, sweep);
            if (rc) return rc;
            // skip colour B in this loop
            ++col;
            while (col < ncol && pt.real[col] <= 0) ++col;
            ++ord;
            continue;
        }
    single:
#else
        (void)pairs;
#endif
        if (tables && !b)
            if (int rc = ensure_proposals(c, sweep)) return rc;
        d3d::MHArgs P;
        fill_colour_args(c, pt, col, ka, deferred ? layers : 0, tables, P);
        if (!deferred) {
            if (int rc = launch_real(c, pt, col, P, sweep)) return rc;
            continue;
        }
        // real + virtual positions: the windows of this launch tile the domain
        const int n_all = pt.off[col + 1] - pt.off[col];
        // the colour's arguments once; every strip its range of the list on its stream.  The kernel
        // variant follows the colour's windows, not the strip's; a strip of virtual positions
        // alone still launches (a storing launch needs their write-back).
        auto launch_strips = [&](int g_cur) {
            P.Gcur = c->gbuf[g_cur];
            const int *so = &pt.soff[(size_t)col * (pt.strips + 1)];
            for (int s = 0; s < pt.strips; ++s) {
                const int n = so[s + 1] - so[s];
                if (n <= 0) continue;
                d3d::MHArgs Ps = P;
                Ps.spx = P.spx + so[s];
                c->stream = s ? c->strip_stream[s - 1] : strips.main;
                const int rc = c->mh_zb ? launch_mh_zb(c, Ps, (unsigned)n, sweep, layers, (unsigned)n_all, (unsigned)s)
                                        : launch_mh_defer(c, Ps, (unsigned)n, sweep, layers, pt.wide, (unsigned)n_all);
                c->stream = strips.main;
                if (rc) return rc;
            }
            push_colour_layer(c, pi, col, g_cur, P.write_back);
            return 0;
        };
        if (strips_ok && pt.order.S > 1) {  // chained: the schedule's step of this colour
            NEED(pt.order.S == pt.strips && pt.order.M == layers && ka < (int)pt.order.steps.size() &&
                     pt.order.steps[(size_t)ka].col == col,
                 D3D_ERR_STATE, "internal: the strips' schedule does not describe colour %d", col);
            if (int rc = strips.enter(pt.order, ka)) return rc;
            if (int rc = launch_strips(strips.buf_of(ka))) return rc;
            if (int rc = strips.leave(ka)) return rc;
            continue;
        }
        if (strips.S > 1 && col / c->fw != strips.row)  // the next colour row: its bands lie one cube row lower
            if (int rc = strips.join()) return rc;
        // The strips part ways at the row's first active colour.  A layer still pending from the row
        // before lies one cube row higher: the G rows it has under a window come from the neighbouring
        // strip too.  They were written before the join, and the buffers that hold such layers take no
        // launch's updates for the rest of this row, so a strip that runs ahead never writes what a
        // strip behind it still reads.
        if (strips_ok && strips.S == 1) {
            int cy, cx;
            colour_residue(c, col, &cy, &cx);
            unsigned locked = 0;
            for (int j = 0; j < c->lay_n; ++j)
                if (c->lay_cy[j] != cy) locked |= 1u << c->lay_g[j];
            if (int rc = strips.fork(pt.strips, col / c->fw, locked)) return rc;
        }
        if (strips.S > 1) {
            if (int rc = launch_strips(strips.free_buf())) return rc;
            continue;
        }
#ifdef D3D_EXPERIMENTS
        if (!b && c->stampbuf && c->stamp_next < c->stamp_launches && (size_t)n_all * 8 <= c->stamp_stride)
            P.stamp = c->stampbuf + (c->stamp_next++) * c->stamp_stride;
#endif
        const int g_cur = pend_free_buf(c);
        int rc;
        if (b) {  // grid = chains x windows; the G buffers by index: all chains rotate theirs alike
            P.batch = b->dev;
            P.b_items = n_all;
            P.b_gcur = g_cur;
            for (int j = 0; j < 3; ++j) P.b_lay_g[j] = j < c->lay_n ? c->lay_g[j] : 0;
            rc = launch_mh_batch(c, P, (unsigned)n_all * b->R, sweep, layers);
        } else {
            rc = c->mh_zb ? launch_mh_zb(c, P, (unsigned)n_all, sweep, layers)
                          : launch_mh_defer(c, P, (unsigned)n_all, sweep, layers, pt.wide);
        }
        if (rc) return rc;
        for (int r = 0; r < (b ? b->R : 1); ++r) push_colour_layer(cs[r], pi, col, g_cur, P.write_back);
    }
    return strips.join();
}

int run_phase(d3d_ctx *c, int phase, uint32_t sweep, bool strips_allowed = false) {
    for (size_t pi = 0; pi < c->parts.size(); ++pi)
        if (c->parts[pi].phase == phase)
            if (int rc = run_part(c, (int)pi, sweep, nullptr, strips_allowed)) return rc;
    return 0;
}

// What follows sweep `s` (the caller's numbering) of a context, in this order.
int end_sweep(d3d_ctx *c, int s, int keep_one_in, SnapQueue &snaps, double *chain_out, double *dlog_out) {
    // lib/run.py:353, 430-432, 449-451 -- streamed: the compute stream only pays for a
    // device-to-device snapshot
    if (s % keep_one_in == 0 && (chain_out || dlog_out))
        if (int rc = snap_push(c, snaps, s / keep_one_in, chain_out, dlog_out)) return rc;
    if (post_due(c, s))  // d3d_post_schedule: this sweep's state into the running moments
        if (int rc = post_sample(c)) return rc;
    // d3d_adapt_begin: the sweep that fills a window moves the jump scales
    if (int rc = adapt_after_sweep(c, s)) return rc;
    // lib/run.py:521-534: squash the error creep with a fresh residual.  A tile
    // first gathers the parameters of the spaxels of its frame from their owners.
    if (c->refresh_every > 0 && s % c->refresh_every == 0) {
        if (plan_has_entries(c, D3D_PLAN_PARAMS)) {
            NEED(c->comm, D3D_ERR_STATE, "parameter gather needs d3d_comm_init");
            if (int rc = halo_exchange(c, D3D_PLAN_PARAMS)) return rc;
        }
        if (int rc = forward_into(c, c->slot[D3D_SLOT_ERR], true)) return rc;
    }
    // d3d_robust_begin / d3d_noise_begin: the weights of a Student-t likelihood, or the variance factors
    // of the channel groups, redrawn from the refreshed residual
    return rescale_after_sweep(c, s);
}

// option halo_timing: the oldest event pair in flight, reduced into halo_ms / halo_count
int halo_drain_one(d3d_ctx *c) {
    const size_t at = c->halo_ev_head;
    float f = 0.f;
    HIP_TRY(hipEventSynchronize(c->halo_ev[2 * at + 1]));
    HIP_TRY(hipEventElapsedTime(&f, c->halo_ev[2 * at], c->halo_ev[2 * at + 1]));
    c->halo_ms += (double)f;
    ++c->halo_count;
    c->halo_ev_head = (at + 1) % d3d_ctx::HALO_RING;
    --c->halo_ev_used;
    return 0;
}

// For the duration of a d3d_mh_sweeps_batch call every chain runs on the leader's stream.  On
// every way out: that stream drained (the chains' device arguments, declared before the scope, go
// after it), each context back on its own stream.
struct BatchScope {
    d3d_ctx **cs;
    std::vector<hipStream_t> own;  // of the contexts switched so far
    ~BatchScope() {
        (void)hipStreamSynchronize(cs[0]->stream);
        for (size_t r = 0; r < own.size(); ++r) cs[r]->stream = own[r];
    }
};

}  // namespace

extern "C" {

int d3d_mh_sweeps(d3d_ctx *c, int n_sweeps, int first_sweep, int keep_one_in, double *chain_out,
                  double *dlog_out, int64_t *accepted) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(chain_ready(c), D3D_ERR_STATE, "taps/data/parameters/mh_config not set");
    NEED(n_sweeps >= 0 && first_sweep >= 0, D3D_ERR_INVALID, "negative sweep count/index");
    NEED(keep_one_in > 0, D3D_ERR_INVALID, "keep_one_in= MUST be a positive integer");
    // a tile whose neighbours' updates reach it needs the halo exchange between the phases
    // phases of a sweep: this tile's own, and those after which a neighbour sends to it
    bool any_plan = false;
    int n_phases = c->n_phases;
    for (int ph = 0; ph < D3D_PLAN_PARAMS; ++ph)
        if (plan_has_entries(c, ph)) {
            any_plan = true;
            n_phases = std::max(n_phases, ph + 1);
        }
    NEED(!any_plan || c->comm, D3D_ERR_STATE,
         "this tile has halo plans: call d3d_comm_init, or drive the phases with d3d_mh_phase "
         "and exchange the halos yourself");
    if (int rc = begin_sweeps(c, true)) return rc;
    c->halo_ev_used = 0;  // (pairs a failed call left behind are dropped)
    c->halo_ev_head = 0;
    SnapQueue snaps;
    if (chain_out || dlog_out)
        if (int rc = snap_setup(c)) return rc;
    // k_mh_flow addresses SLOT_ERR through a raw buffer (32-bit byte offsets)
    const bool flow = c->mh_flow && c->mh_defer == 1 && !c->tiled && c->parts.size() == 1 &&
                      c->Dp <= 256 && c->flow_K > 0 &&
                      c->cube_elems * sizeof(double) < (size_t(1) << 31);
    // One part, no halo plans, the chain form: several sweeps per launch -- up to the next
    // sweep that is saved or followed by a from-scratch residual.
#ifdef D3D_EXPERIMENTS
    const bool chain_batches = !flow && !any_plan && c->parts.size() == 1 && c->parts[0].chain &&
                               c->mh_defer == 1 && n_phases == 1;
#endif
    for (int s = first_sweep; s < first_sweep + n_sweeps; ++s) {
        const uint32_t rs = (uint32_t)s + c->sweep_origin;
#ifdef D3D_EXPERIMENTS
        if (chain_batches) {
            int last = first_sweep + n_sweeps - 1;  // last sweep of this launch
            for (int t = s; t <= last; ++t) {
                const bool saved = t % keep_one_in == 0 && (chain_out || dlog_out);
                const bool refresh = c->refresh_every > 0 && t % c->refresh_every == 0;
                if (saved || refresh || post_due(c, t) || rescale_due(c, t)) {
                    last = t;
                    break;
                }
            }
            if (c->lay_n && c->pend_part != 0)
                if (int rc = flush_pending(c)) return rc;
            if (int rc = launch_mh_chain(c, 0, rs, last - s + 1)) return rc;
            s = last;
        } else if (flow) {
            c->pend_part = 0;
            int rc = launch_mh_flow(c, rs);
            if (rc) return rc;
            c->pend_part = 0;
        } else
#endif
        {
            for (int ph = 0; ph < n_phases; ++ph) {
                int rc = run_phase(c, ph, rs, true);
                if (rc) return rc;
                if (plan_has_entries(c, ph)) {
                    hipEvent_t ev[2] = {nullptr, nullptr};
                    if (c->halo_timing) {
                        // a bounded ring of event pairs: a long call (50 000 sweeps x 2-4
                        // phases) reduces the oldest pair when the ring is full
                        if (c->halo_ev_used == d3d_ctx::HALO_RING)
                            if (int rc2 = halo_drain_one(c)) return rc2;
                        const size_t at = (c->halo_ev_head + c->halo_ev_used) % d3d_ctx::HALO_RING;
                        while (c->halo_ev.size() < 2 * (at + 1)) {
                            hipEvent_t e;
                            HIP_TRY(hipEventCreate(&e));
                            c->halo_ev.push_back(e);
                        }
                        ev[0] = c->halo_ev[2 * at];
                        ev[1] = c->halo_ev[2 * at + 1];
                        ++c->halo_ev_used;
                        HIP_TRY(hipEventRecord(ev[0], c->stream));
                    }
                    rc = halo_exchange(c, ph);
                    if (rc) return rc;
                    if (ev[1]) HIP_TRY(hipEventRecord(ev[1], c->stream));
                }
            }
        }
        if (int rc = end_sweep(c, s, keep_one_in, snaps, chain_out, dlog_out)) return rc;
    }
    unsigned long long acc = 0;
    unsigned flow_err = 0;
    if (int rc = accepted_collect(c)) return rc;
    HIP_TRY(hipMemcpyAsync(&acc, c->accepted, sizeof acc, hipMemcpyDeviceToHost, c->stream));
    if (flow || c->mh_pair || c->chain_used)  // (these kernels raise *flow_err when a flag wait times out)
        HIP_TRY(hipMemcpyAsync(&flow_err, c->flow_err, sizeof flow_err, hipMemcpyDeviceToHost,
                               c->stream));
    while (snaps.count > 0)
        if (int rc = snap_drain_one(c, snaps, chain_out, dlog_out)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    while (c->halo_ev_used > 0)  // option halo_timing
        if (int rc = halo_drain_one(c)) return rc;
    if (accepted) *accepted = (int64_t)acc;
    c->chain_used = false;
    NEED(!flow_err, D3D_ERR_HIP,
         "a dependency wait inside a sweep kernel timed out (k_mh_chain needs all its workgroups "
         "resident: is another process using this GPU?  option mh_chain = 0 avoids it); the "
         "chain state is invalid");
    return D3D_OK;
}

int d3d_mh_sweeps_batch(d3d_ctx **ctxs, int n_ctx, int n_sweeps, int first_sweep, int keep_one_in,
                        double **chain_out, double **dlog_out, int64_t *accepted) {
    NEED(ctxs && n_ctx >= 1, D3D_ERR_INVALID, "no contexts");
    NEED(n_sweeps >= 0 && first_sweep >= 0, D3D_ERR_INVALID, "negative sweep count/index");
    NEED(keep_one_in > 0, D3D_ERR_INVALID, "keep_one_in= MUST be a positive integer");
    d3d_ctx *L = ctxs[0];  // the leader: its stream, its work lists
    for (int r = 0; r < n_ctx; ++r) {
        d3d_ctx *c = ctxs[r];
        NEED(c, D3D_ERR_INVALID, "ctx %d is NULL", r);
        for (int q = 0; q < r; ++q) NEED(ctxs[q] != c, D3D_ERR_INVALID, "ctx %d appears twice", r);
        NEED(chain_ready(c), D3D_ERR_STATE, "ctx %d: taps/data/parameters/mh_config not set", r);
        NEED(!c->tiled && c->parts.size() == 1 && !c->comm, D3D_ERR_UNSUPPORTED,
             "ctx %d is tiled or partitioned: batched chains are whole cubes", r);
        NEED(c->mh_defer == 1 && c->Dp <= 256 && !c->deep, D3D_ERR_UNSUPPORTED,
             "ctx %d: batched chains take cubes up to 256 channels with the default write-back scheme", r);
        const char *const differs = setup_differs(c, L);
        NEED(!differs, D3D_ERR_INVALID, "ctx %d: another %s than ctx 0 (the chains share the work lists, the taps and "
             "the launch's arguments)", r, differs);
        NEED((c->ivar_is_uniform && c->uniform_fast_path) == (L->ivar_is_uniform && L->uniform_fast_path),
             D3D_ERR_INVALID, "ctx %d: uniform and per-voxel variances cannot share a launch", r);
        NEED(c->mh_zigzag == L->mh_zigzag && c->sweep_origin == L->sweep_origin, D3D_ERR_INVALID,
             "ctx %d: another walk order or sweep origin than ctx 0", r);
        // (the chains share the leader's pending-layer state, and a from-scratch residual
        // clears a chain's own: they must all be rebuilt at the same sweeps)
        NEED(c->prior.on == L->prior.on, D3D_ERR_INVALID,
             "ctx %d: the smoothness prior (d3d_prior_begin) is %s, on ctx 0 it is %s (the chains share the "
             "launch's kernel; their weights may differ)", r, c->prior.on ? "on" : "off", L->prior.on ? "on" : "off");
        NEED(c->refresh_every == L->refresh_every, D3D_ERR_INVALID,
             "ctx %d: refresh_every %d differs from ctx 0's %d (batched chains rebuild their residuals together)",
             r, c->refresh_every, L->refresh_every);
        // (and written back at the same sweeps: d3d_robust_begin's draws flush the pending layers)
        const d3d_ctx::Rescale &mine = c->rescale, &lead = L->rescale;
        const RescaleName held = rescale_name(mine.who ? c : L);
        NEED(mine.who == lead.who && (!mine.who || (mine.every == lead.every && mine.start == lead.start)), D3D_ERR_INVALID,
             "ctx %d: %s (d3d_%s_begin) armed, every or start differ from ctx 0's (batched chains write their pending "
             "residual updates back together)", r, held.what, held.api);
    }
    HIP_TRY(hipSetDevice(L->device));
    // saved sweeps (lib/run.py:353, 430-432, 449-451): every chain streams its samples as
    // d3d_mh_sweeps does -- device snapshot on the common stream, copy stream, pinned ring
    std::vector<SnapQueue> snaps(n_ctx);
    if (chain_out || dlog_out)
        for (int r = 0; r < n_ctx; ++r)
            if (int rc = snap_setup(ctxs[r])) return rc;
    auto co = [&](int r) { return chain_out ? chain_out[r] : nullptr; };
    auto lo = [&](int r) { return dlog_out ? dlog_out[r] : nullptr; };
    const d3d_ctx::Part &pt = L->parts[0];
    int most = 0;
    for (int col = 0; col < L->fh * L->fw; ++col) most = std::max(most, pt.off[col + 1] - pt.off[col]);
    // two pending layers where the launch of all chains together fills the chip
    Batch b = {ctxs, n_ctx, (L->Dp <= 160 && (long)most * n_ctx >= L->flow_grid / 2) ? 2 : 1, false, nullptr};
    b.small = b.layers == 1;
    for (int r = 0; r < n_ctx; ++r) {
        ctxs[r]->batch_layers = b.layers;  // (read-only option batch_layers)
        b.small = b.small && mh_small_usable(ctxs[r]);
    }
    DevBuf<d3d::MHChainArgs> dev;
    BatchScope scope = {ctxs};
    for (int r = 0; r < n_ctx; ++r) {
        HIP_TRY(hipStreamSynchronize(ctxs[r]->stream));
        scope.own.push_back(ctxs[r]->stream);
        ctxs[r]->stream = L->stream;
    }
    std::vector<d3d::MHChainArgs> host(n_ctx);
    for (int r = 0; r < n_ctx; ++r) {
        d3d_ctx *c = ctxs[r];
        if (int rc = begin_sweeps(c, true)) return rc;
        if (int rc = flush_pending(c)) return rc;
        if (b.small)
            if (int rc = ensure_tables(c, true)) return rc;
        fill_chain_args(c, host[r], b.small);
    }
    if (b.small)
        if (int rc = ensure_ptab(L)) return rc;
    HIP_TRY(dev.alloc((size_t)n_ctx));
    HIP_TRY(hipMemcpy(dev, host.data(), n_ctx * sizeof(d3d::MHChainArgs), hipMemcpyHostToDevice));
    b.dev = dev;
    for (int s = first_sweep; s < first_sweep + n_sweeps; ++s) {
        const uint32_t rs = (uint32_t)s + L->sweep_origin;
        if (b.small) {  // every chain's proposals and lines of this sweep, one launch
            d3d::MHArgs T;
            fill_mh_args(L, T);
            if (int rc = launch_line_table(L, T, rs, b.dev, n_ctx)) return rc;
        }
        if (int rc = run_part(L, 0, rs, &b)) return rc;
        // d3d_pred_begin: a predictive sample writes its chain's pending layers back, and the chains
        // share the leader's pending-layer state: where one chain samples (tempering: rung 0), all
        // write theirs back
        bool pred_flush = false;
        for (int r = 0; r < n_ctx; ++r) pred_flush = pred_flush || (ctxs[r]->pred.on && post_due(ctxs[r], s));
        if (pred_flush)
            for (int r = 0; r < n_ctx; ++r)
                if (int rc = flush_pending(ctxs[r])) return rc;
        // chain after chain, where d3d_mh_sweeps' loop runs one: the chains share a stream and
        // touch disjoint buffers, so the order across chains does not change any of them
        for (int r = 0; r < n_ctx; ++r)
            if (int rc = end_sweep(ctxs[r], s, keep_one_in, snaps[r], co(r), lo(r))) return rc;
    }
    for (int r = 0; r < n_ctx; ++r)
        while (snaps[r].count > 0)
            if (int rc = snap_drain_one(ctxs[r], snaps[r], co(r), lo(r))) return rc;
    std::vector<unsigned long long> acc(n_ctx, 0);
    for (int r = 0; r < n_ctx; ++r) {
        if (int rc = accepted_collect(ctxs[r])) return rc;  // (on the common stream: BatchScope)
        HIP_TRY(hipMemcpyAsync(&acc[r], ctxs[r]->accepted, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               L->stream));
    }
    HIP_TRY(hipStreamSynchronize(L->stream));
    if (accepted)
        for (int r = 0; r < n_ctx; ++r) accepted[r] = (int64_t)acc[r];
    return D3D_OK;
}

int d3d_mh_phase(d3d_ctx *c, int phase, int sweep) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(chain_ready(c), D3D_ERR_STATE, "taps/data/parameters/mh_config not set");
    // (a tile may have no part in a phase its neighbours have: then there is nothing to do)
    NEED(phase >= 0 && phase < D3D_PLAN_PARAMS && sweep >= 0, D3D_ERR_INVALID,
         "phase %d / sweep %d out of range", phase, sweep);
    if (int rc = begin_sweeps(c, false)) return rc;
    return run_phase(c, phase, (uint32_t)sweep + c->sweep_origin);
}

int d3d_mh_colour(d3d_ctx *c, int colour, int sweep) {
    NEED(c, D3D_ERR_INVALID, "ctx is NULL");
    NEED(chain_ready(c), D3D_ERR_STATE, "taps/data/parameters/mh_config not set");
    NEED(colour >= 0 && colour < c->fh * c->fw && sweep >= 0, D3D_ERR_INVALID,
         "colour %d / sweep %d out of range", colour, sweep);
    if (int rc = begin_sweeps(c, false)) return rc;
    if (int rc = flush_pending(c)) return rc;
    for (const d3d_ctx::Part &pt : c->parts) {
        const int n_real = pt.real[colour];
        if (n_real <= 0) continue;
        d3d::MHArgs P;
        fill_colour_args(c, pt, colour, active_ordinal(pt, colour), 0, 0, P);
        int rc = launch_real(c, pt, colour, P, (uint32_t)sweep + c->sweep_origin);
        if (rc) return rc;
    }
    return D3D_OK;
}

}  // extern "C"
