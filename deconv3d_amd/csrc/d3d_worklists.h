// The work lists of the MH sweep: the parts of a context, the list of every
// (part, colour class) -- real spaxels, then the virtual lattice positions that make a launch's
// windows tile the part's domain -- and what every part's colour launches run as: pending layers,
// the wide and the small form, lattice-row strips and their order.  A pure function of an Input.
// Host-only, no HIP: tests/test_worklists_cpu.py compiles it alone (tests/worklists_dump.cpp) and
// compares every list and decision with a restatement of the rules; d3d_api.hip fills the Input
// from a context, uploads the lists and decides nothing.
//
// Colour classes are GLOBAL: (cy, cx) = ((y + gy0) mod fh, (x + gx0) mod fw), colour cy * fw + cx.
#pragma once

#include <algorithm>
#include <vector>

#include "d3d_strip_order.h"
#include "d3d_strips.h"

namespace d3d_worklists {

// Lattice-row strips an unpartitioned context's chip-filling colour rows run in when option mh_strips
// is 0 (1: none).  What profiles/sweep_strips_ab.txt justifies: two pass the project's rule, three gain
// less, four lose.
constexpr int MH_STRIPS_AUTO = 2;
// How the strips of consecutive colour rows are ordered when option mh_strip_order is 0: 1 joined after
// every colour row, 2 chained row to row by events with one join per sweep (d3d_strip_order.h).  What
// profiles/sweep_chained_ab.txt justifies: chained passes the project's rule with two strips and with
// three (which the z-blocked form loses with: the automatic count stays two), the joined form with none.
constexpr int MH_STRIP_ORDER_AUTO = 2;

struct Entry {  // one window of a launch: 16 bytes, the device reads it as an int4
    int y, x;   // its centre (local; a virtual one may lie up to one period outside the cube)
    int real;   // 1: a spaxel the launch decides; 0: virtual -- write-back only
    int pad;
};

struct Rect {
    int y0, y1, x0, x1;
};

// A PART is a rectangle of spaxels updated together: sweep = for every phase, for
// every part of the phase, for every colour class, one launch (lib/run.py:553-560
// declares the scan order overridable).  An unpartitioned context has one part,
// the whole cube (a tile: its owned rectangle).  The DOMAIN of a part is the set
// of cells its windows touch.
struct Part {
    int y0 = 0, y1 = 0, x0 = 0, x1 = 0;      // spaxels (local)
    int dy0 = 0, dy1 = 0, dx0 = 0, dx1 = 0;  // domain (local)
    int phase = 0;
    int layers = 1;                          // pending layers in use
    bool wide = false;                       // its colour launches take the wide form (MH_WIDE_NS)
    bool small = false;                      // its colour launches do not fill the chip: k_mh_small
    // k_mh_chain (whole sweeps of the part in one launch): slot grid, or chain = false
    // (EXPERIMENTS builds: filled by d3d_api.hip)
    bool chain = false;
    int chain_ns = 0, chain_sx0 = 0, n_sy = 0, n_sx = 0;
    int K = 0;                               // its active colours (those with a real spaxel)
    int last_col = -1;                       // the last of them
    std::vector<int> off;                    // fh*fw + 1: start of each colour's list
    std::vector<int> real;                   // fh*fw: real spaxels of each colour
    // Lattice-row strips (d3d_strips.h): with strips > 1 every colour's list is
    // strip-major -- per strip its real spaxels, then its virtual positions -- and the strips of a
    // colour row run on streams of their own (run_part)
    int strips = 1;                          // 1: whole colour launches
    std::vector<int> soff;                   // [fh*fw][strips + 1] start of each strip in the colour's list
    std::vector<int> sreal;                  // [fh*fw][strips] real spaxels of each strip
    // the strips chained from colour row to colour row (option mh_strip_order; order.S == 0: joined
    // after every colour row): the schedule run_part executes, one step per active colour
    d3d_strip_order::Schedule order;
};

// What the lists and the decisions are a function of.
struct Input {
    int H = 0, W = 0, Dp = 0, fh = 0, fw = 0;
    int gy0 = 0, gx0 = 0;                // tile origin: shifts the local residues of a colour class
    Rect owned = {0, 0, 0, 0};           // the owned rectangle (local)
    bool tiled = false;
    const Rect *part_rects = nullptr;    // the parts as given (none: one part, the owned rectangle) ...
    const int *part_phase = nullptr;     // ... and their phases
    int n_part_rects = 0;
    const unsigned char *mask = nullptr; // [H*W] 1: a spaxel of the chain
    int flow_grid = 0;                   // 4 workgroups per compute unit: what fills the chip
    size_t cube_elems = 0;               // H * W * Dp
    // the sweep settings in effect (pick_mh_geometry)
    int ws_max_dp = 0;                   // deepest cube the wave-specialised kernels take unblocked
    bool mh_zb = false, deep = false;
    int mh_defer = 1, mh_layers_cfg = 2;
    bool mh_layers_forced = false;
    int mh_zigzag = 1, mh_wide = 1, mh_small = 1, mh_props = 1;
    int strips_opt = 0, strip_order_opt = 0;             // options mh_strips, mh_strip_order
    bool chain_opt = false, flow = false, pair = false;  // the experiments that run no strips
    bool uniform = false;                                // the uniform-variance kernels run
};

enum Status { OK = 0, ROW_OUTSIDE_STRIPS = 1 };

inline int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// local residues (ly, lx) of the windows of the (global) colour class `col`
// of a cube whose FSF is fh x fw and whose origin lies at (gy0, gx0) of the whole field
inline void local_residue(int fh, int fw, int gy0, int gx0, int col, int *ly, int *lx) {
    *ly = ((col / fw - gy0) % fh + fh) % fh;
    *lx = ((col % fw - gx0) % fw + fw) % fw;
}
inline void local_residue(const Input &in, int col, int *ly, int *lx) {
    local_residue(in.fh, in.fw, in.gy0, in.gx0, col, ly, lx);
}

// workgroups per window of a colour launch (the z-blocked kernels: one per 256-channel block too)
inline long wgs_per_window(const Input &in) { return in.mh_zb ? (in.Dp + 255) / 256 : 1; }

// f(y, x, real) for every lattice point of colour `col` whose window reaches the part's domain,
// ascending in (y, x)
template <class F>
void for_lattice(const Input &in, const Part &pt, int col, F f) {
    const int fhh = (in.fh - 1) / 2, fhw = (in.fw - 1) / 2;
    int ly, lx;
    local_residue(in, col, &ly, &lx);
    // first lattice coordinates whose window reaches the domain
    const int ys = ly + in.fh * floor_div(pt.dy0 - fhh - ly + in.fh - 1, in.fh);
    const int xs = lx + in.fw * floor_div(pt.dx0 - fhw - lx + in.fw - 1, in.fw);
    for (int y = ys; y - fhh < pt.dy1; y += in.fh)
        for (int x = xs; x - fhw < pt.dx1; x += in.fw)
            f(y, x, y >= pt.y0 && y < pt.y1 && x >= pt.x0 && x < pt.x1 && in.mask[(size_t)y * in.W + x] != 0);
}

// The list of colour `col` of a part appended to *list: its real spaxels (inside the part,
// unmasked) first, then the VIRTUAL positions: every other point of the class's lattice whose
// window intersects the part's domain (masked, in another part, or up to one period outside the
// cube), so that the windows of a launch tile the domain exactly.  Returns the real ones.
inline int list_one_colour(const Input &in, const Part &pt, int col, std::vector<Entry> *list) {
    const size_t at = list->size();
    for_lattice(in, pt, col, [&](int y, int x, bool real) {
        if (real) list->push_back(Entry{y, x, 1, 0});
    });
    const int n_real = (int)(list->size() - at);
    for_lattice(in, pt, col, [&](int y, int x, bool real) {
        if (!real) list->push_back(Entry{y, x, 0, 0});
    });
    return n_real;
}

// k_mh_small (d3d_mh_small.h) can take the context's small parts: thread t <-> channel t in the
// tail; window rows / columns as bits of a 32-bit mask; 32-bit byte offsets into the residual
inline bool small_usable(const Input &in) {
    return in.mh_small && in.mh_props && in.mh_defer == 1 && !in.mh_zb && !in.deep && in.Dp <= 256 &&
           in.fh <= 31 && in.fw <= 31 && (double)in.cube_elems * 8.0 < 4294967296.0;
}

// the part's colour launches run k_mh_small (its small form, or -- option mh_small = 2 -- the chip-filling one)
inline bool part_uses_tables(const Input &in, const Part &pt) {
    if (!small_usable(in)) return false;
    if (pt.small) return true;
#ifdef D3D_EXPERIMENTS
    // the chip-filling form (option mh_small = 2): one or two pending layers, 256 streaming
    // threads.  Bit-identical to k_mh_ws and measured SLOWER than it -- 43.7 against 40.6 us per
    // launch at 300x300x128, 79.6 against 76.8 at 256 channels, 27.7 against 26.5 at 64
    // (profiles/r04_table_kernel_full.txt): a launch that fills the chip is bound by HBM, not by
    // the instruction issue the tables save, and the tables themselves are 3 % more traffic.
    return in.mh_small == 2 && pt.layers <= 2 && !pt.wide;
#else
    return false;
#endif
}

// The context is cut up as far as the LISTS' decisions go (wide, strips): a tile, or part
// rectangles were given -- even a single one.  run_part (d3d_sweep.hip: partitioned_sweep) asks for
// more than one part instead; the two differ for a context given exactly one part rectangle, which
// gets no strips here and still runs the unpartitioned kernels there.
inline bool partitioned_lists(const Input &in) { return in.tiled || in.n_part_rects > 0; }

// Every colour's list of the part strip-major (stable: within a strip the order stays what it was,
// real spaxels first), soff and sreal filled.
inline int split_strips(const Input &in, const d3d_strips::Plan &plan, Part &pt, std::vector<Entry> *list) {
    const int ncol = in.fh * in.fw;
    pt.strips = plan.S;
    pt.soff.assign((size_t)ncol * (plan.S + 1), 0);
    pt.sreal.assign((size_t)ncol * plan.S, 0);
    for (int col = 0; col < ncol; ++col) {
        int ly, lx;
        local_residue(in, col, &ly, &lx);
        auto key = [&](const Entry &e) {
            return 2 * d3d_strips::strip_of_row(plan, d3d_strips::lattice_row(e.y, ly, in.fh)) + (e.real ? 0 : 1);
        };
        const auto b = list->begin() + pt.off[col], e = list->begin() + pt.off[col + 1];
        for (auto it = b; it != e; ++it)
            if (key(*it) < 0) return ROW_OUTSIDE_STRIPS;
        std::stable_sort(b, e, [&](const Entry &p, const Entry &q) { return key(p) < key(q); });
        int *so = &pt.soff[(size_t)col * (plan.S + 1)];
        for (auto it = b; it != e; ++it) {
            const int k = key(*it);
            ++so[k / 2 + 1];
            if (!(k & 1)) ++pt.sreal[(size_t)col * plan.S + k / 2];
        }
        for (int s = 0; s < plan.S; ++s) so[s + 1] += so[s];
    }
    return OK;
}

// The parts, the lists of every (part, colour) one after another in *list (Part::off indexes it),
// the real spaxels of every colour over all parts, the phases of a sweep.
inline int build(const Input &in, std::vector<Part> *parts, std::vector<Entry> *list, std::vector<int> *colour_real,
                 int *n_phases) {
    const int ncol = in.fh * in.fw;
    const int fhh = (in.fh - 1) / 2, fhw = (in.fw - 1) / 2;
    // parts: as given, else one part = the owned rectangle
    parts->clear();
    *n_phases = 1;
    auto add_part = [&](const Rect &r, int phase) {
        Part pt;
        pt.y0 = r.y0;
        pt.y1 = r.y1;
        pt.x0 = r.x0;
        pt.x1 = r.x1;
        pt.phase = phase;
        *n_phases = std::max(*n_phases, phase + 1);
        parts->push_back(pt);
    };
    if (in.n_part_rects == 0) add_part(in.owned, 0);
    for (int i = 0; i < in.n_part_rects; ++i) add_part(in.part_rects[i], in.part_phase[i]);
    list->clear();
    colour_real->assign(ncol, 0);
    const bool partitioned = partitioned_lists(in);
    for (Part &pt : *parts) {
        pt.dy0 = std::max(pt.y0 - fhh, 0);
        pt.dy1 = std::min(pt.y1 + fhh, in.H);
        pt.dx0 = std::max(pt.x0 - fhw, 0);
        pt.dx1 = std::min(pt.x1 + fhw, in.W);
        pt.off.assign(ncol + 1, 0);
        pt.real.assign(ncol, 0);
        const bool empty = pt.y1 <= pt.y0 || pt.x1 <= pt.x0;
        int most = 0;
        pt.K = 0;  // (also the ordinal of the next colour among the part's active ones)
        pt.last_col = -1;
        for (int col = 0; col < ncol; ++col) {
            pt.off[col] = (int)list->size();
            if (empty) continue;
            pt.real[col] = list_one_colour(in, pt, col, list);
            (*colour_real)[col] += pt.real[col];
            const int n_all = (int)list->size() - pt.off[col];
            // Zig-zag over the cube as well: a launch of more workgroups than the chip
            // holds runs them in list order, so every other colour starts where its
            // predecessor ended -- on the lines still in the Infinity Cache.  (Windows of
            // one colour are independent: the order changes no result.)  Only then: in a
            // launch that is resident at once, workgroup i of every colour runs on the same
            // XCD, whose L2 still holds its predecessor's window (64^3: 12.3 vs 12.6 us per
            // launch with the lists reversed).
            if (pt.real[col] > 0) {
                if (in.mh_zigzag && (pt.K & 1) && n_all * wgs_per_window(in) > in.flow_grid) {
                    const auto b = list->begin() + pt.off[col];
                    std::reverse(b, b + pt.real[col]);
                    std::reverse(b + pt.real[col], list->end());
                }
                ++pt.K;
                pt.last_col = col;
            }
            most = std::max(most, n_all);
        }
        pt.off[ncol] = (int)list->size();
        // Launches that do not fill the chip are latency chains: a second layer only adds
        // to their setup (64^3: 12.6 -> 13.0 us per colour), so they keep one.
        const long most_wgs = most * wgs_per_window(in);
        pt.layers = (!in.mh_layers_forced && most_wgs < in.flow_grid / 2) ? 1 : in.mh_layers_cfg;
        pt.wide = pt.layers == 1 && in.mh_wide && partitioned && in.Dp == 128 && most > 0 &&
                  most <= in.flow_grid / 4 && in.mh_defer == 1;
        pt.small = pt.layers == 1 && most_wgs < in.flow_grid / 2;
        // Lattice-row strips (d3d_strips.h): the whole cube of one context, the wave-specialised
        // deferred kernels, launches that fill the chip (a latency-bound launch gains nothing; a
        // forced count lifts that condition).
        // (automatic: not the uniform-variance kernels, whose launches are shorter and lose --
        // profiles/sweep_strips_ab.txt)
        pt.strips = 1;
        pt.soff.clear();
        pt.sreal.clear();
        const int want = in.strips_opt >= 2 ? in.strips_opt
                         : (in.strips_opt == 0 && most_wgs >= in.flow_grid / 2 && !in.uniform) ? MH_STRIPS_AUTO : 1;
        d3d_strips::Plan plan;
        if (want >= 2 && !empty && !partitioned && in.mh_defer == 1 && (in.Dp <= in.ws_max_dp || in.mh_zb) &&
            !part_uses_tables(in, pt) && !in.chain_opt && !in.flow && !in.pair &&
            d3d_strips::plan(in.H, in.fh, want, &plan))
            if (int rc = split_strips(in, plan, pt, list)) return rc;
        // The strips chained from colour row to colour row (d3d_strip_order.h) where the option asks for
        // it and the schedule can be built: every active colour row holds pt.layers colours at least.
        pt.order = d3d_strip_order::Schedule();
        if (pt.strips > 1 && (in.strip_order_opt ? in.strip_order_opt : MH_STRIP_ORDER_AUTO) == 2) {
            std::vector<int> active;
            for (int col = 0; col < ncol; ++col)
                if (pt.real[col] > 0) active.push_back(col);
            (void)d3d_strip_order::build(pt.strips, in.fw, active, pt.layers, &pt.order);
        }
    }
    return OK;
}

}  // namespace d3d_worklists
