// Lattice-row strips chained from colour row to colour row (option
// mh_strip_order): the schedule of one sweep -- per active colour and strip the events the strip's
// stream waits on before its launch, those it records after it, and the G buffer the colour
// writes.  Host-only, no HIP: tests/test_strip_order_cpu.py compiles it alone, builds the access
// sets of every launch of three sweeps from it and proves every conflicting pair ordered;
// d3d_sweep.hip: StripScope executes it and nothing else.
//
// Strip s holds the lattice rows first[s] ... first[s + 1] - 1 (d3d_strips.h); at the colour row
// cy its windows cover the cube rows cy + fh * first[s] - fhh ... cy + fh * (first[s + 1] - 1) + fhh.
// From one active colour row to the next (cy grows inside a sweep) every band moves down, by fewer
// cube rows than a strip holds:
//   DOWN  strip s starts the row a + 1 after strip s + 1 has ended the row a: the lowest cube
//         rows of its band were strip s + 1's, and the layers still pending from the row a have
//         their G rows for them in strip s + 1's first slot row.  Strip s + 1 needs nothing of
//         strip s: what it touches was its own in every earlier row of the sweep.
//   UP    strip s + 1 starts the row a + 1 after strip s has run the first M active colours of the
//         row a -- the only launches that read G rows of another colour row, hence of strip
//         s + 1.  The G buffers are two pools of M + 1, the active rows take them in turn, a row
//         rotates through its pool: strip s + 1 in the row a + 1 writes the pool of the row
//         a - 1, which strip s read in the first M launches of the row a and never again.
//   JOIN  at the sweep's end everything joins: at the wrap the bands jump up and the dependency
//         turns round (strip s reads strip s - 1's last slot row, in the pool of the last row;
//         strip s - 1 writes that pool again in the second row, behind DOWN).  The pools go on
//         alternating across sweeps (pool_after).
// Every active colour row must hold M active colours at least, so that no layer stays pending
// across two changes of row; build() refuses otherwise and the strips keep their join per row.
#pragma once

#include <vector>

#include "d3d_strips.h"

namespace d3d_strip_order {

constexpr int MAX_STRIPS = d3d_strips::MAX_STRIPS;
constexpr int MAX_LAYERS = 3;                 // pending layers a kernel takes at most
constexpr int GSLOTS = 2 * (MAX_LAYERS + 1);  // G buffers the schedule names at most

// events: bit e of a mask is event e
constexpr int EV_FORK = 0;                                            // strip 0 -> every other strip
constexpr int ev_down(int s) { return s; }                            // strip s (>= 1) -> strip s - 1
constexpr int ev_up(int s) { return MAX_STRIPS + s; }                 // strip s (<= S - 2) -> strip s + 1
constexpr int ev_join(int s) { return 2 * MAX_STRIPS - 1 + s; }       // strip s (>= 1) -> strip 0
constexpr int NEV = 3 * MAX_STRIPS - 1;

struct Step {  // one active colour
    int col = 0;                      // its index cy * fw + cx
    int row = 0;                      // ordinal of its colour row among the active ones
    bool first_of_row = false;
    int pool = 0, gidx = 0;           // the G buffer it writes: gslot()
    unsigned pre[MAX_STRIPS] = {};    // events strip s records before the colour's waits (the fork)
    unsigned wait[MAX_STRIPS] = {};   // events strip s waits on before its launch of the colour
    unsigned post[MAX_STRIPS] = {};   // events strip s records after its launch of the colour
};

struct Schedule {
    int S = 0, M = 0, rows = 0;        // strips (0: none), pending-layer capacity, active colour rows
    std::vector<Step> steps;           // the sweep's active colours in order
    unsigned tail_post[MAX_STRIPS] = {};  // the sweep-end join: recorded after the last colour ...
    unsigned tail_wait[MAX_STRIPS] = {};  // ... then waited on
};

// G buffer slot (0 ... 2 * (M + 1) - 1) of a step in a sweep whose first active row takes pool0
inline int gslot(const Schedule &sd, const Step &st, int pool0) { return ((st.pool ^ pool0) & 1) * (sd.M + 1) + st.gidx; }
// pool of the first active row of the sweep after one that began with pool0
inline int pool_after(const Schedule &sd, int pool0) { return (pool0 ^ sd.rows) & 1; }

// colours: the colours with at least one real spaxel, ascending; a colour's row is col / fw.
// false: refused (*out empty) -- S or M out of range, no colour, or an active row of fewer than M colours.
inline bool build(int S, int fw, const std::vector<int> &colours, int M, Schedule *out) {
    *out = Schedule();
    if (S < 2 || S > MAX_STRIPS || M < 1 || M > MAX_LAYERS || fw < 1 || colours.empty()) return false;
    Schedule sd;
    const int n = (int)colours.size();
    sd.steps.resize(n);
    int row = -1, in_row = 0, last_cr = -1;
    for (int k = 0; k < n; ++k) {
        if (colours[k] < 0 || (k && colours[k] <= colours[k - 1])) return false;
        const int cr = colours[k] / fw;
        if (cr != last_cr) {
            if (row >= 0 && in_row < M) return false;
            ++row;
            in_row = 0;
            last_cr = cr;
        }
        Step &st = sd.steps[k];
        st.col = colours[k];
        st.row = row;
        st.first_of_row = in_row == 0;
        st.pool = row & 1;
        st.gidx = in_row % (M + 1);
        ++in_row;
    }
    if (in_row < M) return false;
    sd.rows = row + 1;
    for (int k = 0; k < n; ++k) {
        Step &st = sd.steps[k];
        if (k == 0) {  // FORK
            st.pre[0] |= 1u << EV_FORK;
            for (int s = 1; s < S; ++s) st.wait[s] |= 1u << EV_FORK;
        }
        const bool last_of_row = k + 1 == n || sd.steps[k + 1].row != st.row;
        const bool more_rows = st.row + 1 < sd.rows;
        int ord = 0;  // ordinal of the colour in its row
        for (int j = k; j > 0 && sd.steps[j - 1].row == st.row; --j) ++ord;
        if (more_rows && last_of_row)  // DOWN
            for (int s = 1; s < S; ++s) st.post[s] |= 1u << ev_down(s);
        if (more_rows && ord == M - 1)  // UP
            for (int s = 0; s + 1 < S; ++s) st.post[s] |= 1u << ev_up(s);
        if (st.first_of_row && st.row > 0)
            for (int s = 0; s < S; ++s) {
                if (s + 1 < S) st.wait[s] |= 1u << ev_down(s + 1);
                if (s > 0) st.wait[s] |= 1u << ev_up(s - 1);
            }
    }
    for (int s = 1; s < S; ++s) {  // JOIN
        sd.tail_post[s] |= 1u << ev_join(s);
        sd.tail_wait[0] |= 1u << ev_join(s);
    }
    sd.S = S;
    sd.M = M;
    *out = sd;
    return true;
}

}  // namespace d3d_strip_order
