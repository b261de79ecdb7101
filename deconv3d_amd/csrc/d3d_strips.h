// Lattice-row strips of a colour row: which strip a lattice row of windows
// belongs to.  Host-only, no HIP: tests/test_strips_cpu.py compiles it alone.
//
// The windows of colour class (cy, cx) sit at the cube rows y = cy + fh * i.  Lattice row i runs
// from -1 (a virtual row above the cube whose windows still reach into it) to rows_end - 1 (the
// last row whose window reaches row H - 1 for some cy).  A window of lattice row i covers the cube
// rows cy + fh * i - fhh ... cy + fh * i + fhh: for one cy these bands are disjoint across i, so
// the launches of the colours (cy, 0 ... fw - 1) on one contiguous range of lattice rows neither
// read nor write what another range's launches write.  The rule is the same for every cy and cx.
#pragma once

namespace d3d_strips {

constexpr int MAX_STRIPS = 4;
constexpr int MIN_ROWS = 2;    // lattice rows a strip holds at least
constexpr int ROWS_BEGIN = -1;  // the first lattice row there can be

struct Plan {
    int S = 0;                      // strips (0: no plan)
    int first[MAX_STRIPS + 1] = {}; // strip s holds the lattice rows first[s] ... first[s + 1] - 1
};

// one past the last lattice row there can be: the largest i with cy + fh * i - fhh <= H - 1 is at cy = 0
inline int rows_end(int H, int fh) { return (H - 1 + (fh - 1) / 2) / fh + 1; }

// lattice row of the window at cube row y of a class with row residue cy (y = cy + fh * i, y may be < 0)
inline int lattice_row(int y, int cy, int fh) {
    const int d = y - cy;
    return d >= 0 ? d / fh : -((-d + fh - 1) / fh);
}

// cube rows of lattice row i's band inside the cube, summed over every cy: what its windows stream
inline long row_weight(int H, int fh, int i) {
    const int fhh = (fh - 1) / 2;
    long w = 0;
    for (int cy = 0; cy < fh; ++cy) {
        const int y = cy + fh * i;
        const int lo = y - fhh > 0 ? y - fhh : 0, hi = y + fhh < H - 1 ? y + fhh : H - 1;
        if (hi >= lo) w += hi - lo + 1;
    }
    return w;
}

// S strips of contiguous lattice rows, balanced by the rows of the cube their windows cover (the
// clipped first and last lattice rows are cheaper), MIN_ROWS lattice rows each at least.
// false: refused -- S out of range, or too few lattice rows.
inline bool plan(int H, int fh, int S, Plan *out) {
    *out = Plan();
    if (H < 1 || fh < 1 || S < 2 || S > MAX_STRIPS) return false;
    const int end = rows_end(H, fh);
    if (end - ROWS_BEGIN < MIN_ROWS * S) return false;
    long total = 0;
    for (int i = ROWS_BEGIN; i < end; ++i) total += row_weight(H, fh, i);
    out->first[0] = ROWS_BEGIN;
    long cum = 0;  // weight of the rows before `at`
    int at = ROWS_BEGIN;
    for (int s = 1; s < S; ++s) {
        const int lo = out->first[s - 1] + MIN_ROWS, hi = end - MIN_ROWS * (S - s);
        // the boundary whose cumulated weight is nearest to s / S of the total, within [lo, hi]
        while (at < lo) cum += row_weight(H, fh, at++);
        while (at < hi) {
            const long w = row_weight(H, fh, at);
            if (2 * S * (cum + w) - 2 * s * total > 2 * s * total - 2 * S * cum) break;  // |next| > |here|
            cum += w;
            ++at;
        }
        out->first[s] = at;
    }
    out->first[S] = end;
    out->S = S;
    return true;
}

// strip of lattice row i (ROWS_BEGIN <= i < rows_end), -1 outside
inline int strip_of_row(const Plan &p, int i) {
    for (int s = 0; s < p.S; ++s)
        if (i >= p.first[s] && i < p.first[s + 1]) return s;
    return -1;
}

}  // namespace d3d_strips
