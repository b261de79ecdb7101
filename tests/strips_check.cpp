// The row -> strip rule of deconv3d_amd/csrc/d3d_strips.h over every cube height, FSF height,
// colour row and strip count tests/test_strips_cpu.py asks for.  Host code only; built with
// -fsanitize=address,undefined and run as a child process.  Exit status 0 and "ok <plans> <refused>"
// on success, a message and status 1 on the first violation.
#include <cstdio>
#include <vector>

#include "d3d_strips.h"

static int bad(const char *what, int H, int fh, int S, int cy, int i) {
    std::printf("FAIL %s: H=%d fh=%d S=%d cy=%d row=%d\n", what, H, fh, S, cy, i);
    return 1;
}

static int check(int H, int fh, int S, long *plans, long *refused) {
    using namespace d3d_strips;
    const int fhh = (fh - 1) / 2, end = rows_end(H, fh), rows = end - ROWS_BEGIN;
    Plan p;
    const bool ok = plan(H, fh, S, &p);
    // a strip count that leaves a strip with fewer than MIN_ROWS lattice rows is refused -- and only that
    if (rows < MIN_ROWS * S) {
        if (ok || p.S != 0) return bad("too few rows accepted", H, fh, S, -1, rows);
        ++*refused;
        return 0;
    }
    if (!ok || p.S != S) return bad("refused", H, fh, S, -1, rows);
    ++*plans;
    // strips are contiguous, in order, cover ROWS_BEGIN .. end and hold MIN_ROWS rows each
    if (p.first[0] != ROWS_BEGIN || p.first[S] != end) return bad("ends", H, fh, S, -1, p.first[0]);
    for (int s = 0; s < S; ++s)
        if (p.first[s + 1] - p.first[s] < MIN_ROWS) return bad("short strip", H, fh, S, -1, s);
    // every lattice row there can be, virtual ones included, is in exactly one strip
    for (int i = ROWS_BEGIN - 2; i < end + 2; ++i) {
        int in = 0;
        for (int s = 0; s < S; ++s) in += i >= p.first[s] && i < p.first[s + 1];
        const int s = strip_of_row(p, i);
        const bool inside = i >= ROWS_BEGIN && i < end;
        if (in != (inside ? 1 : 0) || (s >= 0) != inside) return bad("membership", H, fh, S, -1, i);
        if (inside && !(i >= p.first[s] && i < p.first[s + 1])) return bad("strip_of_row", H, fh, S, -1, i);
        if (inside && i > ROWS_BEGIN && strip_of_row(p, i - 1) > s) return bad("order", H, fh, S, -1, i);
    }
    for (int cy = 0; cy < fh; ++cy) {
        // every window row of the class that reaches the cube is a lattice row of the plan ...
        std::vector<int> owner(H, -1);
        for (int y = cy - 2 * fh; y - fhh < H; y += fh) {
            if (y + fhh < 0) continue;
            const int i = lattice_row(y, cy, fh);
            if (cy + fh * i != y) return bad("lattice_row", H, fh, S, cy, i);
            const int s = strip_of_row(p, i);
            if (s < 0) return bad("window row outside the plan", H, fh, S, cy, i);
            // ... and the cube rows of its band belong to no other strip: the bands of different
            // strips are disjoint (and the bands together cover the cube)
            for (int r = y - fhh; r <= y + fhh; ++r) {
                if (r < 0 || r >= H) continue;
                if (owner[r] >= 0 && owner[r] != s) return bad("bands of two strips overlap", H, fh, S, cy, i);
                owner[r] = s;
            }
        }
        for (int r = 0; r < H; ++r) {
            if (owner[r] < 0) return bad("cube row in no band", H, fh, S, cy, r);
            if (r > 0 && owner[r] < owner[r - 1]) return bad("bands out of order", H, fh, S, cy, r);
        }
    }
    return 0;
}

int main() {
    const int fhs[3] = {3, 5, 11};
    long plans = 0, refused = 0;
    for (int k = 0; k < 3; ++k)
        for (int S = 2; S <= 4; ++S) {
            for (int H = 11; H <= 40; ++H)
                if (check(H, fhs[k], S, &plans, &refused)) return 1;
            if (check(300, fhs[k], S, &plans, &refused)) return 1;
        }
    // out of range: refused
    d3d_strips::Plan p;
    if (d3d_strips::plan(300, 11, 1, &p) || d3d_strips::plan(300, 11, 5, &p) || d3d_strips::plan(0, 11, 2, &p)) {
        std::printf("FAIL a strip count or height out of range accepted\n");
        return 1;
    }
    // balance at the flagship shape: no strip more than one lattice row's weight from the mean
    for (int S = 2; S <= 4; ++S) {
        d3d_strips::plan(300, 11, S, &p);
        long total = 0, most = 0;
        for (int i = d3d_strips::ROWS_BEGIN; i < d3d_strips::rows_end(300, 11); ++i) {
            const long w = d3d_strips::row_weight(300, 11, i);
            total += w;
            most = w > most ? w : most;
        }
        for (int s = 0; s < S; ++s) {
            long w = 0;
            for (int i = p.first[s]; i < p.first[s + 1]; ++i) w += d3d_strips::row_weight(300, 11, i);
            if (w * S > total + most * S || w * S < total - most * S) {
                std::printf("FAIL balance: S=%d strip %d weight %ld of %ld\n", S, s, w, total);
                return 1;
            }
        }
    }
    std::printf("ok %ld %ld\n", plans, refused);
    return 0;
}
