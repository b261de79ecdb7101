// The chained schedule of the lattice-row strips (deconv3d_amd/csrc/d3d_strip_order.h) without a
// device.  From the schedule -- the very structure d3d_sweep.hip: StripScope executes -- it lists every
// launch (strip, colour, sweep) of three consecutive sweeps with what the launch reads and writes:
//   the cube rows its windows read, and write where the launch stores (the alternation of M pending
//     layers carried across the sweep boundaries);
//   the (G buffer, slot row) it writes, and reads for every pending layer (covering_coord of
//     d3d_kernels.h over the band's cube rows);
//   the spaxel rows whose state it writes, and with the smoothness prior the rows y +- 1 it reads.
// Happens-before comes from stream order plus the schedule's events (vector clocks).  Every pair of
// launches of different strips whose sets conflict must be ordered, in the sequential colour order.
// Negative controls: the same schedule without the DOWN waits, without the UP waits and without the
// sweep-end join must each report a conflict.  Host code only; built with -fsanitize=address,undefined
// and run as a child process.  "ok <proved> <refused by plan> <refused short row> <controls>" and exit
// status 0 on success, a message and status 1 on the first violation.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "d3d_strip_order.h"
#include "d3d_strips.h"

namespace so = d3d_strip_order;

typedef std::vector<uint64_t> Bits;
static void set_bit(Bits &b, int i) { b[(size_t)i >> 6] |= uint64_t(1) << (i & 63); }
static bool meet(const Bits &a, const Bits &b) {
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i] & b[i]) return true;
    return false;
}

// d3d_kernels.h: covering_coord
static int covering_coord(int q, int c, int per, int hw, int n) {
    int m = (q - c) % per;
    if (m < 0) m += per;
    int s = q - m;
    if (q - s > hw) s += per;
    return (s >= 0 && s < n) ? s : -1;
}

struct Launch {
    int strip = 0, idx = 0;  // its place on its strip's stream
    long seq = 0;            // its colour's place in the sequential order
    int clock[so::MAX_STRIPS] = {};  // launches of every strip that are known to have ended before it starts
    Bits cube_r, cube_w, g_r, g_w, par_w, par_r;
};

struct Layer {
    int cy, g;
};

struct Case {
    int H, fh, fw, S, M;
    d3d_strips::Plan plan;
};

// The launches of `sweeps` sweeps under schedule sd (which the caller may have mutilated).
static std::vector<Launch> launches(const Case &cs, const so::Schedule &sd, int sweeps) {
    const int H = cs.H, fh = cs.fh, fhh = (fh - 1) / 2, S = cs.S;
    const int slot_rows = (H - 1) / fh + 1;
    const size_t wc = (size_t)(H + 63) / 64, wg = (size_t)(so::GSLOTS * slot_rows + 63) / 64;
    std::vector<Launch> out;
    int vc[so::MAX_STRIPS][so::MAX_STRIPS] = {}, ev[so::NEV][so::MAX_STRIPS] = {}, count[so::MAX_STRIPS] = {};
    auto record = [&](unsigned mask, int s) {
        for (int e = 0; e < so::NEV; ++e)
            if ((mask >> e) & 1) std::copy(vc[s], vc[s] + so::MAX_STRIPS, ev[e]);
    };
    auto wait = [&](unsigned mask, int s) {
        for (int e = 0; e < so::NEV; ++e)
            if ((mask >> e) & 1)
                for (int t = 0; t < so::MAX_STRIPS; ++t) vc[s][t] = std::max(vc[s][t], ev[e][t]);
    };
    std::vector<Layer> lay;  // pending layers, oldest first
    int pool0 = 0;
    long seq = 0;
    for (int sw = 0; sw < sweeps; ++sw) {
        for (const so::Step &st : sd.steps) {
            for (int s = 0; s < S; ++s) record(st.pre[s], s);
            for (int s = 0; s < S; ++s) wait(st.wait[s], s);
            const int cy = st.col / cs.fw, g_cur = so::gslot(sd, st, pool0);
            const bool storing = (int)lay.size() >= cs.M;
            for (int s = 0; s < S; ++s) {
                Launch L;
                L.strip = s;
                L.idx = count[s]++;
                L.seq = seq;
                std::copy(vc[s], vc[s] + so::MAX_STRIPS, L.clock);
                vc[s][s] = count[s];
                L.cube_r.assign(wc, 0);
                L.cube_w.assign(wc, 0);
                L.par_w.assign(wc, 0);
                L.par_r.assign(wc, 0);
                L.g_r.assign(wg, 0);
                L.g_w.assign(wg, 0);
                for (int i = cs.plan.first[s]; i < cs.plan.first[s + 1]; ++i) {
                    const int y = cy + fh * i;
                    for (int yy = std::max(0, y - fhh); yy <= std::min(H - 1, y + fhh); ++yy) {
                        set_bit(L.cube_r, yy);
                        if (storing) set_bit(L.cube_w, yy);
                        for (const Layer &l : lay) {
                            const int sy = covering_coord(yy, l.cy, fh, fhh, H);
                            if (sy >= 0) set_bit(L.g_r, l.g * slot_rows + sy / fh);
                        }
                    }
                    if (y >= 0 && y < H) {
                        set_bit(L.g_w, g_cur * slot_rows + y / fh);
                        set_bit(L.par_w, y);
                        if (y > 0) set_bit(L.par_r, y - 1);
                        if (y + 1 < H) set_bit(L.par_r, y + 1);
                    }
                }
                out.push_back(L);
            }
            for (int s = 0; s < S; ++s) record(st.post[s], s);
            if (storing) lay.clear();
            lay.push_back({cy, g_cur});
            ++seq;
        }
        for (int s = 0; s < S; ++s) record(sd.tail_post[s], s);
        for (int s = 0; s < S; ++s) wait(sd.tail_wait[s], s);
        pool0 = so::pool_after(sd, pool0);
        // what follows a sweep on strip 0's stream (snapshot, moments, adaptation, a fresh residual, a
        // write-back of the pending layers): it may read and write everything
        Launch E;
        E.idx = count[0]++;
        E.seq = seq++;
        std::copy(vc[0], vc[0] + so::MAX_STRIPS, E.clock);
        vc[0][0] = count[0];
        E.cube_r.assign(wc, ~uint64_t(0));
        E.par_r.assign(wc, ~uint64_t(0));
        E.g_r.assign(wg, ~uint64_t(0));
        E.cube_w = E.cube_r;
        E.par_w = E.par_r;
        E.g_w.assign(wg, 0);
        out.push_back(E);
    }
    return out;
}

// conflicting pairs of launches that are not ordered in the sequential colour order
static long violations(const std::vector<Launch> &ls, bool prior, const Launch **a_out, const Launch **b_out) {
    long bad = 0;
    for (size_t i = 0; i < ls.size(); ++i)
        for (size_t j = i + 1; j < ls.size(); ++j) {
            const Launch &A = ls[i], &B = ls[j];  // A.seq <= B.seq
            if (A.strip == B.strip) continue;     // stream order
            if (A.seq < B.seq && B.clock[A.strip] > A.idx) continue;  // A ends before B starts
            const bool hit = meet(A.cube_w, B.cube_w) || meet(A.cube_w, B.cube_r) || meet(A.cube_r, B.cube_w) ||
                             meet(A.g_w, B.g_w) || meet(A.g_w, B.g_r) || meet(A.g_r, B.g_w) ||
                             meet(A.par_w, B.par_w) ||
                             (prior && (meet(A.par_w, B.par_r) || meet(A.par_r, B.par_w)));
            if (hit && !bad++) {
                *a_out = &A;
                *b_out = &B;
            }
        }
    return bad;
}

static void strip_waits(so::Schedule &sd, bool down, bool up) {
    unsigned drop = 0;
    for (int s = 0; s < so::MAX_STRIPS; ++s) {
        if (down && s >= 1) drop |= 1u << so::ev_down(s);
        if (up && s + 1 < so::MAX_STRIPS) drop |= 1u << so::ev_up(s);
    }
    for (so::Step &st : sd.steps)
        for (int s = 0; s < so::MAX_STRIPS; ++s) st.wait[s] &= ~drop;
}

static int fail(const char *what, const Case &cs, int set, const Launch *A, const Launch *B) {
    std::printf("FAIL %s: H=%d fh=%d fw=%d S=%d M=%d colour set %d", what, cs.H, cs.fh, cs.fw, cs.S, cs.M, set);
    if (A && B) std::printf(" (strip %d colour #%ld against strip %d colour #%ld)", A->strip, A->seq, B->strip, B->seq);
    std::printf("\n");
    return 1;
}

int main() {
    long proved = 0, refused_plan = 0, refused_short = 0, controls = 0;
    std::vector<int> heights;
    for (int H = 11; H <= 40; ++H) heights.push_back(H);
    heights.push_back(300);
    const int fhs[3] = {3, 5, 11};
    for (int H : heights)
        for (int fh : fhs)
            for (int wide = 0; wide < 2; ++wide) {
                const int fw = wide ? fh : 4;  // (square taps at the flagship height only: fw does not enter the bands)
                if (wide && H != 300) continue;
                for (int S = 2; S <= 4; ++S) {
                    Case cs = {H, fh, fw, S, 0, {}};
                    if (!d3d_strips::plan(H, fh, S, &cs.plan)) {
                        ++refused_plan;
                        continue;
                    }
                    for (int M = 1; M <= so::MAX_LAYERS; ++M) {
                        cs.M = M;
                        // colour sets: 0 all, 1 one whole colour row inactive, 2 single colours inactive
                        for (int set = 0; set < 3; ++set) {
                            std::vector<int> colours;
                            int fewest = fw;
                            for (int r = 0; r < fh; ++r) {
                                int n = 0;
                                for (int x = 0; x < fw; ++x) {
                                    if (set == 1 && r == 1) continue;
                                    if (set == 2 && r % 2 == 0 && x == r % fw) continue;
                                    colours.push_back(r * fw + x);
                                    ++n;
                                }
                                if (n) fewest = std::min(fewest, n);
                            }
                            so::Schedule sd;
                            const bool ok = so::build(S, fw, colours, M, &sd);
                            if (fewest < M) {  // a row that cannot retire its predecessor's layers: refused, and only that
                                if (ok || sd.S) return fail("short row accepted", cs, set, nullptr, nullptr);
                                ++refused_short;
                                continue;
                            }
                            if (!ok || sd.S != S || sd.M != M || sd.steps.size() != colours.size())
                                return fail("refused", cs, set, nullptr, nullptr);
                            for (size_t k = 0; k < colours.size(); ++k)
                                if (sd.steps[k].col != colours[k] || so::gslot(sd, sd.steps[k], 0) >= 2 * (M + 1) ||
                                    so::gslot(sd, sd.steps[k], 1) >= 2 * (M + 1))
                                    return fail("step", cs, set, nullptr, nullptr);
                            const Launch *A = nullptr, *B = nullptr;
                            const std::vector<Launch> ls = launches(cs, sd, 3);
                            if (violations(ls, false, &A, &B)) return fail("unordered conflict", cs, set, A, B);
                            if (violations(ls, true, &A, &B)) return fail("unordered conflict under the prior", cs, set, A, B);
                            ++proved;
                            if (set) continue;
                            // the checker can fail: each edge removed must show
                            so::Schedule cut = sd;
                            strip_waits(cut, true, false);
                            if (!violations(launches(cs, cut, 3), false, &A, &B)) return fail("DOWN removed, no conflict", cs, set, nullptr, nullptr);
                            cut = sd;
                            strip_waits(cut, false, true);
                            if (!violations(launches(cs, cut, 3), false, &A, &B)) return fail("UP removed, no conflict", cs, set, nullptr, nullptr);
                            cut = sd;
                            for (int s = 0; s < so::MAX_STRIPS; ++s) cut.tail_wait[s] = 0;
                            if (!violations(launches(cs, cut, 3), false, &A, &B)) return fail("JOIN removed, no conflict", cs, set, nullptr, nullptr);
                            controls += 3;
                        }
                    }
                }
            }
    std::printf("ok %ld %ld %ld %ld\n", proved, refused_plan, refused_short, controls);
    return 0;
}
