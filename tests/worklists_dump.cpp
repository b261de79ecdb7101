// Prints what d3d_worklists::build (deconv3d_amd/csrc/d3d_worklists.h, host-only) makes of the cases
// on its standard input, as text; tests/test_worklists_cpu.py compares it with a restatement of the
// rules.  A case is three lines:
//   H W Dp fh fw gy0 gx0 oy0 oy1 ox0 ox1 tiled flow_grid ws_max_dp mh_zb deep mh_defer mh_layers_cfg
//     mh_layers_forced mh_zigzag mh_wide mh_small mh_props strips_opt strip_order_opt chain_opt flow pair uniform
//   n_parts, then y0 y1 x0 x1 phase of every part
//   the H * W values of the mask
// Stand-alone, with its own main: compiled by the host compiler with -fsanitize=address,undefined.
#include <cstdio>
#include <iostream>
#include <vector>

#include "d3d_worklists.h"

namespace wl = d3d_worklists;

static void row(const char *name, const std::vector<int> &v) {
    std::printf("%s", name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}

int main() {
    for (;;) {
        wl::Input in;
        int tiled, zb, deep, forced, chain, flow, pair, uniform, n_parts;
        if (!(std::cin >> in.H >> in.W >> in.Dp >> in.fh >> in.fw >> in.gy0 >> in.gx0 >> in.owned.y0 >> in.owned.y1 >>
              in.owned.x0 >> in.owned.x1 >> tiled >> in.flow_grid >> in.ws_max_dp >> zb >> deep >> in.mh_defer >>
              in.mh_layers_cfg >> forced >> in.mh_zigzag >> in.mh_wide >> in.mh_small >> in.mh_props >> in.strips_opt >>
              in.strip_order_opt >> chain >> flow >> pair >> uniform >> n_parts))
            break;
        in.tiled = tiled;
        in.mh_zb = zb;
        in.deep = deep;
        in.mh_layers_forced = forced;
        in.chain_opt = chain;
        in.flow = flow;
        in.pair = pair;
        in.uniform = uniform;
        in.cube_elems = (size_t)in.H * in.W * in.Dp;
        std::vector<wl::Rect> rects(n_parts);
        std::vector<int> phases(n_parts);
        for (int i = 0; i < n_parts; ++i) std::cin >> rects[i].y0 >> rects[i].y1 >> rects[i].x0 >> rects[i].x1 >> phases[i];
        std::vector<unsigned char> mask((size_t)in.H * in.W);
        for (unsigned char &m : mask) {
            int v;
            std::cin >> v;
            m = (unsigned char)v;
        }
        if (!std::cin) {
            std::fprintf(stderr, "truncated case\n");
            return 2;
        }
        in.part_rects = rects.data();
        in.part_phase = phases.data();
        in.n_part_rects = n_parts;
        in.mask = mask.data();

        std::vector<wl::Part> parts;
        std::vector<wl::Entry> list;
        std::vector<int> colour_real;
        int n_phases = 0;
        const int rc = wl::build(in, &parts, &list, &colour_real, &n_phases);
        std::printf("case %d %d %zu %zu %d %d\n", rc, n_phases, parts.size(), list.size(), wl::small_usable(in) ? 1 : 0,
                    wl::partitioned_lists(in) ? 1 : 0);
        row("colour_real", colour_real);
        for (int S = 2; S <= d3d_strips::MAX_STRIPS; ++S) {  // what d3d_strips::plan gives for this cube
            d3d_strips::Plan p;
            d3d_strips::plan(in.H, in.fh, S, &p);
            std::printf("plan %d", p.S);
            for (int s = 0; s <= p.S; ++s) std::printf(" %d", p.first[s]);
            std::printf("\n");
        }
        for (const wl::Part &pt : parts) {
            std::printf("part %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", pt.y0, pt.y1, pt.x0, pt.x1, pt.dy0,
                        pt.dy1, pt.dx0, pt.dx1, pt.phase, pt.layers, pt.wide ? 1 : 0, pt.small ? 1 : 0, pt.strips, pt.K,
                        pt.last_col, pt.order.S, pt.order.M, wl::part_uses_tables(in, pt) ? 1 : 0);
            row("off", pt.off);
            row("real", pt.real);
            row("soff", pt.soff);
            row("sreal", pt.sreal);
        }
        std::printf("list");
        for (const wl::Entry &e : list) std::printf(" %d %d %d %d", e.y, e.x, e.real, e.pad);
        std::printf("\n");
    }
    return 0;
}
