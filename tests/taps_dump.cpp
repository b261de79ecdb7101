// Prints what d3d_taps::analyse (deconv3d_amd/csrc/d3d_taps.h, host-only) makes of the cases on its
// standard input, as text with every double in C's hexadecimal form (exact);
// tests/test_taps_cpu.py compares it with a restatement of the rules.  A case:
//   fh fw D N H W HL flow_grid LSF_RL thr spatial_sep march_hy_opt has_lsf
//   the fh * fw values of the FSF, then (has_lsf) the D values of the LSF
// Stand-alone, with its own main: compiled by the host compiler with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "d3d_taps.h"

static bool read_double(double *v) {
    std::string w;
    if (!(std::cin >> w)) return false;
    *v = std::strtod(w.c_str(), nullptr);  // (takes the hexadecimal form)
    return true;
}

static void row(const char *name, const std::vector<double> &v) {
    std::printf("%s", name);
    for (double x : v) std::printf(" %a", x);
    std::printf("\n");
}

int main() {
    for (;;) {
        int fh, fw, D, N, H, W, HL, flow_grid, RL, spatial_sep, march_hy_opt, has_lsf;
        double thr;
        if (!(std::cin >> fh >> fw >> D >> N >> H >> W >> HL >> flow_grid >> RL)) break;
        if (!read_double(&thr) || !(std::cin >> spatial_sep >> march_hy_opt >> has_lsf)) return 2;
        std::vector<double> fsf((size_t)fh * fw), lsf(has_lsf ? D : 0);
        for (double &v : fsf)
            if (!read_double(&v)) return 2;
        for (double &v : lsf)
            if (!read_double(&v)) return 2;
        const d3d_taps::Result r = d3d_taps::analyse(fh, fw, D, N, H, W, HL, flow_grid, RL, fsf.data(),
                                                     has_lsf ? lsf.data() : nullptr, thr, spatial_sep, march_hy_opt);
        std::printf("case %d %d %d %d %d %d %d %d %d %d\n", r.symx, r.symy, r.sep, r.symt, r.march_hy, r.lsf_empty,
                    r.dense_any, r.dense_ok, r.dense_sym, r.fusable);
        row("uv", r.uv);
        row("quad", r.quad);
        row("quad_sep", r.quad_sep);
        std::printf("shift");
        for (int s : r.shift) std::printf(" %d", s);
        std::printf("\n");
        row("weight", r.weight);
        row("dense", r.dense);
    }
    return 0;
}
