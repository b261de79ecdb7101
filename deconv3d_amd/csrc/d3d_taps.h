// The forms of the taps (d3d_set_taps): what the FSF's symmetries let the spatial kernels use, the
// rows per strip of the march kernels, the LSF's tap list after the cut and its dense form for the
// fused / z-blocked kernels.  A pure function of the shape, the taps and three options.  Host-only,
// no HIP: tests/test_taps_cpu.py compiles it alone (tests/taps_dump.cpp) and compares every value
// with a restatement of the rules; d3d_api.hip uploads what the flags say and decides nothing.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

namespace d3d_taps {

struct Result {
    // FSF
    bool symx = false;             // fsf[k][i] == fsf[k][fw-1-i] bit for bit
    bool symy = false;             // fsf[k][i] == fsf[fh-1-k][i] bit for bit
    bool sep = false;              // fsf == u v^T to rounding, and option spatial_sep allows it
    bool symt = false;             // square, symx, symy and fsf[k][i] == fsf[i][k] bit for bit (radial FSFs)
    std::vector<double> uv;        // [fh + fw] u = centre column / centre tap, v = centre row (sep)
    std::vector<double> quad;      // [(fhh+1)^2] quad[a][e] = fsf[fhh-a][fhh-e] (square, symx, symy; else empty)
    std::vector<double> quad_sep;  // the same table's outer-product form: row 0 = v, row 1 = u (... and sep; else empty)
    int march_hy = 16;             // output rows per strip of the march kernels
    // LSF: out[k] = sum_t weight[t] v[(k + shift[t]) mod N]; empty without an LSF
    std::vector<int> shift;
    std::vector<double> weight;
    bool lsf_empty = false;        // an LSF was given and the cut left no tap: refused
    // its dense form: out[k] = sum_j dense[j] v[(k + j - RL) mod N] (every tap within +-RL channels, N >= 4 RL)
    std::vector<double> dense;     // [2 RL + 1], zeros unless dense_any
    bool dense_any = false;        // ... at ANY depth (k_spectral_blocks, the z-blocked sweep kernels)
    bool dense_ok = false;         // ... and power-of-two depth, N == D (z-major spectral kernel)
    bool dense_sym = false;        // dense_any and mirror-symmetric bit for bit
    bool fusable = false;          // dense_ok and the spectrum within one wavefront (HL divides 64)
};

// Largest magnitude the cut drops.  thr >= 0: taps up to thr * max|lsf| are dropped.  thr < 0 (the
// python host's default -1e-16): an ERROR BOUND -- the smallest taps are dropped as long as their
// summed magnitude stays within |thr| * sum|lsf|, i.e. below the rounding of the fp64 sum itself.
// (1e-20 * max kept a Gaussian's tail out to 9.6 sigma, and the physics-free threshold, not the
// LSF, decided whether the taps fit the +-LSF_RL channels of the fused / z-blocked kernels:
// sigma >= 0.94 px fell off them.  The bound keeps 8.6 sigma: MUSE's 2.4-3.0 A LSF at 1.25 A per
// channel, sigma 0.82-1.02 px, fits.)
inline double lsf_cut(const double *lsf, int D, double thr) {
    double mx = 0.0, total = 0.0;
    for (int t = 0; t < D; ++t) {
        mx = std::fmax(mx, std::fabs(lsf[t]));
        total += std::fabs(lsf[t]);
    }
    if (!(thr < 0.0)) return thr * mx;
    std::vector<double> mag(lsf, lsf + D);
    for (double &m : mag) m = std::fabs(m);
    std::sort(mag.begin(), mag.end());
    double dropped = 0.0, cut = 0.0;
    for (int t = 0; t < D && dropped + mag[t] <= -thr * total; ++t) {
        dropped += mag[t];
        cut = mag[t];
    }
    // (taps EQUAL to the largest dropped magnitude: keep the bound -- drop them only if all fit)
    auto at_or_below = [&](double m) {
        double s = 0.0;
        for (int t = 0; t < D; ++t)
            if (std::fabs(lsf[t]) <= m) s += std::fabs(lsf[t]);
        return s;
    };
    while (at_or_below(cut) > -thr * total && cut > 0.0) {  // shrink to the next smaller magnitude
        double next = 0.0;
        for (int t = 0; t < D; ++t)
            if (mag[t] < cut) next = std::fmax(next, mag[t]);
        cut = next;
    }
    return cut;
}

// fsf: [fh][fw]; lsf: [D] or NULL; N: the padded length of the reference's spectral convolution;
// HL: lanes a spectrum takes; flow_grid: 4 workgroups per compute unit (0: 1024); LSF_RL: the
// reach of the dense form; thr: lsf_cut's; spatial_sep, march_hy_opt: the options.
inline Result analyse(int fh, int fw, int D, int N, int H, int W, int HL, int flow_grid, int LSF_RL, const double *fsf,
                      const double *lsf, double thr, int spatial_sep, int march_hy_opt) {
    Result r;
    auto mirrored = [&](bool in_x) {
        for (int k = 0; k < fh; ++k)
            for (int i = 0; i < fw; ++i)
                if (fsf[k * fw + i] != (in_x ? fsf[k * fw + (fw - 1 - i)] : fsf[(fh - 1 - k) * fw + i])) return false;
        return true;
    };
    r.symx = mirrored(true);
    r.symy = mirrored(false);
    // outer product?  u = centre column / centre tap, v = centre row
    {
        const int cy = (fh - 1) / 2, cx = (fw - 1) / 2;
        const double cc = fsf[cy * fw + cx];
        double amax = 0.0;
        for (int i = 0; i < fh * fw; ++i) amax = std::max(amax, std::fabs(fsf[i]));
        std::vector<double> uv((size_t)fh + fw);
        bool sep = cc != 0.0 && amax > 0.0;
        if (sep) {
            for (int k = 0; k < fh; ++k) uv[k] = fsf[k * fw + cx] / cc;
            for (int m = 0; m < fw; ++m) uv[fh + m] = fsf[cy * fw + m];
            for (int k = 0; k < fh && sep; ++k)
                for (int m = 0; m < fw; ++m)
                    if (!(std::fabs(fsf[k * fw + m] - uv[k] * uv[fh + m]) <= 8.0 * 2.220446049250313e-16 * amax)) {
                        sep = false;
                        break;
                    }
        }
        r.sep = sep && spatial_sep != 0;
        if (r.sep) r.uv = uv;
    }
    if (r.symx && r.symy && fh == fw) {
        // quadrant taps by distance from the centre (k_conv_rows)
        const int fhh = (fh - 1) / 2, nq = fhh + 1;
        r.quad.resize((size_t)nq * nq);
        r.symt = true;
        for (int a = 0; a < nq; ++a)
            for (int m = 0; m < nq; ++m) {
                r.quad[(size_t)a * nq + m] = fsf[(fhh - a) * fw + (fhh - m)];
                r.symt = r.symt && fsf[(fhh - a) * fw + (fhh - m)] == fsf[(fhh - m) * fw + (fhh - a)];
            }
        if (r.sep && nq >= 2) {  // (a 1 x 1 FSF: the table has no second row, and no kernel reads one)
            r.quad_sep.assign((size_t)nq * nq, 0.0);
            const double cc = fsf[fhh * fw + fhh];
            for (int e = 0; e < nq; ++e) r.quad_sep[e] = fsf[fhh * fw + (fhh - e)];
            for (int a = 0; a < nq; ++a) r.quad_sep[(size_t)nq + a] = fsf[(fhh - a) * fw + fhh] / cc;
        }
    }
    // Rows per strip of the march kernels: a strip is one wavefront's worth of z
    // (64 / HL strips per wavefront when the spectrum is shorter), the chip holds
    // two such wavefronts per SIMD, and a strip costs HY + FS - 1 row steps.  Take
    // the HY in 12..20 that needs the fewest rounds of wavefronts and, among those,
    // the fewest steps (300 rows: 15 -> 20 strips of 25 steps, all resident at once;
    // 16 -> 19 strips of 26 steps).
    {
        const int TX = (fw >= 9 ? 3 : 4);
        const long slots = 2L * (flow_grid > 0 ? flow_grid : 1024);  // 8 wavefronts per CU
        const int per_wave = HL >= 64 ? 1 : 64 / (HL > 0 ? HL : 1);
        long best_cost = -1;
        for (int hy = 12; hy <= 20; ++hy) {
            const long strips = (long)((W + TX - 1) / TX) * ((H + hy - 1) / hy);
            const long waves = (strips + per_wave - 1) / per_wave;
            const long cost = ((waves + slots - 1) / slots) * (hy + fh - 1);
            if (best_cost < 0 || cost <= best_cost) {
                best_cost = cost;
                r.march_hy = hy;
            }
        }
        if (march_hy_opt >= 1) r.march_hy = march_hy_opt;
    }
    r.dense.assign((size_t)2 * LSF_RL + 1, 0.0);
    if (!lsf) return r;
    // closed form of convolve_1d: lib/convolution.py:89-160, SURVEY 8(a) a3
    const int diff = N - D;
    const int h = (diff & 1) ? diff / 2 + 1 : diff / 2;  // lib/convolution.py:149-153
    const double cut = lsf_cut(lsf, D, thr);
    for (int t = 0; t < D; ++t) {
        if (!(std::fabs(lsf[t]) > cut)) continue;
        int s = (N / 2 - h - t) % N;
        if (s < 0) s += N;
        r.shift.push_back(s);
        r.weight.push_back(lsf[t]);
    }
    r.lsf_empty = r.shift.empty();
    if (r.lsf_empty) return r;
    // the dense form: one vector, admitted at any depth (dense_any) or only where N == D (dense_ok)
    bool fits = N >= 4 * LSF_RL;
    for (size_t t = 0; fits && t < r.shift.size(); ++t) {
        const int sg = r.shift[t] > N / 2 ? r.shift[t] - N : r.shift[t];
        if (sg < -LSF_RL || sg > LSF_RL) fits = false;
        else r.dense[sg + LSF_RL] += r.weight[t];
    }
    if (!fits) {
        std::fill(r.dense.begin(), r.dense.end(), 0.0);
        return r;
    }
    r.dense_any = true;
    r.dense_ok = N == D;
    r.dense_sym = true;
    for (int j = 0; j < LSF_RL; ++j) r.dense_sym = r.dense_sym && r.dense[j] == r.dense[2 * LSF_RL - j];
    // wave-private LDS forms additionally need the spectrum within one wavefront
    r.fusable = r.dense_ok && HL <= 64 && 64 % HL == 0;
    return r;
}

}  // namespace d3d_taps
