// CPU test of csrc/sift_desc_rows.h: the exact row intervals the descriptor
// kernels enumerate.  For every job (a keypoint's window geometry) and every
// window row, desc_row_interval must return exactly the set of samples that
// pass the oracle's per-sample test -- calcSIFTDescriptor's, restated below as
// descriptor.hip's desc_sample states it -- found by brute force over
// j in [-R-4, R+4].  The kernels drop the per-sample test and the bin clamps
// for enumerated samples, so a sample too many is an LDS add outside the
// histogram and a sample too few a wrong descriptor.
//
// Build: g++ -std=c++17 -O2 -ffp-contract=off (the products and sums must
// round separately, as in the kernels).  No GPU.  Prints one summary line;
// exit status 1 on the first mismatch.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sift_desc_rows.h"

namespace {

constexpr int kD = 4;

struct Job {
    float cos_t, sin_t;  // cos / hist_width, sin / hist_width
    int ptx, pty, rows, cols, radius;
};

// descriptor.hip desc_sample: the oracle's loop body and test.
bool oracle_accepts(const Job& g, int i, int j) {
    const float c_rot = (float)j * g.cos_t - (float)i * g.sin_t;
    const float r_rot = (float)j * g.sin_t + (float)i * g.cos_t;
    const float rbin = r_rot + (float)(kD / 2) - 0.5f;
    const float cbin = c_rot + (float)(kD / 2) - 0.5f;
    const int r = g.pty + i, c = g.ptx + j;
    return rbin > -1 && rbin < kD && cbin > -1 && cbin < kD && r > 0 && r < g.rows - 1 && c > 0 && c < g.cols - 1;
}

float ulps(float x, int n) {
    for (int k = 0; k < std::abs(n); k++) x = std::nextafterf(x, n > 0 ? INFINITY : -INFINITY);
    return x;
}

struct Stats {
    long jobs = 0, rows = 0, nonempty = 0, samples = 0, conservative = 0;
    int max_trim_lo = 0, max_trim_hi = 0;
};

// One job, every row, with the reciprocals off by `inv_ulps` (the kernels use
// the hardware's approximate reciprocal, 1 ulp).
bool check(const Job& g, int inv_ulps, Stats& st) {
    const int R = g.radius;
    const float inv_cos = ulps(1.f / g.cos_t, inv_ulps), inv_sin = ulps(1.f / g.sin_t, -inv_ulps);
    for (int i = -R; i <= R; i++) {
        // the kernels' image clipping (descriptor.hip desc_row)
        const int r = g.pty + i;
        int lo0 = std::max(-R, 1 - g.ptx), hi0 = std::min(R, g.cols - 2 - g.ptx);
        if (r <= 0 || r >= g.rows - 1) hi0 = lo0 - 1;
        int clo = lo0, chi = hi0;
        sift_amd::desc_row_conservative(clo, chi, i, g.cos_t, g.sin_t, inv_cos, inv_sin, R);
        int lo = lo0, hi = hi0;
        sift_amd::desc_row_interval(lo, hi, i, g.cos_t, g.sin_t, inv_cos, inv_sin, R);
        // brute force
        int first = 0, last = -1, count = 0;
        for (int j = -R - 4; j <= R + 4; j++) {
            if (j < -R || j > R || !oracle_accepts(g, i, j)) continue;
            if (!count) first = j;
            last = j;
            count++;
        }
        const int len = std::max(hi - lo + 1, 0), clen = std::max(chi - clo + 1, 0);
        bool ok = len == count && (count == 0 || (lo == first && hi == last && last - first + 1 == count));
        // the trims stay inside the conservative interval
        if (len > 0) ok = ok && lo >= clo && hi <= chi;
        ok = ok && len <= clen;
        if (!ok) {
            std::printf("MISMATCH cos_t=%a sin_t=%a ptx=%d pty=%d rows=%d cols=%d R=%d i=%d inv_ulps=%d: interval [%d, %d] "
                        "conservative [%d, %d] brute force [%d, %d] count %d\n",
                        g.cos_t, g.sin_t, g.ptx, g.pty, g.rows, g.cols, R, i, inv_ulps, lo, hi, clo, chi, first, last,
                        count);
            return false;
        }
        st.rows++;
        st.samples += len;
        st.conservative += clen;
        if (len > 0) {
            st.nonempty++;
            st.max_trim_lo = std::max(st.max_trim_lo, lo - clo);
            st.max_trim_hi = std::max(st.max_trim_hi, chi - hi);
        }
    }
    st.jobs++;
    return true;
}

Job make(float angle_deg, float hist_width, int ptx, int pty, int rows, int cols, int radius) {
    // OpenCV: cos_t = cosf(ori * pi / 180) / hist_width
    const float a = angle_deg * (float)(M_PI / 180);
    return Job{std::cos(a) / hist_width, std::sin(a) / hist_width, ptx, pty, rows, cols, radius};
}

// calcSIFTDescriptor's radius: the window's half diagonal, at most the plane's diagonal.
int natural_radius(float hist_width, int rows, int cols) {
    const int r = (int)std::lround(hist_width * 1.4142135623730951f * (kD + 1) * 0.5f);
    return std::max(1, std::min({r, (int)std::sqrt((double)rows * rows + (double)cols * cols), 63}));
}

}  // namespace

int main() {
    std::mt19937 rng(20240607);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    auto uin = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
    std::vector<Job> jobs;
    const float axes[] = {0.f, 90.f, 180.f, 270.f, 45.f, 360.f, 135.f, 225.f, 315.f};
    // 1. random angle and hist_width 1.5-25 on planes that hold the window or cut it
    for (int n = 0; n < 9000; n++) {
        const int rows = uin(5, 300), cols = uin(6, 300);
        const float hw = uni(1.5f, 25.f);
        jobs.push_back(make(uni(0.f, 360.f), hw, uin(-4, cols + 3), uin(-4, rows + 3), rows, cols,
                            natural_radius(hw, rows, cols)));
    }
    // 2. the axis angles and 45 degrees, exactly; cos_t = +-0 and +-1 / hist_width exactly as well
    for (int n = 0; n < 4000; n++) {
        const int rows = uin(5, 200), cols = uin(6, 200);
        const float hw = uni(1.5f, 25.f);
        Job j = make(axes[n % 9], hw, uin(-2, cols + 1), uin(-2, rows + 1), rows, cols, natural_radius(hw, rows, cols));
        if (n % 18 >= 9) {  // exact zeros instead of cosf(pi / 2)'s 1e-8
            const int q = n % 4;
            j.cos_t = (q == 0 ? 1.f : q == 2 ? -1.f : 0.f) / hw;
            j.sin_t = (q == 1 ? 1.f : q == 3 ? -1.f : 0.f) / hw;
        }
        jobs.push_back(j);
    }
    // 3. keypoints within 2 px of each border and corner
    for (int n = 0; n < 4000; n++) {
        const int rows = uin(20, 200), cols = uin(20, 200);
        const float hw = uni(1.5f, 25.f);
        const int side = n % 8;
        int x = uin(0, cols - 1), y = uin(0, rows - 1);
        const int near_lo = uin(-2, 2), near_hi = uin(-2, 2);
        if (side == 0 || side == 4 || side == 6) x = near_lo;
        if (side == 1 || side == 5 || side == 7) x = cols - 1 + near_hi;
        if (side == 2 || side == 4 || side == 5) y = near_lo;
        if (side == 3 || side == 6 || side == 7) y = rows - 1 + near_hi;
        jobs.push_back(make(n % 3 ? uni(0.f, 360.f) : axes[n % 9], hw, x, y, rows, cols, natural_radius(hw, rows, cols)));
    }
    // 4. planes as small as 6 x 5
    for (int n = 0; n < 2000; n++) {
        const int rows = uin(5, 12), cols = uin(6, 14);
        const float hw = uni(1.5f, 25.f);
        jobs.push_back(make(n % 4 ? uni(0.f, 360.f) : axes[n % 9], hw, uin(-2, cols + 1), uin(-2, rows + 1), rows, cols,
                            natural_radius(hw, rows, cols)));
    }
    // 5. every radius 1 .. 63, with the hist_width that gives it and with unrelated ones
    for (int R = 1; R <= 63; R++)
        for (int n = 0; n < 24; n++) {
            const float hw = n % 2 ? uni(1.5f, 25.f) : std::max(0.3f, R / (1.4142135623730951f * 2.5f) + uni(-0.1f, 0.1f));
            const int rows = uin(5, 260), cols = uin(6, 260);
            jobs.push_back(make(n % 5 ? uni(0.f, 360.f) : axes[n % 9], hw, uin(0, cols - 1), uin(0, rows - 1), rows, cols, R));
        }
    Stats st;
    for (const Job& j : jobs)
        for (int u : {0, 2, -2}) {
            Stats one;
            if (!check(j, u, one)) return 1;
            if (u == 0) {
                st.jobs += one.jobs, st.rows += one.rows, st.nonempty += one.nonempty, st.samples += one.samples;
                st.conservative += one.conservative;
            }
            st.max_trim_lo = std::max(st.max_trim_lo, one.max_trim_lo);
            st.max_trim_hi = std::max(st.max_trim_hi, one.max_trim_hi);
        }
    std::printf("ok jobs=%ld rows=%ld nonempty=%ld samples=%ld conservative=%ld max_trim_lo=%d max_trim_hi=%d\n", st.jobs,
                st.rows, st.nonempty, st.samples, st.conservative, st.max_trim_lo, st.max_trim_hi);
    return 0;
}
