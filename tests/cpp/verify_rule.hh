// The two-view verification rule of include/sift_hip.h restated in plain C++
// (tests/cpp/test_verify.cpp).  Compile with -ffp-contract=off: the rule is
// float32, one rounded operation at a time, nothing fused.
#pragma once

#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "sift_cuda/Types.hh"

namespace verify_rule {

inline uint32_t mix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

// sample[0..7] of hypothesis k (n >= 8).
inline void draw(uint32_t seed, int k, int n, int* sample) {
    const uint32_t base = mix(seed ^ mix((uint32_t)k));
    for (int j = 0; j < 8; j++) {
        const uint32_t h = mix(base + 0x9e3779b9u * (uint32_t)(j + 1));
        int r = (int)(((uint64_t)h * (uint64_t)(n - j)) >> 32);
        // past the earlier picks in ascending order
        bool used[8] = {false, false, false, false, false, false, false, false};
        for (int step = 0; step < j; step++) {
            int lo = -1;
            for (int i = 0; i < j; i++)
                if (!used[i] && (lo < 0 || sample[i] < sample[lo])) lo = i;
            used[lo] = true;
            if (r >= sample[lo]) r++;
        }
        sample[j] = r;
    }
}

struct Side {
    float x[8], y[8], s, ox, oy;
};

inline void normalise(Side& p) {
    float sx = p.x[0], sy = p.y[0];
    for (int i = 1; i < 8; i++) sx = sx + p.x[i], sy = sy + p.y[i];
    const float mx = sx / 8.0f, my = sy / 8.0f;
    float d[8];
    for (int i = 0; i < 8; i++) {
        p.x[i] = p.x[i] - mx;
        p.y[i] = p.y[i] - my;
        d[i] = std::sqrt(p.x[i] * p.x[i] + p.y[i] * p.y[i]);
    }
    float sd = d[0];
    for (int i = 1; i < 8; i++) sd = sd + d[i];
    const float md = sd / 8.0f;
    p.s = 1.41421354f / md;
    for (int i = 0; i < 8; i++) p.x[i] = p.x[i] * p.s, p.y[i] = p.y[i] * p.s;
    p.ox = -(p.s * mx);
    p.oy = -(p.s * my);
}

// pts: (qx, qy, tx, ty) per match.  False (and F zero) for an invalid hypothesis.
inline bool solve(const float* pts, const int* sample, float* F) {
    for (int i = 0; i < 9; i++) F[i] = 0.f;
    Side q, t;
    for (int i = 0; i < 8; i++) {
        const float* p = pts + 4 * (size_t)sample[i];
        q.x[i] = p[0], q.y[i] = p[1], t.x[i] = p[2], t.y[i] = p[3];
    }
    normalise(q);
    normalise(t);
    float A[8][9];
    int perm[9];
    for (int r = 0; r < 8; r++) {
        const float row[9] = {t.x[r] * q.x[r], t.x[r] * q.y[r], t.x[r], t.y[r] * q.x[r], t.y[r] * q.y[r],
                              t.y[r],          q.x[r],          q.y[r], 1.0f};
        for (int c = 0; c < 9; c++) A[r][c] = row[c];
    }
    for (int c = 0; c < 9; c++) perm[c] = c;
    for (int c = 0; c < 8; c++) {
        float best = std::fabs(A[c][c]);
        int pr = c, pc = c;
        for (int r = c; r < 8; r++)
            for (int j = c; j < 9; j++)
                if (std::fabs(A[r][j]) > best) best = std::fabs(A[r][j]), pr = r, pc = j;
        for (int j = 0; j < 9; j++) std::swap(A[c][j], A[pr][j]);
        for (int r = 0; r < 8; r++) std::swap(A[r][c], A[r][pc]);
        std::swap(perm[c], perm[pc]);
        const float p = A[c][c];
        if (p == 0.f || !std::isfinite(p)) return false;
        for (int r = c + 1; r < 8; r++) {
            const float m = A[r][c] / p;
            for (int j = c + 1; j < 9; j++) A[r][j] = A[r][j] - m * A[c][j];
        }
    }
    float y[9], g[9];
    y[8] = 1.0f;
    for (int i = 7; i >= 0; i--) {
        float acc = A[i][i + 1] * y[i + 1];
        for (int j = i + 2; j < 9; j++) acc = acc + A[i][j] * y[j];
        y[i] = (-acc) / A[i][i];
    }
    for (int j = 0; j < 9; j++) g[perm[j]] = y[j];
    float H[9], E[9];
    for (int r = 0; r < 3; r++) {
        H[3 * r] = g[3 * r] * q.s;
        H[3 * r + 1] = g[3 * r + 1] * q.s;
        H[3 * r + 2] = (g[3 * r] * q.ox + g[3 * r + 1] * q.oy) + g[3 * r + 2];
    }
    for (int c = 0; c < 3; c++) {
        E[c] = t.s * H[c];
        E[3 + c] = t.s * H[3 + c];
        E[6 + c] = (t.ox * H[c] + t.oy * H[3 + c]) + H[6 + c];
    }
    float ss = E[0] * E[0];
    for (int i = 1; i < 9; i++) ss = ss + E[i] * E[i];
    const float nrm = std::sqrt(ss);
    bool ok = true;
    for (int i = 0; i < 9; i++) {
        E[i] = E[i] / nrm;
        ok = ok && std::isfinite(E[i]);
    }
    if (!ok) return false;
    for (int i = 0; i < 9; i++) F[i] = E[i];
    return true;
}

inline bool inlier(const float* F, float max_error, const float* p) {
    const float qx = p[0], qy = p[1], tx = p[2], ty = p[3];
    const float a = (F[0] * qx + F[1] * qy) + F[2];
    const float b = (F[3] * qx + F[4] * qy) + F[5];
    const float c = (F[6] * qx + F[7] * qy) + F[8];
    const float nq = a * a + b * b;
    const float u = (F[0] * tx + F[3] * ty) + F[6];
    const float v = (F[1] * tx + F[4] * ty) + F[7];
    const float nr = u * u + v * v;
    const float r = (a * tx + b * ty) + c;
    const float e2 = max_error * max_error;
    const float inf = INFINITY;
    return r * r <= e2 * (nq + nr) && std::fabs(tx - qx) <= inf && std::fabs(ty - qy) <= inf;
}

struct Result {
    float F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int hypothesis = -1, inliers = 0, valid = 0;
    std::vector<sift_cuda::DMatch> list;
};

// The whole operation on host arrays: positions as rows of `stride` floats.
inline Result ransac(const std::vector<sift_cuda::DMatch>& m, const float* qxy, int qstride, int nq, const float* txy,
                     int tstride, int nt, int K, uint32_t seed, float max_error) {
    const int n = (int)m.size();
    std::vector<float> pts(4 * (size_t)n);
    for (int j = 0; j < n; j++) {
        const bool ok = m[j].queryIdx >= 0 && m[j].queryIdx < nq && m[j].trainIdx >= 0 && m[j].trainIdx < nt;
        float row[4] = {NAN, NAN, NAN, NAN};
        if (ok) {  // a record outside its position array is never read through
            const float* q = qxy + (size_t)m[j].queryIdx * qstride;
            const float* t = txy + (size_t)m[j].trainIdx * tstride;
            row[0] = q[0], row[1] = q[1], row[2] = t[0], row[3] = t[1];
        }
        for (int i = 0; i < 4; i++) pts[4 * (size_t)j + i] = row[i];
    }
    Result best;
    if (n < 8) return best;
    for (int k = 0; k < K; k++) {
        int sample[8];
        float F[9];
        draw(seed, k, n, sample);
        if (!solve(pts.data(), sample, F)) continue;
        best.valid++;
        int count = 0;
        for (int j = 0; j < n; j++) count += inlier(F, max_error, &pts[4 * (size_t)j]) ? 1 : 0;
        if (best.hypothesis < 0 || count > best.inliers) {
            best.hypothesis = k;
            best.inliers = count;
            for (int i = 0; i < 9; i++) best.F[i] = F[i];
        }
    }
    if (best.hypothesis >= 0)
        for (int j = 0; j < n; j++)
            if (inlier(best.F, max_error, &pts[4 * (size_t)j])) best.list.push_back(m[j]);
    return best;
}

}  // namespace verify_rule
