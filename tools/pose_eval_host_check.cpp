// Host build of csrc/pose_eval.h: every candidate of the test shapes (B = 2, 3, 4, 9, 10, 12, 64; exact, noisy, coincident and identity
// poses) through pe_candidate / pe_choose / pe_similarity / pe_align / pe_backtrack, against a direct restatement that works on 4 x 4
// matrices as joint_pose_nerf_trainer.py:173-213 does, with every index checked to stay inside B and P.  Plain C++, no HIP:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I sparf_amd/csrc tools/pose_eval_host_check.cpp -o pose_eval_host_check
//   ./pose_eval_host_check        (exit code 0 and "pose_eval_host_check: ok" when every check holds)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define POSE_DEV inline
#include "pose_eval.h"

using namespace sparf;

static int failures = 0;
static void expect(bool ok, const char* what, double got, double want) {
    if (!ok) {
        std::printf("FAIL %s: got %.17g want %.17g\n", what, got, want);
        ++failures;
    }
}
static bool same(double a, double b, double tol) { return (a != a && b != b) || a == b || fabs(a - b) <= tol * (1.0 + fabs(b)); }

static unsigned lcg_state = 1u;
static double uniform() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (double)(lcg_state >> 8) / 16777216.0 * 2.0 - 1.0;
}
// Rodrigues
static void rotation(const double w[3], double R[9]) {
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    const double a = th < 1e-12 ? 1.0 : sin(th) / th, b = th < 1e-12 ? 0.5 : (1 - cos(th)) / (th * th);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0;
            for (int k = 0; k < 3; ++k) kk += K[i * 3 + k] * K[k * 3 + j];
            R[i * 3 + j] = (i == j) + a * K[i * 3 + j] + b * kk;
        }
}
// world-to-camera [R^T | -R^T c] of a camera-to-world rotation and centre, rounded to float
static void w2c_of(const double R[9], const double c[3], float out[12]) {
    for (int i = 0; i < 3; ++i) {
        double t = 0;
        for (int j = 0; j < 3; ++j) {
            out[i * 4 + j] = (float)R[j * 3 + i];
            t -= R[j * 3 + i] * c[j];
        }
        out[i * 4 + 3] = (float)t;
    }
}

struct Set {
    int B;
    std::vector<float> pose, gt;
};
enum Kind { NOISY, EXACT, COINCIDENT, IDENTITY };
static Set make(int B, Kind kind, double noise, unsigned seed) {
    lcg_state = seed;
    Set s{B, std::vector<float>((size_t)B * 12), std::vector<float>((size_t)B * 12)};
    double ws[3] = {uniform(), uniform(), uniform()}, Rs[9], ts[3] = {uniform(), uniform(), uniform()};
    rotation(ws, Rs);
    const double sc = exp(0.7 * uniform());
    for (int i = 0; i < B; ++i) {
        double w[3] = {2 * uniform(), 2 * uniform(), 2 * uniform()}, R[9], c[3] = {3 * uniform(), 3 * uniform(), 3 * uniform()};
        rotation(w, R);
        w2c_of(R, c, &s.gt[(size_t)i * 12]);
        double wn[3] = {noise * uniform(), noise * uniform(), noise * uniform()}, Rn[9], Re[9], ce[3], cn[3];
        rotation(wn, Rn);
        for (int k = 0; k < 3; ++k) cn[k] = c[k] + (kind == EXACT ? 0.0 : noise * uniform()) - ts[k];
        for (int r = 0; r < 3; ++r) {
            ce[r] = (Rs[r] * cn[0] + Rs[3 + r] * cn[1] + Rs[6 + r] * cn[2]) / sc;
            for (int q = 0; q < 3; ++q) {
                double rn = 0, acc = 0;
                for (int k = 0; k < 3; ++k) {
                    rn = 0;
                    for (int m = 0; m < 3; ++m) rn += R[k * 3 + m] * (kind == EXACT ? (m == q) : Rn[m * 3 + q]);
                    acc += Rs[k * 3 + r] * rn;
                }
                Re[r * 3 + q] = acc;
            }
        }
        w2c_of(Re, ce, &s.pose[(size_t)i * 12]);
    }
    if (kind == COINCIDENT)
        for (int k = 0; k < 12; ++k) s.pose[12 + k] = s.pose[k];
    if (kind == IDENTITY)
        for (int i = 0; i < B; ++i)
            for (int k = 0; k < 12; ++k) s.pose[(size_t)i * 12 + k] = (k == 0 || k == 5 || k == 10) ? 1.0f : 0.0f;
    return s;
}

// ---- the direct restatement: 4 x 4 matrices as the reference pads them
struct M4 {
    double m[16];
};
static M4 pad(const double p[12]) {
    M4 r;
    for (int k = 0; k < 12; ++k) r.m[k] = p[k];
    r.m[12] = r.m[13] = r.m[14] = 0.0;
    r.m[15] = 1.0;
    return r;
}
static M4 mul(const M4& a, const M4& b) {
    M4 r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) acc += a.m[i * 4 + k] * b.m[k * 4 + j];
            r.m[i * 4 + j] = acc;
        }
    return r;
}
static M4 inverse(const M4& a) {             // camera.py:37-59
    M4 r;
    for (int k = 0; k < 16; ++k) r.m[k] = 0.0;
    r.m[15] = 1.0;
    for (int i = 0; i < 3; ++i) {
        double t = 0.0;
        for (int j = 0; j < 3; ++j) {
            r.m[i * 4 + j] = a.m[j * 4 + i];
            t += (-a.m[j * 4 + i]) * a.m[j * 4 + 3];
        }
        r.m[i * 4 + 3] = t;
    }
    return r;
}
static void direct_errors(const M4& c2w, const M4& gt, double& eR, double& et) {
    double tr = 0.0, d2 = 0.0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) tr += c2w.m[i * 4 + j] * gt.m[i * 4 + j];
        d2 += (c2w.m[i * 4 + 3] - gt.m[i * 4 + 3]) * (c2w.m[i * 4 + 3] - gt.m[i * 4 + 3]);
    }
    const double c = (double)(float)(1.0 - 1e-7);
    double x = (tr - 1.0) / 2.0;
    x = x < -c ? -c : (x > c ? c : x);
    eR = acos(x);
    et = sqrt(d2);
}
static void direct_candidate(const std::vector<M4>& from, const std::vector<M4>& to, int a, int b, double score[3], std::vector<M4>* aligned_w2c, M4* T_out,
                             double* scale_out) {
    const int B = (int)from.size();
    double df = 0.0, dt = 0.0;
    for (int i = 0; i < 3; ++i) {
        df += (from[a].m[i * 4 + 3] - from[b].m[i * 4 + 3]) * (from[a].m[i * 4 + 3] - from[b].m[i * 4 + 3]);
        dt += (to[a].m[i * 4 + 3] - to[b].m[i * 4 + 3]) * (to[a].m[i * 4 + 3] - to[b].m[i * 4 + 3]);
    }
    const double scale = sqrt(dt) / sqrt(df);
    std::vector<M4> scaled(from);
    for (M4& s : scaled)
        for (int i = 0; i < 3; ++i) s.m[i * 4 + 3] *= scale;
    const M4 T = mul(to[a], inverse(scaled[a]));
    double sR = 0.0, st = 0.0;
    for (int i = 0; i < B; ++i) {
        const M4 w2c = inverse(mul(T, scaled[i]));
        if (aligned_w2c) (*aligned_w2c)[i] = w2c;
        double eR, et;
        direct_errors(inverse(w2c), to[i], eR, et);
        sR += eR;
        st += et;
    }
    score[0] = sR / B * 180. / 3.141592653589793;
    score[1] = st / B;
    score[2] = score[1] * score[0];
    if (T_out) *T_out = T;
    if (scale_out) *scale_out = scale;
}

static void check_set(const Set& s, const char* what, int want_nan_first) {
    const int B = s.B, n = B < PE_MAX_VIEWS ? B : PE_MAX_VIEWS, P = n * (n - 1);
    expect(B <= PE_MAX_POSES && P <= PE_MAX_PAIRS, "sizes", B, P);
    std::vector<double> c2w((size_t)B * 12), gt_c2w((size_t)B * 12), score((size_t)P * 3);
    std::vector<M4> from(B), to(B);
    for (int i = 0; i < B; ++i) {
        double p[12];
        load12(&s.pose[(size_t)i * 12], p);
        pe_invert(p, &c2w[(size_t)i * 12]);
        from[i] = inverse(pad(p));
        load12(&s.gt[(size_t)i * 12], p);
        pe_invert(p, &gt_c2w[(size_t)i * 12]);
        to[i] = inverse(pad(p));
        for (int k = 0; k < 12; ++k) expect(same(c2w[(size_t)i * 12 + k], from[i].m[k], 0.0), "invert", c2w[(size_t)i * 12 + k], from[i].m[k]);
    }
    std::vector<char> seen((size_t)n * n, 0);
    int prev = -1;
    for (int p = 0; p < P; ++p) {
        int a, b;
        pe_pair(p, n, a, b);
        expect(a >= 0 && a < n && b >= 0 && b < n && a != b, "pair inside n", a, b);
        expect(a * n + b > prev && !seen[(size_t)a * n + b], "pair order", a * n + b, prev);        // a outermost, b ascending, each once
        prev = a * n + b;
        seen[(size_t)a * n + b] = 1;
        pe_candidate(c2w.data(), gt_c2w.data(), B, a, b, &score[(size_t)p * 3]);
        double want[3];
        direct_candidate(from, to, a, b, want, nullptr, nullptr, nullptr);
        // (another operation order: 1e-16 on the trace is 2e-13 rad behind acos at the clamp, 1e-11 degrees)
        for (int k = 0; k < 3; ++k) expect(same(score[(size_t)p * 3 + k], want[k], 1e-9), what, score[(size_t)p * 3 + k], want[k]);
    }
    const int best = pe_choose(score.data() + 2, P);
    expect(best >= 0 && best < P, "choice inside P", best, P);
    int want_best = 0;                       // np.argmin: the first NaN, otherwise the first minimum
    bool nan_seen = false;
    for (int p = 0; p < P && !nan_seen; ++p) {
        const double v = score[(size_t)p * 3 + 2];
        if (v != v) {
            want_best = p;
            nan_seen = true;
        } else if (v < score[(size_t)want_best * 3 + 2]) {
            want_best = p;
        }
    }
    expect(best == want_best, "choice", best, want_best);
    if (want_nan_first >= 0) expect(best == want_nan_first && nan_seen, "NaN first", best, want_nan_first);
    // the chosen candidate's similarity and poses, and the backtrack of the ground truth under it
    int a, b;
    pe_pair(best, n, a, b);
    double T[12], scale, want_score[3], want_scale;
    std::vector<M4> want_aligned(B);
    M4 want_T;
    pe_similarity(c2w.data(), gt_c2w.data(), a, b, T, scale);
    direct_candidate(from, to, a, b, want_score, &want_aligned, &want_T, &want_scale);
    expect(same(scale, want_scale, 1e-14), "scale", scale, want_scale);
    for (int k = 0; k < 12; ++k) expect(same(T[k], want_T.m[k], 1e-12), "T", T[k], want_T.m[k]);
    double sim[PE_SIM3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) sim[i * 3 + j] = T[i * 4 + j];
        sim[9 + i] = T[i * 4 + 3];
    }
    sim[12] = scale;
    for (int i = 0; i < B; ++i) {
        double al[12], eR, et, gt_w2c[12], back[12];
        pe_align(T, scale, &c2w[(size_t)i * 12], al);
        for (int k = 0; k < 12; ++k) expect(same(al[k], want_aligned[i].m[k], 1e-11), "aligned", al[k], want_aligned[i].m[k]);
        pe_aligned_errors(al, &gt_c2w[(size_t)i * 12], eR, et);
        // the anchor view is aligned exactly: on the clamp floor, or just above it where its fp32 rotation is short of orthonormal
        if (i == a && std::isfinite(scale)) expect(eR >= acos(pe_clamp_bound()) && eR < 1e-3, "the anchor view sits at the clamp floor", eR, acos(pe_clamp_bound()));
        // backtrack inverts the alignment up to what the fp32 rotations lack of orthonormality (it transposes where an inverse is meant)
        load12(&s.gt[(size_t)i * 12], gt_w2c);
        pe_backtrack(gt_w2c, sim, back);
        double again[12], c_back[12];
        pe_invert(back, c_back);
        pe_align(T, scale, c_back, again);
        if (std::isfinite(scale) && scale > 0)
            for (int k = 0; k < 12; ++k) expect(same(again[k], gt_w2c[k], 5e-6), "backtrack then align", again[k], gt_w2c[k]);
    }
}

int main() {
    expect(pe_clamp_bound() == (double)0.99999988079071044921875, "clamp bound", pe_clamp_bound(), 0.99999988079071044921875);
    expect(fabs(acos(pe_clamp_bound()) - 4.8828125e-4) < 1e-10, "clamp floor", acos(pe_clamp_bound()), 4.8828125e-4);
    const int sizes[] = {2, 3, 4, 9, 10, 12, 64};
    unsigned seed = 7;
    for (int B : sizes) {
        for (double noise : {1e-3, 0.05, 0.3}) check_set(make(B, NOISY, noise, seed++), "noisy", -1);
        check_set(make(B, EXACT, 0.0, seed++), "exact", -1);
    }
    check_set(make(3, COINCIDENT, 0.05, seed++), "coincident", 0);
    check_set(make(3, IDENTITY, 0.05, seed++), "identity", 0);
    check_set(make(9, IDENTITY, 0.05, seed++), "identity", 0);
    // one rotation by pi: the lower clamp
    double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, half[12] = {-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0};
    expect(pe_rotation_distance(I, half) == acos(-pe_clamp_bound()), "lower clamp", pe_rotation_distance(I, half), acos(-pe_clamp_bound()));
    double nan_pose[12];
    for (double& v : nan_pose) v = NAN;
    expect(std::isnan(pe_rotation_distance(I, nan_pose)), "a NaN passes the clamp", pe_rotation_distance(I, nan_pose), NAN);
    if (failures) {
        std::printf("pose_eval_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("pose_eval_host_check: ok\n");
    return 0;
}
