// Host build of csrc/pick.h: the pixel and the ray of EVERY output row of the test shapes (tests/pick_referee.py: images of 7 x 9,
// 12 x 10 and 19 x 21, 1, 5 and 300 picks, a centre share of 0 and 0.4, patches of 1, 2 and 3) against a direct serial restatement, with
// permutations and outputs allocated to their exact sizes; permutation entries of -1, the pool size, INT64_MAX and INT64_MIN, which must
// be clamped into the pool and leave every pixel inside the image; and the pose arithmetic for 1, 2, 3, 6 and 70 cameras -- the search
// in strides of 64 as the kernel's lanes run it against one serial pass, the first index among equal distances, one camera alone, a
// camera at the scene centre (the zero vector: pi / 2 by the formula) and every matrix entry against double arithmetic within the bound
// of its float32 roundings.  Plain C++, no HIP:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I sparf_amd/csrc tools/pick_host_check.cpp -o pick_host_check
//   ./pick_host_check        (exit code 0 and "pick_host_check: ok" when every check holds)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pick.h"

using namespace sparf;

static int failures = 0;
static void expect(bool ok, const char* what, double got, double want, int shape, int at) {
    if (!ok && ++failures <= 20) std::printf("FAIL %s in case %d at %d: got %.17g want %.17g\n", what, shape, at, got, want);
}

static unsigned lcg(unsigned& s) { return s = s * 1664525u + 1013904223u; }

// ---- pixels
static void centre_box(int H, int W, int& x0, int& y0, int& w, int& h) {
    const int dH = (int)(H / 2 * 0.5), dW = (int)(W / 2 * 0.5);
    x0 = W / 2 - dW; y0 = H / 2 - dH; w = 2 * dW; h = 2 * dH;
}

static int pixel_case(int which, int H, int W, int nbr, double fraction, int patch, int border, int wild) {
    PickPixelsArgs a{};
    a.a_w = W - border; a.a_h = H - border; a.W = W; a.patch = patch;
    centre_box(H, W, a.b_x0, a.b_y0, a.b_w, a.b_h);
    const int n_center = fraction > 0 ? (int)(nbr * fraction) : 0, pool_a = a.a_w * a.a_h, pool_b = a.b_w * a.b_h;
    a.n_a = nbr - n_center < pool_a ? nbr - n_center : pool_a;
    a.n_b = n_center < pool_b ? n_center : pool_b;
    unsigned s = 5u + 31u * (unsigned)which;
    // permutations and outputs allocated to their exact sizes: an access outside them is a sanitizer report
    std::vector<int64_t> pa((size_t)a.n_a), pb((size_t)a.n_b);
    const int64_t wilds[4] = {-1, 0, INT64_MAX, INT64_MIN};
    for (int k = 0; k < a.n_a; ++k) pa[k] = wild && k % 2 == 0 ? (wilds[(k / 2) % 4] == 0 ? (int64_t)pool_a : wilds[(k / 2) % 4]) : (int64_t)(lcg(s) % (unsigned)pool_a);
    for (int k = 0; k < a.n_b; ++k) pb[k] = wild && k % 2 == 0 ? (wilds[(k / 2) % 4] == 0 ? (int64_t)pool_b : wilds[(k / 2) % 4]) : (int64_t)(lcg(s) % (unsigned)pool_b);
    a.perm_a = a.n_a ? pa.data() : nullptr;
    a.perm_b = a.n_b ? pb.data() : nullptr;
    a.rows = (a.n_a + a.n_b) * patch * patch;
    std::vector<float> pixels(2 * (size_t)a.rows);
    std::vector<int64_t> rays((size_t)a.rows);
    a.pixels = pixels.data(); a.rays = rays.data();
    for (int r = 0; r < a.rows; ++r) pick_row(a, r);
    int row = 0;
    for (int k = 0; k < a.n_a + a.n_b; ++k) {
        const bool in_a = k < a.n_a;
        int64_t i = in_a ? pa[k] : pb[k - a.n_a];
        const int64_t size = in_a ? pool_a : pool_b;
        i = i < 0 ? 0 : i >= size ? size - 1 : i;
        const int x0 = in_a ? (int)(i % a.a_w) : a.b_x0 + (int)(i % a.b_w), y0 = in_a ? (int)(i / a.a_w) : a.b_y0 + (int)(i / a.b_w);
        for (int dy = 0; dy < patch; ++dy)
            for (int dx = 0; dx < patch; ++dx, ++row) {
                expect(pixels[2 * row] == (float)(x0 + dx), "x", pixels[2 * row], x0 + dx, which, row);
                expect(pixels[2 * row + 1] == (float)(y0 + dy), "y", pixels[2 * row + 1], y0 + dy, which, row);
                expect(rays[row] == (int64_t)(y0 + dy) * W + x0 + dx, "ray", (double)rays[row], (double)((y0 + dy) * W + x0 + dx), which, row);
                expect(x0 + dx >= 0 && x0 + dx < W && y0 + dy >= 0 && y0 + dy < H, "inside the image", x0 + dx, y0 + dy, which, row);
            }
    }
    expect(row == a.rows, "rows", row, a.rows, which, 0);
    // one output alone
    PickPixelsArgs b = a;
    b.pixels = nullptr;
    std::vector<int64_t> rays2((size_t)a.rows);
    b.rays = rays2.data();
    for (int r = 0; r < a.rows; ++r) pick_row(b, r);
    expect(rays2 == rays, "rays alone", 0, 0, which, 0);
    return a.rows;
}

// ---- poses
static const double U = 1.0 / 16777216.0, GAMMA3 = 3 * U / (1 - 3 * U), SLACK = 1.0 + 1.0 / 1024.0;

static void make_poses(std::vector<float>& poses, int B, int row_floats, unsigned seed, int at_centre, int twin_a, int twin_b) {
    poses.assign((size_t)B * row_floats, 0.0f);
    unsigned s = seed;
    for (int b = 0; b < B; ++b) {
        const double al = (lcg(s) % 6283) * 1e-3, be = (lcg(s) % 6283) * 1e-3, ga = (lcg(s) % 6283) * 1e-3;
        const double ca = cos(al), sa = sin(al), cb = cos(be), sb = sin(be), cg = cos(ga), sg = sin(ga);
        const double R[3][3] = {{ca * cb, ca * sb * sg - sa * cg, ca * sb * cg + sa * sg}, {sa * cb, sa * sb * sg + ca * cg, sa * sb * cg - ca * sg}, {-sb, cb * sg, cb * cg}};
        double c[3] = {(lcg(s) % 2001) * 1e-3 - 1.0, (lcg(s) % 2001) * 1e-3 - 1.0, (lcg(s) % 2001) * 1e-3 + 2.0};
        if (b == at_centre) c[0] = c[1] = c[2] = 0.0;
        float* m = poses.data() + (size_t)b * row_floats;
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) m[4 * r + k] = (float)R[r][k];
            m[4 * r + 3] = (float)-(R[r][0] * c[0] + R[r][1] * c[1] + R[r][2] * c[2]);
        }
        if (row_floats == 16) m[15] = 1.0f;
    }
    if (twin_a >= 0)                                     // two cameras at the same centre: the same pose
        for (int k = 0; k < row_floats; ++k) poses[(size_t)twin_b * row_floats + k] = poses[(size_t)twin_a * row_floats + k];
}

static void inverse_d(const float* m, double out[16], double bound[16]) {
    for (int e = 0; e < 16; ++e) { out[e] = 0.0; bound[e] = 0.0; }
    out[15] = 1.0;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = (double)m[4 * c + r];
        double t = 0.0, mag = 0.0;
        for (int k = 0; k < 3; ++k) { t += (double)m[4 * k + r] * (double)m[4 * k + 3]; mag += fabs((double)m[4 * k + r] * (double)m[4 * k + 3]); }
        out[4 * r + 3] = -t;
        bound[4 * r + 3] = GAMMA3 * mag;
    }
}

static void pose_case(int which, int B, int row_floats, int id_self, float w, int at_centre, int twin_a, int twin_b) {
    std::vector<float> poses;
    make_poses(poses, B, row_floats, 900u + (unsigned)which, at_centre, twin_a, twin_b);
    float out[4][16];
    int32_t id_other = -1;
    UnseenPoseArgs a{};
    a.poses_w2c = poses.data(); a.row_floats = row_floats; a.B = B; a.id_self = id_self; a.w = w; a.one_minus_w = (float)(1.0 - (double)w);
    a.w2c_ref = out[0]; a.c2w_ref = out[1]; a.c2w_other = out[2]; a.w2c_unseen = out[3]; a.id_other = &id_other;
    // one serial pass, and the kernel's 64 strided passes merged in the butterfly's order
    double best; int at;
    pick_nearest(a, 0, 1, best, at);
    double lane_best[PICK_WAVE]; int lane_at[PICK_WAVE];
    for (int l = 0; l < PICK_WAVE; ++l) pick_nearest(a, l, PICK_WAVE, lane_best[l], lane_at[l]);
    for (int d = PICK_WAVE / 2; d >= 1; d >>= 1) {
        double nb[PICK_WAVE]; int na[PICK_WAVE];
        for (int l = 0; l < PICK_WAVE; ++l) {
            const bool take = pick_before(lane_best[l ^ d], lane_at[l ^ d], lane_best[l], lane_at[l]);
            nb[l] = take ? lane_best[l ^ d] : lane_best[l];
            na[l] = take ? lane_at[l ^ d] : lane_at[l];
        }
        for (int l = 0; l < PICK_WAVE; ++l) { lane_best[l] = nb[l]; lane_at[l] = na[l]; }
    }
    for (int l = 0; l < PICK_WAVE; ++l) expect(lane_at[l] == at && lane_best[l] == best, "every lane holds the serial result", lane_at[l], at, which, l);
    // a direct restatement of the search
    int want = 0; double wd = 1e300;
    for (int j = 0; j < B; ++j) {
        const double d = j == id_self ? 1e3 : pick_angle(pick_pose(a, id_self), pick_pose(a, j));
        if (d < wd) { wd = d; want = j; }
    }
    expect(at == want, "first index of the minimum", at, want, which, 0);
    if (B == 1) expect(at == 0, "one camera alone", at, 0, which, 0);
    if (twin_a >= 0 && id_self != twin_a && id_self != twin_b) {
        // the twins are equally far: the lower index unless a third camera is nearer
        expect(at != (twin_a > twin_b ? twin_a : twin_b), "the lower index among equals", at, twin_a < twin_b ? twin_a : twin_b, which, 0);
    }
    if (at_centre >= 0 && at_centre != id_self)
        expect(pick_angle(pick_pose(a, id_self), pick_pose(a, at_centre)) == acos(0.0), "a camera at the scene centre", pick_angle(pick_pose(a, id_self), pick_pose(a, at_centre)), acos(0.0), which, 0);
    id_other = (int32_t)at;
    for (int e = 0; e < 16; ++e) pick_pose_outputs(a, at, e);
    // the matrices against double arithmetic
    const float *ms = pick_pose(a, id_self), *mo = pick_pose(a, at);
    double A[16], dA[16], Bm[16], dB[16];
    inverse_d(ms, A, dA);
    inverse_d(mo, Bm, dB);
    const double wq = (double)a.w, vq = (double)a.one_minus_w;
    double bl[16], dbl[16];
    for (int e = 0; e < 16; ++e) {
        bl[e] = wq * A[e] + vq * Bm[e];
        dbl[e] = 2 * U * (fabs(wq * A[e]) + fabs(vq * Bm[e])) + fabs(wq) * dA[e] + fabs(vq) * dB[e];
    }
    for (int e = 0; e < 16; ++e) {
        const int r = e >> 2, c = e & 3;
        const double ref = r < 3 || row_floats == 16 ? (double)ms[e] : (c == 3 ? 1.0 : 0.0);
        expect((double)out[0][e] == ref, "pose_w2c_ref", out[0][e], ref, which, e);
        expect(fabs((double)out[1][e] - A[e]) <= dA[e] * SLACK, "pose_c2w_ref", out[1][e], A[e], which, e);
        expect(fabs((double)out[2][e] - Bm[e]) <= dB[e] * SLACK, "pose_c2w_other", out[2][e], Bm[e], which, e);
        double un, dun;
        if (r == 3) { un = c == 3 ? 1.0 : 0.0; dun = 0.0; }
        else if (c < 3) { un = bl[4 * c + r]; dun = dbl[4 * c + r]; }
        else {
            un = 0.0; dun = 0.0;
            for (int k = 0; k < 3; ++k) {
                un -= bl[4 * k + r] * bl[4 * k + 3];
                dun += GAMMA3 * fabs(bl[4 * k + r] * bl[4 * k + 3]) + dbl[4 * k + r] * fabs(bl[4 * k + 3]) + fabs(bl[4 * k + r]) * dbl[4 * k + 3];
            }
        }
        expect(fabs((double)out[3][e] - un) <= dun * SLACK, "pose_w2c_at_unseen", out[3][e], un, which, e);
    }
}

int main() {
    int which = 0, rows = 0;
    const int images[3][2] = {{7, 9}, {12, 10}, {19, 21}};
    const int nbrs[3] = {1, 5, PICK_BLOCK + 44};
    for (const auto& im : images)
        for (int nbr : nbrs)
            for (double f : {0.0, 0.4})
                for (int patch = 0; patch <= 3; ++patch)         // 0: sample_rays (no patch, a border of 1)
                    for (int wild = 0; wild <= 1; ++wild)
                        rows += pixel_case(which++, im[0], im[1], nbr, f, patch ? patch : 1, patch ? patch - 1 : 1, wild);
    expect(pick_clamp(-1, 48) == 0 && pick_clamp(48, 48) == 47 && pick_clamp(INT64_MAX, 48) == 47 && pick_clamp(INT64_MIN, 48) == 0 && pick_clamp(17, 48) == 17,
           "the clamp", 0, 0, which, 0);
    int poses = 0;
    const int Bs[5] = {1, 2, 3, 6, 70};
    for (int B : Bs)
        for (int row_floats : {12, 16})
            for (int id_self : {0, B / 2, B - 1}) {
                pose_case(which++, B, row_floats, id_self, 0.3f + 0.01f * (float)B, -1, -1, -1);
                if (B >= 3) pose_case(which++, B, row_floats, id_self, 0.77f, (id_self + 1) % B, -1, -1);           // a camera at the scene centre
                if (B >= 6) pose_case(which++, B, row_floats, id_self, 0.5f, -1, (id_self + 2) % B, (id_self + 3) % B);   // two cameras at one centre
                poses += 1;
            }
    if (failures) {
        std::printf("pick_host_check: %d failures\n", failures);
        return 1;
    }
    std::printf("pick_host_check: ok (%d cases, %d pixel rows)\n", which, rows);
    return 0;
}
