// Host build of csrc/photo.h: every term of the photometric / mask / depth-patch loss and its derivative on a handful of values, the
// edge ones included (e = +-delta, fg - opacity = 0, a constant patch), each derivative against a central difference.  Plain C++, no HIP:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I sparf_amd/csrc tools/photo_host_check.cpp -o photo_host_check
//   ./photo_host_check        (exit code 0 and "photo_host_check: ok" when every check holds)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "photo.h"

using namespace sparf;

static int failures = 0;
static void expect(bool ok, const char* what, double got, double want) {
    if (!ok) {
        std::printf("FAIL %s: got %.17g want %.17g\n", what, got, want);
        ++failures;
    }
}
static bool close(double a, double b, double tol) { return fabs(a - b) <= tol * (1.0 + fabs(b)); }

struct Depths {
    const std::vector<double>& d;
    double operator()(int j) const { return d[(size_t)j]; }
};
static double patch_total(const std::vector<double>& d, double c) {
    double total = 0.0, s;
    for (int i = 0; i < (int)d.size(); ++i) {
        photo_patch_row(Depths{d}, (int)d.size(), i, c, s);
        total += s;
    }
    return total;
}

int main() {
    const double delta = 0.5, h = 1e-6;
    // colour: both kinds, both sides of the kink and on it
    const double es[] = {0.0, 0.3, -0.3, 0.5, -0.5, 0.5000001, -0.7, 0.9};
    for (int kind = 0; kind < PHOTO_KINDS; ++kind)
        for (double e : es) {
            double l, dl, lp, lm, t;
            photo_colour(kind, delta, e, l, dl);
            const double a = fabs(e);
            const double want = kind == PHOTO_MSE ? e * e : a <= delta ? 0.5 * e * e : delta * (a - 0.5 * delta);
            expect(l == want, "colour l", l, want);
            photo_colour(kind, delta, e + h, lp, t);
            photo_colour(kind, delta, e - h, lm, t);
            expect(close(dl, (lp - lm) / (2 * h), 1e-5), "colour dl", dl, (lp - lm) / (2 * h));    // (C1 at the kink: both sides give delta)
        }
    {
        double l, dl;
        photo_colour(PHOTO_HUBER, delta, delta, l, dl);
        expect(l == 0.125 && dl == 0.5, "huber at +delta", l, 0.125);
        photo_colour(PHOTO_HUBER, delta, -delta, l, dl);
        expect(l == 0.125 && dl == -0.5, "huber at -delta", dl, -0.5);
    }
    // mask: the derivative with respect to the opacity; sgn(0) = 0
    const double ops_[][2] = {{1.0, 0.25}, {0.0, 0.25}, {1.0, 1.0}, {0.0, 0.0}, {1.0, 0.98}};
    for (auto& fo : ops_) {
        double l;
        const double g = photo_mask(fo[0], fo[1], l), a = fo[0] - fo[1];
        expect(l == fabs(a), "mask l", l, fabs(a));
        expect(g == (a > 0 ? -1.0 : a < 0 ? 1.0 : 0.0), "mask g", g, a);
    }
    // depth patch: P = 2, 3, 8; a constant patch is M^2 c with a gradient of exactly 0
    const double c = 0.001;
    for (int P : {1, 2, 3, 8}) {
        const int M = P * P;
        std::vector<double> d((size_t)M), flat((size_t)M, 2.75);
        for (int i = 0; i < M; ++i) d[(size_t)i] = 2.0 + 0.05 * sin(1.7 * i) + 0.01 * i;
        for (int i = 0; i < M; ++i) {
            double s;
            const double g = photo_patch_row(Depths{d}, M, i, c, s);
            std::vector<double> dp = d, dm = d;
            dp[(size_t)i] += h;
            dm[(size_t)i] -= h;
            const double fd = (patch_total(dp, c) - patch_total(dm, c)) / (2 * h);
            expect(close(g, fd, 1e-5), "patch g", g, fd);
            const double g0 = photo_patch_row(Depths{flat}, M, i, c, s);
            expect(g0 == 0.0 && close(s, M * c, 1e-15), "constant patch", g0, 0.0);
        }
        expect(close(patch_total(flat, c), (double)M * M * c, 1e-15), "constant patch total", patch_total(flat, c), (double)M * M * c);
    }
    // the outputs from given totals: both heads add up, what is off is 0
    {
        float out[PHOTO_OUTS];
        unsigned char m = 1;
        float x = 0.f;
        PhotoArgs a{};
        a.rows = 8; a.kind = PHOTO_HUBER; a.patch = 2; a.out = out; a.rgb_fine = &x; a.fg_mask = &m; a.opacity_fine = &x; a.depth_fine = &x;
        const double tot[PHOTO_NACC] = {1, 2, 3, 4, 5, 6, 7, 8};
        photo_outputs(a, tot);
        expect(out[0] == (float)(2.0 * 3.0 / 24.0), "out[0]", out[0], 0.25);
        expect(out[1] == (float)(0.5 * 11.0 / 8.0), "out[1]", out[1], 0.6875);
        expect(out[2] == (float)(0.02 * 15.0 / 32.0), "out[2]", out[2], 0.02 * 15.0 / 32.0);
        expect(out[3] == (float)(3.0 / 24.0) && out[4] == (float)(4.0 / 24.0), "out[3..4]", out[3], 0.125);
        a.kind = PHOTO_MSE; a.rgb_fine = nullptr; a.fg_mask = nullptr; a.patch = 0;
        photo_outputs(a, tot);
        expect(out[0] == (float)(1.0 / (24.0 + 1e-6)) && out[1] == 0.f && out[2] == 0.f && out[4] == 0.f, "outputs, terms off", out[0], 1.0 / 24.0);
    }
    std::printf(failures ? "photo_host_check: %d FAILED\n" : "photo_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
