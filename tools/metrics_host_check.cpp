// Host build of csrc/metrics.h: the window, the SSIM of a pixel from separable passes plus the residual of the stored 2-D window -- on every
// pixel of the small shapes, against a serial direct 2-D restatement with the float products fl(w_i w_j) --, the composite, the depth terms
// and the finishing arithmetic with its edge cases (mse 0, an empty selection).  Plain C++, no HIP:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I sparf_amd/csrc tools/metrics_host_check.cpp -o metrics_host_check
//   ./metrics_host_check        (exit code 0 and "metrics_host_check: ok" when every check holds)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "metrics.h"

using namespace sparf;

static int failures = 0;
static void expect(bool ok, const char* what, double got, double want) {
    if (!ok) {
        std::printf("FAIL %s: got %.17g want %.17g\n", what, got, want);
        ++failures;
    }
}
static bool close(double a, double b, double tol) { return fabs(a - b) <= tol * (1.0 + fabs(b)); }

struct Image {
    int H, W;
    std::vector<float> v;
    float at(int y, int x) const { return y < 0 || y >= H || x < 0 || x >= W ? 0.0f : v[(size_t)y * W + x]; }      // zero padding
};
static Image make(int H, int W, unsigned seed, float lo, float hi) {
    Image im{H, W, std::vector<float>((size_t)H * W)};
    unsigned s = seed;
    for (float& x : im.v) {
        s = s * 1664525u + 1013904223u;
        x = lo + (hi - lo) * (float)(s >> 8) / 16777216.0f;
    }
    return im;
}

// the five moments of pixel (y, x) as the kernel forms them: rows, then columns, in double; then the residual in float
static void moments_separable(const Image& a, const Image& b, int y, int x, double m[5]) {
    double rows[METRICS_K][5];
    for (int i = 0; i < METRICS_K; ++i) {
        for (int k = 0; k < 5; ++k) rows[i][k] = 0.0;
        for (int j = 0; j < METRICS_K; ++j) {
            const double w = metrics_weight(j), p = (double)a.at(y + i - METRICS_R, x + j - METRICS_R), g = (double)b.at(y + i - METRICS_R, x + j - METRICS_R);
            rows[i][0] += w * p;
            rows[i][1] += w * g;
            rows[i][2] += w * (p * p);
            rows[i][3] += w * (g * g);
            rows[i][4] += w * (p * g);
        }
    }
    float q[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 5; ++k) m[k] = 0.0;
    for (int i = 0; i < METRICS_K; ++i)
        for (int k = 0; k < 5; ++k) m[k] += metrics_weight(i) * rows[i][k];
    for (int i = 0; i < METRICS_K; ++i)
        for (int j = 0; j < METRICS_K; ++j) {
            const float d = metrics_residual(i, j), p = a.at(y + i - METRICS_R, x + j - METRICS_R), g = b.at(y + i - METRICS_R, x + j - METRICS_R);
            q[0] += d * p;
            q[1] += d * g;
            q[2] += d * (p * p);
            q[3] += d * (g * g);
            q[4] += d * (p * g);
        }
    for (int k = 0; k < 5; ++k) m[k] += (double)q[k];
}
// the same by the direct 2-D sum with the stored float window
static void moments_direct(const Image& a, const Image& b, int y, int x, double m[5]) {
    for (int k = 0; k < 5; ++k) m[k] = 0.0;
    for (int i = 0; i < METRICS_K; ++i)
        for (int j = 0; j < METRICS_K; ++j) {
            const double w = (double)metrics_window_2d(i, j), p = (double)a.at(y + i - METRICS_R, x + j - METRICS_R), g = (double)b.at(y + i - METRICS_R, x + j - METRICS_R);
            m[0] += w * p;
            m[1] += w * g;
            m[2] += w * p * p;
            m[3] += w * g * g;
            m[4] += w * p * g;
        }
}

int main() {
    // the window: symmetric, positive, float sum within a spacing of 1; the residual below 2^-24 of the product
    double sum = 0.0;
    for (int k = 0; k < METRICS_K; ++k) {
        sum += metrics_weight(k);
        expect(metrics_weight(k) == metrics_weight(METRICS_K - 1 - k) && metrics_weight(k) > 0.0, "window symmetry", metrics_weight(k), metrics_weight(METRICS_K - 1 - k));
    }
    expect(fabs(sum - 1.0) < 2e-7, "window sum", sum, 1.0);
    for (int i = 0; i < METRICS_K; ++i)
        for (int j = 0; j < METRICS_K; ++j) {
            const double exact = metrics_weight(i) * metrics_weight(j);
            expect(fabs((double)metrics_residual(i, j)) <= exact * 0x1p-24, "residual size", metrics_residual(i, j), exact * 0x1p-24);
            expect(close((double)metrics_window_2d(i, j), exact + (double)metrics_residual(i, j), 1e-15), "residual", metrics_window_2d(i, j), exact);
        }
    // every pixel of the small shapes: random images; a constant one with one pixel off; identical images
    const int shapes[][2] = {{1, 1}, {5, 7}, {11, 11}, {10, 12}, {17, 33}};
    for (auto& hw : shapes) {
        const int H = hw[0], W = hw[1];
        Image a = make(H, W, 17u + H, 0.0f, 1.0f), b = make(H, W, 91u + W, 0.0f, 1.0f);
        Image flat = make(H, W, 5u, 0.5f, 0.5f), off = flat;
        off.v[(size_t)(H / 2) * W + W / 2] = 0.75f;
        const Image* pairs[][2] = {{&a, &b}, {&off, &flat}, {&a, &a}};
        for (auto& pr : pairs)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    double ms[5], md[5];
                    moments_separable(*pr[0], *pr[1], y, x, ms);
                    moments_direct(*pr[0], *pr[1], y, x, md);
                    for (int k = 0; k < 5; ++k) expect(close(ms[k], md[k], 1e-13), "moment", ms[k], md[k]);
                    const double s = metrics_ssim(ms[0], ms[1], ms[2], ms[3], ms[4]), d = metrics_ssim(md[0], md[1], md[2], md[3], md[4]);
                    expect(close(s, d, 1e-9), "ssim", s, d);
                    expect(s <= 1.0 + 1e-12 && s >= -1.0 - 1e-12, "ssim range", s, 1.0);
                    if (pr[0] == pr[1]) expect(s == 1.0, "ssim of identical images", s, 1.0);
                }
    }
    // the composite of a binary mask is x or 1, exactly
    for (float x : {0.0f, 0.3f, 1.0f, 0.99999994f}) {
        expect(metrics_composite((double)x, 1.0) == (double)x, "composite m = 1", metrics_composite((double)x, 1.0), x);
        expect(metrics_composite((double)x, 0.0) == 1.0, "composite m = 0", metrics_composite((double)x, 0.0), 1.0);
    }
    // depth terms
    {
        double sq;
        expect(metrics_depth(2.0, 1.5, 1.0, sq) == 0.5 && sq == 0.25, "depth s = 1", sq, 0.25);
        expect(metrics_depth(2.0, 1.5, 2.0, sq) == 1.0 && sq == 1.0, "depth s = 2", sq, 1.0);
    }
    // finishing arithmetic and its edge cases
    expect(metrics_mse(3.0, 12.0) == 0.25, "mse", metrics_mse(3.0, 12.0), 0.25);
    expect(close(metrics_psnr(0.01), 20.0, 1e-15), "psnr", metrics_psnr(0.01), 20.0);
    expect(isinf(metrics_psnr(metrics_mse(0.0, 12.0))) && metrics_psnr(0.0) > 0, "psnr of mse 0 is +inf", metrics_psnr(0.0), INFINITY);
    expect(isnan(metrics_mse(0.0, 0.0)) && isnan(metrics_psnr(metrics_mse(0.0, 0.0))), "empty selection: NaN", metrics_mse(0.0, 0.0), NAN);
    expect(metrics_abs_e(0.0, 0.0) == 0.0, "abs_e of no pixel is 0", metrics_abs_e(0.0, 0.0), 0.0);
    expect(isnan(metrics_rmse(0.0, 0.0)), "rmse of no pixel is NaN", metrics_rmse(0.0, 0.0), NAN);
    expect(metrics_abs_e(3.0, 2.0) == 3.0 / (2.0 + 1e-6) && metrics_rmse(8.0, 2.0) == 2.0, "abs_e, rmse", metrics_rmse(8.0, 2.0), 2.0);
    // the outputs from given totals: what was not asked for is NaN
    {
        float out[METRICS_HEADS * METRICS_OUTS], x = 0.f;
        int32_t counts[2];
        unsigned char m = 1;
        MetricsArgs a{};
        a.B = 1; a.H = 2; a.W = 2; a.out = out; a.counts = counts;
        a.fine.p = &x; a.mask = &m; a.depth.p = &x; a.depth_gt.p = &x;
        double tot[METRICS_NACC] = {6, 3, 12, 1.5, 2, 8, 1, 2,   9, 0, 12, 0, 0, 0, 0, 0,   2, 2};
        metrics_outputs(a, tot);
        expect(out[0] == 0.25f && out[1] == (float)(-10.0 * log10(0.25)) && out[2] == 0.5f, "head 0", out[0], 0.25);
        expect(out[3] == 0.25f && out[5] == 1.0f && out[6] == (float)(2.0 / (2.0 + 1e-6)) && out[7] == 2.0f && out[9] == 1.0f, "head 0 masked, depth", out[3], 0.25);
        expect(out[10] == 0.0f && isinf(out[11]) && out[12] == 0.75f && isnan(out[16]) && isnan(out[19]), "head 1", out[12], 0.75);
        expect(counts[0] == 2 && counts[1] == 2, "counts", counts[0], 2);
        a.fine.p = nullptr; a.mask = nullptr; a.depth.p = nullptr;
        tot[16] = tot[17] = 0;
        metrics_outputs(a, tot);
        bool off = true;
        for (int i = 3; i < 2 * METRICS_OUTS; ++i) off = off && isnan(out[i]);
        expect(off && out[2] == 0.5f && counts[0] == 0, "what is off is NaN", out[3], NAN);
    }
    std::printf(failures ? "metrics_host_check: %d FAILED\n" : "metrics_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
