// Host build of csrc/colmap.h: the valid and positive predicates, the rows of an image, the image and position of a packed row, the
// clamped entry of the index list behind a row and the loss term and seeds, over EVERY pixel of the test shapes
// (tests/colmap_referee.py SHAPES and recipes) against a straightforward serial restatement: the compaction a serial loop leaves, the
// gather of every selected row under a permutation (with positions outside the count among them, which must stay inside the list),
// and the loss and its seeds by a serial double sum.  Plain C++, no HIP:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I sparf_amd/csrc tools/colmap_host_check.cpp -o colmap_host_check
//   ./colmap_host_check        (exit code 0 and "colmap_host_check: ok" when every check holds)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "colmap.h"

using namespace sparf;

static int failures = 0;
static void expect(bool ok, const char* what, double got, double want, int H, int W, int at) {
    if (!ok && ++failures <= 20) std::printf("FAIL %s at %dx%d, %d: got %.17g want %.17g\n", what, H, W, at, got, want);
}

int main() {
    const int B = 4, quota = 32;
    const int shapes[][2] = {{65, 67}, {16, 16}, {64, 64}};
    for (auto& hw : shapes) {
        const int H = hw[0], W = hw[1], n = H * W;
        // the recipes of tests/colmap_referee.maps_of
        std::vector<float> depth((size_t)B * n, 0.0f), conf((size_t)B * n);
        for (int p = 0; p < n; ++p) {
            if (p % 3 == 0) depth[(size_t)p] = (float)(2 + 0.001 * (p % 97));
            if (p % 137 == 1) depth[(size_t)n + p] = (float)(3 + 0.002 * (p % 53));
            if (p % 2 == 0) depth[(size_t)3 * n + p] = 5e-7f;
            for (int b = 0; b < B; ++b) conf[(size_t)b * n + p] = (float)(0.25 + 0.5 * ((7 * p + 3) % 11) / 11);
        }
        depth[(size_t)3 * n] = 1.5f;
        depth[(size_t)3 * n + n - 1] = 2.5f;
        depth[(size_t)3 * n + 7] = -1.0f;
        // compaction: every pixel through the predicates, in order
        std::vector<int32_t> index((size_t)B * n, -1), count((size_t)2 * B, 0);
        for (int b = 0; b < B; ++b)
            for (int p = 0; p < n; ++p) {
                const float d = depth[(size_t)b * n + p];
                expect(colmap_valid(d) == (d > 0.000001f), "valid", colmap_valid(d), d > 0.000001f, H, W, p);
                expect(colmap_positive(d) == (d > 0.0f), "positive", colmap_positive(d), d > 0.0f, H, W, p);
                expect(!colmap_valid(d) || colmap_positive(d), "valid implies positive", 0, 1, H, W, p);
                if (colmap_valid(d)) index[(size_t)b * n + count[(size_t)b]++] = p;
                count[(size_t)B + b] += colmap_positive(d);
            }
        if (H == 65) {
            const int valid[] = {1452, 32, 0, 2}, positive[] = {1452, 32, 0, 2178};
            for (int b = 0; b < B; ++b) {
                expect(count[(size_t)b] == valid[b], "valid count", count[(size_t)b], valid[b], H, W, b);
                expect(count[(size_t)B + b] == positive[b], "positive count", count[(size_t)B + b], positive[b], H, W, b);
            }
            expect(!colmap_draws(count[1], quota) && colmap_draws(count[0], quota), "a count at the quota draws nothing", 0, 1, H, W, 1);
        }
        expect(!colmap_valid(5e-7f) && colmap_positive(5e-7f) && !colmap_positive(-1.0f) && !colmap_valid(NAN), "thresholds", 0, 1, H, W, 0);
        // rows and the packed order
        int K = 0;
        std::vector<int> off((size_t)B + 1, 0);
        for (int b = 0; b < B; ++b) {
            const int k = count[(size_t)b] < quota ? count[(size_t)b] : quota;
            expect(colmap_rows(count[(size_t)b], quota) == k, "rows", colmap_rows(count[(size_t)b], quota), k, H, W, b);
            expect(colmap_offset(count.data(), b, quota) == K, "offset", colmap_offset(count.data(), b, quota), K, H, W, b);
            off[(size_t)b + 1] = K += k;
        }
        expect(colmap_rows(-3, quota) == 0 && colmap_rows(5, 0) == 0, "rows of nothing", 0, 0, H, W, 0);
        for (int r = 0; r < K + 3; ++r) {
            int b = -1, j = -1, k = -1;
            const bool in = colmap_locate(count.data(), B, quota, r, b, j, k);
            expect(in == (r < K), "locate", in, r < K, H, W, r);
            if (in) expect(r >= off[(size_t)b] && r < off[(size_t)b + 1] && j == r - off[(size_t)b] && k == off[(size_t)b + 1] - off[(size_t)b], "located", b, j, H, W, r);
        }
        // gather: a permutation for every image above the quota, with positions outside [0, count) among its entries
        std::vector<int64_t> sel((size_t)B * quota);
        unsigned s = 2024u + (unsigned)n;
        for (size_t i = 0; i < sel.size(); ++i) {
            s = s * 1664525u + 1013904223u;
            const int c = count[i / quota] > 0 ? count[i / quota] : 1;
            sel[i] = (int64_t)((s >> 8) % (unsigned)c);
            if (i % 11 == 5) sel[i] = -7;
            if (i % 13 == 6) sel[i] = (int64_t)n + 100;
        }
        std::vector<double> target, weight;
        for (int b = 0; b < B; ++b) {
            const int c = count[(size_t)b], k = colmap_rows(c, quota);
            for (int j = 0; j < k; ++j) {
                int64_t want_s = c > quota ? sel[(size_t)b * quota + j] : j;
                want_s = want_s < 0 ? 0 : want_s >= c ? c - 1 : want_s;
                const int want = index[(size_t)b * n + want_s];
                const int got = colmap_pixel_of_row(index.data() + (size_t)b * n, sel.data() + (size_t)b * quota, c, quota, n, j);
                expect(got == want && got >= 0 && got < n, "pixel of row", got, want, H, W, j);
                expect(colmap_pixel_of_row(index.data() + (size_t)b * n, nullptr, c, quota, n, j) == index[(size_t)b * n + j], "first rows", 0, 0, H, W, j);
                expect(colmap_valid(depth[(size_t)b * n + got]), "a selected pixel is valid", 0, 1, H, W, got);
                target.push_back(depth[(size_t)b * n + got]);
                weight.push_back(conf[(size_t)b * n + got]);
            }
        }
        // an index list that holds garbage stays inside the image
        const int32_t bad[] = {-5, n + 9};
        expect(colmap_pixel_of_row(bad, nullptr, 2, quota, n, 0) == 0 && colmap_pixel_of_row(bad, nullptr, 2, quota, n, 1) == n - 1, "clamped pixel", 0, 0, H, W, 0);
        expect(colmap_pixel_of_row(bad, nullptr, 0, quota, n, 0) == 0, "no count", 0, 0, H, W, 0);
        // loss and seeds: serial double sums
        for (int fine = 0; fine < 2; ++fine) {
            double total = 0.0, want_total = 0.0;
            for (int b = 0; b < B; ++b) {
                double sum = 0.0;
                const int k = off[(size_t)b + 1] - off[(size_t)b];
                for (int r = off[(size_t)b]; r < off[(size_t)b + 1]; ++r) {
                    const double d = target[(size_t)r], w = weight[(size_t)r], p = 2.0 + 0.01 * (r % 17), pf = p + 0.0625;
                    sum += w * (d - p) * (d - p) + (fine ? w * (d - pf) * (d - pf) : 0.0);
                    total += colmap_row_term(d, w, p, fine != 0, pf) / k;
                    const double seed = colmap_row_seed(d, w, p, k, B), h = 1e-6;
                    const double num = (0.1 / B) * (w * (d - (p + h)) * (d - (p + h)) - w * (d - (p - h)) * (d - (p - h))) / (2 * h) / k;
                    expect(std::fabs(seed - num) <= 1e-7 * (1.0 + std::fabs(num)), "seed", seed, num, H, W, r);
                }
                if (k) want_total += sum / k;
            }
            const double got = colmap_total(total, B), want = 0.1 * want_total / B;
            expect(std::fabs(got - want) <= 1e-14 * (1.0 + std::fabs(want)), "loss", got, want, H, W, fine);
        }
    }
    std::printf(failures ? "colmap_host_check: %d FAILED\n" : "colmap_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
