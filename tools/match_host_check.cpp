// Host build of csrc/matches.h: the keep predicate, the pixel of a flat index and the rounded flat index over EVERY pixel of the test
// shapes (tests/matches_referee.py SHAPES) against a straightforward serial restatement, under each window form (none, the pre-crop
// window with its - 1, one row, empty), with exact .5 ties of both parities, W - 1, H - 1 and -0.0 among the correspondences; and the
// valid-share division.  Plain C++, no HIP:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I sparf_amd/csrc tools/match_host_check.cpp -o match_host_check
//   ./match_host_check        (exit code 0 and "match_host_check: ok" when every check holds)
#include <cfenv>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "matches.h"

using namespace sparf;

static int failures = 0;
static void expect(bool ok, const char* what, long long got, long long want, int H, int W, int p) {
    if (!ok && ++failures <= 20) std::printf("FAIL %s at %dx%d pixel %d: got %lld want %lld\n", what, H, W, p, got, want);
}

// round half to even without rint: floor, then the tie by the parity of the floor
static long long round_half_even(float v) {
    const double f = floor((double)v), r = (double)v - f;
    if (r > 0.5) return (long long)f + 1;
    if (r < 0.5) return (long long)f;
    return ((long long)f % 2 == 0) ? (long long)f : (long long)f + 1;
}

int main() {
    if (fegetround() != FE_TONEAREST) {
        std::printf("match_host_check: not in round-to-nearest\n");
        return 1;
    }
    const int shapes[][2] = {{7, 9}, {16, 16}, {63, 65}, {64, 64}, {64, 65}, {96, 128}};
    for (auto& hw : shapes) {
        const int H = hw[0], W = hw[1], n = H * W;
        std::vector<unsigned char> mask((size_t)n);
        std::vector<float> cx((size_t)n), cy((size_t)n);
        unsigned s = 12345u + (unsigned)n;
        for (int p = 0; p < n; ++p) {
            s = s * 1664525u + 1013904223u;
            mask[(size_t)p] = (unsigned char)(((s >> 16) % 3 == 0) ? ((s >> 8) % 2 ? 1 : 255) : 0);      // any non-zero byte is true
            const int k = (int)((s >> 4) % 7);
            const float bx = (float)((s >> 9) % (unsigned)W), by = (float)((s >> 13) % (unsigned)H);
            cx[(size_t)p] = k == 0 ? bx + 0.5f : k == 1 ? (float)(W - 1) : k == 2 ? -0.0f : k == 3 ? bx + 0.49999f : bx + 0.25f * (float)k;
            cy[(size_t)p] = k == 0 ? by - 0.5f : k == 1 ? (float)(H - 1) : k == 2 ? 2.5f : k == 3 ? by + 0.50001f : by - 0.125f * (float)k;
        }
        const int dH = (int)(H / 2 * 0.5), dW = (int)(W / 2 * 0.5);
        const MatchWindow windows[] = {{0, H, 0, W}, {H / 2 - dH, H / 2 + dH - 1, W / 2 - dW, W / 2 + dW - 1}, {H / 2, H / 2 + 1, 0, W},
                                       {H / 2, H / 2 - 1, W / 2 - dW, W / 2 + dW - 1}};
        for (const MatchWindow& w : windows) {
            int kept = 0, want_kept = 0;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const int p = y * W + x;
                    const bool want = mask[(size_t)p] != 0 && y >= w.y0 && y < w.y1 && x >= w.x0 && x < w.x1;
                    const bool got = match_keep(mask.data(), p, W, w);
                    expect(got == want, "keep", got, want, H, W, p);
                    kept += got;
                    want_kept += want;
                }
            expect(kept == want_kept, "kept", kept, want_kept, H, W, -1);
            if (w.y1 <= w.y0) expect(kept == 0, "empty window", kept, 0, H, W, -1);
        }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int p = y * W + x;
                float px, py;
                match_pixel(p, W, px, py);
                expect(px == (float)x && py == (float)y, "pixel", (long long)px, x, H, W, p);
                const long long want = round_half_even(cy[(size_t)p]) * W + round_half_even(cx[(size_t)p]);
                const long long got = (long long)match_rounded_flat(cx[(size_t)p], cy[(size_t)p], W);
                expect(got == want, "rounded flat", got, want, H, W, p);
            }
        for (int c : {0, 1, n / 3, n - 1, n}) {
            const float got = match_perc(c, n), want = (float)c / (float)((double)n + 1e-6);
            expect(got == want && got <= 1.0f, "perc", (long long)(got * 1e6f), (long long)(want * 1e6f), H, W, c);
        }
    }
    // torch.round on the values the issue names: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.0 -> 0
    expect(match_rounded_flat(0.5f, 1.5f, 10) == 20, "ties", (long long)match_rounded_flat(0.5f, 1.5f, 10), 20, 0, 10, 0);
    expect(match_rounded_flat(2.5f, -0.0f, 10) == 2, "ties", (long long)match_rounded_flat(2.5f, -0.0f, 10), 2, 0, 10, 0);
    std::printf(failures ? "match_host_check: %d FAILED\n" : "match_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
