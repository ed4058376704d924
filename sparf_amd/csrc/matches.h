// Correspondence sampler: the arguments of the kernels of matches.hip and the per-pixel logic of the sampler of
// CorrespondenceBasedLoss (base_corres_loss.py:260-269, :323-328, :365-369; corres_loss.py:139-155) as plain functions: which pixels of
// the valid-correspondence mask are kept, the pixel of a flat index, and the flat index of a rounded correspondence.  Integer and copy
// work only: nothing is rounded except by rint, so a result either equals the reference's bit for bit or is wrong.  Nothing here touches
// a thread index, LDS or a HIP call; matches.hip owns the ordered compaction and the gather.
// The file also compiles as plain C++ (tools/match_host_check.cpp evaluates it on the host under the sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef MATCH_DEV
#ifdef __HIPCC__
#define MATCH_DEV __host__ __device__ __forceinline__
#else
#define MATCH_DEV inline
#endif
#endif

namespace sparf {

enum {
    MATCH_BLOCK = 256,           // four waves: a tile of the compaction, and the rows of a gather workgroup
    MATCH_CHUNK = 4096,          // pixels up to which one workgroup compacts everything in one launch; above, the pixels of one workgroup
};

struct MatchWindow {             // rows [y0, y1) and columns [x0, x1): may be empty; 0, H, 0, W is no window
    int y0, y1, x0, x1;
};

struct MatchCompactArgs {
    const unsigned char* mask;   // [H][W] bytes 0 / non-0 (torch.bool storage), any alignment
    int H, W, n;                 // n = H W
    MatchWindow win;
    int32_t* index;              // [n]: the flat indices of the kept pixels, ascending
    int32_t* count;              // [1]
    float* perc;                 // [1] or null
    int32_t* ws;                 // [chunks] kept pixels per chunk (n > MATCH_CHUNK), or null
};

struct MatchGatherArgs {
    const int32_t* index;        // [n], its first *count entries written by the compaction
    const int32_t* count;        // [1]
    const int64_t* sel;          // [k] positions in index, or null: the first k
    int k, W, n;                 // n = H W
    const float* corres;         // x at corres[p], y at corres[channel_stride + p]
    int64_t channel_stride;
    const float* conf;           // [n]
    float* pixels_self;          // [k][2]
    int64_t* ray_self;           // [k]
    float* pixels_other;         // [k][2]
    int64_t* ray_other;          // [k]
    float* conf_out;             // [k]
};

// base_corres_loss.py:267-269 (mask & mask_center) on pixel p: kept if its mask byte is set and it lies in the window
static MATCH_DEV bool match_keep(const unsigned char* mask, int p, int W, const MatchWindow& w) {
    if (mask[p] == 0) return false;
    const int y = p / W, x = p - y * W;
    return y >= w.y0 && y < w.y1 && x >= w.x0 && x < w.x1;
}

// base_corres_loss.py:46-48 self.grid at flat index p: (x, y) as floats
static MATCH_DEV void match_pixel(int p, int W, float& x, float& y) {
    x = (float)(p % W);
    y = (float)(p / W);
}

// base_corres_loss.py:326-328: torch.round (half to even, as rintf in the default rounding mode) .long(), then y W + x
static MATCH_DEV int64_t match_rounded_flat(float cx, float cy, int W) { return (int64_t)rintf(cy) * (int64_t)W + (int64_t)rintf(cx); }

// base_corres_loss.py:369 mask.sum() / (mask.nelement() + 1e-6): an int64 tensor over a Python float is a float32 division
static MATCH_DEV float match_perc(int count, int n) { return (float)count / (float)((double)n + 1e-6); }

}  // namespace sparf
