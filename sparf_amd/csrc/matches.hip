// Correspondence sampler: the torch series between "pair chosen" and the two renders of a correspondence iteration
// (base_corres_loss.py:260-269, :323-328, :365-369; corres_loss.py:139-155) as two calls -- compact (the centre window, the mask's sum
// and the row order of the five boolean selections) and gather (the permutation's five gathers, with the rounding of :326-328 done for the
// selected rows only).  The logic of a pixel is matches.h's; this file owns the item of the compaction, the gather and the entry points.
//
// Compaction keeps row-major order and uses no atomics (ordered.h's chunked compaction over MatchItem, in tiles of MATCH_BLOCK pixels).
// Up to MATCH_CHUNK pixels one workgroup does all of it in one launch; above, a counts launch over chunks of MATCH_CHUNK pixels and a
// write launch in which each workgroup adds the counts of the chunks before it in chunk order.  `count` stays in device memory.
// Gather: one thread per selected row; the maps are read in place (channel-first correspondences, any channel stride).  Every address
// comes from the index list -- clamped against the device count and the image size -- and none from a value read out of a map.
#include <hip/hip_runtime.h>

#include "../../include/sparf_hip.h"
#include "matches.h"
#include "ordered.h"

namespace sparf {

// what is compacted (the item of ordered.h's chunked compaction, one image): the pixels of the mask inside the window, their flat indices
// as the rows; `finish` leaves the count and the mask's share of the pixels
struct MatchItem {
    typedef MatchCompactArgs Args;
    typedef OrderedNoShared Shared;
    static constexpr int BLOCK = MATCH_BLOCK, CHUNK = MATCH_CHUNK, NCOUNT = 1;
    static __host__ __device__ int n(const MatchCompactArgs& a) { return a.n; }
    static __host__ __device__ int32_t* ws(const MatchCompactArgs& a) { return a.ws; }
    const MatchCompactArgs& a;
    __device__ MatchItem(const MatchCompactArgs& a_, const OrderedNoShared*, int) : a(a_) {}
    __device__ void flags(int p, bool in, bool (&f)[1]) const { f[0] = in && match_keep(a.mask, p, a.W, a.win); }
    __device__ void place(int p, int j) const { a.index[j] = p; }
    __device__ void mark(int, int) const {}
    static __device__ void finish(const MatchCompactArgs& a, int, const int (&run)[1]) {
        a.count[0] = run[0];
        if (a.perc) a.perc[0] = match_perc(run[0], a.n);
    }
};

// corres_loss.py:139-155 for row j: the pixel behind the j-th selected entry of the index list and what the maps hold there
__global__ void __launch_bounds__(MATCH_BLOCK) match_gather_kernel(MatchGatherArgs a) {
    const int j = (int)blockIdx.x * MATCH_BLOCK + (int)threadIdx.x;
    if (j >= a.k) return;
    const int64_t last = (int64_t)min(max(a.count[0], 1), a.n) - 1;          // (a count of 0 with k > 0 is the caller's error: entry 0, clamped below)
    int64_t s = a.sel ? a.sel[j] : (int64_t)j;
    s = s < 0 ? 0 : s > last ? last : s;
    int p = a.index[s];
    p = p < 0 ? 0 : p >= a.n ? a.n - 1 : p;
    float x, y;
    match_pixel(p, a.W, x, y);
    const float cx = a.corres[p], cy = a.corres[a.channel_stride + (int64_t)p];
    a.pixels_self[2 * (size_t)j] = x;
    a.pixels_self[2 * (size_t)j + 1] = y;
    a.ray_self[j] = (int64_t)p;
    a.pixels_other[2 * (size_t)j] = cx;
    a.pixels_other[2 * (size_t)j + 1] = cy;
    a.ray_other[j] = match_rounded_flat(cx, cy, a.W);
    a.conf_out[j] = a.conf[p];
}

}  // namespace sparf

using namespace sparf;

// ---- the entry points (sparf_hip.h): every argument check comes before any HIP call
static const int64_t kMatchMaxPixels = (int64_t)1 << 30;

int64_t sparf_match_workspace_bytes(int64_t n) {
    return n <= kMatchMaxPixels ? ordered_compact_workspace_bytes<MatchItem>(n, 1) : 0;
}

int sparf_match_compact(const unsigned char* mask, int H, int W, int y0, int y1, int x0, int x1, int32_t* index, int32_t* count, float* perc,
                        void* workspace, void* stream) {
    if (H < 0 || W < 0 || (int64_t)H * W > kMatchMaxPixels || !count) return 1;
    hipStream_t s = (hipStream_t)stream;
    const int n = H * W;
    if (n == 0) {                                        // (an empty tensor has no address; 0 / 1e-6 is 0)
        if (hipMemsetAsync(count, 0, sizeof(int32_t), s) != hipSuccess) return 2;
        return !perc || hipMemsetAsync(perc, 0, sizeof(float), s) == hipSuccess ? 0 : 2;
    }
    if (!mask || !index) return 1;
    MatchCompactArgs a{};
    a.mask = mask; a.H = H; a.W = W; a.n = n; a.win = MatchWindow{y0, y1, x0, x1};
    a.index = index; a.count = count; a.perc = perc; a.ws = (int32_t*)workspace;
    return launch_ordered_compact<MatchItem>(a, 1, s);
}

int sparf_match_gather(const int32_t* index, const int32_t* count, const int64_t* sel, int k, int H, int W, const float* corres,
                       int64_t corres_channel_stride, const float* conf, float* pixels_self, int64_t* ray_self, float* pixels_other,
                       int64_t* ray_other, float* conf_out, void* stream) {
    if (k < 0 || H < 0 || W < 0 || (int64_t)H * W > kMatchMaxPixels || (int64_t)k > kMatchMaxPixels || corres_channel_stride < 0) return 1;
    if (k == 0) return 0;
    if ((int64_t)H * W == 0 || !index || !count || !corres || !conf || !pixels_self || !ray_self || !pixels_other || !ray_other || !conf_out) return 1;
    MatchGatherArgs a{};
    a.index = index; a.count = count; a.sel = sel; a.k = k; a.W = W; a.n = H * W;
    a.corres = corres; a.channel_stride = corres_channel_stride; a.conf = conf;
    a.pixels_self = pixels_self; a.ray_self = ray_self; a.pixels_other = pixels_other; a.ray_other = ray_other; a.conf_out = conf_out;
    hipLaunchKernelGGL(match_gather_kernel, dim3((k + MATCH_BLOCK - 1) / MATCH_BLOCK), dim3(MATCH_BLOCK), 0, (hipStream_t)stream, a);
    return launched();
}
