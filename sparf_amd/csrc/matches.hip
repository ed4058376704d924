// Correspondence sampler: the torch series between "pair chosen" and the two renders of a correspondence iteration
// (base_corres_loss.py:260-269, :323-328, :365-369; corres_loss.py:139-155) as two calls -- compact (the centre window, the mask's sum
// and the row order of the five boolean selections) and gather (the permutation's five gathers, with the rounding of :326-328 done for the
// selected rows only).  The logic of a pixel is matches.h's; this file owns the ordered compaction, the gather and the entry points.
//
// Compaction keeps row-major order and uses no atomics (ordered.h: ordered_compact_range, in tiles of MATCH_BLOCK consecutive pixels).
// Up to MATCH_CHUNK pixels one workgroup does all of it in one launch; above, a counts launch over chunks of MATCH_CHUNK pixels and a
// write launch in which each workgroup adds the counts of the chunks before it in chunk order.  `count` stays in device memory.
// Gather: one thread per selected row; the maps are read in place (channel-first correspondences, any channel stride).  Every address
// comes from the index list -- clamped against the device count and the image size -- and none from a value read out of a map.
#include <hip/hip_runtime.h>

#include "../../include/sparf_hip.h"
#include "matches.h"
#include "ordered.h"

namespace sparf {

static constexpr int MATCH_WAVES = MATCH_BLOCK / 64;

// what is compacted (the item of ordered_compact_range): the pixels of the mask inside the window, their flat indices as the rows
struct MatchItem {
    const MatchCompactArgs& a;
    __device__ void flags(int p, bool in, bool (&f)[1]) const { f[0] = in && match_keep(a.mask, p, a.W, a.win); }
    __device__ void place(int p, int j) const { a.index[j] = p; }
    __device__ void mark(int, int) const {}
};

// the pixels [first, end) by one workgroup: -> base + the number kept (in every thread).  `write`: leave the indices; otherwise count only.
static __device__ int match_compact_range(const MatchCompactArgs& a, int first, int end, int base, bool write, int (*wave_tot)[1]) {
    MatchItem item{a};
    int run[1] = {base};
    ordered_compact_range<MATCH_BLOCK>(item, first, end, write, run, wave_tot);
    return run[0];
}

static __device__ void match_totals(const MatchCompactArgs& a, int total) {
    a.count[0] = total;
    if (a.perc) a.perc[0] = match_perc(total, a.n);
}

// n <= MATCH_CHUNK (or no workspace): one workgroup, every tile in turn
__global__ void __launch_bounds__(MATCH_BLOCK) match_compact_single_kernel(MatchCompactArgs a) {
    __shared__ int wave_tot[MATCH_WAVES][1];
    const int total = match_compact_range(a, 0, a.n, 0, true, wave_tot);
    if (threadIdx.x == 0) match_totals(a, total);
}

// n > MATCH_CHUNK, one workgroup per chunk: the number kept of chunk b at ws[b]
__global__ void __launch_bounds__(MATCH_BLOCK) match_compact_counts_kernel(MatchCompactArgs a) {
    __shared__ int wave_tot[MATCH_WAVES][1];
    const int first = (int)blockIdx.x * MATCH_CHUNK;
    const int total = match_compact_range(a, first, min(a.n, first + MATCH_CHUNK), 0, false, wave_tot);
    if (threadIdx.x == 0) a.ws[blockIdx.x] = total;
}

// same grid: every workgroup adds the counts of the chunks before it in chunk order and writes its chunk; the last one leaves the count
__global__ void __launch_bounds__(MATCH_BLOCK) match_compact_write_kernel(MatchCompactArgs a) {
    __shared__ int wave_tot[MATCH_WAVES][1];
    int base = 0;
    for (int b = 0; b < (int)blockIdx.x; ++b) base += a.ws[b];
    const int first = (int)blockIdx.x * MATCH_CHUNK;
    const int total = match_compact_range(a, first, min(a.n, first + MATCH_CHUNK), base, true, wave_tot);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) match_totals(a, total);
}

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

static inline int64_t match_chunks(int64_t n) { return (n + MATCH_CHUNK - 1) / MATCH_CHUNK; }

static int launch_match_compact(const MatchCompactArgs& a, hipStream_t s) {
    if (a.n <= MATCH_CHUNK || !a.ws) {
        hipLaunchKernelGGL(match_compact_single_kernel, dim3(1), dim3(MATCH_BLOCK), 0, s, a);
        return hipGetLastError() == hipSuccess ? 0 : 2;
    }
    const int chunks = (int)match_chunks(a.n);
    hipLaunchKernelGGL(match_compact_counts_kernel, dim3(chunks), dim3(MATCH_BLOCK), 0, s, a);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(match_compact_write_kernel, dim3(chunks), dim3(MATCH_BLOCK), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace sparf

using namespace sparf;

// ---- the entry points (sparf_hip.h): every argument check comes before any HIP call
static const int64_t kMatchMaxPixels = (int64_t)1 << 30;

int64_t sparf_match_workspace_bytes(int64_t n) {
    return n > MATCH_CHUNK && n <= kMatchMaxPixels ? match_chunks(n) * (int64_t)sizeof(int32_t) : 0;
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
    return launch_match_compact(a, s);
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
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
