// The device routines and the launch schemes behind the loss kernels' promises -- a selection equals torch.where's order bit for bit, a
// sum gives the same bits from call to call -- in their one home: reproj.hip, dcons.hip, photo.hip, matches.hip, colmap.hip and
// depth_err.hip call these and hold no ballot or butterfly of their own (tests/test_tools_cpu.py).  No atomics, and no workgroup waits
// for another inside a launch.
//   routines   block_totals, sum_parts, ordered_compact_range
//   schemes    the chunked sum (ordered_sum_*_kernel<S>, launch_ordered_sum<S>) and the chunked compaction
//              (ordered_compact_*_kernel<Item>, launch_ordered_compact<Item>): one launch up to CHUNK elements or without a workspace,
//              two above.  A unit supplies a policy S or an Item -- its loop or its flags, its outputs, its block and chunk sizes -- and
//              holds no kernel or launcher of these kinds itself (reproj.hip's strided grid with a seeds pass is its own scheme).
//   launched() the result of a kernel launch as the entry points return it
// Out of scope: metrics.hip finishes its tile totals lane-parallel into a workspace, pose_eval.hip has other block sizes and no
// chunks, ray_ops.hip uses float wave sums; optim.hip and the fused MLP units have no such reduction.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace sparf {

// after a kernel launch: 0, or 2 where the launch failed
static inline int launched() { return hipGetLastError() == hipSuccess ? 0 : 2; }

// Fixed-order sums: a thread adds its elements in index order into acc (the caller's loop); here a wave adds its lanes by an xor
// butterfly, d = 32 ... 1 (every lane ends with the same bits), and the waves' sums are added in wave order from LDS:
// red[0] + red[1] + ...  -> tot, in every thread.  A caller that uses red again puts a barrier behind the call.
template <int NACC, int WAVES>
__device__ __forceinline__ void block_totals(const double* acc, double (*red)[NACC], double* tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
        double v = acc[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if (lane == 0) red[wave][j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
        double v = red[0][j];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += red[w][j];
        tot[j] = v;
    }
}

// the partial totals ws[0 .. parts) of the workgroups (or chunks), NACC doubles each, added in part order from zero
template <int NACC>
__device__ __forceinline__ void sum_parts(const double* ws, int parts, double* tot) {
#pragma unroll
    for (int j = 0; j < NACC; ++j) tot[j] = 0.0;
    for (int b = 0; b < parts; ++b)
#pragma unroll
        for (int j = 0; j < NACC; ++j) tot[j] += ws[(size_t)b * NACC + j];
}

// Ordered compaction of the elements [first, end) in tiles of BLOCK consecutive ones, by one workgroup of BLOCK threads.  An element
// has NCOUNT flags: flag 0 keeps it, the others are only counted.  Inside a wave a kept element's rank is the popcount of the wave64
// ballot below its lane, the waves' totals go through LDS in wave order, and the running totals run[] are carried across the tiles,
// so the kept rows stand in source order.  run[0] comes in as the output row of the first kept element; every run[c] goes out, in every
// thread, raised by the number of elements with flag c.  `write`: place the rows; otherwise count only.  The item supplies
//   flags(k, in, f)   f[c] = flag c of element k.  in = k < end: the last tile may be partial, and an element past the end is not read
//                     and has no flag set
//   place(k, j)       store kept element k as output row j
//   mark(k, j)        for every element k < end of a writing pass: j is its row, or -1 (empty where no source-to-row map is kept)
template <int BLOCK, int NCOUNT, class Item>
__device__ __forceinline__ void ordered_compact_range(Item& item, int first, int end, bool write, int (&run)[NCOUNT], int (*wave_tot)[NCOUNT]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t0 = first; t0 < end; t0 += BLOCK) {
        const int k = t0 + (int)threadIdx.x;
        const bool in = k < end;
        bool flag[NCOUNT];
        item.flags(k, in, flag);
        unsigned long long ballot[NCOUNT];
#pragma unroll
        for (int c = 0; c < NCOUNT; ++c) ballot[c] = __ballot(flag[c]);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < NCOUNT; ++c) wave_tot[wave][c] = __popcll(ballot[c]);
        }
        __syncthreads();
        int off = run[0], total = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) {
            const int n0 = wave_tot[w][0];
            if (w < wave) off += n0;
            total += n0;
#pragma unroll
            for (int c = 1; c < NCOUNT; ++c) run[c] += wave_tot[w][c];
        }
        if (write && in) {
            int j = -1;
            if (flag[0]) {
                j = off + __popcll(ballot[0] & ((1ull << lane) - 1ull));      // (j < the number of elements: at most every one is kept)
                item.place(k, j);
            }
            item.mark(k, j);
        }
        run[0] += total;
        __syncthreads();                                 // wave_tot is written again by the next tile
    }
}

// ---- the chunked sum.  A policy S supplies
//   Args, BLOCK, CHUNK, NACC
//   rows(a), ws(a)             the number of rows, and the workspace [chunks][NACC] of partial totals (or null)
//   loop(a, first, end, acc)   the rows first, first + BLOCK, ... < end of one thread into acc[NACC], from zero
//   outputs(a, tot)            what one thread leaves from the totals
// Up to CHUNK rows (or without a workspace) one workgroup does all of it in one launch; above, a launch of one workgroup per chunk of
// CHUNK rows that leaves partial totals, and a one-thread launch that adds them in chunk order.
template <class S>
__global__ void __launch_bounds__(S::BLOCK) ordered_sum_single_kernel(typename S::Args a) {
    __shared__ double red[S::BLOCK / 64][S::NACC];
    double acc[S::NACC], tot[S::NACC];
    S::loop(a, threadIdx.x, S::rows(a), acc);
    block_totals<S::NACC, S::BLOCK / 64>(acc, red, tot);
    if (threadIdx.x == 0) S::outputs(a, tot);
}
template <class S>
__global__ void __launch_bounds__(S::BLOCK) ordered_sum_partial_kernel(typename S::Args a) {
    __shared__ double red[S::BLOCK / 64][S::NACC];
    double acc[S::NACC], tot[S::NACC];
    const int first = (int)blockIdx.x * S::CHUNK;
    S::loop(a, first + (int)threadIdx.x, min(S::rows(a), first + S::CHUNK), acc);
    block_totals<S::NACC, S::BLOCK / 64>(acc, red, tot);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < S::NACC; ++j) S::ws(a)[(size_t)blockIdx.x * S::NACC + j] = tot[j];
    }
}
template <class S>
__global__ void __launch_bounds__(S::BLOCK) ordered_sum_finish_kernel(typename S::Args a, int chunks) {
    double tot[S::NACC];
    sum_parts<S::NACC>(S::ws(a), chunks, tot);
    S::outputs(a, tot);
}

template <class S>
static inline int64_t ordered_sum_chunks(int64_t rows) { return (rows + S::CHUNK - 1) / S::CHUNK; }
template <class S>
static inline int64_t ordered_sum_workspace_bytes(int64_t rows) {
    return rows > S::CHUNK ? ordered_sum_chunks<S>(rows) * S::NACC * (int64_t)sizeof(double) : 0;
}

template <class S>
static int launch_ordered_sum(const typename S::Args& a, hipStream_t s) {
    if (S::rows(a) <= S::CHUNK || !S::ws(a)) {
        hipLaunchKernelGGL(ordered_sum_single_kernel<S>, dim3(1), dim3(S::BLOCK), 0, s, a);
        return launched();
    }
    const int chunks = (int)ordered_sum_chunks<S>(S::rows(a));
    hipLaunchKernelGGL(ordered_sum_partial_kernel<S>, dim3(chunks), dim3(S::BLOCK), 0, s, a);
    if (launched()) return 2;
    hipLaunchKernelGGL(ordered_sum_finish_kernel<S>, dim3(1), dim3(1), 0, s, a, chunks);
    return launched();
}

// ---- the chunked compaction, grid (chunks, images).  An Item (see ordered_compact_range) also supplies
//   Args, BLOCK, CHUNK, NCOUNT
//   Shared, setup(a, sh)       what thread 0 prepares in LDS for the workgroup; OrderedNoShared: nothing, and then no LDS object, no
//                              setup and no barrier are paid for
//   n(a), ws(a)                the elements per image, and the workspace [image][chunk][NCOUNT] of counts (or null)
//   Item(a, sh, image)         sh: the workgroup's Shared, null where it is empty
//   finish(a, image, run)      what one thread leaves from the image's totals
// Up to CHUNK elements (or without a workspace) one workgroup per image does all of it in one launch, every tile in turn; above, a counts
// launch over chunks of CHUNK elements and a write launch on the same grid in which each workgroup adds the counts of the chunks before
// it in chunk order and writes its chunk; the last one of an image leaves the totals.
struct OrderedNoShared {};

template <class Item>
__device__ __forceinline__ const typename Item::Shared* ordered_compact_setup(const typename Item::Args& a) {
    if constexpr (std::is_empty<typename Item::Shared>::value) {
        return nullptr;
    } else {
        __shared__ typename Item::Shared sh;
        if (threadIdx.x == 0) Item::setup(a, sh);
        __syncthreads();
        return &sh;
    }
}

template <class Item>
__global__ void __launch_bounds__(Item::BLOCK) ordered_compact_single_kernel(typename Item::Args a) {
    __shared__ int wave_tot[Item::BLOCK / 64][Item::NCOUNT];
    const int image = (int)blockIdx.y;
    Item item(a, ordered_compact_setup<Item>(a), image);
    int run[Item::NCOUNT] = {};
    ordered_compact_range<Item::BLOCK>(item, 0, Item::n(a), true, run, wave_tot);
    if (threadIdx.x == 0) Item::finish(a, image, run);
}
template <class Item>
__global__ void __launch_bounds__(Item::BLOCK) ordered_compact_counts_kernel(typename Item::Args a) {
    __shared__ int wave_tot[Item::BLOCK / 64][Item::NCOUNT];
    const int image = (int)blockIdx.y, first = (int)blockIdx.x * Item::CHUNK;
    Item item(a, ordered_compact_setup<Item>(a), image);
    int run[Item::NCOUNT] = {};
    ordered_compact_range<Item::BLOCK>(item, first, min(Item::n(a), first + Item::CHUNK), false, run, wave_tot);
    if (threadIdx.x == 0) {
        int32_t* ws = Item::ws(a) + Item::NCOUNT * ((size_t)image * gridDim.x + blockIdx.x);
#pragma unroll
        for (int c = 0; c < Item::NCOUNT; ++c) ws[c] = run[c];
    }
}
template <class Item>
__global__ void __launch_bounds__(Item::BLOCK) ordered_compact_write_kernel(typename Item::Args a) {
    __shared__ int wave_tot[Item::BLOCK / 64][Item::NCOUNT];
    const int image = (int)blockIdx.y, first = (int)blockIdx.x * Item::CHUNK;
    Item item(a, ordered_compact_setup<Item>(a), image);
    const int32_t* ws = Item::ws(a) + Item::NCOUNT * (size_t)image * gridDim.x;
    int run[Item::NCOUNT] = {};
    for (int b = 0; b < (int)blockIdx.x; ++b)
#pragma unroll
        for (int c = 0; c < Item::NCOUNT; ++c) run[c] += ws[Item::NCOUNT * b + c];
    ordered_compact_range<Item::BLOCK>(item, first, min(Item::n(a), first + Item::CHUNK), true, run, wave_tot);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) Item::finish(a, image, run);
}

template <class Item>
static inline int64_t ordered_compact_chunks(int64_t n) { return (n + Item::CHUNK - 1) / Item::CHUNK; }
template <class Item>
static inline int64_t ordered_compact_workspace_bytes(int64_t n, int images) {
    return n > Item::CHUNK ? (int64_t)images * ordered_compact_chunks<Item>(n) * Item::NCOUNT * (int64_t)sizeof(int32_t) : 0;
}

template <class Item>
static int launch_ordered_compact(const typename Item::Args& a, int images, hipStream_t s) {
    if (Item::n(a) <= Item::CHUNK || !Item::ws(a)) {
        hipLaunchKernelGGL(ordered_compact_single_kernel<Item>, dim3(1, images), dim3(Item::BLOCK), 0, s, a);
        return launched();
    }
    const dim3 grid((int)ordered_compact_chunks<Item>(Item::n(a)), images);
    hipLaunchKernelGGL(ordered_compact_counts_kernel<Item>, grid, dim3(Item::BLOCK), 0, s, a);
    if (launched()) return 2;
    hipLaunchKernelGGL(ordered_compact_write_kernel<Item>, grid, dim3(Item::BLOCK), 0, s, a);
    return launched();
}

}  // namespace sparf
