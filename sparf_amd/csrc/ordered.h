// The two device routines behind the loss kernels' promises -- a selection equals torch.where's order bit for bit, a sum gives the same
// bits from call to call -- in their one home: reproj.hip, dcons.hip, photo.hip, matches.hip and colmap.hip call these and hold no
// ballot or butterfly of their own (tests/test_tools_cpu.py).  No atomics, and no workgroup waits for another inside a launch.  Each unit
// keeps its kernels, its launchers and its own block and chunk sizes.
// Out of scope: metrics.hip finishes its tile totals lane-parallel into a workspace, pose_eval.hip has other block sizes and no
// chunks, ray_ops.hip uses float wave sums; optim.hip and the fused MLP units have no such reduction.
#pragma once
#include <hip/hip_runtime.h>

namespace sparf {

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

}  // namespace sparf
