// Weight gradients: dW_l[out][in] = sum over sample rows of dY_l[row][out] * X_l[row][in]
// for the ten layers, as ten split-K MFMA GEMMs ("jobs", layout.h) over the activations
// saved by the forward kernel (X) and the pre-activation gradients written by the dgrad
// kernel (dY).  The contraction runs over rows, so both operands are transposed on their
// way LDS -> registers.  Each workgroup owns one (job, row-range) pair and writes an fp32
// partial [32*MB][32*NB] matrix (+ the bias gradient = column sums of dY); a second kernel
// sums the partials over the splits and scatters them into nn.Linear [out][in] order.
// Deterministic: no atomics.
//
// HBM-bound by design: 2*(M+N)*sizeof(act) bytes per row against 2*M*N flops.
#include <type_traits>

#include "kernels.h"
#include "mlp_dev.h"

namespace sparf {

enum { WG_THREADS = 512, WGRAD_LDS_BYTES = 160 * 1024 };
// streamed-once operands: non-temporal LDS-DMA (MI355X_MICROARCH.md "nt-weights": lands ~18 % sooner)
#define WG_NT " nt"
// Ring refill spread between a tile's MFMAs, and the tile loop as one cross-tile software pipeline: measured, not adopted (HISTORY round 5 "weight
// gradient"; profiles/r05_kernel_ab_spread.log, r05_kernel_ab_wgrad_pipe.log; code retired, last in ebe6c54 and 17caff4).

// sum of the contraction elements one lane holds in an operand fragment (bias gradient)
template <int PREC> struct WOps;
template <> struct WOps<PREC_BF16> {
    static SP_DEV float fsum(bf16x8 v) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += (float)v[j];
        return s;
    }
};
template <> struct WOps<PREC_FP32> {
    static SP_DEV float fsum(float v) { return v; }
};

// ------------------------------------------------------------------ LDS-DMA pipeline
// The saved buffers are tile-major ([tile32][16-byte chunk][row&31][8 elements], layout.h),
// so a 32-row x C-column tile is one contiguous block and its LDS image is made a straight
// copy of it by LDS-DMA (buffer_load ... lds, 1 KiB per wave-instruction, no staging
// registers, no ds_write) -- except that inside each 512-byte chunk block the 32 row slots
// are XOR-swizzled, slot = row ^ ((chunk & 3) << 2), applied on the per-lane SOURCE offset
// and again on the reads: the four chunks a transposing read pass touches then sit on four
// different 64-byte bank groups.
// Ring of NBUF 32-row tile buffers, DEPTH tiles in flight, one barrier per tile:
//     counted vmcnt (tile t landed) -> s_barrier (visible to all, buffer of t-1 free)
//     -> issue DMA(t+DEPTH) -> MFMA on tile t.
// bf16x3 runs the bf16 job on its head planes (layout.h; the two-plane jobs of round 2: code retired, last in ebe6c54).
// ROWS = rows per ring slot: 32 (a whole layout tile, two MFMA k-steps) or 16 (half a tile, one k-step: fp32).
// EB = 4: fp32 operands (v_mfma_f32_32x32x2_f32, one float per lane and k-step, plain
// ds_read_b32 with the same row-slot swizzle: 2-way bank conflicts, MFMA-bound anyway).
// Q8 (layout.h AREA_Q8, bf16-operand modes): both operands arrive as 8-bit integers with one fp32 step per row and vector, half
// the bytes.  The MFMA wants bf16, so a second stage sits between the DMA and the image the fragments are read from: a 32-row
// tile's 1 KiB pieces (one 32-column block each: lanes 0-31 / 32-63 = the two lane halves' 16 slots of the rows) land in an LDS ring
// QD tiles ahead, straight copies; the wave that fetched a piece reads it back, multiplies it out ((u - 128) * step, one step per
// lane: a lane's 16 bytes belong to ONE row) and writes it as two bf16 chunk blocks into the same swizzled image the DMA path builds
// directly; everything from the transposing reads on is shared.  Two images: a wave that writes tile t+1 has passed the barrier of
// tile t, so every wave is done with tile t-1.  (Staging the pieces in registers instead of the LDS ring spilled: the 8 x 10 job
// alone holds 160 accumulator registers.)
// Measured (786 432 rows, same box, profiles/r04_q8_*.log): 1.35 ms -- the time of the bf16 operands with half their bytes.  Probe
// builds say why: the DMA stream alone 0.79 ms, + the conversion 0.84 ms, + the MFMAs WITHOUT conversion 1.06 ms, the MFMA loop on
// its own (no refills) 0.93 ms = 1 900 cycles per 32-row tile where its 2 x 16 MFMAs per SIMD occupy the matrix pipe for 1 024:
// all eight waves meet at one barrier per tile, so the latencies around it (first fragment reads, pipe drain, barrier skew) are paid
// per tile and nothing of another tile's work overlaps them; removing the fragment reads (0.90 ms) or the barrier (-0.1 ms) does not
// change that.  Behind 7.2 GB of bf16 operands (1.07 ms at the 6.7 TB/s a copy reaches) this hides; behind 3.6 GB it is what is left.
// Two re-schedules were built and measured slower: the conversion cut into four-slot units issued behind the MFMAs of the previous
// tile, step rows fetched once per workgroup one tile ahead, DMA operations spread over the MFMA loop (1.43 ms), and the same with
// the conversion as a phase behind the MFMAs (1.47 ms).  Removed again.
// Half jobs inside an 80 KiB LDS budget, two workgroups resident per CU (round 6): 15 % slower; code retired, last in ebe6c54.
template <int MB, int NB, int ROWS = 32, int EB = 2, bool Q8 = false>
SP_DEV void wgrad_job_dma(const WgradArgs& a, int job, char* lds) {
    constexpr bool FP32 = EB == 4;
    static_assert(!Q8 || (ROWS == 32 && EB == 2), "8-bit operands: one bf16 image of whole layout tiles");
    typedef typename std::conditional<FP32, Policy<PREC_FP32>, Policy<PREC_BF16>>::type P;
    typedef typename std::conditional<FP32, float, bf16x8>::type frag_t;
    static_assert(ROWS == 32 || ROWS == 16, "ring slot = a layout tile or half of one");
    static_assert(!FP32 || ROWS == 16, "fp32 operands: 16-row slots");
    constexpr int CS = ROWS * 16;                  // LDS bytes of one 16-byte-chunk block (ROWS row slots)
    constexpr int CPP = 1024 / CS;                 // chunk blocks per 1 KiB DMA piece
    constexpr int KSTEPS = FP32 ? ROWS / 2 : ROWS / 16;                   // MFMA k-steps per slot (K = 2 / 16 rows)
    constexpr int64_t WPARTIAL = wpartial_floats();
    constexpr int EPC = 16 / EB;                                           // elements per 16-byte chunk
    constexpr int M = 32 * MB, N = 32 * NB, CM = M / EPC, CN = N / EPC;    // 16-byte chunks per row
    constexpr int CPB = 32 / EPC;                                          // chunk blocks per 32-column block
    constexpr int DY_BYTES = CM * CS, X_BYTES = CN * CS, BUF_BYTES = DY_BYTES + X_BYTES;
    // ring size: 4 buffers / 3 tiles (96 KiB) in flight per CU.  Filling the whole LDS (up to 8
    // buffers for the narrow jobs) measured the same 1.38 ms: the kernel is not latency-bound.
    constexpr int NBUF_MAX = 4;
    constexpr int NBUF = Q8 ? 2 : WGRAD_LDS_BYTES / BUF_BYTES < NBUF_MAX ? WGRAD_LDS_BYTES / BUF_BYTES : NBUF_MAX;
    constexpr int DEPTH = NBUF - 1;
    constexpr int PIECES = BUF_BYTES / 1024;                              // 1 KiB DMA pieces per tile
    constexpr int PPW_HI = (PIECES + 7) / 8, PPW_LO = PIECES / 8, N_HI = PIECES % 8;   // waves < N_HI issue PPW_HI pieces

    const WJob jb = wjob(job);
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // tile-block-major areas (layout.h): operand tile (tile32, buffer) = area + tile32 * tile bytes + buffer offset
    constexpr int WPREC = FP32 ? PREC_FP32 : PREC_BF16;       // (head planes of bf16x3 = the bf16 image)
    constexpr int64_t DY_TILE = grad_tile_bytes(WPREC), X_TILE = save_tile_bytes(WPREC);
    const char* dy_base = (const char*)a.grad + grad_coloff(jb.gbuf) * 32 * EB;
    const char* x_base = (const char*)a.save + (save_coloff(jb.sbuf) * 32 + (int64_t)jb.xcol0 / EPC * 32 * EPC) * EB;
    (void)dy_base; (void)x_base;

    const int64_t r_begin = a.row_begin + (int64_t)blockIdx.x * a.rows_per_split;
    const int64_t r_end = r_begin + a.rows_per_split < a.rows ? r_begin + a.rows_per_split : a.rows;
    const int ntiles = r_begin < r_end ? (int)((r_end - r_begin + ROWS - 1) / ROWS) : 0;   // last tile ends <= rows_pad

    // DMA source offset of this lane inside a 1 KiB piece = CPP chunk blocks (chunk CPP*q + cip):
    // lane L fills row slot (L % ROWS) of chunk block cip = L / ROWS and must fetch the row
    // slot ^ swizzle(chunk & 3) of that chunk (global chunk blocks are always 32 rows = 512 B)
    const int cip = lane / ROWS, slot = lane % ROWS;
    const int voff_even = (cip * 32 + (slot ^ (((0 + cip) & 3) << 2))) * 16;            // CPP*q = 0 (mod 4)
    const int voff_odd = (cip * 32 + (slot ^ (((CPP + cip) & 3) << 2))) * 16;          // CPP*q = 2 (mod 4): only when CPP == 2

    // piece i (of PPW_HI) of this wave for tile t
    auto issue_piece = [&](int t, int i) {
        char* dst = lds + (t % NBUF) * BUF_BYTES;
        const int64_t tile32 = (r_begin >> 5) + t / (32 / ROWS);
        const int half_off = (t % (32 / ROWS)) * 256;                      // second 16 rows of the layout tile
        {
            const int p = i * 8 + wave;                    // wave-uniform piece id
            if (p < PIECES) {
                const bool is_x = p >= DY_BYTES / 1024;
                const int q = is_x ? p - DY_BYTES / 1024 : p;
                // byte offset of chunk block CPP*q of this operand tile inside its tile block
                const int64_t soff = tile32 * (is_x ? X_TILE : DY_TILE) + (CPP * q) * 512 + half_off;
                const int voff = (CPP == 2 && (q & 1)) ? voff_odd : voff_even;
                // Issued from inline asm on purpose: hipcc orders every LDS read behind a
                // compiler-visible LDS-DMA with s_waitcnt vmcnt(0), which would drain the
                // whole prefetch ring at each tile.  M0 = LDS destination (wave-uniform),
                // saved/restored inside the statement; completion is tracked by the counted
                // s_waitcnt vmcnt(N) below (no other VMEM operation lives in the tile loop).
                const char* src = (is_x ? x_base : dy_base) + soff + (unsigned)voff;
                const unsigned lds_dst = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(dst + p * 1024);
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" WG_NT "\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
            }
        }
    };
    auto issue_tile = [&](int t) {
#pragma unroll
        for (int i = 0; i < PPW_HI; ++i) issue_piece(t, i);
    };

    // bf16: an MFMA operand fragment = 8 consecutive rows (k) of one column (lane&31), fetched with two
    // transposing LDS reads.  ds_read_b64_tr_b16: inside each 16-lane group the 16 x 4 b16 values loaded
    // from the lanes' own addresses are exchanged so that lane i receives element (i&3) of lanes 4j+(i>>2),
    // j = 0..3 (verified on hardware: tools/probes/tr_probe.hip).  Offsets of this lane: 16-lane group g covers
    // k-half g>>1 and feature half g&1; lane i of the group addresses row (i>>2), 8 bytes (i&1)
    // of chunk (g&1)*2 + ((i&3)>>1) of the 32-column block
    const int i16 = lane & 15, g = lane >> 4;
    const int c3 = (g & 1) * 2 + ((i16 & 3) >> 1);
    int roff[2];
#pragma unroll
    for (int q4 = 0; q4 < 2; ++q4) {
        const int prow = ((((g >> 1) << 1 | q4) ^ c3) << 2) | (i16 >> 2);
        roff[q4] = c3 * CS + prow * 16 + (i16 & 1) * 8;
    }
    // fp32: lane l supplies element (row 2*kk + (l>>5), column l&31) of the 32-column block: chunk
    // (l&31)/4, float (l&31)%4; the row slot carries the same XOR swizzle as the DMA applied
    const int f_chunk = (lane & 31) >> 2, f_off = f_chunk * CS + (lane & 3) * 4, f_sw = (f_chunk & 3) << 2;
    auto frag = [&](const char* region, int kk, int blk) -> frag_t {
        if constexpr (FP32) {
            const int row = 2 * kk + h;
            return *(const float*)(region + blk * CPB * CS + f_off + ((row ^ f_sw) << 4));
        } else {
            typedef short s16x4 __attribute__((ext_vector_type(4)));
            typedef short s16x8 __attribute__((ext_vector_type(8)));
            const char* base = region + blk * CPB * CS + kk * 256;           // k-step kk: rows 16*kk .. 16*kk+15 of the slot
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + roff[0]));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + roff[1]));
            s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            return __builtin_bit_cast(bf16x8, v);
        }
    };

    // Output blocks of this wave.  "n-owner" (NB a multiple of 8): the wave keeps one X fragment
    // (n-block = wave) and streams the MB dY fragments; "m-owner" (MB divides 8): it keeps one
    // dY fragment (m-block = wave % MB) and streams X fragments n = wave / MB + (8 / MB) * j.
    // Either way the tile loop is branch-free straight-line code: a block index past the end is
    // clamped (its product is computed and discarded) instead of branched around.
    constexpr bool N_OWNER = NB % 8 == 0;
    static_assert(N_OWNER || 8 % MB == 0, "job shape not covered by the wave assignment");
    constexpr int WPM = N_OWNER ? 1 : 8 / MB;                       // waves sharing an m-block
    constexpr int NJ = N_OWNER ? MB : (NB + WPM - 1) / WPM;         // blocks (accumulators) per wave
    constexpr int NBIAS = N_OWNER ? (MB + 7) / 8 : 1;               // bias m-blocks summed by this wave
    constexpr int NS = KSTEPS * NJ;                                 // streamed fragments per ring slot
    constexpr int PF = NS < 6 ? NS : 6;                             // fragments read ahead of their MFMA
    const int fix_blk = N_OWNER ? wave : wave % MB;
    auto str_blk = [&](int j) {
        if constexpr (N_OWNER) return j;
        else { const int nb = wave / MB + WPM * j; return nb < NB ? nb : NB - 1; }
    };

    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    float bsum[NBIAS];
#pragma unroll
    for (int b = 0; b < NBIAS; ++b) bsum[b] = 0.f;

    // MFMAs of one ring slot: the transposing fragment reads, the products, the bias column sums
    auto compute_tile = [&](const char* dy_t) {
        const char* x_t = dy_t + DY_BYTES;
        const char* fix_t = N_OWNER ? x_t : dy_t;
        const char* str_t = N_OWNER ? dy_t : x_t;

        frag_t fx[KSTEPS], ring[PF];
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) fx[kk] = frag(fix_t, kk, fix_blk);
#pragma unroll
        for (int i = 0; i < PF; ++i) ring[i] = frag(str_t, i / NJ, str_blk(i % NJ));
        // bias gradient = column sums of dY: n-owner waves read "their" m-block once more,
        // m-owner waves already hold it
        frag_t bf[NBIAS][KSTEPS];
        if constexpr (N_OWNER) {
#pragma unroll
            for (int b = 0; b < NBIAS; ++b) {
                const int mb = wave + 8 * b < MB ? wave + 8 * b : MB - 1;
#pragma unroll
                for (int kk = 0; kk < KSTEPS; ++kk) bf[b][kk] = frag(dy_t, kk, mb);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < KSTEPS; ++kk) bf[0][kk] = fx[kk];
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int kk = i / NJ, j = i % NJ;
            // A = dY fragment, B = X fragment
            const frag_t& A_ = N_OWNER ? ring[i % PF] : fx[kk];
            const frag_t& B_ = N_OWNER ? fx[kk] : ring[i % PF];
            acc[j] = P::template mfma_part<0>(A_, B_, acc[j]);
            if (i + PF < NS) ring[i % PF] = frag(str_t, (i + PF) / NJ, str_blk((i + PF) % NJ));
            __builtin_amdgcn_sched_barrier(0);      // keep MFMA i, then the read for MFMA i + PF
        }
#pragma unroll
        for (int b = 0; b < NBIAS; ++b)
#pragma unroll
            for (int kk = 0; kk < KSTEPS; ++kk) bsum[b] += WOps<WPREC>::fsum(bf[b][kk]);
    };
    if constexpr (!Q8) {
        for (int t = 0; t < DEPTH && t < ntiles; ++t) issue_tile(t);
        for (int t = 0; t < ntiles; ++t) {
            // wait for this wave's pieces of tile t: at most (tiles still in flight behind it)
            // x (pieces per tile) of its DMA operations may remain outstanding
            const int ahead = ntiles - 1 - t < DEPTH - 1 ? ntiles - 1 - t : DEPTH - 1;
            static_assert((DEPTH - 1) * PPW_HI <= 63, "vmcnt immediate");
            if (ahead == DEPTH - 1) {                                  // steady state
                if (wave < N_HI) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DEPTH - 1) * PPW_HI) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DEPTH - 1) * PPW_LO) : "memory");
            } else {                                                   // the last DEPTH-1 tiles of the range
                static_for<DEPTH - 1>([&](auto ac) {
                    constexpr int A = decltype(ac)::value;
                    if (ahead == A) {
                        if (wave < N_HI) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A * PPW_HI) : "memory");
                        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A * PPW_LO) : "memory");
                    }
                });
            }
            __syncthreads();          // a bare s_barrier here: the compiler sees no VMEM in flight
            if (t + DEPTH < ntiles) issue_tile(t + DEPTH);
            compute_tile(lds + (t % NBUF) * BUF_BYTES);
        }
    } else {
        // LDS: [bf16 image 0][bf16 image 1][QD ring slots of PQ 1 KiB 8-bit pieces][QD x 8 waves x {dY steps, X steps} (256 B each)]
        constexpr int PQ = MB + NB;                            // 1 KiB pieces per tile: dY blocks 0..MB-1, X blocks 0..NB-1
        constexpr int QSLOT = PQ * 1024, SSLOT = 8 * 512;
        constexpr int QD_FIT = (WGRAD_LDS_BYTES - 2 * BUF_BYTES) / (QSLOT + SSLOT), QD = QD_FIT < 4 ? QD_FIT : 4;     // tiles in flight
        static_assert(QD >= 2, "LDS budget of the 8-bit operand ring");
        constexpr int QP_HI = (PQ + 7) / 8, QP_LO = PQ / 8, QN_HI = PQ % 8;        // pieces per wave: waves < QN_HI take QP_HI
        constexpr int64_t DYQ_TILE = grad_tile_bytes(AREA_Q8), XQ_TILE = save_tile_bytes(AREA_Q8);
        const char* dyq = (const char*)a.grad + grad_buf_tile_off(AREA_Q8, jb.gbuf);
        const char* xq = (const char*)a.save + save_buf_tile_off(AREA_Q8, jb.sbuf) + (jb.xcol0 / 32) * 1024;       // (a 32-column block of the 8-bit areas = 1 KiB)
        const char* dys = (const char*)a.grad + grad_step_tile_off(jb.gbuf, 0);
        const char* xs = (const char*)a.save + save_step_tile_off(jb.sbuf, 0);
        char* ring8 = lds + 2 * BUF_BYTES;
        char* steps = ring8 + QD * QSLOT;
        const int row = lane & 31;
        auto dma = [&](const char* src, char* dst, auto widec) {
            const unsigned lds_dst = (unsigned)(size_t)(__attribute__((address_space(3))) char*)dst;
            unsigned keep;
            if constexpr (decltype(widec)::value)
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" WG_NT "\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
            else
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off" WG_NT "\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
        };
        // this wave's pieces of tile t and the two step rows it multiplies them back with (a wave converts what it fetched itself:
        // its own counted vmcnt is all the synchronisation the ring needs)
        // operation k of this wave for tile t: its QP_HI pieces, then the two step rows (QP_HI + 2 operations; the counted waits
        // below count operations, absent pieces of the waves >= QN_HI are not issued and not counted)
        auto issue_q8_op = [&](int t, int k) {
            const int64_t tile32 = (r_begin >> 5) + t;
            if (k < QP_HI) {
                char* slot = ring8 + (t % QD) * QSLOT;
                const int p = k * 8 + wave;                    // wave-uniform piece id
                if (p < PQ) {
                    const bool is_x = p >= MB;
                    const int C = is_x ? p - MB : p;
                    dma((is_x ? xq + tile32 * XQ_TILE : dyq + tile32 * DYQ_TILE) + C * 1024 + lane * 16, slot + p * 1024, std::true_type{});
                }
            } else {
                char* sw = steps + (t % QD) * SSLOT + wave * 512;
                if (k == QP_HI) dma(dys + tile32 * DYQ_TILE + lane * 4, sw, std::false_type{});             // [part 0][part 1] x 32 rows
                else dma(xs + tile32 * XQ_TILE + lane * 4, sw + 256, std::false_type{});
            }
        };
        auto issue_q8 = [&](int t) {
#pragma unroll
            for (int k = 0; k < QP_HI + 2; ++k) issue_q8_op(t, k);
        };
        auto convert_q8 = [&](int t, char* dst) {
            const char* slot = ring8 + (t % QD) * QSLOT;
            const char* sw = steps + (t % QD) * SSLOT + wave * 512;
#pragma unroll
            for (int i = 0; i < QP_HI; ++i) {
                const int p = i * 8 + wave;
                if (p < PQ) {
                    const bool is_x = p >= MB;
                    const int C = is_x ? p - MB : p;
                    const int part = (is_x ? jb.xcol0 / 32 + C : C) >= 8 ? 1 : 0;       // the vector the block belongs to (layout.h AREA_Q8)
                    const u32x4 q = *(const u32x4*)(slot + p * 1024 + lane * 16);
                    const float step = *(const float*)(sw + (is_x ? 256 : 0) + part * 128 + row * 4), off = -128.0f * step;
                    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
                    u32x4 o[2];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned w = q[j];
                        const bf16x2_t lo = {(__bf16)fmaf((float)(w & 0xffu), step, off), (__bf16)fmaf((float)((w >> 8) & 0xffu), step, off)};
                        const bf16x2_t hi = {(__bf16)fmaf((float)((w >> 16) & 0xffu), step, off), (__bf16)fmaf((float)(w >> 24), step, off)};
                        o[j >> 1][2 * (j & 1)] = __builtin_bit_cast(unsigned, lo);
                        o[j >> 1][2 * (j & 1) + 1] = __builtin_bit_cast(unsigned, hi);
                    }
                    // slots [16 C, 16 C + 8) and [16 C + 8, 16 C + 16) of half h = bf16 chunk blocks 4 C + h and 4 C + 2 + h of the operand
                    char* region = dst + (is_x ? DY_BYTES : 0);
                    const int k0 = 4 * C + h, k1 = k0 + 2;
                    *(u32x4*)(region + k0 * CS + ((row ^ ((k0 & 3) << 2)) << 4)) = o[0];
                    *(u32x4*)(region + k1 * CS + ((row ^ ((k1 & 3) << 2)) << 4)) = o[1];
                }
            }
        };
        for (int t = 0; t < QD && t < ntiles; ++t) issue_q8(t);
        for (int t = 0; t < ntiles; ++t) {
            // this wave's operations of tile t have landed: at most (tiles in flight behind it) x (its operations per tile) remain
            const int ahead = ntiles - 1 - t < QD - 1 ? ntiles - 1 - t : QD - 1;
            static_for<QD>([&](auto ac) {
                constexpr int A = decltype(ac)::value;
                if (ahead == A) {
                    if (wave < QN_HI) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A * (QP_HI + 2)) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A * (QP_LO + 2)) : "memory");
                }
            });
            char* buf = lds + (t & 1) * BUF_BYTES;
            convert_q8(t, buf);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // ring slot read, bf16 image written
            if (t + QD < ntiles) issue_q8(t + QD);                          // (into the slot just consumed)
            asm volatile("s_barrier" ::: "memory");                         // bare barrier: the image of tile t is complete, that of t-1 free
            compute_tile(buf);
        }
    }

    float* out = a.partial + (int64_t)blockIdx.x * WPARTIAL;
    float* mat = out + wjob_mat_off(job);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int m = N_OWNER ? j : fix_blk;
        const int nb_raw = N_OWNER ? wave : wave / MB + WPM * j;
        if (nb_raw < NB) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int po = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
                mat[(int64_t)po * N + nb_raw * 32 + (lane & 31)] = acc[j][r];
            }
        }
    }
    float* bo = out + wjob_bias_off(job);
#pragma unroll
    for (int b = 0; b < NBIAS; ++b) {
        const int m = N_OWNER ? wave + 8 * b : wave;       // m-owner: the first MB waves hold each m once
        const float sum = bsum[b] + __shfl_xor(bsum[b], 32);
        if (m < MB && lane < 32) bo[32 * m + lane] = sum;
    }
}

template <int PREC, bool Q8, int MB, int NB> SP_DEV void wgrad_dispatch(const WgradArgs& a, int job, char* lds) {
    if constexpr (Q8) {
        static_assert(PREC != PREC_FP32, "8-bit areas: bf16-operand modes");
        wgrad_job_dma<MB, NB, 32, 2, true>(a, job, lds);
    } else if constexpr (PREC == PREC_BF16 || PREC == PREC_X3) {
        wgrad_job_dma<MB, NB>(a, job, lds);               // (bf16x3: the bf16 job on the head planes)
    } else {
        wgrad_job_dma<MB, NB, 16, 4>(a, job, lds);        // fp32: LDS-DMA ring of 16-row slots (8.9 -> 7.3 ms vs register staging)
    }
}

template <int PREC, bool Q8 = false>
__global__ void __launch_bounds__(WG_THREADS) wgrad_kernel(WgradArgs a) {
    // the whole 160 KiB LDS of the CU, declared statically: gfx950 launches 163 840 B of static LDS
    // without the per-function opt-in dynamic LDS above 64 KiB would need (no host-side state)
    __shared__ __attribute__((aligned(16))) char lds[WGRAD_LDS_BYTES];
    const int job = blockIdx.y;
    switch (job) {
        case 0: wgrad_dispatch<PREC, Q8, 8, 2>(a, job, lds); break;
        case 4: wgrad_dispatch<PREC, Q8, 8, 10>(a, job, lds); break;
        case 7: wgrad_dispatch<PREC, Q8, 9, 8>(a, job, lds); break;
        case 8: wgrad_dispatch<PREC, Q8, 4, 9>(a, job, lds); break;
        case 9: wgrad_dispatch<PREC, Q8, 1, 4>(a, job, lds); break;
        default: wgrad_dispatch<PREC, Q8, 8, 8>(a, job, lds); break;
    }
}

// out[p] = sum_s partial[s][wsrc[p]], s ascending.  The additions of one element form a chain (the order is part of the
// result), the loads do not: RED_AHEAD splits are loaded before the first of them is added, so a thread waits for memory once per
// RED_AHEAD splits and not once per split (128 and 64 dependent gathered loads per element made the kernel run at half the
// bandwidth its 0.42 GB per step need).  The compiler does not do this on its own: it keeps the loop's loads next to their adds.
enum { RED_AHEAD = 16 };
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ partial, int nsplit, const int32_t* __restrict__ wsrc,
                                                           float* __restrict__ out) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N_PARAMS) return;
    constexpr int64_t WPARTIAL = wpartial_floats();
    const float* src = partial + wsrc[p];
    float s = 0.f;
    int k = 0;
    for (; k + RED_AHEAD <= nsplit; k += RED_AHEAD) {
        float v[RED_AHEAD];
#pragma unroll
        for (int j = 0; j < RED_AHEAD; ++j) v[j] = src[(int64_t)(k + j) * WPARTIAL];
#pragma unroll
        for (int j = 0; j < RED_AHEAD; ++j) s += v[j];
    }
    for (; k < nsplit; ++k) s += src[(int64_t)k * WPARTIAL];
    out[p] = s;
}

// the split-K partial products of `nsplit` row ranges (a.partial = the first of their partial blocks), then
// grad_out = their sum, un-permuted into nn.Linear order
int launch_wgrad(int prec, bool q8, const WgradArgs& a, int nsplit, const int32_t* wsrc, float* grad_out, hipStream_t s) {
    if (a.rows <= 0 || nsplit <= 0) return 1;
    dim3 grid(nsplit, N_WJOBS), block(WG_THREADS);
    if (q8) {            // one kernel for both bf16-operand modes: the areas are the same
        if (prec != PREC_BF16 && prec != PREC_X3) return 1;
        hipLaunchKernelGGL((wgrad_kernel<PREC_BF16, true>), grid, block, 0, s, a);
    } else if (prec == PREC_BF16) hipLaunchKernelGGL(wgrad_kernel<PREC_BF16>, grid, block, 0, s, a);
    else if (prec == PREC_X3) hipLaunchKernelGGL(wgrad_kernel<PREC_X3>, grid, block, 0, s, a);
    else if (prec == PREC_FP32) hipLaunchKernelGGL(wgrad_kernel<PREC_FP32>, grid, block, 0, s, a);
    else return 1;
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((N_PARAMS + 255) / 256), dim3(256), 0, s, a.partial, nsplit, wsrc, grad_out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace sparf
