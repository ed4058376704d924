// Host-only: the plan of a pass -- which kernels sparf_pass_forward / sparf_pass_backward launch, over which rows, with which
// arguments -- computed by ONE function per direction (plan_forward, plan_backward), so that the pass calls, the single-kernel
// entry point sparf_launch_kernel and the sparf_debug_* exports (api.hip) cannot disagree.  No HIP call but the cached num_cus().
#pragma once
#include "../../include/sparf_hip.h"

#include "kernels.h"
#include "streams.h"

namespace sparf {

static constexpr int64_t kPartialFloats = wpartial_floats();      // (compile time: streams.h's constexpr enumeration loops are not re-run per call)

static constexpr bool prec_ok(int p) { return p >= 0 && p < N_PREC; }
// A pass's precision id may carry SPARF_SAVE_Q8 (sparf_hip.h): the arithmetic of `base`, save and gradient areas in the 8-bit format
// (layout.h AREA_Q8); the modes that have such a forward kernel (kernels.h: the bf16-operand ones).  Or SPARF_SAVE_MASKS: a
// ray-gradient-only pass of any base precision -- the save area holds the ReLU mask words only (layout.h AREA_MASKS), the backward
// runs no weight gradient.  Not both.
struct PassPrec { int base; bool q8, masks; int af; bool ok; int save; };      // save: what the training forward leaves (kernels.h FWD_SAVE_*)
static constexpr PassPrec pass_prec(int p) {
    PassPrec r{};
    r.base = p & ~(SPARF_SAVE_Q8 | SPARF_SAVE_MASKS);
    r.q8 = (p & SPARF_SAVE_Q8) != 0;
    r.masks = (p & SPARF_SAVE_MASKS) != 0;
    r.save = r.q8 ? FWD_SAVE_Q8 : r.masks ? FWD_SAVE_MASKS : FWD_SAVE_PLANES;
    r.ok = prec_ok(r.base) && (!r.q8 || find_mlp_fwd(r.base, FWD_SAVE_Q8)) && !(r.q8 && r.masks);
    r.af = r.masks ? (int)AREA_MASKS : area_format(r.ok ? r.base : 0, r.q8);
    return r;
}
// one launch set takes up to 2^27 sample rows (the per-row outputs are indexed with 32-bit element offsets);
// the save / gradient areas are addressed per 32-row tile block (layout.h) and have no limit of their own
static inline bool rows_ok(int64_t rows) { return rows <= ((int64_t)1 << 27); }
static inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }
static inline int num_cus() {
    // CU count of the current device, looked up once per device: an immutable hardware attribute (the only
    // process-level state of the library), so that the pass calls issue no device queries -- they may be
    // running under hipGraph stream capture
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0) {
        int n = 256;
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        cached[dev] = n > 0 ? n : 256;
    }
    return cached[dev];
}
static inline int mlp_grid(int prec, int64_t rows) {
    const int tile = nwaves_of(prec) * 32;
    const int64_t ntiles = (rows + tile - 1) / tile;
    const int cus = num_cus();
    return (int)(ntiles < cus ? ntiles : cus);
}
// Workgroup geometry of the bf16x3 data-gradient kernel for a launch over `rows` rows (mlp_dev.h PolicyX3DgradT): both kernels run
// one workgroup per CU striding over their tiles, so a launch lasts (rounds of tiles) x (time of one tile).  The 8-wave kernel's
// 256-row tile is 12-17 % cheaper per row, but its last round may be mostly empty: 32 768 rows (the coarse pass of a 512-ray
// step) are 128 of its tiles -- half the chip idle for a whole tile time -- and exactly one round of 128-row tiles.  A 128-row
// tile of the 4-wave kernel takes X3_W4_TILE_PCT % of a 256-row tile's time -- and a launch whose rows are some full rounds plus a poor
// last one can run the full rounds in 8 waves and the remainder in 4 (x3_dgrad_rows8 below) -- (measured, profiles/r06_dgrad_geometry.log: 0.066-0.071 ms
// against 0.097-0.112 ms per round; 32 768 rows 0.112 -> 0.071 ms, with pose gradients 0.115 -> 0.080; 98 304 rows a wash, every
// other shape of the table the 8-wave kernel by 5-12 %).
enum { X3_W4_TILE_PCT = 64 };
// -> the leading rows that go through the 8-wave kernel (a whole number of its rounds; 0: none, rows: all); the rest, if any, follow in
// a second launch of the 4-wave kernel over [rows8, rows).  Three candidates in units of one 256-row tile time / 100: every round in
// 8 waves; every round in 4 waves; the full 8-wave rounds + the remainder in 128-row tiles (+ X3_SPLIT_LAUNCH_PCT for the second launch):
// 98 304 rows (the fine pass of a 512-ray step) are 1.5 rounds of 256-row tiles = 2 tile times, or 1 + 0.64.
enum { X3_SPLIT_LAUNCH_PCT = 6 };
static inline int64_t x3_dgrad_rows8(int64_t rows) {
    const int64_t cus = num_cus(), round8 = 256 * cus, round4 = 128 * cus;
    const int64_t full8 = rows / round8, rem = rows - full8 * round8;
    const int64_t all8 = (rows + round8 - 1) / round8 * 100, all4 = (rows + round4 - 1) / round4 * X3_W4_TILE_PCT;
    const int64_t split = (full8 > 0 && rem > 0) ? full8 * 100 + (rem + round4 - 1) / round4 * X3_W4_TILE_PCT + X3_SPLIT_LAUNCH_PCT : INT64_MAX;
    if (split < all8 && split < all4) return full8 * round8;
    return all4 < all8 ? 0 : rows;
}

// split-K of the weight gradient: `rows` rows in about n row ranges of equal size, a multiple of 64 rows
struct Split { int nsplit, rows_per_split; };
static inline Split split_evenly(int64_t rows, int64_t n) {
    int64_t rps = ((rows + n - 1) / n + 63) / 64 * 64;
    if (rps < 64) rps = 64;                                   // rows == 0: one empty split
    n = (rows + rps - 1) / rps;
    return Split{(int)(n < 1 ? 1 : n), (int)rps};
}
static inline Split wgrad_splits(int64_t rows) {
    // ~4096 rows per split (measured: 2048 is slower for >= 256 k rows), but at least 25 splits when the
    // pass is small, so that the 10 jobs still fill the 256 CUs (65 k rows: 0.195 -> 0.148 ms) in ONE round of
    // workgroups (round 3 used 26: 260 workgroups, four of them a second round on their own -- the far rows'
    // 32 768-row fp32 passes of round 4 took 0.47 ms that way)
    // (round 4 re-measured the split size on the final kernels, same box: 3072 ... 49152 rows per split move the config-1 step by
    // <= 1 % (6.61-6.72 ms, inside the run-to-run spread) and 16384 costs configs 2 / 4 2-4 %: profiles/r04l_wgrad_rows_per_split.log)
    int64_t n = (rows + 4095) / 4096;
    const int64_t fill = rows / 512 < 25 ? rows / 512 : 25;
    if (n < fill) n = fill;
    if (n < 1) n = 1;
    if (n > 128) n = 128;
    return split_evenly(rows, n);
}
// the split of an active range of `rows_active` rows of a pass of `rows_total`.  wgrad_splits is NOT monotone in its row count
// (12289 rays x 64 samples: 127 splits, a sub-range of 8684 rays: 128), and the workspace's `partial` blocks were sized for the
// whole pass (bwd_ws_layout): never more splits than it holds
static inline Split split_of_range(int64_t rows_total, int64_t rows_active) {
    const Split whole = wgrad_splits(rows_total);
    if (rows_active == rows_total) return whole;
    const Split s = wgrad_splits(rows_active);
    return s.nsplit > whole.nsplit ? split_evenly(rows_active, whole.nsplit) : s;
}

// backward workspace layout
struct BwdWs {
    int64_t grad, d_sigma, d_z, d_len, partial, dp, dv, total;
    int nsplit;               // partial blocks: the split count of the whole pass
};
static inline BwdWs bwd_ws_layout(int af, int nrays, int nsamp, int pose) {          // af: area format of the pass (layout.h)
    BwdWs w;
    const int64_t rows = (int64_t)nrays * nsamp;
    int64_t o = 0;
    w.grad = o; o += align256(grad_area_bytes(af, rows));
    w.d_sigma = o; o += align256(rows * 4);
    w.d_z = o; o += align256(rows * 12);
    w.d_len = o; o += align256((int64_t)nrays * 4);
    w.nsplit = af == AREA_MASKS ? 0 : wgrad_splits(rows).nsplit;          // (a ray-gradient-only pass: no gradient area above, no partial blocks)
    w.partial = o; o += align256((int64_t)w.nsplit * kPartialFloats * 4);
    w.dp = o; if (pose) o += align256(rows * 12);
    w.dv = o; if (pose) o += align256(rows * 128);
    w.total = o;
    return w;
}

// far_count = K > 0: the last K samples of every ray go through far_prec as well (sparf_hip.h "far rows").  far_prec: fp32 only
// (row routing is compiled into the fp32 forward kernels, mlp_fwd_impl.h); main precision: a bf16-plane save layout (bf16, bf16x3)
// far_count = -1: far TILES by value (inference only): 128-row tiles whose largest depth sample exceeds far_thr go to far_prec, the
// others to prec; needs nsamp % 32 == 0 (a 32-row wave tile then lies inside one ray, whose samples increase)
static constexpr bool far_ok(int far_count, int far_prec, int nsamp, int prec) {
    if (far_count == 0) return true;
    if (far_prec != PREC_FP32 || prec == PREC_FP32) return false;
    // tile routing decides per WORKGROUP tile (nwaves x 32 rows): both launches must cut the rows into the same tiles, or a tile of
    // the wider kernel that straddles the threshold would be skipped by it and only half-evaluated by the other (the
    // 8-wave bf16 kernels against the 4-wave fp32 far kernel; bf16x3 runs 4 waves)
    if (far_count == -1) return nsamp % 32 == 0 && nwaves_of(prec) == nwaves_of(far_prec);
    return far_count > 0 && far_count < nsamp;
}

// the nine upstream gradients a segment may carry: where sparf_segment_t holds each and where the kernels' table does
struct SegGrad { const float* sparf_segment_t::*in; const float* (SegTable::*out)[MAX_SEGMENTS]; };
static constexpr SegGrad kSegGrads[] = {
    {&sparf_segment_t::g_rgb, &SegTable::g_rgb}, {&sparf_segment_t::g_depth, &SegTable::g_depth}, {&sparf_segment_t::g_opacity, &SegTable::g_opacity},
    {&sparf_segment_t::g_weights, &SegTable::g_weights}, {&sparf_segment_t::g_depth_var, &SegTable::g_depth_var}, {&sparf_segment_t::g_rgb_var, &SegTable::g_rgb_var},
    {&sparf_segment_t::g_all_cumulated, &SegTable::g_all_cum}, {&sparf_segment_t::g_density, &SegTable::g_density}, {&sparf_segment_t::g_rgb_samples, &SegTable::g_rgb_samples}};
static inline bool seg_active(const sparf_segment_t& s) {            // has rays and an upstream gradient
    if (s.nrays <= 0) return false;
    for (const SegGrad& g : kSegGrads)
        if (s.*g.in) return true;
    return false;
}
// host segment array -> by-value kernel table; false if the segments do not tile [0, nrays) in order
static inline bool seg_table(int nseg, const sparf_segment_t* seg, int nrays, bool grads, SegTable* out) {
    out->n = 0;
    if (nseg == 0) return true;
    if (nseg < 0 || nseg > MAX_SEGMENTS || !seg) return false;
    int next = 0;
    for (int i = 0; i < nseg; ++i) {
        if (seg[i].ray0 != next || seg[i].nrays < 0) return false;
        next += seg[i].nrays;
        out->ray0[i] = seg[i].ray0;
        out->noise_scale[i] = seg[i].noise_scale;
        for (const SegGrad& g : kSegGrads) (out->*g.out)[i] = grads ? seg[i].*g.in : nullptr;
    }
    if (next != nrays) return false;
    // empty segments share their ray0 with the next one: the select chain keeps the LAST match, which is the non-empty one
    out->n = nseg;
    return true;
}

// ---- forward
struct FwdLaunch {                   // one launch_mlp_fwd: on mlp_grid(prec, a.rows) workgroups
    int prec, save;                  // save: FWD_INFER / FWD_SAVE_PLANES / FWD_SAVE_Q8 / FWD_SAVE_MASKS
    MlpFwdArgs a;
};
enum { FAR_NONE = 0, FAR_ROWS, FAR_TILES };
struct FwdPlan {
    FwdLaunch main, far;             // far: only if far_kind
    int far_kind;
    bool masks;                      // ray-gradient-only pass: far rows leave and transplant mask words only
    bool far_setup;                  // a launch_ray_setup of its own for the far launch, into far_venc_ws (the per-ray view-encoding rows
                                     // are laid out per precision: element type AND 16-byte-chunk order, ray_setup_kernel)
    CompositeFwdArgs c;
};
static inline MlpFwdArgs mlp_fwd_args(const sparf_pass_fwd_t* p) {
    return MlpFwdArgs{(const char*)p->packed, p->c2f, p->center, p->dir, p->venc_ws, p->t, (int64_t)p->nrays * p->nsamp, p->nsamp,
                      p->sigma_raw, p->rgb_samples, p->save};
}
// -> ABI status code; 0 with nrays == 0: nothing to launch (the plan is not filled)
static inline int plan_forward(const sparf_pass_fwd_t* p, FwdPlan* f) {
    if (!p) return 1;
    const PassPrec pp = pass_prec(p->prec);
    const int prec = pp.base;
    if (!pp.ok || p->nrays < 0 || p->nsamp <= 0) return 1;
    if (pp.q8 && p->far_count > 0) return 1;           // far rows are transplanted into plane save areas only
    if (p->nrays == 0) return 0;
    if (!rows_ok((int64_t)p->nrays * p->nsamp)) return 4;
    if (!p->center || !p->dir || !p->t || !p->packed || !p->c2f || !p->venc_ws || !p->raylen || !p->sigma_raw || !p->rgb_samples ||
        !p->density || !p->weights || !p->rgb || !p->depth || !p->opacity || !p->depth_var || !p->rgb_var || !p->all_cumulated)
        return 1;
    if (!far_ok(p->far_count, p->far_prec, p->nsamp, prec)) return 1;
    if (p->far_count && (!p->far_packed || (p->save != nullptr && !p->far_ws) || (p->far_prec != prec && !p->far_venc_ws))) return 1;
    if (p->far_count == -1 && p->save != nullptr) return 1;            // tile routing: inference passes only
    f->masks = pp.masks;
    f->main = FwdLaunch{prec, p->save ? pp.save : (int)FWD_INFER, mlp_fwd_args(p)};
    f->far_kind = p->far_count == 0 ? FAR_NONE : p->far_count == -1 ? FAR_TILES : FAR_ROWS;
    f->far_setup = f->far_kind != FAR_NONE && p->far_prec != prec;
    f->far = FwdLaunch{p->far_prec, FWD_INFER, f->main.a};
    MlpFwdArgs& a = f->far.a;
    a.packed = (const char*)p->far_packed;
    if (f->far_setup) a.venc = p->far_venc_ws;
    a.save = nullptr;
    if (f->far_kind == FAR_TILES) {
        // far tiles by value: the main launch takes the tiles whose depth samples all stay below the threshold, the far precision's
        // inference kernel the others (every tile is evaluated by exactly one of the two launches; the one that skips a tile spends
        // four loads on it)
        f->main.a.tile_thr = a.tile_thr = p->far_thr;
        f->main.a.tile_take = 1;
        a.tile_take = 2;
    } else if (f->far_kind == FAR_ROWS) {
        // far rows: the last K samples of every ray once more, through the far precision's kernels, as a pass of nrays K-sample
        // rays whose outputs land on the main launch's (stream order: they replace what it wrote there); in a training pass what
        // the far launch saved -- activations and ReLU masks -- is then transplanted into the main save area, so that the backward
        // of the pass (bf16-operand arithmetic for every row) differentiates the forward that was actually composited
        a.rows = (int64_t)p->nrays * p->far_count;
        a.nsamp = p->far_count;
        a.row_stride = p->nsamp;
        a.row_off = p->nsamp - p->far_count;
        // (a ray-gradient-only pass: the far precision's masks-only kernel, far_ws an AREA_MASKS area of nrays * K rows)
        if (p->save) { a.save = p->far_ws; f->far.save = pp.masks ? FWD_SAVE_MASKS : FWD_SAVE_PLANES; }
    }
    f->c = CompositeFwdArgs{p->nrays, p->nsamp, p->t, p->sigma_raw, p->noise, p->noise_scale, p->rgb_samples, p->raylen, p->white_bg,
                            p->weights, p->density, p->rgb, p->depth, p->opacity, p->depth_var, p->rgb_var, p->all_cumulated, {}};
    return seg_table(p->nseg, p->seg, p->nrays, false, &f->c.seg) ? 0 : 1;
}

// ---- backward
struct BwdLaunch {                   // one launch_mlp_bwd of kernel k: on mlp_grid(k->prec, n) workgroups
    const MlpBwdKernel* k;
    MlpBwdArgs a;
    int64_t n;                       // rows of the launch
};
struct BwdPlan {
    PassPrec pp;
    bool pose;                       // ray gradients wanted (d_center and d_dir); always, in a ray-gradient-only pass (pp.masks)
    int64_t rows;                    // of the whole pass; 0: empty batch, nothing below is filled
    int ray0, ray1;                  // active rays [ray0, ray1) and their rows [row0, row1): what the kernels run over
    int64_t row0, row1;
    bool no_grad;                    // segmented pass none of whose segments has an upstream gradient: every result is zero
    BwdWs ws;
    Split split;                     // of the active rows (never more splits than ws holds partial blocks)
    CompositeBwdArgs c;
    MlpBwdArgs m;                    // data gradient over all active rows, cut into
    BwdLaunch dgrad[2];              // its ndgrad launches (plan_dgrad)
    int ndgrad;
    WgradArgs g;
    RayReduceArgs r;                 // only if pose
};
// The data-gradient launches of a plan over its active rows.  A mode whose kernel comes in two geometries (kernels.h: bf16x3 over plane or
// masks-only areas) sends the leading x3_dgrad_rows8 rows through the 8-wave one and the rest, if any, through the 4-wave one behind it;
// every other mode all rows through the one it has.  `pin` (measurement: sparf_launch_kernel 3 / 4) = 8 | 4 forces one of the two for
// the whole range; 0: the plan's choice.
static inline void plan_dgrad(BwdPlan* b, int pin) {
    const MlpBwdKernel *k8 = find_mlp_bwd(b->pp.base, b->pose, 8, b->pp.save), *k4 = find_mlp_bwd(b->pp.base, b->pose, 4, b->pp.save);
    const int64_t rows = b->row1 - b->row0;
    const int64_t rows8 = !k4 ? rows : !k8 ? 0 : pin == 8 ? rows : pin == 4 ? 0 : x3_dgrad_rows8(rows);
    b->ndgrad = 0;
    if (rows8 > 0) {
        BwdLaunch& l = b->dgrad[b->ndgrad++] = BwdLaunch{k8, b->m, rows8};
        l.a.rows = b->row0 + rows8;
    }
    if (rows8 < rows) {
        BwdLaunch& l = b->dgrad[b->ndgrad++] = BwdLaunch{k4, b->m, rows - rows8};
        l.a.row_begin = b->row0 + rows8;
    }
}
// -> ABI status code.  whole_pass (sparf_launch_kernel): the kernels cover rows [0, nrays * nsamp) whatever the segment table says;
// pin: plan_dgrad's
static inline int plan_backward(const sparf_pass_bwd_t* p, bool whole_pass, BwdPlan* b, int pin = 0) {
    if (!p) return 1;
    const PassPrec pp = b->pp = pass_prec(p->prec);
    if (!pp.ok || p->nrays < 0 || p->nsamp <= 0) return 1;
    const int64_t rows = b->rows = (int64_t)p->nrays * p->nsamp;
    if (p->nrays == 0) return p->grad_params || pp.masks ? 0 : 1;         // empty batch: zero parameter gradients (ray-gradient-only: nothing)
    if (!rows_ok(rows)) return 4;
    const bool pose = b->pose = p->d_center != nullptr;
    if (pose != (p->d_dir != nullptr)) return 1;
    if (pp.masks && !pose) return 1;                          // a ray-gradient-only pass without ray gradients
    if (!p->center || !p->dir || !p->t || !p->packed || !p->c2f || !p->tables || !p->save || !p->raylen || !p->sigma_raw ||
        !p->rgb_samples || !p->weights || !p->ws || (!p->grad_params && !pp.masks))
        return 1;
    const BwdWs& w = b->ws = bwd_ws_layout(pp.af, p->nrays, p->nsamp, pose);
    char* ws = (char*)p->ws;
    float *d_sigma = (float*)(ws + w.d_sigma), *d_z = (float*)(ws + w.d_z), *d_len = (float*)(ws + w.d_len);
    float *dp = (float*)(ws + w.dp), *dv = (float*)(ws + w.dv);
    CompositeBwdArgs& c = b->c;
    c = CompositeBwdArgs{p->nrays, p->nsamp, p->t, p->sigma_raw, p->noise, p->noise_scale, p->rgb_samples, p->raylen, p->weights,
                         p->white_bg, p->g_rgb, p->g_depth, p->g_opacity, p->g_weights, d_sigma, d_z, pose ? d_len : nullptr, {}, 0};
    c.g_depth_var = p->g_depth_var; c.g_rgb_var = p->g_rgb_var; c.g_all_cum = p->g_all_cumulated;
    c.g_density = p->g_density; c.g_rgb_samples = p->g_rgb_samples;
    if (!seg_table(p->nseg, p->seg, p->nrays, true, &c.seg)) return 1;
    // Active ray range of a segmented pass: the segments that received an upstream gradient.  Rays are independent, so a
    // segment without one contributes nothing to any gradient; issued as separate calls autograd would not even call its
    // backward (the coarse pass of a correspondence render whose loss reads depth_fine only).  The backward kernels run
    // over the covering range [first active segment, last active segment] when that range starts on a 32-row tile.
    b->ray0 = 0; b->ray1 = p->nrays; b->no_grad = false;
    if (p->nseg > 0 && !whole_pass) {
        int first = -1, last = -1;
        for (int i = 0; i < p->nseg; ++i)
            if (seg_active(p->seg[i])) {
                if (first < 0) first = i;
                last = i;
            }
        b->no_grad = first < 0;
        if (b->no_grad) return 0;
        b->ray0 = p->seg[first].ray0;
        b->ray1 = p->seg[last].ray0 + p->seg[last].nrays;
        if (((int64_t)b->ray0 * p->nsamp) % 32 != 0) b->ray0 = 0;       // (64 / 192 samples per ray: always aligned)
    }
    const int ray0 = b->ray0, ray1 = b->ray1;
    const int64_t row0 = b->row0 = (int64_t)ray0 * p->nsamp, row1 = b->row1 = (int64_t)ray1 * p->nsamp;
    c.ray_base = ray0;
    c.nrays = ray1 - ray0;
    b->split = split_of_range(rows, row1 - row0);
    b->m = MlpBwdArgs{(const char*)p->packed, p->c2f, p->center, p->dir, p->t, row1, p->nsamp, p->save, ws + w.grad, d_sigma, d_z, dp, dv, row0, rows};
    plan_dgrad(b, pin);
    b->g = WgradArgs{p->save, ws + w.grad, row1, b->split.rows_per_split, (float*)(ws + w.partial), row0};
    if (pose) {
        b->r = RayReduceArgs{ray1 - ray0, p->nsamp, p->t, dp, dv, p->dir, p->raylen, d_len, p->c2f + 10, p->d_center, p->d_dir, ray0};
        b->r.accumulate = p->accumulate_rays;
    }
    return 0;
}

// A plan that succeeds names only kernels that exist (kernels.h): every precision id pass_prec accepts has its inference and its
// training forward and, with and without pose gradients (ray-gradient-only: with), a data-gradient kernel in one of the two geometries
// plan_dgrad looks for; every far precision far_ok accepts has the forwards a far launch can be (inference, plane saves, mask words).
constexpr bool plan_kernels_exist() {
    const int flags[] = {0, SPARF_SAVE_Q8, SPARF_SAVE_MASKS};
    for (int base = 0; base < N_PREC; ++base) {
        for (int f : flags) {
            const PassPrec pp = pass_prec(base | f);
            if (!pp.ok) continue;
            if (!find_mlp_fwd(base, FWD_INFER) || !find_mlp_fwd(base, pp.save)) return false;
            for (int pose = pp.masks ? 1 : 0; pose < 2; ++pose)
                if (!find_mlp_bwd(base, pose != 0, 8, pp.save) && !find_mlp_bwd(base, pose != 0, 4, pp.save)) return false;
        }
        for (int far = 0; far < N_PREC; ++far)
            if (far_ok(1, far, 2, base) && !(find_mlp_fwd(far, FWD_INFER) && find_mlp_fwd(far, FWD_SAVE_PLANES) && find_mlp_fwd(far, FWD_SAVE_MASKS))) return false;
    }
    return true;
}
static_assert(plan_kernels_exist(), "pass_plan.h accepts a pass for which kernels.h lists no kernel");

}  // namespace sparf
