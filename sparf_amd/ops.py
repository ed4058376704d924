"""torch <-> libsparf_hip glue: tensor allocation, stream hand-off and the autograd
boundary.  PyTorch is plumbing here (device memory, current stream, autograd graph edges);
every FLOP of the hot path runs in the HIP kernels behind the C ABI.
"""
import ctypes
import math
from collections import namedtuple
from ctypes import c_void_p

import torch

from . import lib as L


_C2F_OFF = {}
# what a pass returns, in order, under the reference's composite keys; the C structs call the per-sample density plain `density`
PASS_KEYS = ("rgb", "depth", "opacity", "weights", "depth_var", "rgb_var", "all_cumulated", "density_samples", "rgb_samples")
RENDER_KEYS = PASS_KEYS + ("t",)
_PASS_FIELDS = tuple("density" if k == "density_samples" else k for k in PASS_KEYS)
_GRAD_FIELDS = tuple("g_" + k for k in _PASS_FIELDS)


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


# what the forward of a pass leaves behind for its backward
SAVE_NONE, SAVE_FULL, SAVE_MASKS = "none", "full", "masks"


def save_kind(grad_mode, rays_need_grad, params_need_grad, prec):
    """(grad mode at the call site, the rays need a gradient, any parameter of THIS pass's network needs one, precision id of the pass)
    -> SAVE_NONE: nothing differentiable, the inference kernel runs; SAVE_MASKS: a ray-gradient-only pass (sparf_hip.h
    SPARF_SAVE_MASKS) -- the rays are the pass's only differentiable inputs: pose optimisation against a frozen network; SAVE_FULL: a
    training pass.  The '+q8' precisions keep the full route.  Decided per pass: a frozen coarse network next to a trainable fine one is a
    mixed render."""
    if not grad_mode or not (rays_need_grad or params_need_grad):
        return SAVE_NONE
    if rays_need_grad and not params_need_grad and not (prec & L.SAVE_Q8):
        return SAVE_MASKS
    return SAVE_FULL


def pass_save_kind(grad_mode, rays_need_grad, params_need_grad, prec, any_need_grad):
    """save_kind of one pass of a call, `any_need_grad`: any input of the call needs a gradient -- a pass with no differentiable input
    of its own next to one that has (a frozen network under rays without a gradient beside a trainable one; some other input that
    carries a gradient flag) takes the full route"""
    kind = save_kind(grad_mode, rays_need_grad, params_need_grad, prec)
    return SAVE_FULL if (kind == SAVE_NONE and grad_mode and any_need_grad) else kind


def pass_prec_of(prec, kind):
    """the precision id a pass of save kind `kind` hands the C ABI"""
    return prec | L.SAVE_MASKS if kind == SAVE_MASKS else prec


def has_param_grad(prec):
    """whether the backward of a pass with precision id `prec` computes a parameter gradient: not a ray-gradient-only one"""
    return not (prec & L.SAVE_MASKS)


def pack_weights(params, prec, out=None):
    """params: 20 tensors (W0,b0,...,W9,b9) in nn.Linear layout on one cuda device.
    Returns the packed uint8 blob consumed by the pass kernels."""
    prec = L.base_prec(prec)
    lib = L.load()
    dev = params[0].device
    L.require_gpu(dev)
    for p, (o, i) in zip(params[0::2], L.LAYER_SHAPES):
        if tuple(p.shape) != (o, i):
            raise L.SparfError(f"unsupported architecture: weight {tuple(p.shape)} where {(o, i)} is compiled in "
                               "(8x256 feature MLP with skip at 4, 128-wide colour branch, L_3D=10, L_view=4)")
    ps = [_f32(p) for p in params]
    arr = (c_void_p * 20)(*[p.data_ptr() for p in ps])
    nbytes = lib.sparf_packed_bytes(prec)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tables = L.tables_device(L.base_prec(prec), dev)
    L.call("sparf_pack_weights", dev, prec, arr, L.ptr(tables), L.ptr(out))
    return out


def c2f_weights(progress, barf_c2f, device):
    """The 16-float band-weight vector of one pass (frequency_nerf.py:248-253), computed on the
    device from the CURRENT value of `progress` -- never cached: the reference trainer rewrites
    progress.data every iteration (nerf_trainer.py:273-275), which no version counter sees."""
    L.require_gpu(device)
    if barf_c2f is None:              # no masking: the constant vector, made once per device
        dev = _resolve(device)        # a bare "cuda" must not bind the cache entry to whichever device was current first
        if dev not in _C2F_OFF:       # built on the device (no pageable host->device copy: legal under stream capture)
            v = torch.ones(16, dtype=torch.float32, device=dev)
            v[14:] = 0.0
            _C2F_OFF[dev] = v
        return _C2F_OFF[dev]
    out = torch.empty(16, dtype=torch.float32, device=device)
    prog = _f32(progress).reshape(1).to(device)
    L.call("sparf_c2f_weights", device, L.ptr(prog), 1, float(barf_c2f[0]), float(barf_c2f[1]), L.ptr(out))
    return out


def _resolve(device):
    """torch.device with an index: the reference trainer hands Graph a bare 'cuda' (base_trainer.py:109), tensors made on it live
    on 'cuda:<current>'"""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _check_out(out, shape, device):
    if out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or _resolve(out.device) != _resolve(device):
        raise L.SparfError(f"out= must be a dense float32 {tuple(shape)} tensor on {device}")
    return out


def sample_coarse(nrays, nsamp, dmin, scale, inverse, device, jitter=None, u_const=0.5, dmax_ray=None, range_dev=None, out=None):
    """range_dev: optional float32 device tensor {dmin, dmax} (or {dmin}) replacing the floats.
    out: optional [nrays, nsamp] destination (a row slice of a shared ray buffer, Graph.render_batch)."""
    L.require_gpu(device)
    t = torch.empty(nrays, nsamp, dtype=torch.float32, device=device) if out is None else _check_out(out, (nrays, nsamp), device)
    j = _f32(jitter).reshape(nrays, nsamp) if jitter is not None else None
    dm = _f32(dmax_ray).reshape(nrays) if dmax_ray is not None else None
    L.call("sparf_sample_coarse", device, L.ptr(j), float(u_const), L.ptr(dm), L.ptr(range_dev), float(dmin), float(scale), int(bool(inverse)),
           nrays, nsamp, L.ptr(t))
    return t


def _fine_grid(lib, u_mid, dev):
    """(entry point, grid) of a resampling call.  A HOST grid (the reference draws it on the CPU, renderer.py:439) travels in the launch
    arguments: no host -> device copy; one too long for them is copied to the device after all."""
    if u_mid.device.type == "cuda":
        return lib.sparf_sample_fine, u_mid
    if u_mid.numel() > 256:
        return lib.sparf_sample_fine, u_mid.to(dev)
    return lib.sparf_sample_fine_hostgrid, u_mid


def sample_fine(weights, t_coarse, u_mid, dmin, dmax, want_unsorted=False, range_dev=None, out=None):
    """weights, t_coarse [R, Nc]; u_mid [Nf].  Returns (sorted union [R, Nc+Nf], t_fine or None).
    out: optional [R, Nc+Nf] destination for the sorted union."""
    lib = L.load()
    dev = weights.device
    L.require_gpu(dev)
    R, Nc = weights.shape
    Nf = u_mid.numel()
    w, tc, um = _f32(weights), _f32(t_coarse), _f32(u_mid)
    out = torch.empty(R, Nc + Nf, dtype=torch.float32, device=dev) if out is None else _check_out(out, (R, Nc + Nf), dev)
    tf = torch.empty(R, Nf, dtype=torch.float32, device=dev) if want_unsorted else None
    fn, um = _fine_grid(lib, um, dev)
    with L.on(dev):
        L.check(fn(L.ptr(w), L.ptr(tc), L.ptr(um), L.ptr(range_dev), float(dmin), float(dmax), R, Nc, Nf, L.ptr(tf),
                   L.ptr(out), L.stream_ptr(dev)), "sparf_sample_fine")
    return out, tf


def _segments(a, segs, grads=None):
    """the segment table of the pass struct `a`: a ctypes array of sparf_segment_t from [(ray0, nrays, noise_scale), ...] (+ per-segment
    upstream gradients), set on `a` and returned for the caller to keep alive"""
    if len(segs) > L.MAX_SEGMENTS:
        raise L.SparfError(f"at most {L.MAX_SEGMENTS} ray segments per pass")
    arr = (L.Segment * len(segs))()
    for i, (r0, n, ns) in enumerate(segs):
        arr[i].ray0, arr[i].nrays, arr[i].noise_scale = int(r0), int(n), float(ns)
        for k, x in zip(_GRAD_FIELDS, grads[i] if grads is not None else ()):
            setattr(arr[i], k, x.data_ptr() if x is not None else None)
    a.nseg, a.seg = len(segs), arr
    return arr


def _venc_bytes(prec, R):
    """view-encoding workspace of a pass over R rays: 32 values per ray in the operand format of `prec`"""
    return R * 32 * (2 if L.base_prec(prec) == L.PREC_BF16 else 4)


def _fill_pass_fwd(*, prec, nrays, nsamp, center, dir, t, noise, noise_scale, white_bg, packed, c2f, save, venc_ws,
                   raylen, sigma_raw, rgb_samples, density, weights, rgb, depth, opacity, depth_var, rgb_var, all_cumulated):
    """sparf_pass_fwd_t from addresses (int | None) and scalars: the ONE place that names its fields, all required keywords -- a field
    a route forgets is a TypeError, not a null pointer.  Segment table and far rows are set on the result (prepare_pass_fwd)."""
    return L.PassFwd(prec=prec, nrays=nrays, nsamp=nsamp, center=center, dir=dir, t=t, noise=noise, noise_scale=float(noise_scale),
                     white_bg=int(bool(white_bg)), packed=packed, c2f=c2f, save=save, venc_ws=venc_ws, raylen=raylen, sigma_raw=sigma_raw,
                     rgb_samples=rgb_samples, density=density, weights=weights, rgb=rgb, depth=depth, opacity=opacity, depth_var=depth_var,
                     rgb_var=rgb_var, all_cumulated=all_cumulated)


def _fill_pass_bwd(*, prec, nrays, nsamp, center, dir, t, noise, noise_scale, white_bg, packed, c2f, tables, save, raylen, sigma_raw,
                   rgb_samples, weights, ws, grad_params, d_center, d_dir, g_rgb, g_depth, g_opacity, g_weights, g_depth_var, g_rgb_var,
                   g_all_cumulated, g_density, g_rgb_samples, accumulate_rays=0):
    """sparf_pass_bwd_t, as _fill_pass_fwd; the nine upstream gradients (_GRAD_FIELDS) are None where an output has none"""
    return L.PassBwd(prec=prec, nrays=nrays, nsamp=nsamp, center=center, dir=dir, t=t, noise=noise, noise_scale=float(noise_scale),
                     white_bg=int(bool(white_bg)), packed=packed, c2f=c2f, tables=tables, save=save, raylen=raylen, sigma_raw=sigma_raw,
                     rgb_samples=rgb_samples, weights=weights, g_rgb=g_rgb, g_depth=g_depth, g_opacity=g_opacity, g_weights=g_weights, ws=ws,
                     grad_params=grad_params, d_center=d_center, d_dir=d_dir, g_depth_var=g_depth_var, g_rgb_var=g_rgb_var,
                     g_all_cumulated=g_all_cumulated, g_density=g_density, g_rgb_samples=g_rgb_samples, accumulate_rays=accumulate_rays)


def _addr(x):
    return x.data_ptr() if x is not None else None


def _contig32(g):
    return g if (g.dtype is torch.float32 and g.is_contiguous()) else g.detach().to(torch.float32).contiguous()


def prepare_pass_fwd(prec, R, N, dev, *, save, noise_scale, white_bg, segs=None, far=None, **addr):
    """Everything of a sparf_pass_forward call but the pass's inputs and results, whose addresses (int | None) the caller hands over as
    `addr`: center, dir, t, noise, packed, c2f and the eleven results of _PASS_F32.  -> (struct, save area | None, what to keep alive
    until the stream has run the call: the caching allocator hands it out again in stream order).
    prec: the pass precision id, with SAVE_MASKS for a ray-gradient-only pass (pass_save_kind, pass_prec_of): the save area is then the
    mask words only.  save: whether the pass saves for a backward.
    segs: optional [(ray0, nrays, noise_scale), ...] ray segments (include/sparf_hip.h sparf_segment_t).
    far: optional (K, far_prec, address of the far_prec packed weights) -- the last K samples of every ray also run through far_prec
    (sparf_hip.h "far rows"); what the far launch saves is transplanted into the pass's save area by the call, its own area is scratch
    (of the far precision's masks-only format when `prec` carries SAVE_MASKS) -- or (threshold, ...) with a FLOAT threshold: far TILES
    by value, inference passes only (far_count = -1)."""
    lib = L.load()
    save_buf = torch.empty(lib.sparf_save_bytes(prec, R * N), dtype=torch.uint8, device=dev) if save else None
    venc = torch.empty(_venc_bytes(prec, R), dtype=torch.uint8, device=dev)
    a = _fill_pass_fwd(prec=prec, nrays=R, nsamp=N, noise_scale=noise_scale, white_bg=white_bg, save=_addr(save_buf), venc_ws=venc.data_ptr(), **addr)
    keep = [venc]
    if segs:
        keep.append(_segments(a, segs))
    if far is not None:
        k, fprec, fpacked = far
        if isinstance(k, float):
            if save or N % 32 != 0:
                raise L.SparfError("far tiles by value: inference passes with a multiple of 32 samples per ray only")
            a.far_count, a.far_thr = -1, k
        else:
            if not 0 < k < N:
                raise L.SparfError(f"far rows: 0 < K < samples per ray, got K = {k} of {N}")
            if save:
                far_ws = torch.empty(lib.sparf_save_bytes(fprec | (prec & L.SAVE_MASKS), R * k), dtype=torch.uint8, device=dev)
                a.far_ws = far_ws.data_ptr()
                keep.append(far_ws)
            a.far_count = int(k)
        a.far_prec, a.far_packed = int(fprec), fpacked
        if fprec != L.base_prec(prec):              # the view-encoding rows are laid out per precision: the far launch gets its own
            fvenc = torch.empty(_venc_bytes(fprec, R), dtype=torch.uint8, device=dev)
            a.far_venc_ws = fvenc.data_ptr()
            keep.append(fvenc)
    return a, save_buf, keep


def prepare_pass_bwd(prec, R, N, dev, *, grads, grad_params, d_center, d_dir, noise_scale, white_bg, accumulate_rays=0, segs=None, **addr):
    """Everything of a sparf_pass_backward call but the addresses (int | None) of what its forward read and left behind, handed over as
    `addr` (center, dir, t, noise, packed, c2f, save, raylen, sigma_raw, rgb_samples, weights), and of its results: grad_params
    [N_PARAMS] (ignored by a ray-gradient-only pass -- `prec` with SAVE_MASKS, has_param_grad: it computes none), d_center, d_dir [R,3]
    (both None: no ray gradients; accumulate_rays = 1: the call adds to them).  -> (struct, what to keep alive).
    grads = (g_rgb, g_depth, g_opacity, g_weights[, g_depth_var, g_rgb_var, g_all_cumulated, g_density, g_rgb_samples]) tensors, any
    may be None; with `segs` a list of such tuples, one per ray segment (each tensor covering only its segment's rays).  They are made
    dense float32 here."""
    dense = lambda gt: [_contig32(g) if g is not None else None for g in gt]
    gseg = [dense(gt) for gt in grads] if segs else None
    gs = dense(grads) if not segs else []       # (segmented: the table carries them)
    gs += [None] * (9 - len(gs))
    ws = torch.empty(L.load().sparf_bwd_workspace_bytes(prec, R, N, int(d_center is not None)), dtype=torch.uint8, device=dev)
    tables = L.tables_device(L.base_prec(prec), dev)
    a = _fill_pass_bwd(prec=prec, nrays=R, nsamp=N, noise_scale=noise_scale, white_bg=white_bg, tables=tables.data_ptr(), ws=ws.data_ptr(),
                       grad_params=grad_params if has_param_grad(prec) else None, d_center=d_center, d_dir=d_dir, accumulate_rays=accumulate_rays,
                       **addr, **{k: _addr(g) for k, g in zip(_GRAD_FIELDS, gs)})
    keep = [ws, tables] + gs
    if segs:
        keep += [_segments(a, segs, gseg), gseg]
    return a, keep


def build_pass_fwd(prec, c, d, tt, nz, noise_scale, white_bg, packed, c2f, save, segs=None, far=None):
    """Allocate outputs and fill the C struct of sparf_pass_forward (prepare_pass_fwd).  Returns
    (struct, outputs dict, save buffer or None, scratch list to keep alive).
    far: optional (K | threshold, far_prec, far_packed tensor)."""
    dev = c.device
    R, N = tt.shape
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    out = dict(raylen=f(R), sigma_raw=f(R, N), rgb_samples=f(R, N, 3), density=f(R, N), weights=f(R, N), rgb=f(R, 3),
               depth=f(R), opacity=f(R), depth_var=f(R), rgb_var=f(R), all_cumulated=f(R))
    a, save_buf, keep = prepare_pass_fwd(prec, R, N, dev, save=save, noise_scale=noise_scale, white_bg=white_bg, segs=segs,
                                         far=(far[0], far[1], far[2].data_ptr()) if far is not None else None, center=c.data_ptr(),
                                         dir=d.data_ptr(), t=tt.data_ptr(), noise=_addr(nz), packed=packed.data_ptr(), c2f=c2f.data_ptr(),
                                         **{k: v.data_ptr() for k, v in out.items()})
    return a, out, save_buf, keep


def build_pass_bwd(prec, c, d, tt, nz, noise_scale, white_bg, packed, c2f, save, fwd_out, grads, pose, segs=None):
    """Allocate the results and fill the C struct of sparf_pass_backward (prepare_pass_bwd: `grads`, `segs`).  Returns
    (struct, gp, dc, dd, keep): the parameter gradient [N_PARAMS] (None for a ray-gradient-only pass) and, with `pose`, the gradients
    of the ray origins and directions."""
    dev = c.device
    R, N = tt.shape
    gp = torch.empty(L.N_PARAMS, dtype=torch.float32, device=dev) if has_param_grad(prec) else None
    dc = torch.empty(R, 3, dtype=torch.float32, device=dev) if pose else None
    dd = torch.empty(R, 3, dtype=torch.float32, device=dev) if pose else None
    a, keep = prepare_pass_bwd(prec, R, N, dev, grads=grads, grad_params=_addr(gp), d_center=_addr(dc), d_dir=_addr(dd), noise_scale=noise_scale,
                               white_bg=white_bg, segs=segs, center=_addr(c), dir=_addr(d), t=_addr(tt), noise=_addr(nz), packed=_addr(packed),
                               c2f=_addr(c2f), save=_addr(save), **{k: _addr(fwd_out[k]) for k in ("raylen", "sigma_raw", "rgb_samples", "weights")})
    return a, gp, dc, dd, keep


def _param_grad_views(gp, shapes, needs):
    """the flat parameter gradient cut into the parameters' shapes: views of it, None where no gradient is wanted"""
    views, off = [], 0
    for shp, need in zip(shapes, needs):
        n = math.prod(shp)
        views.append(gp[off:off + n].view(shp) if need else None)
        off += n
    return views


class NerfPass(torch.autograd.Function):
    """One network (coarse or fine) over R rays x N samples: fused MLP + compositing.

    Inputs  center [R,3], dirs [R,3], t [R,N], noise [R,N] | None, then the 20 parameter
            tensors (only used to route gradients; the kernels read `packed`).
    Outputs rgb [R,3], depth [R], opacity [R], weights [R,N], depth_var [R], rgb_var [R], all_cumulated [R], density [R,N],
            rgb_samples [R,N,3] (PASS_KEYS) -- ALL differentiable, as in the reference, where NeRF.composite is plain autograd
            (frequency_nerf.py:317-338; C ABI 6.  Rounds 1-4 marked the last five non-differentiable: a loss on depth_var
            silently received a zero gradient, VERDICT r04 missing-3).
    segs    None, or [(ray0, nrays, noise_scale), ...]: the rays of SEVERAL render calls laid back to back, one launch
            set.  The nine outputs are then returned PER SEGMENT as views of the pass's buffers (no split copies), the upstream gradients
            consumed per segment through the C ABI's segment table (no gather copies); the noise scales are the table's, `noise_scale`
            is not used.  (One segment is not the same call as none: the C side then walks the active ray range.)
    """

    @staticmethod
    def forward(ctx, center, dirs, t, noise, noise_scale, white_bg, prec, packed, c2f, grad_mode, far, segs, *params):
        dev = center.device
        L.require_gpu(dev)
        c, d, tt = _f32(center), _f32(dirs), _f32(t)
        nz = _f32(noise) if noise is not None else None
        noise_scale = 0.0 if segs else float(noise_scale)
        # needs_input_grad ignores the caller's grad mode (and forward() itself always runs with
        # grad disabled): `grad_mode` = torch.is_grad_enabled() at the call site.  Without it
        # nothing is saved and the inference kernel runs.
        kind = pass_save_kind(bool(grad_mode), ctx.needs_input_grad[0] or ctx.needs_input_grad[1], any(ctx.needs_input_grad[12:]), prec,
                              any(ctx.needs_input_grad))
        need_grad = kind != SAVE_NONE
        prec = pass_prec_of(prec, kind)
        ctx.set_materialize_grads(False)          # absent upstream gradients arrive as None, not as zero tensors
        a, out, save, _keep = build_pass_fwd(prec, c, d, tt, nz, noise_scale, white_bg, packed, c2f, need_grad, segs=segs, far=far)
        L.call("sparf_pass_forward", dev, ctypes.byref(a))
        if need_grad:       # (far rows leave nothing of their own behind: their saves were transplanted into `save`)
            ctx.save_for_backward(c, d, tt, nz, packed, c2f, save, out["raylen"], out["sigma_raw"], out["rgb_samples"], out["weights"])
            ctx.meta = (noise_scale, int(bool(white_bg)), prec, [tuple(p.shape) for p in params], list(segs) if segs else None)
        whole = [out[k] for k in _PASS_FIELDS]
        return tuple(x[r0:r0 + n] for (r0, n, _) in segs for x in whole) if segs else tuple(whole)

    @staticmethod
    def backward(ctx, *g):
        c, d, tt, nz, packed, c2f, save, raylen, sigma_raw, rgb_samples, weights = ctx.saved_tensors
        noise_scale, white_bg, prec, shapes, segs = ctx.meta
        pose = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        fwd_out = dict(raylen=raylen, sigma_raw=sigma_raw, rgb_samples=rgb_samples, weights=weights)
        if segs:
            g = [g[9 * i:9 * i + 9] for i in range(len(segs))]
        a, gp, dc, dd, _keep = build_pass_bwd(prec, c, d, tt, nz, noise_scale, white_bg, packed, c2f, save, fwd_out, g, pose, segs=segs)
        L.call("sparf_pass_backward", c.device, ctypes.byref(a))
        return (dc if ctx.needs_input_grad[0] else None, dd if ctx.needs_input_grad[1] else None, None, None, None, None, None,
                None, None, None, None, None, *_param_grad_views(gp, shapes, ctx.needs_input_grad[12:]))


def nerf_pass_segments(center, dirs, t, noise, white_bg, prec, packed, c2f, params, segs, far=None):
    """-> list (one per segment) of dicts with the reference's composite keys (flat ray axis)"""
    flat = NerfPass.apply(center, dirs, t, noise, 0.0, white_bg, prec, packed, c2f, torch.is_grad_enabled(), far, list(segs), *params)
    return [dict(zip(PASS_KEYS, flat[9 * i:9 * i + 9])) for i in range(len(segs))]


def nerf_pass(center, dirs, t, noise, noise_scale, white_bg, prec, packed, c2f, params, far=None):
    """Convenience wrapper returning a dict with the reference's composite keys (flat ray axis).
    c2f: the pass's band-weight vector (c2f_weights).  far: (K, far_prec, far_packed) or None (build_pass_fwd)."""
    return dict(zip(PASS_KEYS, NerfPass.apply(center, dirs, t, noise, noise_scale, white_bg, prec, packed, c2f, torch.is_grad_enabled(),
                                              far, None, *params)))


def ray_request(B, pixels, ray_idx, all_rays=None):
    """(per_image, N, ray_idx) of a request for rays of B poses, without generating them: N rays per image, selected by pixels [N,2] |
    [B,N,2], else by ray_idx [N] | [B,N], else all `all_rays` = H*W of them.  A 2-D ray_idx whose first dimension is not the batch is
    one list for every image: it comes back flattened."""
    if pixels is not None:
        return int(pixels.dim() == 3), pixels.shape[-2], None
    if ray_idx is None:
        return 0, all_rays, None
    if ray_idx.dim() == 2 and ray_idx.shape[0] != B:
        ray_idx = ray_idx.reshape(-1)
    return int(ray_idx.dim() == 2), ray_idx.shape[-1], ray_idx


def _ray_sel(pose, pixels, ray_idx):
    """(sel tensor, is_pixels, per_image, N) of a ray-generation request"""
    per_image, N, ray_idx = ray_request(pose.shape[0], pixels, ray_idx)
    if pixels is not None:
        sel = _f32(pixels)
        if per_image and sel.shape[0] != pose.shape[0]:
            raise ValueError("per-image pixels must have one row per pose")
    else:
        sel = ray_idx.to(device=pose.device, dtype=torch.int64).contiguous()
    return sel, pixels is not None, per_image, N


def _ray_gen_launch(P, K, sel, is_px, per_image, width, B, N, center, ray):
    Pp = L.ptr
    L.call("sparf_ray_gen_forward", P.device, Pp(P), Pp(K), Pp(sel if is_px else None), Pp(None if is_px else sel), per_image, int(width), B, N,
           Pp(center), Pp(ray))


def _ray_gen_pose_grad(P, K, sel, is_px, per_image, width, B, N, g_center, g_ray):
    if g_center is None and g_ray is None:
        return None
    gc = _f32(g_center) if g_center is not None else None
    gr = _f32(g_ray) if g_ray is not None else None
    d_pose = torch.empty(B, 3, 4, device=P.device, dtype=torch.float32)
    Pp = L.ptr
    L.call("sparf_ray_gen_backward", P.device, Pp(P), Pp(K), Pp(sel if is_px else None), Pp(None if is_px else sel), per_image, int(width), B, N,
           Pp(gc), Pp(gr), Pp(d_pose))
    return d_pose


def _ray_gen_pixel_grad(P, K, per_image, B, N, g_ray, pix_shape):
    """d loss / d pixels of ray generation: ray = R^T K^-1 [x, y, 1] (camera.py:296-306, 321-326, 400-406), so
    d/d(x, y) = (K^-1[:, :2])^T R d/d ray; the ray origin does not depend on the pixel.  The reference's ray generation is
    plain autograd and the depth-consistency loss hands it pixel coordinates that DO carry a gradient (projections of points
    back-projected with a rendered depth, depth_cons_loss.py:199-201, 254-262 -> :291: nothing is detached), so the gradient
    flows on into the reference render that produced that depth.  Two small batched matrix products in PyTorch: K^-1 in
    float64 as the fused kernel uses it."""
    if g_ray is None:
        return None
    from .camera import _intr_inverse
    R = P[:, :, :3]
    Kinv = _intr_inverse(K)
    dg = g_ray.reshape(B, N, 3) @ R.transpose(-1, -2)              # R . d ray, as row vectors
    dxy = dg @ Kinv[:, :, :2]                                      # [B, N, 2]
    return dxy.reshape(pix_shape) if per_image else dxy.sum(0).reshape(pix_shape)


class RayGen(torch.autograd.Function):
    """Ray origins / directions for the selected pixels of every image in one launch
    (replaces camera.get_center_and_ray[_at_pixels], camera.py:347-416).

    pose [B,3,4] w2c (differentiable), intr [B,3,3] (no gradient), pixels [N,2] | [B,N,2]
    float (x, y) OR ray_idx [N] | [B,N] int64 flat indices (pixel centres, +0.5).
    Returns center, ray [B,N,3]."""

    @staticmethod
    def forward(ctx, pose, intr, pixels, ray_idx, width):
        dev = pose.device
        L.require_gpu(dev)
        B = pose.shape[0]
        P, K = _f32(pose), _f32(intr)
        sel, is_px, per_image, N = _ray_sel(pose, pixels, ray_idx)
        center = torch.empty(B, N, 3, device=dev, dtype=torch.float32)
        ray = torch.empty(B, N, 3, device=dev, dtype=torch.float32)
        _ray_gen_launch(P, K, sel, is_px, per_image, width, B, N, center, ray)
        ctx.save_for_backward(P, K, sel)
        ctx.meta = (is_px, per_image, int(width), B, N)
        ctx.pix_shape = tuple(pixels.shape) if pixels is not None else None
        ctx.set_materialize_grads(False)
        return center, ray

    @staticmethod
    def backward(ctx, g_center, g_ray):
        P, K, sel = ctx.saved_tensors
        is_px, per_image, width, B, N = ctx.meta
        d_pose = _ray_gen_pose_grad(P, K, sel, *ctx.meta, g_center, g_ray) if ctx.needs_input_grad[0] else None
        d_pix = _ray_gen_pixel_grad(P, K, per_image, B, N, g_ray, ctx.pix_shape) if (is_px and ctx.needs_input_grad[2]) else None
        return d_pose, None, d_pix, None, None


def ray_gen(pose, intr, pixels=None, ray_idx=None, width=0):
    return RayGen.apply(pose, intr, pixels, ray_idx, width)


class RayGenMany(torch.autograd.Function):
    """Ray generation of SEVERAL render requests into ONE [2, R_total, 3] (centres, directions) buffer, each request
    at its row offset (Graph.render_batch): one autograd node, no concatenation; the backward hands
    every request's pose its own gradient from that request's rows of the buffer gradient.
    specs: [(intr, pixels, ray_idx, width), ...]; poses: the matching [B_i,3,4] tensors.
    (Writing the requests into views of a shared buffer with in-place autograd was tried first: a custom Function that
    marks a VIEW dirty drops the history an earlier in-place write gave the base -- the first request's pose lost its
    gradient; reproduced on CPU with plain torch ops around it.)"""

    @staticmethod
    def forward(ctx, specs, *poses):
        dev = poses[0].device
        L.require_gpu(dev)
        reqs, total = [], 0
        for (intr, pixels, ray_idx, width), pose in zip(specs, poses):
            sel, is_px, per_image, N = _ray_sel(pose, pixels, ray_idx)
            B = pose.shape[0]
            reqs.append((_f32(pose), _f32(intr), sel, (is_px, per_image, int(width), B, N), total))
            total += B * N
        rays = torch.empty(2, total, 3, device=dev, dtype=torch.float32)
        for P, K, sel, meta, off in reqs:
            n = meta[3] * meta[4]
            if n > 0:
                _ray_gen_launch(P, K, sel, *meta, rays[0, off:off + n], rays[1, off:off + n])
        ctx.save_for_backward(*[t for r in reqs for t in r[:3]])
        ctx.metas = [(r[3], r[4]) for r in reqs]
        ctx.set_materialize_grads(False)
        return rays

    @staticmethod
    def backward(ctx, g):
        out = [None]
        saved = ctx.saved_tensors
        for i, (meta, off) in enumerate(ctx.metas):
            n = meta[3] * meta[4]
            if g is None or n == 0 or not ctx.needs_input_grad[1 + i]:
                out.append(None)
                continue
            P, K, sel = saved[3 * i:3 * i + 3]
            out.append(_ray_gen_pose_grad(P, K, sel, *meta, g[0, off:off + n], g[1, off:off + n]))
        return tuple(out)


def ray_gen_many(specs, poses):
    """-> rays [2, R_total, 3]; request i occupies rows [off_i, off_i + B_i * N_i) in request order"""
    return RayGenMany.apply(list(specs), *poses)


class PhotometricLoss(torch.autograd.Function):
    """MSE_loss / huber_loss (delta 0.5, x2) of base_losses.py:151-156 on rgb and optionally
    rgb_fine against one target, summed (base_losses.py:303-311): one launch for the loss
    and its gradient seed."""

    @staticmethod
    def forward(ctx, rgb, rgb_fine, target, kind, delta):
        lib = L.load()
        dev = rgb.device
        L.require_gpu(dev)
        p, t = _f32(rgb), _f32(target)
        pf = _f32(rgb_fine) if rgb_fine is not None else None
        if t.numel() != p.numel() or (pf is not None and pf.numel() != p.numel()):
            raise ValueError("photometric_loss: rgb, rgb_fine and target must have the same number of elements")
        loss = torch.empty((), device=dev, dtype=torch.float32)
        need, need_f = ctx.needs_input_grad[0], pf is not None and ctx.needs_input_grad[1]
        d = torch.empty_like(p) if need else None
        df = torch.empty_like(pf) if need_f else None
        P = L.ptr
        ws = torch.empty(int(lib.sparf_photometric_workspace_floats()), device=dev, dtype=torch.float32) if p.numel() > 65536 else None
        L.call("sparf_photometric_loss", dev, P(p), P(pf), P(t), p.numel(), int(kind), float(delta), P(loss), P(d), P(df), P(ws))
        ctx.save_for_backward(d, df)
        ctx.shapes = (rgb.shape, rgb_fine.shape if rgb_fine is not None else None)
        return loss

    @staticmethod
    def backward(ctx, g):
        d, df = ctx.saved_tensors
        return (d.view(ctx.shapes[0]) * g if d is not None else None, df.view(ctx.shapes[1]) * g if df is not None else None,
                None, None, None)


def photometric_loss(rgb, target, rgb_fine=None, huber=False, delta=0.5):
    return PhotometricLoss.apply(rgb, rgb_fine, target, 1 if huber else 0, delta)


# ---------------------------------------------------------------------------------------------- pose parameterisations
def _pose_empty(like, *shape):
    return torch.empty(*shape, device=like.device, dtype=torch.float32)


class Se3Pose(torch.autograd.Function):
    """camera.lie.se3_to_SE3 (camera.py:142-157, the truncated series of :180-205) and, with a base, camera.pose.compose([refine, base])
    (:100-115) in one launch per direction.  xi [n,6] = (w, u), base [n,3,4] or None, want_refine: also return refine [n,3,4].
    -> (pose [n,3,4], refine | None); without a base the pose IS the refinement and refine is None."""

    @staticmethod
    def forward(ctx, xi, base, want_refine):
        dev = xi.device
        L.require_gpu(dev)
        x = _f32(xi)
        b = _f32(base) if base is not None else None
        n = x.shape[0]
        pose = _pose_empty(x, n, 3, 4)
        refine = _pose_empty(x, n, 3, 4) if (want_refine and b is not None) else None
        P = L.ptr
        L.call("sparf_pose_se3_forward", dev, P(x), P(b), n, P(refine), P(pose))
        ctx.save_for_backward(x, b)
        ctx.set_materialize_grads(False)
        return pose, refine

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pose, g_refine):
        x, b = ctx.saved_tensors
        need_xi, need_base = ctx.needs_input_grad[0], b is not None and ctx.needs_input_grad[1]
        if (g_pose is None and g_refine is None) or not (need_xi or need_base):
            return None, None, None
        n = x.shape[0]
        gp = _f32(g_pose) if g_pose is not None else torch.zeros(n, 3, 4, device=x.device, dtype=torch.float32)
        gr = _f32(g_refine) if g_refine is not None else None
        d_xi = _pose_empty(x, n, 6)
        d_base = _pose_empty(x, n, 3, 4) if need_base else None
        P = L.ptr
        L.call("sparf_pose_se3_backward", x.device, P(x), P(b), n, P(gp), P(gr), P(d_xi), P(d_base))
        return d_xi if need_xi else None, d_base, None


class ComposePose(torch.autograd.Function):
    """camera.pose.compose_pair_b_at_a (camera.py:108-115): a, b [n,3,4] -> b o a = [R_b R_a | R_b t_a + t_b]."""

    @staticmethod
    def forward(ctx, a, b):
        dev = a.device
        L.require_gpu(dev)
        pa, pb = _f32(a), _f32(b)
        n = pa.shape[0]
        out = _pose_empty(pa, n, 3, 4)
        P = L.ptr
        L.call("sparf_pose_compose_forward", dev, P(pa), P(pb), n, P(out))
        ctx.save_for_backward(pa, pb)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        pa, pb = ctx.saved_tensors
        if g is None or not any(ctx.needs_input_grad):
            return None, None
        n = pa.shape[0]
        d_a, d_b = _pose_empty(pa, n, 3, 4), _pose_empty(pa, n, 3, 4)
        P = L.ptr
        L.call("sparf_pose_compose_backward", pa.device, P(pa), P(pb), n, P(_f32(g)), P(d_a), P(d_b))
        return d_a if ctx.needs_input_grad[0] else None, d_b if ctx.needs_input_grad[1] else None


class D9Pose(torch.autograd.Function):
    """The 6D rotation model (two_columns.py:42-62 r6d2mat and the concatenation of :177-178): d9 [n,9] = (t, r1, r2) in
    pose_to_d9's order -> [R | t] [n,3,4], or with `invert` camera.pose.invert of it (camera.py:92-98)."""

    @staticmethod
    def forward(ctx, d9, invert):
        dev = d9.device
        L.require_gpu(dev)
        x = _f32(d9)
        n = x.shape[0]
        pose = _pose_empty(x, n, 3, 4)
        P = L.ptr
        L.call("sparf_pose_d9_forward", dev, P(x), int(bool(invert)), n, P(pose))
        ctx.save_for_backward(x)
        ctx.invert = int(bool(invert))
        ctx.set_materialize_grads(False)
        return pose

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None
        n = x.shape[0]
        d_d9 = _pose_empty(x, n, 9)
        P = L.ptr
        L.call("sparf_pose_d9_backward", x.device, P(x), ctx.invert, n, P(_f32(g)), P(d_d9))
        return d_d9, None


# ---------------------------------------------------------------------------------------------- correspondence loss
REPROJ_LOSS_TYPES = {"huber": 0, "l1": 1, "mse": 2, "epe": 3}          # include/sparf_hip.h loss_type


def _reproj_call(name, dev, n, head, opts, outs):
    """one entry point of the correspondence loss on the current stream: the input pointers, n and the options, the
    output pointers, the workspace (above the one-workgroup limit only) -- no host synchronisation, no readback"""
    ws = L.workspace(L.load().sparf_reproj_workspace_bytes(n), dev, torch.float64)
    L.call(name, dev, *map(L.ptr, head), n, *opts, *map(L.ptr, outs), L.ptr(ws))


def _reproj_opts(loss_type, pixel_thresh, depth_thresh):
    if loss_type.lower() not in REPROJ_LOSS_TYPES:
        raise ValueError("Wrong loss type: {}".format(loss_type))
    return (REPROJ_LOSS_TYPES[loss_type.lower()], int(pixel_thresh is not None), float(pixel_thresh or 0.0),
            int(depth_thresh is not None), float(depth_thresh or 0.0))


def _flat(t, n, what, op="correspondence loss", rows="matches"):
    """[n] or [n,1] (or [1,n,1], as a render returns it) -> dense float32 [n]; `op` and `rows` name the caller in the message"""
    if t.numel() != n:
        raise ValueError(f"{op}: {what} has {t.numel()} elements for {n} {rows}")
    return _f32(t).reshape(n)


def _pix(t, op="correspondence loss"):
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError(f"{op}: pixels must be [n,2]")
    return _f32(t)


def _mat(t, shapes, what, op="correspondence loss"):
    """a dense float32 copy of a matrix the kernels read whole: its shape is checked here, the library sees a pointer only"""
    if tuple(t.shape) not in shapes:
        raise ValueError(f"{op}: {what} must be {' or '.join(str(list(x)) for x in shapes)}, got {list(t.shape)}")
    return _f32(t)


def _seed(s, like, g):
    return (s * g).view(like) if s is not None else None


class ReprojLoss(torch.autograd.Function):
    """compute_render_and_repro_loss_w_repro_thres (corres_loss.py:50-95) for one direction i -> j: one library call for the loss, the
    two stats, the valid mask and the gradient seeds of depth_i and T_itoj [4,4]; the backward multiplies the seeds by the upstream
    scalar.  pixel_thresh / depth_thresh None: that check is off.  -> (loss, perc_val_pix_rep, perc_val_depth_rep, valid [n,1] | None)"""

    @staticmethod
    def forward(ctx, pixels_i, depth_i, intr_i, pixels_j, depth_j, intr_j, T_itoj, weights, loss_type, pixel_thresh, depth_thresh, want_valid):
        dev = depth_i.device
        L.require_gpu(dev)
        opts = _reproj_opts(loss_type, pixel_thresh, depth_thresh)
        pi, pj = _pix(pixels_i), _pix(pixels_j)
        n = pi.shape[0]
        if pj.shape[0] != n:
            raise ValueError("correspondence loss: pixels_i and pixels_j must have one row per match")
        K_i, K_j, T = _mat(intr_i, [(3, 3)], "intr_i"), _mat(intr_j, [(3, 3)], "intr_j"), _mat(T_itoj, [(4, 4)], "T_itoj")
        di = _flat(depth_i, n, "depth_i")
        dj = _flat(depth_j, n, "depth_j") if depth_j is not None else None
        w = _flat(weights, n, "weights") if weights is not None else None
        out = torch.empty(4, device=dev, dtype=torch.float32)
        d_di = torch.empty(n, device=dev, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        d_T = torch.empty(4, 4, device=dev, dtype=torch.float32) if ctx.needs_input_grad[6] else None
        valid = torch.empty(n, 1, device=dev, dtype=torch.bool) if want_valid else None
        _reproj_call("sparf_reproj_loss", dev, n, (pi, di, K_i, pj, dj, K_j, T, w), opts, (out, d_di, d_T, valid))
        ctx.save_for_backward(d_di, d_T)
        ctx.depth_shape = depth_i.shape
        loss, pix, dep, _ = out.unbind(0)
        ctx.mark_non_differentiable(*(t for t in (pix, dep, valid) if t is not None))
        return loss, pix, dep, valid

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        d_di, d_T = ctx.saved_tensors
        return (None, _seed(d_di, ctx.depth_shape, g), None, None, None, None, _seed(d_T, (4, 4), g), None, None, None, None, None)


class ReprojPairLoss(torch.autograd.Function):
    """corres_loss.py:183-219 of compute_loss_on_image_pair for one view pair: both compositions of the relative pose, the two (four
    with fine depths) re-projection terms, their mean and the stats in one library call, with the gradient seeds of every depth and of
    both w2c poses [3,4].  -> (loss, perc_val_pix_rep, perc_val_depth_rep, depth_in_corr_loss)"""

    @staticmethod
    def forward(ctx, pixels_self, pixels_other, depth_self, depth_other, depth_fine_self, depth_fine_other, intr_self, intr_other,
                pose_self, pose_other, weights, loss_type, pixel_thresh, depth_thresh):
        dev = depth_self.device
        L.require_gpu(dev)
        opts = _reproj_opts(loss_type, pixel_thresh, depth_thresh)
        if (depth_fine_self is None) != (depth_fine_other is None):
            raise ValueError("correspondence loss: fine depths for one view only")
        ps, po = _pix(pixels_self), _pix(pixels_other)
        n = ps.shape[0]
        if po.shape[0] != n:
            raise ValueError("correspondence loss: pixels_self and pixels_other must have one row per match")
        K = [_mat(t, [(3, 3)], "an intrinsics matrix") for t in (intr_self, intr_other)]
        P = [_mat(t, [(3, 4), (4, 4)], "a w2c pose")[:3].contiguous() for t in (pose_self, pose_other)]
        depths = [depth_self, depth_other, depth_fine_self, depth_fine_other]
        d = [_flat(t, n, "a depth") if t is not None else None for t in depths]
        w = _flat(weights, n, "weights") if weights is not None else None
        out = torch.empty(4, device=dev, dtype=torch.float32)
        seeds = [torch.empty(n, device=dev, dtype=torch.float32) if (t is not None and ctx.needs_input_grad[2 + i]) else None
                 for i, t in enumerate(depths)]
        d_pose = [torch.empty(3, 4, device=dev, dtype=torch.float32) if ctx.needs_input_grad[8 + i] else None for i in range(2)]
        _reproj_call("sparf_reproj_pair_loss", dev, n, (ps, po, *d, *K, *P, w), opts, (out, *seeds, *d_pose))
        ctx.save_for_backward(*seeds, *d_pose)
        ctx.shapes = [t.shape if t is not None else None for t in depths] + [pose_self.shape, pose_other.shape]
        loss, pix, dep, mean = out.unbind(0)
        ctx.mark_non_differentiable(pix, dep, mean)
        return loss, pix, dep, mean

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        saved = ctx.saved_tensors
        grads = [_seed(s, shape, g) for s, shape in zip(saved[:4], ctx.shapes[:4])]
        for s, shape in zip(saved[4:], ctx.shapes[4:]):
            if s is not None and shape[-2] == 4:            # a [4,4] pose: its bottom row is a constant of the composition
                s = torch.cat([s, torch.zeros_like(s[:1])])
            grads.append(s * g if s is not None else None)
        return (None, None, *grads[:4], None, None, *grads[4:], None, None, None, None)


# ---------------------------------------------------------------------------------------------- depth-consistency loss
DCONS_LOSS_TYPES = {"huber": 0, "l1": 1, "mse": 2}          # include/sparf_hip.h: `epe` is not a kernel case


def _dcons_call(name, dev, *args, ws_for=None):
    """one entry point of the depth-consistency loss on the current stream; `ws_for`: the number of points of a call
    that takes a workspace (above the one-workgroup limit only)"""
    tail = ()
    if ws_for is not None:
        tail = (L.ptr(L.workspace(L.load().sparf_dcons_workspace_bytes(ws_for), dev, torch.float64)),)
    L.call(name, dev, *args, *tail)


def _dcons_compacted(dev, n):
    """dst [n], src [room for n], count [1]: the index tensors of an ordered compaction"""
    i32 = lambda k: torch.empty(k, device=dev, dtype=torch.int32)
    return i32(n), i32(n), i32(1)


def _dcons_count(count, n):
    """the one readback of a compaction: 4 bytes, the number of rays of the render that follows"""
    return int(count.item()) if n else 0


def _pose_rows(t, what, op):
    m = _mat(t, [(3, 4), (4, 4)], what, op)
    return m, m.shape[0]


class DconsProject(torch.autograd.Function):
    """depth_cons_loss.py:247-259 (with `points_w` None also :209, batch_backproject_to_3d of pixels_ref [n,2] and depth_ref through
    intr_ref and pose_c2w_ref): batch_project into the unseen view, the five-way mask on the stored values and its selections as one
    ordered compaction.  depth_min: a float or a float32 scalar on the device (then it is never read back).
    -> (pixels [c,2], pseudo_depth [c], index [c] int32: the source row of each output row).  Gradients go to points_w or depth_ref."""

    @staticmethod
    def forward(ctx, points_w, pixels_ref, depth_ref, intr_ref, pose_c2w_ref, pose_w2c_unseen, intr_unseen, H, W, depth_min):
        dev = pose_w2c_unseen.device
        L.require_gpu(dev)
        op = "depth-consistency project"
        P, prows = _pose_rows(pose_w2c_unseen, "pose_w2c_unseen", op)
        K = _mat(intr_unseen, [(3, 3)], "intr_unseen", op)
        if points_w is not None:
            if any(t is not None for t in (pixels_ref, depth_ref, intr_ref, pose_c2w_ref)):
                raise ValueError("depth-consistency project: world points or a back-projection, not both")
            if points_w.dim() != 2 or points_w.shape[1] != 3:
                raise ValueError("depth-consistency project: points_w must be [n,3]")
            head, rrows = (_f32(points_w), None, None, None, None), 0
            n = head[0].shape[0]
        else:
            if any(t is None for t in (pixels_ref, depth_ref, intr_ref, pose_c2w_ref)):
                raise ValueError("depth-consistency project: the back-projection needs pixels_ref, depth_ref, intr_ref and pose_c2w_ref")
            px = _pix(pixels_ref, op)
            n = px.shape[0]
            T, rrows = _pose_rows(pose_c2w_ref, "pose_c2w_ref", op)
            head = (None, px, _flat(depth_ref, n, "depth_ref", op, "points"), _mat(intr_ref, [(3, 3)], "intr_ref", op), T)
        dmin_dev = None
        if isinstance(depth_min, torch.Tensor):
            dmin_dev, depth_min = _f32(depth_min).reshape(1), 0.0
        uv = torch.empty(n, 2, device=dev, dtype=torch.float32)
        z = torch.empty(n, device=dev, dtype=torch.float32)
        dst, src, count = _dcons_compacted(dev, n)
        p = L.ptr
        _dcons_call("sparf_dcons_project", dev, *map(p, head), rrows, p(P), prows, p(K), n, int(H), int(W), float(depth_min), p(dmin_dev),
                    p(uv), p(z), p(dst), p(src), p(count), ws_for=n)
        c = _dcons_count(count, n)
        ctx.save_for_backward(*head, P, K, dst)
        ctx.rows, ctx.shape = (rrows, prows), (points_w if points_w is not None else depth_ref).shape
        ctx.set_materialize_grads(False)
        index = src[:c]
        ctx.mark_non_differentiable(index)
        return uv[:c], z[:c], index

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_uv, g_z, _):
        *head, P, K, dst = ctx.saved_tensors
        if (g_uv is None and g_z is None) or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[2]):
            return (None,) * 10
        dev, n, by_points = dst.device, dst.shape[0], head[0] is not None
        out = torch.empty((n, 3) if by_points else (n,), device=dev, dtype=torch.float32)
        p = L.ptr
        _dcons_call("sparf_dcons_project_backward", dev, *map(p, head), ctx.rows[0], p(P), ctx.rows[1], p(K), n, p(dst),
                    p(_f32(g_uv) if g_uv is not None else None), p(_f32(g_z) if g_z is not None else None),
                    p(out if by_points else None), p(None if by_points else out))
        out = out.view(ctx.shape)
        return (out if by_points else None, None, None if by_points else out) + (None,) * 7


class DconsSelect(torch.autograd.Function):
    """depth_cons_loss.py:277-283: keep = vis >= thresh (an fp32 compare) and the same ordered compaction of pixels [m,2], pseudo_depth
    [m] and vis [m].  -> (pixels [c,2], pseudo_depth [c], vis [c], index [c] int32).  Gradients go to pixels and pseudo_depth."""

    @staticmethod
    def forward(ctx, vis, pixels, pseudo_depth, thresh):
        dev = vis.device
        L.require_gpu(dev)
        op = "visibility select"
        uv = _pix(pixels, op)
        m = uv.shape[0]
        v, z = _flat(vis, m, "vis", op, "points"), _flat(pseudo_depth, m, "pseudo_depth", op, "points")
        uv_o, z_o, v_o = torch.empty_like(uv), torch.empty_like(z), torch.empty_like(v)
        dst, src, count = _dcons_compacted(dev, m)
        p = L.ptr
        _dcons_call("sparf_dcons_select", dev, p(v), p(uv), p(z), m, float(thresh), p(uv_o), p(z_o), p(v_o), p(dst), p(src), p(count), ws_for=m)
        c = _dcons_count(count, m)
        ctx.save_for_backward(dst)
        ctx.shapes = (pixels.shape, pseudo_depth.shape)
        ctx.set_materialize_grads(False)
        vis_out, index = v_o[:c], src[:c]
        ctx.mark_non_differentiable(vis_out, index)
        return uv_o[:c], z_o[:c], vis_out, index

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_uv, g_z, *_):
        dst, = ctx.saved_tensors
        need_uv, need_z = ctx.needs_input_grad[1] and g_uv is not None, ctx.needs_input_grad[2] and g_z is not None
        if not (need_uv or need_z):
            return None, None, None, None
        dev, m = dst.device, dst.shape[0]
        d_uv = torch.empty(m, 2, device=dev, dtype=torch.float32) if need_uv else None
        d_z = torch.empty(m, device=dev, dtype=torch.float32) if need_z else None
        p = L.ptr
        _dcons_call("sparf_dcons_select_backward", dev, p(dst), p(_f32(g_uv) if need_uv else None), p(_f32(g_z) if need_z else None), m, p(d_uv),
                    p(d_z))
        return None, d_uv.view(ctx.shapes[0]) if need_uv else None, d_z.view(ctx.shapes[1]) if need_z else None, None


class DconsLoss(torch.autograd.Function):
    """depth_cons_loss.py:293-312 over the m kept points: w = vis opacity (detached), l = compute_diff_loss(pseudo_depth - depth) with
    weights w, the same on depth_fine / opacity_fine when given, avg_vis_weight of the last term -- one library call that also leaves the
    gradient seeds of pseudo_depth, depth and depth_fine; the backward multiplies them by the upstream scalar.  -> (loss, avg_vis_weight)"""

    @staticmethod
    def forward(ctx, pseudo_depth, vis, depth, opacity, depth_fine, opacity_fine, loss_type):
        dev = depth.device
        L.require_gpu(dev)
        if loss_type.lower() not in DCONS_LOSS_TYPES:
            raise ValueError("Wrong loss type: {}".format(loss_type))
        if (depth_fine is None) != (opacity_fine is None):
            raise ValueError("depth-consistency loss: depth_fine and opacity_fine come together")
        m = pseudo_depth.numel()
        tensors = (pseudo_depth, vis, depth, opacity, depth_fine, opacity_fine)
        names = ("pseudo_depth", "vis", "depth", "opacity", "depth_fine", "opacity_fine")
        head = [_flat(t, m, name, "depth-consistency loss", "points") if t is not None else None for t, name in zip(tensors, names)]
        out = torch.empty(2, device=dev, dtype=torch.float32)
        seeds = [torch.empty(m, device=dev, dtype=torch.float32) if (tensors[i] is not None and ctx.needs_input_grad[i]) else None for i in (0, 2, 4)]
        p = L.ptr
        _dcons_call("sparf_dcons_loss", dev, *map(p, head), m, DCONS_LOSS_TYPES[loss_type.lower()], p(out), *map(p, seeds), ws_for=m)
        ctx.save_for_backward(*seeds)
        ctx.shapes = [tensors[i].shape if tensors[i] is not None else None for i in (0, 2, 4)]
        loss, avg = out.unbind(0)
        ctx.mark_non_differentiable(avg)
        return loss, avg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        d_zp, d_depth, d_fine = (_seed(s, shape, g) for s, shape in zip(ctx.saved_tensors, ctx.shapes))
        return d_zp, None, d_depth, None, d_fine, None, None


# ---------------------------------------------------------------------------------------------- photometric, mask and depth-patch loss
PHOTO_KINDS = {"mse": 0, "huber": 1}                        # include/sparf_hip.h
PHOTO_HUBER_DELTA = 0.5                                     # base_losses.py:156
PHOTO_MAX_PATCH = 8                                         # csrc/photo.h PHOTO_MAX_PATCH


class PhotoReguLoss(torch.autograd.Function):
    """BasePhotoandReguLoss.compute_loss (base_losses.py:243-323, :180-194) and compute_mse_on_rays (metrics.py:33-75) in one library
    call: the ground-truth colours and the mask are gathered in the kernel out of image [B,3,H,W] and fg_mask (bool,
    B H W elements, or None) by ray_idx ([N] shared, [B,N] per image, or None: full images); rgb / rgb_fine [B,N,3], opacity* and depth*
    [B,N,1] in any shape of as many elements.  kind "mse" | "huber" (delta), patch = P or 0.  The six seeds that needs_input_grad asks
    for come from the same launch; the backward multiplies each by the upstream scalar of its own loss and makes no call.
    -> (render, fg_mask, depth_patch, mse, mse_fine) as 0-dim tensors; a term that is off is 0, mse* are not differentiable."""

    @staticmethod
    def forward(ctx, image, fg_mask, ray_idx, rgb, rgb_fine, opacity, opacity_fine, depth, depth_fine, kind, delta, patch, charbonnier):
        op = "photometric loss"
        dev = rgb.device
        L.require_gpu(dev)
        if kind not in PHOTO_KINDS:
            raise ValueError(f"{op}: kind must be one of {sorted(PHOTO_KINDS)}")
        patch = int(patch or 0)
        if image.dim() < 3 or image.shape[1] != 3:
            raise ValueError(f"{op}: image must be [B,3,H,W] or [B,3,H*W]")
        B = image.shape[0]
        HW = image[0, 0].numel() if B else 0
        if rgb.shape[-1] != 3 or (B and rgb.numel() % (3 * B)):
            raise ValueError(f"{op}: rgb must be [B,N,3] for the {B} images")
        rows = rgb.numel() // 3
        N = rows // B if B else 0
        per_image = 0
        if ray_idx is not None:
            if ray_idx.dtype != torch.int64 or tuple(ray_idx.shape) not in ((N,), (B, N)):
                raise ValueError(f"{op}: ray_idx must be int64 [{N}] or [{B}, {N}], got {ray_idx.dtype} {list(ray_idx.shape)}")
            per_image = int(ray_idx.dim() == 2)
            ray_idx = ray_idx.detach().contiguous()
        elif N != HW:
            raise ValueError(f"{op}: without ray_idx the render is of full images: {N} rays for {HW} pixels")
        if fg_mask is not None:
            if fg_mask.dtype != torch.bool or fg_mask.numel() != B * HW:
                raise ValueError(f"{op}: fg_mask must be torch.bool with one element per pixel")
            if opacity is None:
                raise ValueError(f"{op}: the mask term needs opacity")
            fg_mask = fg_mask.detach().contiguous()
        if patch:
            if not 0 < patch <= PHOTO_MAX_PATCH:
                raise ValueError(f"{op}: patch size must be 1..{PHOTO_MAX_PATCH}")
            if depth is None:
                raise ValueError(f"{op}: the depth-patch term needs depth")
            if N % (patch * patch):
                raise ValueError(f"{op}: {N} rays per image are no whole number of {patch}x{patch} patches")
        tensors = (rgb, rgb_fine, opacity, opacity_fine, depth, depth_fine)
        names = ("rgb", "rgb_fine", "opacity", "opacity_fine", "depth", "depth_fine")
        head = [_flat(t, rows * (3 if i < 2 else 1), name, op, "rays") if t is not None else None for i, (t, name) in enumerate(zip(tensors, names))]
        out = torch.empty(5, device=dev, dtype=torch.float32)
        seeds = [torch.empty_like(head[i]) if (t is not None and ctx.needs_input_grad[3 + i]) else None for i, t in enumerate(tensors)]
        ws = L.workspace(L.load().sparf_photo_regu_workspace_bytes(rows), dev, torch.float64)
        p, img = L.ptr, _f32(image)
        L.call("sparf_photo_regu_loss", dev, p(img), p(fg_mask), p(ray_idx), per_image, B, HW, N, *map(p, head), PHOTO_KINDS[kind], float(delta), patch,
               float(charbonnier), p(out), *map(p, seeds), p(ws))
        ctx.save_for_backward(*seeds)
        ctx.shapes = [t.shape if t is not None else None for t in tensors]
        ctx.set_materialize_grads(False)
        render, mask, dpatch, mse, mse_fine = out.unbind(0)
        ctx.mark_non_differentiable(mse, mse_fine)
        return render, mask, dpatch, mse, mse_fine

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_render, g_mask, g_patch, *_):
        ups = (g_render, g_render, g_mask, g_mask, g_patch, g_patch)
        grads = [_seed(s, shape, g) if g is not None else None for s, shape, g in zip(ctx.saved_tensors, ctx.shapes, ups)]
        return (None, None, None, *grads, None, None, None, None)


# ---------------------------------------------------------------------------------------------- correspondence sampler
# SURVEY 8f next-9.  Plain functions: nothing here carries a gradient (every input is detached in the reference).
def match_window(window, H, W):
    """(y0, y1, x0, x1) as the Python slices mask[y0:y1, x0:x1] read them -> the same half-open window with 0 <= y0, y1 <= H, 0 <= x0,
    x1 <= W (an empty one stays empty); None -> the whole image"""
    if window is None:
        return 0, H, 0, W
    y0, y1, _ = slice(int(window[0]), int(window[1])).indices(H)
    x0, x1, _ = slice(int(window[2]), int(window[3])).indices(W)
    return y0, y1, x0, x1


def _match_mask(mask):
    """the mask [H,W] or [H,W,1] (torch.bool) as H W bytes in row-major order -> (tensor, H, W); dense already in every form the
    reference hands over (a slice of [M,1,H,W], permuted), made dense once otherwise"""
    if mask.dtype != torch.bool or mask.dim() not in (2, 3) or (mask.dim() == 3 and mask.shape[-1] != 1):
        raise ValueError(f"correspondence sampler: the mask must be torch.bool [H,W] or [H,W,1], got {mask.dtype} {list(mask.shape)}")
    m = mask.detach()
    m = m[..., 0] if m.dim() == 3 else m
    return (m if m.is_contiguous() else m.contiguous()), m.shape[0], m.shape[1]


def _match_corres(corres, H, W):
    """the correspondence map as [H,W,2] (the reference's permuted view of a channel-first map, read in place) or channel-first
    [2,H,W] -> (tensor whose data_ptr is x of pixel 0, channel stride in elements); any other float32 layout is made dense once"""
    c = corres.detach()
    if tuple(c.shape) == (H, W, 2):
        c = c.permute(2, 0, 1)
    elif tuple(c.shape) != (2, H, W):
        raise ValueError(f"correspondence sampler: the correspondence map must be [{H},{W},2] or [2,{H},{W}], got {list(corres.shape)}")
    if c.dtype != torch.float32:
        raise ValueError("correspondence sampler: the correspondence map must be float32")
    planar = H * W <= 1 or (c[0].is_contiguous() and c.stride(0) >= 0)
    if not planar:
        c = c.contiguous()
    return c, int(c.stride(0)) if H * W else 0


def _match_conf(conf, H, W):
    """the confidence map [H,W,1], [1,H,W] or [H,W] as H W floats in row-major order"""
    c = conf.detach()
    if c.dtype != torch.float32 or c.numel() != H * W or tuple(c.shape) not in ((H, W, 1), (1, H, W), (H, W)):
        raise ValueError(f"correspondence sampler: the confidence map must be float32 [{H},{W},1], [1,{H},{W}] or [{H},{W}], got "
                         f"{c.dtype} {list(conf.shape)}")
    c = c.reshape(H, W)                                  # (dropping a dimension of one element is a view)
    return c if c.is_contiguous() else c.contiguous()


def match_compact(mask, window=None, want_perc=True):
    """sparf_match_compact: the pixels of mask (torch.bool [H,W] or [H,W,1]) inside window -> (index [H W] int32 whose first count
    entries are their flat indices in row-major order, count [1] int32, perc [1] float32 or None), all on the device: no readback"""
    m, H, W = _match_mask(mask)
    dev = m.device
    L.require_gpu(dev)
    y0, y1, x0, x1 = match_window(window, H, W)
    n = H * W
    index = torch.empty(n, device=dev, dtype=torch.int32)
    count = torch.empty(1, device=dev, dtype=torch.int32)
    perc = torch.empty(1, device=dev, dtype=torch.float32) if want_perc else None
    ws = L.workspace(L.load().sparf_match_workspace_bytes(n), dev, torch.int32)
    p = L.ptr
    L.call("sparf_match_compact", dev, p(m), H, W, y0, y1, x0, x1, p(index), p(count), p(perc), p(ws))
    return index, count, perc


def match_gather(index, count, sel, k, H, W, corres, conf):
    """sparf_match_gather for k rows: index / count as match_compact left them, sel int64 [k] positions in index or None (the first k),
    the maps in the forms of _match_corres / _match_conf.  -> (pixels_self [k,2] float32, ray_self [k] int64, pixels_other [k,2]
    float32, ray_other [k] int64, conf [k,1] float32).  k == 0: empty tensors, no call."""
    dev = index.device
    k = int(k)
    f32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
    i64 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int64)
    outs = (f32(k, 2), i64(k), f32(k, 2), i64(k), f32(k, 1))
    if k == 0:
        return outs
    L.require_gpu(dev)
    if sel is not None:
        if sel.dtype != torch.int64 or sel.numel() != k:
            raise ValueError(f"correspondence sampler: the selection must be int64 [{k}], got {sel.dtype} {list(sel.shape)}")
        sel = sel.detach().reshape(-1).contiguous()
    c, stride = _match_corres(corres, H, W)
    cf = _match_conf(conf, H, W)
    p = L.ptr
    L.call("sparf_match_gather", dev, p(index), p(count), p(sel), k, H, W, ctypes.c_void_p(c.data_ptr()), stride, p(cf), *map(p, outs))
    return outs


# ---------------------------------------------------------------------------------------------- DS-NeRF sparse depth loss
# SparseCOLMAPDepthLoss.compute_loss (base_losses.py:326-402) around its renders.  The selection carries no gradient;
# the loss gives one to the rendered depths only.
COLMAP_ALL_ROWS = 1 << 30                                   # a quota that cuts nothing: `count` then holds the row counts themselves


def _colmap_map(t, what):
    """a COLMAP map [B,1,H,W] (or [B,H,W]) float32 -> (dense [B, H W] view of its own storage, B, H, W); only another layout is copied"""
    if t.dtype != torch.float32 or t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[1] != 1):
        raise ValueError(f"sparse depth loss: {what} must be float32 [B,1,H,W] or [B,H,W], got {t.dtype} {list(t.shape)}")
    B, (H, W) = t.shape[0], t.shape[-2:]
    d = t.detach()
    d = d if d.is_contiguous() else d.contiguous()
    return d.view(B, H * W), B, H, W


def colmap_compact(colmap_depth):
    """sparf_colmap_compact over the B images of colmap_depth [B,1,H,W] (read in place) -> (index [B, H W] int32 whose first count[b]
    entries of row b are the flat indices of the pixels of image b with depth > 1e-6 in row-major order, count [2 B] int32: those
    numbers, then the numbers of pixels with depth > 0), both on the device: no readback"""
    d, B, H, W = _colmap_map(colmap_depth, "colmap_depth")
    if B == 0:
        raise ValueError("sparse depth loss: no image")
    dev = d.device
    L.require_gpu(dev)
    n = H * W
    index = torch.empty(B, n, device=dev, dtype=torch.int32)
    count = torch.empty(2 * B, device=dev, dtype=torch.int32)
    ws = L.workspace(L.load().sparf_colmap_workspace_bytes(B, n, 0), dev, torch.int32)
    p = L.ptr
    L.call("sparf_colmap_compact", dev, p(d), B, H, W, p(index), p(count), p(ws))
    return index, count


def colmap_gather(index, count, sel, quota, K, H, W, colmap_depth, colmap_conf, images=None, outs=None):
    """sparf_colmap_gather: the K = sum_b min(count[b], quota) selected rows of the images [b0, b1) (`images`; None: all of them), packed
    in image order.  sel: int64 [b1 - b0, quota] positions in each image's index row, read for the images with count[b] > quota (a
    single [quota] row serves a range whose FIRST image is the only one above the quota), or None: the first rows everywhere.
    outs: (ray_idx, target, weight) dense [K] tensors to fill, or None: new ones.
    -> (ray_idx [K] int64, target [K] float32, weight [K] float32).  K == 0: no call."""
    dev = index.device
    K, quota = int(K), int(quota)
    if outs is None:
        outs = (torch.empty(K, device=dev, dtype=torch.int64), torch.empty(K, device=dev, dtype=torch.float32),
                torch.empty(K, device=dev, dtype=torch.float32))
    if K == 0:
        return outs
    L.require_gpu(dev)
    d, B, _, _ = _colmap_map(colmap_depth, "colmap_depth")
    c, Bc, Hc, Wc = _colmap_map(colmap_conf, "colmap_conf")
    if (Bc, Hc, Wc) != (B, H, W) or tuple(index.shape) != (B, H * W):
        raise ValueError("sparse depth loss: colmap_depth, colmap_conf and the index list are of different sizes")
    b0, b1 = (0, B) if images is None else images
    if not 0 <= b0 < b1 <= B:
        raise ValueError(f"sparse depth loss: images {images} of {B}")
    if sel is not None:
        if sel.dtype != torch.int64 or sel.numel() not in (quota, (b1 - b0) * quota):
            raise ValueError(f"sparse depth loss: the selection must be int64 [{b1 - b0}, {quota}] or [{quota}], got {sel.dtype} {list(sel.shape)}")
        sel = sel.detach().reshape(-1).contiguous()
    if any(o.numel() != K for o in outs):
        raise ValueError(f"sparse depth loss: the outputs must hold {K} rows")
    p = L.ptr
    L.call("sparf_colmap_gather", dev, p(index[b0:b1]), p(count[b0:b1]), p(sel), b1 - b0, H, W, quota, K, p(d[b0:b1]), p(c[b0:b1]), *map(p, outs))
    return outs


def _adjacent(ts):
    """whether the dense float32 tensors `ts` lie one behind the other in one storage (the rendered depths of one pass buffer)"""
    for a, b in zip(ts, ts[1:]):
        if a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr() or a.data_ptr() + 4 * a.numel() != b.data_ptr():
            return False
    return True


def _colmap_packed(ts, K):
    """the rendered depths of the images as one dense [K] float32 tensor: read in place where they are adjacent views of one buffer,
    one torch.cat otherwise"""
    ts = [t.detach() for t in ts]
    if all(t.dtype == torch.float32 and t.is_contiguous() for t in ts) and (len(ts) == 1 or _adjacent(ts)):
        return torch.as_strided(ts[0], (K,), (1,))
    return torch.cat([t.reshape(-1).to(torch.float32) for t in ts])


class ColmapLoss(torch.autograd.Function):
    """base_losses.py:391-400 over the packed rows of every rendered image in one library call, which also leaves the gradient seeds of
    the rendered depths; the backward multiplies them by the upstream scalar and makes no call.  count: int32 on the device, image b
    holds min(count[b], quota) rows; nd depths (any shape, one per image with rows, in image order), then none or nd fine depths.
    -> the loss, a 0-dim tensor"""

    @staticmethod
    def forward(ctx, target, weight, count, quota, batch_size, nd, *depths):
        op = "sparse depth loss"
        dev = target.device
        L.require_gpu(dev)
        nd, B, quota = int(nd), int(batch_size), int(quota)
        if len(depths) not in (nd, 2 * nd) or nd == 0:
            raise ValueError(f"{op}: {len(depths)} depth tensors for {nd} rendered images")
        coarse, fine = depths[:nd], depths[nd:]
        K = target.numel()
        if sum(t.numel() for t in coarse) != K or (fine and [t.numel() for t in fine] != [t.numel() for t in coarse]):
            raise ValueError(f"{op}: the rendered depths do not hold the {K} selected rows")
        if count.dtype != torch.int32 or count.numel() < B:
            raise ValueError(f"{op}: the counts must be int32 [{B}] on the device")
        t, w = _flat(target, K, "target", op, "rows"), _flat(weight, K, "weight", op, "rows")
        p_c = _colmap_packed(coarse, K)
        p_f = _colmap_packed(fine, K) if fine else None
        out = torch.empty(1, device=dev, dtype=torch.float32)
        need_c, need_f = any(ctx.needs_input_grad[6:6 + nd]), any(ctx.needs_input_grad[6 + nd:])
        s_c = torch.empty(K, device=dev, dtype=torch.float32) if need_c else None
        s_f = torch.empty(K, device=dev, dtype=torch.float32) if need_f else None
        ws = L.workspace(L.load().sparf_colmap_workspace_bytes(0, 0, K), dev, torch.float64)
        p = L.ptr
        L.call("sparf_colmap_loss", dev, p(t), p(w), p(count.detach().contiguous()), B, quota, K, p(p_c), p(p_f), p(out), p(s_c), p(s_f), p(ws))
        ctx.save_for_backward(s_c, s_f)
        ctx.shapes = [d.shape for d in depths]
        ctx.nd = nd
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        s_c, s_f = ctx.saved_tensors
        grads = []
        for s, shapes in ((s_c, ctx.shapes[:ctx.nd]), (s_f, ctx.shapes[ctx.nd:])):
            if s is None:
                grads += [None] * len(shapes)
                continue
            sg, off = s * g, 0
            for shape in shapes:
                grads.append(sg[off:off + shape.numel()].view(shape))
                off += shape.numel()
        return (None,) * 6 + tuple(grads)


# ---------------------------------------------------------------------------------------------- evaluation metrics
# SURVEY 8f next-10.  A plain function: evaluation carries no gradient.
METRICS_OUTS = ("mse", "psnr", "ssim", "mse_masked", "psnr_masked", "ssim_masked", "abs_e", "rmse", "abs_e_scaled", "rmse_scaled")     # csrc/metrics.h


def _metrics_image(t, B, H, W, name):
    """an image [B,3,H,W] float32 in whatever strides it comes (a permuted channel-last render, an offset slice): read in place; only
    a view with a negative stride (none of torch's) would be made dense"""
    if t.dtype != torch.float32 or tuple(t.shape) != (B, 3, H, W):
        raise ValueError(f"image metrics: {name} must be float32 [{B},3,{H},{W}], got {t.dtype} {list(t.shape)}")
    t = t.detach()
    return t if all(s >= 0 for s in t.stride()) else t.contiguous()


def _metrics_rows(t, B, HW, dtypes, name):
    """depth [B, H W] in any shape of as many elements per image (float32), or a validity mask (bool / uint8) -> [B, HW] view"""
    if t.dtype not in dtypes or t.shape[0] != B or t.numel() != B * HW:
        raise ValueError(f"image metrics: {name} must be {dtypes[0]} with {HW} elements for each of the {B} images, got {t.dtype} {list(t.shape)}")
    return t.detach().reshape(B, HW)


def image_metrics(pred, gt, pred_fine=None, fg_mask=None, depth=None, depth_fine=None, depth_gt=None, valid_depth_gt=None, depth_scale=1.0):
    """sparf_image_metrics: pred / pred_fine / gt float32 [B,3,H,W] in any strides; fg_mask torch.bool or uint8 0/1, B H W elements
    ([B,H,W] or [B,1,H,W]); depth / depth_fine / depth_gt float32 and valid_depth_gt bool, H W elements per image.
    -> (out [2,10] float32: a row per head in the order of METRICS_OUTS, NaN for what was not asked for; counts [2] int32: foreground
    pixels, valid depth pixels), on the device: two launches, no readback"""
    if gt.dim() != 4 or gt.shape[1] != 3:
        raise ValueError(f"image metrics: gt must be [B,3,H,W], got {list(gt.shape)}")
    B, _, H, W = gt.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"image metrics: empty images {list(gt.shape)}")
    dev = gt.device
    L.require_gpu(dev)
    if (depth is not None or depth_fine is not None) and depth_gt is None:
        raise ValueError("image metrics: a depth needs depth_gt")
    if depth_fine is not None and pred_fine is None:
        raise ValueError("image metrics: depth_fine needs pred_fine")
    a = L.ImageMetrics(B=B, H=H, W=W, depth_scale=float(depth_scale))
    keep = []

    def put(name, t):
        keep.append(t)
        setattr(a, name, t.data_ptr())
        getattr(a, name + "_stride")[:] = t.stride()

    put("pred", _metrics_image(pred, B, H, W, "pred"))
    put("gt", _metrics_image(gt, B, H, W, "gt"))
    if pred_fine is not None:
        put("pred_fine", _metrics_image(pred_fine, B, H, W, "pred_fine"))
    if fg_mask is not None:
        if fg_mask.dtype not in (torch.bool, torch.uint8) or fg_mask.numel() != B * H * W or fg_mask.shape[0] != B:
            raise ValueError(f"image metrics: fg_mask must be torch.bool (or 0/1 bytes) with one element per pixel, got {fg_mask.dtype} {list(fg_mask.shape)}")
        put("fg_mask", fg_mask.detach().reshape(B, H, W))
    for name, t, dtypes in (("depth", depth, (torch.float32,)), ("depth_fine", depth_fine, (torch.float32,)), ("depth_gt", depth_gt, (torch.float32,)),
                            ("valid_depth_gt", valid_depth_gt if depth_gt is not None else None, (torch.bool, torch.uint8))):
        if t is not None:
            put(name, _metrics_rows(t, B, H * W, dtypes, name))
    out = torch.empty(2, len(METRICS_OUTS), device=dev, dtype=torch.float32)
    counts = torch.empty(2, device=dev, dtype=torch.int32)
    nb = int(L.load().sparf_image_metrics_workspace_bytes(B, H, W))
    ws = torch.empty(max(nb // 8, 1), device=dev, dtype=torch.float64)         # (always one: the struct's pointer is never null)
    a.out, a.counts, a.workspace, a.workspace_bytes = out.data_ptr(), counts.data_ptr(), ws.data_ptr(), nb
    L.call("sparf_image_metrics", dev, ctypes.byref(a))
    return out, counts


# ---------------------------------------------------------------------------------------------- depth errors on rendered rays
# compute_depth_error_on_rays (metrics.py:81-134), both heads.  A plain function: the reference runs it under no_grad.
DEPTH_ERR_OUTS = ("abs_e", "rmse", "abs_e_fine", "rmse_fine")            # csrc/depth_err.h


def _depth_err_rows(t, B, name):
    """a rendered depth [B,N,1] or [B,N] float32 -> dense [B,N]"""
    if t.dtype != torch.float32 or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 1) or t.shape[0] != B:
        raise ValueError(f"depth error on rays: {name} must be float32 [{B},N,1] or [{B},N], got {t.dtype} {list(t.shape)}")
    return t.detach().reshape(B, t.numel() // B if B else 0).contiguous()


def ray_depth_err(depth_gt, valid_depth_gt, depth, depth_fine=None, ray_idx=None, img_idx=None, scale=1.0):
    """sparf_ray_depth_err: depth_gt float32 [B_maps,H,W] or [B_maps,1,H,W] and valid_depth_gt (torch.bool or 0/1 bytes, as many
    elements; None: every pixel) are the maps of the scene, read in place (only another layout is copied); depth / depth_fine float32
    [B,N,1] or [B,N]; ray_idx int64 [N] (one list for all images) or [B,N], None for full images; img_idx int64 [B] on the device: the
    map of each rendered image, None for the first B maps in order; scale a number, or a one-element tensor -- on the operands' device
    it is passed by pointer (converted there if it is not float32) and never read back, a host tensor is rounded to float32 on the host.
    -> (out [4] float32: abs_e, rmse, abs_e_fine, rmse_fine -- the fine pair 0 without depth_fine; count [1] int32: the valid rows), on
    the device: one library call, no readback"""
    op = "depth error on rays"
    if depth_gt.dtype != torch.float32 or depth_gt.dim() not in (3, 4) or (depth_gt.dim() == 4 and depth_gt.shape[1] != 1) or depth_gt.shape[0] < 1:
        raise ValueError(f"{op}: depth_gt must be float32 [B,1,H,W] or [B,H,W] of at least one map, got {depth_gt.dtype} {list(depth_gt.shape)}")
    dev = depth_gt.device
    L.require_gpu(dev)
    B_maps, HW = depth_gt.shape[0], depth_gt.shape[-2] * depth_gt.shape[-1]
    gt = depth_gt.detach()
    gt = gt if gt.is_contiguous() else gt.contiguous()
    valid = None
    if valid_depth_gt is not None:
        if valid_depth_gt.dtype not in (torch.bool, torch.uint8) or valid_depth_gt.numel() != B_maps * HW:
            raise ValueError(f"{op}: valid_depth_gt must be torch.bool with one element per pixel of depth_gt, got {valid_depth_gt.dtype} "
                             f"{list(valid_depth_gt.shape)}")
        valid = valid_depth_gt.detach()
        valid = valid if valid.is_contiguous() else valid.contiguous()
    B = depth.shape[0]
    d = _depth_err_rows(depth, B, "depth")
    N = d.shape[1]
    df = None
    if depth_fine is not None:
        df = _depth_err_rows(depth_fine, B, "depth_fine")
        if df.shape != d.shape:
            raise ValueError(f"{op}: depth_fine has {list(depth_fine.shape)} for a depth of {list(depth.shape)}")
    per_image = 0
    if ray_idx is not None:
        if ray_idx.dtype != torch.int64 or tuple(ray_idx.shape) not in ((N,), (B, N)):
            raise ValueError(f"{op}: ray_idx must be int64 [{N}] or [{B}, {N}], got {ray_idx.dtype} {list(ray_idx.shape)}")
        per_image = int(ray_idx.dim() == 2)
        ray_idx = ray_idx.detach().contiguous()
    elif N != HW:
        raise ValueError(f"{op}: without ray_idx the render is of full images: {N} rays for {HW} pixels")
    if img_idx is not None:
        if img_idx.dtype != torch.int64 or img_idx.numel() != B:
            raise ValueError(f"{op}: img_idx must be int64 [{B}], got {img_idx.dtype} {list(img_idx.shape)}")
        img_idx = img_idx.detach().reshape(-1).contiguous()
    scale_dev = None
    if torch.is_tensor(scale):
        if scale.numel() != 1:
            raise ValueError(f"{op}: the scale must be one number, got {list(scale.shape)}")
        s32 = scale.detach().reshape(1).to(torch.float32)
        scale_dev, scale = (s32, 1.0) if s32.device == dev else (None, float(s32))
    out = torch.empty(len(DEPTH_ERR_OUTS), device=dev, dtype=torch.float32)
    count = torch.empty(1, device=dev, dtype=torch.int32)
    ws = L.workspace(L.load().sparf_ray_depth_err_workspace_bytes(B * N), dev, torch.float64)
    p = L.ptr
    # (a fine head without rows is an empty tensor and has no address: `out` marks it present -- a call without rows reads no input)
    fine = p(out) if df is not None and df.numel() == 0 else p(df)
    L.call("sparf_ray_depth_err", dev, p(gt), p(valid), p(img_idx), p(ray_idx), per_image, B_maps, B, HW, N, p(d), fine, float(scale), p(scale_dev),
           p(out), p(count), p(ws))
    return out, count


# ---------------------------------------------------------------------------------------------- pixel picks and the unseen pose
PICK_MAX_ROWS = 1 << 30          # csrc/pick.hip kPickMaxRows


def _pick_perm(perm, name, dev):
    if perm is None:
        return None, 0
    if perm.dtype != torch.int64 or perm.dim() != 1 or _resolve(perm.device) != dev:
        raise ValueError(f"pick pixels: {name} must be int64 [n] on {dev}, got {perm.dtype} {list(perm.shape)} on {perm.device}")
    return (perm.detach().contiguous(), perm.numel()) if perm.numel() else (None, 0)


def pick_pixels(perm_a, perm_b, pool_a, pool_b, W, patch=1, *, pixels=True, rays=True, device=None):
    """sparf_pick_pixels: perm_a / perm_b int64 [n] on the device (None or empty: no pick of that pool) index pool_a = (a_w, a_h), the
    grid [0,a_w) x [0,a_h), and pool_b = (b_x0, b_y0, b_w, b_h), a box, both row-major (None: (0, 0) / (0, 0, 0, 0)); an entry outside its
    pool is clamped into it.  -> (pixels float32 [(n_a + n_b) patch^2, 2] = (x, y), rays int64 [...] = y W + x), the picks of A before those
    of B, each expanded by the patch offsets (dy outer, dx inner); an output not asked for is None: one launch, no readback"""
    dev = device if device is not None else next((t.device for t in (perm_a, perm_b) if t is not None), None)
    if dev is None:
        raise ValueError("pick pixels: no permutation and no device")
    dev = _resolve(dev)                                   # (a bare 'cuda', as the reference trainer holds it, is the current device)
    L.require_gpu(dev)
    pa, n_a = _pick_perm(perm_a, "perm_a", dev)
    pb, n_b = _pick_perm(perm_b, "perm_b", dev)
    a_w, a_h = (int(v) for v in (pool_a or (0, 0)))
    b_x0, b_y0, b_w, b_h = (int(v) for v in (pool_b or (0, 0, 0, 0)))
    W, patch = int(W), int(patch)
    if W <= 0 or not 1 <= patch <= 1024:
        raise ValueError(f"pick pixels: W must be positive and patch in [1, 1024], got W {W} patch {patch}")
    rows = (n_a + n_b) * patch * patch
    if rows > PICK_MAX_ROWS:
        raise ValueError(f"pick pixels: {rows} rows, at most 2^30")
    for n, x0, y0, w, h, name in ((n_a, 0, 0, a_w, a_h, "A"), (n_b, b_x0, b_y0, b_w, b_h, "B")):
        if n and (x0 < 0 or y0 < 0 or w <= 0 or h <= 0 or w * h > PICK_MAX_ROWS or x0 + w + patch - 1 > W):
            raise ValueError(f"pick pixels: pool {name} ({x0}, {y0}, {w}, {h}) with a patch of {patch} does not lie in rows of {W} pixels")
    out_px = torch.empty(rows, 2, device=dev, dtype=torch.float32) if pixels else None
    out_rays = torch.empty(rows, device=dev, dtype=torch.int64) if rays else None
    if rows and (pixels or rays):
        p = L.ptr
        L.call("sparf_pick_pixels", dev, p(pa), n_a, p(pb), n_b, a_w, a_h, b_x0, b_y0, b_w, b_h, W, patch, p(out_px), p(out_rays))
    return out_px, out_rays


UNSEEN_POSE_OUTS = ("pose_w2c_ref", "pose_c2w_ref", "pose_c2w_other", "pose_w2c_at_unseen")


def unseen_pose(poses_w2c, id_self, w):
    """sparf_unseen_pose: poses_w2c float32 [B,3,4] or [B,4,4] on the device, id_self an int in [0, B), w a number (1 - w is taken in
    double and rounded to float32 once, as torch handles the scalar).  -> (out float32 [4,4,4]: pose_w2c_ref, pose_c2w_ref,
    pose_c2w_other, pose_w2c_at_unseen; id_other int32 [1]) on the device: one launch, no readback"""
    op = "unseen pose"
    if poses_w2c.dtype != torch.float32 or poses_w2c.dim() != 3 or tuple(poses_w2c.shape[1:]) not in ((3, 4), (4, 4)) or poses_w2c.shape[0] < 1:
        raise ValueError(f"{op}: poses_w2c must be float32 [B,3,4] or [B,4,4] of at least one pose, got {poses_w2c.dtype} {list(poses_w2c.shape)}")
    dev = poses_w2c.device
    L.require_gpu(dev)
    B, id_self, w = poses_w2c.shape[0], int(id_self), float(w)
    if not 0 <= id_self < B:
        raise ValueError(f"{op}: id_self {id_self} outside [0, {B})")
    poses = poses_w2c.detach()
    poses = poses if poses.is_contiguous() else poses.contiguous()
    out = torch.empty(len(UNSEEN_POSE_OUTS), 4, 4, device=dev, dtype=torch.float32)
    id_other = torch.empty(1, device=dev, dtype=torch.int32)
    p = lambda k: ctypes.c_void_p(out.data_ptr() + 64 * k)
    L.call("sparf_unseen_pose", dev, L.ptr(poses), poses.shape[1] * 4, B, id_self, w, 1.0 - w, p(0), p(1), p(2), p(3), L.ptr(id_other))
    return out, id_other


# ---------------------------------------------------------------------------------------------- stand-alone compositing
class Composite(torch.autograd.Function):
    """NeRF.composite (frequency_nerf.py:283-343) on caller-built per-sample values (C ABI 6 sparf_composite_forward / _backward):
    ray [R,3], density [R,N] (after softplus), rgb_samples [R,N,3] (after the sigmoid), t [R,N].
    -> rgb [R,3], depth, opacity [R], weights [R,N], depth_var, rgb_var, all_cumulated [R]: all differentiable w.r.t. density,
    rgb_samples and the ray (through its length: dist = delta * |ray|, :302-308); the depth samples receive none."""

    @staticmethod
    def forward(ctx, ray, density, rgb_samples, t, white_bg):
        dev = ray.device
        L.require_gpu(dev)
        d, dn, cs, tt = _f32(ray), _f32(density), _f32(rgb_samples), _f32(t)
        R, N = tt.shape
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        out = dict(raylen=f(R), weights=f(R, N), rgb=f(R, 3), depth=f(R), opacity=f(R), depth_var=f(R), rgb_var=f(R), all_cumulated=f(R))
        a = L.CompositeFwd(nrays=R, nsamp=N, white_bg=int(bool(white_bg)), dir=d.data_ptr(), t=tt.data_ptr(), density=dn.data_ptr(),
                           rgb_samples=cs.data_ptr(), **{k: v.data_ptr() for k, v in out.items()})
        L.call("sparf_composite_forward", dev, ctypes.byref(a))
        ctx.save_for_backward(d, dn, cs, tt, out["raylen"], out["weights"])
        ctx.white_bg = int(bool(white_bg))
        ctx.set_materialize_grads(False)
        return out["rgb"], out["depth"], out["opacity"], out["weights"], out["depth_var"], out["rgb_var"], out["all_cumulated"]

    @staticmethod
    def backward(ctx, *g7):
        d, dn, cs, tt, raylen, weights = ctx.saved_tensors
        dev = d.device
        R, N = tt.shape
        gs = [_f32(g) if g is not None else None for g in g7]
        d_dens = torch.empty(R, N, dtype=torch.float32, device=dev)
        d_rgbs = torch.empty(R, N, 3, dtype=torch.float32, device=dev)
        need_ray = ctx.needs_input_grad[0]
        d_dir = torch.empty(R, 3, dtype=torch.float32, device=dev) if need_ray else None
        d_len = torch.empty(R, dtype=torch.float32, device=dev) if need_ray else None
        P = lambda x: x.data_ptr() if x is not None else None
        a = L.CompositeBwd(nrays=R, nsamp=N, white_bg=ctx.white_bg, dir=P(d), t=P(tt), density=P(dn), rgb_samples=P(cs), raylen=P(raylen),
                           weights=P(weights), g_rgb=P(gs[0]), g_depth=P(gs[1]), g_opacity=P(gs[2]), g_weights=P(gs[3]), g_depth_var=P(gs[4]),
                           g_rgb_var=P(gs[5]), g_all_cumulated=P(gs[6]), d_density=P(d_dens), d_rgb_samples=P(d_rgbs), d_dir=P(d_dir), d_len_ws=P(d_len))
        L.call("sparf_composite_backward", dev, ctypes.byref(a))
        return d_dir, d_dens if ctx.needs_input_grad[1] else None, d_rgbs if ctx.needs_input_grad[2] else None, None, None


def composite(ray, density, rgb_samples, t, white_bg):
    """-> dict with the reference's composite keys (flat ray axis)"""
    if t.requires_grad and torch.is_grad_enabled():
        raise L.SparfError("composite: depth samples that require a gradient are not supported (none of the reference's callers "
                           "differentiates them: renderer.py:323 no_grad, :405-407 fresh draws)")
    return dict(zip(PASS_KEYS[:7], Composite.apply(ray, density, rgb_samples, t, white_bg)))       # (the per-sample two are its inputs)


# ---------------------------------------------------------------------------------------------- one render call = one autograd node
# Graph.render (renderer.py:250-345) behind ONE autograd.Function: coarse depths -> coarse pass -> resampling + merge -> fine pass, issued
# from one Python frame through the C ABI with every fp32 result of BOTH passes in ONE allocation (an "arena": the outputs are views of
# it), the per-pass C structs filled from cached offset tables, and one backward that runs both passes' backward calls and hands
# the parameter gradients over as views of one [2, N_PARAMS] buffer.  Round 4 ran a render as two NerfPass nodes + ~15 allocations
# + ~40 ctypes attribute stores per pass: 1.2 ms of host time per render + backward (profiles/r04_host_overhead.log), which is what
# the six render calls per iteration of the unmodified SPARF losses were bounded by.
_PASS_F32 = (("raylen", 1, 0), ("sigma_raw", 0, 1), ("rgb_samples", 0, 3), ("density", 0, 1), ("weights", 0, 1), ("rgb", 3, 0), ("depth", 1, 0),
             ("opacity", 1, 0), ("depth_var", 1, 0), ("rgb_var", 1, 0), ("all_cumulated", 1, 0), ("t", 0, 1))     # (name, floats per ray, floats per sample)
_PARAM_SIZES = [n for (o, i) in L.LAYER_SHAPES for n in (o * i, o)]
_PLANS = {}


class _RenderPlan:
    """offsets (in floats) of every fp32 result of a render inside its two arenas, for R rays, Nc coarse and Nf fine samples.  Arena 0
    holds what is per RAY (rgb, depth, opacity, the variances, all_cumulated, |ray|, the band weights), arena 1 what is per SAMPLE
    (depths, raw density, colours, density, weights): a caller that keeps `ret.rgb` of a slice alive -- Graph.render_by_slices does, until
    its final cat; so does logging code -- pins a few floats per ray, not the ~28 bytes per sample row and pass of the whole render
    (a 756 x 1008 evaluation image retained 5.5 GB that way when both lived in one allocation)."""

    def __init__(self, R, Nc, Nf):
        self.R, self.Nc, self.Nf = R, Nc, Nf
        self.off, self.order, tot = {}, ([], []), [0, 0]
        for tag, N in (("c", Nc), ("f", Nc + Nf)):
            if tag == "f" and Nf == 0:           # no fine pass (gated off / no fine network): nothing reserved for it
                continue
            for name, per_ray, per_samp in _PASS_F32:
                k = 0 if per_samp == 0 else 1
                n = R * (per_ray + per_samp * N)
                n_al = (n + 63) // 64 * 64                       # 256-byte granules
                self.off[tag + name] = (tot[k], n, k)
                self.order[k].append((tag + name, n_al))
                tot[k] += n_al
            self.off[tag + "c2f"] = (tot[0], 16, 0)
            self.order[0].append((tag + "c2f", 64))
            tot[0] += 64
        self.total = tuple(tot)


def _plan(R, Nc, Nf):
    key = (R, Nc, Nf)
    p = _PLANS.get(key)
    if p is None:
        if len(_PLANS) > 256:
            _PLANS.clear()
        p = _PLANS[key] = _RenderPlan(R, Nc, Nf)
    return p


# One pass of a render, as RenderFn's forward and backward see it.  tag: "c" | "f", the prefix of its results in the arena plan; prec: the
# pass precision id (pass_prec_of).  The forward adds far ((K, far_prec) | None), the far_prec packed weights and the network's progress
# scalar; the backward the address of the band weights its forward was given, its save area and the pass's nine upstream gradients.
_Pass = namedtuple("_Pass", "tag N prec packed noise far far_packed prog c2f save grads", defaults=(None,) * 6)


class RenderFn(torch.autograd.Function):
    """inputs : center, dirs [R,3] (differentiable); cfg (dict, below); jitter [R,Nc] | None, u_mid [Nf] | None, noise_c [R,Nc] | None,
                noise_f [R,Nc+Nf] | None, range_dev | None, packed_c, packed_f | None, far_packed_c, far_packed_f | None,
                prog_c, prog_f (the networks' `progress` scalars, device fp32: the BARF band weights of each pass are computed from
                their CURRENT device value inside this call, frequency_nerf.py:248-253; ignored when cfg['c2f'] is None); theta_c, theta_f:
                the networks' parameters as ONE flat autograd tensor each (NeRF.flat_params: the route of the parameter gradient -- the
                kernels read the packed streams) or None (no gradient wanted).
                u_mid may be a HOST tensor (the grid of renderer.py:439 is drawn on the CPU): it then travels in the launch arguments.
       cfg    : R, Nc, Nf, fine, dmin, dmax, scale, inverse, u_const, noise_scale, white_bg, prec_c, prec_f (pass precision ids), far_c, far_f
                ((K, far_prec) | None), c2f ((start, end) | None), grad (torch.is_grad_enabled() at the call site)
       outputs: per pass (coarse, then fine if cfg['fine']) rgb [R,3], depth, opacity [R], weights [R,N], depth_var, rgb_var, all_cumulated
                [R], density [R,N], rgb_samples [R,N,3] (differentiable) and t [R,N] (the pass's depth samples; no gradient)."""

    @staticmethod
    def forward(ctx, center, dirs, cfg, jitter, u_mid, noise_c, noise_f, range_dev, packed_c, packed_f, far_packed_c, far_packed_f, prog_c, prog_f, theta_c, theta_f):
        lib = L.load()
        dev = center.device
        R, Nc, Nf, fine = cfg["R"], cfg["Nc"], cfg["Nf"], cfg["fine"]
        plan = _plan(R, Nc, Nf if fine else 0)
        c, d = _contig32(center), _contig32(dirs)
        need_grad = bool(cfg["grad"]) and any(ctx.needs_input_grad)
        # per pass: a network none of whose parameters wants a gradient (theta is None) under rays that do = a ray-gradient-only pass
        rays_grad = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        precs = [pass_prec_of(cfg[k], pass_save_kind(bool(cfg["grad"]), rays_grad, ctx.needs_input_grad[i], cfg[k], need_grad))
                 for k, i in (("prec_c", 14), ("prec_f", 15))]
        ctx.set_materialize_grads(False)
        arenas = (torch.empty(plan.total[0], dtype=torch.float32, device=dev), torch.empty(plan.total[1], dtype=torch.float32, device=dev))
        bases = (arenas[0].data_ptr(), arenas[1].data_ptr())
        A = lambda name: bases[plan.off[name][2]] + 4 * plan.off[name][0]
        stream = L.stream_ptr(dev)
        passes = [_Pass("c", Nc, precs[0], packed_c, noise_c, cfg["far_c"], far_packed_c, prog_c)]
        if fine:
            passes.append(_Pass("f", Nc + Nf, precs[1], packed_f, noise_f, cfg["far_f"], far_packed_f, prog_f))
        saves, keep = [], []
        c2f_off = None if cfg["c2f"] is not None else c2f_weights(None, None, dev).data_ptr()     # no masking: the constant vector of the device
        with L.on(dev):
            L.check(lib.sparf_sample_coarse(L.ptr(jitter), float(cfg["u_const"]), None, L.ptr(range_dev), float(cfg["dmin"]), float(cfg["scale"]),
                                            int(cfg["inverse"]), R, Nc, c_void_p(A("ct")), stream), "sparf_sample_coarse")
            for p in passes:
                tag = p.tag
                if c2f_off is None:       # the pass's band weights, from the device value of its network's progress right now
                    if p.prog.dtype is not torch.float32 or p.prog.device != dev:
                        raise L.SparfError("NeRF.progress must be a float32 scalar on the renderer's device")
                    L.check(lib.sparf_c2f_weights(c_void_p(p.prog.data_ptr()), 1, float(cfg["c2f"][0]), float(cfg["c2f"][1]), c_void_p(A(tag + "c2f")), stream),
                            "sparf_c2f_weights")
                if tag == "f":
                    fn, grid = _fine_grid(lib, u_mid, dev)
                    L.check(fn(c_void_p(A("cweights")), c_void_p(A("ct")), L.ptr(grid), L.ptr(range_dev), float(cfg["dmin"]), float(cfg["dmax"]),
                               R, Nc, Nf, None, c_void_p(A("ft")), stream), "sparf_sample_fine")
                a, save, scratch = prepare_pass_fwd(
                    p.prec, R, p.N, dev, save=need_grad, noise_scale=cfg["noise_scale"] if p.noise is not None else 0.0, white_bg=cfg["white_bg"],
                    far=(p.far[0], p.far[1], p.far_packed.data_ptr()) if p.far is not None else None, center=c.data_ptr(), dir=d.data_ptr(),
                    t=A(tag + "t"), noise=_addr(p.noise), packed=p.packed.data_ptr(), c2f=c2f_off if c2f_off is not None else A(tag + "c2f"),
                    **{k: A(tag + k) for k, _, _ in _PASS_F32[:-1]})        # (all but "t": what the pass writes)
                L.check(lib.sparf_pass_forward(ctypes.byref(a), stream), "sparf_pass_forward")
                saves.append(save)
                keep += scratch
        # the results: views of the two arenas, one split per arena + one view each
        pieces = {}
        for k in (0, 1):
            pieces.update(zip([n for n, _ in plan.order[k]], arenas[k].split_with_sizes([s for _, s in plan.order[k]])))
        outs = []
        for p in passes:
            tag, N = p.tag, p.N
            g = lambda name, *shape: pieces[tag + name][:plan.off[tag + name][1]].view(*shape) if plan.off[tag + name][1] != pieces[tag + name].numel() \
                else pieces[tag + name].view(*shape)
            outs += [g("rgb", R, 3), g("depth", R), g("opacity", R), g("weights", R, N), g("depth_var", R), g("rgb_var", R), g("all_cumulated", R),
                     g("density", R, N), g("rgb_samples", R, N, 3), g("t", R, N)]
        ctx.mark_non_differentiable(*outs[9::10])
        if need_grad:
            ctx.save_for_backward(c, d, arenas[0], arenas[1], noise_c, noise_f, packed_c, packed_f, *saves)
            ctx.cfg, ctx.plan, ctx.npass, ctx.c2f_off, ctx.precs = cfg, plan, len(passes), c2f_off, precs
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g):
        lib = L.load()
        cfg, plan, npass = ctx.cfg, ctx.plan, ctx.npass
        c, d, arena_ray, arena_samp, noise_c, noise_f, packed_c, packed_f, *saves = ctx.saved_tensors
        dev = c.device
        R, Nc, Nf = cfg["R"], cfg["Nc"], cfg["Nf"]
        bases = (arena_ray.data_ptr(), arena_samp.data_ptr())
        A = lambda name: bases[plan.off[name][2]] + 4 * plan.off[name][0]
        pose = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        c2f_of = lambda tag: ctx.c2f_off if ctx.c2f_off is not None else A(tag + "c2f")       # the vector the forward of that pass was given
        passes = [_Pass("c", Nc, ctx.precs[0], packed_c, noise_c, c2f=c2f_of("c"), save=saves[0], grads=g[0:9])]
        if npass == 2:
            passes.append(_Pass("f", Nc + Nf, ctx.precs[1], packed_f, noise_f, c2f=c2f_of("f"), save=saves[1], grads=g[10:19]))
        active = [p for p in passes if any(x is not None for x in p.grads)]
        full = {p.tag for p in active if has_param_grad(p.prec)}
        gp = torch.empty(2, L.N_PARAMS, dtype=torch.float32, device=dev) if full else None
        rays = torch.empty(2, R, 3, dtype=torch.float32, device=dev) if (pose and active) else None
        stream = L.stream_ptr(dev)
        keep = []
        with L.on(dev):
            for i, p in enumerate(active):
                a, scratch = prepare_pass_bwd(
                    p.prec, R, p.N, dev, grads=p.grads, grad_params=gp.data_ptr() + (0 if p.tag == "c" else 4 * L.N_PARAMS) if p.tag in full else None,
                    d_center=_addr(rays[0]) if pose else None, d_dir=_addr(rays[1]) if pose else None, accumulate_rays=int(i > 0),
                    noise_scale=cfg["noise_scale"] if p.noise is not None else 0.0, white_bg=cfg["white_bg"], center=c.data_ptr(), dir=d.data_ptr(),
                    t=A(p.tag + "t"), noise=_addr(p.noise), packed=p.packed.data_ptr(), c2f=p.c2f, save=p.save.data_ptr(),
                    **{k: A(p.tag + k) for k in ("raylen", "sigma_raw", "rgb_samples", "weights")})
                L.check(lib.sparf_pass_backward(ctypes.byref(a), stream), "sparf_pass_backward")
                keep += scratch
        g_c = gp[0] if "c" in full else None
        g_f = gp[1] if "f" in full else None
        return (rays[0] if (rays is not None and ctx.needs_input_grad[0]) else None, rays[1] if (rays is not None and ctx.needs_input_grad[1]) else None,
                None, None, None, None, None, None, None, None, None, None, None, None, g_c, g_f)


class FlatParams(torch.autograd.Function):
    """The 20 parameter tensors of a network as ONE flat tensor (NeRF.flat_params): forward = one `cat`, backward = the flat gradient cut
    into the parameters' shapes as views of itself -- one autograd node where `torch.cat([p.reshape(-1) ...])` is eleven."""

    @staticmethod
    def forward(ctx, *params):
        ctx.shapes = [tuple(p.shape) for p in params]
        ctx.set_materialize_grads(False)          # a network whose pass received no gradient keeps p.grad = None (as under per-parameter inputs)
        return torch.cat([p.reshape(-1) for p in params])

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * len(ctx.shapes)
        sizes = [math.prod(s) for s in ctx.shapes]
        parts = g.split_with_sizes(sizes)
        return tuple(x if len(s) == 1 else x.view(s) for x, s in zip(parts, ctx.shapes))


def render_fused(center, dirs, cfg, jitter, u_mid, noise_c, noise_f, range_dev, packed_c, packed_f, far_packed_c, far_packed_f, prog_c, prog_f, theta_c, theta_f):
    """-> (coarse dict, fine dict | None) with the reference's composite keys + 't' (flat ray axis)"""
    cfg = dict(cfg, grad=torch.is_grad_enabled())
    flat = RenderFn.apply(center, dirs, cfg, jitter, u_mid, noise_c, noise_f, range_dev, packed_c, packed_f, far_packed_c, far_packed_f, prog_c, prog_f,
                          theta_c, theta_f)
    coarse = dict(zip(RENDER_KEYS, flat[:10]))
    fine = dict(zip(RENDER_KEYS, flat[10:20])) if cfg["fine"] else None
    return coarse, fine
