"""Float64 referee of the pose parameterisations (tests/test_pose_cpu.py, tests/test_pose_gpu.py): the same formulas as
include/sparf_hip.h states them, in torch.float64 on the CPU, with autograd for the vector-Jacobian products -- so the hand-derived
backward kernels are checked against a derivation they do not share.  The series are written as polynomials in theta^2, which is
the same function as the reference's sum over theta^(2i) and has a plain derivative at w = 0 (zero, what autograd gives the
reference there).

Bounds (the issue's): forward, every element within ONE fp32 spacing of the float64 value -- a double result rounded once is within
half a spacing, the other half covers double rounding; gradients, relative L2 per tensor <= 2^-22 -- a correctly rounded result is
<= 2^-24, the margin covers cancellation between terms.  The torch restatement (sparf_amd.camera.*_torch) runs in fp32 like the
reference and is held to 4x the reference's own distance from this referee on the same fixture case."""
import math
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose.npz")
NS = (1, 3, 65)                     # 65: a second 64-thread workgroup with one live lane
XI_CASES = ("zero", "s1e-7", "s0.05", "s1.5", "w3.1")
D9_CASES = ("init", "generic")
GRAD_BOUND = 2.0 ** -22
TERMS = 11


def fixture():
    return dict(np.load(FIXTURE))


def f64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).clone()


def _poly(x, k):
    return sum((-1.0) ** i * x ** i / float(math.factorial(2 * i + k)) for i in range(TERMS))


def _skew(w):
    O = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([O, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], O, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], O], -1)], -2)


def se3(xi):
    w, u = xi[..., :3], xi[..., 3:]
    x = (w * w).sum(-1)[..., None, None]
    wx = _skew(w)
    wx2 = wx @ wx
    I = torch.eye(3, dtype=xi.dtype)
    R = I + _poly(x, 1) * wx + _poly(x, 2) * wx2
    V = I + _poly(x, 2) * wx + _poly(x, 3) * wx2
    return torch.cat([R, V @ u[..., None]], -1)


def compose(a, b):
    return torch.cat([b[..., :3] @ a[..., :3], b[..., :3] @ a[..., 3:] + b[..., 3:]], -1)


def invert(p):
    Rt = p[..., :3].transpose(-1, -2)
    return torch.cat([Rt, -Rt @ p[..., 3:]], -1)


def _normalize(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def d9_pose(d9, inv=False):
    t, a1, a2 = d9[..., :3], d9[..., 3:6], d9[..., 6:]
    b1 = _normalize(a1)
    b2 = _normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1)
    p = torch.cat([torch.stack([b1, b2, torch.linalg.cross(b1, b2, dim=-1)], -2), t[..., None]], -1)
    return invert(p) if inv else p


def vjp(fn, inputs, grads):
    """fn(*inputs) -> tensor or tuple of tensors; grads: matching upstream gradients (None = no gradient on that output)
    -> (outputs as float64 numpy, gradients w.r.t. every input as float64 numpy)"""
    xs = [f64(x).requires_grad_() for x in inputs]
    out = fn(*xs)
    outs = out if isinstance(out, tuple) else (out,)
    loss = sum((o * f64(g)).sum() for o, g in zip(outs, grads) if g is not None)
    gs = torch.autograd.grad(loss, xs, allow_unused=True)
    return [o.detach().numpy() for o in outs], [g.numpy() if g is not None else np.zeros(x.shape) for g, x in zip(gs, xs)]


def se3_chain(xi, base):
    r = se3(xi)
    return compose(r, base), r


def to_np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def fwd_excess(got, want64):
    """max over elements of |got - want| / spacing(fp32(|want|)): <= 1 passes"""
    got, want64 = to_np(got).astype(np.float64), np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, (got.shape, want64.shape)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want64) / np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)))


def fwd_abs(got, want64):
    got = to_np(got).astype(np.float64)
    return float(np.max(np.abs(got - want64))) if got.size else 0.0


def rel_l2(got, want64):
    got, want64 = to_np(got).astype(np.float64), np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, (got.shape, want64.shape)
    den = float(np.sqrt((want64 ** 2).sum()))
    num = float(np.sqrt(((got - want64) ** 2).sum()))
    return num / den if den > 0 else num
