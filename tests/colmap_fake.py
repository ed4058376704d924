"""A stand-in for the loaded library under ops.colmap_compact / ops.colmap_gather / ops.ColmapLoss (tests/fake_lib.Recorder over
the three entry points of the DS-NeRF sparse depth loss).  The tensors are host memory here, so compact answers
through its `count` pointer with the counts of `valid` / `positive` (default: what tests/colmap_referee.py counts in the map behind the
`depth` pointer) -- the glue's one readback then reads numbers --, gather fills its outputs from the maps as the kernel would, and loss
writes 0.  The workspace query answers as the library does and is not recorded.
Also here: DepthNet, the `net` of a loss module whose render is an exact function of the image and the ray list."""
import ctypes

import numpy as np
import torch

from tests import fake_lib

COLMAP_CALLS = {
    "sparf_colmap_compact": ("depth", "B", "H", "W", "index", "count", "workspace"),
    "sparf_colmap_gather": ("index", "count", "sel", "B", "H", "W", "quota", "K", "depth", "conf", "ray_idx", "target", "weight"),
    "sparf_colmap_loss": ("target", "weight", "count", "B", "quota", "K", "depth", "depth_fine", "out", "d_depth", "d_depth_fine", "workspace"),
}
CHUNK = 4096                     # csrc/colmap.h COLMAP_CHUNK


def workspace_bytes(B, n, rows):
    chunks = lambda m: (m + CHUNK - 1) // CHUNK
    return max(B * chunks(n) * 8 if B > 0 and n > CHUNK else 0, chunks(rows) * 8 if rows > CHUNK else 0)


def _array(address, n, dtype):
    size = n * np.dtype(dtype).itemsize
    return np.frombuffer((ctypes.c_char * size).from_address(address), dtype=dtype)


class ColmapFakeLib(fake_lib.Recorder):
    def __init__(self):
        super().__init__(COLMAP_CALLS)
        self.valid = self.positive = None        # per-image counts compact reports (None: counted in the map)

    def sparf_colmap_workspace_bytes(self, B, n, rows):
        return workspace_bytes(B, n, rows)

    def after(self, name, raw, rec):
        getattr(self, "_" + name[len("sparf_colmap_"):])(raw)

    def _compact(self, a):
        B, n = a["B"], a["H"] * a["W"]
        depth = _array(a["depth"], B * n, np.float32).reshape(B, n)
        index, count = _array(a["index"], B * n, np.int32).reshape(B, n), _array(a["count"], 2 * B, np.int32)
        for b in range(B):
            idx = np.nonzero(depth[b] > np.float32(1e-6))[0]
            if self.valid is not None:
                idx = np.arange(min(self.valid[b], n))
            index[b, :len(idx)] = idx
            count[b] = len(idx)
            count[B + b] = int((depth[b] > 0).sum()) if self.positive is None else self.positive[b]

    def _gather(self, a):
        B, n, quota = a["B"], a["H"] * a["W"], a["quota"]
        index, count = _array(a["index"], B * n, np.int32).reshape(B, n), _array(a["count"], B, np.int32)
        depth, conf = (_array(a[k], B * n, np.float32).reshape(B, n) for k in ("depth", "conf"))
        outs = [_array(a[k], a["K"], t) for k, t in (("ray_idx", np.int64), ("target", np.float32), ("weight", np.float32))]
        r = 0
        for b in range(B):
            k = min(int(count[b]), quota)
            pos = _array(a["sel"] + 8 * b * quota, k, np.int64) if a["sel"] and count[b] > quota else np.arange(k)
            p = index[b][np.clip(pos, 0, max(int(count[b]) - 1, 0))] if k else np.zeros(0, dtype=np.int64)
            outs[0][r:r + k], outs[1][r:r + k], outs[2][r:r + k] = p, depth[b][p], conf[b][p]
            r += k
        assert r == a["K"], (r, a["K"])

    def _loss(self, a):
        ctypes.c_float.from_address(a["out"]).value = 0.0
        for k in ("d_depth", "d_depth_fine"):
            if a[k]:
                _array(a[k], a["K"], np.float32)[:] = 0.0


def installed():
    return fake_lib.installed(ColmapFakeLib())


class DepthNet:
    """the `net` of a SparseCOLMAPDepthLoss: poses whose [0, 3] entry is the image's number, and a render whose depth is an exact
    function of that number and of ray_idx (tests/colmap_referee.rendered_np); records the ray list of every call"""

    def __init__(self, B, fine=True, device="cpu", grad=False):
        self.calls, self.fine = [], fine
        self.pose = torch.eye(4)[:3].repeat(B, 1, 1).to(device)
        self.pose[:, 0, 3] = torch.arange(B, dtype=torch.float32)
        self.scale = torch.ones((), device=device, requires_grad=grad)           # what a gradient is taken to

    def get_w2c_pose(self, opt, data_dict, mode=None):
        return self.pose

    def render_image_at_specific_pose_and_rays(self, opt, data_dict, pose, intr, H, W, ray_idx=None, mode=None, iter=None):
        from sparf_amd.edict import EasyDict as edict
        assert pose.shape == (3, 4) and mode == "train" and ray_idx.dtype == torch.int64
        self.calls.append(ray_idx.clone())
        d = (2.0 + 0.25 * pose[0, 3] + ((ray_idx * 37) % 101).to(torch.float32) / 128.0) * self.scale
        ret = edict(depth=d[None, :, None], rgb=torch.zeros(1, len(ray_idx), 3))
        if self.fine:
            ret.depth_fine = (d + 0.0625 * self.scale)[None, :, None]
        return ret
