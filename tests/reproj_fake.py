"""A stand-in for the loaded library under ops.ReprojLoss / ReprojPairLoss (tests/fake_lib.Recorder over the two entry points of the
correspondence loss).  The workspace query answers as the library does (host arithmetic) and is not recorded."""
from tests import fake_lib

_OPTS = ("n", "loss_type", "pix_check", "pix_thresh", "depth_check", "depth_thresh")
REPROJ_CALLS = {
    "sparf_reproj_loss": ("pixels_i", "depth_i", "K_i", "pixels_j", "depth_j", "K_j", "T_itoj", "weights") + _OPTS +
                         ("out", "d_depth_i", "d_T", "valid", "workspace"),
    "sparf_reproj_pair_loss": ("pixels_self", "pixels_other", "depth_self", "depth_other", "depth_fine_self", "depth_fine_other", "K_self",
                               "K_other", "pose_self", "pose_other", "weights") + _OPTS +
                              ("out", "d_depth_self", "d_depth_other", "d_depth_fine_self", "d_depth_fine_other", "d_pose_self", "d_pose_other",
                               "workspace"),
}
SINGLE_MAX = 4096                # csrc/reproj.h REPROJ_SINGLE_MAX
WORKSPACE_BYTES = 4 * 64 * 21 * 8


class ReprojFakeLib(fake_lib.Recorder):
    def __init__(self):
        super().__init__(REPROJ_CALLS)

    def sparf_reproj_workspace_bytes(self, n):
        return WORKSPACE_BYTES if n > SINGLE_MAX else 0


def installed():
    return fake_lib.installed(ReprojFakeLib())
