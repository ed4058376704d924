"""A stand-in for the loaded library under ops.Se3Pose / ComposePose / D9Pose (tests/fake_lib.Recorder over the six pose entry points)."""
from tests import fake_lib

POSE_CALLS = {
    "sparf_pose_se3_forward": ("xi", "base", "n", "refine_out", "pose_out"),
    "sparf_pose_se3_backward": ("xi", "base", "n", "d_pose", "d_refine", "d_xi", "d_base"),
    "sparf_pose_compose_forward": ("a", "b", "n", "out"),
    "sparf_pose_compose_backward": ("a", "b", "n", "d_out", "d_a", "d_b"),
    "sparf_pose_d9_forward": ("d9", "invert", "n", "pose_out"),
    "sparf_pose_d9_backward": ("d9", "invert", "n", "d_pose", "d_d9"),
}


def installed():
    return fake_lib.installed(fake_lib.Recorder(POSE_CALLS))
