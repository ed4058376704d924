"""The pose-evaluation kernels on the GPU (csrc/pose_eval.hip behind sparf_amd.pose_eval): every case of
tests/pose_eval_referee.py against the float64 referee -- one fp32 spacing of the referee's value per finite output (taken at the floors
that file derives), NaN in the same places, the index equal -- and against the reference's own recorded values; sets against single
calls, repeated calls and replays of a captured graph bit for bit; the backtrack round trip; the installed methods.  Fixtures only.
Run with `pytest -m gpu`."""
import types

import numpy as np
import pytest
import torch

from sparf_amd import camera
from sparf_amd import pose_eval as PE
from sparf_amd.edict import EasyDict as edict
from tests import pose_eval_referee as R

pytestmark = pytest.mark.gpu
OUTPUTS = ("stats", "errors", "aligned", "sim3", "scores")


def dev():
    return torch.device("cuda:0")


def D(a):
    return torch.from_numpy(np.array(a)).to(dev())


def operands(name):
    pose, gt = R.inputs(name)
    return D(pose), D(gt) if R.CASES[name]["gt_sets"] > 1 else D(gt[0])


@pytest.fixture(scope="module")
def results():
    """per case, computed once: the inputs, the referee's values and the kernel's (on the host, with a leading set axis)"""
    cache = {}

    def get(name):
        if name not in cache:
            pose, gt = R.inputs(name)
            res = PE.evaluate_poses(*operands(name), align=R.CASES[name]["align"])
            assert all(res[k].is_cuda and res[k].dtype == torch.float32 for k in OUTPUTS if k != "sim3") and res.best.dtype == torch.int32
            assert res.sim3.packed.is_cuda and res.sim3.type == 'traj_align'
            cache[name] = (pose, gt, R.want(pose, gt, R.CASES[name]["align"]), R.result_arrays(res))
        return cache[name]
    return get


@pytest.mark.parametrize("name", R.CASES)
def test_kernel_against_the_referee(results, name):
    pose, gt, w, got = results(name)
    c = R.CASES[name]
    print(name, "best", got["best"], "referee", w["best"])
    assert np.array_equal(got["best"], w["best"])
    assert got["scores"].shape == w["scores"].shape
    for s in range(c["S"]):
        gs, ws = R.set_of(got, s), R.set_of(w, s)
        d = R.distances(gs, ws)
        print(name, s, "kernel to float64, worst of each output:", {k: R.worst({k: v}) for k, v in d.items()}, "fp32 spacings")
        for k in OUTPUTS:
            assert R.same_pattern(gs[k], ws[k]), (k, gs[k], ws[k])
        assert R.worst(d) <= R.BOUND, d
        if not c["align"]:
            assert np.array_equal(gs["aligned"], pose[s]) and np.array_equal(gs["sim3"], np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float32))
            assert np.array_equal(gs["errors"][0], gs["errors"][1]) and np.array_equal(gs["stats"][:2], gs["stats"][2:])
    if name == "coincident_b3":
        assert got["best"][0] == 0 and np.isnan(got["scores"][0, [0, 2]]).all() and np.isfinite(got["scores"][0, [1, 3, 4, 5]]).all() and np.isnan(got["aligned"]).all()
    if name == "identity_b3":
        assert np.isnan(got["scores"]).all() and np.isnan(got["stats"][0, 2:]).all() and np.isfinite(got["stats"][0, :2]).all() and np.isfinite(got["errors"][0, 0]).all()
    if name.startswith("exact"):
        assert (got["errors"][0, 1, :, 0] == np.float32(np.arccos(R.CLAMP))).all()          # every pose on the reference's floor


@pytest.mark.parametrize("name", R.CASES)
def test_kernel_against_the_references_recorded_values(results, name):
    """no farther from the reference's value than the reference's own distance from float64 plus the kernel's bound; its index where
    the case is decisive"""
    fx = R.fixture()
    pose, gt, w, got = results(name)
    dec = fx[f"decisive_{name}"]
    assert np.array_equal(got["best"][dec], fx[f"ref_best_{name}"][dec])
    for s in range(R.CASES[name]["S"]):
        gs, ws = R.set_of(got, s), R.set_of(w, s)
        for k in ("stats", "aligned", "sim3", "scores"):
            ref, refdist = fx[f"ref_{k}_{name}"][s], fx[f"refdist_{k}_{name}"][s]
            assert R.same_pattern(gs[k], ref), (k, gs[k], ref)
            d = R.distances(gs, ws, against={k: ref})[k]                                     # in the spacings of the referee's value
            fin = np.isfinite(d)
            print(name, s, k, "kernel to reference:", d[fin].max() if fin.any() else 0.0, "reference to float64:", refdist[fin].max() if fin.any() else 0.0)
            assert (d[fin] <= refdist[fin] + R.BOUND).all(), (k, d, refdist)


def bits(res):
    return [res[k].cpu().numpy().copy().view(np.uint32) for k in ("stats", "errors", "aligned", "scores")] + \
        [res.sim3.packed.cpu().numpy().copy().view(np.uint32), res.best.cpu().numpy().copy()]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["s3_gt1_n0.05", "s3_gt3_n0.3", "noalign_s3"])
def test_sets_give_the_bits_of_single_calls_and_calls_repeat(name):
    pose, gt = operands(name)
    align = R.CASES[name]["align"]
    whole = PE.evaluate_poses(pose, gt, align=align)
    assert same(bits(PE.evaluate_poses(pose, gt, align=align)), bits(whole))
    for s in range(pose.shape[0]):
        one = PE.evaluate_poses(pose[s], gt[s] if gt.dim() == 4 else gt, align=align)
        assert one.stats.shape == (4,) and one.best.dim() == 0
        part = edict({k: whole[k][s] for k in ("stats", "errors", "aligned", "scores", "best")}, sim3=PE.sim3_of(whole.sim3.packed[s]))
        assert same(bits(one), bits(part)), s


def chain(pose, gt, test_gt):
    res = PE.evaluate_poses(pose, gt)
    return res, PE.backtrack(test_gt, res.sim3)


def test_graph_replays_give_the_eager_bits():
    """a capture of evaluate_poses + backtrack on one stream, no parallel branches, no readback inside"""
    pose, gt = operands("b9_n0.05")
    test_gt = D(R.inputs("b3_n0.3")[1][0])
    res, back = chain(pose, gt, test_gt)
    eager = bits(res) + [back.cpu().numpy().view(np.uint32).copy()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(pose, gt, test_gt)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, back = chain(pose, gt, test_gt)
    for _ in range(2):
        for t in (res.stats, res.errors, res.aligned, res.sim3.packed, res.best, back):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same(bits(res) + [back.cpu().numpy().view(np.uint32).copy()], eager)


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["S"] == 1 and n not in R.DEGENERATE])
def test_backtrack_against_the_referee_and_the_round_trip(results, name):
    """backtrack of the ground truth under the returned similarity: within a spacing of the referee's backtrack under the same 13 floats,
    and as close to the estimated poses as the referee's own round trip (recorded by the generator) plus one spacing"""
    pose, gt, w, got = results(name)
    sim = got["sim3"][0]
    back = PE.backtrack(D(gt[0]), PE.sim3_of(D(sim))).cpu().numpy()
    B, fl = pose.shape[1], w["floor"][0]
    d = R.spacings(back, R.backtrack(gt[0], sim), R.pose_floor(B, fl))
    rt = R.spacings(back, pose[0].astype(np.float64), R.pose_floor(B, fl))
    figure = R.fixture()[f"roundtrip_{name}"][0]
    print(name, "backtrack to float64:", np.nanmax(d), "round trip:", np.nanmax(rt), "referee's:", figure)
    assert np.nanmax(d) <= R.BOUND
    assert np.nanmax(rt) <= figure + 1.0
    loose = edict(R=D(sim[:9]).reshape(1, 3, 3), t=D(sim[9:12]).reshape(1, 3, 1), s=float(sim[12]), type='traj_align')     # a Python float s
    assert np.array_equal(PE.backtrack(D(gt[0]), loose).cpu().numpy().view(np.uint32), back.view(np.uint32))


class _Trainer:
    """a stand-in for CommonPoseEvaluation"""
    def __init__(self, fixed=1):
        self.settings = edict(camera=edict(n_first_fixed_poses=fixed))
        self.device = dev()


def test_installed_methods_and_the_pose_chain_on_the_device():
    pose, gt = operands("b9_n0.05")
    pose = pose[0]                                           # [B,3,4], as a trainer hands them
    res = PE.evaluate_poses(pose, gt)
    mod = types.SimpleNamespace(backtrack_from_aligning_the_trajectory=PE.backtrack_torch)
    cam = types.SimpleNamespace(lie=types.SimpleNamespace(), pose=types.SimpleNamespace())
    PE.install(_Trainer, mod)
    camera.install(cam)
    try:
        tr = _Trainer()
        st = tr.evaluate_any_poses(None, pose, gt)
        assert list(st) == list(PE.STATS)
        for i, v in enumerate(st.values()):
            assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda and torch.equal(v, res.stats[i])
        aligned, sim3 = tr.prealign_w2c_small_camera_systems(None, pose, gt)
        assert torch.equal(aligned, res.aligned) and torch.equal(sim3.packed, res.sim3.packed) and sim3.s.dim() == 0 and sim3.type == 'traj_align'
        err = tr.evaluate_camera_alignment(None, res.aligned, gt)
        # on the STORED aligned poses: the referee on those fp32 operands, both errors within the bound
        stored = R.want(res.aligned.cpu().numpy()[None], gt.cpu().numpy()[None], False)
        got = torch.stack([err.R, err.t], dim=-1).cpu().numpy()
        d = R.spacings(got, stored["errors"][0, 0], np.broadcast_to(np.array([0, stored["floor"][0]]), got.shape))
        print("installed evaluate_camera_alignment on the stored aligned poses, to float64:", d.max(axis=0))
        assert err.R.shape == err.t.shape == (9,) and d.max() <= R.BOUND
        before = tr.evaluate_camera_alignment(None, pose, gt)
        assert torch.equal(before.R, res.errors[0, :, 0]) and torch.equal(before.t, res.errors[0, :, 1])
        fixed = _Trainer(fixed=2)
        st = fixed.evaluate_any_poses(None, pose, gt)
        assert torch.equal(st["error_R"], res.stats[0]) and torch.equal(st["error_t"], res.stats[1])
        # Graph.get_w2c_pose in mode test-optim (joint_pose_nerf_trainer.py:728-739): the backtrack, then compose with the refinement
        test_gt = D(R.inputs("b3_n0.3")[1][0][:1])
        refine = D(np.array([[[0.995, -0.0998, 0, 0.01], [0.0998, 0.995, 0, -0.02], [0, 0, 1, 0.03]]], dtype=np.float32))
        chained = cam.pose.compose_pair_b_at_a(pose_a=refine, pose_b=mod.backtrack_from_aligning_the_trajectory(test_gt, sim3))
        back = PE.backtrack(test_gt, res.sim3)
        assert torch.equal(chained, camera.pose.compose_pair_b_at_a(refine, back)) and chained.shape == (1, 3, 4) and chained.is_cuda
        want = R.backtrack(test_gt.cpu().numpy(), res.sim3.packed.cpu().numpy())
        assert np.nanmax(R.spacings(back.cpu().numpy(), want, R.pose_floor(1, float(np.linalg.norm(R.invert(want)[0, :, 3]))))) <= R.BOUND
    finally:
        camera.uninstall()
        PE.uninstall()
