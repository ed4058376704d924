"""Pose evaluation without a GPU (sparf_amd/pose_eval.py, csrc/pose_eval.hip): the torch restatement against the
float64 referee (tests/pose_eval_referee.py) and against the reference's recorded values (tests/golden/pose_eval.npz), the argument checks
of the two entry points, and the glue on a stand-in library (tests/pose_eval_fake.py): one call per function, every hand-over rule, the
install / uninstall round trip, the result's keys and shapes."""
import ctypes
import types

import numpy as np
import pytest
import torch

from sparf_amd import lib as L
from sparf_amd import pose_eval as PE
from sparf_amd.edict import EasyDict as edict
from tests import pose_eval_fake
from tests import pose_eval_referee as R


def T(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return t if dtype is None else t.to(dtype)


def run_torch(name, dtype):
    c = R.CASES[name]
    pose, gt = R.inputs(name)
    gt_t = T(gt, dtype) if c["gt_sets"] > 1 else T(gt[0], dtype)
    return R.result_arrays(PE.evaluate_poses_torch(T(pose, dtype), gt_t, c["align"])), pose, gt


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_in_float64_against_the_referee(name, monkeypatch):
    """the same lines on the same operands, in another operation order (torch's matmul): a tenth of an fp32 spacing -- a centre distance
    of 1e-7 between centres of norm 10 carries 1e-15 of them, 1e-8 of itself, and acos at the clamp amplifies 1e-16 by 2e3.  A
    float64 tensor clamps at 1 - 1e-7 itself, not at its fp32 rounding: the referee is given that bound for this comparison (its own
    is pinned by test_clamp_floor_of_an_exact_alignment and by the float32 comparisons)."""
    monkeypatch.setattr(R, "CLAMP", 1.0 - 1e-7)
    got, pose, gt = run_torch(name, torch.float64)
    w = R.want(pose, gt, R.CASES[name]["align"])
    assert np.array_equal(got["best"], w["best"])
    for s in range(pose.shape[0]):
        gs, ws = R.set_of(got, s), R.set_of(w, s)
        for k in ("stats", "errors", "aligned", "sim3", "scores"):
            assert R.same_pattern(gs[k], ws[k]), (k, gs[k], ws[k])
        assert R.worst(R.distances(gs, ws)) <= 0.1


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_in_float32_against_the_recorded_reference(name):
    """Both are fp32 evaluations of the same lines; each lies from float64 as far as the recorded distance of the reference at most, so
    they are no farther apart than twice that (+ 2 spacings for the roundings of the comparison).  The index is the reference's where
    the case is decisive."""
    fx = R.fixture()
    got, pose, gt = run_torch(name, torch.float32)
    w = R.want(pose, gt, R.CASES[name]["align"])
    dec = fx[f"decisive_{name}"]
    assert np.array_equal(got["best"][dec], fx[f"ref_best_{name}"][dec])
    for s in range(pose.shape[0]):
        ws = R.set_of(w, s)
        ref = dict(stats=fx[f"ref_stats_{name}"][s], errors=ws["errors"], aligned=fx[f"ref_aligned_{name}"][s], sim3=fx[f"ref_sim3_{name}"][s],
                   scores=fx[f"ref_scores_{name}"][s])
        gs = R.set_of(got, s)
        same_choice = got["best"][s] == fx[f"ref_best_{name}"][s]
        for k in ("stats", "aligned", "sim3", "scores"):
            if k in ("aligned", "sim3") and not same_choice:
                continue                                 # another candidate's poses (an undecisive case)
            assert R.same_pattern(gs[k], ref[k]), (k, gs[k], ref[k])
            fin = np.isfinite(ws[k])
            mine, theirs = R.distances(dict(ref, **{k: gs[k]}), ws)[k], fx[f"refdist_{k}_{name}"][s]
            assert (mine[fin] <= 2 * theirs[fin] + 2).all(), (k, mine, theirs)


def test_backtrack_restatement_against_the_referee_and_the_reference():
    """in float32 against the recorded reference, in the spacings and floors of the referee: both are fp32 evaluations of the same lines,
    so the restatement lies from float64 no farther than twice the reference's own distance (+ 2 for the roundings of the comparison)"""
    fx = R.fixture()
    for name in ("b3_n0.05", "b9_n0.3", "exact_b3", "noalign_b3"):
        pose, gt = R.inputs(name)
        sim = fx[f"ref_sim3_{name}"][0]
        sim3 = edict(R=T(sim[:9]).reshape(1, 3, 3), t=T(sim[9:12]).reshape(1, 3, 1), s=T(sim[12]))
        want = R.backtrack(gt[0], sim)
        floor = R.pose_floor(len(want), R.want(pose, gt, R.CASES[name]["align"])["floor"][0])
        mine = R.spacings(PE.backtrack_torch(T(gt[0]), sim3).numpy(), want, floor)
        theirs = R.spacings(fx[f"ref_back_{name}"][0], want, floor)
        assert (mine <= 2 * theirs + 2).all(), (name, mine, theirs)
        sim64 = edict(R=sim3.R.double(), t=sim3.t.double(), s=float(sim[12]))              # a Python float s: the large-system path's form
        assert np.allclose(PE.backtrack_torch(T(gt[0], torch.float64), sim64).numpy(), R.backtrack(gt[0], sim), rtol=0, atol=1e-12)


def test_the_rule_of_the_choice_and_the_candidate_order():
    assert [PE.pair_of(p, 3) for p in range(6)] == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    assert PE.n_pairs(2) == 2 and PE.n_pairs(9) == 72 and PE.n_pairs(10) == 90 and PE.n_pairs(12) == 90 and PE.pair_of(89, 12) == (9, 8)
    fx = R.fixture()
    sc = fx["ref_scores_coincident_b3"][0][:, 2]
    assert np.isnan(sc[[0, 2]]).all() and np.isfinite(sc[[1, 3, 4, 5]]).all() and fx["ref_best_coincident_b3"][0] == 0
    got, pose, gt = run_torch("coincident_b3", torch.float32)
    assert got["best"][0] == 0 and np.isnan(got["aligned"]).all() and np.isnan(got["stats"][0, 2:]).all() and np.isfinite(got["stats"][0, :2]).all()
    got, pose, gt = run_torch("identity_b3", torch.float32)
    assert got["best"][0] == 0 and np.isnan(got["scores"]).all() and np.isfinite(got["errors"][0, 0]).all() and np.isnan(got["errors"][0, 1]).all()


def test_clamp_floor_of_an_exact_alignment():
    """every aligned pose of an exact similarity sits on the reference's floor acos(float32(1 - 1e-7)) = 4.8828e-4 rad, not float64's 4.4721e-4"""
    assert R.CLAMP == float(np.float32(1 - 1e-7)) and abs(np.arccos(R.CLAMP) - 4.8828e-4) < 1e-8
    pose, gt = R.inputs("exact_b3")
    w = R.want(pose, gt)
    assert (w["errors"][0, 1, :, 0] == np.arccos(R.CLAMP)).all()
    ref = R.fixture()["ref_stats_exact_b3"][0, 2]                  # (the mean and the degrees in fp32: a spacing or two)
    assert abs(ref - np.arccos(R.CLAMP) * 180. / np.pi) <= 2 * np.spacing(ref) < abs(ref - np.arccos(1 - 1e-7) * 180. / np.pi)


# ---- the C ABI
def test_abi_version_and_argument_checks():
    lib = L.load()
    assert L.ABI_VERSION == 7 and lib.sparf_abi_version() == 7
    p = ctypes.c_void_p(64)                                   # any non-NULL address: every check comes before a HIP call
    full = dict(pose=p, pose_gt=p, gt_sets=1, S=1, B=3, flags=L.POSE_EVAL_ALIGN, stats=p, errors=p, aligned=p, sim3=p, best=p, scores=None)
    call = lambda **kw: lib.sparf_pose_eval(ctypes.byref(L.PoseEval(**dict(full, **kw))), None)
    assert lib.sparf_pose_eval(None, None) == 1
    assert call(S=0) == 0 and call(S=0, pose=None, stats=None, B=1000) == 0                    # nothing to do, whatever else it holds
    assert call(S=-1) == 1 and call(B=-1) == 1 and call(B=0) == 1 and call(B=L.POSE_EVAL_MAX_POSES + 1) == 1
    assert call(B=1) == 1 and call(flags=2) == 1 and call(gt_sets=2) == 1 and call(gt_sets=0) == 1
    for name in ("pose", "pose_gt", "stats", "errors", "aligned", "sim3", "best"):
        assert call(**{name: None}) == 1, name
    assert lib.sparf_pose_backtrack(None, 0, None, 0, None, None) == 0
    assert lib.sparf_pose_backtrack(p, -1, p, 0, p, None) == 1 and lib.sparf_pose_backtrack(p, 2, p, -13, p, None) == 1
    assert lib.sparf_pose_backtrack(None, 2, p, 0, p, None) == 1 and lib.sparf_pose_backtrack(p, 2, None, 0, p, None) == 1
    assert lib.sparf_pose_backtrack(p, 2, p, 0, None, None) == 1
    assert ctypes.sizeof(L.PoseEval) == 80 and L.POSE_EVAL_MAX_PAIRS == R.MAX_PAIRS == PE.MAX_PAIRS


# ---- the glue on the stand-in library
def some(B, S=None, dtype=torch.float32):
    rs = np.random.RandomState(B)
    shape = (B, 3, 4) if S is None else (S, B, 3, 4)
    return T(rs.standard_normal(shape), dtype), T(rs.standard_normal(shape), dtype)


def test_one_call_per_function_and_the_result():
    with pose_eval_fake.installed() as lib:
        pose, gt = some(3)
        res = PE.evaluate_poses(pose, gt)
        assert len(lib.calls) == 1
        c = lib.calls[0]
        assert (c["entry"], c["S"], c["B"], c["gt_sets"], c["flags"]) == ("sparf_pose_eval", 1, 3, 1, L.POSE_EVAL_ALIGN)
        assert c["pose"] == pose.data_ptr() and c["pose_gt"] == gt.data_ptr()
        assert set(res) == {"stats", "errors", "aligned", "best", "scores", "sim3"}
        assert set(res.sim3) == {"R", "t", "s", "type", "packed"} and res.sim3.type == 'traj_align'
        assert (res.stats.shape, res.errors.shape, res.aligned.shape, res.best.shape, res.scores.shape) == ((4,), (2, 3, 2), (3, 3, 4), (), (6, 3))
        assert (res.sim3.R.shape, res.sim3.t.shape, res.sim3.s.shape, res.sim3.packed.shape) == ((1, 3, 3), (1, 3, 1), (), (13,))
        assert res.best.dtype == torch.int32 and int(res.best) == pose_eval_fake.BEST and tuple(res.stats.tolist()) == pose_eval_fake.STATS
        for v in (res.sim3.R, res.sim3.t, res.sim3.s):                                        # views of the packed 13 floats
            assert v.untyped_storage().data_ptr() == res.sim3.packed.untyped_storage().data_ptr()
        # sets, with one ground truth and with one per set
        pose4, gt4 = some(5, S=2)
        res = PE.evaluate_poses(pose4, gt4[0], align=False)
        c = lib.calls[-1]
        assert len(lib.calls) == 2 and (c["S"], c["B"], c["gt_sets"], c["flags"]) == (2, 5, 1, 0)
        assert (res.stats.shape, res.errors.shape, res.aligned.shape, res.best.tolist(), res.scores.shape) == ((2, 4), (2, 2, 5, 2), (2, 5, 3, 4), [-1, -1], (2, 0, 3))
        assert (res.sim3.R.shape, res.sim3.t.shape, res.sim3.s.shape, res.sim3.packed.shape) == ((2, 1, 3, 3), (2, 1, 3, 1), (2,), (2, 13))
        res = PE.evaluate_poses(pose4, gt4)
        assert len(lib.calls) == 3 and lib.calls[-1]["gt_sets"] == 2 and res.scores.shape == (2, 20, 3)
        # backtrack: the packed similarity as it is; R, t and a Python float packed otherwise
        n = len(lib.calls)
        sim = PE.sim3_of(torch.arange(13, dtype=torch.float32))
        out = PE.backtrack(gt, sim)
        c = lib.calls[-1]
        assert len(lib.calls) == n + 1 and (c["entry"], c["n"], c["sim3_stride"], c["sim3"]) == ("sparf_pose_backtrack", 3, 0, sim.packed.data_ptr())
        assert torch.equal(out, gt + 1)
        loose = edict(R=torch.eye(3).unsqueeze(0), t=torch.tensor([1., 2., 3.]).reshape(1, 3, 1), s=2.5, type='traj_align')
        PE.backtrack(gt, loose)
        assert len(lib.calls) == n + 2 and lib.calls[-1]["sim3_values"] == (1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 2, 3, 2.5)
        # a packed similarity of another dtype (the restatement's on float64 operands) is converted, not handed over as it lies
        PE.backtrack(gt, PE.sim3_of(torch.arange(13, dtype=torch.float64) / 4))
        assert len(lib.calls) == n + 3 and lib.calls[-1]["sim3_values"] == tuple(i / 4 for i in range(13))
        with pytest.raises(ValueError):
            PE.evaluate_poses(pose, gt4)
        with pytest.raises(ValueError):
            PE.evaluate_poses(pose4, some(5, S=3)[1])


def test_hand_over_rules():
    with pose_eval_fake.installed() as lib:
        pose, gt = some(3)
        want = PE.evaluate_poses_torch(pose, gt)
        same = lambda a: torch.equal(a.stats, want.stats) and torch.equal(a.aligned, want.aligned) and int(a.best) == int(want.best)
        with PE.unfused():
            assert same(PE.evaluate_poses(pose, gt))
            PE.backtrack(gt, want.sim3)
        res64 = PE.evaluate_poses(pose.double(), gt.double())                               # float64
        assert res64.stats.dtype == torch.float64 and res64.sim3.packed.dtype == torch.float64
        PE.backtrack(gt.double(), res64.sim3)
        big, big_gt = some(L.POSE_EVAL_MAX_POSES + 1)                                       # more than 64 poses
        assert PE.evaluate_poses(big, big_gt).scores.shape == (90, 3)
        one, one_gt = some(1)                                                               # fewer than two: the reference's own failure
        with pytest.raises(ValueError):
            PE.evaluate_poses(one, one_gt)
        first = edict(want.sim3, type='align_to_first')                                     # another kind of similarity
        assert torch.equal(PE.backtrack(gt, first), PE.backtrack_torch(gt, first))
        assert lib.calls == []
        assert PE.evaluate_poses(one, one_gt, align=False).best == -1 and len(lib.calls) == 1  # one pose without the search is the kernel's
    pose, gt = some(3)
    assert PE.evaluate_poses(pose, gt).stats.device.type == "cpu"                           # CPU tensors, the real predicate


class _Trainer:
    """a stand-in for CommonPoseEvaluation: the three methods answer with their names"""
    device = torch.device("cpu")

    def __init__(self, fixed=1):
        self.settings = edict(camera=edict(n_first_fixed_poses=fixed))

    def evaluate_camera_alignment(self, opt, a, b):
        return "original evaluate_camera_alignment"

    def prealign_w2c_small_camera_systems(self, opt, a, b):
        return "original prealign_w2c_small_camera_systems"

    def evaluate_any_poses(self, opt, a, b):
        return "original evaluate_any_poses"


class _Sub(_Trainer):
    pass


def test_install_and_uninstall_round_trip():
    def original_backtrack(pose, sim3):
        return "original backtrack"
    align_mod = types.SimpleNamespace(backtrack_from_aligning_the_trajectory=original_backtrack, other=1)
    trainer_mod = types.SimpleNamespace(backtrack_from_aligning_the_trajectory=original_backtrack)
    unrelated = types.SimpleNamespace(x=1)
    before = dict(vars(_Trainer))
    PE.install(_Trainer, align_mod, trainer_mod, unrelated)
    try:
        with pytest.raises(RuntimeError):
            PE.install(_Trainer)
        assert align_mod.backtrack_from_aligning_the_trajectory is PE.backtrack and trainer_mod.backtrack_from_aligning_the_trajectory is PE.backtrack
        assert not hasattr(unrelated, "backtrack_from_aligning_the_trajectory")
        with pose_eval_fake.installed() as lib:
            tr = _Sub()
            pose, gt = some(6)
            st = tr.evaluate_any_poses(None, pose, gt)
            assert len(lib.calls) == 1 and lib.calls[0]["flags"] == L.POSE_EVAL_ALIGN and list(st) == list(PE.STATS)
            assert all(v.dim() == 0 and v.dtype == torch.float32 for v in st.values()) and tuple(float(v) for v in st.values()) == pose_eval_fake.STATS
            aligned, sim3 = tr.prealign_w2c_small_camera_systems(None, pose, gt)
            assert len(lib.calls) == 2 and aligned.shape == (6, 3, 4) and sim3.type == 'traj_align' and sim3.R.shape == (1, 3, 3)
            err = tr.evaluate_camera_alignment(None, pose, gt)
            assert len(lib.calls) == 3 and lib.calls[-1]["flags"] == 0 and err.R.shape == err.t.shape == (6,)
            # more than 10 poses: the original evaluate_any_poses; CPU-style operands (float64): the original methods
            big, big_gt = some(11)
            assert tr.evaluate_any_poses(None, big, big_gt) == "original evaluate_any_poses"
            assert tr.prealign_w2c_small_camera_systems(None, big, big_gt)[0].shape == (11, 3, 4) and len(lib.calls) == 4
            assert tr.evaluate_any_poses(None, pose.double(), gt.double()) == "original evaluate_any_poses"
            assert tr.prealign_w2c_small_camera_systems(None, pose.double(), gt.double()) == "original prealign_w2c_small_camera_systems"
            assert tr.evaluate_camera_alignment(None, pose.double(), gt.double()) == "original evaluate_camera_alignment"
            assert len(lib.calls) == 4
            with PE.unfused():                                                              # the restatement, not the original
                assert list(tr.evaluate_any_poses(None, pose, gt)) == list(PE.STATS) and len(lib.calls) == 4
            # n_first_fixed_poses > 1: no search, the poses themselves, the identity without a type
            fixed = _Sub(fixed=2)
            st = fixed.evaluate_any_poses(None, pose, gt)
            assert len(lib.calls) == 5 and lib.calls[-1]["flags"] == 0
            aligned, sim3 = fixed.prealign_w2c_small_camera_systems(None, pose, gt)
            assert aligned is pose and sim3.s == 1. and "type" not in sim3 and torch.equal(sim3.R, torch.eye(3)[None])
            assert len(lib.calls) == 5                                                      # nothing to compute: no launch
            # the backtrack under the trainer module's name; another kind of similarity goes to the original function
            assert torch.equal(trainer_mod.backtrack_from_aligning_the_trajectory(gt, PE.sim3_of(torch.ones(13))), gt + 1)
            assert trainer_mod.backtrack_from_aligning_the_trajectory(gt, edict(PE.sim3_of(torch.ones(13)), type='align_to_first')) == "original backtrack"
    finally:
        PE.uninstall()
    assert dict(vars(_Trainer)) == before and align_mod.backtrack_from_aligning_the_trajectory is original_backtrack
    assert trainer_mod.backtrack_from_aligning_the_trajectory is original_backtrack and PE._installer.originals == {} and PE._installer.patched == []
    PE.install(_Sub)                                           # a class without methods of its own goes back to having none
    PE.uninstall()
    assert not any(m in vars(_Sub) for m in PE.METHODS) and _Sub().evaluate_any_poses(None, 1, 2) == "original evaluate_any_poses"
