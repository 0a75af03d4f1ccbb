"""CPU pins for chains of 1 to 6 dof (tests/chains.py), runnable without a GPU:
  * the C oracle against the NumPy restatement on every stack tests/test_gpu_small_chains.py runs: equal status words, torques within
    1e-9 on every instance neither refuses -- the reference side is pinned at these sizes before the GPU is compared with it;
  * a motion-force task with more controlled directions than the robot has dof (k > n) is refused by the engine's controller and
    per-task interface, the Python and C++ facades, the C oracle and the restatement (undefined in the reference);
  * a 32-dof chain is accepted and a 33-dof chain refused by the engine and the oracle."""
import os
import subprocess

import numpy as np
import pytest

import chains as CH
import restatement as RS
import workloads as W
from oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
CASES = [(kind, n, s) for kind, ns in (("random", range(1, 6)), ("planar", range(2, 5)), ("puma", [6]))
         for n in ns for s in sorted(CH.cycle_stacks(n, kind))]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


@pytest.mark.parametrize("kind,n,stack", CASES, ids=[f"{k}{n}-{s}" for k, n, s in CASES])
def test_oracle_matches_restatement(kind, n, stack):
    model = W.RobotModel(CH.small_chain(n, kind))
    tasks, opts = CH.cycle_stacks(n, kind)[stack]
    rng = np.random.default_rng(7 * n + len(stack))
    B = 36
    q = CH.postures(rng, model, kind, B)
    dq = rng.uniform(-0.5, 0.5, (B, n))
    goals = CH.goals(rng, model, tasks, q)
    tau, st = Oracle(model, tasks, **opts).step(q, dq, goals)
    tr, sr = RS.controller_step(model, tasks, q, dq, goals, **opts)
    assert np.array_equal(st, sr), (st, sr)
    ok = st != 1
    assert ok.all()   # no stack here has an instance both refuse
    err = W.torque_error(tau[ok], tr[ok])
    print(f"{kind} n={n} {stack}: statuses {sorted(set(st.tolist()))}, oracle vs restatement {err:.2e}")
    assert err <= 1e-9


def test_small_chain_stacks_reach_the_blending_region():
    """the GPU comparison is only as strong as its postures: both regular and blended (status 8) instances occur at every n >= 2"""
    for kind, ns in (("random", range(2, 6)), ("planar", range(2, 5)), ("puma", [6])):
        for n in ns:
            model = W.RobotModel(CH.small_chain(n, kind))
            seen = set()
            for stack, (tasks, opts) in CH.cycle_stacks(n, kind).items():
                rng = np.random.default_rng(n)
                q = CH.postures(rng, model, kind, 60)
                _, st = Oracle(model, tasks, **opts).step(q, np.zeros_like(q), CH.goals(rng, model, tasks, q))
                seen |= set(st.tolist())
            assert {0, 8} <= seen, (kind, n, seen)


def _too_many_directions(n):
    """motion-force tasks with k > n for a chain of n dof (n <= 5): the full task, and a partial one with n + 1 directions"""
    rot = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]
    k = n + 1
    dt, dr = CH.XYZ[:min(k, 3)], rot[:k - min(k, 3)] or None
    return [W.motion_force_task("full", f"link{n}", (0.0, 0.0, 0.1)),
            W.motion_force_task("partial", f"link{n}", (0.0, 0.0, 0.1), dirs_trans=dt, dirs_rot=dr)]


@pytest.mark.parametrize("kind,n", [("random", 1), ("random", 2), ("random", 3), ("random", 4), ("random", 5), ("planar", 4)])
def test_task_with_more_directions_than_dof_is_refused(sp, kind, n):
    from sai_primitives_amd.controller import controller_from_specs, tasks_from_specs
    desc = CH.small_chain(n, kind)
    model = W.RobotModel(desc)
    q = np.zeros((2, n))
    for mf in _too_many_directions(n):
        tasks = [mf, W.joint_task("posture")]
        goals = CH.goals(np.random.default_rng(0), model, tasks, q)
        with pytest.raises(ValueError, match="more directions than the robot has dof"):
            Oracle(model, tasks)
        with pytest.raises(ValueError, match="use a partial task"):
            RS.controller_step(model, tasks, q, q, goals)
        with pytest.raises(sp.SaipUnsupported, match=rf"\[{mf['name']}\] controls \d directions but the robot has only {n} dof.*use a partial task"):
            controller_from_specs(desc, tasks, 4, device=-1)
        robot = sp.SaiModel(desc, 4, device=-1)
        alone = tasks_from_specs(robot, [mf])[0]
        with pytest.raises(sp.SaipUnsupported, match="use a partial task"):
            alone.updateTaskModel(np.eye(n))   # the per-task interface (TemplateTask::updateTaskModel) is refused the same way
    if n >= 3:   # k = 3 <= n: accepted everywhere
        tasks = [W.motion_force_task("position", f"link{n}", (0.0, 0.0, 0.1), dirs_trans=CH.XYZ, dirs_rot=None), W.joint_task("posture")]
        Oracle(model, tasks)
        controller_from_specs(desc, tasks, 4, device=-1)


def test_full_task_on_six_dof_is_accepted(sp):
    from sai_primitives_amd.controller import controller_from_specs
    desc = CH.puma_arm()
    tasks = [W.motion_force_task("hand", "link6", (0.1, 0.0, 0.0)), W.joint_task("posture")]
    Oracle(W.RobotModel(desc), tasks)
    _, ctrl, _ = controller_from_specs(desc, tasks, 4, device=-1)
    assert ctrl.getTaskNames() == ["hand", "posture"]


def _robot_file(path, desc):
    jt = {"fixed": 0, "revolute": 1, "prismatic": 2}
    with open(path, "w") as f:
        f.write(f"{len(desc['links'])}\n")
        for l in desc["links"]:
            vals = l["origin_xyz"] + l["origin_rpy"] + l["axis"] + [l["mass"]] + l["com"] + l["inertia"] + \
                [l["q_lower"], l["q_upper"], l["velocity_limit"], l["effort_limit"]]
            f.write(f"{l['name']} {jt[l['joint_type']]} " + " ".join(repr(float(v)) for v in vals) + "\n")


def build_facade(tmp_path, desc):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = str(tmp_path / "facade_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "facade_example.cpp"),
                           "-L" + PKG, "-lsaip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    robot = str(tmp_path / "robot.txt")
    _robot_file(robot, desc)
    return exe, robot


@pytest.mark.parametrize("n", [2, 4])
def test_cpp_facade_refuses_more_directions_than_dof(tmp_path, n):
    exe, robot = build_facade(tmp_path, CH.planar_arm(n))
    out = subprocess.run([exe, robot, "kgtn", "-1", f"link{n}"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "FACADE_KGTN_OK" in out.stdout, out.stdout + out.stderr


def test_32_dof_accepted_33_refused(sp):
    rng = np.random.default_rng(32)
    d32 = CH.random_chain(rng, 32, "chain32", fixed_after=(5, 20))
    d33 = CH.random_chain(rng, 33, "chain33")
    assert sp.SaiModel(d32, 4, device=-1).dof() == 32
    assert Oracle(W.RobotModel(d32), [W.joint_task("posture")]).n == 32
    with pytest.raises(sp.SaipUnsupported, match="more than 32 degrees of freedom"):
        sp.SaiModel(d33, 4, device=-1)
    with pytest.raises(ValueError, match="orc_create failed"):
        Oracle(W.RobotModel(d33), [W.joint_task("posture")])
