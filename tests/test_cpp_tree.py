"""A kinematic tree through the header-only C++ facade (tests/cpp/tree_example.cpp): SaiModel(links, parent, ...), jointParent, and one
control cycle of a dual-arm stack equal to the same cycle through the Python facade."""
import os
import subprocess

import numpy as np
import pytest

import trees as TR
import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")


def _build(tmp_path, desc):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = str(tmp_path / "tree_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "tree_example.cpp"),
                           "-L" + PKG, "-lsaip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    robot = tmp_path / "robot.txt"
    m = W.RobotModel(desc)
    par = TR.parent_index(m)
    jt = {"fixed": 0, "revolute": 1, "prismatic": 2}
    with open(robot, "w") as f:
        f.write(f"{len(m.links)}\n")
        for l, p in zip(m.links, par):
            vals = l["origin_xyz"] + l["origin_rpy"] + l["axis"] + [l["mass"]] + l["com"] + l["inertia"] + \
                [l["q_lower"], l["q_upper"], l["velocity_limit"], l["effort_limit"]]
            f.write(f"{l['name']} {jt[l['joint_type']]} {p} " + " ".join(repr(float(v)) for v in vals) + "\n")
    return exe, str(robot)


def test_cpp_tree_topology(tmp_path):
    desc = TR.dual_panda_torso()
    exe, robot = _build(tmp_path, desc)
    out = subprocess.run([exe, robot, "topology"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "TREE_TOPOLOGY_OK" in out.stdout, out.stdout + out.stderr
    line = [x for x in out.stdout.splitlines() if x.startswith("TREE_PARENTS")][0]
    assert [int(v) for v in line.split()[1:]] == TR.joint_parents(W.RobotModel(desc))


@pytest.mark.gpu
def test_cpp_tree_cycle_matches_python(tmp_path):
    from sai_primitives_amd.controller import controller_from_specs
    desc = TR.dual_panda_torso()
    m = W.RobotModel(desc)
    exe, robot = _build(tmp_path, desc)
    B = 128
    rng = np.random.default_rng(9)
    q = rng.uniform(-0.8, 0.8, (B, m.dof))
    dq = rng.uniform(-0.5, 0.5, (B, m.dof))
    tasks = TR.dual_stack(m)
    goals = TR.tree_goals(rng, m, tasks, q)
    goals = [goals[0][:, :24], goals[1][:, :24], goals[2]]
    blob = np.concatenate([q.T, dq.T] + [g.T for g in goals], axis=0)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    np.ascontiguousarray(blob).tofile(inp)
    out = subprocess.run([exe, robot, "run", str(B), str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "TREE_RUN_OK" in out.stdout, out.stdout + out.stderr
    tau = np.fromfile(outp).reshape(m.dof, B).T
    r, ctrl, _ = controller_from_specs(desc, tasks, B, device=0)
    r.setQ(q)
    r.setDq(dq)
    r.updateModel()
    ctrl.updateControllerTaskModels()
    ctrl.setGoals(goals)
    ref = ctrl.computeControlTorques()
    assert ctrl.kernelName().startswith("saip_cycle_wg_tree")
    ok = (ctrl.status & 1) == 0
    assert ok.sum() > B // 2
    assert np.array_equal(tau[ok], ref[ok])
