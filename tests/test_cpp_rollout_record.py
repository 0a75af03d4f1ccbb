"""The resident pipeline and the rollout recorder through the header-only C++ facade (tests/cpp/rollout_record_example.cpp): a recorded
5-period rollout of a Panda stack at B = 16 gives the same log, summaries, final state and torques, bit for bit, as the Python facade
given the same inputs."""
import numpy as np
import pytest

import workloads as W
from test_rollout_record_cpu import _robot_file, build_example


@pytest.mark.gpu
def test_cpp_recorded_rollout_matches_python(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    import subprocess
    B, K, n = 16, 5, 7
    d = W.make_inputs(2, B)
    q, dq = d["q"], np.zeros((B, n))
    g_mf, g_jt = d["goals"][0][:, :24].copy(), d["goals"][1].copy()
    g_mf[:, 12:] = 0.0    # a fixed goal pose near the current one, a posture goal, no feed-forward terms
    g_jt[:, n:] = 0.0
    blob = np.concatenate([q.T, dq.T, g_mf.T, g_jt.T], axis=0)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    np.ascontiguousarray(blob).tofile(inp)
    out = subprocess.run([exe, _robot_file(tmp_path), "run", str(B), str(K), str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RECORD_RUN_OK" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(outp)
    rows = 3 * n + 18
    assert list(raw[:4]) == [K, rows, 1, 1]
    at = 4
    parts = []
    for shape in ((K, rows, B), (K, B), (8, B), (n, B), (n, B), (n, B)):
        size = int(np.prod(shape))
        parts.append(raw[at:at + size].reshape(shape))
        at += size
    assert at == raw.size
    c_log, c_status, c_summary, c_q, c_dq, c_tau = parts

    robot = sp.SaiModel("panda_arm", B, device=0)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0.0, 0.0, 0.07)), sp.JointTask(robot)
    mf.disableInternalOtg()
    jt.disableInternalOtg()
    ctrl = sp.RobotController(robot, [mf, jt])
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.updateControllerTaskModels()
    mf.setGoalPosition(g_mf[:, 0:3])
    mf.setGoalOrientation(g_mf[:, 3:12].reshape(B, 3, 3))
    mf.setGoalLinearVelocity(g_mf[:, 12:15])
    mf.setGoalAngularVelocity(g_mf[:, 15:18])
    mf.setGoalLinearAcceleration(g_mf[:, 18:21])
    mf.setGoalAngularAcceleration(g_mf[:, 21:24])
    jt.setGoalPosition(g_jt[:, :n])
    jt.setGoalVelocity(g_jt[:, n:2 * n])
    jt.setGoalAcceleration(g_jt[:, 2 * n:])
    ctrl.recordRollouts(K, 1, ("q", "dq", "tau", "pose", "error"), task=mf, summaries=True)
    ctrl.rolloutAsync(K, 5e-4, 2, gravity=(0.0, 0.0, 0.0))
    ctrl.synchronize()
    log, summ = ctrl.rolloutLog(), ctrl.rolloutSummary()
    p_q, p_dq = ctrl.pullState()
    p_tau = ctrl.getTorques()
    p_log = np.concatenate([log["q"], log["dq"], log["tau"], log["position"], log["orientation"].reshape(K, B, 9), log["position_error"],
                            log["orientation_error"]], axis=2).transpose(0, 2, 1)

    def same(a, b):
        a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
        return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))

    assert list(log["period"]) == [1, 2, 3, 4, 5]
    assert same(c_log, p_log) and same(c_status, log["status"]) and same(c_summary, summ.T)
    assert same(c_q, p_q.T) and same(c_dq, p_dq.T) and same(c_tau, p_tau.T)
    assert same(c_q, c_log[-1, :n]) and same(c_tau, c_log[-1, 2 * n:3 * n])
    assert np.abs(c_log[-1, :n] - q.T).max() > 1e-5 and summ[:, 0].min() > 0.0     # the arms moved under nonzero torques
