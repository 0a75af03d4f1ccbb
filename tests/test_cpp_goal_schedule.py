"""Goal schedules through the header-only C++ facade (tests/cpp/goal_schedule_example.cpp): the circle of the reference's example 06 as
keyframes resident on the device, one per period, followed by one rolloutAsync(K) of a Panda stack at B = 16 -- the example itself checks
state, torques and goal against its host-driven loop (setGoalPosition / LinearVelocity / LinearAcceleration and rolloutAsync(1) per
period), bit for bit."""
import subprocess

import numpy as np
import pytest

import workloads as W
from test_goal_schedule_cpu import build_example
from test_rollout_record_cpu import _robot_file


@pytest.mark.gpu
def test_cpp_circle_schedule_matches_the_host_driven_loop(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    B, K = 16, 12
    q = W.make_inputs(2, B)["q"]
    qf = tmp_path / "q.bin"
    np.ascontiguousarray(q.T).tofile(qf)
    out = subprocess.run([exe, _robot_file(tmp_path), "run", str(B), str(K), str(qf)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SCHEDULE_RUN_OK" in out.stdout, out.stdout + out.stderr
