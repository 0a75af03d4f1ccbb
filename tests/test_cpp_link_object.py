"""The pushed object through the header-only C++ facade (tests/cpp/link_object_example.cpp): its host checks without a device, and on the GPU
a rollout in which the Panda's end-effector sphere pushes a one-sphere body, at B = 70; the example checks itself."""
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from test_rollout_record_cpu import _robot_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")


def build_example(tmp_path):
    exe = str(tmp_path / "link_object_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "link_object_example.cpp"),
                           "-L" + PKG, "-lsaip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_link_object_example_host_checks(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    out = subprocess.run([exe, _robot_file(tmp_path), "cfgonly"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "LINK_OBJECT_CFG_OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_link_object_rollout(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    B, K = 70, 6
    q = W.make_inputs(2, B)["q"]
    qf = tmp_path / "q.bin"
    np.ascontiguousarray(q.T).tofile(qf)
    out = subprocess.run([exe, _robot_file(tmp_path), "run", str(B), str(K), str(qf)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "LINK_OBJECT_RUN_OK" in out.stdout, out.stdout + out.stderr
