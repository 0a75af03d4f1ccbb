"""The actuation chain through the header-only C++ facade (tests/cpp/plant_chain_example.cpp): its host checks without a device, and on the
GPU a Panda with the config-2 stack whose chain of delay 2 actuates, bit for bit, what a twin without a chain actuated two periods earlier."""
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from test_rollout_record_cpu import _robot_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")


def build_example(tmp_path):
    exe = str(tmp_path / "plant_chain_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plant_chain_example.cpp"),
                           "-L" + PKG, "-lsaip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_plant_chain_example_host_checks(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    out = subprocess.run([exe, _robot_file(tmp_path), "cfgonly"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "PLANT_CHAIN_CFG_OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_plant_chain_delays_by_two_periods(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    B = 70
    qf = tmp_path / "q.bin"
    np.ascontiguousarray(W.make_inputs(2, B)["q"].T).tofile(qf)
    out = subprocess.run([exe, _robot_file(tmp_path), "run", str(B), str(qf)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "PLANT_CHAIN_RUN_OK" in out.stdout, out.stdout + out.stderr
