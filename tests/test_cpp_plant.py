"""The plant model through the header-only C++ facade (tests/cpp/plant_example.cpp): its host checks without a device, and on the GPU a
Panda with the config-2 stack that carries a payload on the flange for 200 periods while the actuator of joint 2 saturates on every
second instance."""
import os
import subprocess

import numpy as np
import pytest

import workloads as W
from test_rollout_record_cpu import _robot_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")


def build_example(tmp_path):
    exe = str(tmp_path / "plant_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plant_example.cpp"),
                           "-L" + PKG, "-lsaip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_plant_example_host_checks(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    out = subprocess.run([exe, _robot_file(tmp_path), "cfgonly"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "PLANT_CFG_OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_plant_payload_run(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    B, K, n = 70, 200, 7
    ld = (B + 31) // 32 * 32
    q = W.make_inputs(2, B)["q"]
    qf, of = tmp_path / "q.bin", tmp_path / "out.bin"
    np.ascontiguousarray(q.T).tofile(qf)
    out = subprocess.run([exe, _robot_file(tmp_path), "run", str(B), str(K), str(qf), str(of)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "PLANT_RUN_OK" in out.stdout, out.stdout + out.stderr
    rows = {int(l.split()[1]): np.array(l.split()[2:], float) for l in out.stdout.splitlines() if l.startswith("PLANT_SUMMARY")}
    assert sorted(rows) == [0, 1, 2, 3] and all(r.shape == (B,) for r in rows.values())
    limited = np.arange(B) % 2 == 0
    assert (rows[1][limited] > 0).all() and not rows[1][~limited].any()            # the clipped torque: on the limited instances only
    assert (rows[2][limited] > 0).all() and not rows[2][~limited].any()            # ... and the substeps it happened in
    assert not rows[0].any()                                                        # no friction in this plant
    assert (rows[3] != 0).all()                                                     # the payload did work on every arm
    raw = np.fromfile(of).reshape(4 + n, ld)
    assert np.array_equal(raw[:4, :B], np.array([rows[r] for r in range(4)]))
    assert not raw[:, B:].any()                                                     # the padding columns were never written
    assert np.isfinite(raw).all() and raw[4:, :B].any()
