#!/usr/bin/env python3
"""Kinematic-tree cost on the device: a torso yaw carrying two Pandas (15 dof, tests/trees.py dual_panda_torso) with [MotionForceTask on each
flange, JointTask], B = 4096, against the same 15 links written as a serial chain and forced onto the general kernel (setKernel(1)): what
generality costs over a chain.  Cycles timed with saip_batch_time_steps; the integrate and model-query kernels of the tree run alongside,
so a `rocprofv3 --kernel-trace --stats` run of this script shows every tree kernel.  B=<n> in the environment changes the batch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import copy  # noqa: E402

import numpy as np  # noqa: E402
import trees as TR  # noqa: E402
import workloads as W  # noqa: E402
from sai_primitives_amd.controller import controller_from_specs  # noqa: E402

B = int(os.environ.get("B", "4096"))
tree = TR.dual_panda_torso()
chain = copy.deepcopy(tree)
for l in chain["links"]:
    l.pop("parent", None)
chain["name"] = "dual_panda_as_chain"
rng = np.random.default_rng(0)
for name, desc, kernel in (("tree", tree, 0), ("chain on the general kernel", chain, 1)):
    m = W.RobotModel(desc)
    tasks = TR.dual_stack(m)
    robot, ctrl, _ = controller_from_specs(desc, tasks, B, device=0)
    ctrl.setKernel(kernel)
    q = rng.uniform(-0.8, 0.8, (B, m.dof))
    robot.setQ(q)
    robot.setDq(np.zeros((B, m.dof)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    ctrl.updateControllerTaskModels()
    ctrl.computeControlTorques()
    steps = 200
    ms = ctrl.timeSteps(steps, 20) / steps  # (total elapsed ms of the timed region)
    print(f"{name}: {ctrl.kernelName()} B={B} {ms * 1e3:.1f} us per cycle = {B / ms / 1e3:.2f} M cycles/s")
    if kernel == 0:
        for _ in range(20):
            ctrl.integrate(5e-4, 1)
        ctrl.synchronize()
        for _ in range(10):
            robot.M()
            robot.JWorldFrame("left_link7")
