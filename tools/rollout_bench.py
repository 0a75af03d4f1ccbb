#!/usr/bin/env python3
"""Closed-loop period on the device (internal OTGs -> control cycle -> 2 dynamics substeps) and the integrate kernel alone, cfg2 tasks.
   SAIP_LIB=<path> selects the build (same-session A/B).
   --record-stride N / --record-channels q,dq,tau,pose,error / --record-summaries attach a rollout recorder (any of them does: stride 1,
   channels q,dq,tau, no summaries unless given; --record-channels none = summaries only) and the line gains what was recorded.
   --no-otg runs the stack without internal OTGs (the cycle launch integrates in-kernel); --repeats R times the closed-loop period R times."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import workloads as W  # noqa: E402
from sai_primitives_amd.controller import controller_from_specs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--record-stride", type=int, default=None)
ap.add_argument("--record-channels", default=None)
ap.add_argument("--record-summaries", action="store_true")
ap.add_argument("--no-otg", action="store_true")
ap.add_argument("--repeats", type=int, default=1)
args = ap.parse_args()
record = args.record_stride is not None or args.record_channels is not None or args.record_summaries

for B in [int(x) for x in os.environ.get("BATCHES", "4096,65536").split(",")]:
    d = W.make_inputs(2, B)
    robot, ctrl, tasks = controller_from_specs(d["model"].name, d["tasks"], B, device=0, disable_otg=args.no_otg)
    robot.setQ(d["q"])
    robot.setDq(np.zeros((B, 7)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    mf, jt = tasks
    mf.setGoalPosition(mf.getGoalPosition() + np.array([0.05, -0.04, 0.03]))
    ctrl.updateControllerTaskModels()
    K = 400
    what = ""
    if record:
        stride = 1 if args.record_stride is None else args.record_stride
        channels = ("q", "dq", "tau") if args.record_channels is None else tuple(c for c in args.record_channels.split(",") if c not in ("", "none"))
        ctrl.recordRollouts(max(1, K // stride), stride, channels, task=mf, summaries=args.record_summaries)
        what = f"; recorder: stride {stride}, channels {','.join(channels) or 'none'}, summaries {'on' if args.record_summaries else 'off'}"
    ctrl.rolloutAsync(50, 5e-4, 2, gravity=(0, 0, 0))
    ctrl.synchronize()
    for _ in range(args.repeats):
        if record:
            ctrl.resetRolloutRecorder()
        t0 = time.perf_counter()
        ctrl.rolloutAsync(K, 5e-4, 2, gravity=(0, 0, 0))
        ctrl.synchronize()
        dt = time.perf_counter() - t0
        t0 = time.perf_counter()
        for _ in range(200):
            ctrl.integrate(5e-4, 2, gravity=(0, 0, 0))
        ctrl.synchronize()
        di = time.perf_counter() - t0
        n = f", {ctrl.rolloutLog()['status'].shape[0]} samples" if record else ""
        print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B}: closed-loop period {dt / K * 1e6:.1f} us = {B * K / dt / 1e6:.1f} M robot-periods/s; "
              f"integrate (2 substeps) {di / 200 * 1e6:.1f} us{what}{n}")
