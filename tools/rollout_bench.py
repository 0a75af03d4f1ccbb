#!/usr/bin/env python3
"""Closed-loop period on the device (internal OTGs -> control cycle -> 2 dynamics substeps) and the integrate kernel alone, cfg2 tasks.
   SAIP_LIB=<path> selects the build (same-session A/B).
   --record-stride N / --record-channels q,dq,tau,pose,error / --record-summaries attach a rollout recorder (any of them does: stride 1,
   channels q,dq,tau, no summaries unless given; --record-channels none = summaries only) and the line gains what was recorded.
   --no-otg runs the stack without internal OTGs (the cycle launch integrates in-kernel); --repeats R times the closed-loop period R times.
   --goal-schedule hold|linear times, in the same setting and run, the period without a schedule, the period cut into one rollout call per
   period (no fused integrate + next-OTG launch, nothing else changed) and the period with a per-instance schedule on the position and
   orientation rows of the motion-force task (8 keyframes, stride 50; linear interpolates the orientation on SO(3)).
   --snapshot prints the bytes of a state snapshot of the stack and, event-timed on the engine stream (mean of 50 back-to-back calls), a
   save, an identity restore, a random-permutation restore, a broadcast restore and plain hipMemcpyAsync device-to-device copies of
   segments of the same sizes (the yardstick of DESIGN.md 4.10).
   --sampler attaches a resident rollout sampler to a 16-keyframe position + orientation schedule of the motion-force task and prints the
   event-timed mean of 50 calls each of perturb, cost and update, and beside them the host round trip they replace: rolloutSummary(), the
   NumPy perturb and update of tests/sampler_ref.py, detach and attach of the new keyframes, by wall clock around a synchronise
   (DESIGN.md 4.11).  --sampler --scenarios M [--risk mean|max|cvar] [--alpha A] groups the batch into M scenario blocks of B / M candidates
   before the timing (M = 1, the default, makes no call at all: the ungrouped sampler of any build) and prints M, the risk and, with
   M > 1, one shareScenarioTables() call over all five attachments drawn per instance, event-timed the same way.
   --contact [--contact-planes P] [--contact-sensor] [--contact-stack 2|13] [--substeps S] times, interleaved in the same run, the
   closed-loop period without and with contact planes attached to the motion-force task (P planes: a table just under the control point
   and P - 1 far walls), and the integrate call alone both ways; --contact-stack 13 runs config 13's closed-loop force stack
   (DESIGN.md 4.12).  With --contact-points N [--contact-patches 1|2] the same run also times a contact patch of N points (1..8) in place of
   the single-point attachment, and the event-timed mean of 200 one-substep integrate calls plain, with the single point and with the
   patch: the differences are the contact launches alone.  Two patches run on the dual-arm tree, one patch per flange, the single point
   on the left one.
   --clearance [--clearance-spheres S] [--clearance-obstacles O] [--clearance-pairs P] times, interleaved in the same run, the closed-loop
   period without and with a clearance monitor of S link spheres, O batch-uniform obstacles (capsules, every fourth a half-space) and P self
   pairs, and prints the event-timed mean of 200 back-to-back evaluations alone.
   --link-contact [--lc-spheres S] [--lc-obstacles O] [--lc-per-instance] [--substeps N] times, interleaved in the same run, the closed-loop
   period without and with link contact of S link spheres against O obstacles (capsules, every fourth a floor; soft materials with
   friction), and prints the event-timed mean of 200 back-to-back EVALUATE launches alone and of 200 one-substep integrate calls both
   ways: their difference is the APPLY launch.
   --link-contact --link-object [--lo-spheres P] times, interleaved in the same run, the period with that link contact alone and with the
   pushed object of P corner spheres on top (the launch with the object replaces the link-contact launch), the one-substep integrate
   call and the EVALUATE launch alone both ways.
   --plant [--plant-wrenches W] [--substeps S] times, interleaved in the same run, the closed-loop period without and with a per-instance
   plant model (tight actuators, friction, stops at the model's limits and W payload-like wrenches, 0..4) and the event-timed mean of 200
   one-substep integrate calls both ways: the difference is the plant launch alone.
   --inertia [--inertia-payloads P] [--substeps S] times, interleaved in the same run, the closed-loop period without and with a per-instance
   inertia table (link masses within 20 %, centres of mass within 2 cm, P box payloads of up to 3 kg, 0..2, drawn on the device), the
   event-timed mean of 200 integrate calls both ways and of 50 draws of the whole table.
   --sensing [--sensing-wrench] [--substeps S] times, interleaved in the same run, the closed-loop period without and with a per-instance
   sensing model (encoder offsets, 14-bit position resolution, position and velocity noise; with --sensing-wrench also contact planes with
   the simulated sensor, attached throughout, and a biased, quantised, noisy wrench table on their task) and the event-timed mean of 200
   measurements of q, dq alone.
   --sensing-chain DEPTH [--substeps S] times, interleaved in the same run, the closed-loop period with that sensing model alone and with a
   per-instance sensing chain of DEPTH taps behind it (delays 0..DEPTH across the instances, finite-difference velocity and both filters
   on), and the event-timed mean of 200 measurements alone both ways.
   --plant --plant-chain DEPTH [--plant-wrenches W] [--substeps S] times, interleaved in the same run, the closed-loop period with that plant
   model alone and with a per-instance actuation chain of DEPTH taps in front of it (delays 0..DEPTH across the instances, rate limit and
   lag on), and the event-timed mean of 200 one-substep integrate calls both ways.
   --env-schedule {obstacles,planes,both} [--env-mode hold|linear] [--substeps S] times, interleaved in the same run, the closed-loop period
   with a clearance monitor (8 spheres, 4 obstacles) and / or one per-instance contact plane attached, without and with an environment
   schedule of three keyframes over the timed rollout on their tables, and the event-timed mean of 200 one-substep integrate calls both
   ways: with planes that is the static against the MOVING contact launch.
   --guards times, interleaved in the same run, the closed-loop period without and with resident guards on the motion-force task (a force
   guard into a HOLD phase, a timed guard into an OFFSET phase, so that the launch walks the kinematics and writes the goal) and the
   event-timed mean of 200 back-to-back evaluations alone."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import workloads as W  # noqa: E402
from sai_primitives_amd.controller import controller_from_specs  # noqa: E402


def stream_timer(ctrl):
    """timed_us(fn, reps, first=None): the mean, in microseconds, of `reps` back-to-back calls of fn between two HIP events recorded on the
    engine stream, after one call of `first` (fn itself by default) and a synchronise; and the HIP runtime the events came from"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipEventCreate.argtypes, hip.hipEventRecord.argtypes, hip.hipEventSynchronize.argtypes = [C.POINTER(vp)], [vp, vp], [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    stream = ctrl.devicePointers()["stream"]
    ev = [vp(), vp()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def timed_us(fn, reps=50, first=None):
        (first or fn)()
        ctrl.synchronize()
        assert hip.hipEventRecord(ev[0], stream) == 0
        for _ in range(reps):
            fn()
        assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        return ms.value / reps * 1e3

    return timed_us, hip


ap = argparse.ArgumentParser()
ap.add_argument("--record-stride", type=int, default=None)
ap.add_argument("--record-channels", default=None)
ap.add_argument("--record-summaries", action="store_true")
ap.add_argument("--no-otg", action="store_true")
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--goal-schedule", choices=("hold", "linear"), default=None)
ap.add_argument("--snapshot", action="store_true")
ap.add_argument("--sampler", action="store_true")
ap.add_argument("--scenarios", type=int, default=1, metavar="M")
ap.add_argument("--risk", choices=("mean", "max", "cvar"), default="mean")
ap.add_argument("--alpha", type=float, default=None)
ap.add_argument("--contact", action="store_true")
ap.add_argument("--contact-planes", type=int, default=1)
ap.add_argument("--contact-sensor", action="store_true")
ap.add_argument("--contact-stack", type=int, choices=(2, 13), default=2)
ap.add_argument("--contact-points", type=int, default=None)
ap.add_argument("--contact-patches", type=int, choices=(1, 2), default=1)
ap.add_argument("--substeps", type=int, default=2)
ap.add_argument("--clearance", action="store_true")
ap.add_argument("--clearance-spheres", type=int, default=8)
ap.add_argument("--clearance-obstacles", type=int, default=4)
ap.add_argument("--clearance-pairs", type=int, default=0)
ap.add_argument("--link-contact", action="store_true")
ap.add_argument("--lc-spheres", type=int, default=8)
ap.add_argument("--lc-obstacles", type=int, default=4)
ap.add_argument("--lc-per-instance", action="store_true")
ap.add_argument("--link-object", action="store_true", help="with --link-contact: the pushed object on top; the leg with link contact alone runs interleaved")
ap.add_argument("--lo-spheres", type=int, default=8)
ap.add_argument("--guards", action="store_true")
ap.add_argument("--env-schedule", choices=("obstacles", "planes", "both"), default=None)
ap.add_argument("--env-mode", choices=("hold", "linear"), default="linear")
ap.add_argument("--plant", action="store_true")
ap.add_argument("--plant-wrenches", type=int, choices=range(5), default=1)
ap.add_argument("--plant-chain", type=int, choices=range(9), default=None, metavar="DEPTH")
ap.add_argument("--sensing", action="store_true")
ap.add_argument("--sensing-wrench", action="store_true")
ap.add_argument("--sensing-chain", type=int, choices=range(9), default=None, metavar="DEPTH")
ap.add_argument("--inertia", action="store_true")
ap.add_argument("--inertia-payloads", type=int, choices=range(3), default=1)
args = ap.parse_args()
if args.plant_chain is not None and not args.plant:
    ap.error("--plant-chain needs --plant: the actuation chain stands in front of the plant model")
record = args.record_stride is not None or args.record_channels is not None or args.record_summaries

for B in [int(x) for x in os.environ.get("BATCHES", "4096,65536").split(",")]:
    dual = args.contact and args.contact_points is not None and args.contact_patches == 2
    if dual:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import trees as TR
        desc = TR.dual_panda_torso()
        model = W.RobotModel(desc)
        d = dict(model=model, tasks=TR.dual_stack(model))
        d["q"] = np.clip(np.random.default_rng(0).uniform(-0.8, 0.8, (B, model.dof)), model.q_lower + 0.1, model.q_upper - 0.1)
        robot, ctrl, tasks = controller_from_specs(desc, d["tasks"], B, device=0, disable_otg=args.no_otg)
    else:
        d = W.make_inputs(args.contact_stack if args.contact else 2, B)
        robot, ctrl, tasks = controller_from_specs(d["model"].name, d["tasks"], B, device=0, disable_otg=args.no_otg)
    robot.setQ(d["q"])
    robot.setDq(np.zeros((B, d["model"].dof)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    mf, jt = tasks[0], tasks[-1]
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
    if args.snapshot:
        import ctypes as C
        timed_us, hip = stream_timer(ctrl)
        vp = C.c_void_p
        hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(vp), C.c_size_t], [vp]
        hip.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
        stream = ctrl.devicePointers()["stream"]
        snap = ctrl.saveState()
        segs = snap.segments()
        ends = [s["offset"] for s in segs[1:]] + [snap.nbytes()]
        sizes = [e - s["offset"] for s, e in zip(segs, ends)]          # the segments' arrays, padding columns included
        bufs = [vp(), vp()]
        for p in bufs:
            assert hip.hipMalloc(C.byref(p), snap.nbytes()) == 0
        rng = np.random.default_rng(0)
        perm, bcast = rng.permutation(B).astype(np.int32), np.full(B, B // 2, np.int32)

        def copies():
            for s, n in zip(segs, sizes):
                assert hip.hipMemcpyAsync(bufs[0].value + s["offset"], bufs[1].value + s["offset"], n, 3, stream) == 0   # device to device

        for _ in range(args.repeats):
            t = dict(save=timed_us(lambda: ctrl.saveState(snap)), identity=timed_us(lambda: ctrl.restoreState(snap)),
                     permutation=timed_us(lambda: ctrl.restoreState(snap, perm)), broadcast=timed_us(lambda: ctrl.restoreState(snap, bcast)),
                     copies=timed_us(copies))
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'}: snapshot {snap.nbytes()} bytes in "
                  f"{len(segs)} segments; save {t['save']:.1f} us; identity restore {t['identity']:.1f} us; permutation restore {t['permutation']:.1f} us; "
                  f"broadcast restore {t['broadcast']:.1f} us; hipMemcpyAsync D2D per segment {t['copies']:.1f} us")
        for p in bufs:
            hip.hipFree(p)
        snap.close()
        continue
    if args.sampler:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import sampler_ref as SR
        timed_us, _ = stream_timer(ctrl)

        KF, sigma, T = 16, np.array([0.02, 0.02, 0.02, 0.05, 0.05, 0.05]), 0.05
        nominal = np.repeat(mf._get_goal()[0, :12][None], KF, axis=0)
        ctrl.recordRollouts(8, max(1, K // 8), ("pose",), task=mf, summaries=True)     # 8 samples over the K periods rolled below
        mf.setGoalSchedule((0, 12), np.repeat(nominal[:, None], B, axis=1), stride=25, mode="linear")
        mf.attachSampler(sigma, nominal=nominal, exempt=1)
        ctrl.seedSampler(1)
        ctrl.rolloutAsync(K, 5e-4, 2, gravity=(0, 0, 0))
        w8, target = np.array([1e-4, 1.0, 1.0, 0, 0, 0, 0, 10.0]), nominal[0, :3] + 0.03
        grouped = ""
        if args.scenarios > 1:
            M, n = args.scenarios, d["model"].dof
            ctrl.setSamplerScenarios(M, args.risk, args.alpha if args.risk == "cvar" else None)
            # one share call with all five attachments per instance: tables as the --plant, --inertia and --sensing runs draw them
            ctrl.attachPlant(np.zeros((n, B, 10)) + [1.0, 0, np.inf, 0, 0, 0, -np.inf, np.inf, 0, 0], wrenches=[(d["tasks"][0]["link"], (0, 0, 0), "world", np.zeros((B, 8)))],
                             per_instance=True)
            ctrl.attachActuationChain(np.zeros((n, B, 3)) + [0.0, np.inf, 0.0], per_instance=True, depth=2)
            ctrl.attachInertia(per_instance=True, payload_links=[d["tasks"][0]["link"]])
            ctrl.attachSensing(joints=np.zeros((n, B, 6)), per_instance=True)
            ctrl.attachSensingChain(np.zeros((n, B, 4)), per_instance=True, depth=2)
            ctrl.randomizePlant(1, 0, joints=(np.tile([0.8, 0, np.inf, 0, 0, 0, -np.inf, np.inf, 0, 0], (n, 1)), np.tile([1.0, 0, np.inf, 0.1, 0, 0, -np.inf, np.inf, 0, 0], (n, 1))))
            ctrl.randomizeInertia(2, 0, bodies=(np.tile([0.8, 0, 0, 0], (n, 1)), np.tile([1.2, 0, 0, 0], (n, 1))))
            ctrl.sensingRandomize(3, 0, joints=(np.tile([-1e-3, 0, 0, -1e-3, 0, 0], (n, 1)), np.tile([1e-3, 0, 0, 1e-3, 0, 0], (n, 1))))
            share_us, arrays = timed_us(ctrl.shareScenarioTables), ctrl.shareScenarioTables()
            for detach in (ctrl.detachSensingChain, ctrl.detachSensing, ctrl.detachInertia, ctrl.detachPlant):
                detach()
            grouped = f"; scenarios {M} x {B // M} candidates, risk {args.risk}; share of {arrays} arrays {share_us:.1f} us"

        def host_round(rnd):
            S = ctrl.rolloutSummary()
            cost = S @ w8
            keys = SR.perturb(nominal, sigma, 1, rnd, 0, B, 1, 3)
            w, res = SR.weights(cost, T)
            new = SR.update(nominal, keys, w, res["best"], 3)
            mf.clearGoalSchedule()
            mf.setGoalSchedule((0, 12), keys, stride=25, mode="linear")
            ctrl.synchronize()
            return new

        for r in range(args.repeats):
            t = dict(perturb=timed_us(ctrl.perturbGoalSchedules), cost=timed_us(lambda: ctrl.rolloutCost(w8, target, 0.1, 1.0)),
                     update=timed_us(lambda: ctrl.updateSampler(T)))
            mf.detachSampler()
            ctrl.synchronize()
            t0 = time.perf_counter()
            for i in range(3):
                host_round(i)
            host = (time.perf_counter() - t0) / 3 * 1e6
            mf.attachSampler(sigma, nominal=nominal, exempt=1)
            if args.scenarios > 1:                         # the detach above reset the setting
                ctrl.setSamplerScenarios(args.scenarios, args.risk, args.alpha if args.risk == "cvar" else None)
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'}: sampler, {KF} keyframes of position + "
                  f"orientation: perturb {t['perturb']:.1f} us; cost {t['cost']:.1f} us; update {t['update']:.1f} us; host round trip (summary, NumPy perturb + "
                  f"update, detach + attach) {host:.0f} us{grouped}")
        continue
    if args.env_schedule:
        sub, mode = args.substeps, args.env_mode
        with_o, with_p = args.env_schedule in ("obstacles", "both"), args.env_schedule in ("planes", "both")
        rng = np.random.default_rng(0)
        names = [f"link{i}" for i in range(1, 8)] + ["end-effector"]
        spheres = [(names[s % 8], rng.uniform(-0.05, 0.05, 3), 0.05) for s in range(8)]
        obst = np.zeros((4, 8))
        obst[:, 1:4] = rng.uniform(-0.8, 0.8, (4, 3))
        obst[:, 4:7] = obst[:, 1:4] + rng.uniform(-0.3, 0.3, (4, 3))
        obst[:, 7] = 0.03
        obst[3] = [1.0, 0.0, 0.0, 1.0, -0.2, 0.0, 0.0, 0.0]                   # a floor
        ko = np.repeat(obst[None], 3, axis=0)                                 # the capsules drift 5 cm per keyframe, the floor rises 1 cm
        ko[1:, :3, 1:7] += np.array([0.05, 0.1])[:, None, None]
        ko[1:, 3, 4] += np.array([0.01, 0.02])
        p0 = robot.position(d["tasks"][0]["link"], tuple(d["tasks"][0]["pos_in_link"]))
        planes = np.zeros((1, B, 8))
        planes[0] = [0.0, 0.0, 1.0, 0.0, 2.0e4, 400.0, 0.3, 1e-3]
        planes[0, :, 3] = p0[:, 2] + 1e-3                                     # a table 1 mm above every control point ...
        kp = np.zeros((3, 1, B, 12))
        kp[:, 0, :, :8] = planes[0]
        kp[:, 0, :, 3] += np.array([0.0, 1e-3, 0.0])[:, None]                 # ... that rises 1 mm and comes back, on a belt along +x
        kp[:, 0, :, 8] = 0.05
        timed_us, _ = stream_timer(ctrl)

        def period_us():
            ctrl.rewindEnvironment(0)
            t0 = time.perf_counter()
            ctrl.rolloutAsync(K, 5e-4, sub, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / K * 1e6

        def substep_us():
            return timed_us(lambda: ctrl.integrate(5e-4, 1, gravity=(0, 0, 0)), 200)

        for _ in range(args.repeats):
            if with_o:
                ctrl.attachClearance(spheres, obst, margin=0.05)
            if with_p:
                mf.attachContactPlanes(planes, sensor=False, per_instance=True)
            period_us()
            static, static_s = period_us(), substep_us()
            if with_o:
                ctrl.setObstacleSchedule(ko, stride=K // 2, mode=mode)        # two keyframe intervals span the K periods of a timed rollout
            if with_p:
                mf.setContactSchedule(kp, stride=K // 2, mode=mode)
            period_us()
            sched, moving_s = period_us(), substep_us()
            ctrl.clearEnvironmentSchedules()
            again = period_us()
            if with_o:
                ctrl.detachClearance()
            if with_p:
                mf.detachContactPlanes()
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'} substeps {sub}, env schedule "
                  f"{args.env_schedule} ({mode}): closed-loop period with the attachment(s) and no schedule {static:.1f} us; scheduled {sched:.1f} us; "
                  f"unscheduled again {again:.1f} us; one substep on the stream, static / with the schedule attached {static_s:.2f} / {moving_s:.2f} us")
        continue
    if args.contact:
        P, sub = args.contact_planes, args.substeps
        p0 = robot.position(d["tasks"][0]["link"], tuple(d["tasks"][0]["pos_in_link"]))
        planes = np.zeros((P, B, 8))
        planes[:] = [1.0, 0.0, 0.0, -10.0, 2.0e4, 400.0, 0.3, 1e-3]          # far walls: evaluated, never active
        planes[0] = [0.0, 0.0, 1.0, 0.0, 2.0e4, 400.0, 0.3, 1e-3]
        planes[0, :, 3] = p0[:, 2] + 1e-3                                     # a table 1 mm above every control point

        def period_us():
            t0 = time.perf_counter()
            ctrl.rolloutAsync(K, 5e-4, sub, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / K * 1e6

        def integrate_us():
            t0 = time.perf_counter()
            for _ in range(200):
                ctrl.integrate(5e-4, sub, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / 200 * 1e6

        if args.contact_points is not None:
            timed_us, _ = stream_timer(ctrl)

            def substep_us():
                return timed_us(lambda: ctrl.integrate(5e-4, 1, gravity=(0, 0, 0)), 200)

            N = args.contact_points
            ang = 2.0 * np.pi * np.arange(N) / N
            pts = np.column_stack([0.05 * np.cos(ang), 0.05 * np.sin(ang), np.zeros(N)]) if N > 1 else np.zeros((1, 3))
            carriers = [(t, s["link"], tuple(s["pos_in_link"])) for t, s in zip(tasks[:args.contact_patches], d["tasks"])]
            tables = []
            for t, link, pos in carriers:       # per patch: a table 1 mm above its lowest point, and the far walls
                pz = np.stack([robot.position(link, tuple(np.asarray(pos) + r))[:, 2] for r in pts]).min(axis=0)
                tb = planes.copy()
                tb[0, :, 3] = pz + 1e-3
                tables.append(tb)
            for _ in range(args.repeats):
                plain, plain_i, plain_s = period_us(), integrate_us(), substep_us()
                mf.attachContactPlanes(planes, sensor=args.contact_sensor, per_instance=True)
                period_us()
                one, one_i, one_s = period_us(), integrate_us(), substep_us()
                mf.detachContactPlanes()
                for (t, _, _), tb in zip(carriers, tables):
                    t.attachContactPatch(pts, tb, sensor=args.contact_sensor, per_instance=True)
                period_us()
                pat, pat_i, pat_s = period_us(), integrate_us(), substep_us()
                touching = int((mf.contactPatchReadout()["n_touch"] > 0).sum())
                ctrl._call("saip_batch_contact_patch_detach", -1)
                print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} {'dual-arm tree' if dual else f'cfg{args.contact_stack}'} otg "
                      f"{'off' if args.no_otg else 'on'} substeps {sub}, {P} plane(s), sensor {'on' if args.contact_sensor else 'off'}: period / integrate / "
                      f"one substep on the stream: unattached {plain:.1f} / {plain_i:.1f} / {plain_s:.2f} us; single point {one:.1f} / {one_i:.1f} / "
                      f"{one_s:.2f} us; {args.contact_patches} patch(es) of {N} points {pat:.1f} / {pat_i:.1f} / {pat_s:.2f} us; launch alone: single point "
                      f"{one_s - plain_s:.2f} us, patch {pat_s - plain_s:.2f} us ({touching} of {B} instances touching at the end)")
            continue
        for _ in range(args.repeats):
            plain, plain_i = period_us(), integrate_us()
            mf.attachContactPlanes(planes, sensor=args.contact_sensor, per_instance=True)
            period_us()
            with_c, with_i = period_us(), integrate_us()
            touching = int((mf.contactReadout()["active"] > 0).sum())
            mf.detachContactPlanes()
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} cfg{args.contact_stack} otg {'off' if args.no_otg else 'on'} substeps {sub}: "
                  f"closed-loop period {plain:.1f} us, integrate {plain_i:.1f} us; with {P} contact plane(s), sensor {'on' if args.contact_sensor else 'off'}: "
                  f"period {with_c:.1f} us, integrate {with_i:.1f} us ({touching} of {B} instances touching at the end)")
        continue
    if args.clearance:
        S, O, P = args.clearance_spheres, args.clearance_obstacles, args.clearance_pairs
        rng = np.random.default_rng(0)
        names = [f"link{i}" for i in range(1, 8)] + ["end-effector"]
        spheres = [(names[s % 8], rng.uniform(-0.05, 0.05, 3), 0.05) for s in range(S)]
        obst = np.zeros((O, 8))
        obst[:, 1:4] = rng.uniform(-0.8, 0.8, (O, 3))
        obst[:, 4:7] = obst[:, 1:4] + rng.uniform(-0.3, 0.3, (O, 3))
        obst[:, 7] = 0.03
        obst[3::4] = [1.0, 0.0, 0.0, 1.0, -0.2, 0.0, 0.0, 0.0]               # every fourth: a floor
        pairs = [(p % S, (p % S + 1 + p // S) % S) for p in range(P)]
        timed_us, _ = stream_timer(ctrl)

        def period_us():
            t0 = time.perf_counter()
            ctrl.rolloutAsync(K, 5e-4, args.substeps, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / K * 1e6

        def evaluate_us():
            return timed_us(lambda: ctrl._call("saip_batch_clearance_evaluate"), 200, first=ctrl.evaluateClearance)

        for _ in range(args.repeats):
            plain = period_us()
            ctrl.attachClearance(spheres, obst if O else None, pairs or None, margin=0.05)
            period_us()
            with_c, alone = period_us(), evaluate_us()
            under = int((ctrl.clearanceSummary()["min_distance"] < 0.05).sum())
            ctrl.detachClearance()
            again = period_us()
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'} substeps {args.substeps}: "
                  f"closed-loop period {plain:.1f} us; with a clearance monitor of {S} spheres, {O} obstacles, {P} pairs {with_c:.1f} us; without it again "
                  f"{again:.1f} us; one evaluation alone {alone:.2f} us ({under} of {B} instances under the margin)")
        continue
    if args.guards:
        # the sensed force is 0 without a contact: "norm >= 0" fires in the first period, HOLD for 100 periods, then OFFSET for the rest
        guards = [{"from": 0, "to": 1, "signal": "force", "axis": "norm", "cmp": ">=", "threshold": 0.0},
                  {"from": 1, "to": 2, "signal": "periods", "threshold": 100}]
        phases = [dict(mode="free"), dict(mode="hold"), dict(mode="offset", offset=(0.0, 0.0, 0.01))]
        timed_us, _ = stream_timer(ctrl)

        def period_us():
            t0 = time.perf_counter()
            ctrl.rolloutAsync(K, 5e-4, args.substeps, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / K * 1e6

        for _ in range(args.repeats):
            snap = ctrl.saveState()
            plain = period_us()
            ctrl.restoreState(snap)
            snap.close()
            mf.attachGuards(guards, phases)
            snap = ctrl.saveState()
            period_us()
            ctrl.restoreState(snap)
            ctrl.resetGuards()
            with_g = period_us()
            alone = timed_us(lambda: ctrl._call("saip_batch_guard_evaluate"), 200, first=ctrl.evaluateGuards)
            offset = int((ctrl.guardState()["phase"] == 2).sum())
            ctrl.restoreState(snap)
            snap.close()
            mf.detachGuards()
            again = period_us()
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'} substeps {args.substeps}: "
                  f"closed-loop period {plain:.1f} us; with guards (force -> HOLD -> OFFSET) {with_g:.1f} us; without them again {again:.1f} us; "
                  f"one evaluation alone {alone:.2f} us ({offset} of {B} instances ended in the OFFSET phase)")
        continue
    if args.link_contact:
        S, O = args.lc_spheres, args.lc_obstacles
        rng = np.random.default_rng(0)
        names = [f"link{i}" for i in range(1, 8)] + ["end-effector"]
        spheres = [(names[s % 8], rng.uniform(-0.05, 0.05, 3), 0.05) for s in range(S)]
        obst = np.zeros((O, 8))
        obst[:, 1:4] = rng.uniform(-0.8, 0.8, (O, 3))
        obst[:, 4:7] = obst[:, 1:4] + rng.uniform(-0.3, 0.3, (O, 3))
        obst[:, 7] = 0.03
        obst[3::4] = [1.0, 0.0, 0.0, 1.0, -0.2, 0.0, 0.0, 0.0]               # every fourth: a floor
        mats = np.tile([2.0e3, 40.0, 0.3, 1e-3], (O, 1))                     # soft: k dt^2 / m_eff stays far below 1 at dt = 5e-4
        if args.lc_per_instance:
            obst = np.ascontiguousarray(np.repeat(obst[:, None, :], B, axis=1))
        timed_us, _ = stream_timer(ctrl)

        def period_us():
            t0 = time.perf_counter()
            ctrl.rolloutAsync(K, 5e-4, args.substeps, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / K * 1e6

        def integrate_us():
            return timed_us(lambda: ctrl._call("saip_batch_integrate", 5e-4, 1, None, 0.0), 200)

        def evaluate_us():
            return timed_us(lambda: ctrl._call("saip_batch_link_contact_evaluate"), 200, first=ctrl.evaluateLinkContact)

        if args.link_object:
            # the pushed object on top of link contact: a box of corner spheres in front of the end-effector, resting state; the leg with link
            # contact alone (the launch the object's launch replaces) runs before and after it in the same process.  Every instance of this
            # bench starts at the same posture, so instance 0's end-effector position places the object for all of them
            P = args.lo_spheres
            corners = [(np.array([sx, sy, sz]) * 0.04, 0.03) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)][:P]
            ctrl.attachLinkContact(spheres, obst, mats, per_instance=args.lc_per_instance)
            place = np.r_[robot.position("end-effector", (0.0, 0.0, 0.03))[0] + [0.08, 0.0, 0.0], 1.0, np.zeros(9)]
            for _ in range(args.repeats):
                snap = ctrl.saveState()
                plain, plain_i, plain_e = period_us(), integrate_us(), evaluate_us()
                ctrl.restoreState(snap)
                ctrl.attachLinkObject(corners, [2.0e3, 40.0, 0.3, 1e-3], [0.5, 1e-3, 1e-3, 1e-3], state=place)
                both = ctrl.saveState()                                      # (the directory has the object's segment now)
                period_us()
                ctrl.restoreState(both)
                ctrl.resetObjectSummary()
                with_o, with_i, alone = period_us(), integrate_us(), evaluate_us()
                touched = int((ctrl.objectSummary()["substeps_in_contact"] > 0).sum())
                ctrl.detachLinkObject()
                ctrl.restoreState(snap)
                again = period_us()
                ctrl.restoreState(snap)
                both.close()
                snap.close()
                n_sub = args.substeps
                print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'} substeps {n_sub}, link contact of {S} spheres, {O} obstacles: "
                      f"period {plain:.1f} us, integrate {plain_i:.2f} us, EVALUATE launch {plain_e:.2f} us; with the object of {P} spheres: period {with_o:.1f} us "
                      f"(+{(with_o - plain) / n_sub:.2f} us per substep), integrate {with_i:.2f} us, launch alone {alone:.2f} us; without it again {again:.1f} us "
                      f"({touched} of {B} instances pushed)")
            ctrl.detachLinkContact()
            continue
        for _ in range(args.repeats):
            snap = ctrl.saveState()
            plain, plain_i = period_us(), integrate_us()
            ctrl.restoreState(snap)
            ctrl.attachLinkContact(spheres, obst, mats, per_instance=args.lc_per_instance)
            period_us()
            ctrl.restoreState(snap)
            ctrl.resetLinkContactSummary()
            with_c, with_i, alone = period_us(), integrate_us(), evaluate_us()
            touched = int((ctrl.linkContactSummary()["substeps_in_contact"] > 0).sum())
            ctrl.detachLinkContact()
            ctrl.restoreState(snap)
            again = period_us()
            ctrl.restoreState(snap)
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'} substeps {args.substeps}: "
                  f"closed-loop period {plain:.1f} us, integrate {plain_i:.2f} us; with link contact of {S} spheres, {O} "
                  f"{'per-instance' if args.lc_per_instance else 'batch-uniform'} obstacles: period {with_c:.1f} us, integrate {with_i:.2f} us; without it again "
                  f"{again:.1f} us; one EVALUATE launch alone {alone:.2f} us ({touched} of {B} instances touched)")
        continue
    if args.plant:
        Wn = args.plant_wrenches
        rng = np.random.default_rng(0)
        table = np.repeat(ctrl.neutralPlantJoints()[:, None, :], B, axis=1)
        table[..., 0], table[..., 1], table[..., 2] = rng.uniform(0.95, 1.05, (7, B)), rng.uniform(-0.1, 0.1, (7, B)), rng.uniform(20.0, 80.0, (7, B))
        table[..., 3], table[..., 4], table[..., 5] = rng.uniform(0.0, 0.2, (7, B)), rng.uniform(0.0, 0.3, (7, B)), 0.05
        table[..., 8], table[..., 9] = 500.0, 5.0
        names = ["end-effector", "link6", "link4", "link2"]
        wr = []
        for w in range(Wn):
            v = np.zeros((B, 8))
            v[:, 2], v[:, 6:] = -9.81 * rng.uniform(0.2, 1.0, B), [-np.inf, np.inf]
            wr.append((names[w], (0.0, 0.0, 0.05), "link" if w % 2 else "world", v))
        timed_us, _ = stream_timer(ctrl)

        def period_us():
            t0 = time.perf_counter()
            ctrl.rolloutAsync(K, 5e-4, args.substeps, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / K * 1e6

        def substep_us():
            return timed_us(lambda: ctrl.integrate(5e-4, 1, gravity=(0, 0, 0)), 200)

        if args.plant_chain is not None:
            depth = args.plant_chain
            chain = np.zeros((7, B, 3))
            chain[..., 0], chain[..., 1], chain[..., 2] = rng.integers(0, depth + 1, (7, B)), rng.uniform(2e3, 2e4, (7, B)), rng.uniform(5e-4, 5e-3, (7, B))
            ctrl.attachPlant(table, wr, per_instance=True)
            period_us()
            for _ in range(args.repeats):
                plain, plain_s = period_us(), substep_us()
                ctrl.attachActuationChain(chain, per_instance=True, depth=depth)
                period_us()
                with_c, with_s = period_us(), substep_us()
                nbytes = ctrl.actuationChainInfo()["state_bytes"]
                finite = bool(np.isfinite(ctrl.pullState()[0]).all())
                ctrl.detachActuationChain()
                again, again2 = period_us(), period_us()
                print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'} substeps {args.substeps}: "
                      f"closed-loop period with the plant model alone {plain:.1f} us; with a per-instance actuation chain of depth {depth} in front of it {with_c:.1f} us; "
                      f"alone again {again:.1f} us, and once more {again2:.1f} us; one substep on the stream {plain_s:.2f} us without, {with_s:.2f} us with the chain "
                      f"({nbytes} bytes of chain state; state finite: {finite})")
            ctrl.detachPlant()
            continue
        for _ in range(args.repeats):
            plain, plain_s = period_us(), substep_us()
            ctrl.attachPlant(table, wr, per_instance=True)
            period_us()
            with_p, with_s = period_us(), substep_us()
            clipped = int((ctrl.plantSummary()["max_clip"] > 0).sum())
            ctrl.detachPlant()
            again = period_us()
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'} substeps {args.substeps}: "
                  f"closed-loop period {plain:.1f} us; with a per-instance plant model and {Wn} wrench(es) {with_p:.1f} us; without it again {again:.1f} us; "
                  f"one substep on the stream {plain_s:.2f} us plain, {with_s:.2f} us with the plant: launch alone {with_s - plain_s:.2f} us "
                  f"({clipped} of {B} instances clipped a torque)")
        continue
    if args.sensing_chain is not None:
        rng = np.random.default_rng(0)
        depth, T = args.sensing_chain, 5e-4
        table = np.zeros((7, B, 6))
        table[..., 0], table[..., 1], table[..., 2] = rng.uniform(-5e-3, 5e-3, (7, B)), 2 * np.pi / 2 ** 14, 1e-4
        table[..., 3], table[..., 4], table[..., 5] = rng.uniform(-1e-2, 1e-2, (7, B)), 0.0, 5e-3
        chain = np.zeros((7, B, 4))
        chain[..., 0], chain[..., 1] = rng.integers(0, depth + 1, (7, B)), 1.0
        chain[..., 2], chain[..., 3] = ctrl.sensingChainAlpha(200.0, T), ctrl.sensingChainAlpha(50.0, T)
        timed_us, _ = stream_timer(ctrl)

        def period_us():
            t0 = time.perf_counter()
            ctrl.rolloutAsync(K, T, args.substeps, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / K * 1e6

        ctrl.attachSensing(table, per_instance=True, seed=1)
        period_us()
        for _ in range(args.repeats):
            plain = period_us()
            alone_s = timed_us(ctrl.measureState, 200)
            ctrl.attachSensingChain(chain, per_instance=True, depth=depth, sample_time=T)
            period_us()
            with_c = period_us()
            alone_c = timed_us(ctrl.measureState, 200)
            nbytes = ctrl.sensingChainInfo()["state_bytes"]
            finite = bool(np.isfinite(ctrl.pullState()[0]).all())
            ctrl.detachSensingChain()
            again, again2 = period_us(), period_us()
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'} substeps {args.substeps}: "
                  f"closed-loop period with the sensing model alone {plain:.1f} us; with a per-instance sensing chain of depth {depth} behind it {with_c:.1f} us; "
                  f"alone again {again:.1f} us, and once more {again2:.1f} us; one measurement alone {alone_s:.2f} us without, {alone_c:.2f} us with the chain "
                  f"({nbytes} bytes of chain state; state finite: {finite})")
        ctrl.detachSensing()
        continue
    if args.sensing:
        rng = np.random.default_rng(0)
        table = np.zeros((7, B, 6))
        table[..., 0], table[..., 1], table[..., 2] = rng.uniform(-5e-3, 5e-3, (7, B)), 2 * np.pi / 2 ** 14, 1e-4
        table[..., 3], table[..., 4], table[..., 5] = rng.uniform(-1e-2, 1e-2, (7, B)), 0.0, 5e-3
        wrench = None
        if args.sensing_wrench:   # the sensed wrench needs a simulated sensor: a table 2 mm inside every tool, as --contact has it
            p = robot.position("end-effector", (0, 0, 0.07))
            planes = np.zeros((1, B, 8))
            planes[0] = [0, 0, 1, 0, 2.0e4, 400.0, 0.3, 1e-3]
            planes[0, :, 3] = p[:, 2] + 2e-3
            mf.attachContactPlanes(planes, sensor=True, per_instance=True)
            wrench = {mf: np.tile([0.5, 0.01, 0.2], (6, B, 1))}
        timed_us, _ = stream_timer(ctrl)

        def period_us():
            t0 = time.perf_counter()
            ctrl.rolloutAsync(K, 5e-4, args.substeps, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / K * 1e6

        for _ in range(args.repeats):
            plain = period_us()
            ctrl.attachSensing(table, wrenches=wrench, per_instance=True, seed=1)
            period_us()
            with_s = period_us()
            alone = timed_us(ctrl.measureState, 200)
            noisy = float(np.abs(ctrl.measuredState()[0] - ctrl.pullState()[0]).max())
            ctrl.detachSensing()
            again, again2 = period_us(), period_us()
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'} substeps {args.substeps}: "
                  f"closed-loop period {plain:.1f} us; with a per-instance sensing model{' and a wrench table' if wrench else ''} {with_s:.1f} us; without it "
                  f"again {again:.1f} us, and once more {again2:.1f} us; one measurement of q, dq alone {alone:.2f} us (largest |q_meas - q| {noisy:.2e})")
        continue
    if args.inertia:
        Pn = args.inertia_payloads
        lo, hi = np.tile([0.8, -0.02, -0.02, -0.02], (7, 1)), np.tile([1.2, 0.02, 0.02, 0.02], (7, 1))
        plo, phi = np.zeros((Pn, 7)), np.tile([3.0, 0.05, 0.05, 0.05, 0.08, 0.08, 0.08], (Pn, 1))
        timed_us, _ = stream_timer(ctrl)

        def period_us():
            t0 = time.perf_counter()
            ctrl.rolloutAsync(K, 5e-4, args.substeps, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / K * 1e6

        def integrate_us():
            return timed_us(lambda: ctrl.integrate(5e-4, args.substeps, gravity=(0, 0, 0)), 200)

        def draw(rnd=0):
            ctrl.randomizeInertia(1, rnd, bodies=(lo, hi), payloads=(plo, phi) if Pn else None)

        for _ in range(args.repeats):
            plain, plain_i = period_us(), integrate_us()
            ctrl.attachInertia(per_instance=True, payload_links=["end-effector", "link4"][:Pn])
            draw()
            period_us()
            with_t, with_i = period_us(), integrate_us()
            draw_us = timed_us(draw, 50)
            heaviest = float(ctrl.inertiaRows()[6, :, 0].max())
            ctrl.detachInertia()
            again = period_us()
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'} substeps {args.substeps}: "
                  f"closed-loop period {plain:.1f} us; with a per-instance inertia table and {Pn} payload(s) {with_t:.1f} us; without it again {again:.1f} us; "
                  f"integrate on the stream {plain_i:.2f} us plain, {with_i:.2f} us with the table; one draw of the table {draw_us:.2f} us, uploads "
                  f"of the bounds included (the heaviest last body has {heaviest:.2f} kg)")
        continue
    if args.goal_schedule:
        def timed(calls, steps):
            t0 = time.perf_counter()
            for _ in range(calls):
                ctrl.rolloutAsync(steps, 5e-4, 2, gravity=(0, 0, 0))
            ctrl.synchronize()
            return (time.perf_counter() - t0) / (calls * steps) * 1e6

        rng = np.random.default_rng(0)
        goal = mf._get_goal()[:, :12]
        keys = np.repeat(goal[None], 8, axis=0)
        keys[:, :, :3] += rng.uniform(-0.03, 0.03, (8, B, 3))
        for k in range(8):      # small rotations about the vertical in front of the goal orientation
            a = rng.uniform(-0.2, 0.2, B)
            Rz = np.zeros((B, 3, 3))
            Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1.0
            keys[k, :, 3:] = (Rz @ goal[:, 3:].reshape(B, 3, 3)).reshape(B, 9)
        for _ in range(args.repeats):
            plain = timed(1, K)
            unfused = timed(K, 1)
            mf.setGoalSchedule((0, 12), keys, stride=50, mode=args.goal_schedule)
            timed(1, 50)
            ctrl.rewindGoalSchedules()
            scheduled = timed(1, K)
            mf.clearGoalSchedule()
            mf.setGoalPosition(goal[:, :3])
            mf.setGoalOrientation(goal[:, 3:].reshape(B, 3, 3))
            print(f"{os.path.basename(os.environ.get('SAIP_LIB', 'libsaip.so'))} B={B} otg {'off' if args.no_otg else 'on'}: closed-loop period {plain:.1f} us; "
                  f"one rollout call per period {unfused:.1f} us; with a {args.goal_schedule} goal schedule {scheduled:.1f} us")
        continue
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
