"""Test-side robot descriptions and task stacks for serial chains of any size (a helper module, not a conftest):

  * random_chain: n dof, revolute / prismatic mix, general and axis-aligned axes, offset inertias, optional massive fixed links in
    the middle of the chain and at the tip (the engine merges those into their parent body; workloads.fk / mass_matrix and the C
    oracle treat every link as its own body, so they check that merge independently);
  * planar_arm: n revolute joints about z, 0.5 m links along x (the shape of a planar RR..R arm);
  * puma_arm: a 6R arm of the PUMA layout (waist, shoulder, elbow, spherical wrist), written from plain geometry;
  * goals: goal blocks near the current pose;
  * cycle_stacks: the task stacks the small-chain tests run, each valid for its dof (no motion-force task with more controlled
    directions than the robot has joints)."""
import numpy as np

import workloads as W

XYZ = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]


def _link(name, joint_type, xyz, rpy, axis, mass, com, inertia, lo=-2.5, hi=2.5, effort=40.0):
    return dict(name=name, joint_type=joint_type, origin_xyz=list(map(float, xyz)), origin_rpy=list(map(float, rpy)),
                axis=list(map(float, axis)), mass=float(mass), com=list(map(float, com)), inertia=list(map(float, inertia)),
                q_lower=float(lo), q_upper=float(hi), velocity_limit=3.0, effort_limit=float(effort), q_nominal_deg=0.0)


def _random_inertia(rng, lo=0.004, hi=0.03):
    ine = rng.uniform(lo, hi, 3)
    off = rng.uniform(-0.002, 0.002, 3)
    return [ine[0], ine[1], ine[2], off[0], off[1], off[2]]


def random_chain(rng, n, name, *, fixed_after=(), fixed_tip=False, prismatic_share=0.2):
    """n movable links link1..linkn; a massive fixed link `fixed<i>` follows link i for every i in fixed_after, and a massive fixed
    `tool` link ends the chain when fixed_tip (both with a rotated frame, so their inertia is rotated into the parent body)"""
    links = []
    for i in range(n):
        prismatic = i > 0 and rng.random() < prismatic_share
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        if rng.random() < 0.4:
            ax = np.eye(3)[rng.integers(3)]
        links.append(_link(f"link{i + 1}", "prismatic" if prismatic else "revolute",
                           rng.uniform(-0.05, 0.15, 3) if i else [0.0, 0.0, 0.1], rng.uniform(-1.0, 1.0, 3), ax, rng.uniform(0.3, 2.0),
                           rng.uniform(-0.05, 0.05, 3), _random_inertia(rng), -0.3 if prismatic else -2.5, 0.3 if prismatic else 2.5,
                           rng.uniform(20, 60)))
        if i + 1 in fixed_after:
            links.append(_fixed(rng, f"fixed{i + 1}"))
    if fixed_tip:
        links.append(_fixed(rng, "tool"))
    return dict(name=name, links=links)


def _fixed(rng, name):
    return _link(name, "fixed", rng.uniform(-0.05, 0.1, 3), rng.uniform(-1.0, 1.0, 3), [0.0, 0.0, 1.0], rng.uniform(1.0, 3.0),
                 rng.uniform(-0.05, 0.05, 3), _random_inertia(rng, 0.01, 0.05))


def planar_arm(n, name=None):
    """n revolute joints about z, links of 0.5 m along x, each a slender 1 kg rod centred on its link (moves in the xy plane)"""
    rod = [0.0005, 0.021, 0.021, 0.0, 0.0, 0.0]   # 1 kg, 0.5 m, 1 cm radius: about its own axis / across it
    links = [_link(f"link{i + 1}", "revolute", [0.5 if i else 0.0, 0.0, 0.0], [0, 0, 0], [0, 0, 1], 1.0, [0.25, 0.0, 0.0], rod,
                   -2.9, 2.9, 50.0) for i in range(n)]
    return dict(name=name or f"planar{n}r", links=links)


def puma_arm(name="puma6"):
    """6R: waist (z), shoulder and elbow (y, parallel), a spherical wrist roll (x) - pitch (y) - roll (x) whose axes meet in one point.
    Elbow singular at q3 = 0 (the forearm stretched along the upper arm), wrist singular at q5 = 0 (axes 4 and 6 aligned)."""
    spec = [  # xyz of the joint in the previous link, axis, mass, com, inertia
        ([0.0, 0.0, 0.66], [0, 0, 1], 8.0, [0.0, 0.0, -0.1], [0.2, 0.2, 0.35, 0.0, 0.0, 0.0]),
        ([0.0, 0.24, 0.0], [0, 1, 0], 17.0, [0.2, 0.0, 0.01], [0.13, 0.52, 0.54, 0.0, 0.01, 0.0]),
        ([0.43, -0.09, 0.0], [0, 1, 0], 4.8, [0.2, 0.0, 0.0], [0.07, 0.09, 0.08, 0.0, 0.002, 0.0]),
        ([0.43, 0.0, 0.0], [1, 0, 0], 0.8, [0.0, 0.0, 0.02], [0.002, 0.0018, 0.0013, 0.0, 0.0, 0.0001]),
        ([0.0, 0.0, 0.0], [0, 1, 0], 0.35, [0.0, 0.0, 0.01], [0.0003, 0.0004, 0.0003, 0.0, 0.0, 0.0]),
        ([0.0, 0.0, 0.0], [1, 0, 0], 0.1, [0.03, 0.0, 0.0], [0.00015, 0.00015, 0.00004, 0.0, 0.0, 0.0]),
    ]
    effort = [97.0, 186.0, 89.0, 24.0, 20.0, 21.0]
    links = [_link(f"link{i + 1}", "revolute", xyz, [0, 0, 0], ax, m, c, ine, -2.8, 2.8, effort[i])
             for i, (xyz, ax, m, c, ine) in enumerate(spec)]
    return dict(name=name, links=links)


def puma_postures(rng, B):
    """a third near the wrist singularity (q5 ~ 0), a third near the elbow singularity (q3 ~ 0), a third clearly regular"""
    q = rng.uniform(-2.0, 2.0, (B, 6))
    a, b = B // 3, 2 * B // 3
    q[:a, 4] = rng.uniform(-0.08, 0.08, a)
    q[a:b, 2] = rng.uniform(-0.08, 0.08, b - a)
    q[b:, 2] = rng.choice([-1, 1], B - b) * rng.uniform(0.5, 2.0, B - b)
    q[b:, 4] = rng.choice([-1, 1], B - b) * rng.uniform(0.5, 2.0, B - b)
    return q


def goals(rng, model, tasks, q):
    """goal blocks near the current pose (the generator of workloads.make_inputs for any chain)"""
    B, n = q.shape
    frames = W.fk(model, q)
    out = []
    for t in tasks:
        if t["type"] == "motion_force":
            R, o = frames[model.link_index(t["link"])]
            x = o + np.einsum("bij,j->bi", R, np.asarray(t["pos_in_link"], float))
            Rg = W._expm_so3(rng.uniform(-0.2, 0.2, (B, 3))) @ (R @ np.asarray(t["rot_in_link"], float))
            g = np.concatenate([x + rng.uniform(-0.05, 0.05, (B, 3)), Rg.reshape(B, 9), rng.uniform(-0.1, 0.1, (B, 6)),
                                rng.uniform(-0.5, 0.5, (B, 6))], axis=1)
            gs = W.goal_size(t, n)
            if gs > 24:
                g = np.concatenate([g, rng.uniform(-2, 2, (B, gs - 24))], axis=1)
            out.append(g)
        else:
            S = W.joint_selection(t, n)
            m = S.shape[0]
            out.append(np.concatenate([q @ S.T + rng.uniform(-0.3, 0.3, (B, m)), rng.uniform(-0.1, 0.1, (B, m)),
                                       rng.uniform(-0.5, 0.5, (B, m))], axis=1))
    return out


def _general_selection(n):
    """an (n-1) x n selection of full row rank that is not made of unit rows"""
    S = np.eye(n)[: n - 1].copy()
    S[:, n - 1] += 0.5
    S[0, :] += 0.25
    return S.tolist()


def cycle_stacks(n, kind):
    """name -> (tasks, options) for a chain of n dof; kind 'random' (links link1..linkn), 'planar' or 'puma'.  Every stack is valid
    for its n: the motion-force tasks control at most n directions."""
    tip = f"link{n}"
    S = {}
    if kind == "puma":
        full = dict(ki_pos=2.0, ki_ori=1.0)
        S["full_joint"] = ([W.motion_force_task("hand", tip, (0.1, 0.0, 0.0), **full), W.joint_task("posture", ki=1.0)],
                           dict(gravity_comp=True))
        S["position_joint"] = ([W.motion_force_task("hand", tip, (0.1, 0.0, 0.0), dirs_trans=XYZ, dirs_rot=None, kp_pos=[120.0, 90.0, 150.0]),
                                W.joint_task("posture", kp=[30.0, 40.0, 50.0, 60.0, 70.0, 80.0])], dict(torque_saturation=True))
        S["full_joint_unhandled"] = ([W.motion_force_task("hand", tip, (0.1, 0.0, 0.0), singularity_handling=False),
                                      W.joint_task("posture")], dict(gravity_comp=True))
        S["position_joint_unhandled"] = ([W.motion_force_task("hand", tip, (0.1, 0.0, 0.0), dirs_trans=XYZ, dirs_rot=None,
                                                              singularity_handling=False), W.joint_task("posture")], {})
        return S
    S["joint"] = ([W.joint_task("posture", ki=1.0)], dict(gravity_comp=True))
    if n >= 2:
        S["joint_partial"] = ([W.joint_task("sel", S=_general_selection(n), kp=40.0, kv=12.0)], {})
        S["joint_partial_posture"] = ([W.joint_task("sel", S=[n - 1], kp=[70.0], kv=[15.0], ki=[2.0]),
                                       W.joint_task("posture", decoupling=W.IMPEDANCE)], dict(torque_saturation=True))
    if kind == "planar":
        dirs_rot = [[0, 0, 1]] if n >= 3 else None
        S["planar_joint"] = ([W.motion_force_task("hand", tip, (0.5, 0.0, 0.0), dirs_trans=XYZ[:2], dirs_rot=dirs_rot, ki_pos=2.0),
                              W.joint_task("posture")], dict(gravity_comp=True))
        if n == 4:  # the controller of a planar 4R arm: link4, compliant frame 0.5 m along x, x, y and rotation about z
            S["planar4_controller"] = ([W.motion_force_task("motion_force_task", "link4", (0.5, 0.0, 0.0), dirs_trans=XYZ[:2],
                                                            dirs_rot=[[0, 0, 1]]), W.joint_task("joint_task")], {})
        return S
    if n >= 2:
        S["xy_joint"] = ([W.motion_force_task("hand", tip, (0.0, 0.02, 0.1), dirs_trans=XYZ[:2], dirs_rot=None, decoupling=W.FULL_DYNAMIC_DECOUPLING),
                          W.joint_task("posture", decoupling=W.FULL_DYNAMIC_DECOUPLING)], dict(gravity_comp=True))
    if n >= 3:
        S["position_joint"] = ([W.motion_force_task("hand", tip, (0.0, 0.02, 0.1), dirs_trans=XYZ, dirs_rot=None, ki_pos=3.0),
                                W.joint_task("posture", ki=1.5)], dict(gravity_comp=True, torque_saturation=True, joint_limit_avoidance=True))
        S["position_joint_impedance"] = ([W.motion_force_task("hand", tip, (0.0, 0.0, 0.08), dirs_trans=XYZ, dirs_rot=None, decoupling=W.IMPEDANCE,
                                                              vel_sat=True, lin_sat=0.05),
                                          W.joint_task("posture", decoupling=W.IMPEDANCE, vel_sat=True, sat=0.4)], {})
        S["position_joint_bie"] = ([W.motion_force_task("hand", tip, (0.0, 0.0, 0.08), dirs_trans=XYZ, dirs_rot=None, bie_threshold=0.4),
                                    W.joint_task("posture", bie_threshold=0.4)], {})
    if n >= 4:
        S["joint_above_mf"] = ([W.joint_task("base", S=[0], kp=[60.0], kv=[12.0], ki=[2.0]),
                                W.motion_force_task("hand", tip, (0.0, 0.0, 0.08), dirs_trans=XYZ, dirs_rot=None, ki_pos=3.0),
                                W.joint_task("posture", decoupling=W.IMPEDANCE)], {})
    if n >= 5:
        S["position_tilt_joint"] = ([W.motion_force_task("hand", tip, (0.0, 0.02, 0.1), dirs_trans=XYZ, dirs_rot=[[0, 0, 1], [1, 0, 1]], ki_ori=2.0),
                                     W.joint_task("posture")], dict(gravity_comp=True))
    return S


def small_chain(n, kind, seed=0):
    """the robot description each small-chain test uses for (n, kind): random chains carry a massive fixed link mid-chain (n >= 2)
    and at the tip"""
    if kind == "planar":
        return planar_arm(n)
    if kind == "puma":
        return puma_arm()
    rng = np.random.default_rng(1000 + 17 * n + seed)
    return random_chain(rng, n, f"chain{n}", fixed_after=(1,) if n >= 2 else (), fixed_tip=True)


def postures(rng, model, kind, B):
    if kind == "puma":
        return puma_postures(rng, B)
    return rng.uniform(0.8 * model.q_lower, 0.8 * model.q_upper, (B, model.dof))
