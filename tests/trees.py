"""Test-side kinematic-tree robots and a NumPy tree oracle (a helper module, not a conftest).

Robots are composed here from the in-repo panda_arm.json and tests/chains.py; every link may carry "parent" (a link name, None for the
fixed base, absent for the link listed before it):
  * dual_panda_fixed_torso: a forest, two 7-dof Pandas on a fixed torso link with its own mass;
  * dual_panda_torso: 15 dof, a revolute torso yaw carrying both arms;
  * panda_with_side_frames: a Panda with fixed side frames off link4 and off the flange (massless or massive); a chain after merging;
  * random_tree: seeded trees of revolute and prismatic joints with fixed links in the middle of the tree, some with two children;
  * chain_as_tree: any chain description with every parent written out.

tree_fk / tree_jacobian / tree_mass_matrix are workloads.fk / jacobian / mass_matrix over a tree: each link starts from its parent's
frame, and a point's Jacobian has a column for each movable link on the path from the base.  `tree_oracle()` swaps them into workloads and
oracle/restatement.py (which imports them by name), so the restatement's controller, gravity vector, forward dynamics and energy become a
tree oracle without any change to the files under oracle/."""
import contextlib
import copy
import os

import numpy as np

import chains as CH
import workloads as W

_ROBOTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sai-primitives_amd", "robots")


def panda_links(prefix=""):
    import json
    with open(os.path.join(_ROBOTS, "panda_arm.json")) as f:
        links = copy.deepcopy(json.load(f)["links"])
    for l in links:
        l["name"] = prefix + l["name"]
    return links


def _arm(prefix, parent, xyz, rpy):
    links = panda_links(prefix)
    links[0]["parent"] = parent
    links[0]["origin_xyz"] = list(map(float, xyz))
    links[0]["origin_rpy"] = list(map(float, rpy))
    for a, b in zip(links, links[1:]):
        b["parent"] = a["name"]
    return links


def _torso(name, joint_type):
    return CH._link(name, joint_type, [0.0, 0.0, 0.4], [0, 0, 0], [0, 0, 1], 12.0, [0.0, 0.02, 0.2], [0.5, 0.45, 0.3, 0.001, 0.0, 0.002],
                    -2.6, 2.6, 120.0)


def dual_panda_fixed_torso():
    """forest: a massive fixed torso on the base, two 7-dof arms on it (dof 0..6 left, 7..13 right)"""
    torso = _torso("torso", "fixed")
    torso["parent"] = None
    links = [torso] + _arm("left_", "torso", [0.0, 0.25, 0.3], [-0.6, 0.0, 0.0]) + _arm("right_", "torso", [0.0, -0.25, 0.3], [0.6, 0.0, 0.0])
    return dict(name="dual_panda_fixed_torso", links=links)


def dual_panda_torso():
    """15 dof: a revolute torso yaw (dof 0) carrying two arms (dof 1..7 left, 8..14 right), with a fixed shoulder plate in between"""
    torso = _torso("torso", "revolute")
    torso["parent"] = None
    plate = CH._link("shoulders", "fixed", [0.0, 0.0, 0.3], [0.0, 0.0, 0.1], [0, 0, 1], 2.0, [0.0, 0.0, 0.05], [0.02, 0.03, 0.04, 0.0, 0.0, 0.0])
    plate["parent"] = "torso"
    links = [torso, plate] + _arm("left_", "shoulders", [0.0, 0.25, 0.0], [-0.6, 0.0, 0.0]) + _arm("right_", "shoulders", [0.0, -0.25, 0.0], [0.6, 0.0, 0.0])
    return dict(name="dual_panda_torso", links=links)


def panda_with_side_frames(massive=False):
    """a Panda with a camera off link4 and a tool frame beside the flange (fixed side branches): still a chain after merging"""
    links = panda_links()
    m = 0.4 if massive else 0.0
    ine = [0.001, 0.002, 0.0015, 0.0, 0.0001, 0.0] if massive else [0.0] * 6
    cam = CH._link("camera", "fixed", [0.05, 0.02, 0.03], [0.3, -0.2, 0.1], [0, 0, 1], m, [0.01, 0.0, 0.02], ine)
    cam["parent"] = "link4"
    tool = CH._link("tool_side", "fixed", [0.04, -0.03, 0.02], [0.0, 0.4, -0.3], [0, 0, 1], m, [0.0, 0.01, 0.0], ine)
    tool["parent"] = "link7"
    # the camera goes between link4 and link5 in the list; link5 names link4 as its parent
    for l, p in zip(links[1:], links):
        l["parent"] = p["name"]
    out = links[:4] + [cam] + links[4:] + [tool]
    return dict(name="panda_side_frames" + ("_massive" if massive else ""), links=out)


def chain_as_tree(desc):
    """the same chain with every parent written out"""
    d = copy.deepcopy(desc)
    for i, l in enumerate(d["links"]):
        l["parent"] = d["links"][i - 1]["name"] if i else None
    d["name"] = desc["name"] + "_as_tree"
    return d


def random_tree(seed, n):
    """n movable links j1..jn; each hangs off a random earlier link (or the base), about one in three links is followed by a massive
    fixed link, and some fixed links have two children"""
    rng = np.random.default_rng(seed)
    links = []
    for i in range(n):
        prismatic = i > 0 and rng.random() < 0.2
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        if rng.random() < 0.4:
            ax = np.eye(3)[rng.integers(3)]
        l = CH._link(f"j{i + 1}", "prismatic" if prismatic else "revolute", rng.uniform(-0.1, 0.2, 3), rng.uniform(-1.0, 1.0, 3), ax,
                     rng.uniform(0.3, 2.0), rng.uniform(-0.05, 0.05, 3), CH._random_inertia(rng), -0.3 if prismatic else -2.5,
                     0.3 if prismatic else 2.5, rng.uniform(20, 60))
        l["parent"] = None if not links else links[int(rng.integers(-1, len(links)))]["name"] if rng.random() < 0.9 else None
        if l["parent"] is None and links and rng.random() < 0.5:
            l["parent"] = links[-1]["name"]
        links.append(l)
        if rng.random() < 0.35:
            f = CH._fixed(rng, f"f{i + 1}")
            f["parent"] = l["name"]
            links.append(f)
    return dict(name=f"tree{n}_{seed}", links=links)


# --------------------------------------------------------------------------- NumPy tree kinematics
def parent_index(model):
    """parent link index of every link of a workloads.RobotModel (descriptions without "parent": the link before)"""
    names = {l["name"]: i for i, l in enumerate(model.links)}
    out = []
    for i, l in enumerate(model.links):
        if "parent" not in l:
            out.append(i - 1)
        else:
            out.append(-1 if l["parent"] is None else names[l["parent"]])
    return out


def joint_parents(model):
    """movable parent body of every joint (what SaiModel.jointParent returns)"""
    par = parent_index(model)
    body = []
    out = []
    for i, l in enumerate(model.links):
        b = body[par[i]] if par[i] >= 0 else -1
        if l["joint_type"] != "fixed":
            out.append(b)
            b = model.dof_of_link[i]
        body.append(b)
    return out


def tree_fk(model, q):
    """q (B,n) -> list of (R (B,3,3), o (B,3)) per link"""
    q = np.asarray(q, float)
    B = q.shape[0]
    par = parent_index(model)
    out = []
    for li, l in enumerate(model.links):
        if par[li] >= 0:
            R, o = out[par[li]]
        else:
            R, o = np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), np.zeros((B, 3))
        o = o + R @ np.asarray(l["origin_xyz"], float)
        R = R @ W.rot_rpy(l["origin_rpy"])
        d = model.dof_of_link[li]
        if l["joint_type"] == "revolute":
            R = R @ W.rodrigues(l["axis"], q[:, d])
        elif l["joint_type"] == "prismatic":
            a = np.asarray(l["axis"], float)
            o = o + (R @ (a / np.linalg.norm(a))) * q[:, d][:, None]
        out.append((R, o))
    return out


def tree_jacobian(model, frames, link, p_world):
    """(B,6,n) geometric Jacobian [Jv;Jw] of a point fixed in `link`: a column for each movable link on the path from the base"""
    B = p_world.shape[0]
    J = np.zeros((B, 6, model.dof))
    par = parent_index(model)
    li = link
    while li >= 0:
        d = model.dof_of_link[li]
        if d >= 0:
            R, o = frames[li]
            a = np.asarray(model.links[li]["axis"], float)
            z = R @ (a / np.linalg.norm(a))
            if model.links[li]["joint_type"] == "revolute":
                J[:, 0:3, d] = np.cross(z, p_world - o)
                J[:, 3:6, d] = z
            else:
                J[:, 0:3, d] = z
        li = par[li]
    return J


def tree_mass_matrix(model, frames):
    """M = sum over links of m Jv^T Jv + Jw^T (R I R^T) Jw"""
    B = frames[0][0].shape[0]
    M = np.zeros((B, model.dof, model.dof))
    for li, l in enumerate(model.links):
        R, o = frames[li]
        c = o + R @ np.asarray(l["com"], float)
        J = tree_jacobian(model, frames, li, c)
        ixx, iyy, izz, ixy, ixz, iyz = l["inertia"]
        I = np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]])
        Iw = R @ I @ np.swapaxes(R, 1, 2)
        Jv, Jw = J[:, :3], J[:, 3:]
        M += l["mass"] * np.swapaxes(Jv, 1, 2) @ Jv + np.swapaxes(Jw, 1, 2) @ Iw @ Jw
    return M


@contextlib.contextmanager
def tree_oracle():
    """workloads.fk / jacobian / mass_matrix and their names inside oracle/restatement.py replaced by the tree versions"""
    import restatement as RS
    saved = [(mod, name, getattr(mod, name)) for mod in (W, RS) for name in ("fk", "jacobian", "mass_matrix")]
    try:
        for mod in (W, RS):
            mod.fk, mod.jacobian, mod.mass_matrix = tree_fk, tree_jacobian, tree_mass_matrix
        yield RS
    finally:
        for mod, name, f in saved:
            setattr(mod, name, f)


def tree_goals(rng, model, tasks, q):
    """chains.goals with the tree kinematics"""
    with tree_oracle():
        return CH.goals(rng, model, tasks, q)


def dual_stack(model, *, partial=False, decoupling=None):
    """[MF on the left flange, MF on the right flange, full JointTask] for a dual-arm description"""
    kw = dict(decoupling=decoupling) if decoupling is not None else {}
    if partial:
        kw.update(dirs_trans=CH.XYZ, dirs_rot=None)
    return [W.motion_force_task("left", "left_link7", (0.0, 0.0, 0.1), **kw), W.motion_force_task("right", "right_link7", (0.0, 0.0, 0.1), **kw),
            W.joint_task("posture", **({"decoupling": decoupling} if decoupling is not None else {}))]
