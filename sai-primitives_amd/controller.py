"""Batched mirror of the reference's task/controller interface on top of the C-ABI.

Same class and method names as the reference (camelCase kept on purpose so that call sequences read like
/root/reference/examples/05-using_robot_controller/05-using_robot_controller.cpp:103-196), with every
per-robot Eigen vector replaced by a (B, size) NumPy array.  Differences from the reference, all loud:
  * one SaiModel object = B robot instances of the same robot (state arrays are (B, dof));
  * the internal OTG is ENABLED by default like in the reference: the acceleration-limited mode (the reference default) of both
    the joint OTG (OTG_joints) and the Cartesian OTG (OTG_6dof_cartesian) runs on the device; the jerk-limited mode raises
    SaipUnsupported;
  * a task can be driven by hand exactly like in the reference (TemplateTask.h:43-60: updateTaskModel(N_prec), computeTorques(),
    computeTorques(tau_prec), get*Nullspace; examples/04-task_and_redundancy): inside a RobotController it uses the controller's batch,
    on its own it owns a private one-task batch on the same device.
"""
from __future__ import annotations

import ctypes as C
import weakref
import enum
import json
import math
import os
from dataclasses import dataclass

import numpy as np

from . import capi

_ROBOT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "robots")
_JT = {"fixed": 0, "revolute": 1, "prismatic": 2}


class TaskType(enum.IntEnum):  # TemplateTask.h:19-24
    UNDEFINED = 0
    JOINT_LIMIT_AVOIDANCE_TASK = 1
    JOINT_TASK = 2
    MOTION_FORCE_TASK = 3


class DynamicDecouplingType(enum.IntEnum):  # SaiPrimitivesCommonDefinitions.h:14-20
    FULL_DYNAMIC_DECOUPLING = 0
    BOUNDED_INERTIA_ESTIMATES = 1
    IMPEDANCE = 2


@dataclass
class PIDGains:  # SaiPrimitivesCommonDefinitions.h:26-32
    kp: float
    kv: float
    ki: float


def load_robot_description(name_or_path: str) -> dict:
    path = name_or_path if os.path.exists(name_or_path) else os.path.join(_ROBOT_DIR, name_or_path + ".json")
    with open(path) as f:
        return json.load(f)


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _check_otg_limits(who, **limits):
    """what the reference's OTG wrappers check before they touch any member (OTG_joints.cpp:41-86, OTG_6dof_cartesian.cpp:59-117): every
    limit strictly positive.  Checked here so that a task outside any batch rejects the call as well, before anything is logged."""
    for what, v in limits.items():
        if not np.all(np.asarray(v) > 0):
            raise ValueError(f"max {what} cannot be 0 or negative in any directions in {who}::setMax{what.capitalize()}")


def _soa(a, B, comps, what):
    """(B, comps) user array -> contiguous [comps][B] host staging array"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1 and comps == a.shape[0]:
        a = np.broadcast_to(a, (B, comps))
    if a.shape != (B, comps):
        raise ValueError(f"{what}: expected shape ({B}, {comps}), got {a.shape}")
    return np.ascontiguousarray(a.T)


def _link_parents(links):
    """parent link indices of a robot description whose links name their "parent" (a link name, or None for the fixed base; a link
    without the key hangs off the link listed before it), or None when no link names one (a serial chain, as every description was)"""
    if not any("parent" in l for l in links):
        return None
    index = {}
    out = []
    for i, l in enumerate(links):
        if "parent" not in l:
            out.append(i - 1)
        elif l["parent"] is None:
            out.append(-1)
        else:
            if l["parent"] not in index:  # unknown, or listed after its child: the C-ABI reports the latter with the link's name
                known = {x["name"]: k for k, x in enumerate(links)}
                if l["parent"] not in known:
                    raise ValueError(f"link {l['name']}: parent link {l['parent']} is not in the robot description")
                out.append(known[l["parent"]])
            else:
                out.append(index[l["parent"]])
        index[l["name"]] = i
    return out


class SaiModel:
    """B instances of one robot (batched stand-in for SaiModel::SaiModel: constants + q/dq state)."""

    def __init__(self, description, batch_size: int, device: int = 0):
        desc = load_robot_description(description) if isinstance(description, str) else description
        self.description = desc
        links = desc["links"]
        arr = (capi.LinkDesc * len(links))()
        for d, l in zip(arr, links):
            d.name = l["name"].encode()
            d.joint_type = _JT[l["joint_type"]]
            d.origin_xyz[:] = l["origin_xyz"]
            d.origin_rpy[:] = l["origin_rpy"]
            d.axis[:] = l["axis"]
            d.mass = l["mass"]
            d.com[:] = l["com"]
            d.inertia[:] = l["inertia"]
            d.q_lower, d.q_upper = l["q_lower"], l["q_upper"]
            d.velocity_limit, d.effort_limit = l["velocity_limit"], l["effort_limit"]
        L = capi.lib()
        h = C.c_void_p()
        parents = _link_parents(links)
        if parents is None:
            capi.check(L.saip_model_create_serial_chain(arr, len(links), C.byref(h)))
        else:
            capi.check(L.saip_model_create_tree(arr, (C.c_int * len(links))(*parents), len(links), C.byref(h)))
        self._h = h
        self._n = L.saip_model_dof(h)
        self.batch_size = int(batch_size)
        self.device = int(device)
        self._q = np.zeros((self.batch_size, self._n))
        self._dq = np.zeros((self.batch_size, self._n))
        self._controller = None
        # every batch that mirrors this robot's state: the RobotController and the private batches of tasks driven by hand.  Weak
        # references: a controller the user dropped must be collectable (its __del__ frees the device batch) and must not keep receiving
        # the robot's state at every updateModel()
        self._controllers = weakref.WeakSet()
        self._state_version = 0
        # model queries (position(), J(), M(), ...): the state of the last updateModel(), mirrored into a batch of their own (created at
        # the first query, pushed to at every updateModel(); a setQ() that no updateModel() followed is never seen), and T_world_robot
        self._model_q, self._model_dq = self._q.copy(), self._dq.copy()
        self._model_version = 0
        self._mq = None
        self._mq_version = -1
        self._T_base = np.eye(4)

    def __del__(self):
        if getattr(self, "_mq", None):  # the query batch refers to the model: it goes first
            capi.lib().saip_batch_destroy(self._mq)
            self._mq = None
        if getattr(self, "_h", None):
            capi.lib().saip_model_destroy(self._h)
            self._h = None

    def dof(self) -> int:
        return self._n

    def q(self):
        return self._q

    def dq(self):
        return self._dq

    def setQ(self, q):
        q = np.asarray(q, float)
        if q.shape != (self.batch_size, self._n):
            raise ValueError(f"setQ: expected shape ({self.batch_size}, {self._n})")
        self._q = q.copy()
        self._state_version += 1

    def setDq(self, dq):
        dq = np.asarray(dq, float)
        if dq.shape != (self.batch_size, self._n):
            raise ValueError(f"setDq: expected shape ({self.batch_size}, {self._n})")
        self._dq = dq.copy()
        self._state_version += 1

    def updateModel(self):
        """pushes q/dq to the device; kinematics and dynamics are evaluated inside the cycle kernel.  The model queries below answer for
        this state until the next updateModel()."""
        for c in list(self._controllers):
            c._push_state()
        self._model_q, self._model_dq = self._q.copy(), self._dq.copy()
        self._model_version += 1
        if self._mq is not None:
            self._push_model_state()

    def jointLimits(self):
        n = self._n
        out = [np.zeros(n) for _ in range(4)]
        capi.check(capi.lib().saip_model_joint_limits(self._h, *[_dptr(a) for a in out]))
        return dict(position_lower=out[0], position_upper=out[1], velocity=out[2], effort=out[3])

    def linkIndex(self, name: str) -> int:
        return capi.lib().saip_model_link_index(self._h, name.encode())

    def jointParent(self, joint: int) -> int:
        """movable parent body of joint `joint` (-1: the fixed base); the topology of a tree after fixed-link merging"""
        p = capi.lib().saip_model_joint_parent(self._h, int(joint))
        if p == -2:
            raise ValueError(f"jointParent: joint index {joint} out of range [0, {self._n})")
        return p

    # -- model queries: the SaiModel accessors at the state of the last updateModel() (C-ABI saip_batch_model_frames_host /
    # saip_batch_model_dynamics_host on a model-only batch).  Links by name or by linkIndex() value.
    def _link(self, link) -> int:
        if isinstance(link, str):
            i = self.linkIndex(link)
            if i < 0:
                raise ValueError(f"link {link} does not exist in the robot model")
            return i
        return int(link)

    def _push_model_state(self):
        if self.device >= 0 and self._mq_version != self._model_version:
            q, dq = np.ascontiguousarray(self._model_q.T), np.ascontiguousarray(self._model_dq.T)
            capi.check(capi.lib().saip_batch_set_state_host(self._mq, _dptr(q), _dptr(dq)))
            self._mq_version = self._model_version

    def _query_batch(self):
        if self._mq is None:
            L = capi.lib()
            h = C.c_void_p()
            capi.check(L.saip_batch_create(self._h, self.batch_size, self.device, C.byref(h)))
            try:
                capi.check(L.saip_batch_finalize_model_only(h))
                _set_base(h, self._T_base)
            except Exception:
                L.saip_batch_destroy(h)
                raise
            self._mq = h
        self._push_model_state()
        return self._mq

    def _frames(self, frames, flags):
        """frames: [(link, pos_in_link)] -> (n_frames, rows, B) as saip_batch_model_frames_host writes it"""
        return _model_frames(self._query_batch(), self, frames, flags)

    def _frame(self, link, pos, world, jacobian=False):
        flags = (capi.SAIP_QUERY_WORLD if world else 0) | (capi.SAIP_QUERY_JACOBIAN if jacobian else 0)
        return self._frames([(link, pos)], flags)[0]

    def position(self, link, pos_in_link=(0.0, 0.0, 0.0)):
        """(B, 3) SaiModel::position: the point pos_in_link of the link in the robot base frame"""
        return self._frame(link, pos_in_link, False)[0:3].T.copy()

    def rotation(self, link):
        """(B, 3, 3) SaiModel::rotation: orientation of the link in the robot base frame"""
        return self._frame(link, None, False)[3:12].T.reshape(-1, 3, 3).copy()

    def _transform(self, link, pos, world):
        r = self._frame(link, pos, world)
        T = np.zeros((self.batch_size, 4, 4))
        T[:, :3, :3] = r[3:12].T.reshape(-1, 3, 3)
        T[:, :3, 3] = r[0:3].T
        T[:, 3, 3] = 1.0
        return T

    def transform(self, link, pos_in_link=(0.0, 0.0, 0.0)):
        """(B, 4, 4) SaiModel::transform: pose of the frame (link, pos_in_link) in the robot base frame"""
        return self._transform(link, pos_in_link, False)

    def linearVelocity(self, link, pos_in_link=(0.0, 0.0, 0.0)):
        """(B, 3) SaiModel::linearVelocity of the point pos_in_link of the link, robot base frame"""
        return self._frame(link, pos_in_link, False)[12:15].T.copy()

    def angularVelocity(self, link):
        """(B, 3) SaiModel::angularVelocity of the link, robot base frame"""
        return self._frame(link, None, False)[15:18].T.copy()

    def _jac(self, link, pos, world):
        return self._frame(link, pos, world, jacobian=True)[18:].T.reshape(self.batch_size, 6, self._n).copy()

    def J(self, link, pos_in_link=(0.0, 0.0, 0.0)):
        """(B, 6, dof) SaiModel::J = [Jv; Jw] of the point pos_in_link of the link, robot base frame"""
        return self._jac(link, pos_in_link, False)

    def Jv(self, link, pos_in_link=(0.0, 0.0, 0.0)):
        """(B, 3, dof) SaiModel::Jv"""
        return self._jac(link, pos_in_link, False)[:, :3].copy()

    def Jw(self, link):
        """(B, 3, dof) SaiModel::Jw"""
        return self._jac(link, None, False)[:, 3:].copy()

    def positionInWorld(self, link, pos_in_link=(0.0, 0.0, 0.0)):
        """(B, 3) SaiModel::positionInWorld: position() mapped through TRobotBase()"""
        return self._frame(link, pos_in_link, True)[0:3].T.copy()

    def rotationInWorld(self, link):
        """(B, 3, 3) SaiModel::rotationInWorld"""
        return self._frame(link, None, True)[3:12].T.reshape(-1, 3, 3).copy()

    def transformInWorld(self, link, pos_in_link=(0.0, 0.0, 0.0)):
        """(B, 4, 4) SaiModel::transformInWorld"""
        return self._transform(link, pos_in_link, True)

    def linearVelocityInWorld(self, link, pos_in_link=(0.0, 0.0, 0.0)):
        """(B, 3) SaiModel::linearVelocityInWorld"""
        return self._frame(link, pos_in_link, True)[12:15].T.copy()

    def angularVelocityInWorld(self, link):
        """(B, 3) SaiModel::angularVelocityInWorld"""
        return self._frame(link, None, True)[15:18].T.copy()

    def JWorldFrame(self, link, pos_in_link=(0.0, 0.0, 0.0)):
        """(B, 6, dof) SaiModel::JWorldFrame: J() with both blocks rotated into the world frame"""
        return self._jac(link, pos_in_link, True)

    def JvWorldFrame(self, link, pos_in_link=(0.0, 0.0, 0.0)):
        """(B, 3, dof) SaiModel::JvWorldFrame"""
        return self._jac(link, pos_in_link, True)[:, :3].copy()

    def JwWorldFrame(self, link):
        """(B, 3, dof) SaiModel::JwWorldFrame"""
        return self._jac(link, None, True)[:, 3:].copy()

    def setTRobotBase(self, T):
        """SaiModel::setTRobotBase: (4, 4) T_world_robot, the same for every instance.  It reaches the world-frame queries of every batch
        of this robot; gravity, jointGravityVector() and every torque stay in the robot base frame (include/saip.h)"""
        T = np.array(T, dtype=float)
        if T.shape != (4, 4):
            raise ValueError("setTRobotBase: expected a 4 x 4 homogeneous transform")
        for h in [self._mq] + [c._h for c in list(self._controllers)]:
            if h:
                _set_base(h, T)
        self._T_base = T

    def TRobotBase(self):
        """(4, 4) SaiModel::TRobotBase"""
        return self._T_base.copy()

    def _dynamics(self, which):
        return _model_dynamics(self._query_batch(), self, which)

    def M(self):
        """(B, dof, dof) SaiModel::M: joint-space mass matrix"""
        return self._dynamics(("M",))["M"]

    def MInv(self):
        """(B, dof, dof) SaiModel::MInv"""
        return self._dynamics(("M_inv",))["M_inv"]

    def jointGravityVector(self):
        """(B, dof) SaiModel::jointGravityVector: what gravity compensation adds to the torques (model gravity, robot base frame)"""
        return self._dynamics(("g",))["g"]

    def coriolisForce(self):
        """(B, dof) SaiModel::coriolisForce: C(q, dq) dq, so that M qdd + b + g = tau"""
        return self._dynamics(("b",))["b"]


def _set_base(h, T):
    R = np.ascontiguousarray(T[:3, :3], dtype=float)
    p = np.ascontiguousarray(T[:3, 3], dtype=float)
    capi.check(capi.lib().saip_batch_set_robot_base(h, _dptr(R), _dptr(p)))


def _frame_args(robot, frames):
    """[(link, pos_in_link or None)] or [link] -> (n, int32 link array, float64 [n][3] positions)"""
    frames = [f if isinstance(f, tuple) else (f, None) for f in frames]
    links = np.array([robot._link(l) for l, _ in frames], dtype=np.int32)
    pos = np.array([np.zeros(3) if p is None else np.asarray(p, float).reshape(3) for _, p in frames], dtype=float)
    return len(frames), links, np.ascontiguousarray(pos)


def _model_frames(h, robot, frames, flags, out=None):
    """host: (n_frames, rows, B); device (out = tensor of shape (n_frames, rows, ld) or pointer): enqueued on the batch stream"""
    L = capi.lib()
    nf, links, pos = _frame_args(robot, frames)
    lp = links.ctypes.data_as(C.POINTER(C.c_int))
    rows = L.saip_batch_model_frame_rows(h, int(flags))
    if out is None:
        res = np.empty((nf, max(rows, 1), robot.batch_size))
        capi.check(L.saip_batch_model_frames_host(h, nf, lp, _dptr(pos), int(flags), _dptr(res)))
        return res
    ptr = _device_ptr(out, (nf, rows, L.saip_batch_ld(h)), "getModelFrames")
    capi.check(L.saip_batch_model_frames_device(h, nf, lp, _dptr(pos), int(flags), C.c_void_p(ptr)))
    return out


_DYN_KEYS = ("M", "M_inv", "g", "b")


def _model_dynamics(h, robot, which, out=None):
    """host: dict of the requested quantities, (B, dof, dof) / (B, dof); device (out = {key: tensor (rows, ld) or pointer}): enqueued"""
    L = capi.lib()
    n, B = robot.dof(), robot.batch_size
    rows = {"M": n * n, "M_inv": n * n, "g": n, "b": n}
    if out is not None:
        bad = set(out) - set(_DYN_KEYS)
        if bad:
            raise ValueError(f"getModelDynamics: unknown outputs {sorted(bad)} (expected some of {_DYN_KEYS})")
        ld = L.saip_batch_ld(h)
        ptrs = [C.c_void_p(_device_ptr(out[k], (rows[k], ld), "getModelDynamics")) if k in out else None for k in _DYN_KEYS]
        capi.check(L.saip_batch_model_dynamics_device(h, *ptrs))
        return out
    host = {k: np.empty((rows[k], B)) for k in which}
    capi.check(L.saip_batch_model_dynamics_host(h, *[_dptr(host[k]) if k in host else None for k in _DYN_KEYS]))
    return {k: (v.T.reshape(B, n, n) if k in ("M", "M_inv") else v.T).copy() for k, v in host.items()}   # (by name: n * n == n at 1 dof)


def _device_ptr(out, shape, who):
    if isinstance(out, int):
        return out
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous() or str(out.dtype) != "torch.float64":
        raise ValueError(f"{who}: expected a contiguous float64 device tensor of shape {tuple(shape)}")
    return out.data_ptr()


class _Task:
    """common part of TemplateTask (TemplateTask.h:26-124)"""
    _type = TaskType.UNDEFINED

    def __init__(self, robot: SaiModel, task_name: str, loop_timestep: float):
        self._robot, self._name, self._dt = robot, task_name, float(loop_timestep)
        self._otg_enabled = True  # reference default (JointTask.h:38, MotionForceTask.h:67)
        self._ctrl = None
        self._id = -1
        self._log = []  # every configuration call, replayed into the batch the task joins (its RobotController's or its private one)
        self._keepalive = {}  # (setter, field) -> the arrays its logged arguments point into: replaced, hence released, with the log entry
        self._manual = False  # model last updated through updateTaskModel(N_prec) rather than updateControllerTaskModels()

    # -- TemplateTask accessors
    def getConstRobotModel(self):
        return self._robot

    def getLoopTimestep(self):
        return self._dt

    def getTaskType(self):
        return self._type

    def getTaskName(self):
        return self._name

    def _log_call(self, fn_name, args, key=None, keep=None):
        """the configuration log replayed into the batch the task joins holds the LAST call per setter (per field for setters that address
        several): a caller that sets gains every cycle neither grows it nor replays duplicates.  `keep`: the arrays the logged pointer arguments
        point into; they live exactly as long as the entry."""
        k = (fn_name, key)
        self._log = [e for e in self._log if e[2] != k]
        self._log.append((fn_name, args, k))
        if keep is not None:
            self._keepalive[k] = keep
        else:
            self._keepalive.pop(k, None)

    def _cfg(self, fn_name, *args, keep=None):
        """one configuration call: into the engine first when the task sits in a batch -- a call the engine rejects raises and leaves the log (and
        whatever the caller commits behind this call) as it was, like the reference leaves its members untouched when a setter throws
        (JointTask.cpp:400-409) -- then into the replay log"""
        if self._ctrl is not None:
            self._ctrl._call(fn_name, self._id, *args)
        self._log_call(fn_name, args, keep=keep)

    def reInitializeTask(self):
        """TemplateTask::reInitializeTask of this task alone: goal := current pose, integrators := 0, OTG re-initialised"""
        self._need_ctrl()._push_state()
        self._ctrl._call("saip_batch_reinitialize_task", self._id)

    # -- the reference's per-task interface, TemplateTask.h:43-60 (driven by hand in examples/04-task_and_redundancy/04-task_and_redundancy.cpp:141-206)
    def updateTaskModel(self, N_prec):
        """TemplateTask::updateTaskModel(N_prec): N_prec = nullspace of the higher-priority tasks, (dof, dof) for every instance,
        (B, dof, dof), or the DeviceNullspace another task's getTaskAndPreviousNullspace(device=True) returned (stays on the GPU)."""
        ctrl = self._need_ctrl()
        ctrl._push_state()
        n, B = self._robot.dof(), ctrl.batch_size
        L = capi.lib()
        if isinstance(N_prec, DeviceNullspace):
            if N_prec.n != n or N_prec.batch_size != B:
                raise ValueError("N_prec matrix size not consistent with robot dof in updateTaskModel")
            if N_prec.ctrl is not ctrl:
                capi.check(L.saip_batch_wait_for(ctrl._h, N_prec.ctrl._h))
            capi.check(L.saip_batch_task_update_model_device(ctrl._h, self._id, N_prec.ptr))
        else:
            a = np.asarray(N_prec, float)
            if a.ndim < 2 or a.shape[-1] != a.shape[-2]:  # JointTask.cpp:219-223
                raise ValueError("N_prec matrix not square in updateTaskModel")
            if a.shape[-1] != n or a.ndim > 3 or (a.ndim == 3 and a.shape[0] != B):  # :224-229
                raise ValueError("N_prec matrix size not consistent with robot dof in updateTaskModel")
            a = np.ascontiguousarray(np.broadcast_to(a, (B, n, n)).reshape(B, n * n).T)
            capi.check(L.saip_batch_task_update_model(ctrl._h, self._id, _dptr(a)))
        self._manual = True

    def computeTorques(self, tau_prec=None):
        """TemplateTask::computeTorques() / computeTorques(tau_prec): (B, dof) torques of THIS task; tau_prec (B, dof) = torques of the
        previous tasks (the joint task feed-forward compensates them, JointTask.cpp:285-292).  Per-instance status in self.status."""
        ctrl = self._need_ctrl()
        if not self._manual:
            raise capi.SaipError(f"task [{self._name}]: call updateTaskModel(N_prec) before computeTorques()")
        n, B = self._robot.dof(), ctrl.batch_size
        tau, st = np.empty((n, B)), np.zeros(B, np.uint8)
        tp = None if tau_prec is None else _soa(tau_prec, B, n, "tau_prec")
        capi.check(capi.lib().saip_batch_task_compute_torques(ctrl._h, self._id, None if tp is None else _dptr(tp), _dptr(tau),
                                                               st.ctypes.data_as(C.POINTER(C.c_ubyte))))
        self.status = st
        return tau.T.copy()

    def _manual_nullspace(self, which, device):
        ctrl = self._need_ctrl()
        n, B = self._robot.dof(), ctrl.batch_size
        if device:
            ptr = capi.lib().saip_batch_task_device_nullspace(ctrl._h, self._id, which)
            return DeviceNullspace(ctrl, self, which, ptr, n, B)
        out = np.empty((n * n, B))
        args = [None, None, None]
        args[which] = _dptr(out)
        capi.check(capi.lib().saip_batch_task_get_nullspaces_host(ctrl._h, self._id, *args))
        return out.T.reshape(B, n, n).copy()

    def _gains(self, fn, kp, kv, ki):
        self._gain_cache = getattr(self, "_gain_cache", {})
        self._gain_cache[fn] = tuple(np.atleast_1d(np.asarray(x, float)).copy() for x in (kp, kv, ki))
        kp, kv, ki = (np.atleast_1d(np.asarray(x, float)) for x in (kp, kv, ki))
        size = max(kp.shape[0], kv.shape[0], ki.shape[0])
        for x in (kp, kv, ki):
            if x.ndim != 1 or x.shape[0] not in (1, size):
                raise ValueError("kp, kv and ki must be scalars or vectors of the same size")
        k = [np.ascontiguousarray(np.broadcast_to(x, (size,))) for x in (kp, kv, ki)]
        self._cfg(fn, _dptr(k[0]), _dptr(k[1]), _dptr(k[2]), size, keep=k)

    def setDynamicDecouplingType(self, t):
        self._cfg("saip_batch_set_dynamic_decoupling_type", int(t))

    def setBoundedInertiaEstimateThreshold(self, thr: float):
        self._bie_threshold = max(float(thr), 0.0) if self._type == TaskType.JOINT_TASK else float(thr)  # JointTask.h:372-378 clamps, SingularityHandler.h:81-86 does not
        self._cfg("saip_batch_set_bie_threshold", float(thr))

    def disableInternalOtg(self):
        self._otg_enabled = False
        self._cfg("saip_batch_set_internal_otg", 0)

    def getInternalOtgEnabled(self):
        return self._otg_enabled

    def _desired_block(self):
        """(B, goal_components): what the control law tracks -- the internal OTG's output when enabled, else the goal"""
        ctrl = self._need_ctrl()
        gs = capi.lib().saip_batch_goal_components(ctrl._h, self._id)
        out = np.empty((gs, ctrl._robot.batch_size))
        ctrl._call("saip_batch_get_desired_host", self._id, _dptr(out))
        return out.T

    def getInternalOtgStatus(self):
        """(goal_reached (B,) bool = OTG::isGoalReached, flags (B,) int, result (B,) int = ruckig::Result of the last cycle)"""
        ctrl = self._need_ctrl()
        fl, res = np.zeros(ctrl._robot.batch_size, np.int32), np.zeros(ctrl._robot.batch_size, np.int32)
        ip = C.POINTER(C.c_int)
        ctrl._call("saip_batch_get_otg_status_host", self._id, fl.ctypes.data_as(ip), res.ctypes.data_as(ip))
        return (fl & 1).astype(bool), fl, res

    def enableVelocitySaturation(self, *values):
        """MotionForceTask: (linear_vel_sat, angular_vel_sat); JointTask: (value) or (vector of task dof); () keeps the defaults"""
        self._vel_sat = True
        if values:
            v = np.ascontiguousarray(np.concatenate([np.atleast_1d(np.asarray(x, float)) for x in values]))
            self._sat_vel = tuple(v.tolist())
            self._cfg("saip_batch_set_saturation_velocities", _dptr(v), int(v.shape[0]), keep=v)
        self._cfg("saip_batch_set_velocity_saturation", 1)

    def disableVelocitySaturation(self):
        self._vel_sat = False
        self._cfg("saip_batch_set_velocity_saturation", 0)

    def _cached_gains(self, fn, default):
        g = getattr(self, "_gain_cache", {}).get(fn)
        return [PIDGains(*d) for d in default] if g is None else [PIDGains(*v) for v in zip(*(np.broadcast_to(x, (max(len(y) for y in g),)) for x in g))]

    def _need_ctrl(self):
        """the batch this task is evaluated in: its RobotController's, or -- for a task driven by hand like in the reference's example 04 --
        a private one-task batch created on first use"""
        if self._ctrl is None:
            RobotController(self._robot, [self], _private=True)
        return self._ctrl

    def _set_field(self, first, comps, value, what):
        ctrl = self._need_ctrl()
        a = _soa(value, ctrl._robot.batch_size, comps, what)
        capi.check(capi.lib().saip_batch_set_goal_field_host(ctrl._h, self._id, first, comps, _dptr(a)))

    def _get_goal(self):
        ctrl = self._need_ctrl()
        gs = capi.lib().saip_batch_goal_components(ctrl._h, self._id)
        out = np.empty((gs, ctrl._robot.batch_size))
        capi.check(capi.lib().saip_batch_get_goal_host(ctrl._h, self._id, _dptr(out)))
        return out.T.copy()

    # -- goal schedules: time-varying goals inside rolloutAsync, from keyframes resident on the device (saip.h)
    _SCHED_MODES = {"hold": capi.SAIP_SCHEDULE_HOLD, "linear": capi.SAIP_SCHEDULE_LINEAR}

    def _schedule_fields(self):
        """field name -> (first component, components) of this task's goal block"""
        return {}

    def setGoalSchedule(self, field, keyframes, stride=1, mode="hold"):
        """attach a goal schedule to this task: period c of the controller's rollouts uses keyframe c // stride ("hold") or goes from it
        towards the next one by the fraction (c % stride) / stride ("linear": component-wise, orientations on SO(3)); the last keyframe
        is held.  field: a name of the goal setters ("position", "orientation", "linear_velocity", ... / joint task: "position",
        "velocity", "acceleration") or (first, count) goal components.  keyframes: (K, count) for every instance or (K, B, count) per
        instance; orientations also as (K, 3, 3) / (K, B, 3, 3)."""
        ctrl = self._need_ctrl()
        B = ctrl.batch_size
        if isinstance(field, str):
            fields = self._schedule_fields()
            if field not in fields:
                raise ValueError(f"setGoalSchedule: unknown field {field!r} (one of {sorted(fields)})")
            first, count = fields[field]
        else:
            first, count = (int(v) for v in field)
        if mode not in self._SCHED_MODES:
            raise ValueError(f"setGoalSchedule: unknown mode {mode!r} (one of {sorted(self._SCHED_MODES)})")
        k = np.asarray(keyframes, float)
        if count == 9 and k.shape[-2:] == (3, 3):
            k = k.reshape(k.shape[:-2] + (9,))
        if k.ndim == 2 and k.shape[1] == count:
            a, per_instance = np.ascontiguousarray(k), 0
        elif k.ndim == 3 and k.shape[1:] == (B, count):
            a, per_instance = np.ascontiguousarray(k.transpose(0, 2, 1)), 1
        else:
            raise ValueError(f"setGoalSchedule: keyframes of shape (K, {count}) or (K, {B}, {count}) expected, got {k.shape}")
        ctrl._call("saip_batch_goal_schedule_attach", self._id, first, count, _dptr(a), a.shape[0], int(stride), self._SCHED_MODES[mode], per_instance)

    def clearGoalSchedule(self):
        """detach this task's schedule; its goal keeps the values applied last"""
        self._need_ctrl()._call("saip_batch_goal_schedule_detach", self._id)

    def goalScheduleInfo(self):
        """dict first, count, n_keyframes, stride, mode, period (the period counter every schedule of the controller shares)"""
        v = [C.c_int(0) for _ in range(5)]
        period = C.c_longlong(0)
        self._need_ctrl()._call("saip_batch_goal_schedule_info", self._id, *(C.byref(x) for x in v), C.byref(period))
        mode = {m: name for name, m in self._SCHED_MODES.items()}[v[4].value]
        return dict(first=v[0].value, count=v[1].value, n_keyframes=v[2].value, stride=v[3].value, mode=mode, period=period.value)

    def goalScheduleDevice(self):
        """device pointer of the resident keyframes, (K, count, ld) per instance or (K, count): rewrite them in place on the controller's
        stream (or behind synchronize()) and the next rollout follows the new ones.  None without a schedule."""
        ctrl = self._need_ctrl()
        return capi.lib().saip_batch_goal_schedule_device(ctrl._h, self._id)

    # -- resident rollout sampler: perturb this task's scheduled keyframes around a nominal plan, update the plan from costs (saip.h)
    def _sampler_shape(self):
        """(first, count, K, rotation rows start inside the range or None, d) of this task's schedule as a sampler sees it"""
        info = self.goalScheduleInfo()
        first, count = info["first"], info["count"]
        rot = isinstance(self, MotionForceTask) and first <= 3 and first + count >= 12
        return first, count, info["n_keyframes"], (3 - first if rot else None), (count - 6 if rot else count)

    def _sampler_plan(self, nominal, what):
        _, count, K, _, _ = self._sampler_shape()
        a = np.asarray(nominal, float)
        if count == 9 and a.shape[-2:] == (3, 3):
            a = a.reshape(a.shape[:-2] + (9,))
        if a.shape != (K, count):
            raise ValueError(f"{what}: a nominal plan of shape ({K}, {count}) expected, got {a.shape}")
        return np.ascontiguousarray(a)

    def attachSampler(self, sigma, nominal=None, exempt=1):
        """attach a sampler to this task's goal schedule (per-instance keyframes): perturbGoalSchedules() rewrites the keyframes as
        nominal + sigma * noise, updateSampler() folds the costs back into the nominal plan.  sigma: (d,) standard deviations or one
        number for all; the coordinates are the scheduled rows in order, an orientation (rows 3..11 of a motion-force task) counting as
        three tangent coordinates in radians.  nominal: (K, count), orientations also as (K, 3, 3); None takes instance 0's keyframes.
        exempt: instances 0 .. exempt - 1 always run the nominal plan itself."""
        ctrl = self._need_ctrl()
        _, count, K, _, d = self._sampler_shape()
        sg = np.asarray(sigma, float)
        sg = np.full(d, float(sg)) if sg.ndim == 0 else np.ascontiguousarray(sg)
        if sg.shape != (d,):
            raise ValueError(f"attachSampler: sigma of shape ({d},) expected, got {sg.shape}")
        nom = None if nominal is None else self._sampler_plan(nominal, "attachSampler")
        ctrl._call("saip_batch_sampler_attach", self._id, _dptr(sg), None if nom is None else _dptr(nom), int(exempt))

    def detachSampler(self):
        self._need_ctrl()._call("saip_batch_sampler_detach", self._id)

    def samplerNominal(self):
        """the nominal plan (K, count), read back from the device (waits for the engine stream)"""
        ctrl = self._need_ctrl()
        capi.check(capi.lib().saip_batch_sampler_info(ctrl._h, self._id, None, None, None, None))
        _, count, K, _, _ = self._sampler_shape()
        out = np.empty((K, count))
        ctrl._call("saip_batch_sampler_get_nominal_host", self._id, _dptr(out))
        return out

    def setSamplerNominal(self, nominal):
        ctrl = self._need_ctrl()
        capi.check(capi.lib().saip_batch_sampler_info(ctrl._h, self._id, None, None, None, None))
        ctrl._call("saip_batch_sampler_set_nominal_host", self._id, _dptr(self._sampler_plan(nominal, "setSamplerNominal")))

    def samplerInfo(self):
        """dict d, exempt, seed, round (seed and round are the controller's)"""
        d, ex, seed, rnd = C.c_int(0), C.c_int(0), C.c_ulonglong(0), C.c_longlong(0)
        self._need_ctrl()._call("saip_batch_sampler_info", self._id, C.byref(d), C.byref(ex), C.byref(seed), C.byref(rnd))
        return dict(d=d.value, exempt=ex.value, seed=seed.value, round=rnd.value)

    def getTaskNullspace(self, device=False):
        """(B, dof, dof) nullspace projector N of this task for the current state (TemplateTask.h:71-77)"""
        if self._manual:
            return self._manual_nullspace(0, device)
        ctrl = self._need_ctrl()
        n = self._robot.dof()
        out = np.empty((n * n, ctrl._robot.batch_size))
        capi.check(capi.lib().saip_batch_get_task_nullspace_host(ctrl._h, self._id, _dptr(out)))
        return out.T.reshape(ctrl._robot.batch_size, n, n).copy()

    def getPreviousTasksNullspace(self):
        """(B, dof, dof) N_prec this task was updated with: the product N_{t-1} ... N_0 of the tasks above it (TemplateTask.h:79-83,
        RobotController.cpp:68-77); the identity for the first task"""
        if self._manual:
            return self._manual_nullspace(1, False)
        ctrl = self._need_ctrl()
        n, B = self._robot.dof(), ctrl._robot.batch_size
        Np = np.broadcast_to(np.eye(n), (B, n, n)).copy()
        for s in range(self._id):
            out = np.empty((n * n, B))
            capi.check(capi.lib().saip_batch_get_task_nullspace_host(ctrl._h, s, _dptr(out)))
            Np = out.T.reshape(B, n, n) @ Np
        return Np

    def getTaskAndPreviousNullspace(self, device=False):
        """(B, dof, dof) N N_prec, what the next task in the hierarchy is updated with (TemplateTask.h:85-89); device=True (after
        updateTaskModel) returns a DeviceNullspace handle instead: pass it to the next task's updateTaskModel, nothing crosses PCIe"""
        if self._manual:
            return self._manual_nullspace(2, device)
        return self.getTaskNullspace() @ self.getPreviousTasksNullspace()


class DeviceNullspace:
    """a (B, dof, dof) nullspace matrix resident on the GPU ([dof*dof][ld] row-major per instance): what task.getTaskAndPreviousNullspace(
    device=True) returns and task.updateTaskModel accepts.  Valid until the producing task's next updateTaskModel."""

    def __init__(self, ctrl, task, which, ptr, n, batch_size):
        self.ctrl, self.task, self.which, self.ptr, self.n, self.batch_size = ctrl, task, which, ptr, n, batch_size

    def numpy(self):
        return self.task._manual_nullspace(self.which, False)


class MotionForceTask(_Task):
    """MotionForceTask.h:96-110.  controlled_directions_* = None -> full 6-dof task."""
    _type = TaskType.MOTION_FORCE_TASK

    def __init__(self, robot, link_name, compliant_frame_pos=(0.0, 0.0, 0.0), compliant_frame_rot=None,
                 controlled_directions_translation=None, controlled_directions_rotation=None,
                 task_name="motion_force_task", is_force_motion_parametrization_in_compliant_frame=False, loop_timestep=0.001):
        super().__init__(robot, task_name, loop_timestep)
        self._compliant_param = bool(is_force_motion_parametrization_in_compliant_frame)
        if is_force_motion_parametrization_in_compliant_frame:
            self._cfg("saip_batch_set_parametrization_in_compliant_frame", 1)
        self.link_name = link_name
        self.pos = np.asarray(compliant_frame_pos, float).reshape(3).copy()
        self.rot = None if compliant_frame_rot is None else np.ascontiguousarray(np.asarray(compliant_frame_rot, float).reshape(9))
        self.partial = controlled_directions_translation is not None or controlled_directions_rotation is not None
        none = np.zeros((0, 3))
        self.dt_ = np.ascontiguousarray(np.asarray(controlled_directions_translation if controlled_directions_translation is not None else none, float).reshape(-1, 3))
        self.dr_ = np.ascontiguousarray(np.asarray(controlled_directions_rotation if controlled_directions_rotation is not None else none, float).reshape(-1, 3))
        if self.partial and len(self.dt_) == 0 and len(self.dr_) == 0:  # MotionForceTask.cpp:47-53
            raise ValueError("controlled_directions_translation and controlled_directions_rotation cannot both be empty "
                             "in MotionForceTask::MotionForceTask")

    def _add(self, L, h):
        tid = C.c_int(-1)
        capi.check(L.saip_batch_add_motion_force_task(
            h, self._name.encode(), self.link_name.encode(), _dptr(self.pos), None if self.rot is None else _dptr(self.rot),
            _dptr(self.dt_) if len(self.dt_) else None, len(self.dt_) if self.partial else -1,
            _dptr(self.dr_) if len(self.dr_) else None, len(self.dr_) if self.partial else -1, self._dt, C.byref(tid)))
        return tid.value

    def _schedule_fields(self):
        return {"position": (0, 3), "orientation": (3, 9), "linear_velocity": (12, 3), "angular_velocity": (15, 3),
                "linear_acceleration": (18, 3), "angular_acceleration": (21, 3), "force": (24, 3), "moment": (27, 3),
                "sensed_force": (30, 3), "sensed_moment": (33, 3)}

    # goals, MotionForceTask.h:211-247
    def setGoalPosition(self, x):
        self._set_field(0, 3, x, "setGoalPosition")

    def setGoalOrientation(self, R):
        R = np.asarray(R, float)
        B = self._need_ctrl().batch_size
        if R.shape == (3, 3):
            R = np.broadcast_to(R, (B, 3, 3))
        self._set_field(3, 9, R.reshape(B, 9), "setGoalOrientation")

    def setGoalLinearVelocity(self, v):
        self._set_field(12, 3, v, "setGoalLinearVelocity")

    def setGoalAngularVelocity(self, w):
        self._set_field(15, 3, w, "setGoalAngularVelocity")

    def setGoalLinearAcceleration(self, a):
        self._set_field(18, 3, a, "setGoalLinearAcceleration")

    def setGoalAngularAcceleration(self, a):
        self._set_field(21, 3, a, "setGoalAngularAcceleration")

    def setGoalForce(self, f):  # MotionForceTask.h setGoalForce / setGoalMoment
        self._set_field(24, 3, f, "setGoalForce")

    def setGoalMoment(self, m):
        self._set_field(27, 3, m, "setGoalMoment")

    def _space(self, fn, dim, axis):
        a = np.ascontiguousarray(np.asarray(axis if axis is not None else (0.0, 0.0, 0.0), float).reshape(3))
        if self._ctrl is None:
            self._log_call(fn, (int(dim), _dptr(a), None), keep=a)
            return None
        ch = C.c_int(0)
        self._ctrl._call(fn, self._id, int(dim), _dptr(a), C.byref(ch))
        self._log_call(fn, (int(dim), _dptr(a), None), keep=a)
        return bool(ch.value)

    def parametrizeForceMotionSpaces(self, force_space_dimension, force_or_motion_single_axis=None):  # MotionForceTask.h:560-580
        self._force_dim = int(force_space_dimension)
        if force_or_motion_single_axis is not None and self._force_dim in (1, 2):
            self._force_axis = np.asarray(force_or_motion_single_axis, float).reshape(3) / np.linalg.norm(force_or_motion_single_axis)
        return self._space("saip_batch_parametrize_force_motion_spaces", force_space_dimension, force_or_motion_single_axis)

    def parametrizeMomentRotMotionSpaces(self, moment_space_dimension, moment_or_rot_motion_single_axis=None):
        self._moment_dim = int(moment_space_dimension)
        if moment_or_rot_motion_single_axis is not None and self._moment_dim in (1, 2):
            self._moment_axis = np.asarray(moment_or_rot_motion_single_axis, float).reshape(3) / np.linalg.norm(moment_or_rot_motion_single_axis)
        return self._space("saip_batch_parametrize_moment_rot_motion_spaces", moment_space_dimension, moment_or_rot_motion_single_axis)

    def setForceControlGains(self, kp, kv, ki=0.0):
        self._force_gains = (float(kp), float(kv), float(ki))
        self._cfg("saip_batch_set_force_control_gains", float(kp), float(kv), float(ki))

    def setMomentControlGains(self, kp, kv, ki=0.0):
        self._moment_gains = (float(kp), float(kv), float(ki))
        self._cfg("saip_batch_set_moment_control_gains", float(kp), float(kv), float(ki))

    def setClosedLoopForceControl(self, enabled: bool):
        self._cfg("saip_batch_set_closed_loop_force_control", int(enabled))

    def setClosedLoopMomentControl(self, enabled: bool):
        self._cfg("saip_batch_set_closed_loop_moment_control", int(enabled))

    def enablePassivity(self):  # MotionForceTask.h:630: POPC passivity observer / controller around the closed-loop force control
        self._cfg("saip_batch_set_passivity", 1)

    def disablePassivity(self):
        self._cfg("saip_batch_set_passivity", 0)

    # -- contact planes and the simulated force sensor of the resident simulator (saip.h)
    @staticmethod
    def _contact_planes(planes, per_instance, B, who, n_planes=None):
        a = np.asarray(planes, float)
        W = capi.SAIP_CONTACT_PLANE_WORDS
        if per_instance:
            if a.ndim != 3 or a.shape[1:] != (B, W) or (n_planes is not None and a.shape[0] != n_planes):
                raise ValueError(f"{who}: per-instance planes of shape ({'P' if n_planes is None else n_planes}, {B}, {W}) expected, got {a.shape}")
            return np.ascontiguousarray(a.transpose(0, 2, 1))
        if a.ndim != 2 or a.shape[1] != W or (n_planes is not None and a.shape[0] != n_planes):
            raise ValueError(f"{who}: planes of shape ({'P' if n_planes is None else n_planes}, {W}) expected, got {a.shape}")
        return np.ascontiguousarray(a)

    def attachContactPlanes(self, planes, point=(0.0, 0.0, 0.0), sensor=True, per_instance=False):
        """give the resident simulator something to touch: one contact point (`point`, in this task's control frame) on this task's body
        against 1..4 world-fixed half-spaces.  planes: (P, 8) rows { n[3], offset, stiffness k, damping c, friction mu, slip speed v_s },
        or (P, B, 8) with per_instance.  While attached, integrate() and rolloutAsync() add the contact force to the torques in front of
        every substep; with `sensor` a rollout period starts by writing the wrench a force sensor would report into this task's sensed
        force / moment (contactSense() does the same for a host-driven loop)."""
        ctrl = self._need_ctrl()
        a = self._contact_planes(planes, per_instance, ctrl.batch_size, "attachContactPlanes")
        rc = np.ascontiguousarray(np.asarray(point, float).reshape(-1))
        if rc.shape != (3,):
            raise ValueError(f"attachContactPlanes: a point of shape (3,) expected, got {rc.shape}")
        ctrl._call("saip_batch_contact_attach", self._id, _dptr(rc), a.shape[0], _dptr(a), int(bool(per_instance)), int(bool(sensor)))

    def _contact_info(self):
        v = [C.c_int(0) for _ in range(4)]
        rc = np.zeros(3)
        ctrl = self._need_ctrl()
        ctrl._call("saip_batch_contact_info", *(C.byref(x) for x in v), _dptr(rc))
        if v[0].value != self._id:
            raise capi.SaipError(f"the contact planes of this controller are attached to task {v[0].value}, not to [{self.getTaskName()}]")
        return dict(task=v[0].value, n_planes=v[1].value, per_instance=bool(v[2].value), sensor=bool(v[3].value), point=rc)

    def contactInfo(self):
        """dict task, n_planes, per_instance, sensor, point"""
        return self._contact_info()

    def detachContactPlanes(self):
        self._contact_info()
        self._need_ctrl()._call("saip_batch_contact_detach")

    def setContactPlanes(self, planes):
        """replace the plane table (same shape as attached); takes effect with the next launch"""
        info = self._contact_info()
        ctrl = self._need_ctrl()
        a = self._contact_planes(planes, info["per_instance"], ctrl.batch_size, "setContactPlanes", info["n_planes"])
        ctrl._call("saip_batch_contact_set_planes_host", _dptr(a))

    def contactPlanesDevice(self):
        """device pointer of the resident plane table, (P, 8) or (P, 8, ld), for domain randomisation on the device; None when detached"""
        return capi.lib().saip_batch_contact_planes_device(self._need_ctrl()._h)

    def contactTorquesDevice(self):
        """device pointer of (dof, ld) commanded + contact torques of the last integrated substep; None when detached"""
        return capi.lib().saip_batch_contact_torques_device(self._need_ctrl()._h)

    def contactReadout(self):
        """dict of the last contact launch: force (B, 3) on the robot in the world frame, point (B, 3), distance (B,) the smallest signed
        distance over the planes, active (B,) the number of planes in contact (waits for the engine stream)"""
        self._contact_info()
        ctrl = self._need_ctrl()
        out = np.empty((capi.SAIP_CONTACT_READOUT_ROWS, ctrl.batch_size))
        ctrl._call("saip_batch_contact_readout_host", _dptr(out))
        return dict(force=out[0:3].T.copy(), point=out[3:6].T.copy(), distance=out[6].copy(), active=out[7].astype(int))

    def contactSummary(self):
        """dict of the running summaries over the integrated substeps: impulse (B,) sum dt * normal force, max_force (B,), max_penetration
        (B,), substeps_in_contact (B,) (waits for the engine stream)"""
        self._contact_info()
        ctrl = self._need_ctrl()
        out = np.empty((capi.SAIP_CONTACT_SUMMARY_ROWS, ctrl.batch_size))
        ctrl._call("saip_batch_contact_summary_host", _dptr(out))
        return dict(impulse=out[0].copy(), max_force=out[1].copy(), max_penetration=out[2].copy(), substeps_in_contact=out[3].astype(int))

    def resetContactSummary(self):
        self._contact_info()
        self._need_ctrl()._call("saip_batch_contact_summary_reset")

    # -- guards: event-triggered phases and goal switching inside rollouts (saip.h)
    _GUARD_SIGNALS = {"periods": capi.SAIP_GUARD_PERIODS, "force": capi.SAIP_GUARD_FORCE, "moment": capi.SAIP_GUARD_MOMENT, "position": capi.SAIP_GUARD_POSITION,
                      "pos_error": capi.SAIP_GUARD_POS_ERROR, "ori_error": capi.SAIP_GUARD_ORI_ERROR, "joint_speed": capi.SAIP_GUARD_JOINT_SPEED}
    _GUARD_AXES = {"x": 0, "y": 1, "z": 2, "norm": 3}
    _GUARD_CMPS = {">=": capi.SAIP_GUARD_GE, "<=": capi.SAIP_GUARD_LE}
    _GUARD_MODES = {"free": capi.SAIP_GUARD_FREE, "hold": capi.SAIP_GUARD_HOLD, "offset": capi.SAIP_GUARD_OFFSET}

    @classmethod
    def _guard_rows(cls, guards, per_instance, B, who):
        """the guard table as the C ABI takes it: (G, 8), or (G, 8, B) per instance.  A guard is a dict from, to, signal (a name or its
        number), axis ('x', 'y', 'z', 'norm' or a number; default 0), cmp ('>=' or '<='), threshold, hold (default 1), blank (default 0);
        with per_instance any value may be a (B,) array."""
        guards = list(guards)
        out = np.zeros((len(guards), capi.SAIP_GUARD_WORDS, B if per_instance else 1))
        for g, d in enumerate(guards):
            unknown = set(d) - {"from", "to", "signal", "axis", "cmp", "threshold", "hold", "blank"}
            if unknown:
                raise ValueError(f"{who}: guard {g}: unknown keys {sorted(unknown)}")
            for key in ("from", "to", "signal", "threshold"):
                if key not in d:
                    raise ValueError(f"{who}: guard {g}: key [{key}] is missing")
            sig, axis, cmp = d["signal"], d.get("axis", 0), d.get("cmp", ">=")
            for name, val, table in (("signal", sig, cls._GUARD_SIGNALS), ("axis", axis, cls._GUARD_AXES), ("cmp", cmp, cls._GUARD_CMPS)):
                if isinstance(val, str) and val not in table:
                    raise ValueError(f"{who}: guard {g}: unknown {name} {val!r} (one of {sorted(table)})")
            words = (d["from"], d["to"], cls._GUARD_SIGNALS.get(sig, sig) if isinstance(sig, str) else sig, cls._GUARD_AXES.get(axis, axis) if isinstance(axis, str) else axis,
                     cls._GUARD_CMPS.get(cmp, cmp) if isinstance(cmp, str) else cmp, d["threshold"], d.get("hold", 1), d.get("blank", 0))
            for k, w in enumerate(words):
                w = np.asarray(w, float)
                if w.ndim and not (per_instance and w.shape == (B,)):
                    raise ValueError(f"{who}: guard {g}: a scalar{' or a (%d,) array' % B if per_instance else ''} expected for word {k}, got shape {w.shape}")
                out[g, k, :] = w
        return np.ascontiguousarray(out if per_instance else out[:, :, 0])

    def attachGuards(self, guards, phases, per_instance=False):
        """make the rollout closed loop in time: every instance carries a phase, `guards` move it on what the instance senses, `phases`
        say what a phase does to this task's goal.  guards: 1..8 dicts (see _guard_rows), e.g. dict(**{'from': 0}, to=1, signal='force',
        axis='norm', cmp='>=', threshold=5.0, hold=2); phases: 1..8 dicts mode ('free', 'hold', 'offset') and, for 'offset', offset (3,)
        in the world frame.  Phase 0 must be 'free'.  A 'hold' phase keeps the pose latched at the transition into it, 'offset' that pose
        moved by the offset.  rolloutAsync() evaluates the guards in every period in front of the OTG step and the cycle;
        ctrl.evaluateGuards() does the same for a host-driven loop."""
        ctrl = self._need_ctrl()
        a = self._guard_rows(guards, per_instance, ctrl.batch_size, "attachGuards")
        phases = list(phases)
        ph = np.zeros((len(phases), capi.SAIP_GUARD_PHASE_WORDS))
        for p, d in enumerate(phases):
            mode = d.get("mode", "free")
            if isinstance(mode, str) and mode not in self._GUARD_MODES:
                raise ValueError(f"attachGuards: phase {p}: unknown mode {mode!r} (one of {sorted(self._GUARD_MODES)})")
            ph[p, 0] = self._GUARD_MODES[mode] if isinstance(mode, str) else mode
            off = np.asarray(d.get("offset", (0.0, 0.0, 0.0)), float).reshape(-1)
            if off.shape != (3,):
                raise ValueError(f"attachGuards: phase {p}: an offset of shape (3,) expected, got {off.shape}")
            ph[p, 1:] = off
        ctrl._call("saip_batch_guard_attach", self._id, a.shape[0], _dptr(a), int(bool(per_instance)), ph.shape[0], _dptr(ph))

    def detachGuards(self):
        ctrl = self._need_ctrl()
        info = ctrl.guardInfo()
        if info["task"] != self._id:
            raise capi.SaipError(f"the guards of this controller are attached to task {info['task']}, not to [{self.getTaskName()}]")
        ctrl._call("saip_batch_guard_detach")

    def setGuards(self, guards):
        """replace the guard table (as many guards as attached); phases, counters and latches stay"""
        ctrl = self._need_ctrl()
        info = ctrl.guardInfo()
        a = self._guard_rows(guards, info["per_instance"], ctrl.batch_size, "setGuards")
        if a.shape[0] != info["n_guards"]:
            raise ValueError(f"setGuards: {info['n_guards']} guards expected, got {a.shape[0]}")
        ctrl._call("saip_batch_guard_set_guards_host", _dptr(a))

    # -- contact patches: up to eight contact points on this task's body, net force and moment, a wrench sensor (saip.h)
    def attachContactPatch(self, points, planes, sensor=True, per_instance=False):
        """multi-point contact: `points` (n, 3), 1..8 offsets in this task's control frame, against the patch's own 1..4 planes (format of
        attachContactPlanes: (P, 8), or (P, B, 8) with per_instance).  While attached, integrate() and rolloutAsync() add the net contact
        torques in front of every substep; with `sensor` a rollout period starts by writing the sensed force AND moment of the patch
        (contactPatchSense() does the same for a host-driven loop).  Up to two patches per controller, on different tasks; never
        together with attachContactPlanes."""
        ctrl = self._need_ctrl()
        a = self._contact_planes(planes, per_instance, ctrl.batch_size, "attachContactPatch")
        pts = np.ascontiguousarray(np.asarray(points, float))
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError(f"attachContactPatch: points of shape (n, 3) expected, got {pts.shape}")
        ctrl._call("saip_batch_contact_patch_attach", self._id, pts.shape[0], _dptr(pts), a.shape[0], _dptr(a), int(bool(per_instance)), int(bool(sensor)))

    def contactPatchInfo(self):
        """dict n_patches (of the controller), n_points, n_planes, per_instance, sensor, points (n, 3)"""
        v = [C.c_int(0) for _ in range(5)]
        pts = np.zeros((capi.SAIP_CONTACT_PATCH_MAX_POINTS, 3))
        self._need_ctrl()._call("saip_batch_contact_patch_info", self._id, *(C.byref(x) for x in v), _dptr(pts))
        return dict(n_patches=v[0].value, n_points=v[1].value, n_planes=v[2].value, per_instance=bool(v[3].value), sensor=bool(v[4].value),
                    points=pts[:v[1].value].copy())

    def detachContactPatch(self):
        self._need_ctrl()._call("saip_batch_contact_patch_detach", self._id)

    def setContactPatchPlanes(self, planes):
        """replace the plane table of this task's patch (same shape as attached); takes effect with the next launch"""
        info = self.contactPatchInfo()
        ctrl = self._need_ctrl()
        a = self._contact_planes(planes, info["per_instance"], ctrl.batch_size, "setContactPatchPlanes", info["n_planes"])
        ctrl._call("saip_batch_contact_patch_set_planes_host", self._id, _dptr(a))

    def contactPatchPlanesDevice(self):
        """device pointer of the patch's resident plane table, (P, 8) or (P, 8, ld); None without a patch"""
        return capi.lib().saip_batch_contact_patch_planes_device(self._need_ctrl()._h, self._id)

    def contactPatchReadoutDevice(self):
        """device pointer of the patch's readout (20, ld); None without a patch"""
        return capi.lib().saip_batch_contact_patch_readout_device(self._need_ctrl()._h, self._id)

    def contactPatchSummaryDevice(self):
        """device pointer of the patch's summaries (6, ld); None without a patch"""
        return capi.lib().saip_batch_contact_patch_summary_device(self._need_ctrl()._h, self._id)

    def contactPatchTorquesDevice(self):
        """device pointer of (dof, ld) commanded + contact torques of the last integrated substep (shared by the patches); None without one"""
        return capi.lib().saip_batch_contact_patch_torques_device(self._need_ctrl()._h)

    def contactPatchReadout(self):
        """dict of the last launch that evaluated this patch: force (B, 3) and moment (B, 3) about the control point on the robot, world
        frame; distance (B,) the smallest signed distance over the points; n_touch (B,) points in contact; deepest (B,) the index of the
        deepest point; control_point (B, 3); normal_forces (B, 8) per point slot (waits for the engine stream)"""
        ctrl = self._need_ctrl()
        out = np.empty((capi.SAIP_CONTACT_PATCH_READOUT_ROWS, ctrl.batch_size))
        ctrl._call("saip_batch_contact_patch_readout_host", self._id, _dptr(out))
        return dict(force=out[0:3].T.copy(), moment=out[3:6].T.copy(), distance=out[6].copy(), n_touch=out[7].astype(int), deepest=out[8].astype(int),
                    control_point=out[9:12].T.copy(), normal_forces=out[12:20].T.copy())

    def contactPatchSummary(self):
        """dict of the running summaries over the integrated substeps: impulse, max_force, max_penetration, substeps_in_contact, max_moment,
        substeps_in_full_contact, each (B,) (waits for the engine stream)"""
        ctrl = self._need_ctrl()
        out = np.empty((capi.SAIP_CONTACT_PATCH_SUMMARY_ROWS, ctrl.batch_size))
        ctrl._call("saip_batch_contact_patch_summary_host", self._id, _dptr(out))
        return dict(impulse=out[0].copy(), max_force=out[1].copy(), max_penetration=out[2].copy(), substeps_in_contact=out[3].astype(int),
                    max_moment=out[4].copy(), substeps_in_full_contact=out[5].astype(int))

    def resetContactPatchSummary(self):
        """zero this patch's summaries on the stream (what goes with a snapshot restore: the summaries are not part of a snapshot)"""
        self._need_ctrl()._call("saip_batch_contact_patch_summary_reset", self._id)

    # -- environment schedule of this task's contact surfaces: planes that move inside rollouts (saip.h)
    def _contact_target(self, who):
        """(target, per_instance) of whichever of contact planes or contact patch this task has"""
        ctrl = self._need_ctrl()
        L, v = capi.lib(), [C.c_int(0) for _ in range(5)]
        if L.saip_batch_contact_info(ctrl._h, C.byref(v[0]), None, C.byref(v[2]), None, None) == capi.SAIP_OK and v[0].value == self._id:
            return capi.SAIP_ENV_TARGET_PLANES, bool(v[2].value)
        if L.saip_batch_contact_patch_info(ctrl._h, self._id, None, None, None, C.byref(v[3]), None, None) == capi.SAIP_OK:
            return capi.SAIP_ENV_TARGET_PATCH, bool(v[3].value)
        raise capi.SaipError(f"{who}: task [{self.getTaskName()}] has neither contact planes nor a contact patch")

    def setContactSchedule(self, keyframes, stride=1, mode="hold", first=0):
        """let the planes of this task's contact planes or contact patch move during rollouts.  keyframes: (K, n, 12), or (K, n, B, 12) when
        the planes are per instance, rows { n[3], offset, k, c, mu, v_s, u[3], 0 }: the eight plane words and the velocity u of the
        surface in the base frame (a conveyor).  Period c of a rollout uses keyframe c // stride ("hold") or goes from it towards the next
        by (c % stride) / stride ("linear"); the last keyframe is held.  The schedule covers planes first .. first + n - 1.  In "linear"
        a moving offset gives the surface its normal velocity; damping and friction act on the velocity relative to the surface."""
        ctrl = self._need_ctrl()
        target, per = self._contact_target("setContactSchedule")
        ctrl._env_schedule_attach("setContactSchedule", target, self._id, keyframes, capi.SAIP_ENV_PLANE_WORDS, per, stride, mode, first)

    def clearContactSchedule(self):
        """detach the schedule; the planes keep the values written last"""
        target, _ = self._contact_target("clearContactSchedule")
        self._need_ctrl()._call("saip_batch_env_schedule_detach", target, self._id)

    def contactScheduleInfo(self):
        """dict first, n_items, n_keyframes, stride, mode, per_instance, period"""
        target, _ = self._contact_target("contactScheduleInfo")
        return self._need_ctrl()._env_schedule_info(target, self._id)

    def contactVelocityDevice(self):
        """device pointer of the surface velocities the schedule writes, (P, 4) or (P, 4, ld) rows { v_p[3], w_n }; None without a schedule"""
        target, _ = self._contact_target("contactVelocityDevice")
        return capi.lib().saip_batch_env_schedule_velocity_device(self._need_ctrl()._h, target, self._id)

    def updateSensedForceAndMoment(self, sensed_force_sensor_frame, sensed_moment_sensor_frame):  # MotionForceTask.cpp:805-828
        self._set_field(30, 3, sensed_force_sensor_frame, "updateSensedForceAndMoment (force)")
        self._set_field(33, 3, sensed_moment_sensor_frame, "updateSensedForceAndMoment (moment)")

    def setForceControlParameters(self, kff_force=0.95, kff_moment=0.95, max_force_feedback=20.0, max_moment_feedback=10.0):
        """setFeedforwardForceGain / MomentGain, setMaxForceControlFeedbackOutput / Moment (MotionForceTask.h:330-355)"""
        self._force_params = dict(kff_force=float(kff_force), kff_moment=float(kff_moment), max_force_feedback=float(max_force_feedback),
                                  max_moment_feedback=float(max_moment_feedback))
        self._cfg("saip_batch_set_force_control_parameters", float(kff_force), float(kff_moment), float(max_force_feedback), float(max_moment_feedback))

    def setControlToSensorTransform(self, R, p):
        """_T_control_to_sensor of setForceSensorFrame (MotionForceTask.cpp:802): rotation (3,3) and translation (3,)"""
        R, p = np.ascontiguousarray(np.asarray(R, float).reshape(9)), np.ascontiguousarray(np.asarray(p, float).reshape(3))
        self._cfg("saip_batch_set_control_to_sensor_transform", _dptr(R), _dptr(p), keep=(R, p))

    # remaining MotionForceTask.h surface: aliases, host-side getters of what was configured, integrator resets
    def setPosControlGainsUnsafe(self, kp, kv, ki=0.0):  # MotionForceTask.h: same as the checked setter (the engine validates itself)
        self.setPosControlGains(kp, kv, ki)

    def setOriControlGainsUnsafe(self, kp, kv, ki=0.0):
        self.setOriControlGains(kp, kv, ki)

    def getPosControlGains(self):
        """list of PIDGains (one entry for isotropic gains), defaults MotionForceTask.h:40-45"""
        return self._cached_gains("saip_batch_set_pos_control_gains", [(100.0, 20.0, 0.0)])

    def getOriControlGains(self):
        return self._cached_gains("saip_batch_set_ori_control_gains", [(200.0, 28.3, 0.0)])

    def getForceControlGains(self):
        return PIDGains(*getattr(self, "_force_gains", (0.7, 10.0, 1.3)))  # MotionForceTask.h:50-52

    def getMomentControlGains(self):
        return PIDGains(*getattr(self, "_moment_gains", (0.7, 10.0, 1.3)))

    def getForceSpaceDimension(self):
        return getattr(self, "_force_dim", 0)

    def getMomentSpaceDimension(self):
        return getattr(self, "_moment_dim", 0)

    def getVelocitySaturationEnabled(self):
        return getattr(self, "_vel_sat", False)

    def getLinearSaturationVelocity(self):
        return getattr(self, "_sat_vel", (0.3, np.pi / 3))[0]  # MotionForceTask.h:64-65

    def getAngularSaturationVelocity(self):
        return getattr(self, "_sat_vel", (0.3, np.pi / 3))[1]

    def getBoundedInertiaEstimateThreshold(self):
        return getattr(self, "_bie_threshold", 0.1)

    def _fcp(self, **kw):
        cur = dict(kff_force=0.95, kff_moment=0.95, max_force_feedback=20.0, max_moment_feedback=10.0)
        cur.update(getattr(self, "_force_params", {}))
        cur.update(kw)
        self.setForceControlParameters(**cur)

    def setFeedforwardForceGain(self, k):  # MotionForceTask.h:330-355
        self._fcp(kff_force=float(k))

    def setFeedforwardmomentGain(self, k):
        self._fcp(kff_moment=float(k))

    def setMaxForceControlFeedbackOutput(self, v):
        self._fcp(max_force_feedback=float(v))

    def setMaxMomentControlFeedbackOutput(self, v):
        self._fcp(max_moment_feedback=float(v))

    def getFeedforwardForceGain(self):
        return getattr(self, "_force_params", {}).get("kff_force", 0.95)

    def getFeedforwardmomentGain(self):
        return getattr(self, "_force_params", {}).get("kff_moment", 0.95)

    def getMaxForceControlFeedbackOutput(self):
        return getattr(self, "_force_params", {}).get("max_force_feedback", 20.0)

    def getMaxMomentControlFeedbackOutput(self):
        return getattr(self, "_force_params", {}).get("max_moment_feedback", 10.0)

    def resetIntegrators(self):  # MotionForceTask.cpp:988-1002
        self._need_ctrl()._call("saip_batch_reset_integrators", self._id, 3)

    def _current_pose(self):
        ctrl = self._need_ctrl()
        ctrl._push_state()
        B = ctrl._robot.batch_size
        pos, rot = np.empty((3, B)), np.empty((9, B))
        capi.check(capi.lib().saip_batch_get_current_pose_host(ctrl._h, self._id, _dptr(pos), _dptr(rot)))
        return pos.T.copy(), rot.T.reshape(B, 3, 3).copy()

    def getCurrentPosition(self):
        """(B, 3) control point in the world frame at the robot's current state, MotionForceTask.h:121"""
        return self._current_pose()[0]

    def getCurrentOrientation(self):
        """(B, 3, 3) compliant-frame orientation in the world frame, MotionForceTask.h:136"""
        return self._current_pose()[1]

    # task-space diagnostics (one kernel launch for all seven quantities; C-ABI saip_batch_get_task_diagnostics_host)
    _DIAG_ROWS = {"position_error": (0, 3), "orientation_error": (3, 6), "linear_velocity": (6, 9), "angular_velocity": (9, 12),
                  "sensed_force": (12, 15), "sensed_moment": (15, 18), "unit_mass_force": (18, 24)}

    def getTaskDiagnostics(self):
        """dict of (B, 3) / (B, 6) arrays at the robot's current state: position_error, orientation_error, linear_velocity, angular_velocity,
        sensed_force, sensed_moment (control point, world frame) and unit_mass_force -- what the getters below return, from one launch.
        unit_mass_force is the control law evaluated at that state (see saip.h); no task state is changed."""
        ctrl = self._need_ctrl()
        ctrl._push_state()
        out = np.empty((24, ctrl._robot.batch_size))
        capi.check(capi.lib().saip_batch_get_task_diagnostics_host(ctrl._h, self._id, _dptr(out)))
        return {k: out[a:b].T.copy() for k, (a, b) in self._DIAG_ROWS.items()}

    def getTaskDiagnosticsDevice(self, out):
        """asynchronous variant on the batch stream: writes the 24 rows into device memory of shape (24, ld), ld = the batch's leading
        dimension (row r, instance b at r * ld + b): `out` is a contiguous float64 device tensor of that shape or a raw device pointer (int)"""
        ctrl = self._need_ctrl()
        ctrl._push_state()
        ld = capi.lib().saip_batch_ld(ctrl._h)
        if isinstance(out, int):
            ptr = out
        else:
            if tuple(out.shape) != (24, ld) or not out.is_contiguous() or str(out.dtype) != "torch.float64":
                raise ValueError(f"getTaskDiagnosticsDevice: expected a contiguous float64 tensor of shape (24, {ld})")
            ptr = out.data_ptr()
        capi.check(capi.lib().saip_batch_task_diagnostics_device(ctrl._h, self._id, C.c_void_p(ptr)))
        return out

    def getPositionError(self):
        """(B, 3) sigmaPosition (goal - current position), MotionForceTask.cpp:540-542"""
        return self.getTaskDiagnostics()["position_error"]

    def getOrientationError(self):
        """(B, 3) sigmaOrientation orientationError(goal, current), MotionForceTask.cpp:544-546"""
        return self.getTaskDiagnostics()["orientation_error"]

    def getCurrentLinearVelocity(self):
        """(B, 3) rows 0-2 of (P J) dq, MotionForceTask.cpp:293-295"""
        return self.getTaskDiagnostics()["linear_velocity"]

    def getCurrentAngularVelocity(self):
        """(B, 3) rows 3-5 of (P J) dq, MotionForceTask.cpp:296-298"""
        return self.getTaskDiagnostics()["angular_velocity"]

    def getSensedForceControlWorldFrame(self):
        """(B, 3) sensed force at the control point in the world frame, MotionForceTask.cpp:805-828"""
        return self.getTaskDiagnostics()["sensed_force"]

    def getSensedMomentControlWorldFrame(self):
        """(B, 3) sensed moment at the control point in the world frame, MotionForceTask.cpp:805-828"""
        return self.getTaskDiagnostics()["sensed_moment"]

    def getUnitMassForce(self):
        """(B, 6) position / orientation term of the control law (MotionForceTask.h:266) evaluated at the current state"""
        return self.getTaskDiagnostics()["unit_mass_force"]

    def _sigma(self, dim, axis, sel, R):
        """sigmaPosition / sigmaOrientation, MotionForceTask.cpp:892-971: sel (I - sigma_force) sel^T with the force (moment) space given
        by `dim` and `axis`, in the compliant frame when the task is parametrised there"""
        B = R.shape[0]
        I = np.broadcast_to(np.eye(3), (B, 3, 3))
        if dim == 0:
            core = np.zeros((B, 3, 3))
        elif dim == 3:
            core = I
        else:
            a = (R @ axis) if self._compliant_param else np.broadcast_to(axis, (B, 3))
            aa = np.einsum("bi,bj->bij", a, a)
            core = aa if dim == 1 else I - aa
        sf = sel @ core @ sel.T if dim in (1, 2) else (sel if dim == 3 else core)
        return sel @ (I - sf) @ sel.T

    def goalPositionReached(self, tolerance, verbose=False):
        """(B,) bool: sqrt(e^T sigmaPosition e) < tolerance with e = goal - current position, MotionForceTask.cpp:548-563"""
        pos, R = self._current_pose()
        e = self.getGoalPosition() - pos
        S = self._sigma(getattr(self, "_force_dim", 0), getattr(self, "_force_axis", np.array([0.0, 0.0, 1.0])), self.getTaskProjection()[0][:3, :3], R)
        err = np.sqrt(np.maximum(np.einsum("bi,bij,bj->b", e, S, e), 0.0))
        if verbose:
            print("position error in MotionForceTask :", err, "\nTolerance :", tolerance)
        return err < tolerance

    def goalOrientationReached(self, tolerance, verbose=False):
        """(B,) bool: sqrt(dphi^T sigmaOrientation dphi) < tolerance, dphi = orientationError(goal, current), MotionForceTask.cpp:565-579"""
        _, R = self._current_pose()
        Rd = self.getGoalOrientation()
        dphi = -0.5 * sum(np.cross(R[:, :, c], Rd[:, :, c]) for c in range(3))
        S = self._sigma(getattr(self, "_moment_dim", 0), getattr(self, "_moment_axis", np.array([0.0, 0.0, 1.0])), self.getTaskProjection()[0][3:, 3:], R)
        err = np.sqrt(np.maximum(np.einsum("bi,bij,bj->b", dphi, S, dphi), 0.0))
        if verbose:
            print("orientation error in MotionForceTask :", err, "\nTolerance :", tolerance)
        return err < tolerance

    def resetIntegratorsLinear(self):
        self._need_ctrl()._call("saip_batch_reset_integrators", self._id, 1)

    def resetIntegratorsAngular(self):
        self._need_ctrl()._call("saip_batch_reset_integrators", self._id, 2)

    def getGoalPosition(self):
        return self._get_goal()[:, 0:3]

    def getGoalOrientation(self):
        return self._get_goal()[:, 3:12].reshape(-1, 3, 3)

    # internal Cartesian OTG (OTG_6dof_cartesian), acceleration-limited mode on the device.  MotionForceTask.h:387-423
    def enableInternalOtgAccelerationLimited(self, max_linear_velocity=0.3, max_linear_acceleration=2.0,
                                             max_angular_velocity=np.pi / 3, max_angular_acceleration=2 * np.pi):
        v = np.ascontiguousarray([float(max_linear_velocity), float(max_angular_velocity)])
        a = np.ascontiguousarray([float(max_linear_acceleration), float(max_angular_acceleration)])
        _check_otg_limits("OTG_6dof_cartesian", velocity=v, acceleration=a)
        self._cfg("saip_batch_set_otg_acceleration_limited", _dptr(v), _dptr(a), 2, keep=(v, a))
        self._otg_enabled = True

    def enableInternalOtgJerkLimited(self, max_linear_velocity=0.3, max_linear_acceleration=2.0, max_linear_jerk=10.0,
                                     max_angular_velocity=np.pi / 3, max_angular_acceleration=2 * np.pi, max_angular_jerk=10 * np.pi):
        """MotionForceTask.h:416-421 / MotionForceTask.cpp:525-545 (defaults: MotionForceTask.h:68-73)"""
        v = np.ascontiguousarray([float(max_linear_velocity), float(max_angular_velocity)])
        a = np.ascontiguousarray([float(max_linear_acceleration), float(max_angular_acceleration)])
        j = np.ascontiguousarray([float(max_linear_jerk), float(max_angular_jerk)])
        _check_otg_limits("OTG_6dof_cartesian", velocity=v, acceleration=a, jerk=j)
        self._cfg("saip_batch_set_otg_jerk_limited", _dptr(v), _dptr(a), _dptr(j), 2, keep=(v, a, j))
        self._otg_enabled = True

    # desired state = OTG output when enabled, else the goal (MotionForceTask.h getDesired*)
    def getDesiredPosition(self):
        return self._desired_block()[:, 0:3]

    def getDesiredOrientation(self):
        return self._desired_block()[:, 3:12].reshape(-1, 3, 3)

    def getDesiredLinearVelocity(self):
        return self._desired_block()[:, 12:15]

    def getDesiredAngularVelocity(self):
        return self._desired_block()[:, 15:18]

    def getDesiredLinearAcceleration(self):
        return self._desired_block()[:, 18:21]

    def getDesiredAngularAcceleration(self):
        return self._desired_block()[:, 21:24]

    # gains, MotionForceTask.h:272-300
    def setPosControlGains(self, kp, kv, ki=0.0):
        self._gains("saip_batch_set_pos_control_gains", kp, kv, ki)

    def setOriControlGains(self, kp, kv, ki=0.0):
        self._gains("saip_batch_set_ori_control_gains", kp, kv, ki)

    def enableSingularityHandling(self):  # MotionForceTask.h:715-725
        self._cfg("saip_batch_set_singularity_handling", 1)

    def disableSingularityHandling(self):
        """near-singular instances then use the non-singular part of the task only (status 2) instead of being flagged (status 1)"""
        self._cfg("saip_batch_set_singularity_handling", 0)

    def setSingularityStrategies(self, enabled=True):
        """blended type-1 / type-2 strategies of SingularityHandler for instances inside the singularity bounds (status bit 8): ON by default
        like in the reference; off (an engine extra): such instances are flagged (status 1) instead"""
        self._cfg("saip_batch_set_singularity_strategies", int(bool(enabled)))

    def setSingularityHandlingGains(self, kp_type_1, kv_type_1, kv_type_2):  # MotionForceTask.h:749
        self._cfg("saip_batch_set_singularity_gains", float(kp_type_1), float(kv_type_1), float(kv_type_2))

    def handleAllSingularitiesAsType1(self, flag):  # MotionForceTask.h:698
        self._cfg("saip_batch_set_all_singularities_type1", int(bool(flag)))

    def setType1Posture(self, q_des):  # MotionForceTask.h:707; (dof,) for every instance or (B, dof)
        q = np.ascontiguousarray(q_des, dtype=np.float64)
        self._cfg("saip_batch_set_type1_posture", q.ctypes.data_as(C.POINTER(C.c_double)), int(q.ndim == 2))

    def setSingularityHandlingBounds(self, s_min, s_max):  # MotionForceTask.h:736
        self._cfg("saip_batch_set_singularity_bounds", float(s_min), float(s_max))

    def getTaskProjection(self):
        ctrl = self._need_ctrl()
        P, Bm, k = np.zeros(36), np.zeros(36), C.c_int(0)
        capi.check(capi.lib().saip_batch_get_task_projection(ctrl._h, self._id, _dptr(P), _dptr(Bm), C.byref(k)))
        return P.reshape(6, 6), Bm.reshape(6, 6)[:, :k.value].copy()


class JointTask(_Task):
    """JointTask.h:56-75.  joint_selection_matrix = None -> full joint task."""
    _type = TaskType.JOINT_TASK

    def __init__(self, robot, joint_selection_matrix=None, task_name="joint_task", loop_timestep=0.001):
        super().__init__(robot, task_name, loop_timestep)
        self.S = None
        if joint_selection_matrix is not None:
            S = np.ascontiguousarray(np.asarray(joint_selection_matrix, float))
            if S.ndim != 2 or S.shape[1] != robot.dof():  # JointTask.cpp:28-32
                raise ValueError("joint selection matrix size not consistent with robot dof in JointTask constructor")
            self.S = S

    def _add(self, L, h):
        tid = C.c_int(-1)
        if self.S is None:
            capi.check(L.saip_batch_add_joint_task(h, self._name.encode(), None, 0, self._dt, C.byref(tid)))
        else:
            capi.check(L.saip_batch_add_joint_task(h, self._name.encode(), _dptr(self.S), self.S.shape[0], self._dt, C.byref(tid)))
        return tid.value

    def getTaskDof(self):
        return self._robot.dof() if self.S is None else self.S.shape[0]

    def isFullJointTask(self):
        return self.getTaskDof() == self._robot.dof()

    def _schedule_fields(self):
        m = self.getTaskDof()
        return {"position": (0, m), "velocity": (m, m), "acceleration": (2 * m, m)}

    # goals, JointTask.h:140-175
    def setGoalPosition(self, q):
        self._set_field(0, self.getTaskDof(), q, "goal position vector size not consistent with task dof in JointTask::setGoalPosition")

    def setGoalVelocity(self, dq):
        m = self.getTaskDof()
        self._set_field(m, m, dq, "goal velocity vector size not consistent with task dof in JointTask::setGoalVelocity")

    def setGoalAcceleration(self, ddq):
        m = self.getTaskDof()
        self._set_field(2 * m, m, ddq, "goal acceleration vector size not consistent with task dof in JointTask::setGoalAcceleration")

    def getGoalPosition(self):
        return self._get_goal()[:, :self.getTaskDof()]

    def setGains(self, kp, kv, ki=0.0):  # JointTask.h:237-257
        self._gains("saip_batch_set_joint_gains", kp, kv, ki)

    def setGainsUnsafe(self, kp, kv, ki=0.0):  # same as the checked setter (the engine validates itself)
        self.setGains(kp, kv, ki)

    def getGains(self):
        """list of PIDGains (one entry for isotropic gains), defaults JointTask.h:31-33"""
        return self._cached_gains("saip_batch_set_joint_gains", [(50.0, 14.0, 0.0)])

    def getJointSelectionMatrix(self):
        return np.eye(self._robot.dof()) if self.S is None else self.S.reshape(self.getTaskDof(), self._robot.dof()).copy()

    def getCurrentPosition(self):
        """S q of the robot's current state, (B, task dof)"""
        return self._robot._q @ self.getJointSelectionMatrix().T

    def getCurrentVelocity(self):
        return self._robot._dq @ self.getJointSelectionMatrix().T

    def getGoalVelocity(self):
        m = self.getTaskDof()
        return self._get_goal()[:, m:2 * m]

    def getGoalAcceleration(self):
        m = self.getTaskDof()
        return self._get_goal()[:, 2 * m:3 * m]

    def getVelocitySaturationEnabled(self):
        return getattr(self, "_vel_sat", False)

    def goalPositionReached(self, tol):
        """(B,) bool: sqrt(e^T U U^T e) < tol with e = current - goal and U = matrixRangeBasis(S N_prec) (JointTask.cpp:437-446; tolerance
        1e-3 as JointTask.cpp:233); N_prec comes from the device, the small SVDs run on the host"""
        e = self.getCurrentPosition() - self.getGoalPosition()
        Jp = self.getJointSelectionMatrix()[None] @ self.getPreviousTasksNullspace()
        out = np.zeros(e.shape[0], bool)
        for b in range(e.shape[0]):
            U, sv, _ = np.linalg.svd(Jp[b], full_matrices=False)
            keep = (sv >= 1e-3 * sv[0]) if sv[0] >= 1e-3 and np.linalg.norm(Jp[b]) >= 1e-3 else np.zeros(len(sv), bool)
            c = U[:, keep].T @ e[b]
            out[b] = np.sqrt(c @ c) < tol
        return out

    def getVelocitySaturationMaxVelocity(self):
        v = np.asarray(getattr(self, "_sat_vel", (np.pi / 3,)), float)  # JointTask.h:44
        return np.broadcast_to(v, (self.getTaskDof(),)).copy() if v.shape[0] in (1, self.getTaskDof()) else v

    def getBoundedInertiaEstimateThreshold(self):
        return getattr(self, "_bie_threshold", 0.1)

    def resetIntegrators(self):
        self._need_ctrl()._call("saip_batch_reset_integrators", self._id, 1)

    # internal OTG, JointTask.h:272-327.  Acceleration-limited mode (the reference default) runs on the device.
    def enableInternalOtgAccelerationLimited(self, max_velocity=np.pi / 3.0, max_acceleration=2.0 * np.pi):
        v, a = np.atleast_1d(np.asarray(max_velocity, float)), np.atleast_1d(np.asarray(max_acceleration, float))
        m = self.getTaskDof()
        if v.shape != a.shape or v.ndim != 1 or v.shape[0] not in (1, m):  # JointTask.cpp:367-373
            raise ValueError("max velocity or max acceleration vector size not consistent with task dof in JointTask::enableInternalOtgAccelerationLimited")
        v, a = np.ascontiguousarray(v), np.ascontiguousarray(a)
        _check_otg_limits("OTG_joints", velocity=v, acceleration=a)
        self._cfg("saip_batch_set_otg_acceleration_limited", _dptr(v), _dptr(a), int(v.shape[0]), keep=(v, a))
        self._otg_enabled = True

    def enableInternalOtgJerkLimited(self, max_velocity, max_acceleration, max_jerk):
        """JointTask.h:298-316 / JointTask.cpp:383-410: third-order (jerk-limited) Ruckig profiles; scalars or one value per task dof.  The OTG
        is re-initialised at the current task position when it was off or acceleration-limited (the engine does so at the next cycle)"""
        v, a, j = (np.ascontiguousarray(np.atleast_1d(np.asarray(x, float))) for x in (max_velocity, max_acceleration, max_jerk))
        if not (v.shape == a.shape == j.shape) or v.shape[0] not in (1, self.getTaskDof()):
            raise ValueError("max velocity, max acceleration or max jerk vector size not consistent with task dof in JointTask::enableInternalOtgJerkLimited")
        _check_otg_limits("OTG_joints", velocity=v, acceleration=a, jerk=j)
        self._cfg("saip_batch_set_otg_jerk_limited", _dptr(v), _dptr(a), _dptr(j), int(v.shape[0]), keep=(v, a, j))
        self._otg_enabled = True

    def getDesiredPosition(self):  # JointTask.h:185-200: the OTG output when enabled, else the goal
        return self._desired_block()[:, :self.getTaskDof()]

    def getDesiredVelocity(self):
        m = self.getTaskDof()
        return self._desired_block()[:, m:2 * m]

    def getDesiredAcceleration(self):
        m = self.getTaskDof()
        return self._desired_block()[:, 2 * m:]


class RobotController:
    """RobotController.h:47-90 for B robots at once."""

    def __init__(self, robot: SaiModel, tasks, _private=False, leading_dimension=None, _adopt=None):
        """leading_dimension (engine extra): the leading dimension of the device arrays when it must be larger than the batch rounded up
        to 32 -- the shards of a sharded run all take the largest shard's, so that the final all-gather moves slabs of one shape.
        _adopt: an unfinalized batch handle owned by somebody else (saip_multi_batch of sharding.MultiController): tasks are added here, the
        owner finalizes all its batches together and then calls _after_finalize(); the handle is not destroyed by this object."""
        L = capi.lib()
        if len(tasks) == 0:  # RobotController.cpp:11-14
            raise ValueError("RobotController must have at least one task")
        for t in tasks:
            if t.getConstRobotModel() is not robot:  # :28-31
                raise ValueError("All tasks must have the same robot model in RobotController")
        for t in tasks:
            if t._ctrl is not None and not t._ctrl._private:
                raise ValueError(f"task [{t.getTaskName()}] already belongs to a RobotController")
        self._owns = _adopt is None
        if self._owns:
            h = C.c_void_p()
            capi.check(L.saip_batch_create(robot._h, robot.batch_size, robot.device, C.byref(h)))
        else:
            h = C.c_void_p(_adopt)
        if leading_dimension is not None:
            try:
                capi.check(L.saip_batch_set_leading_dimension(h, int(leading_dimension)))
            except Exception:
                if self._owns:
                    L.saip_batch_destroy(h)
                raise
        self._h = h
        self._robot = robot
        self.batch_size = robot.batch_size
        self._tasks = list(tasks)
        self._private = bool(_private)  # the one-task batch of a task driven by hand (TemplateTask.h:43-60), not a user-visible controller
        try:
            for t in tasks:
                t._id = t._add(L, h)
            if self._owns:
                capi.check(L.saip_batch_finalize(h))  # remaining constructor checks, :32-58
        except Exception:
            if self._owns:
                L.saip_batch_destroy(h)
            self._h = None
            raise
        if self._owns:
            self._after_finalize()

    def _after_finalize(self):
        """the part of the constructor behind saip_batch_finalize: the tasks' logged configuration is replayed into the batch"""
        L, h, robot, tasks, _private = capi.lib(), self._h, self._robot, self._tasks, self._private
        for t in tasks:
            goal = None
            if t._ctrl is not None:  # the task was driven by hand before: it moves here (configuration replayed, goal kept; integrators start afresh)
                if robot.device >= 0:
                    old_id, t._id = t._id, 0
                    goal = t._get_goal()
                    t._id = old_id
                t._ctrl._release()
            t._ctrl = self
            t._manual = False
            for fn, args, _key in t._log:
                self._call(fn, t._id, *args)
            if goal is not None:
                a = np.ascontiguousarray(goal.T)
                capi.check(L.saip_batch_set_goal_host(h, t._id, _dptr(a)))
        if not _private:
            robot._controller = self
        robot._controllers.add(self)
        _set_base(h, robot._T_base)
        self._pushed_version = -1
        self._has_device = robot.device >= 0
        self._rec_mask = 0  # channels of the attached rollout recorder

    def __del__(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owns", True):
                capi.lib().saip_batch_destroy(self._h)
            self._h = None

    def _release(self):
        """a private one-task batch whose task joins a RobotController"""
        self._robot._controllers.discard(self)
        self.__del__()

    def _call(self, fn_name, *args):
        capi.check(getattr(capi.lib(), fn_name)(self._h, *args))

    def _push_state(self):
        r = self._robot
        if self._pushed_version != r._state_version:
            q, dq = np.ascontiguousarray(r._q.T), np.ascontiguousarray(r._dq.T)
            capi.check(capi.lib().saip_batch_set_state_host(self._h, _dptr(q), _dptr(dq)))
            self._pushed_version = r._state_version

    # -- reference API
    def updateControllerTaskModels(self):
        self._push_state()
        self._call("saip_batch_update_task_models")
        for t in self._tasks:
            t._manual = False

    def computeControlTorques(self):
        """returns (B, dof) joint torques; per-instance status in self.status (0 ok; bit 0 = refused: that row holds the last valid torques --
        zero before the first -- or NaN with setFlaggedTorquePolicy(True); check the status, not isnan)"""
        n, B = self._robot.dof(), self.batch_size
        tau = np.empty((n, B))
        st = np.zeros(B, np.uint8)
        capi.check(capi.lib().saip_batch_compute_control_torques(self._h, _dptr(tau), st.ctypes.data_as(C.POINTER(C.c_ubyte))))
        self.status = st
        return tau.T.copy()

    def enableGravityCompensation(self, e: bool):
        self._call("saip_batch_enable_gravity_compensation", int(e))

    def enableJointLimitAvoidance(self, e: bool):
        self._call("saip_batch_enable_joint_limit_avoidance", int(e))

    def enableTorqueSaturation(self, e: bool):
        self._call("saip_batch_enable_torque_saturation", int(e))

    def reinitializeTasks(self):
        self._push_state()
        self._call("saip_batch_reinitialize_tasks")

    def getTaskNames(self):
        return [t.getTaskName() for t in self._tasks]

    def _by_name(self, name, typ, what):
        for t in self._tasks:
            if t.getTaskName() == name:
                if t.getTaskType() != typ:  # RobotController.cpp:124-158
                    raise ValueError(f"Task {name} is not a {what}, and cannot be casted as such in RobotController::GetTaskByName")
                return t
        raise ValueError(f"Task {name} not found in RobotController::GetTaskByName")

    def getJointTaskByName(self, name):
        return self._by_name(name, TaskType.JOINT_TASK, "JointTask")

    def getMotionForceTaskByName(self, name):
        return self._by_name(name, TaskType.MOTION_FORCE_TASK, "MotionForceTask")

    # -- engine extras (resident pipelines, benchmarking)
    def setFlaggedTorquePolicy(self, nan: bool):
        """torques of instances that end a cycle flagged (status 1): False (default) = the last valid torques are held, True = NaN"""
        self._call("saip_batch_set_flagged_torque_policy", int(bool(nan)))

    def setFlaggedRecompute(self, on_list: bool):
        """where the eight-lane kernels recompute instances outside the non-singular branch: False (default) = in the kernel's slow tail, True = on the
        device-side list behind every cycle (saip_batch_set_flagged_recompute: faster when many instances of one group are singular at once)"""
        self._call("saip_batch_set_flagged_recompute", int(bool(on_list)))

    def setIntegratorTracking(self, always: bool):
        self._call("saip_batch_set_integrator_tracking", int(always))

    def setKernel(self, which: int):
        self._call("saip_batch_set_kernel", int(which))

    def kernelName(self) -> str:
        return capi.lib().saip_batch_kernel_name(self._h).decode()

    def setGoals(self, goals):
        """goals[t]: (B, goal_components) whole goal block per task, controller order"""
        for t, g in zip(self._tasks, goals):
            gs = capi.lib().saip_batch_goal_components(self._h, t._id)
            g = np.asarray(g, float)
            if g.ndim == 2 and g.shape[1] in (24, 30) and gs > g.shape[1]:  # no goal / sensed force and moment given: zeros
                g = np.concatenate([g, np.zeros((g.shape[0], gs - g.shape[1]))], axis=1)
            a = _soa(g, self.batch_size, gs, f"goal of task {t.getTaskName()}")
            capi.check(capi.lib().saip_batch_set_goal_host(self._h, t._id, _dptr(a)))

    def stepAsync(self):
        self._call("saip_batch_step_async")

    # -- the step after the path: resident forward dynamics (what the examples do with sim->integrate(), examples/05-...cpp:225-231)
    @staticmethod
    def _grav(gravity):
        if gravity is None:
            return None, None
        g = np.ascontiguousarray(np.asarray(gravity, float).reshape(3))
        return g, _dptr(g)

    def integrate(self, dt: float, substeps: int = 1, gravity=None, damping: float = 0.0):
        """semi-implicit Euler steps of the resident state under the torques of the last cycle; gravity None = model gravity"""
        self._push_state()
        g, gp = self._grav(gravity)
        self._call("saip_batch_integrate", float(dt), int(substeps), gp, float(damping))

    def rolloutAsync(self, steps: int, sim_dt: float, substeps: int = 1, gravity=None, damping: float = 0.0):
        """`steps` closed-loop periods {internal OTGs, control cycle, integrate} enqueued without host synchronisation"""
        self._push_state()
        g, gp = self._grav(gravity)
        self._call("saip_batch_rollout_async", int(steps), float(sim_dt), int(substeps), gp, float(damping))

    def contactSense(self):
        """enqueue the simulated sensor of the attached contact planes (task.attachContactPlanes) at the current state: what a rollout
        period does first, for a host-driven loop { contactSense, computeControlTorques / stepAsync, integrate }"""
        self._call("saip_batch_contact_info", None, None, None, None, None)  # without an attachment: that error, before the device is needed
        self._push_state()
        self._call("saip_batch_contact_sense")

    def contactPatchSense(self):
        """enqueue the simulated sensors of the attached contact patches (task.attachContactPatch) at the current state: what a rollout
        period does first, for a host-driven loop { contactPatchSense, computeControlTorques / stepAsync, integrate }"""
        self._call("saip_batch_contact_patch_info", -1, None, None, None, None, None, None)  # without a patch: that error, before the device is needed
        self._push_state()
        self._call("saip_batch_contact_patch_sense")

    # -- guards: event-triggered phases inside rollouts (task.attachGuards; saip.h)
    def guardInfo(self):
        """dict task, n_guards, per_instance, n_phases, needs_pose"""
        v = [C.c_int(0) for _ in range(5)]
        self._call("saip_batch_guard_info", *(C.byref(x) for x in v))
        return dict(task=v[0].value, n_guards=v[1].value, per_instance=bool(v[2].value), n_phases=v[3].value, needs_pose=bool(v[4].value))

    def evaluateGuards(self):
        """enqueue one evaluation of the guards at the current state: what a rollout period does in front of its OTG step and cycle, for a
        host-driven loop { contactSense, evaluateGuards, stepAsync, integrate }"""
        self.guardInfo()  # without an attachment: that error, before the device is needed
        self._push_state()
        self._call("saip_batch_guard_evaluate")

    def resetGuards(self):
        """every instance back to phase 0 with counters, entry times and latches cleared, on the engine stream"""
        self._call("saip_batch_guard_reset")

    def guardState(self):
        """dict phase (B,), since (B,), clock (B,), run (G, B), entry (P, B) (the period of the first entry into a phase, -1: never),
        fires (G, B), latch (12, B) (position 3, rotation 9 row-major) (waits for the engine stream)"""
        info = self.guardInfo()
        B, G, P = self.batch_size, info["n_guards"], info["n_phases"]
        a = dict(phase=np.zeros(B, np.int32), since=np.zeros(B, np.int32), clock=np.zeros(B, np.int32), run=np.zeros((G, B), np.int32),
                 entry=np.zeros((P, B), np.int32), fires=np.zeros((G, B), np.int32), latch=np.zeros((12, B)))
        ip = C.POINTER(C.c_int)
        self._call("saip_batch_guard_state_host", *(a[k].ctypes.data_as(ip) for k in ("phase", "since", "clock", "run", "entry", "fires")), _dptr(a["latch"]))
        return a

    def guardReadout(self):
        """dict of what the last guard launch saw: force, moment, pos_error, ori_error (norms), joint_speed (B,) and position (B, 3); NaN
        where the guard and phase tables did not need the quantity (waits for the engine stream)"""
        self.guardInfo()
        out = np.empty((capi.SAIP_GUARD_READOUT_ROWS, self.batch_size))
        self._call("saip_batch_guard_readout_host", _dptr(out))
        return dict(force=out[0].copy(), moment=out[1].copy(), pos_error=out[2].copy(), ori_error=out[3].copy(), joint_speed=out[4].copy(), position=out[5:8].T.copy())

    def guardCost(self, phase, w_time, w_miss=float("inf")):
        """cost += w_time * (period of the first entry into `phase`), or w_miss where the instance never got there, on the device, after
        rolloutCost(); the default w_miss makes "never got there" an invalid sample to updateSampler()"""
        self._call("saip_batch_guard_add_cost", int(phase), float(w_time), float(w_miss))

    # -- clearance monitor: link spheres against world-fixed obstacles and against each other, inside rollouts (saip.h)
    @staticmethod
    def _clearance_obstacles(obstacles, per_instance, B, who, n_obstacles=None):
        a = np.asarray(obstacles, float)
        W, O = capi.SAIP_CLEARANCE_OBSTACLE_WORDS, "O" if n_obstacles is None else n_obstacles
        if per_instance:
            if a.ndim != 3 or a.shape[1:] != (B, W) or (n_obstacles is not None and a.shape[0] != n_obstacles):
                raise ValueError(f"{who}: per-instance obstacles of shape ({O}, {B}, {W}) expected, got {a.shape}")
            return np.ascontiguousarray(a.transpose(0, 2, 1))
        if a.ndim != 2 or a.shape[1] != W or (n_obstacles is not None and a.shape[0] != n_obstacles):
            raise ValueError(f"{who}: obstacles of shape ({O}, {W}) expected, got {a.shape}")
        return np.ascontiguousarray(a)

    def attachClearance(self, spheres, obstacles=None, pairs=None, margin=0.0, per_instance=False, keep_centres=False):
        """watch the clearance of the robot during rollouts.  spheres: up to 32 of (link name, centre in the link frame (3), radius);
        obstacles: up to 16 rows { kind, a[3], b[3], r } -- kind 0 a capsule (segment a-b, radius r; a == b a sphere), kind 1 a half-space
        (a the unit normal, b[0] the offset) -- of shape (O, 8), or (O, B, 8) with per_instance; pairs: up to 64 (s1, s2) of sphere
        indices checked against each other; margin >= 0: distances below it are penalised.  While attached every period of
        rolloutAsync() advances clearanceSummary(); clearanceCost() adds it to the sampler's cost."""
        spheres = list(spheres)
        links = np.empty(len(spheres), np.int32)
        centres, radii = np.zeros((len(spheres), 3)), np.zeros(len(spheres))
        for s, sph in enumerate(spheres):
            if len(sph) != 3:
                raise ValueError(f"attachClearance: sphere {s}: (link, centre, radius) expected")
            links[s] = self._robot.linkIndex(sph[0])
            if links[s] < 0:
                raise ValueError(f"attachClearance: sphere {s}: unknown link [{sph[0]}]")
            c = np.asarray(sph[1], float).reshape(-1)
            if c.shape != (3,):
                raise ValueError(f"attachClearance: sphere {s}: a centre of shape (3,) expected, got {c.shape}")
            centres[s], radii[s] = c, float(sph[2])
        a = None if obstacles is None else self._clearance_obstacles(obstacles, per_instance, self.batch_size, "attachClearance")
        p = None if pairs is None else np.ascontiguousarray(pairs, np.int32)
        if p is not None and p.size and (p.ndim != 2 or p.shape[1] != 2):
            raise ValueError(f"attachClearance: pairs of shape (P, 2) expected, got {p.shape}")
        n_o, n_p = 0 if a is None else a.shape[0], 0 if p is None else p.size // 2
        ip = C.POINTER(C.c_int)
        self._call("saip_batch_clearance_attach", len(spheres), links.ctypes.data_as(ip), _dptr(centres), _dptr(radii), n_o, None if n_o == 0 else _dptr(a),
                   int(bool(per_instance)), n_p, None if n_p == 0 else p.ctypes.data_as(ip), float(margin), int(bool(keep_centres)))
        self._clearance_pairs = np.zeros((0, 2), int) if n_p == 0 else p.reshape(-1, 2).astype(int)

    def clearanceInfo(self):
        """dict n_spheres, n_obstacles, per_instance, n_pairs, margin, keep_centres, period (monitored periods since the last reset)"""
        v = [C.c_int(0) for _ in range(5)]
        m, per = C.c_double(0), C.c_longlong(0)
        self._call("saip_batch_clearance_info", C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), C.byref(m), C.byref(v[4]), C.byref(per))
        return dict(n_spheres=v[0].value, n_obstacles=v[1].value, per_instance=bool(v[2].value), n_pairs=v[3].value, margin=m.value,
                    keep_centres=bool(v[4].value), period=per.value)

    def detachClearance(self):
        self._call("saip_batch_clearance_detach")

    def setClearanceObstacles(self, obstacles):
        """replace the obstacle table (same shape as attached); takes effect with the next launch"""
        info = self.clearanceInfo()
        a = self._clearance_obstacles(obstacles, info["per_instance"], self.batch_size, "setClearanceObstacles", info["n_obstacles"])
        self._call("saip_batch_clearance_set_obstacles_host", _dptr(a))

    def evaluateClearance(self):
        """enqueue one evaluation at the current state: clearanceReadout() (and the kept centres) only, the summaries stay"""
        self.clearanceInfo()  # without an attachment: that error, before the device is needed
        self._push_state()
        self._call("saip_batch_clearance_evaluate")

    def clearanceReadout(self):
        """dict of the last clearance launch: distance (B,) the smallest signed distance, item (B,) its number, closest: per instance
        ("obstacle", sphere, obstacle), ("pair", s1, s2) or None (invalid instance), penalty (B,), under_margin (B,), point (B, 3) the
        centre of the closest item's (first) sphere, pair_distance (B,) the smallest self-pair distance (waits for the engine stream)"""
        info = self.clearanceInfo()
        out = np.empty((capi.SAIP_CLEARANCE_READOUT_ROWS, self.batch_size))
        self._call("saip_batch_clearance_readout_host", _dptr(out))
        S, O = info["n_spheres"], info["n_obstacles"]
        item = out[1].astype(int)
        closest = [None if k < 0 else ("obstacle", int(k) // O, int(k) % O) if k < S * O else ("pair",) + tuple(int(x) for x in self._clearance_pairs[k - S * O])
                   for k in item]
        return dict(distance=out[0].copy(), item=item, closest=closest, penalty=out[2].copy(), under_margin=out[3].astype(int), point=out[4:7].T.copy(),
                    pair_distance=out[7].copy())

    def clearanceSummary(self):
        """dict over the monitored periods: min_distance (B,) (NaN once an instance was invalid), penalty (B,) sum dt * penalty,
        periods_in_collision (B,), first_collision (B,) the index of the first period with a negative distance, else -1 (waits for the
        engine stream)"""
        self.clearanceInfo()
        out = np.empty((capi.SAIP_CLEARANCE_SUMMARY_ROWS, self.batch_size))
        self._call("saip_batch_clearance_summary_host", _dptr(out))
        return dict(min_distance=out[0].copy(), penalty=out[1].copy(), periods_in_collision=out[2].astype(int), first_collision=out[3].astype(int))

    def resetClearanceSummary(self):
        """summaries back to +inf, 0, 0, -1 and the period counter to 0; pair it with restoreState (the summaries are not part of a snapshot)"""
        self._call("saip_batch_clearance_summary_reset")

    def clearanceCentresDevice(self):
        """device pointer of the (3 S, ld) sphere centres of the last launch; None unless attached with keep_centres"""
        return capi.lib().saip_batch_clearance_centres_device(self._h)

    def clearanceCost(self, w_penalty, w_collision=float("inf"), d_safe=0.0):
        """cost += w_penalty * summary penalty + (min_distance < d_safe ? w_collision : 0) on the device, after rolloutCost(); an infinite
        cost is an invalid sample to updateSampler(), so the default w_collision makes collision a hard constraint"""
        self._call("saip_batch_clearance_add_cost", float(w_penalty), float(w_collision), float(d_safe))

    # -- link contact: world-fixed obstacles push back on the robot's link spheres in front of every integration substep (saip.h)
    def attachLinkContact(self, spheres, obstacles, materials, per_instance=False, keep=False):
        """let obstacles push back on the robot.  spheres: up to 32 of (link name, centre in the link frame (3), radius); obstacles: up to
        16 rows as in attachClearance, of shape (O, 8), or (O, B, 8) with per_instance; materials: (O, 4) rows { k, c, mu, v_s }
        (stiffness, damping, friction, slip-regularisation speed).  While attached every integration substep of integrate() and
        rolloutAsync() adds sum_s J_v(c_s)^T F_s to the torques it integrates and advances linkContactSummary(); keep: centres,
        velocities and sphere forces of the last launch stay on the device (linkContactKeepDevice)."""
        spheres = list(spheres)
        links = np.empty(len(spheres), np.int32)
        centres, radii = np.zeros((len(spheres), 3)), np.zeros(len(spheres))
        for s, sph in enumerate(spheres):
            if len(sph) != 3:
                raise ValueError(f"attachLinkContact: sphere {s}: (link, centre, radius) expected")
            links[s] = self._robot.linkIndex(sph[0])
            if links[s] < 0:
                raise ValueError(f"attachLinkContact: sphere {s}: unknown link [{sph[0]}]")
            c = np.asarray(sph[1], float).reshape(-1)
            if c.shape != (3,):
                raise ValueError(f"attachLinkContact: sphere {s}: a centre of shape (3,) expected, got {c.shape}")
            centres[s], radii[s] = c, float(sph[2])
        a = self._clearance_obstacles(obstacles, per_instance, self.batch_size, "attachLinkContact")
        m = np.ascontiguousarray(materials, float)
        if m.shape != (a.shape[0], capi.SAIP_LINK_CONTACT_MATERIAL_WORDS):
            raise ValueError(f"attachLinkContact: materials of shape ({a.shape[0]}, {capi.SAIP_LINK_CONTACT_MATERIAL_WORDS}) expected, got {m.shape}")
        self._call("saip_batch_link_contact_attach", len(spheres), links.ctypes.data_as(C.POINTER(C.c_int)), _dptr(centres), _dptr(radii), a.shape[0], _dptr(a),
                   _dptr(m), int(bool(per_instance)), int(bool(keep)))

    def linkContactInfo(self):
        """dict n_spheres, n_obstacles, per_instance, keep"""
        v = [C.c_int(0) for _ in range(4)]
        self._call("saip_batch_link_contact_info", C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]))
        return dict(n_spheres=v[0].value, n_obstacles=v[1].value, per_instance=bool(v[2].value), keep=bool(v[3].value))

    def detachLinkContact(self):
        self._call("saip_batch_link_contact_detach")

    def setLinkContactObstacles(self, obstacles):
        """replace the obstacle table (same shape as attached); takes effect with the next launch"""
        info = self.linkContactInfo()
        a = self._clearance_obstacles(obstacles, info["per_instance"], self.batch_size, "setLinkContactObstacles", info["n_obstacles"])
        self._call("saip_batch_link_contact_set_obstacles_host", _dptr(a))

    def setLinkContactMaterials(self, materials):
        """replace the material table (O, 4); takes effect with the next launch"""
        info = self.linkContactInfo()
        m = np.ascontiguousarray(materials, float)
        if m.shape != (info["n_obstacles"], capi.SAIP_LINK_CONTACT_MATERIAL_WORDS):
            raise ValueError(f"setLinkContactMaterials: materials of shape ({info['n_obstacles']}, {capi.SAIP_LINK_CONTACT_MATERIAL_WORDS}) expected, got {m.shape}")
        self._call("saip_batch_link_contact_set_materials_host", _dptr(m))

    def evaluateLinkContact(self):
        """enqueue one evaluation at the current state: linkContactReadout() (and the kept arrays) only, torques and summaries stay"""
        self.linkContactInfo()  # without an attachment: that error, before the device is needed
        self._push_state()
        self._call("saip_batch_link_contact_evaluate")

    def linkContactReadout(self):
        """dict of the last link-contact launch: force (B, 3) the net force on the robot, distance (B,) the smallest signed distance over
        all items, item (B,) its number, closest: per instance (sphere, obstacle) or None (invalid instance), active (B,) active items,
        normal_force (B,) sum f_n, peak_force (B,) the largest single-item |f| (waits for the engine stream)"""
        info = self.linkContactInfo()
        out = np.empty((capi.SAIP_LINK_CONTACT_READOUT_ROWS, self.batch_size))
        self._call("saip_batch_link_contact_readout_host", _dptr(out))
        O = info["n_obstacles"]
        item = out[4].astype(int)
        closest = [None if k < 0 else (int(k) // O, int(k) % O) for k in item]
        return dict(force=out[0:3].T.copy(), distance=out[3].copy(), item=item, closest=closest, active=out[5].astype(int), normal_force=out[6].copy(),
                    peak_force=out[7].copy())

    def linkContactSummary(self):
        """dict over the integrated substeps: impulse (B,) sum dt sum f_n (NaN once an instance was invalid), peak_force (B,),
        max_penetration (B,), substeps_in_contact (B,) (waits for the engine stream)"""
        self.linkContactInfo()
        out = np.empty((capi.SAIP_LINK_CONTACT_SUMMARY_ROWS, self.batch_size))
        self._call("saip_batch_link_contact_summary_host", _dptr(out))
        return dict(impulse=out[0].copy(), peak_force=out[1].copy(), max_penetration=out[2].copy(), substeps_in_contact=out[3].astype(int))

    def resetLinkContactSummary(self):
        """summaries back to 0; pair it with restoreState (the summaries are not part of a snapshot)"""
        self._call("saip_batch_link_contact_summary_reset")

    def linkContactTorquesDevice(self):
        """device pointer of the (dof, ld) commanded + link-contact torques of the last integrated substep; None when detached"""
        return capi.lib().saip_batch_link_contact_torques_device(self._h)

    def linkContactKeepDevice(self):
        """device pointer of the (9 S, ld) centres, velocities and sphere forces of the last launch; None unless attached with keep"""
        return capi.lib().saip_batch_link_contact_keep_device(self._h)

    def linkContactCost(self, w_impulse, w_peak=0.0):
        """cost += w_impulse * summary impulse + w_peak * summary peak force on the device, after rolloutCost()"""
        self._call("saip_batch_link_contact_add_cost", float(w_impulse), float(w_peak))

    # -- link object: a free rigid body the robot's link spheres push, the second stage of link contact (saip.h)
    def attachLinkObject(self, spheres, material, inertial, per_instance=False, state=None):
        """attach the pushed object (needs attachLinkContact).  spheres: up to 8 of (centre in the body frame (3), radius); material: (4,)
        { k, c, mu, v_s } of robot-object contact; inertial: (4,) { m, Ix, Iy, Iz }, or (B, 4) with per_instance; state: as setObjectState
        takes it (default: the body frame on the world frame, at rest).  While attached every integration substep of integrate() and
        rolloutAsync() lets the robot's spheres and the link-contact obstacles push the body and integrates it; objectState() is part of
        saveState() / restoreState()."""
        spheres = list(spheres)
        centres, radii = np.zeros((len(spheres), 3)), np.zeros(len(spheres))
        for s, sph in enumerate(spheres):
            if len(sph) != 2:
                raise ValueError(f"attachLinkObject: sphere {s}: (centre, radius) expected")
            c = np.asarray(sph[0], float).reshape(-1)
            if c.shape != (3,):
                raise ValueError(f"attachLinkObject: sphere {s}: a centre of shape (3,) expected, got {c.shape}")
            centres[s], radii[s] = c, float(sph[1])
        m = np.ascontiguousarray(material, float)
        if m.shape != (capi.SAIP_LINK_CONTACT_MATERIAL_WORDS,):
            raise ValueError(f"attachLinkObject: a material of shape ({capi.SAIP_LINK_CONTACT_MATERIAL_WORDS},) expected, got {m.shape}")
        inr = self._object_inertial(inertial, per_instance, "attachLinkObject")
        x = None if state is None else self._object_state(state, "attachLinkObject")
        self._call("saip_batch_link_object_attach", len(spheres), _dptr(centres), _dptr(radii), _dptr(m), _dptr(inr), int(bool(per_instance)))
        if x is not None:
            try:
                self._call("saip_batch_link_object_set_state_host", _dptr(x[0]), x[1])
            except Exception:
                self._call("saip_batch_link_object_detach")
                raise

    def _object_inertial(self, inertial, per_instance, who):
        a, W = np.asarray(inertial, float), capi.SAIP_LINK_OBJECT_INERTIAL_WORDS
        want = (self.batch_size, W) if per_instance else (W,)
        if a.shape != want:
            raise ValueError(f"{who}: {'per-instance ' if per_instance else ''}inertial words of shape {want} expected, got {a.shape}")
        return np.ascontiguousarray(a.T)

    def _object_state(self, state, who):
        a, R = np.asarray(state, float), capi.SAIP_LINK_OBJECT_STATE_ROWS
        if a.shape == (R,):
            return np.ascontiguousarray(a), 0
        if a.shape == (self.batch_size, R):
            return np.ascontiguousarray(a.T), 1
        raise ValueError(f"{who}: a state of shape ({R},) or ({self.batch_size}, {R}) expected, got {a.shape}")

    def linkObjectInfo(self):
        """dict n_spheres, per_instance (of the inertial words)"""
        v = [C.c_int(0) for _ in range(2)]
        self._call("saip_batch_link_object_info", C.byref(v[0]), C.byref(v[1]))
        return dict(n_spheres=v[0].value, per_instance=bool(v[1].value))

    def detachLinkObject(self):
        self._call("saip_batch_link_object_detach")

    def setObjectState(self, state):
        """(13,) for every instance or (B, 13): p (3), quaternion (w, x, y, z) body to world (normalised here), v (3), omega (3, world frame)"""
        x, per = self._object_state(state, "setObjectState")
        self._call("saip_batch_link_object_set_state_host", _dptr(x), per)

    def setObjectInertial(self, inertial):
        """replace the inertial words { m, Ix, Iy, Iz } (same shape as attached)"""
        info = self.linkObjectInfo()
        self._call("saip_batch_link_object_set_inertial_host", _dptr(self._object_inertial(inertial, info["per_instance"], "setObjectInertial")))

    def objectState(self):
        """(B, 13) the object's state (waits for the engine stream)"""
        self.linkObjectInfo()
        out = np.empty((capi.SAIP_LINK_OBJECT_STATE_ROWS, self.batch_size))
        self._call("saip_batch_link_object_state_host", _dptr(out))
        return np.ascontiguousarray(out.T)

    def objectReadout(self):
        """dict of the last link-contact launch: force (B, 3) and moment (B, 3) (about the body origin) of the robot on the object,
        world_force (B, 3), distance (B,) the smallest robot-object distance, item (B,) its number s P + p (-1: invalid instance),
        closest: per instance (robot sphere, object sphere) or None, active (B,) active robot-object items, raw (B, 12)"""
        info = self.linkObjectInfo()
        out = np.empty((capi.SAIP_LINK_OBJECT_READOUT_ROWS, self.batch_size))
        self._call("saip_batch_link_object_readout_host", _dptr(out))
        P = info["n_spheres"]
        item = np.where(np.isnan(out[10]), -1, out[10]).astype(int)
        closest = [None if k < 0 else (int(k) // P, int(k) % P) for k in item]
        return dict(force=out[0:3].T.copy(), moment=out[3:6].T.copy(), world_force=out[6:9].T.copy(), distance=out[9].copy(), item=item, closest=closest,
                    active=np.where(np.isnan(out[11]), 0, out[11]).astype(int), raw=np.ascontiguousarray(out.T))

    def objectSummary(self):
        """dict over the integrated substeps: impulse (B,) sum dt sum f_n of the robot on the object (NaN once an instance was invalid),
        max_penetration (B,) robot-object, max_world_penetration (B,) object-world, substeps_in_contact (B,), raw (B, 4)"""
        self.linkObjectInfo()
        out = np.empty((capi.SAIP_LINK_OBJECT_SUMMARY_ROWS, self.batch_size))
        self._call("saip_batch_link_object_summary_host", _dptr(out))
        return dict(impulse=out[0].copy(), max_penetration=out[1].copy(), max_world_penetration=out[2].copy(), substeps_in_contact=out[3].astype(int),
                    raw=np.ascontiguousarray(out.T))

    def resetObjectSummary(self):
        """summaries back to 0 (they are not part of a snapshot; the object's state is)"""
        self._call("saip_batch_link_object_summary_reset")

    def objectStateDevice(self):
        """device pointer of the (13, ld) object state; None when detached"""
        return capi.lib().saip_batch_link_object_state_device(self._h)

    def objectCost(self, target_p, w_pos, target_quat=None, w_ori=0.0):
        """cost += w_pos |p - target_p|^2 + w_ori (1 - (q . target_quat)^2) on the device, after rolloutCost(); an object state that is
        not finite costs +inf"""
        tp = np.ascontiguousarray(target_p, float).reshape(-1)
        if tp.shape != (3,):
            raise ValueError(f"objectCost: a target position of shape (3,) expected, got {tp.shape}")
        tq = None
        if target_quat is not None:
            tq = np.ascontiguousarray(target_quat, float).reshape(-1)
            if tq.shape != (4,):
                raise ValueError(f"objectCost: a target quaternion of shape (4,) expected, got {tq.shape}")
        self._call("saip_batch_link_object_add_cost", _dptr(tp), float(w_pos), None if tq is None else _dptr(tq), float(w_ori))

    # -- environment schedules: obstacles and contact surfaces that move inside rollouts (saip.h)
    _ENV_MODES = {"hold": capi.SAIP_ENV_HOLD, "linear": capi.SAIP_ENV_LINEAR}

    def _env_schedule_attach(self, who, target, task, keyframes, W, per_instance, stride, mode, first):
        if mode not in self._ENV_MODES:
            raise ValueError(f"{who}: unknown mode {mode!r} (one of {sorted(self._ENV_MODES)})")
        k, B = np.asarray(keyframes, float), self.batch_size
        if per_instance:
            if k.ndim != 4 or k.shape[2:] != (B, W):
                raise ValueError(f"{who}: the table is per instance: keyframes of shape (K, n, {B}, {W}) expected, got {k.shape}")
            a = np.ascontiguousarray(k.transpose(0, 1, 3, 2))
        else:
            if k.ndim != 3 or k.shape[2] != W:
                raise ValueError(f"{who}: the table is batch-uniform: keyframes of shape (K, n, {W}) expected, got {k.shape}")
            a = np.ascontiguousarray(k)
        self._call("saip_batch_env_schedule_attach", target, task, int(first), a.shape[1], _dptr(a), a.shape[0], int(stride), self._ENV_MODES[mode])

    def _env_schedule_info(self, target, task):
        v = [C.c_int(0) for _ in range(6)]
        period = C.c_longlong(0)
        self._call("saip_batch_env_schedule_info", target, task, *(C.byref(x) for x in v), C.byref(period))
        mode = {m: name for name, m in self._ENV_MODES.items()}[v[4].value]
        return dict(first=v[0].value, n_items=v[1].value, n_keyframes=v[2].value, stride=v[3].value, mode=mode, per_instance=bool(v[5].value),
                    period=period.value)

    def setObstacleSchedule(self, keyframes, stride=1, mode="hold", first=0):
        """let the obstacles of the clearance monitor move during rollouts.  keyframes: (K, n, 8), or (K, n, B, 8) when the obstacle table is
        per instance, rows as in attachClearance.  The monitor of rollout period c looks at the state at the END of the period, so it sees
        keyframe (c + 1) // stride ("hold") or that one moved towards the next by ((c + 1) % stride) / stride ("linear"; half-space
        normals stay unit); the last keyframe is held.  The schedule covers obstacles first .. first + n - 1."""
        info = self.clearanceInfo()
        self._env_schedule_attach("setObstacleSchedule", capi.SAIP_ENV_TARGET_OBSTACLES, -1, keyframes, capi.SAIP_CLEARANCE_OBSTACLE_WORDS,
                                  info["per_instance"], stride, mode, first)

    def clearObstacleSchedule(self):
        """detach the schedule; the obstacles keep the values written last"""
        self._call("saip_batch_env_schedule_detach", capi.SAIP_ENV_TARGET_OBSTACLES, -1)

    def obstacleScheduleInfo(self):
        """dict first, n_items, n_keyframes, stride, mode, per_instance, period"""
        return self._env_schedule_info(capi.SAIP_ENV_TARGET_OBSTACLES, -1)

    def clearEnvironmentSchedules(self):
        """detach every environment schedule of the controller"""
        self._call("saip_batch_env_schedule_detach", -1, -1)

    def rewindEnvironment(self, period=0):
        """the next rollout period is period `period` of the environment schedules: 0 to replay them, the current period to start a
        receding-horizon prediction at the current time; what goes with restoreState (tables are not part of a snapshot)"""
        self._call("saip_batch_env_schedule_rewind", int(period))

    # -- plant model: actuator limits, friction, joint stops and external wrenches in front of every integration substep (saip.h)
    PLANT_JOINT_WORDS = ("gain", "bias", "tau_max", "fv", "fc", "v_s", "q_lo", "q_hi", "k_stop", "c_stop")

    def neutralPlantJoints(self):
        """the (dof, 10) joint table that changes nothing: gain 1, no offset, no limit, no friction, the model's joint limits as stops of
        stiffness 0 -- a starting point for attachPlant(joints=...)"""
        lim = self._robot.jointLimits()
        lo, hi = lim["position_lower"], lim["position_upper"]
        ok = lo <= hi
        t = np.zeros((self._robot.dof(), capi.SAIP_PLANT_JOINT_WORDS))
        t[:, 0], t[:, 2] = 1.0, np.inf
        t[:, 6], t[:, 7] = np.where(ok, lo, -np.inf), np.where(ok, hi, np.inf)
        return t

    @staticmethod
    def _plant_table(table, per_instance, B, rows, words, who, what):
        a = np.asarray(table, float)
        if per_instance:
            if a.shape != (rows, B, words):
                raise ValueError(f"{who}: per-instance {what} of shape ({rows}, {B}, {words}) expected, got {a.shape}")
            return np.ascontiguousarray(a.transpose(0, 2, 1))
        if a.shape != (rows, words):
            raise ValueError(f"{who}: {what} of shape ({rows}, {words}) expected, got {a.shape}")
        return np.ascontiguousarray(a)

    def attachPlant(self, joints=None, wrenches=None, per_instance=False):
        """put a plant model between the commanded torques and the resident simulator.  joints: (dof, 10) rows { gain, bias, tau_max, fv,
        fc, v_s, q_lo, q_hi, k_stop, c_stop }, or (dof, B, 10) with per_instance; None: neutral rows with the model's joint limits and
        k_stop = 0.  wrenches: up to 4 of (link name, point in the link frame (3), "world" or "link", values) with values { F[3], M[3],
        p_start, p_end } of shape (8,), or (B, 8) with per_instance; six values act for ever.  A wrench acts in the periods
        p_start <= p < p_end of plantInfo()["period"], which integrate() and every rollout period advance by one.  While attached,
        integrate() and rolloutAsync() run the plant in front of every substep (and in front of the contact launch, if any)."""
        B, who = self.batch_size, "attachPlant"
        jt = None if joints is None else self._plant_table(joints, per_instance, B, self._robot.dof(), capi.SAIP_PLANT_JOINT_WORDS, who, "joints")
        wrenches = [] if wrenches is None else list(wrenches)
        Wn = len(wrenches)
        links, frames = np.zeros(max(Wn, 1), np.int32), np.zeros(max(Wn, 1), np.int32)
        points = np.zeros((max(Wn, 1), 3))
        vals = []
        for k, w in enumerate(wrenches):
            if len(w) != 4:
                raise ValueError(f"{who}: wrench {k}: (link, point, frame, values) expected")
            links[k] = self._robot.linkIndex(w[0])
            if links[k] < 0:
                raise ValueError(f"{who}: wrench {k}: unknown link [{w[0]}]")
            p = np.asarray(w[1], float).reshape(-1)
            if p.shape != (3,):
                raise ValueError(f"{who}: wrench {k}: a point of shape (3,) expected, got {p.shape}")
            points[k] = p
            if w[2] not in ("world", "link"):
                raise ValueError(f"{who}: wrench {k}: frame 'world' or 'link' expected, got {w[2]!r}")
            frames[k] = capi.SAIP_PLANT_FRAME_LINK if w[2] == "link" else capi.SAIP_PLANT_FRAME_WORLD
            v = np.asarray(w[3], float)
            if v.shape[-1:] == (6,):
                v = np.concatenate([v, np.broadcast_to([-np.inf, np.inf], v.shape[:-1] + (2,))], axis=-1)
            want = (B, capi.SAIP_PLANT_WRENCH_WORDS) if per_instance else (capi.SAIP_PLANT_WRENCH_WORDS,)
            if v.shape != want:
                raise ValueError(f"{who}: wrench {k}: values of shape {want} (or with 6 in place of 8) expected, got {v.shape}")
            vals.append(v)
        wt = None if Wn == 0 else self._plant_table(np.stack(vals), per_instance, B, Wn, capi.SAIP_PLANT_WRENCH_WORDS, who, "wrench values")
        ip = C.POINTER(C.c_int)
        self._call("saip_batch_plant_attach", None if jt is None else _dptr(jt), int(bool(per_instance)), Wn, links.ctypes.data_as(ip), _dptr(points),
                   frames.ctypes.data_as(ip), None if wt is None else _dptr(wt), int(bool(per_instance)))

    def plantInfo(self):
        """dict per_instance_joints, n_wrenches, per_instance_wrenches, period (the period the next integration belongs to)"""
        v = [C.c_int(0) for _ in range(3)]
        per = C.c_longlong(0)
        self._call("saip_batch_plant_info", C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(per))
        return dict(per_instance_joints=bool(v[0].value), n_wrenches=v[1].value, per_instance_wrenches=bool(v[2].value), period=per.value)

    def detachPlant(self):
        self._call("saip_batch_plant_detach")

    def setPlantJoints(self, joints):
        """replace the joint table (same shape as attached); takes effect with the next launch"""
        info = self.plantInfo()
        a = self._plant_table(joints, info["per_instance_joints"], self.batch_size, self._robot.dof(), capi.SAIP_PLANT_JOINT_WORDS, "setPlantJoints", "joints")
        self._call("saip_batch_plant_set_joints_host", _dptr(a))

    def setPlantWrenches(self, values):
        """replace the wrench values: (W, 8), or (W, B, 8) when attached per instance; the sites stay"""
        info = self.plantInfo()
        a = self._plant_table(values, info["per_instance_wrenches"], self.batch_size, info["n_wrenches"], capi.SAIP_PLANT_WRENCH_WORDS, "setPlantWrenches",
                              "wrench values")
        self._call("saip_batch_plant_set_wrenches_host", _dptr(a))

    def randomizePlant(self, seed, round=0, joints=None, wrenches=None):
        """draw the per-instance tables on the device: joints = (lo, hi), two (dof, 10) tables, wrenches = (lo, hi), two (W, 8) tables;
        every word of every instance is uniform between its bounds (lo == hi: exactly lo), reproducibly for (seed, round); None leaves
        that table alone.  Tables attached without per_instance are refused."""
        info = self.plantInfo()

        def pair(b, rows, words, what):
            if b is None:
                return None, None
            lo, hi = (self._plant_table(x, False, 0, rows, words, "randomizePlant", what) for x in b)
            return lo, hi
        jl, jh = pair(joints, self._robot.dof(), capi.SAIP_PLANT_JOINT_WORDS, "joint bounds")
        wl, wh = pair(wrenches, info["n_wrenches"], capi.SAIP_PLANT_WRENCH_WORDS, "wrench bounds")
        self._call("saip_batch_plant_randomize", int(seed) & (2**64 - 1), int(round), *(None if x is None else _dptr(x) for x in (jl, jh, wl, wh)))

    def setPlantPeriod(self, period):
        """the plant's period counter (wrench windows); pair it with restoreState, since the counter is not part of a snapshot"""
        self._call("saip_batch_plant_set_period", int(period))

    def plantSummary(self):
        """dict over the integrated substeps: friction_loss (B,) sum dt sum_j |fr_j dq_j|, max_clip (B,) the largest torque the actuator
        limits cut off, substeps_limited (B,) substeps in which a joint clipped or a stop acted, external_work (B,) sum dt sum ext_j dq_j
        (waits for the engine stream)"""
        self.plantInfo()
        out = np.empty((capi.SAIP_PLANT_SUMMARY_ROWS, self.batch_size))
        self._call("saip_batch_plant_summary_host", _dptr(out))
        return dict(friction_loss=out[0].copy(), max_clip=out[1].copy(), substeps_limited=out[2].astype(int), external_work=out[3].copy())

    def resetPlantSummary(self):
        self._call("saip_batch_plant_summary_reset")

    def plantJointsDevice(self):
        """device pointer of the resident joint table, (dof, 10) or (dof, 10, ld); None when detached"""
        return capi.lib().saip_batch_plant_joints_device(self._h)

    def plantWrenchesDevice(self):
        """device pointer of the resident wrench values, (W, 8) or (W, 8, ld); None when detached or without wrenches"""
        return capi.lib().saip_batch_plant_wrenches_device(self._h)

    def plantTorquesDevice(self):
        """device pointer of the (dof, ld) actuated torques of the last integrated substep; None when detached"""
        return capi.lib().saip_batch_plant_torques_device(self._h)

    def plantSummaryDevice(self):
        """device pointer of the (4, ld) running summaries; None when detached"""
        return capi.lib().saip_batch_plant_summary_device(self._h)

    # -- the two chains (below: the actuation chain; behind the sensing model: the sensing chain) share these helpers.  k is what differs:
    # (C prefix, words, leading shape of taps per unit of depth, noun, the public methods' stem, neutral words that are not 0, whether the
    # info has a sample time)
    def _chain_rows(self, k, table, per_instance, who):
        if isinstance(table, dict):
            table = {**k[5], **table}  # the neutral words: a dict names only what it changes
        return self._sense_rows(table, k[1], per_instance, self._robot.dof(), who, "chain table")

    def _chain_attach(self, k, table, per_instance, depth, *more):
        t = None if table is None else self._chain_rows(k, table, per_instance, "attach" + k[4])
        self._call(k[0] + "_attach", None if t is None else _dptr(t), int(bool(per_instance)), int(depth), *more)

    def _chain_info(self, k, who=None):
        """the info dict; with who, that method's refusal of a detached chain"""
        v, T, nb = [C.c_int(0) for _ in range(3)], [C.c_double(0)] * k[6], C.c_size_t(0)
        self._call(k[0] + "_info", *(C.byref(x) for x in v + T + [nb]))
        info = dict(attached=bool(v[0].value), per_instance=bool(v[1].value), depth=v[2].value, **({"sample_time": T[0].value} if T else {}), state_bytes=nb.value)
        if who and not info["attached"]:
            raise capi.SaipError(f"{who}: no {k[3]} is attached (attach{k[4]})")
        return info

    def _chain_set_table(self, k, table):
        who = f"set{k[4]}Table"
        self._call(k[0] + "_set_table_host", _dptr(self._chain_rows(k, table, self._chain_info(k, who)["per_instance"], who)))

    def _chain_randomize(self, k, who, seed, round, lo, hi):
        self._chain_info(k, who)
        lo, hi = (self._plant_table(x, False, 0, self._robot.dof(), len(k[1]), who, "chain bounds") for x in (lo, hi))
        self._call(k[0] + "_randomize", int(seed) & (2**64 - 1), int(round), _dptr(lo), _dptr(hi))

    def _chain_state(self, k, who):
        n, B, d = self._robot.dof(), self.batch_size, self._chain_info(k, who)["depth"]
        taps, filt, primed = np.zeros((n,) + k[2] + (d, B)), np.empty((n, 3, B)), np.empty((n, B), np.int32)
        self._call(k[0] + "_state_host", _dptr(taps) if d else None, _dptr(filt), primed.ctypes.data_as(C.POINTER(C.c_int)))
        return dict(taps=np.ascontiguousarray(np.moveaxis(taps, -1, 0)), filt=np.ascontiguousarray(filt.transpose(2, 0, 1)), primed=np.ascontiguousarray(primed.T))

    def _chain_state_device(self, k):
        p = [C.c_void_p() for _ in range(3)]
        self._call(k[0] + "_state_device", C.byref(p[0]), C.byref(p[1]), C.byref(p[2]))
        return tuple(x.value for x in p)

    # -- actuation chain: delay line, slew-rate limit and first-order lag between the commanded torque and the plant's joint rows; its state
    # is snapshot state
    PLANT_CHAIN_WORDS = ("delay", "rate_max", "tau_lag")
    _ACTUATION_CHAIN = ("saip_batch_plant_chain", PLANT_CHAIN_WORDS, (), "actuation chain", "ActuationChain", {"rate_max": np.inf}, 0)

    def attachActuationChain(self, table=None, per_instance=False, depth=0):
        """put an actuation chain in front of the attached plant model (attachPlant() first; attachPlant() alone is a neutral carrier).
        table: (dof, 3) rows { delay, rate_max, tau_lag } (or (dof, B, 3) with per_instance), or a dict { word: scalar or (dof,) or
        (dof, B) } of the words that differ from the neutral row 0, inf, 0; None: neutral.  delay: whole control periods, 0..depth
        (depth <= 8); rate_max > 0: the largest change of the torque per second (inf: no limit); tau_lag >= 0: the time constant of a
        first-order lag in seconds (0: none).  The delay line moves once per period (integrate() call or rollout period), the rate limit
        and the lag run every substep.  The chain's state is part of saveState() / restoreState()."""
        self._chain_attach(self._ACTUATION_CHAIN, table, per_instance, depth)

    def detachActuationChain(self):
        self._call("saip_batch_plant_chain_detach")

    def actuationChainInfo(self):
        """dict attached, per_instance, depth, state_bytes (device bytes of taps, filt and primed); needs a plant model"""
        return self._chain_info(self._ACTUATION_CHAIN)

    def setActuationChainTable(self, table):
        """replace the chain table (same layout as attached); the state stays (resetActuationChain() starts afresh)"""
        self._chain_set_table(self._ACTUATION_CHAIN, table)

    def actuationChainRandomize(self, seed, round=0, lo=None, hi=None):
        """draw the per-instance chain table on the device between two (dof, 3) tables; lo == hi gives lo exactly (an infinite rate_max
        stays infinite); delay is rounded to the nearest integer and clamped to 0..depth after the draw; reproducible for (seed, round)"""
        self._chain_randomize(self._ACTUATION_CHAIN, "actuationChainRandomize", seed, round, lo, hi)

    def resetActuationChain(self):
        """the next period primes the chain again: every tap, x_held and both filters start from that period's command (enqueued, no wait)"""
        self._call("saip_batch_plant_chain_reset")

    def actuationChainState(self):
        """dict taps (B, dof, depth), filt (B, dof, 3) { x_held, y_rate, y_lag }, primed (B, dof) int (waits for the engine stream): for
        tests and debugging"""
        return self._chain_state(self._ACTUATION_CHAIN, "actuationChainState")

    def actuationChainStateDevice(self):
        """device pointers (taps, filt, primed) of the state arrays, (depth dof, ld), (3 dof, ld) float64 and (dof, ld) int32; taps is
        None at depth 0"""
        return self._chain_state_device(self._ACTUATION_CHAIN)

    def actuationChainTableDevice(self):
        """device pointer of the resident chain table, (dof, 3) or (dof, 3, ld); None when detached"""
        return capi.lib().saip_batch_plant_chain_table_device(self._h)

    # -- sensing model: offset, noise and quantisation between the resident state and what the controller reads of it (saip.h)
    SENSE_JOINT_WORDS = ("q_off", "q_res", "q_sigma", "dq_off", "dq_res", "dq_sigma")
    SENSE_AXIS_WORDS = ("off", "res", "sigma")

    def _sense_rows(self, table, names, per_instance, rows, who, what):
        """(rows, words) or (rows, B, words) from an array of that shape or from a dict { word: scalar, (rows,) or (rows, B) }"""
        B = self.batch_size
        if isinstance(table, dict):
            unknown = set(table) - set(names)
            if unknown:
                raise ValueError(f"{who}: unknown {what} words {sorted(unknown)} (known: {list(names)})")
            a = np.zeros((rows, B, len(names)) if per_instance else (rows, len(names)))
            for k, name in enumerate(names):
                if name in table:
                    v = np.asarray(table[name], float)
                    if v.ndim == 2 and not per_instance:
                        raise ValueError(f"{who}: {what} word {name}: per-instance values need per_instance=True")
                    try:
                        a[..., k] = v[:, None] if v.ndim == 1 and per_instance else v
                    except ValueError:
                        raise ValueError(f"{who}: {what} word {name}: a scalar, ({rows},) or ({rows}, {B}) expected, got {v.shape}") from None
            table = a
        return self._plant_table(table, per_instance, B, rows, len(names), who, what)

    def _sense_wrenches(self, wrenches, per_instance, who):
        """(task ids, the stacked tables laid out for the C entry or None)"""
        wrenches = {} if wrenches is None else dict(wrenches)
        ids, tabs = [], []
        for task, t in wrenches.items():
            ids.append(int(task._id if hasattr(task, "_id") else task))
            tabs.append(self._sense_rows(t, self.SENSE_AXIS_WORDS, per_instance, 6, who, "wrench table"))  # (6, 3) or (6, 3, B)
        return np.asarray(ids + [0] * (1 - min(len(ids), 1)), np.int32), len(ids), (np.ascontiguousarray(np.stack(tabs)) if tabs else None)

    def attachSensing(self, joints=None, wrenches=None, per_instance=False, seed=0):
        """put a sensing model between the resident simulator and the controller.  joints: (dof, 6) rows { q_off, q_res, q_sigma, dq_off,
        dq_res, dq_sigma } (or (dof, B, 6) with per_instance), or a dict { word: scalar or (dof,) or (dof, B) }; None: neutral (zeros).
        wrenches: { motion-force task (or its id): (6, 3) rows { off, res, sigma } per axis F then M } (or (6, B, 3), or the same kind of
        dict), at most two tasks: they perturb the sensed wrench a simulated sensor writes (contact planes, contact patches).  A measured
        value is x + off, plus sigma z when sigma > 0, rounded to a multiple of res when res > 0; z is a function of (seed, instance,
        row, period), the period counter of sensingInfo() advanced by integrate() and every rollout period.  While attached, every control
        cycle, per-task entry and internal OTG reads the measured q, dq; the simulator, the recorder and the model queries keep the true state."""
        who = "attachSensing"
        jt = None if joints is None else self._sense_rows(joints, self.SENSE_JOINT_WORDS, per_instance, self._robot.dof(), who, "joints")
        ids, S, wt = self._sense_wrenches(wrenches, per_instance, who)
        self._call("saip_batch_sensing_attach", None if jt is None else _dptr(jt), int(bool(per_instance)), S, ids.ctypes.data_as(C.POINTER(C.c_int)),
                   None if wt is None else _dptr(wt), int(bool(per_instance)), int(seed) & (2**64 - 1))

    def sensingInfo(self):
        """dict per_instance_joints, n_wrench_tasks, per_instance_wrenches, period (the period the next measurement belongs to)"""
        v = [C.c_int(0) for _ in range(3)]
        per = C.c_longlong(0)
        self._call("saip_batch_sensing_info", C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(per))
        return dict(per_instance_joints=bool(v[0].value), n_wrench_tasks=v[1].value, per_instance_wrenches=bool(v[2].value), period=per.value)

    def detachSensing(self):
        self._call("saip_batch_sensing_detach")

    def setSensingJoints(self, joints):
        """replace the joint table (same layout as attached); the next cycle takes a new measurement"""
        info = self.sensingInfo()
        a = self._sense_rows(joints, self.SENSE_JOINT_WORDS, info["per_instance_joints"], self._robot.dof(), "setSensingJoints", "joints")
        self._call("saip_batch_sensing_set_joints_host", _dptr(a))

    def setSensingWrenches(self, tables):
        """replace the wrench tables: a list of (6, 3) (or (6, B, 3)) tables in the order the tasks were attached in"""
        info = self.sensingInfo()
        tabs = [self._sense_rows(t, self.SENSE_AXIS_WORDS, info["per_instance_wrenches"], 6, "setSensingWrenches", "wrench table") for t in tables]
        if len(tabs) != info["n_wrench_tasks"]:
            raise ValueError(f"setSensingWrenches: {info['n_wrench_tasks']} tables expected, got {len(tabs)}")
        a = np.ascontiguousarray(np.stack(tabs)) if tabs else None
        self._call("saip_batch_sensing_set_wrenches_host", None if a is None else _dptr(a))

    def setSensingSeed(self, seed):
        self._call("saip_batch_sensing_seed", int(seed) & (2**64 - 1))

    def setSensingPeriod(self, period):
        """the noise's period counter, 0 <= period < 2^32; pair it with restoreState, since the counter is not part of a snapshot"""
        self._call("saip_batch_sensing_set_period", int(period))

    def sensingRandomize(self, seed, round=0, joints=None, wrenches=None):
        """draw the per-instance tables on the device: joints = (lo, hi), two (dof, 6) tables, wrenches = (lo, hi), two (S, 6, 3) tables;
        every word of every instance is uniform between its bounds (lo == hi: exactly lo), reproducibly for (seed, round); None leaves
        that table alone.  Tables attached without per_instance are refused."""
        info = self.sensingInfo()
        jl = jh = wl = wh = None
        if joints is not None:
            jl, jh = (self._plant_table(x, False, 0, self._robot.dof(), capi.SAIP_SENSE_JOINT_WORDS, "sensingRandomize", "joint bounds") for x in joints)
        if wrenches is not None:
            S = info["n_wrench_tasks"]
            wl, wh = (self._plant_table(np.asarray(x, float).reshape(-1, capi.SAIP_SENSE_WRENCH_WORDS), False, 0, S, capi.SAIP_SENSE_WRENCH_WORDS,
                                        "sensingRandomize", "wrench bounds") for x in wrenches)
        self._call("saip_batch_sensing_randomize", int(seed) & (2**64 - 1), int(round), *(None if x is None else _dptr(x) for x in (jl, jh, wl, wh)))

    def measureState(self):
        """enqueue the measurement of the resident q, dq now (a host-driven loop's first step; needed after writes through device pointers)"""
        self.sensingInfo()  # without an attachment: that error, before the device is needed
        self._push_state()
        self._call("saip_batch_sensing_measure")

    def measuredState(self):
        """(q_meas, dq_meas), each (B, dof): what the controller last read (waits for the engine stream)"""
        self.sensingInfo()
        n, B = self._robot.dof(), self.batch_size
        q, dq = np.empty((n, B)), np.empty((n, B))
        self._call("saip_batch_sensing_measured_host", _dptr(q), _dptr(dq))
        return np.ascontiguousarray(q.T), np.ascontiguousarray(dq.T)

    def sensingJointsDevice(self):
        """device pointer of the resident joint table, (dof, 6) or (dof, 6, ld); None when detached"""
        return capi.lib().saip_batch_sensing_joints_device(self._h)

    def sensingWrenchesDevice(self):
        """device pointer of the resident wrench tables, (S, 6, 3) or (S, 6, 3, ld); None when detached or without wrench tasks"""
        return capi.lib().saip_batch_sensing_wrenches_device(self._h)

    def measuredStateDevice(self):
        """device pointers (q_meas, dq_meas), each (dof, ld); (None, None) when detached"""
        L = capi.lib()
        return L.saip_batch_sensing_measured_q_device(self._h), L.saip_batch_sensing_measured_dq_device(self._h)

    # -- sensing chain: delay line, finite-difference velocity and low-pass behind the sensing model's joint rows; its state is snapshot state
    SENSE_CHAIN_WORDS = ("delay", "vel_mode", "a_q", "a_dq")
    _SENSING_CHAIN = ("saip_batch_sensing_chain", SENSE_CHAIN_WORDS, (2,), "sensing chain", "SensingChain", {}, 1)

    @staticmethod
    def sensingChainAlpha(cutoff_hz, sample_time):
        """the low-pass coefficient a = 1 - exp(-2 pi f_c sample_time) of a first-order filter with cutoff f_c (Hz) sampled every
        sample_time seconds, for the a_q / a_dq words (scalars or arrays)"""
        return 1.0 - np.exp(-2.0 * np.pi * np.asarray(cutoff_hz, float) * float(sample_time))

    def attachSensingChain(self, table=None, per_instance=False, depth=0, sample_time=1e-3):
        """put a sensing chain behind the attached sensing model (attachSensing() first; attachSensing() alone is a neutral carrier).
        table: (dof, 4) rows { delay, vel_mode, a_q, a_dq } (or (dof, B, 4) with per_instance), or a dict { word: scalar or (dof,) or
        (dof, B) }; None: neutral.  delay: whole samples, 0..depth (depth <= 8); vel_mode 1: dq is the finite difference of the delayed q
        over sample_time; a_q, a_dq in [0, 1]: y += a (x - y), 0 for no filter (sensingChainAlpha() from a cutoff).  Every measurement the
        engine takes is one sample: one per state change, one per rollout period, one per measureState().  The chain's state is part of
        saveState() / restoreState()."""
        self._chain_attach(self._SENSING_CHAIN, table, per_instance, depth, float(sample_time))

    def detachSensingChain(self):
        self._call("saip_batch_sensing_chain_detach")

    def sensingChainInfo(self):
        """dict attached, per_instance, depth, sample_time, state_bytes (device bytes of taps, filt and primed); needs a sensing model"""
        return self._chain_info(self._SENSING_CHAIN)

    def setSensingChainTable(self, table):
        """replace the chain table (same layout as attached); the state stays (resetSensingChain() starts afresh)"""
        self._chain_set_table(self._SENSING_CHAIN, table)

    def sensingChainRandomize(self, seed, round=0, lo=None, hi=None):
        """draw the per-instance chain table on the device between two (dof, 4) tables; delay and vel_mode are rounded to the nearest
        integer and clamped to 0..depth and 0..1 after the draw; reproducible for (seed, round)"""
        self._chain_randomize(self._SENSING_CHAIN, "sensingChainRandomize", seed, round, lo, hi)

    def resetSensingChain(self):
        """the next sample primes the chain again: every tap, q_prev and both filters start from that sample (enqueued, no wait)"""
        self._call("saip_batch_sensing_chain_reset")

    def sensingChainState(self):
        """dict taps (B, dof, 2, depth) { q, dq } x tap, filt (B, dof, 3) { q_prev, y_q, y_dq }, primed (B, dof) int (waits for the engine
        stream): for tests and debugging"""
        return self._chain_state(self._SENSING_CHAIN, "sensingChainState")

    def sensingChainStateDevice(self):
        """device pointers (taps, filt, primed) of the state arrays, (2 depth dof, ld), (3 dof, ld) float64 and (dof, ld) int32; taps is
        None at depth 0"""
        return self._chain_state_device(self._SENSING_CHAIN)

    def sensingChainTableDevice(self):
        """device pointer of the resident chain table, (dof, 4) or (dof, 4, ld); None when detached"""
        return capi.lib().saip_batch_sensing_chain_table_device(self._h)

    # -- plant inertia: the masses, centres of mass and inertias the resident integrator reads in place of the model's (saip.h)
    INERTIA_ROW_WORDS = ("m", "cx", "cy", "cz", "Ixx", "Iyy", "Izz", "Ixy", "Ixz", "Iyz")

    def attachInertia(self, rows=None, per_instance=False, payload_links=()):
        """give the simulated robot inertial parameters of its own: rows (dof, 10) of { m, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Ixz, Iyz } per
        movable body (COM in the body frame, inertia about it in body axes), or (dof, B, 10) with per_instance; None: the model's own rows.
        payload_links: up to 2 link names, the sites of the payloads of setInertiaParts() / randomizeInertia().  While attached,
        integrate() and rolloutAsync() integrate with the table; the controller keeps computing with the model."""
        who = "attachInertia"
        rt = None if rows is None else self._plant_table(rows, per_instance, self.batch_size, self._robot.dof(), capi.SAIP_INERTIA_ROW_WORDS, who, "rows")
        names = list(payload_links)
        links = np.zeros(max(len(names), 1), np.int32)
        for p, name in enumerate(names):
            links[p] = self._robot.linkIndex(name)
            if links[p] < 0:
                raise ValueError(f"{who}: payload {p}: unknown link [{name}]")
        self._call("saip_batch_inertia_attach", None if rt is None else _dptr(rt), int(bool(per_instance)), len(names), links.ctypes.data_as(C.POINTER(C.c_int)))

    def inertiaInfo(self):
        """dict per_instance, n_payloads, payload_bodies (the movable body of every payload site), payload_positions (P, 3) and
        payload_rotations (P, 3, 3): the site links' frames in those bodies"""
        v = [C.c_int(0), C.c_int(0)]
        bodies = (C.c_int * capi.SAIP_INERTIA_MAX_PAYLOADS)()
        frames = np.zeros((capi.SAIP_INERTIA_MAX_PAYLOADS, 12))
        self._call("saip_batch_inertia_info", C.byref(v[0]), C.byref(v[1]), bodies, _dptr(frames))
        P = v[1].value
        return dict(per_instance=bool(v[0].value), n_payloads=P, payload_bodies=[bodies[p] for p in range(P)],
                    payload_positions=frames[:P, :3].copy(), payload_rotations=frames[:P, 3:].reshape(P, 3, 3).copy())

    def detachInertia(self):
        self._call("saip_batch_inertia_detach")

    def setInertiaRows(self, rows):
        """replace the table (same shape as attached); takes effect with the next integration"""
        info = self.inertiaInfo()
        a = self._plant_table(rows, info["per_instance"], self.batch_size, self._robot.dof(), capi.SAIP_INERTIA_ROW_WORDS, "setInertiaRows", "rows")
        self._call("saip_batch_inertia_set_rows_host", _dptr(a))

    def _inertia_parts(self, x, rows, words, who, what):
        """(array in the C-ABI layout or None, per-instance flag) of a part table (rows, words) or (rows, B, words)"""
        if x is None:
            return None, 0
        a = np.asarray(x, float)
        per = a.ndim == 3
        return self._plant_table(a, per, self.batch_size, rows, words, who, what), int(per)

    def setInertiaParts(self, bodies=None, payloads=None):
        """compose the table on the device from scaled links plus payloads.  bodies: (dof, 4) of { s, dx, dy, dz } -- m' = s m, I' = s I,
        c' = c + d of the model's values -- or (dof, B, 4); None: { 1, 0, 0, 0 }.  payloads: (P, 7) of { m_p, c_p (3), hx, hy, hz }, a
        uniform box of half-extents h in the frame of its site link (attachInertia(payload_links=...)), or (P, B, 7); None: no mass."""
        info = self.inertiaInfo()
        bt, perb = self._inertia_parts(bodies, self._robot.dof(), capi.SAIP_INERTIA_BODY_WORDS, "setInertiaParts", "bodies")
        pt, perp = self._inertia_parts(payloads, info["n_payloads"], capi.SAIP_INERTIA_PAYLOAD_WORDS, "setInertiaParts", "payloads")
        self._call("saip_batch_inertia_set_parts_host", None if bt is None else _dptr(bt), perb, None if pt is None else _dptr(pt), perp)

    def randomizeInertia(self, seed, round=0, bodies=None, payloads=None):
        """draw the parts of every instance on the device and compose them: bodies = (lo, hi), two (dof, 4) tables, payloads = (lo, hi),
        two (P, 7) tables; every word is uniform between its bounds (lo == hi: exactly lo), reproducibly for (seed, round); None stands
        for the neutral words.  A table attached without per_instance is refused."""
        info = self.inertiaInfo()

        def pair(b, rows, words, what):
            if b is None:
                return None, None
            lo, hi = (self._plant_table(x, False, 0, rows, words, "randomizeInertia", what) for x in b)
            return lo, hi
        bl, bh = pair(bodies, self._robot.dof(), capi.SAIP_INERTIA_BODY_WORDS, "body bounds")
        pl, ph = pair(payloads, info["n_payloads"], capi.SAIP_INERTIA_PAYLOAD_WORDS, "payload bounds")
        self._call("saip_batch_inertia_randomize", int(seed) & (2**64 - 1), int(round), *(None if x is None else _dptr(x) for x in (bl, bh, pl, ph)))

    def inertiaRows(self):
        """the resident table read back: (dof, 10), or (dof, B, 10) when attached per instance (waits for the engine stream)"""
        info = self.inertiaInfo()
        n, W = self._robot.dof(), capi.SAIP_INERTIA_ROW_WORDS
        if not info["per_instance"]:
            out = np.empty((n, W))
            self._call("saip_batch_inertia_rows_host", _dptr(out))
            return out
        out = np.empty((n, W, self.batch_size))
        self._call("saip_batch_inertia_rows_host", _dptr(out))
        return np.ascontiguousarray(out.transpose(0, 2, 1))

    def inertiaRowsDevice(self):
        """device pointer of the resident table, (dof, 10) or (dof, 10, ld); None when detached"""
        return capi.lib().saip_batch_inertia_rows_device(self._h)

    def rewindGoalSchedules(self):
        """the period counter of the tasks' goal schedules (task.setGoalSchedule) back to 0: the next rollout starts at the first keyframe"""
        self._call("saip_batch_goal_schedule_rewind")

    # -- resident rollout sampler: the device steps of a sampling-MPC round (task.attachSampler; saip.h)
    def seedSampler(self, seed):
        """the seed of the samplers' noise; the round counter goes back to 0"""
        self._call("saip_batch_sampler_seed", C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF))

    def perturbGoalSchedules(self):
        """rewrite the resident keyframes of every sampled task around its nominal plan (one launch); advances the round counter"""
        self._call("saip_batch_sampler_perturb")

    def rolloutCost(self, summary_weights=None, target=None, path_weight=0, final_weight=0):
        """one cost per instance on the device from what the recorder holds: sum_r summary_weights[r] * rolloutSummary()[:, r]
        + path_weight * sum over the logged samples of |position - target|^2 + final_weight * |last logged position - target|^2"""
        w = t = None
        if summary_weights is not None:
            w = np.ascontiguousarray(summary_weights, float)
            if w.shape != (capi.SAIP_RECORD_SUMMARY_ROWS,):
                raise ValueError(f"rolloutCost: {capi.SAIP_RECORD_SUMMARY_ROWS} summary weights expected, got shape {w.shape}")
        if target is not None:
            t = np.ascontiguousarray(target, float)
            if t.shape != (3,):
                raise ValueError(f"rolloutCost: a target of shape (3,) expected, got {t.shape}")
        self._call("saip_batch_sampler_cost", None if w is None else _dptr(w), None if t is None else _dptr(t), float(path_weight), float(final_weight))

    def setRolloutCost(self, cost):
        """upload (B,) costs in place of rolloutCost() (NaN and +-inf mark an instance as invalid)"""
        c = np.ascontiguousarray(cost, float)
        if c.shape != (self.batch_size,):
            raise ValueError(f"setRolloutCost: {self.batch_size} costs expected, got shape {c.shape}")
        self._call("saip_batch_sampler_set_cost_host", _dptr(c))

    def getRolloutCost(self):
        """(B,) the costs on the device (waits for the engine stream)"""
        out = np.empty(self.batch_size)
        self._call("saip_batch_sampler_get_cost_host", _dptr(out))
        return out

    def updateSampler(self, temperature):
        """softmin-weighted update of every sampled task's nominal plan from the costs (MPPI; a tiny temperature takes the best);
        writes samplerResult() and the "best" source map of restoreState on the device.  Asynchronous."""
        self._call("saip_batch_sampler_update", float(temperature))

    def shiftSampler(self, n):
        """nominal[k] <- nominal[min(k + n, K - 1)]: the warm start of a receding horizon"""
        self._call("saip_batch_sampler_shift", int(n))

    def samplerResult(self):
        """dict best, n_valid, min_cost, sum_w, ess of the last updateSampler() (waits for the engine stream)"""
        best, nv = C.c_int(0), C.c_int(0)
        mc, sw, ess = C.c_double(0), C.c_double(0), C.c_double(0)
        self._call("saip_batch_sampler_result_host", C.byref(best), C.byref(nv), C.byref(mc), C.byref(sw), C.byref(ess))
        return dict(best=best.value, n_valid=nv.value, min_cost=mc.value, sum_w=sw.value, ess=ess.value)

    # -- scenario groups: B = C * M instances as C candidate plans rolled out in M scenarios each (saip.h)
    _SAMPLER_RISKS = {"mean": capi.SAIP_SAMPLER_RISK_MEAN, "max": capi.SAIP_SAMPLER_RISK_MAX, "cvar": capi.SAIP_SAMPLER_RISK_CVAR}

    def setSamplerScenarios(self, n_scenarios, risk="mean", alpha=None):
        """make the batch n_scenarios blocks of C = B / n_scenarios candidate plans (instance i = s * C + c): perturbGoalSchedules()
        gives candidate c the same keyframes in every block, updateSampler() folds the scenario costs of a candidate into one group
        cost under `risk` -- "mean", "max" (the worst scenario) or "cvar" (the mean of the worst ceil(alpha * M) scenarios, alpha in
        (0, 1]) -- and updates the plan over candidates.  n_scenarios = 1 is the ungrouped sampler."""
        if risk not in self._SAMPLER_RISKS:
            raise ValueError(f"setSamplerScenarios: unknown risk {risk!r} (one of {sorted(self._SAMPLER_RISKS)})")
        M, tail = int(n_scenarios), 0
        if risk == "cvar":
            if alpha is None or not (0.0 < float(alpha) <= 1.0):
                raise ValueError(f"setSamplerScenarios: risk \"cvar\" needs alpha in (0, 1], got {alpha!r}")
            tail = min(M, max(1, math.ceil(float(alpha) * M)))
        elif alpha is not None:
            raise ValueError(f"setSamplerScenarios: alpha = {alpha!r} applies to risk \"cvar\" only, not to {risk!r}")
        self._call("saip_batch_sampler_set_scenarios", M, self._SAMPLER_RISKS[risk], tail)

    def samplerScenarios(self):
        """dict n_scenarios, n_candidates, risk ("mean" / "max" / "cvar"), tail (the scenarios CVAR averages, else 0)"""
        m, c, r, t = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._call("saip_batch_sampler_scenarios_info", C.byref(m), C.byref(c), C.byref(r), C.byref(t))
        names = {v: k for k, v in self._SAMPLER_RISKS.items()}
        return dict(n_scenarios=m.value, n_candidates=c.value, risk=names[r.value], tail=t.value)

    def samplerGroupCost(self):
        """(C,) the group cost per candidate of the last updateSampler() (waits for the engine stream); without scenario groups
        the per-instance costs themselves"""
        out = np.empty(self.samplerScenarios()["n_candidates"])
        self._call("saip_batch_sampler_get_group_cost_host", _dptr(out))
        return out

    def shareScenarioTables(self):
        """every resident per-instance table a randomize*() call can fill (plant, actuation chain, inertia, sensing, sensing chain):
        column i takes column (i // C) * C, so that scenario s is the same simulated robot for every candidate.  Returns the number
        of arrays touched.  Asynchronous."""
        n = C.c_int(0)
        self._call("saip_batch_sampler_share_scenario_tables", C.byref(n))
        return n.value

    # -- state snapshots: the complete per-instance state, saved on the device and written back through a source index (saip.h)
    def saveState(self, snapshot=None):
        """capture the complete resident state of every instance (robot state, torques, goals, integrators, internal OTGs, singularity
        and passivity state) into `snapshot`, or into a new StateSnapshot; asynchronous on the engine stream.  Returns the snapshot."""
        self._push_state()
        if snapshot is None:
            snapshot = StateSnapshot(self)
        elif snapshot._ctrl is not self:
            raise ValueError("saveState: the snapshot belongs to another controller")
        self._call("saip_batch_snapshot_save", snapshot._handle())
        return snapshot

    def restoreState(self, snapshot, source=None):
        """instance i takes the state instance source[i] had when `snapshot` was saved.  source: None (every instance its own), an int
        (that instance's state into all), a sequence / NumPy int array of B indices (checked on the host), or a torch int32 device
        tensor of B indices read in stream order (an entry outside 0 .. B-1 leaves that instance as it is), or "best": the map the last
        updateSampler() left on the device.  Asynchronous.  The rollout
        recorder and the goal schedules are not part of a snapshot: pair with resetRolloutRecorder() / rewindGoalSchedules()."""
        if not isinstance(snapshot, StateSnapshot) or snapshot._ctrl is not self:
            raise ValueError("restoreState: the snapshot belongs to another controller")
        B, h = self.batch_size, snapshot._handle()
        if source is None:
            self._call("saip_batch_snapshot_restore", h, None)
        elif isinstance(source, str):
            if source != "best":
                raise ValueError(f"restoreState: unknown source {source!r} (the only named source is \"best\")")
            ptr = capi.lib().saip_batch_sampler_best_map_device(self._h)
            if not ptr:
                raise capi.SaipError("restoreState: source \"best\" needs a sampler (task.attachSampler)")
            self._call("saip_batch_snapshot_restore_device", h, C.c_void_p(ptr))
        elif hasattr(source, "data_ptr") and getattr(source, "is_cuda", False):
            import torch
            if source.dtype != torch.int32 or source.numel() != B or not source.is_contiguous():
                raise ValueError(f"restoreState: a contiguous int32 device tensor of {B} indices expected")
            self._call("saip_batch_snapshot_restore_device", h, C.c_void_p(source.data_ptr()))
        else:
            src = np.asarray(source.cpu() if hasattr(source, "cpu") else source)
            if src.dtype.kind not in "iu":
                raise ValueError("restoreState: integer source indices expected")
            if src.ndim == 0:
                src = np.full(B, int(src))
            if src.shape != (B,):
                raise ValueError(f"restoreState: {B} source indices expected, got shape {src.shape}")
            if ((src < 0) | (src >= B)).any():
                raise ValueError(f"restoreState: source indices must lie in 0 .. {B - 1}")
            src = np.ascontiguousarray(src, dtype=np.int32)
            self._call("saip_batch_snapshot_restore", h, src.ctypes.data_as(C.POINTER(C.c_int)))
        self._pushed_version = self._robot._state_version  # the device holds the restored state, not the SaiModel mirror (pullState reads it back)

    # -- rollout recorder: per-period trajectory log and running summaries of rolloutAsync, kept on the device (saip.h)
    _REC_CHANNELS = {"q": capi.SAIP_RECORD_Q, "dq": capi.SAIP_RECORD_DQ, "tau": capi.SAIP_RECORD_TAU, "pose": capi.SAIP_RECORD_POSE,
                     "error": capi.SAIP_RECORD_ERROR}

    def recordRollouts(self, capacity: int, stride: int = 1, channels=("q", "dq", "tau"), task=None, summaries: bool = False):
        """attach a recorder to the rollouts of this controller: every stride-th period is sampled into a ring of the last `capacity`
        samples.  channels: any of "q", "dq", "tau", "pose", "error" (the last two of `task`, a MotionForceTask of this controller or
        its name).  summaries: running per-instance summaries over every period (rolloutSummary)."""
        mask = 0
        for c in channels:
            if c not in self._REC_CHANNELS:
                raise ValueError(f"recordRollouts: unknown channel {c!r} (one of {sorted(self._REC_CHANNELS)})")
            mask |= self._REC_CHANNELS[c]
        if isinstance(task, str):
            task = self.getMotionForceTaskByName(task)
        if task is not None and task not in self._tasks:
            raise ValueError("recordRollouts: the task does not belong to this controller")
        self._call("saip_batch_rollout_recorder_attach", int(capacity), int(stride), mask, -1 if task is None else task._id, int(bool(summaries)))
        self._rec_mask = mask

    def stopRecordingRollouts(self):
        self._call("saip_batch_rollout_recorder_detach")
        self._rec_mask = 0

    def resetRolloutRecorder(self):
        """period counter back to 0, log emptied, summaries zeroed"""
        self._call("saip_batch_rollout_recorder_reset")

    def rolloutLog(self):
        """the samples in chronological order: dict of (n, B, dof) arrays "q", "dq", "tau", (n, B, 3) "position", (n, B, 3, 3) "orientation",
        (n, B, 3) "position_error" and "orientation_error" for the recorded channels, plus "status" (n, B) and "period" (n,)"""
        L = capi.lib()
        n, rows, first, stride = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._call("saip_batch_rollout_log_info", C.byref(n), C.byref(rows), C.byref(first), C.byref(stride))
        n, rows, B, dof = n.value, rows.value, self.batch_size, self._robot.dof()
        out, st = np.zeros((n, rows, B)), np.zeros((n, B), np.uint8)
        if n:
            self._call("saip_batch_rollout_log_host", _dptr(out), st.ctypes.data_as(C.POINTER(C.c_ubyte)))
        # the rows of a sample: the recorded channels in the order of their bits
        log = {"status": st, "period": first.value + stride.value * np.arange(n)}
        at = 0
        widths = {"q": dof, "dq": dof, "tau": dof, "pose": 12, "error": 6}
        for name in ("q", "dq", "tau", "pose", "error"):
            if not (self._rec_mask & self._REC_CHANNELS[name]):
                continue
            blk = out[:, at:at + widths[name]].transpose(0, 2, 1)
            at += widths[name]
            if name == "pose":
                log["position"] = blk[:, :, :3].copy()
                log["orientation"] = blk[:, :, 3:].reshape(n, B, 3, 3).copy()
            elif name == "error":
                log["position_error"] = blk[:, :, :3].copy()
                log["orientation_error"] = blk[:, :, 3:].copy()
            else:
                log[name] = blk.copy()
        assert at == rows
        return log

    def rolloutSummary(self):
        """(B, 8): sum T tau.tau, sum T |e_pos|^2, sum T |e_ori|^2, max |e_pos|, max |e_ori|, max |tau_j|, max |dq_j|, periods with
        status != 0 (saip.h)"""
        out = np.empty((capi.SAIP_RECORD_SUMMARY_ROWS, self.batch_size))
        self._call("saip_batch_rollout_summary_host", _dptr(out))
        return out.T.copy()

    def setTorques(self, tau):
        """overwrite the resident torques the next integrate() applies: (B, dof)"""
        a = _soa(np.asarray(tau, float), self.batch_size, self._robot.dof(), "torques")
        self._call("saip_batch_set_torques_host", _dptr(a))

    # -- robot-model queries at the RESIDENT state (what integrate() / rolloutAsync() left on the device, or the state last pushed)
    def getModelFrames(self, frames, jacobian=False, world=False, out=None):
        """kinematics of up to 8 frames in one launch: frames = [link or (link, pos_in_link)], links by name or index.  Returns
        (n_frames, rows, B): rows 0-2 position, 3-11 rotation (row-major), 12-14 linear velocity, 15-17 angular velocity, then with
        jacobian the 6 x dof [Jv; Jw] row-major; robot base frame, or through TRobotBase() with world.  out: a contiguous float64
        device tensor of shape (n_frames, rows, ld) or a raw device pointer: written asynchronously on the batch stream"""
        flags = (capi.SAIP_QUERY_JACOBIAN if jacobian else 0) | (capi.SAIP_QUERY_WORLD if world else 0)
        return _model_frames(self._h, self._robot, frames, flags, out)

    def getModelDynamics(self, out=None):
        """M, M_inv (B, dof, dof), g, b (B, dof) at the resident state: dict.  out: {key: device tensor of shape (dof*dof or dof, ld) or
        pointer} for any of the keys "M", "M_inv", "g", "b" (the others are not computed), written asynchronously on the batch stream"""
        return _model_dynamics(self._h, self._robot, _DYN_KEYS, out)

    def pullState(self):
        """read the resident state back into the SaiModel mirror (after integrate / rolloutAsync); returns (q, dq) (B, dof)"""
        r = self._robot
        n, B = r.dof(), self.batch_size
        q, dq = np.empty((n, B)), np.empty((n, B))
        self._call("saip_batch_get_state_host", _dptr(q), _dptr(dq))
        r._q, r._dq = q.T.copy(), dq.T.copy()
        r._state_version += 1
        self._pushed_version = r._state_version  # the device already holds this state
        return r._q, r._dq

    def synchronize(self):
        self._call("saip_batch_synchronize")

    def getTorques(self):
        n, B = self._robot.dof(), self.batch_size
        tau = np.empty((n, B))
        st = np.zeros(B, np.uint8)
        capi.check(capi.lib().saip_batch_get_torques_host(self._h, _dptr(tau), st.ctypes.data_as(C.POINTER(C.c_ubyte))))
        self.status = st
        return tau.T.copy()

    def timeSteps(self, steps: int, warmup: int = 0) -> float:
        ms = C.c_double(0)
        capi.check(capi.lib().saip_batch_time_steps(self._h, steps, warmup, C.byref(ms)))
        return ms.value

    def timeStepsBegin(self, steps: int):
        """enqueue `steps` cycles between two HIP events on the engine stream and return without waiting (saip_batch_time_steps_begin)"""
        capi.check(capi.lib().saip_batch_time_steps_begin(self._h, int(steps)))

    def timeStepsEnd(self) -> float:
        """event time (ms) of the cycles timeStepsBegin enqueued; call it behind the caller's own wait for the device"""
        ms = C.c_double(0)
        capi.check(capi.lib().saip_batch_time_steps_end(self._h, C.byref(ms)))
        return ms.value

    def timeStepsGather(self, steps: int, comm=None, gathered_ptr=None, every_step: bool = False):
        """(elapsed_ms, gather_ms) of `steps` cycles with the torque all-gather inside the timed region (saip_batch_time_steps_gather): one gather
        behind the last cycle, or one behind every cycle; comm None (one rank) issues no collective"""
        e, g = C.c_double(0), C.c_double(0)
        capi.check(capi.lib().saip_batch_time_steps_gather(self._h, comm, C.c_void_p(gathered_ptr) if gathered_ptr else None, int(steps),
                                                           1 if every_step else 0, C.byref(e), C.byref(g)))
        return e.value, g.value

    def devicePointers(self):
        L = capi.lib()
        return dict(q=L.saip_batch_device_q(self._h), dq=L.saip_batch_device_dq(self._h), tau=L.saip_batch_device_tau(self._h),
                    status=L.saip_batch_device_status(self._h), ld=L.saip_batch_ld(self._h), stream=L.saip_batch_stream(self._h))

    def bindTauDevice(self, ptr):
        self._call("saip_batch_bind_tau_device", C.c_void_p(ptr))


class StateSnapshot:
    """A device-resident copy of the complete state of a RobotController's instances (RobotController.saveState / restoreState)."""
    KINDS = {capi.SAIP_SNAPSHOT_SOA: "soa", capi.SAIP_SNAPSHOT_GROUPED: "grouped", capi.SAIP_SNAPSHOT_AOS: "aos"}

    def __init__(self, controller):
        h = C.c_void_p()
        controller._call("saip_batch_snapshot_create", C.byref(h))
        self._h, self._ctrl = h, controller

    def _handle(self):
        if not self._h:
            raise capi.SaipError("the StateSnapshot has been closed")
        return self._h

    def segments(self):
        """the layout: a list of dicts name, rows, elem_bytes, group, kind ("soa" rows x [ld], "grouped" rows x [B * group], "aos" [ld]
        records), offset (of the segment inside tobytes())"""
        L, out = capi.lib(), []
        for i in range(L.saip_snapshot_segments(self._handle())):
            name, rows, eb, grp, kind, off = C.c_char_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
            capi.check(L.saip_snapshot_segment_info(self._h, i, C.byref(name), C.byref(rows), C.byref(eb), C.byref(grp), C.byref(kind), C.byref(off)))
            out.append(dict(name=name.value.decode(), rows=rows.value, elem_bytes=eb.value, group=grp.value, kind=self.KINDS[kind.value], offset=off.value))
        return out

    def nbytes(self):
        return capi.lib().saip_snapshot_bytes(self._handle())

    def tobytes(self):
        """the snapshot as a host blob (waits for the engine stream): header with magic, format version and layout fingerprint, then
        the segments.  Not a stable format across versions of the library."""
        buf = np.empty(self.nbytes(), np.uint8)
        self._ctrl._call("saip_snapshot_export_host", self._handle(), buf.ctypes.data_as(C.c_void_p), buf.size)
        return buf.tobytes()

    @classmethod
    def frombytes(cls, controller, data):
        """a new snapshot of `controller` filled from a blob of tobytes(); the controller must have the layout the blob was taken from
        (same robot, batch size and task stack with the same features enabled), else ValueError"""
        snap = cls(controller)
        buf = np.frombuffer(bytes(data), np.uint8)
        try:
            controller._call("saip_snapshot_import_host", snap._h, buf.ctypes.data_as(C.c_void_p), buf.size)
        except Exception:
            snap.close()
            raise
        return snap

    def close(self):
        if getattr(self, "_h", None):
            capi.lib().saip_snapshot_destroy(self._h)  # (valid after the batch is gone too: the batch frees the device memory then)
            self._h = None

    def __del__(self):
        self.close()


def controller_from_specs(description, tasks, batch_size, device=0, *, disable_otg=True, leading_dimension=None):
    """Build (robot, controller, task objects) from workloads.py-style task specs (used by tests and bench)."""
    robot = SaiModel(description, batch_size, device)
    objs = tasks_from_specs(robot, tasks, disable_otg=disable_otg)
    ctrl = RobotController(robot, objs, leading_dimension=leading_dimension)
    return robot, ctrl, objs


def tasks_from_specs(robot, tasks, *, disable_otg=True):
    """task objects (not yet in any RobotController) from workloads.py-style task specs"""
    objs = []
    for t in tasks:
        if t["type"] == "motion_force":
            o = MotionForceTask(robot, t["link"], t["pos_in_link"], t.get("rot_in_link"), t.get("dirs_trans"), t.get("dirs_rot"),
                                task_name=t["name"], loop_timestep=t.get("dt", 0.001),
                                is_force_motion_parametrization_in_compliant_frame=t.get("param_in_compliant_frame", False))
            o.setPosControlGains(t["kp_pos"], t["kv_pos"], t["ki_pos"])
            o.setOriControlGains(t["kp_ori"], t["kv_ori"], t["ki_ori"])
            o.setSingularityHandlingBounds(t["s_min"], t["s_max"])
            if not t.get("singularity_handling", True):
                o.disableSingularityHandling()
            o.setSingularityStrategies(bool(t.get("singularity_strategies", True)))
            if "sh_gains" in t:
                o.setSingularityHandlingGains(*t["sh_gains"])
            if t.get("sh_all_type1", False):
                o.handleAllSingularitiesAsType1(True)
            if t.get("cl_force") or t.get("cl_moment"):
                o.setForceControlParameters(t.get("kff_force", 0.95), t.get("kff_moment", 0.95), t.get("max_force_fb", 20.0), t.get("max_moment_fb", 10.0))
                o.setControlToSensorTransform(t.get("Rcs", np.eye(3)), t.get("tcs", np.zeros(3)))
                o.setClosedLoopForceControl(bool(t.get("cl_force")))
                o.setClosedLoopMomentControl(bool(t.get("cl_moment")))
                if t.get("passivity"):
                    o.enablePassivity()
            o.setForceControlGains(t.get("kp_force", 0.7), t.get("kv_force", 10.0), t.get("ki_force", 1.3))
            o.setMomentControlGains(t.get("kp_moment", 0.7), t.get("kv_moment", 10.0), t.get("ki_moment", 1.3))
            if t.get("force_dim", 0):
                o.parametrizeForceMotionSpaces(t["force_dim"], t.get("force_axis"))
            if t.get("moment_dim", 0):
                o.parametrizeMomentRotMotionSpaces(t["moment_dim"], t.get("moment_axis"))
            if t.get("vel_sat", False):
                o.enableVelocitySaturation(t["lin_sat"], t["ang_sat"])
        else:
            S = t["S"]
            if S is not None:
                S = np.asarray(S, float)
                if S.ndim == 1:
                    rows = [int(i) for i in S]
                    S = np.zeros((len(rows), robot.dof()))
                    S[np.arange(len(rows)), rows] = 1.0
            o = JointTask(robot, S, task_name=t["name"], loop_timestep=t.get("dt", 0.001))
            o.setGains(t["kp"], t["kv"], t["ki"])
            if t.get("vel_sat", False):
                o.enableVelocitySaturation(t["sat"])
        o.setDynamicDecouplingType(t["decoupling"])
        o.setBoundedInertiaEstimateThreshold(t["bie_threshold"])
        if disable_otg:
            o.disableInternalOtg()
        objs.append(o)
    return objs
