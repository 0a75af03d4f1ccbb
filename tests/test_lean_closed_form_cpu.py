"""Closed form of the headline stack's torques (full 6-dof MotionForceTask on 7 joints + full JointTask in its nullspace) that
the lean eight-lane kernel evaluates, restated in NumPy and checked against the literal reference path (explicit inverses, SVDs).

With G = J J^T, z spanning null(J), C = diag(max(thr - M_ii, 0)), w = J^T G^-1 F_um, p = M z, mu = z.p, s = M^-1 z:
    tau_1 = M_x (w - z (z^T M_x w) / (z^T M_x z))           M_x = M (full decoupling) or M + C (bounded inertia); J^T F_um (impedance)
    tau   = tau_1 + p ((z.ddq_d - s.tau_1) + rho (z.f)) / |z|^2
    rho   = 1 | |z|^2 / mu | mu / (mu - z^T C z + (C z)^T (M + C)^-1 (C z))
No J M^-1 J^T, no inverse of it."""
import itertools

import numpy as np
import pytest

import workloads as W
import restatement as RS

B = 48
DECS = (W.FULL_DYNAMIC_DECOUPLING, W.BOUNDED_INERTIA_ESTIMATES, W.IMPEDANCE)


def closed_form_torque(model, tasks, q, dq, goals, F_um, J):
    """one instance; F_um and J are the control law's force and the task Jacobian of the reference path (`details`)"""
    mf, jt = tasks
    n = model.dof
    M = W.mass_matrix(model, W.fk(model, q[None]))[0]
    G = J @ J.T
    Pn = np.eye(n) - J.T @ np.linalg.solve(G, J)
    z = Pn[int(np.argmax(np.sum(Pn * Pn, axis=1)))]
    w = J.T @ np.linalg.solve(G, F_um)

    def clamp(thr):
        return np.maximum(thr - np.diag(M), 0.0)

    if mf["decoupling"] == W.IMPEDANCE:
        tau1 = J.T @ F_um
    else:
        Mx = M + (np.diag(clamp(mf["bie_threshold"])) if mf["decoupling"] == W.BOUNDED_INERTIA_ESTIMATES else 0.0)
        tau1 = Mx @ (w - z * (z @ Mx @ w) / (z @ Mx @ z))
    p = M @ z
    mu = z @ p
    s = np.linalg.solve(M, z)
    zz = z @ z
    if jt["decoupling"] == W.FULL_DYNAMIC_DECOUPLING:
        rho = 1.0
    elif jt["decoupling"] == W.IMPEDANCE:
        rho = zz / mu
    else:
        c = clamp(jt["bie_threshold"])
        cz = c * z
        rho = mu / (mu - z @ cz + cz @ np.linalg.solve(M + np.diag(c), cz))
    g = np.asarray(goals[1], float)
    qd, dqd, ddqd = g[:n], g[n:2 * n], g[2 * n:]
    e = q - qd
    ie = e * jt["dt"]
    f = -jt["kp"] * e - jt["kv"] * (dq - dqd) - jt["ki"] * ie
    return tau1 + p * ((z @ ddqd - s @ tau1) + rho * (z @ f)) / zz


@pytest.fixture(scope="module")
def inputs():
    return W.make_inputs(2, B)


@pytest.mark.parametrize("thr,nclamp", [(0.0, "0"), (0.1, "1"), (1.0, ">=2")], ids=["thr0.0", "thr0.1", "thr1.0"])
@pytest.mark.parametrize("mf_dec,jt_dec", list(itertools.product(DECS, DECS)))
def test_closed_form_matches_reference_path(inputs, mf_dec, jt_dec, thr, nclamp):
    d = inputs
    model = d["model"]
    tasks = W.config_tasks(2)
    tasks[0].update(decoupling=mf_dec, bie_threshold=thr)
    tasks[1].update(decoupling=jt_dec, bie_threshold=thr)
    ref = np.empty((B, model.dof))
    got = np.empty_like(ref)
    for b in range(B):
        goals = [g[b] for g in d["goals"]]
        det = []
        ref[b] = RS.controller_step_single(model, tasks, d["q"][b], d["dq"][b], goals, details=det)
        got[b] = closed_form_torque(model, tasks, d["q"][b], d["dq"][b], goals, det[0]["F_um"], det[0]["J"])
        Mdiag = np.diag(W.mass_matrix(model, W.fk(model, d["q"][b][None]))[0])
        k = int(np.sum(thr - Mdiag > 0.0))
        assert {"0": k == 0, "1": k == 1, ">=2": k >= 2}[nclamp], (b, k)
    err = W.torque_error(got, ref)
    print("closed form vs reference path: decoupling", mf_dec, jt_dec, "threshold", thr, "err", err)
    assert err < 1e-9
