"""The exact dynamics oracle tests/dynamics_ref.py earns its place (CPU only): its double evaluation against its long-double evaluation,
against the finite-difference oracle oracle/restatement.forward_dynamics and against the mass matrices of workloads.py / tests/trees.py;
the residual check on the oracle's own solution; and the residual check's teeth -- four subtly wrong models it must tell from the right
one at the bound the device tests assert (test_gpu_dynamics_exact.BOUND = 8, in units of n eps).

Inputs of every test here: seed 20 + the robot's dof, q uniform inside the joint limits (clipped to +-2.5), |dq| <= 3 rad/s, tau uniform in
+-5, g = (1.3, -2.1, -9.0), dt = 2^-6; B = 6 (chain30: 3)."""
import copy

import numpy as np
import pytest

import chains as CH  # noqa: F401  (tests/trees.py builds on it)
import dynamics_ref as DR
import inertia_ref as IR
import restatement as RS
import trees as TR
import workloads as W

BOUND = 8.0                        # the bound of tests/test_gpu_dynamics_exact.py
G_TILTED = (1.3, -2.1, -9.0)
DT = 2.0 ** -6
ROBOTS = ["panda_arm", "panda_sliding_base", "chain30", "dual_panda_fixed_torso", "dual_panda_torso", "random12_9"]
_TREES = {"dual_panda_fixed_torso": TR.dual_panda_fixed_torso, "dual_panda_torso": TR.dual_panda_torso, "random12_9": lambda: TR.random_tree(12, 9)}


def _robot(name):
    """(workloads.RobotModel, is a tree)"""
    if name in _TREES:
        return W.RobotModel(_TREES[name]()), True
    return W.load_robot(name), False


def _inputs(m, B):
    rng = np.random.default_rng(20 + m.dof)
    q = rng.uniform(np.maximum(m.q_lower, -2.5), np.minimum(m.q_upper, 2.5), (B, m.dof))
    return q, rng.uniform(-3.0, 3.0, (B, m.dof)), rng.uniform(-5.0, 5.0, (B, m.dof))


@pytest.fixture(scope="module")
def cases():
    """per robot, computed once: the inputs and the bias in both precisions"""
    memo = {}

    def get(name):
        if name not in memo:
            m, tree = _robot(name)
            q, dq, tau = _inputs(m, 3 if name == "chain30" else 6)
            md = DR.Model(m)
            memo[name] = dict(m=m, tree=tree, md=md, q=q, dq=dq, tau=tau, h64=DR.bias(md, q, dq, G_TILTED, np.complex128),
                              hld=DR.bias(md, q, dq, G_TILTED, np.clongdouble))
        return memo[name]
    return get


@pytest.mark.parametrize("name", ROBOTS)
def test_double_agrees_with_long_double(cases, name):
    """|h(complex128) - h(clongdouble)| <= 64 eps H per row (measured: 0.73 .. 4.7 over the six robots); H itself is the same in both to
    rounding"""
    c = cases(name)
    (h, H), (hl, Hl) = c["h64"], c["hld"]
    ratio = float((np.abs(h - hl) / (DR.EPS * Hl)).max())
    print(f"{name}: complex128 against clongdouble, worst |dh| / (eps H) = {ratio:.3g}, max abs difference {float(np.abs(h - hl).max()):.2e} for |h| up to {np.abs(h).max():.0f}")
    assert ratio <= 64.0
    assert np.abs(H - Hl).max() <= 64 * DR.EPS * np.abs(Hl).max()
    assert (Hl >= np.abs(hl)).all()


@pytest.mark.parametrize("name", ROBOTS)
def test_agrees_with_the_finite_difference_oracle(cases, name):
    c = cases(name)
    for grav, damping in ((G_TILTED, 0.0), ((0.0, 0.0, 0.0), 0.3)):
        mine = DR.forward_dynamics(c["md"], c["q"], c["dq"], c["tau"], grav, damping, np.float64)
        with (TR.tree_oracle() if c["tree"] else _plain()) as rs:
            ref = rs.forward_dynamics(c["m"], c["q"], c["dq"], c["tau"], g=grav, damping=damping)
        err = np.abs(mine - ref).max() / max(1.0, np.abs(mine).max())
        print(f"{name}: finite-difference oracle against the exact one, gravity {grav}: {err:.2e} relative")
        assert err < 1e-8


class _plain:
    def __enter__(self):
        return RS

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize("name", ROBOTS)
def test_mass_matrix_matches_the_existing_ones(cases, name):
    c = cases(name)
    m, q = c["m"], c["q"]
    want = TR.tree_mass_matrix(m, TR.tree_fk(m, q)) if c["tree"] else W.mass_matrix(m, W.fk(m, q))
    M, Mabs = DR.mass_matrix(c["md"], q, np.float64, with_abs=True)
    Ml = DR.mass_matrix(c["md"], q, np.longdouble)
    assert np.abs(M - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    assert (np.abs(M - Ml) <= 64 * DR.EPS * Mabs).all() and (Mabs >= np.abs(M) * (1 - 1e-12)).all()
    U = DR.potential_energy(c["md"], q, G_TILTED)
    with (TR.tree_oracle() if c["tree"] else _plain()) as rs:
        E = rs.total_energy(m, q, np.zeros_like(q), g=G_TILTED)
    assert np.abs(U - E).max() <= 1e-13 * max(1.0, np.abs(E).max())


@pytest.mark.parametrize("name", ["panda_arm", "panda_sliding_base", "chain30", "dual_panda_torso"])
def test_residual_of_the_oracles_own_solution(cases, name):
    """float64 np.linalg.solve on the oracle's own M and h, fed back as dq1 = dq0 + dt qdd: at most 1 n eps"""
    c = cases(name)
    for grav, damping in ((G_TILTED, 0.0), ((0.0, 0.0, 0.0), 0.3)):
        qdd = DR.forward_dynamics(c["md"], c["q"], c["dq"], c["tau"], grav, damping, np.float64)
        val, b, i = DR.residual_check(c["md"], c["q"], c["dq"], c["dq"] + DT * qdd, c["tau"], DT, grav, damping)
        print(f"{name}: residual of the oracle's own double solution, gravity {grav}: {val:.3g} n eps (instance {b}, row {i})")
        assert val <= 1.0
        # and the check does see a plainly wrong step
        bad = qdd.copy()
        bad[:, 0] *= 1 + 1e-9
        assert DR.residual_check(c["md"], c["q"], c["dq"], c["dq"] + DT * bad, c["tau"], DT, grav, damping)[0] > 1e3


# ------------------------------------------------------------------ teeth
# The Panda at the inputs of _inputs() (seed 27, B = 6, |dq| <= 3, g = (1.3, -2.1, -9.0), tau in +-5, dt = 2^-6, no damping): the wrong
# model's exact acceleration (long double), stored as dq1 in double, against the right model.  Residuals measured with these inputs, in
# n eps: centre of mass 6.4e4, product of inertia 4.0e4, parallel-axis term 2.7e10, gravity's x 5.0e13 (the right model's own acceleration:
# below 0, under the recovery term); none needed a larger |dq| or a steeper tilt to clear the bound of 8.
def _panda_desc():
    m = W.load_robot("panda_arm")
    return dict(name=m.name, links=copy.deepcopy(m.links))


def _com_shifted():
    d = _panda_desc()
    d["links"][3]["com"][0] += 1e-9                                       # link4's centre of mass, 1 nm along x
    return d


def _product_of_inertia_changed():
    d = _panda_desc()
    l = d["links"][4]                                                     # link5: Ixy by 1e-9 of its largest moment
    l["inertia"][3] += 1e-9 * max(l["inertia"][:3])
    return d


PAYLOAD = np.array([[2.0, 0.01, -0.02, 0.1, 0.05, 0.04, 0.03]])           # 2 kg box in the hand, off the link's own centre of mass


def _with_payload(drop_parallel_axis):
    base = _panda_desc()
    d = IR.instance_description(base, IR.neutral_bodies(7), PAYLOAD, ["end-effector"])
    if drop_parallel_axis:                                                # the payload's own m_p PA(c_p - c) left out of the link's inertia
        l = d["links"][[x["name"] for x in d["links"]].index("end-effector")]
        pa = IR.parallel_axis((PAYLOAD[0, 1:4] - np.asarray(l["com"], float))[None])[0]
        l["inertia"] = [float(x - PAYLOAD[0, 0] * p) for x, p in zip(l["inertia"], pa)]
    return d


TEETH = {"com shifted by 1e-9 m": (lambda: _panda_desc(), _com_shifted, G_TILTED, G_TILTED),
         "product of inertia changed by 1e-9": (lambda: _panda_desc(), _product_of_inertia_changed, G_TILTED, G_TILTED),
         "payload's parallel-axis term dropped": (lambda: _with_payload(False), lambda: _with_payload(True), G_TILTED, G_TILTED),
         "gravity's x component dropped": (lambda: _panda_desc(), lambda: _panda_desc(), G_TILTED, (0.0, G_TILTED[1], G_TILTED[2]))}


@pytest.mark.parametrize("what", sorted(TEETH))
def test_residual_check_has_teeth(what):
    right, wrong, g_right, g_wrong = TEETH[what]
    md, bad = DR.Model(W.RobotModel(right())), DR.Model(W.RobotModel(wrong()))
    q, dq, tau = _inputs(W.load_robot("panda_arm"), 6)
    own = DR.forward_dynamics(md, q, dq, tau, g_right, 0.0, np.longdouble)
    ok = DR.residual_check(md, q, dq, dq + DT * own.astype(float), tau, DT, g_right, 0.0)[0]
    qdd = DR.forward_dynamics(bad, q, dq, tau, g_wrong, 0.0, np.longdouble)
    val, b, i = DR.residual_check(md, q, dq, dq + DT * qdd.astype(float), tau, DT, g_right, 0.0)
    print(f"{what}: residual {val:.3g} n eps (instance {b}, row {i}); the right model's own acceleration: {ok:.3g}")
    assert ok <= 1.0
    assert val > BOUND
