"""The period plan of the resident simulator, host side (no GPU needed): csrc/saip_period_plan.h compiled alone with g++
(tests/cpp/period_plan_host.cpp, also under ASan/UBSan) over every combination of facts -- planes and patches never both, n in {6, 7, 8},
every other fact a boolean -- and the invariants of the torque chain and of the two fused forms on the table it prints.  The invariants are
stated over the table (what a flipped fact may and may not change, what the nearest attached stage is), not as the header's formulas."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "sai-primitives_amd", "csrc", "saip_period_plan.h")
FACTS = ["planes", "patches", "plant", "link_contact", "inertia", "sensing", "goals_written", "any_otg", "tree", "n"]
PLAN = ["per_substep", "link_contact_in", "contact_in", "integrator_in", "offer_cycle_sim", "may_fuse_next_otg"]
COMMANDED, PLANT, LINK_CONTACT, PLANES, PATCHES = range(5)              # how the program prints a TauBuf


def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "period_plan_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{facts tuple: plan dict} of the plain build; the sanitizer build, run stand-alone, prints the same"""
    outs = []
    for name, extra in (("period_plan_host", []), ("period_plan_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = _build(tmp_path_factory.mktemp(name), name, extra)
        run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and not run.stderr, run.stderr
        outs.append(run.stdout)
    assert outs[0] == outs[1]
    rows = np.array([[int(w) for w in line.split()] for line in outs[0].splitlines()])
    assert rows.shape == (3 * 2 ** 7 * 3, len(FACTS) + len(PLAN))
    t = {tuple(r[:len(FACTS)]): dict(zip(PLAN, r[len(FACTS):])) for r in rows}
    assert len(t) == len(rows) and not any(f[0] and f[1] for f in t)     # every combination once, planes and patches never both
    assert {f[-1] for f in t} == {6, 7, 8}
    return t


def _f(facts):
    return dict(zip(FACTS, facts))


def _flipped(facts, name):
    f = list(facts)
    f[FACTS.index(name)] ^= 1
    return tuple(f)


def test_header_is_plain_cxx_and_listed():
    from sai_primitives_amd import capi
    src = open(HEADER).read()
    assert not re.findall(r"^\s*#\s*include", src, flags=re.M)           # nothing from HIP: nothing at all (g++ builds the program below from it)
    assert "csrc/saip_period_plan.h" in capi.HEADERS
    internal = open(os.path.join(os.path.dirname(HEADER), "saip_engine_internal.h")).read()
    assert '#include "saip_period_plan.h"' in internal and "contact_tau_cmd" not in internal


def test_every_stage_reads_the_nearest_attached_stage_in_front_of_it(table):
    for facts, plan in table.items():
        f = _f(facts)
        # the chain in order, with the buffer each attached stage writes
        chain = [("plant", PLANT if f["plant"] else None), ("link_contact", LINK_CONTACT if f["link_contact"] else None),
                 ("contact", PLANES if f["planes"] else PATCHES if f["patches"] else None)]
        for reader, upto in (("link_contact_in", 1), ("contact_in", 2), ("integrator_in", 3)):
            written = [buf for _, buf in chain[:upto] if buf is not None]
            assert plan[reader] == (written[-1] if written else COMMANDED), (f, reader)


def test_a_substep_stage_bars_both_fused_forms(table):
    for facts, plan in table.items():
        f = _f(facts)
        staged = bool(f["planes"] or f["patches"] or f["plant"] or f["link_contact"])
        assert bool(plan["per_substep"]) == staged, f
        if staged:
            assert not plan["offer_cycle_sim"] and not plan["may_fuse_next_otg"], f


def test_inertia_or_sensing_bars_both_fused_forms(table):
    for facts, plan in table.items():
        f = _f(facts)
        if f["inertia"] or f["sensing"]:
            assert not plan["offer_cycle_sim"] and not plan["may_fuse_next_otg"], f


def test_written_goals_bar_the_next_otg_and_leave_the_cycle_offer_alone(table):
    for facts, plan in table.items():
        if _f(facts)["goals_written"]:
            assert not plan["may_fuse_next_otg"], facts
        assert table[_flipped(facts, "goals_written")]["offer_cycle_sim"] == plan["offer_cycle_sim"], facts


def test_dof_and_trees(table):
    for facts, plan in table.items():
        f = _f(facts)
        if f["n"] != 7:
            assert not plan["offer_cycle_sim"] and not plan["may_fuse_next_otg"], f
        if f["tree"]:
            assert not plan["may_fuse_next_otg"], f
        assert table[_flipped(facts, "tree")]["offer_cycle_sim"] == plan["offer_cycle_sim"], f      # plan_cycle has the last word on trees


def test_the_bare_seven_dof_chain(table):
    bare = [(facts, plan) for facts, plan in table.items() if not any(facts[:6]) and facts[-1] == 7]
    assert len(bare) == 8
    for facts, plan in bare:
        f = _f(facts)
        assert bool(plan["offer_cycle_sim"]) == (not f["any_otg"]), f                               # exactly when no OTG is on
        assert bool(plan["may_fuse_next_otg"]) == (not f["goals_written"] and not f["tree"]), f     # exactly when nothing above bars it
        assert plan["link_contact_in"] == plan["contact_in"] == plan["integrator_in"] == COMMANDED and not plan["per_substep"]
    # the fused forms are offered somewhere: the invariants above are not vacuous
    assert any(p["offer_cycle_sim"] for p in table.values()) and any(p["may_fuse_next_otg"] for p in table.values())
    # and nowhere off the bare 7-dof chain
    for facts, plan in table.items():
        if plan["offer_cycle_sim"] or plan["may_fuse_next_otg"]:
            assert not any(facts[:6]) and facts[-1] == 7, facts
