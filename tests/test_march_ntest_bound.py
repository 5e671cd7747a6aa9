"""Two CPU checks of the reasoning behind the march shortcuts of rt_march.hip, block [C], over the synthetic tables of
tests/march_steps.py and a pixel column of the shipped file, with the instrumented copy of the oracle's march.

1. The bound behind the instance without the |n - n0| < 0.05 test (rt_plan.hip, "the largest index change a step can
   see"): no integrator step sees more than 0.24 of the largest index difference between neighbouring nodes.
2. The division-free test of the step-candidate pruning never leaves out a candidate that is below dzcap."""
import numpy as np
import pytest

import march_steps
from march_steps import BINDING_CASES, synthetic


def neighbour_dn(p):
    dn = 0.0
    for g in p.gain[1:]:
        n = g.n.reshape(g.Ny, g.Nx)
        dn = max(dn, float(np.abs(np.diff(n, axis=0)).max()), float(np.abs(np.diff(n, axis=1)).max()))
    return dn


CASES = {k: v[0] for k, v in BINDING_CASES.items()}
CASES["step_0.03"] = lambda: synthetic(lambda X, Y: 1.0 + 0.0005 * X + 0.03 * ((X >= 4) & (Y >= 4)), 30, 30)
CASES["steep"] = lambda: synthetic(lambda X, Y: 1.0 + 0.5 * np.clip(X - 2, 0, 2) + 0.5 * np.clip(Y - 2, 0, 2), 600, 600)


@pytest.mark.parametrize("case", sorted(CASES))
def test_no_step_sees_more_than_a_quarter_of_the_neighbour_difference(case):
    p = CASES[case]()
    st = march_steps.steps(p, p.build_rays())
    assert st["inner"] > 1000
    assert st["max_dn"] <= 0.24 * neighbour_dn(p) + 2e-6, (st["max_dn"], neighbour_dn(p))
    # ... and the division-free test of the step-candidate pruning never leaves out a candidate below dzcap
    assert st["prune_wrong"] == 0 and st["prunable"].sum() > 0


def test_shipped_tables_are_far_inside_the_proof(ase_small):
    dn = neighbour_dn(ase_small)
    assert 8 * 0.24 * dn <= 0.05 - 1e-5          # what rt_hip_plan_create asks for
    st = march_steps.steps(ase_small, ase_small.build_rays(np.arange(30 * 25 * 266, 31 * 25 * 266, dtype=np.int64)))
    assert st["max_dn"] <= 0.24 * dn + 2e-6 and st["n_exit"] == 0
    # h1 can be pruned in every step here, h2 and h4 in nearly every one
    assert st["prune_wrong"] == 0 and st["prunable"][0] == st["inner"] and (st["prunable"][1:] > 0.95 * st["inner"]).all()
