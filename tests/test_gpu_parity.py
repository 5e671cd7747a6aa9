"""Parity of the HIP path (through the C ABI) with the reference / oracle.

Tolerances: the march record (gvl, evl, ivl, flags, cell-steps) is integer /
float32 work reproduced bit for bit; image and I_ang are float64 sums whose
order differs (atomics, shuffle tree) and whose exp() comes from a different
libm: gate 1e-5 rel-L2 (BASELINE.json north_star).  Expected: ~1e-8 with emission
(the kernel takes the source function es/gs once per sub-segment where the CPU
divides two float32 products per frequency: relative difference < 1.2e-7 per term),
~1e-14 in the seeded gain-only mode.
"""
import importlib

import numpy as np
import pytest

from conftest import rel_l2
from element_gate import DEFAULT_TIER, TIGHT_TIER, contribution_counts, counts_from_oracle, gate_outputs

rt = importlib.import_module("raytrace-miniapp_amd")
pytestmark = pytest.mark.gpu

TOL = 1e-5          # north_star gate
TOL_TIGHT = 2e-7    # one float rounding of es/gs per sub-segment (frequency kernel); seeded gain-only mode stays ~1e-14


def _check_probe(hip_probe, ora):
    assert np.array_equal(hip_probe["steps"], ora["steps"])
    assert np.array_equal(hip_probe["flags"] & 3, ora["flags"] & 3)
    assert np.array_equal(hip_probe["ivl"], ora["ivl"])
    assert np.array_equal(hip_probe["gvl"].view(np.uint32), ora["gvl"].view(np.uint32))
    assert np.array_equal(hip_probe["evl"].view(np.uint32), ora["evl"].view(np.uint32))


def test_ase_small_image_vs_reference(hip, ase_small, ase_ref):
    with hip.Plan(ase_small) as plan:
        out = plan.set_ray_grid().run().fetch()
    assert out["failure_code"] == 0
    assert out["stats"]["n_rays"] == 399000
    assert out["stats"]["cell_steps"] == 4768067          # SURVEY.md 3.3, measured on the reference
    assert rel_l2(out["image"], ase_ref["image"]) < TOL_TIGHT
    assert rel_l2(out["I_ang"], ase_ref["I_ang"]) < TOL_TIGHT
    gate_outputs(out, ase_ref, ase_small, contribution_counts(ase_small), DEFAULT_TIER, "parity: ASE_small against ASE_small_ref_cpu.npz")
    # the reference harness' own gate against the golden image embedded in the file
    assert rel_l2(out["image"], ase_small.golden_image) < 5.2e-7


def test_ase_small_march_record_bit_exact(hip, oracle, ase_small):
    ids = np.arange(0, ase_small.n_rays_total, 37, dtype=np.int64)
    rays = ase_small.build_rays(ids)
    with hip.Plan(ase_small) as plan:
        plan.set_rays(rays).enable_probe().run()
        out = plan.fetch()
        pr = plan.fetch_probe()
    ora = oracle.probe(ase_small, rays, want_Iv=False)
    _check_probe(pr, ora)
    ok = ora["err"] == 0
    assert np.array_equal(pr["ray2"]["x"][ok], ora["ray2"]["x"][ok])
    assert np.array_equal(pr["ray2"]["y"][ok], ora["ray2"]["y"][ok])
    assert out["failure_code"] == 0


def test_seed_small_image_vs_reference(hip, oracle, seed_small, seed_ref):
    with hip.Plan(seed_small) as plan:
        out = plan.set_ray_grid().run().fetch()
    assert out["failure_code"] == 0
    assert out["stats"]["n_rays"] == 7803000
    assert out["stats"]["cell_steps"] == 53573880
    assert rel_l2(out["image"], seed_ref["image"]) < TOL
    assert rel_l2(out["I_ang"], seed_ref["I_ang"]) < TOL
    gate_outputs(out, seed_ref, seed_small, counts_from_oracle(oracle, seed_small), TIGHT_TIER, "parity: seed_small against seed_small_ref_cpu.npz")
    assert rel_l2(out["image"], seed_small.golden_image) < 5.2e-7


def test_seed_small_march_record_bit_exact(hip, oracle, seed_small):
    ids = np.arange(0, seed_small.n_rays_total, 1009, dtype=np.int64)
    rays = seed_small.build_rays(ids)
    with hip.Plan(seed_small) as plan:
        plan.set_rays(rays).enable_probe().run()
        plan.fetch()
        pr = plan.fetch_probe()
    ora = oracle.probe(seed_small, rays, want_Iv=False)
    _check_probe(pr, ora)


def test_selftest_of_exact_shortcuts_on_the_device(hip):
    """The exact shortcuts of the march against the IEEE sequences on the device itself: inv_norm (rsq + Markstein
    + Newton) for every float of its range and every 256th bit pattern elsewhere; the short division sequence
    (fdiv_nr / fdiv_one_nr) for every divisor of [0.25, 4) and 2^28 operand pairs of the integrator's ranges."""
    n, bad = hip.HipLibrary.get().selftest(0)
    n_inv_norm = (0x3f880000 - 0x3f700000) + (1 << 24)
    n_one_over = 4 << 23
    assert n > n_inv_norm + n_one_over + (1 << 27)      # (pairs 96 binades apart are skipped: never the minimum)
    assert bad == 0


def test_exact_emission_mode_matches_the_cpu_loop_to_rounding(hip, oracle, ase_small, ase_ref):
    """rt_hip_plan_set_exact_emission: the CPU's per-frequency el/gl (Helper.h:549-557) instead of the
    per-sub-segment source function -- the whole ASE_small image against the reference's CPU loop
    at the level of f64 summation order and libm differences, and the default mode beside it."""
    with hip.Plan(ase_small) as plan:
        plan.set_ray_grid()
        fast = plan.run().fetch()
        exact = plan.set_exact_emission(True).run().fetch()
        again = plan.set_exact_emission(False).run().fetch()
    assert rel_l2(exact["image"], ase_ref["image"]) < 1e-11 and rel_l2(exact["I_ang"], ase_ref["I_ang"]) < 1e-11
    assert rel_l2(fast["image"], ase_ref["image"]) < TOL_TIGHT
    assert 1e-12 < rel_l2(fast["image"], exact["image"]) < TOL_TIGHT      # the two modes do differ, by a float rounding
    assert rel_l2(again["image"], fast["image"]) < 1e-13
    counts = contribution_counts(ase_small)
    gate_outputs(exact, ase_ref, ase_small, counts, TIGHT_TIER, "parity: ASE_small, exact emission, against ASE_small_ref_cpu.npz")
    gate_outputs(fast, ase_ref, ase_small, counts, DEFAULT_TIER, "parity: ASE_small, default emission before the exact run")
    gate_outputs(again, fast, ase_small, counts, "reordering", "parity: default emission after the exact run against before it")
    assert exact["stats"]["cell_steps"] == fast["stats"]["cell_steps"]
