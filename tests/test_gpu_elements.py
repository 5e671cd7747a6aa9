"""image and I_ang of the HIP path against oracle.image_loop ELEMENT BY ELEMENT (tests/element_gate.py): which pixel,
which frequency slot, which angle cell, whether every ray arrived -- for the whole shipped grids, every variant of the
deposit, the frequency counts where a last element goes wrong alone, ragged lists with rays on the edges of the deposit
cells, the 6 384 000-ray stand-in and random problems.

Tiers (element_gate.py): default emission mode 1e-5 per element; exact emission and the seeded (gain-only)
mode 1e-11 per element.  The deposit code is the same in exact and default emission, so the exact run of every variant
is the one that sees a deposit defect at rounding level.  Every comparison prints its measured figures
(profiles/element_parity.txt)."""
import copy
import importlib
import os

import numpy as np
import pytest

from element_gate import DEFAULT_TIER, TIGHT_TIER, counts_from_oracle, deposit_cells, gate_outputs
from test_gpu_fuzz import random_case, random_grid_case

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
pytestmark = pytest.mark.gpu


def device_runs(hip, p, rays=None):
    """[(mode, tier, outputs)] of one plan: the seeded mode once, the emission mode in its default and exact forms."""
    with hip.Plan(p) as plan:
        if rays is None:
            plan.set_ray_grid()
        else:
            plan.set_rays(rays)
        if p.seed is not None:
            return [("seeded", TIGHT_TIER, plan.run().fetch())]
        fast = plan.run().fetch()
        exact = plan.set_exact_emission(True).run().fetch()
    return [("default emission", DEFAULT_TIER, fast), ("exact emission", TIGHT_TIER, exact)]


def check(hip, oracle, p, rays, label, ref=None, counts=None, n_threads=8):
    """Both tiers of p (its whole grid, or the list `rays`) against the oracle's image loop; returns (ref, counts)."""
    if ref is None:
        ref = oracle.image_loop(p, rays, n_threads=n_threads)
    assert ref["failure_code"] == 0, (label, "the oracle reports failing rays", ref["failure_code"])
    if counts is None:
        counts = counts_from_oracle(oracle, p, rays, n_threads=n_threads)
    for mode, tier, out in device_runs(hip, p, rays):
        assert out["failure_code"] == 0, (label, mode)
        assert out["stats"]["cell_steps"] == ref["counters"]["cell_steps"], (label, mode)
        figs = gate_outputs(out, ref, p, counts, tier, f"{label} / {mode}")
        assert figs["image"]["count"] == ref["image"].size and figs["I_ang"]["count"] == ref["I_ang"].size
    return ref, counts


# ---------------------------------------------------------------------------------------------- the shipped grids
_whole = {}


@pytest.mark.parametrize("own_cells", [True, False])
@pytest.mark.parametrize("name", ["ASE_small", "seed_small"])
def test_whole_shipped_grids(hip, oracle, ase_small, seed_small, name, own_cells, monkeypatch):
    """Every ray of the file, with the own-cell shortcut of the deposit and with every cell searched (getIndex)."""
    p = ase_small if name == "ASE_small" else seed_small
    if not own_cells:
        monkeypatch.setenv("RT_HIP_NO_OWN_CELLS", "1")
    _whole[name] = check(hip, oracle, p, None, f"whole {name}, {'own cells' if own_cells else 'cells searched'}", *_whole.get(name, ()))


# ---------------------------------------------------------------------------------------------- deposit variants
def _variant(name, ase_small, seed_small):
    """(problem, ray list or None for the grid) -- the constructions of test_deposit_modes_of_the_seeded_pass and
    test_lds_layout_extremes_of_the_frequency_kernel (tests/test_gpu_edges.py), and their emission-mode counterparts."""
    rng = np.random.default_rng(7)
    if name in ("seeded_shuffled_list", "seeded_beyond_the_cache_nv300"):
        ids = np.sort(rng.permutation(seed_small.n_rays_total)[:60000]).astype(np.int64)
        if name == "seeded_shuffled_list":
            return seed_small, seed_small.build_rays(rng.permutation(ids))       # row cache keyed by distinct pixels
        wide = problem_mod.resample_frequency(seed_small, 300)                   # no room for cache rows: segmented scan
        return wide, wide.build_rays(ids[::3])
    if name == "seeded_grid_tables":
        sub = copy.copy(seed_small)
        sub.seed_beam = copy.copy(seed_small.seed_beam)
        sub.seed_beam.x = seed_small.seed_beam.x[10:14].copy()
        return sub, None
    if name == "seeded_long_rows_nv700":
        return problem_mod.regrid_seed_beam(problem_mod.resample_frequency(seed_small, 700), nx=6, ny=3, na=20, nb=20), None
    if name == "ase_shuffled_list":
        ids = rng.permutation(ase_small.n_rays_total)[:60000].astype(np.int64)
        return ase_small, ase_small.build_rays(ids)
    if name == "ase_up_to_3_runs":                          # 36 rays per pixel: a tile of 64 rays holds at most 3 pixels
        return problem_mod.regrid_beam(ase_small, nx=20, ny=10, na=6, nb=6), None
    if name == "ase_row_cache":                             # 4 rays per pixel: 16 pixels per tile
        return problem_mod.regrid_beam(ase_small, nx=30, ny=20, na=2, nb=2), None
    if name == "ase_long_rows_nv700":
        return problem_mod.regrid_beam(problem_mod.resample_frequency(ase_small, 700), nx=4, ny=3, na=9, nb=7), None
    if name == "ase_one_ray_per_pixel":                     # exclusive grid: rows are stored, not added
        return problem_mod.regrid_beam(problem_mod.resample_frequency(ase_small, 128), nx=70, ny=33, a_centre=-1.0, b_centre=-4.5), None
    if name == "ase_i_ang_in_lds_64x64":
        return problem_mod.regrid_beam(ase_small, nx=3, ny=2, na=64, nb=64), None
    if name == "ase_i_ang_global_atomics_80x70":
        return problem_mod.regrid_beam(ase_small, nx=2, ny=2, na=80, nb=70), None
    raise KeyError(name)


@pytest.mark.parametrize("name", ["seeded_shuffled_list", "seeded_beyond_the_cache_nv300", "seeded_grid_tables",
                                  "seeded_long_rows_nv700", "ase_shuffled_list", "ase_up_to_3_runs", "ase_row_cache",
                                  "ase_long_rows_nv700", "ase_one_ray_per_pixel", "ase_i_ang_in_lds_64x64",
                                  "ase_i_ang_global_atomics_80x70"])
def test_deposit_variants(hip, oracle, ase_small, seed_small, name):
    p, rays = _variant(name, ase_small, seed_small)
    ref, counts = check(hip, oracle, p, rays, f"deposit variant {name}")
    if rays is None:            # the same grid through the ray list: no own cells, no grid tables, no exclusive stores
        check(hip, oracle, p, p.build_rays(), f"deposit variant {name}, as a list", ref, counts)


# ---------------------------------------------------------------------------------------------- frequency counts
@pytest.mark.parametrize("nv", [1, 3, 6, 50, 64, 65, 130, 512])
def test_frequency_counts(hip, oracle, ase_small, nv):
    """VEC 1 / 2 / 4 and their tails, the last frequency of every 64-lane chunk: exact emission at the tight tier
    (and the default mode beside it)."""
    if nv > 1:
        p = problem_mod.resample_frequency(ase_small, nv)
    else:
        p = copy.copy(ase_small)
        p.beam = copy.copy(ase_small.beam)
        p.beam.dv = np.ascontiguousarray(ase_small.beam.dv[20:21])
        p.gain = [rt.Gain(g.x, g.y, g.n, g.g0, g.E0, g.gv.reshape(-1, 52)[:, 20:21].copy(), 1) for g in ase_small.gain]
    rays = p.build_rays(np.arange(0, p.n_rays_total, 211, dtype=np.int64))
    check(hip, oracle, p, rays, f"K = {nv}, every 211th ray")
    small = problem_mod.regrid_beam(p, nx=9, ny=5, na=7, nb=6)          # and a whole grid (own cells, one launch)
    check(hip, oracle, small, None, f"K = {nv}, 9 x 5 x 7 x 6 grid")


# ---------------------------------------------------------------------------------------------- ragged lists, cell edges
def edge_rays(p, n):
    """n rays of p's grid whose launch x, y, a, b are moved onto edges of deposit cells: g[i] +- d/2, as the float32
    next to it on either side and the nearest one."""
    b = p.beam
    rays = p.build_rays(200000 + np.arange(n, dtype=np.int64))
    j = np.arange(n)
    for t, (key, g, d) in enumerate((("x", b.x, b.dx), ("y", b.y, b.dy), ("a", b.a, b.da), ("b", b.b, b.db))):
        i = (3 * j + 5 * t + j // 6) % len(g)
        sign = np.where((j + t) % 2 == 0, 0.5, -0.5)
        v = (g[i] + sign * d).astype(np.float32)
        side = (j // 2 + t) % 3
        lo, hi = np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))
        rays[key] = np.where(side == 0, v, np.where(side == 1, lo, hi))
    return rays


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_ragged_lists_with_rays_on_cell_edges(hip, oracle, ase_small, n):
    rays = edge_rays(ase_small, n)
    cells = deposit_cells(ase_small, rays)
    if n > 1:       # (one ray has one cell)
        for c in cells:
            assert len(np.unique(c[c >= 0])) >= 2
        assert any((c < 0).any() for c in cells), "some edge rays fall off the grid"
    ref, counts = check(hip, oracle, ase_small, rays, f"{n} rays on cell edges", n_threads=1)
    assert counts[0].sum() == int(((cells[0] >= 0) & (cells[1] >= 0)).sum())
    plain = ase_small.build_rays(200000 + np.arange(n, dtype=np.int64))
    check(hip, oracle, ase_small, plain, f"{n} rays of the grid", n_threads=1)


# ---------------------------------------------------------------------------------------------- the stand-in
def test_ase_medium_standin_element_by_element(hip, oracle, ase_small):
    """scale_problem(16): 6 384 000 rays.  No whole-array reference of this size is committed (the fixtures of the
    stand-in hold its grids only), so the reference side is oracle.image_loop with 16 threads, as in
    test_gpu_fullsize.py."""
    p = rt.scale_problem(ase_small, 16.0)
    assert p.n_rays_total == 6384000
    check(hip, oracle, p, None, "stand-in, 6 384 000 rays", n_threads=min(16, os.cpu_count() or 1))


# ---------------------------------------------------------------------------------------------- random problems
@pytest.mark.parametrize("i", range(40))
def test_random_cases(hip, oracle, ase_small, seed_small, i):
    """The random problems of test_gpu_fuzz.py: lists (seeds 1000 ...) and uniform grids (seeds 77000 ...)."""
    if i < 20:
        p, rays = random_case(np.random.default_rng(1000 + i), ase_small, seed_small)
        label = f"random list {1000 + i}"
    else:
        p, shape = random_grid_case(np.random.default_rng(77000 + i - 20), ase_small, seed_small)
        rays, label = None, f"random grid {77000 + i - 20} {shape}"
    check(hip, oracle, p, rays, f"{label} (N = {p.N}, K = {p.beam.nv}, seeded {p.seed is not None})", n_threads=4)
