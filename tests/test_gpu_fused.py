"""The one-launch run (raytrace-miniapp_amd/csrc/rt_fused.hip: march and frequency pass as two phases of the same
persistent waves) against the oracle and against the two-kernel run of the same plan.

It is taken by itself for the emission mode on the beam's own ray grid (what RayTrace::create_image builds for an
ASE file, src/RayTraceImage.cpp:283-328) when the frequency pass fits into LDS beside the march tables;
RT_HIP_FUSED=2 keeps the two kernels.  Both must give the CPU loop's image (RayTraceImageCPU.cpp:19-70)."""
import copy
import importlib
import os

import numpy as np
import pytest

from conftest import rel_l2
from element_gate import DEFAULT_TIER, TIGHT_TIER, contribution_counts, counts_from_oracle, gate_outputs

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
pytestmark = pytest.mark.gpu
TIGHT = 2e-7   # one float rounding of es/gs per sub-segment (frequency kernel)


def run_grid(hip, p, fused, **grid):
    os.environ["RT_HIP_FUSED"] = "1" if fused else "2"
    try:
        with hip.Plan(p) as plan:
            plan.set_ray_grid(**grid)
            out = plan.run().fetch()
            out["fused"] = plan.last_fused()
    finally:
        os.environ.pop("RT_HIP_FUSED", None)
    return out


def same_images(a, b, p, counts, label, tol=1e-13):
    """Two device runs of one problem: the deposit order of the atomics differs, nothing else -- whole-array and,
    with the counts of the rays deposited into every element, under the reordering gate of element_gate.py."""
    assert rel_l2(a["image"], b["image"]) < tol and rel_l2(a["I_ang"], b["I_ang"]) < tol
    gate_outputs(a, b, p, counts, "reordering", f"one launch: {label}, against the two kernels")
    for key in ("n_rays", "cell_steps", "n_escaped", "n_skipped"):
        assert a["stats"][key] == b["stats"][key], key
    assert a["failure_code"] == b["failure_code"]


def test_one_launch_run_of_the_shipped_file_equals_the_reference_and_the_two_kernel_run(hip, ase_small, ase_ref):
    one, two = run_grid(hip, ase_small, True), run_grid(hip, ase_small, False)
    assert one["fused"] and not two["fused"]
    assert one["stats"]["n_rays"] == 399000 and one["stats"]["cell_steps"] == 4768067
    assert rel_l2(one["image"], ase_ref["image"]) < TIGHT and rel_l2(one["I_ang"], ase_ref["I_ang"]) < TIGHT
    counts = contribution_counts(ase_small)
    gate_outputs(one, ase_ref, ase_small, counts, DEFAULT_TIER, "one launch: ASE_small against ASE_small_ref_cpu.npz")
    gate_outputs(two, ase_ref, ase_small, counts, DEFAULT_TIER, "two kernels: ASE_small against ASE_small_ref_cpu.npz")
    same_images(one, two, ase_small, counts, "ASE_small")
    # the default (no environment) is the one-launch run
    with hip.Plan(ase_small) as plan:
        plan.set_ray_grid().run()
        assert plan.last_fused()
        m, f = plan.kernel_times()
        assert m > 0 and f < 0.05 * m          # one launch: the whole time is on the first event pair


@pytest.mark.parametrize("scale", [0.25, 2.0, 16.0])
def test_one_launch_run_on_scaled_problems_takes_every_work_group_size(hip, oracle, ase_small, scale):
    """scale_problem (the reference's own enlargement rule, CreateImageHelpers.cpp:104-150) at 0.25, 2 and 16 (the
    ASE_medium stand-in): sixteen waves per work-group at every size since round 5, twelve of them marching."""
    p = rt.scale_problem(ase_small, scale)
    if p.beam.na * p.beam.nb < 32:
        pytest.skip("fewer than 32 rays per pixel: the run keeps two kernels")
    one, two = run_grid(hip, p, True), run_grid(hip, p, False)
    assert one["fused"] and not two["fused"]
    counts = contribution_counts(p)
    same_images(one, two, p, counts, f"scale_problem({scale:g})")
    if scale <= 2.0:
        ref = oracle.image_loop(p, p.build_rays())
        assert one["stats"]["cell_steps"] == ref["counters"]["cell_steps"]
        assert rel_l2(one["image"], ref["image"]) < TIGHT and rel_l2(one["I_ang"], ref["I_ang"]) < TIGHT
        gate_outputs(one, ref, p, counts, DEFAULT_TIER, f"one launch: scale_problem({scale:g}) against the oracle")


def test_one_launch_run_with_ragged_ray_ranges_and_strides(hip, oracle, ase_small):
    """Sub-ranges of the ray grid (N_start / N_parallel, RayTraceImage.cpp:300-313): a last tile with fewer than 64
    rays, fewer tiles than waves, a single ray."""
    total = ase_small.n_rays_total
    for first, stride, count in [(0, 1, 64 * 1000 + 17), (5, 3, 40000), (0, 1, 1), (123, 1, 63), (0, 7, total // 7)]:
        one = run_grid(hip, ase_small, True, first=first, stride=stride, count=count)
        two = run_grid(hip, ase_small, False, first=first, stride=stride, count=count)
        assert one["fused"] and one["stats"]["n_rays"] == count
        ids = first + stride * np.arange(count, dtype=np.int64)
        counts = contribution_counts(ase_small, ase_small.build_rays(ids))
        same_images(one, two, ase_small, counts, f"rays {first} + {stride} i, i < {count}")
        ref = oracle.image_loop(ase_small, ase_small.build_rays(ids))
        assert one["stats"]["cell_steps"] == ref["counters"]["cell_steps"]
        assert rel_l2(one["image"], ref["image"]) < TIGHT and rel_l2(one["I_ang"], ref["I_ang"]) < TIGHT
        gate_outputs(one, ref, ase_small, counts, DEFAULT_TIER, f"one launch: rays {first} + {stride} i, i < {count}, against the oracle")


@pytest.mark.parametrize("N", [2, 4])
def test_one_launch_run_for_other_numbers_of_lengths(hip, oracle, ase_small, N):
    """N != 3: the generic instance of the frequency pass (any number of sub-segments) inside the one launch, as long
    as the tables leave room for it."""
    p = copy.copy(ase_small)
    g = ase_small.gain
    p.gain = [g[0]] + [g[1 + (i % 2)] for i in range(N - 1)]   # (N follows the number of tables)
    one, two = run_grid(hip, p, True), run_grid(hip, p, False)
    # (N = 4: three lengths of tables fill the LDS, no room for the frequency pass beside them -- two kernels)
    assert one["fused"] == (N == 2) and not two["fused"]
    counts = contribution_counts(p)
    same_images(one, two, p, counts, f"N = {N}")
    ref = oracle.image_loop(p, p.build_rays())
    assert rel_l2(one["image"], ref["image"]) < TIGHT and rel_l2(one["I_ang"], ref["I_ang"]) < TIGHT
    gate_outputs(one, ref, p, counts, DEFAULT_TIER, f"one launch: N = {N} against the oracle")


def test_one_launch_run_reports_failing_rays_like_the_cpu_loop(hip, oracle, ase_small):
    """Error -3 / -2 (Helper.h:582-594) found by the frequency phase: the run is repeated on the march records
    (checking pass + deposit without the failing rays) by the stand-alone frequency kernel."""
    from test_gpu_edges import same_outputs_in_a_failing_run
    # (NaN and sign-flipped tables: outside the element gate, whole-array comparison only)
    p = copy.copy(ase_small)
    g = ase_small.gain[2]
    gv = g.gv.copy()
    gv[::7] = np.nan
    p.gain = ase_small.gain[:2] + [rt.Gain(g.x, g.y, g.n, g.g0, g.E0, gv, g.Nv)]
    one = run_grid(hip, p, True)
    ref = oracle.image_loop(p, p.build_rays())
    assert one["fused"]
    assert ref["failure_code"] & (1 << 3) and one["failure_code"] == ref["failure_code"]
    same_outputs_in_a_failing_run(one, ref)
    gv = -np.abs(g.gv)
    p.gain = ase_small.gain[:2] + [rt.Gain(g.x, g.y, g.n, g.g0, g.E0, gv, g.Nv)]
    one = run_grid(hip, p, True)
    ref = oracle.image_loop(p, p.build_rays())
    assert ref["failure_code"] & (1 << 2) and one["failure_code"] == ref["failure_code"]
    same_outputs_in_a_failing_run(one, ref)


def test_what_keeps_the_two_kernels(hip, ase_small, seed_small):
    """Probe, path tracer, seeded mode, ray lists, fewer than 32 rays per pixel: the two-kernel run, whatever the
    environment says."""
    os.environ["RT_HIP_FUSED"] = "1"
    try:
        with hip.Plan(ase_small) as plan:
            plan.set_ray_grid().enable_probe().run()
            assert not plan.last_fused()
        with hip.Plan(ase_small) as plan:
            plan.set_rays(ase_small.build_rays(np.arange(0, 64 * 500, dtype=np.int64))).run()
            assert not plan.last_fused()
        with hip.Plan(seed_small) as plan:
            plan.set_ray_grid(count=64 * 2000).run()
            assert not plan.last_fused()
        few = problem_mod.regrid_beam(ase_small, na=4, nb=4)
        with hip.Plan(few) as plan:
            plan.set_ray_grid().run()
            assert not plan.last_fused()
    finally:
        os.environ.pop("RT_HIP_FUSED", None)


def test_exact_emission_mode_inside_the_one_launch(hip, oracle, ase_small):
    os.environ["RT_HIP_FUSED"] = "1"
    try:
        with hip.Plan(ase_small) as plan:
            plan.set_ray_grid(count=64 * 900 + 5).set_exact_emission().run()
            out = plan.fetch()
            assert plan.last_fused()
    finally:
        os.environ.pop("RT_HIP_FUSED", None)
    rays = ase_small.build_rays(np.arange(64 * 900 + 5, dtype=np.int64))
    ref = oracle.image_loop(ase_small, rays)
    assert rel_l2(out["image"], ref["image"]) < 1e-11 and rel_l2(out["I_ang"], ref["I_ang"]) < 1e-11
    gate_outputs(out, ref, ase_small, contribution_counts(ase_small, rays), TIGHT_TIER, "one launch: exact emission, 57 605 rays, against the oracle")


@pytest.mark.parametrize("seed", range(12))
def test_random_grids_through_the_one_launch_run(hip, oracle, ase_small, seed):
    """Random ray-grid sizes and frequency counts (rows padded to four frequencies, windows of 64): one launch
    against the two kernels and, for the smaller ones, the oracle."""
    rng = np.random.default_rng(1000 + seed)
    na, nb = int(rng.integers(6, 24)), int(rng.integers(6, 24))
    nx, ny = int(rng.integers(3, 40)), int(rng.integers(2, 20))
    p = problem_mod.regrid_beam(ase_small, nx=nx, ny=ny, na=na, nb=nb)
    if rng.random() < 0.5:
        p = problem_mod.resample_frequency(p, int(rng.integers(5, 150)))
    if na * nb < 32:
        pytest.skip("fewer than 32 rays per pixel")
    one, two = run_grid(hip, p, True), run_grid(hip, p, False)
    assert one["fused"] and not two["fused"]
    counts = contribution_counts(p)
    same_images(one, two, p, counts, f"random grid {1000 + seed} ({nx} x {ny} x {na} x {nb}, K = {p.beam.nv})", tol=1e-12)
    if p.n_rays_total <= 400000:
        ref = oracle.image_loop(p, p.build_rays())
        assert one["stats"]["cell_steps"] == ref["counters"]["cell_steps"]
        assert rel_l2(one["image"], ref["image"]) < TIGHT and rel_l2(one["I_ang"], ref["I_ang"]) < TIGHT
        gate_outputs(one, ref, p, counts, DEFAULT_TIER, f"one launch: random grid {1000 + seed} against the oracle")


@pytest.mark.parametrize("split", ["2", "3"])
def test_tiles_split_over_four_waves_give_the_same_image(hip, oracle, ase_small, split, monkeypatch):
    """The one-launch run hands the last tiles of a work-group to four waves, a quarter of the frequencies each
    (rt_march.hip: tile_publish).  RT_HIP_FUSED_SPLIT=3 splits EVERY tile, 2 none: both against the two-kernel run and
    the oracle, for frequency counts that divide unevenly, a failing run included (every part may report the ray; the
    checking repeat leaves the CPU loop's report)."""
    from test_gpu_edges import same_outputs_in_a_failing_run
    monkeypatch.setenv("RT_HIP_FUSED_SPLIT", split)
    for nv in (52, 33, 130, 20):
        p = ase_small if nv == 52 else problem_mod.resample_frequency(ase_small, nv)
        one, two = run_grid(hip, p, True, count=64 * 700 + 9), run_grid(hip, p, False, count=64 * 700 + 9)
        assert one["fused"] and not two["fused"]
        same_images(one, two, p, contribution_counts(p, p.build_rays(np.arange(64 * 700 + 9, dtype=np.int64))),
                    f"tile split {split}, K = {nv}", tol=1e-12)
    rays = ase_small.build_rays(np.arange(64 * 700 + 9, dtype=np.int64))
    ref = oracle.image_loop(ase_small, rays)
    one = run_grid(hip, ase_small, True, count=64 * 700 + 9)
    assert rel_l2(one["image"], ref["image"]) < TIGHT and rel_l2(one["I_ang"], ref["I_ang"]) < TIGHT
    gate_outputs(one, ref, ase_small, contribution_counts(ase_small, rays), DEFAULT_TIER, f"one launch: tile split {split} against the oracle")
    # a failing run: NaNs in the lineshape of one length (outside the element gate, whole-array comparison only)
    p = copy.copy(ase_small)
    g = ase_small.gain[2]
    gv = g.gv.copy()
    gv[::7] = np.nan
    p.gain = ase_small.gain[:2] + [rt.Gain(g.x, g.y, g.n, g.g0, g.E0, gv, g.Nv)]
    one = run_grid(hip, p, True)
    ref = oracle.image_loop(p, p.build_rays())
    assert one["fused"] and one["failure_code"] == ref["failure_code"] and ref["failure_code"] & (1 << 3)
    same_outputs_in_a_failing_run(one, ref)


@pytest.mark.parametrize("split", ["2", "3"])
def test_invalid_rays_are_reported_once_however_a_tile_is_split(hip, oracle, ase_small, split, monkeypatch):
    """Error -1 (Helper.h:515: the ray ends nearly perpendicular to z) is found by the preamble of the frequency pass,
    which every part of a split tile repeats: only the part that starts at frequency 0 reports it.  A beam whose
    angle grid reaches +-1550 mrad: the rays of its two outermost angles are invalid, all others trace as usual."""
    monkeypatch.setenv("RT_HIP_FUSED_SPLIT", split)
    p = copy.copy(ase_small)
    b = copy.copy(ase_small.beam)
    b.a = np.linspace(-1550.0, 1550.0, 32)
    b.da = float(b.a[1] - b.a[0])
    b.b = b.b[:2].copy()
    b.x, b.y = b.x[30:31].copy(), b.y[5:6].copy()
    p.beam = b
    rays = p.build_rays()
    assert len(rays) == 64
    ref = oracle.image_loop(p, rays)
    one, two = run_grid(hip, p, True), run_grid(hip, p, False)
    assert one["fused"] and not two["fused"]
    assert ref["failure_code"] == 1 << 1 and one["failure_code"] == two["failure_code"] == ref["failure_code"]
    n_bad = len(ref["failed_rays"])
    assert n_bad == 4 and len(one["failed_rays"]) == n_bad and len(two["failed_rays"]) == n_bad
    counts = counts_from_oracle(oracle, p, rays)          # (the four invalid rays deposit nothing and are not counted)
    same_images(one, two, p, counts, f"invalid rays, tile split {split}", tol=1e-12)
    assert rel_l2(one["image"], ref["image"]) < TIGHT
    gate_outputs(one, ref, p, counts, DEFAULT_TIER, f"one launch: invalid rays, tile split {split}, against the oracle")


@pytest.mark.parametrize("env", [
    {"RT_HIP_FUSED_CONSUMERS": "0", "RT_HIP_LATE_X10": "0"},                 # the round-4 run: every wave marches, no late zone
    {"RT_HIP_FUSED_CONSUMERS": "4", "RT_HIP_LATE_X10": "0"},
    {"RT_HIP_FUSED_CONSUMERS": "0", "RT_HIP_LATE_X10": "60"},
    {"RT_HIP_FUSED_CONSUMERS": "7", "RT_HIP_LATE_X10": "1000", "RT_HIP_LATE_WAVES": "1"},   # a quarter of the list for one wave
    {"RT_HIP_FUSED_NODES": "0"},                                             # every list entry takes the global links
    {"RT_HIP_FUSED_NODES": "3"},                                             # LDS nodes and overflow mixed on one stack
    {"RT_HIP_FUSED_CONSUMERS_FIRST": "1"},
    {"RT_HIP_MARCH_THREADS": "256", "RT_HIP_FUSED_CONSUMERS": "1"},
    {"RT_HIP_MARCH_THREADS": "64"},                                          # one wave per work-group: it marches, then consumes
])
def test_consumer_waves_late_zone_and_list_storage_leave_the_image_alone(hip, oracle, ase_small, env, monkeypatch):
    """Round 5 of the one-launch run: waves that only run the frequency pass (consumers), the end of the ray list kept
    for the first waves of each work-group (late zone), list nodes in LDS with overflow to global links -- whatever the
    mix, every ray is marched once and every tile integrated once: counters and image of the two-kernel run."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = 64 * 1500 + 17
    one, two = run_grid(hip, ase_small, True, count=n), run_grid(hip, ase_small, False, count=n)
    assert one["fused"] and not two["fused"]
    assert one["stats"]["n_rays"] == n
    same_images(one, two, ase_small, contribution_counts(ase_small, ase_small.build_rays(np.arange(n, dtype=np.int64))),
                f"96 017 rays, {env}", tol=1e-12)
    whole = run_grid(hip, ase_small, True)
    assert whole["stats"]["cell_steps"] == 4768067 and whole["failure_code"] == 0


def test_seeded_mode_as_one_launch(hip, oracle, seed_small, seed_ref, monkeypatch):
    """The gain-only instance of the one-launch kernel (RT_HIP_FUSED_SEED=1; two kernels are the rule for this mode,
    profiles/r05_seed_fused_ab.txt): row caches for the consumers beside the tables, for the others over them once the
    march is done.  seed_small.dat against the reference's CPU loop and against the two-kernel run."""
    two = run_grid(hip, seed_small, True)
    assert not two["fused"]
    monkeypatch.setenv("RT_HIP_FUSED_SEED", "1")
    for extra in ({}, {"RT_HIP_FUSED_CONSUMERS": "2", "RT_HIP_FUSED_ROWS": "5"}, {"RT_HIP_FUSED_NODES": "0"}):
        for k, v in extra.items():
            monkeypatch.setenv(k, v)
        one = run_grid(hip, seed_small, True)
        assert one["fused"]
        assert one["stats"]["n_rays"] == 7803000 and one["stats"]["cell_steps"] == 53573880
        assert rel_l2(one["image"], seed_ref["image"]) < 1e-12 and rel_l2(one["I_ang"], seed_ref["I_ang"]) < 1e-12
        counts = counts_from_oracle(oracle, seed_small)
        gate_outputs(one, seed_ref, seed_small, counts, TIGHT_TIER, f"one launch: seed_small {extra} against seed_small_ref_cpu.npz")
        same_images(one, two, seed_small, counts, f"seed_small {extra}", tol=1e-12)
        for k in extra:
            monkeypatch.delenv(k)
    part = run_grid(hip, seed_small, True, count=64 * 3000 + 5)
    monkeypatch.delenv("RT_HIP_FUSED_SEED")
    same_images(part, run_grid(hip, seed_small, True, count=64 * 3000 + 5), seed_small,
                counts_from_oracle(oracle, seed_small, seed_small.build_rays(np.arange(64 * 3000 + 5, dtype=np.int64))),
                "seed_small, 192 005 rays", tol=1e-12)


@pytest.mark.parametrize("env", [{"RT_HIP_LATE2_X10": "0"}, {"RT_HIP_LATE2_X10": "400", "RT_HIP_LATE_WAVES": "1"},
                                 {"RT_HIP_LATE2_X10": "60", "RT_HIP_LATE_CAP": "100", "RT_HIP_MARCH_THREADS": "256"},
                                 {"RT_HIP_MARCH_MODE": "0"}, {"RT_HIP_MARCH_MODE": "2"}])
def test_late_zone_and_compile_time_mode_of_the_march_kernel_leave_the_records_alone(hip, oracle, seed_small, ase_small, env, monkeypatch):
    """The march as a kernel of its own (seeded mode; emission with RT_HIP_FUSED=2): the late zone of its ray list
    (RT_HIP_LATE2_X10 / RT_HIP_LATE_WAVES / RT_HIP_LATE_CAP) and the instance with the method fixed at compile time
    (RT_HIP_MARCH_MODE) hand every ray out exactly once and march it as ever: records bit-identical to the oracle's."""
    import numpy as np
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RT_HIP_FUSED", "2")
    for p, n in ((seed_small, 64 * 2900 + 11), (ase_small, 64 * 1300 + 5)):
        rays = p.build_rays(np.arange(n, dtype=np.int64))
        with hip.Plan(p) as plan:
            plan.set_ray_grid(count=n).enable_probe().run()
            out = plan.fetch()
            pr = plan.fetch_probe()
            assert not plan.last_fused()
        assert out["stats"]["n_rays"] == n
        ref = oracle.probe(p, rays, want_Iv=False)
        for key in ("gvl", "evl"):
            assert np.array_equal(pr[key].view(np.uint32), ref[key].view(np.uint32)), key
        assert np.array_equal(pr["ivl"], ref["ivl"]) and np.array_equal(pr["steps"], ref["steps"])
