"""Step mode on the GPU (rt_step_kernel, rt_hip_step_loop): E_v, nf and I_ang without the image cube, against the
reductions (backend.step_outputs_from_image, long-double sums) of the reference's own cubes, of the oracle's cube and of
the cube the same plan produces in image mode.

Gates (tests/element_gate.py, assert_elements on every element, none left out):
    nf     n_e = rays deposited into the pixel; DEFAULT_TIER in default emission, TIGHT_TIER in exact emission and seeded mode
    E_v    n_e = all rays that deposit into any pixel; tier + (n_e + K) 2^-52 (the tier bounds the terms, the rest is the
           reordering of a sum that long)
    I_ang  as in image mode
    two device runs of the same rays (step mode against the reduced cube of the same plan): reordering_tol only, and an
    element nothing deposits into must be exactly 0
The measured figures are printed before every assertion (ELEMENT_PARITY_FILE appends them to a file:
profiles/step_parity.txt)."""
import copy
import importlib

import numpy as np
import pytest

from element_gate import DEFAULT_TIER, EPS, TIGHT_TIER, assert_elements, contribution_counts, counts_from_oracle, reordering_tol

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- helpers
def reduced(hip, p, out):
    """E_v, nf of a cube (a result dict with image and I_ang), with its I_ang."""
    ref = hip.step_outputs_from_image(p, out["image"])
    ref["I_ang"] = np.asarray(out["I_ang"])
    return ref


def gate_step(got, ref, p, counts, tol, label):
    """assert_elements on nf, E_v and I_ang; tol = a tier, or "reordering" for two device runs of the same rays."""
    b = p.beam
    n_img, n_ang = counts
    n_dep = int(np.sum(n_img))                  # rays that deposit into any pixel
    if isinstance(tol, str):
        t_nf, t_ev, t_ang = reordering_tol(n_img, b.nv), float(reordering_tol(n_dep, b.nv)), reordering_tol(n_ang, b.nv)
    else:
        t_nf, t_ev, t_ang = tol, tol + (n_dep + b.nv) * EPS, tol
    figs = dict(nf=assert_elements(got["nf"], ref["nf"], n_img, t_nf, f"{label} / nf"),
                E_v=assert_elements(got["E_v"], ref["E_v"], np.array([n_dep]), t_ev, f"{label} / E_v"),
                I_ang=assert_elements(got["I_ang"], ref["I_ang"], n_ang, t_ang, f"{label} / I_ang", (b.nb, b.na)))
    assert figs["nf"]["count"] == b.nx * b.ny and figs["E_v"]["count"] == b.nv and figs["I_ang"]["count"] == b.na * b.nb
    return figs


def set_rays(plan, rays):
    return plan.set_ray_grid() if rays is None else plan.set_rays(rays)


def image_then_step(hip, p, rays, monkeypatch, exact=False):
    """(image-mode outputs as two kernels, step-mode outputs, step-mode fetch) of ONE plan."""
    monkeypatch.setenv("RT_HIP_FUSED", "2")     # image mode as two kernels: what the step kernel stands in for
    with hip.Plan(p) as plan:
        set_rays(plan, rays)
        if exact:
            plan.set_exact_emission(True)
        img = plan.run().fetch()
        assert not plan.last_fused()
        plan.enable_step().run()
        step = plan.fetch_step()
        info = plan.fetch()
        assert info["image"] is None and not plan.last_fused()
        assert np.array_equal(info["I_ang"], step["I_ang"])
    return img, step, info


def own_cube_and_oracle(hip, oracle, p, rays, label, tier, monkeypatch, n_threads=4):
    """Step mode against the reduced cube of the same plan (reordering only), then against the oracle's, at the tier."""
    img, step, info = image_then_step(hip, p, rays, monkeypatch)
    ora = oracle.image_loop(p, p.build_rays() if rays is None else rays, n_threads=n_threads)
    assert info["failure_code"] == img["failure_code"] == ora["failure_code"] == 0, label
    assert info["stats"]["cell_steps"] == img["stats"]["cell_steps"] == ora["counters"]["cell_steps"], label
    counts = counts_from_oracle(oracle, p, rays, n_threads=n_threads)
    gate_step(step, reduced(hip, p, img), p, counts, "reordering", f"{label} / step against the plan's own cube")
    gate_step(step, reduced(hip, p, ora), p, counts, tier, f"{label} / step against the oracle's cube")
    return step, counts


# ---------------------------------------------------------------------------------------------- 1. reference fixtures
_fixture_counts = {}


@pytest.mark.parametrize("name,exact", [("ASE_small", False), ("ASE_small", True), ("seed_small", False)])
def test_reference_fixtures(hip, oracle, ase_small, seed_small, ase_ref, seed_ref, name, exact, monkeypatch):
    """The whole shipped grids against the reductions of the reference's own cubes: on the ray grid (plan) and through
    rt_hip_step_loop with the full list (recognised as the grid there, verified ray by ray)."""
    p, fx = (ase_small, ase_ref) if name == "ASE_small" else (seed_small, seed_ref)
    if name == "ASE_small":
        assert p.n_rays_total == 399000
    tier = TIGHT_TIER if (exact or p.seed is not None) else DEFAULT_TIER
    mode = "seeded" if p.seed is not None else ("exact emission" if exact else "default emission")
    ref = reduced(hip, p, fx)
    if name not in _fixture_counts:
        _fixture_counts[name] = contribution_counts(p) if p.seed is None else counts_from_oracle(oracle, p, None, n_threads=8)
    counts = _fixture_counts[name]
    with hip.Plan(p) as plan:
        plan.set_ray_grid().enable_step()
        if exact:
            plan.set_exact_emission(True)
        plan.run()
        grid = plan.fetch_step()
        assert plan.fetch()["failure_code"] == 0 and plan.image_ptr == 0
    gate_step(grid, ref, p, counts, tier, f"fixture {name}, {mode} / ray grid")
    if exact:
        monkeypatch.setenv("RT_HIP_EXACT_EMISSION", "1")   # (the loop signature has no parameter for it)
    loop = hip.step_loop(p, p.build_rays())
    assert loop["failure_code"] == 0 and len(loop["failed_rays"]) == 0
    assert loop["stats"]["n_rays"] == p.n_rays_total
    gate_step(loop, ref, p, counts, tier, f"fixture {name}, {mode} / rt_hip_step_loop")
    gate_step(loop, grid, p, counts, "reordering", f"fixture {name}, {mode} / rt_hip_step_loop against the plan")


# ---------------------------------------------------------------------------------------------- 2. the plan's own cube
def test_ragged_tile_with_pixel_runs_across_the_tile_boundary(hip, oracle, ase_small, monkeypatch):
    """210 rays: three full tiles and a ragged one, runs of 35 rays per pixel that straddle the tile boundaries."""
    p = problem_mod.regrid_beam(ase_small, nx=3, ny=2, na=5, nb=7)
    assert p.n_rays_total == 210
    own_cube_and_oracle(hip, oracle, p, None, "3 x 2 x 5 x 7 grid", DEFAULT_TIER, monkeypatch)
    own_cube_and_oracle(hip, oracle, p, p.build_rays(), "3 x 2 x 5 x 7 grid as a list", DEFAULT_TIER, monkeypatch)


def test_shuffled_list_with_rays_off_the_image_and_off_the_angular_grid(hip, oracle, ase_small, monkeypatch):
    """Every 211th ray in random order; an eighth of them off the image in x (pixel -1, angle cell valid: they count for
    I_ang only), another eighth off the angular grid (angle -1, pixel valid: they count for E_v and nf only)."""
    b = ase_small.beam
    rng = np.random.default_rng(11)
    ids = rng.permutation(np.arange(0, ase_small.n_rays_total, 211, dtype=np.int64))
    rays = ase_small.build_rays(ids)
    n = len(rays)
    rays["x"][: n // 8] = np.float32(b.x[-1] + 0.75 * b.dx)
    rays["a"][n // 8: n // 4] = np.float32(b.a[-1] + 0.75 * b.da)
    from element_gate import deposit_cells
    ix, iy, ia, ib = deposit_cells(ase_small, rays)
    assert (ix[: n // 8] < 0).all() and (ia[: n // 8] >= 0).all() and (ib[: n // 8] >= 0).all()
    assert (ia[n // 8: n // 4] < 0).all() and (ix[n // 8: n // 4] >= 0).all() and (iy[n // 8: n // 4] >= 0).all()
    step, counts = own_cube_and_oracle(hip, oracle, ase_small, rays, "shuffled list, rays off the image and off the angles",
                                       DEFAULT_TIER, monkeypatch)
    assert int(counts[0].sum()) == n - n // 8 and int(counts[1].sum()) == n - (n // 4 - n // 8)


def test_strided_ray_grid(hip, oracle, ase_small, monkeypatch):
    q = copy.copy(ase_small)
    q.N_start, q.N_parallel = 3, 7
    own_cube_and_oracle(hip, oracle, q, None, "ray grid, first 3 stride 7", DEFAULT_TIER, monkeypatch)


def test_one_ray_per_pixel_plain_stores_and_a_ragged_tile(hip, oracle, ase_small, monkeypatch):
    """na = nb = 1 on the beam's own grid: the exclusive detection of the host, nf by plain stores; 70 x 33 pixels are
    36 tiles and a ragged one, nv = 64."""
    p = problem_mod.regrid_beam(problem_mod.resample_frequency(ase_small, 64), nx=70, ny=33, a_centre=-1.0, b_centre=-4.5)
    assert p.n_rays_total % 64 != 0 and p.beam.nv == 64
    own_cube_and_oracle(hip, oracle, p, None, "one ray per pixel, 70 x 33, nv 64", DEFAULT_TIER, monkeypatch)


def test_one_ray_per_pixel_256_x_256_nv_512(hip, oracle, ase_small, monkeypatch):
    p = problem_mod.regrid_beam(problem_mod.resample_frequency(ase_small, 512), nx=256, ny=256, a_centre=-1.0, b_centre=-4.5)
    own_cube_and_oracle(hip, oracle, p, None, "one ray per pixel, 256 x 256, nv 512", DEFAULT_TIER, monkeypatch, n_threads=16)


@pytest.mark.parametrize("nv", [1, 2, 3, 5, 130, 300])
def test_frequency_counts(hip, oracle, ase_small, nv, monkeypatch):
    """Odd K, K = 2 mod 4, K below and above the 64 lanes of a flush, K that is no multiple of 4 (padding columns)."""
    if nv > 1:
        p = problem_mod.resample_frequency(ase_small, nv)
    else:
        p = copy.copy(ase_small)
        p.beam = copy.copy(ase_small.beam)
        p.beam.dv = np.ascontiguousarray(ase_small.beam.dv[20:21])
        p.gain = [rt.Gain(g.x, g.y, g.n, g.g0, g.E0, g.gv.reshape(-1, 52)[:, 20:21].copy(), 1) for g in ase_small.gain]
    rays = p.build_rays(np.arange(0, p.n_rays_total, 257, dtype=np.int64))
    own_cube_and_oracle(hip, oracle, p, rays, f"K = {nv}, every 257th ray", DEFAULT_TIER, monkeypatch)


@pytest.mark.parametrize("N", [2, 5, 9])
def test_other_numbers_of_lengths(hip, oracle, ase_small, N, monkeypatch):
    """N = 3 takes the instances with the sub-segments unrolled (SF = 6), every other N the generic ones."""
    p = copy.copy(ase_small)
    g = ase_small.gain
    p.gain = [g[0]] + [g[1 + (i % 2)] for i in range(N - 1)]
    rays = p.build_rays(np.arange(0, p.n_rays_total, 397, dtype=np.int64))
    own_cube_and_oracle(hip, oracle, p, rays, f"N = {N}, every 397th ray", DEFAULT_TIER, monkeypatch)


@pytest.mark.parametrize("case", ["shuffled_list", "sub_grid"])
def test_seeded(hip, oracle, seed_small, case, monkeypatch):
    """Method 2 deposits at the exit ray, with mirrored y: 60 000 rays in random order (many short runs of a pixel per
    tile), and the 4 x 25 x 51 x 51 sub-grid on the device-generated grid with its seed-factor tables."""
    if case == "shuffled_list":
        rng = np.random.default_rng(7)
        ids = np.sort(rng.permutation(seed_small.n_rays_total)[:60000]).astype(np.int64)
        p, rays = seed_small, seed_small.build_rays(rng.permutation(ids))
    else:
        p = copy.copy(seed_small)
        p.seed_beam = copy.copy(seed_small.seed_beam)
        p.seed_beam.x = seed_small.seed_beam.x[10:14].copy()
        rays = None
        assert p.n_rays_total == 4 * 25 * 51 * 51
    own_cube_and_oracle(hip, oracle, p, rays, f"seeded, {case}", TIGHT_TIER, monkeypatch)


# ---------------------------------------------------------------------------------------------- 3. failing runs
def _ray_set(rays):
    return sorted(tuple(np.asarray(r.tolist(), dtype=np.float32).view(np.uint32).tolist()) for r in rays)


def same_step_outputs_in_a_failing_run(out, ref, tol=1e-6):
    """The whole-array rule of same_outputs_in_a_failing_run (tests/test_gpu_edges.py) on the three step outputs: the
    same non-finite entries, the finite ones within tol of the norm."""
    for key in ("E_v", "nf", "I_ang"):
        a, b = np.asarray(out[key]), np.asarray(ref[key])
        fa, fb = np.isfinite(a), np.isfinite(b)
        assert np.array_equal(fa, fb), key
        assert np.array_equal(np.isnan(a), np.isnan(b)), key
        assert np.array_equal(a[~fa & ~np.isnan(a)], b[~fb & ~np.isnan(b)]), key
        nb = np.linalg.norm(b[fb])
        d = np.linalg.norm(a[fa] - b[fb])
        print(f"failing run / {key}: finite {int(fa.sum())} of {a.size}, |got - ref| / |ref| = {d / nb if nb > 0 else d:.3e}")
        assert d <= tol * nb if nb > 0 else np.all(a[fa] == 0), key


def failing_inputs(ase_small):
    """The three inputs of test_failure_codes_match_the_cpu_loop (tests/test_gpu_edges.py), built the same way."""
    rays = ase_small.build_rays(np.arange(0, ase_small.n_rays_total, 997, dtype=np.int64))
    bad = rays.copy()
    bad["a"][7] = 1500.0                                     # error -1: almost perpendicular to z (Helper.h:515)
    g = ase_small.gain[2]
    nan_p, neg_p = copy.copy(ase_small), copy.copy(ase_small)
    gv = g.gv.copy()
    gv[::7] = np.nan                                         # error -3: NaNs in the lineshape
    nan_p.gain = ase_small.gain[:2] + [rt.Gain(g.x, g.y, g.n, g.g0, g.E0, gv, g.Nv)]
    neg_p.gain = ase_small.gain[:2] + [rt.Gain(g.x, g.y, g.n, g.g0, g.E0, -np.abs(g.gv), g.Nv)]   # error -2
    return dict(invalid_ray=(ase_small, bad, 1 << 1), nan_lineshape=(nan_p, rays, 1 << 3), negative_lineshape=(neg_p, rays, 1 << 2))


@pytest.mark.parametrize("case", ["invalid_ray", "nan_lineshape", "negative_lineshape"])
def test_failing_runs(hip, oracle, ase_small, case, monkeypatch):
    p, rays, bit = failing_inputs(ase_small)[case]
    img, step, info = image_then_step(hip, p, rays, monkeypatch)
    ora = oracle.image_loop(p, rays)
    assert ora["failure_code"] & bit and info["failure_code"] == img["failure_code"] == ora["failure_code"]
    assert _ray_set(info["failed_rays"]) == _ray_set(img["failed_rays"])
    ref = reduced(hip, p, ora)
    loop = hip.step_loop(p, rays)                            # (staged outputs, then the repeat: the stale ones must not come back)
    assert loop["failure_code"] == ora["failure_code"] and _ray_set(loop["failed_rays"]) == _ray_set(img["failed_rays"])
    if case == "invalid_ray":
        assert len(info["failed_rays"]) == 1 and info["failed_rays"][0] == rays[7]
        counts = counts_from_oracle(oracle, p, rays)         # (the failing ray is not counted)
        gate_step(step, ref, p, counts, DEFAULT_TIER, "error -1 / step against the oracle's cube")
        gate_step(step, reduced(hip, p, img), p, counts, "reordering", "error -1 / step against the plan's own cube")
        gate_step(loop, ref, p, counts, DEFAULT_TIER, "error -1 / rt_hip_step_loop against the oracle's cube")
    else:   # NaN and sign-flipped tables are no non-negative inputs: whole-array rule
        same_step_outputs_in_a_failing_run(step, ref)
        same_step_outputs_in_a_failing_run(step, reduced(hip, p, img))
        same_step_outputs_in_a_failing_run(loop, ref)


# ---------------------------------------------------------------------------------------------- 4. contract
def test_contract(hip, ase_small, monkeypatch):
    import ctypes as C

    cabi = rt.cabi
    p = ase_small
    rays = p.build_rays(np.arange(0, p.n_rays_total, 499, dtype=np.int64))
    b = p.beam
    with hip.Plan(p) as plan:
        lib, h = plan.hl.lib, plan._h
        plan.set_rays(rays).enable_step()
        # before a run: nothing to fetch, no pointers
        with pytest.raises(hip.RayTraceError, match="step run"):
            plan.fetch_step()
        assert lib.rt_hip_plan_step_ptrs(h, None, None) == cabi.RT_ERR_ARG
        # one output mode at a time
        assert lib.rt_hip_plan_enable_path(h, 1) == cabi.RT_ERR_ARG
        assert lib.rt_hip_plan_enable_spectra(h, 1) == cabi.RT_ERR_ARG
        plan.enable_step(False)
        plan.enable_path()
        assert lib.rt_hip_plan_enable_step(h, 1) == cabi.RT_ERR_ARG
        plan.enable_path(False).enable_spectra()
        assert lib.rt_hip_plan_enable_step(h, 1) == cabi.RT_ERR_ARG
        plan.enable_spectra(False).enable_step()
        # a step run takes no image buffer
        import torch
        dev = torch.device("cuda", 0)
        cube = torch.zeros(8, dtype=torch.float64, device=dev)
        assert lib.rt_hip_plan_run(h, None, C.c_void_p(cube.data_ptr()), None) == cabi.RT_ERR_ARG
        # ... an I_ang buffer of the caller's it does take
        ang = torch.full((b.nb, b.na), 7.0, dtype=torch.float64, device=dev)
        plan.run(iang_ptr=ang.data_ptr())
        own = plan.fetch_step()
        torch.cuda.synchronize()
        assert plan.image_ptr == 0, "a plan that has only run in step mode holds no cube"
        assert not plan.last_fused()
        assert np.array_equal(ang.cpu().numpy().reshape(-1), own["I_ang"])
        # fetch: no image pointer, the rest as ever
        img = np.empty(b.nx * b.ny * b.nv)
        assert lib.rt_hip_plan_fetch(h, cabi._dp(img), None, None, None, 0, None, None) == cabi.RT_ERR_ARG
        plan.run()
        info = plan.fetch()
        assert info["image"] is None and info["failure_code"] == 0 and info["stats"]["n_rays"] == len(rays)
        march_ms, freq_ms = plan.kernel_times()
        assert freq_ms > 0 and march_ms > 0 and info["stats"]["freq_ms"] > 0
        step = plan.fetch_step()
        t = plan.step_tensors()
        assert t["E_v"].shape == (b.nv,) and t["nf"].shape == (b.ny, b.nx) and t["I_ang"].shape == (b.nb, b.na)
        for key in ("E_v", "nf", "I_ang"):
            assert np.array_equal(t[key].cpu().numpy().reshape(-1), step[key]), key
        assert step["E_v"].all() and step["nf"].any()
        for key in ("E_v", "nf", "I_ang"):      # the same rays again: the same sums up to their order
            n_e = len(rays)
            assert_elements(own[key], step[key], np.array([n_e]), float(reordering_tol(n_e, b.nv)), f"contract / two step runs / {key}")
        # debug bit 0: no step kernel, outputs stay zero; bit 1: the step kernel over the records of the previous run
        plan.set_debug(1).run()
        z = plan.fetch_step()
        assert not z["E_v"].any() and not z["nf"].any() and not z["I_ang"].any()
        plan.set_debug(0).run()
        plan.set_debug(2).run()
        again = plan.fetch_step()
        for key in ("E_v", "nf", "I_ang"):
            assert_elements(again[key], step[key], np.array([len(rays)]), float(reordering_tol(len(rays), b.nv)), f"contract / debug bit 1 / {key}")
        plan.set_debug(0)
        # the probe works in step mode, and gives what it gives in image mode
        plan.enable_probe().run()
        probe = plan.fetch_probe()
        with_probe = plan.fetch_step()
        for key in ("E_v", "nf", "I_ang"):
            assert_elements(with_probe[key], step[key], np.array([len(rays)]), float(reordering_tol(len(rays), b.nv)), f"contract / probe on / {key}")
        # and off again: image mode unchanged
        plan.enable_step(False)
        back = plan.run().fetch()
        assert plan.image_ptr != 0
        probe_img = plan.fetch_probe()
        for key in ("gvl", "evl", "ivl", "flags", "steps"):
            assert np.array_equal(probe[key], probe_img[key]), key
        assert np.array_equal(probe["ray2"].view(np.uint32), probe_img["ray2"].view(np.uint32))
        assert int(probe["steps"].sum()) == back["stats"]["cell_steps"]
    with hip.Plan(p) as fresh:
        want = fresh.set_rays(rays).run().fetch()
    counts = contribution_counts(p, rays)
    from element_gate import gate_outputs
    if not (np.array_equal(back["image"], want["image"]) and np.array_equal(back["I_ang"], want["I_ang"])):
        gate_outputs(back, want, p, counts, "reordering", "contract / image mode after step mode against a fresh plan")
    # the host-pointer entry refuses NULL outputs
    m = cabi.Marshalled(p)
    code = C.c_uint(0)
    nf = np.zeros(b.nx * b.ny)
    rc = plan.hl.lib.rt_hip_step_loop(0, m.N, C.byref(m.beam), m.gain, m.seed_ref, p.method, cabi.rays_ptr(rays), len(rays), p.scale,
                                      None, cabi._dp(nf), None, C.byref(code), None, 0, None, None)
    assert rc == cabi.RT_ERR_ARG
