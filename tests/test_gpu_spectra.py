"""Spectra mode on the GPU: RayTrace::calc_ray for every ray of a run (rt_spec_kernel) and its host-pointer batched
form (rt_hip_calc_rays), against the reference's own calc_ray outputs (tests/golden/*_ref_rays.npz), against the
oracle's per-ray probe, and against the image path of the same plan.

The gate is the project's parity gate, 1e-5 rel-L2, applied PER RAY over the K frequencies; err is compared ray by ray,
ray2 bit for bit, and a row that is all zero on the CPU must be all zero here.  Measured figures are printed before every
assertion; with SPECTRA_PARITY_FILE set in the environment they are appended to that file as well (this is how
profiles/spectra_parity.txt was taken).

Measured on an MI355X (profiles/spectra_parity.txt): the largest per-ray rel-L2 against the reference fixtures is 5.6e-8
in the default emission mode (one float rounding of es/gs per sub-segment), 4e-14 in the exact mode, 2e-16 in the
gain-only mode; 4.2e-6 on the clean rays of the return-code input, whose sign-flipped table makes gain and absorption
cancel (1e-13 in the exact mode on the same input)."""
import copy
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_l2
from element_gate import assert_elements, contribution_counts, gate_outputs, reordering_tol

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
pytestmark = pytest.mark.gpu
GATE = 1e-5


def note(line):
    print(line)
    path = os.environ.get("SPECTRA_PARITY_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def ray2_bits_equal(a, b, mask):
    return all(np.array_equal(a[k][mask].view(np.uint32), b[k][mask].view(np.uint32)) for k in "xyab")


def row_figures(got, ref):
    """(largest per-ray rel-L2, largest per-element relative difference, rows compared, zero rows) of [n][K] spectra;
    rows that are all zero in ref must be all zero in got (asserted)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    zero = ~ref.any(axis=1)
    assert not got[zero].any(), "a row that is all zero on the CPU is not all zero here"
    g, r = got[~zero], ref[~zero]
    if len(r) == 0:
        return 0.0, 0.0, 0, int(zero.sum())
    l2 = np.linalg.norm(g - r, axis=1) / np.linalg.norm(r, axis=1)
    nz = r != 0
    el = float((np.abs(g - r)[nz] / np.abs(r)[nz]).max()) if nz.any() else 0.0
    return float(l2.max()), el, len(r), int(zero.sum())


def check_against(out, ref, label, clean=None):
    """err equal ray by ray, ray2 bit-equal where err != -1, Iv within the gate on the rays with err == 0."""
    assert np.array_equal(out["err"], ref["err"]), label
    assert ray2_bits_equal(out["ray2"], ref["ray2"], ref["err"] != -1), label
    ok = ref["err"] == 0 if clean is None else clean
    assert not out["Iv"][ref["err"] == -1].any(), label
    l2, el, n, nzero = row_figures(out["Iv"][ok], ref["Iv"][ok])
    note(f"{label}: rows {n} (+{nzero} zero rows), max per-ray rel-L2 {l2:.3e}, max per-element rel diff {el:.3e}")
    assert l2 < GATE, (label, l2)
    return n, nzero


# ---------------------------------------------------------------- 1. the reference's own calc_ray outputs
@pytest.mark.parametrize("name,zero_rows", [("ASE_small", 0), ("seed_small", 26)])
def test_reference_fixtures(hip, name, zero_rows):
    p = rt.datfile.load(GOLDEN / f"{name}.dat.xz")
    fx = np.load(GOLDEN / f"{name}_ref_rays.npz")
    stride, n = int(fx["stride"]), fx["Iv"].shape[0]
    assert n == 400 and not fx["err"].any()          # no ray is left out
    rays = p.build_rays(np.arange(n, dtype=np.int64) * stride)
    ref = dict(err=fx["err"].astype(np.int32), Iv=fx["Iv"], ray2=rt.cabi.rays_from_array(fx["ray2"]))
    assert int((~fx["Iv"].any(axis=1)).sum()) == zero_rows
    runs = []
    with hip.Plan(p) as plan:
        plan.set_rays(rays).enable_spectra().run()
        runs.append(("plan", plan.fetch_spectra()))
        assert plan.fetch()["failure_code"] == 0
        plan.set_exact_emission(True).run()
        runs.append(("plan, exact emission", plan.fetch_spectra()))
    runs.append(("calc_rays", hip.calc_rays(p, rays)))
    os.environ["RT_HIP_EXACT_EMISSION"] = "1"
    try:
        runs.append(("calc_rays, exact emission", hip.calc_rays(p, rays)))
    finally:
        del os.environ["RT_HIP_EXACT_EMISSION"]
    for label, out in runs:
        assert out["Iv"].shape == fx["Iv"].shape
        rows, nzero = check_against(out, ref, f"fixture {name} / {label}")
        assert rows + nzero == n and nzero == zero_rows
    # the one-ray mirror of RayTrace::calc_ray
    e, Iv, r2 = hip.calc_ray(p, rays[7])
    assert e == 0 and np.array_equal(Iv, runs[2][1]["Iv"][7]) and r2 == tuple(float(runs[2][1]["ray2"][7][k]) for k in "xyab")


# ---------------------------------------------------------------- 2. spectra mode against image mode
def own_cells(g, d):
    """RayTraceImageCPU.cpp:11-16 on the float a ray carries: grid point i falls into deposit cell i."""
    v = g.astype(np.float32).astype(np.float64)
    return np.array_equal(np.searchsorted(g, v - 0.5 * d, side="left"), np.arange(len(g)))


def test_spectra_sum_to_the_image_full_size_on_the_device(hip, ase_small):
    import torch

    p = rt.scale_problem(ase_small, 16.0)
    b = p.beam
    assert p.n_rays_total == 6384000
    assert own_cells(b.x, b.dx) and own_cells(b.y, b.dy) and own_cells(b.a, b.da) and own_cells(b.b, b.db)
    K, nx, ny, na, nb = b.nv, b.nx, b.ny, b.na, b.nb
    with hip.Plan(p) as plan:
        plan.set_ray_grid()
        img = plan.run().fetch()
        plan.enable_spectra().run()
        st = plan.fetch()
        assert img["failure_code"] == 0 and st["failure_code"] == 0 and st["stats"]["n_rays"] == p.n_rays_total
        assert st["image"] is None
        t = plan.spectra_tensor()
        assert tuple(t.shape) == (p.n_rays_total, K) and t.data_ptr() == plan.spectra_ptr()
        v = t.view(nx, ny, na * nb, K)                                       # ray order: x, y, a, b with b fastest
        image = (v.sum(dim=2) * p.scale).permute(1, 0, 2).contiguous().cpu().numpy().ravel()   # [ny][nx][K]
        dv2 = torch.tensor(2.0 * b.dv, dtype=torch.float64, device=t.device)
        iang = torch.matmul(v, dv2).sum(dim=(0, 1)).view(na, nb).t().contiguous().cpu().numpy().ravel()  # k + m na
        del t, v
    e_img, e_ang = rel_l2(image, img["image"]), rel_l2(iang, img["I_ang"])
    note(f"stand-in 6 384 000 rays, sums of the spectra against image mode: image rel-L2 {e_img:.3e}, I_ang rel-L2 {e_ang:.3e}")
    assert np.linalg.norm(img["image"]) > 0 and np.linalg.norm(img["I_ang"]) > 0
    assert e_img < GATE and e_ang < GATE
    # element by element: the same rows summed in another order
    gate_outputs(dict(image=image, I_ang=iang), img, p, contribution_counts(p), "reordering", "spectra: stand-in 6 384 000 rays, sums of the spectra against image mode")


def test_spectra_sum_to_the_image_ase_small_host_arrays(hip, ase_small):
    p = ase_small
    b = p.beam
    assert own_cells(b.x, b.dx) and own_cells(b.y, b.dy) and own_cells(b.a, b.da) and own_cells(b.b, b.db)
    K, nx, ny, na, nb = b.nv, b.nx, b.ny, b.na, b.nb
    with hip.Plan(p) as plan:
        plan.set_ray_grid()
        img = plan.run().fetch()
        sp = plan.enable_spectra().run().fetch_spectra()
    assert not sp["err"].any()
    v = sp["Iv"].reshape(nx, ny, na * nb, K)
    image = (v.sum(axis=2) * p.scale).transpose(1, 0, 2).ravel()
    iang = (v @ (2.0 * b.dv)).sum(axis=(0, 1)).reshape(na, nb).T.ravel()
    e_img, e_ang = rel_l2(image, img["image"]), rel_l2(iang, img["I_ang"])
    note(f"ASE_small, sums of the spectra against image mode: image rel-L2 {e_img:.3e}, I_ang rel-L2 {e_ang:.3e}")
    assert e_img < GATE and e_ang < GATE
    gate_outputs(dict(image=image, I_ang=iang), img, p, contribution_counts(p), "reordering", "spectra: ASE_small, sums of the spectra against image mode")


def test_spectra_sum_to_the_image_seeded(hip, seed_small):
    p = seed_small
    rays = p.build_rays(np.arange(0, p.n_rays_total, 19, dtype=np.int64))
    assert len(rays) == 410685
    K = p.beam.nv
    with hip.Plan(p) as plan:
        plan.set_rays(rays)
        img = plan.run().fetch()
        sp = plan.enable_spectra().run().fetch_spectra()
    assert img["failure_code"] == 0 and not sp["err"].any()
    lhs = sp["Iv"].sum(axis=0) * p.scale
    rhs = img["image"].reshape(-1, K).sum(axis=0)
    e = rel_l2(lhs, rhs)
    note(f"seed_small, every 19th ray, sum over rays of Iv scale against sum over pixels of the image: rel-L2 {e:.3e}")
    assert np.linalg.norm(rhs) > 0 and e < GATE
    # per frequency: both sides are sums of the same len(rays) non-negative terms, in other orders
    assert_elements(lhs, rhs, np.full(K, len(rays)), reordering_tol(np.full(K, len(rays)), K), "spectra: seed_small, every 19th ray, sum over rays against sum over pixels, per frequency")


# ---------------------------------------------------------------- 3. return codes
def test_return_codes(hip, oracle, ase_small):
    p = copy.copy(ase_small)
    g = p.gain[2]
    K = g.Nv
    gv = g.gv.copy().reshape(g.Ny, g.Nx, K)
    gv[:, :g.Nx // 2, 5] = np.nan
    gv[:g.Ny // 3, g.Nx // 2:, :] *= -1
    p.gain = list(p.gain)
    p.gain[2] = rt.Gain(g.x, g.y, g.n, g.g0, g.E0, gv.reshape(g.gv.shape), g.Nv)
    rays = p.build_rays(np.arange(0, p.n_rays_total, 997, dtype=np.int64))
    assert len(rays) == 401
    rays["a"][7::40] = 1500.0
    ref = oracle.probe(p, rays)
    counts = {c: int((ref["err"] == c).sum()) for c in (0, -1, -2, -3)}
    note(f"return codes, oracle: {counts}")
    assert counts[-1] >= 10 and counts[-2] >= 10 and counts[-3] >= 10 and counts[0] >= 150
    with hip.Plan(p) as plan:
        plan.set_rays(rays).enable_spectra().run()
        out = plan.fetch_spectra()
        st = plan.fetch()
        exact = plan.set_exact_emission(True).run().fetch_spectra()
    check_against(out, ref, "return codes / plan")
    assert st["failure_code"] == 0b1110
    # (the clean rays here cross tables of both signs: gain and absorption cancel in Iv, which multiplies the one float
    # rounding of es / gs of the default update -- the exact mode shows what is left without it)
    check_against(exact, ref, "return codes / plan, exact emission")
    assert 0 < len(st["failed_rays"]) <= rt.cabi.RT_N_FAILED_MAX
    check_against(hip.calc_rays(p, rays), ref, "return codes / calc_rays")


# ---------------------------------------------------------------- 4. edges
def test_no_rays(hip, ase_small):
    K = ase_small.beam.nv
    with hip.Plan(ase_small) as plan:
        plan.set_rays(np.zeros(0, rt.cabi.RAY_DTYPE)).enable_spectra().run()
        out = plan.fetch_spectra()
        assert plan.fetch()["failure_code"] == 0
    assert out["Iv"].shape == (0, K) and len(out["ray2"]) == 0 and len(out["err"]) == 0
    out = hip.calc_rays(ase_small, np.zeros((0, 4)))
    assert out["Iv"].shape == (0, K) and len(out["ray2"]) == 0 and len(out["err"]) == 0


@pytest.mark.parametrize("n", [1, 65])
def test_one_ray_and_a_ragged_tile(hip, oracle, ase_small, n):
    rays = ase_small.build_rays(np.arange(n, dtype=np.int64) * 5003 + 1234)
    ref = oracle.probe(ase_small, rays)
    with hip.Plan(ase_small) as plan:
        out = plan.set_rays(rays).enable_spectra().run().fetch_spectra()
    assert check_against(out, ref, f"{n} rays / plan")[0] > 0
    check_against(hip.calc_rays(ase_small, rt.cabi.rays_to_array(rays)), ref, f"{n} rays / calc_rays, [n][4] input")


def test_row_stride_is_k_not_the_padded_k(hip, oracle, seed_small):
    assert seed_small.beam.nv == 82
    rays = seed_small.build_rays(np.arange(0, seed_small.n_rays_total, 40009, dtype=np.int64))
    ref = oracle.probe(seed_small, rays)
    assert ref["Iv"].any(axis=1).sum() >= 50
    with hip.Plan(seed_small) as plan:
        out = plan.set_rays(rays).enable_spectra().run().fetch_spectra()
    assert out["Iv"].shape == (len(rays), 82)
    check_against(out, ref, "seed_small, K = 82 / plan")
    check_against(hip.calc_rays(seed_small, rays), ref, "seed_small, K = 82 / calc_rays")


def test_strided_device_grid(hip, oracle, ase_small, seed_small):
    for p in (ase_small, problem_mod.regrid_seed_beam(seed_small, nx=9, ny=7, na=11, nb=6)):
        rays = p.build_rays(np.arange(3, p.n_rays_total, 7, dtype=np.int64))
        ref = oracle.probe(p, rays)
        with hip.Plan(p) as plan:
            out = plan.set_ray_grid(first=3, stride=7).enable_spectra().run().fetch_spectra()
        assert len(out["err"]) == len(rays)
        check_against(out, ref, f"strided grid ({len(rays)} rays, seeded {p.seed is not None})")


@pytest.mark.parametrize("which", ["ase", "seed"])
def test_escaped_rays(hip, oracle, ase_small, seed_small, which):
    p = ase_small if which == "ase" else seed_small
    rng = np.random.default_rng(4242)
    gx, gy = p.gain[1].x, p.gain[1].y
    n = 600
    rays = np.zeros(n, rt.cabi.RAY_DTYPE)
    rays["x"] = rng.uniform(gx[0] - 0.1 * (gx[-1] - gx[0]), gx[-1] + 0.1 * (gx[-1] - gx[0]), n)
    rays["y"] = rng.uniform(-1.1 * gy[-1], 1.1 * gy[-1], n)
    rays["a"] = rng.uniform(-60, 60, n)
    rays["b"] = rng.uniform(-60, 60, n)
    ref = oracle.probe(p, rays)
    assert int((ref["flags"] & 1).sum()) >= 20 and int(((ref["flags"] & 1) == 0).sum()) >= 20
    with hip.Plan(p) as plan:
        plan.set_rays(rays).enable_probe().enable_spectra().run()     # the probe is allowed beside the spectra
        out = plan.fetch_spectra()
        pr = plan.fetch_probe()
    check_against(out, ref, f"escaped rays ({which})")
    assert np.array_equal(pr["flags"] & 3, ref["flags"] & 3) and np.array_equal(pr["steps"], ref["steps"])
    assert ray2_bits_equal(pr["ray2"], out["ray2"], np.ones(n, bool))


def test_chunked_calc_rays_equals_unchunked(hip, ase_small, monkeypatch):
    rays = ase_small.build_rays(np.arange(0, ase_small.n_rays_total, 397, dtype=np.int64))
    assert len(rays) > 1000
    whole = hip.calc_rays(ase_small, rays)
    for chunk in ("128", "333"):
        monkeypatch.setenv("RT_HIP_CALC_RAYS_CHUNK", chunk)      # documented test hook: rays per chunk
        parts = hip.calc_rays(ase_small, rays)
        monkeypatch.delenv("RT_HIP_CALC_RAYS_CHUNK")
        assert np.array_equal(parts["Iv"], whole["Iv"]) and np.array_equal(parts["err"], whole["err"])
        assert np.array_equal(parts["ray2"].view(np.uint32), whole["ray2"].view(np.uint32))
        assert parts["stats"]["n_rays"] == len(rays) == whole["stats"]["n_rays"]
        assert parts["stats"]["cell_steps"] == whole["stats"]["cell_steps"]
    assert whole["Iv"].any()


def test_spectra_and_path_tracer_exclude_each_other(hip, ase_small):
    with hip.Plan(ase_small) as plan:
        plan.enable_spectra()
        with pytest.raises(hip.RayTraceError, match="status 1"):
            plan.enable_path()
    with hip.Plan(ase_small) as plan:
        plan.enable_path()
        with pytest.raises(hip.RayTraceError, match="status 1"):
            plan.enable_spectra()
    with hip.Plan(ase_small) as plan:      # a spectra run has no image to fetch or to write into
        plan.set_rays(ase_small.build_rays(np.arange(10))).enable_spectra().run()
        with pytest.raises(hip.RayTraceError, match="status 1"):
            plan.hl.check(plan.hl.lib.rt_hip_plan_fetch(plan._h, rt.cabi._dp(np.zeros(ase_small.beam.nx * ase_small.beam.ny * ase_small.beam.nv)),
                                                        None, None, None, 0, None, None), "rt_hip_plan_fetch")


def test_mode_switching_leaves_nothing_behind(hip, ase_small):
    """An image-mode run after a spectra run equals the image-mode run before it bit for bit.  Shapes whose image mode
    is itself reproducible: one ray per pixel (rows are stored, not added); with a single tile I_ang is one wave's sum
    as well.  (Where several waves add into I_ang the order of the additions differs between ANY two runs.)"""
    for nx, ny, iang_bitwise in ((8, 8, True), (70, 33, False)):
        p = problem_mod.regrid_beam(problem_mod.resample_frequency(ase_small, 64), nx=nx, ny=ny, a_centre=-1.0, b_centre=-4.5)
        with hip.Plan(p) as plan:
            plan.set_ray_grid()
            a = plan.run().fetch()
            sp = plan.enable_spectra().run().fetch_spectra()
            assert plan.spectra_ptr() != 0
            b = plan.enable_spectra(False).run().fetch()
            assert plan.spectra_ptr() == 0
        assert sp["Iv"].any() and a["image"].any()
        assert np.array_equal(a["image"], b["image"])
        assert a["failure_code"] == b["failure_code"] == 0 and a["stats"]["cell_steps"] == b["stats"]["cell_steps"]
        if iang_bitwise:
            assert np.array_equal(a["I_ang"], b["I_ang"])
        else:
            assert rel_l2(a["I_ang"], b["I_ang"]) < 1e-13


# ---------------------------------------------------------------- 5. randomised problems
def test_random_problems_match_the_oracle(hip, oracle, ase_small, seed_small):
    from test_gpu_fuzz import random_case, random_grid_case

    tot = dict(rays=0, seeded=0, escaped=0, rows=0, zero_cases=0)
    for i in range(40):
        rng = np.random.default_rng(9000 + i)
        if i % 2 == 0:
            p, rays = random_case(rng, ase_small, seed_small)
        else:
            p, _ = random_grid_case(rng, ase_small, seed_small)
            rays = p.build_rays()
        ref = oracle.probe(p, rays)
        assert not ref["err"].any(), f"case {i}: the oracle reports failing rays"
        with hip.Plan(p) as plan:
            (plan.set_rays(rays) if i % 2 == 0 else plan.set_ray_grid()).enable_spectra().run()
            out = plan.fetch_spectra()
            assert plan.fetch()["failure_code"] == 0
        rows, nzero = check_against(out, ref, f"random case {i} (N = {p.N}, K = {p.beam.nv}, {len(rays)} rays, seeded {p.seed is not None})")
        assert rows + nzero == len(rays)                # no ray is left out
        if i % 8 == 0:                                  # and through the host-pointer entry
            check_against(hip.calc_rays(p, rays), ref, f"random case {i} / calc_rays")
        tot["rays"] += len(rays)
        tot["seeded"] += p.seed is not None
        tot["escaped"] += int((ref["flags"] & 1).sum())
        tot["rows"] += rows
        tot["zero_cases"] += rows == 0
    note(f"random problems: {tot}")
    assert tot["rows"] >= 40000 and tot["rays"] >= 50000
