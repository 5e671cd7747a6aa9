"""Device tier of the seed-profile tests: the seed factor f0 fx fy fa fb as the device computes it, on the crafted profiles
of tests/seed_profiles.py (non-uniform axes, limiter data, plateaus, sign changes, short axes, a narrow range on float32
nodes, overflowing data), against the reference's own RayTrace::calc_seed as tests/golden/seed_profiles_ref.npz records it.

  pchip, seed_factor   pchip_eval and seed_factor of csrc/rt_math.h behind one elementwise kernel each
                       (csrc/librt_hip_devmath.so): BIT-EQUAL to the fixture on every point, a NaN for a NaN.  The two are
                       IEEE double add, mul, div and compare, built with -ffp-contract=off -fno-fast-math: a difference
                       is a finding about the compiler or the code, not noise.  Launches of 1, 63 and 65 points give the
                       prefix of the whole launch; NaN and +-inf give f = 0
  seed_tab             the product's rt_seed_tab_kernel (csrc/rt_march.hip), unchanged, on grids with out-of-range entries
                       on both sides, entries on the end nodes, entries whose float rounding crosses an end node in either
                       direction, NaN and +-inf; 4, 255, 257 and 3003 entries (one thread, a ragged last work-group, and
                       fewer work-groups than entries need: the grid-stride loop).  Every sf / sin equals the per-point
                       kernel at (double)(float) g[i]; f0 sf sf sf sf with the flags, in place_ray's order, equals
                       seed_factor at the same float points, bitwise
  through the C ABI    three 450-ray problems (seed_small's gains and frequency axis, seven tiles and a ragged one of two
                       rays) that carry a crafted profile: the plan on the ray grid (seed tables), the same rays as a list
                       (seed_factor per ray) and rt_hip_image_loop against oracle.image_loop, element by element at
                       TIGHT_TIER; grid against list at the reordering bound; spectra (plan and rt_hip_calc_rays) against
                       oracle.probe; step outputs against the reduced oracle cube; the stored case against the
                       reference's own image / I_ang

The measured figures are printed before every assertion; DEVMATH_PARITY_FILE / ELEMENT_PARITY_FILE append them to a file
(profiles/seed_parity.txt is such a run on an MI355X)."""
import numpy as np
import pytest

import devmath as dm
import devmath_inputs as di
import seed_profiles as sp
from element_gate import TIGHT_TIER, counts_from_oracle, gate_outputs
from test_gpu_devmath import assert_prefixes
from test_gpu_spectra import check_against
from test_gpu_step import gate_step, reduced

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    return dm.Device.get()


@pytest.fixture(scope="module")
def fixture():
    return sp.load_fixture()


def assert_same_bits(name, got, want, describe):
    bad = sp.differing(got, want)
    dm.note(f"{name}: {np.asarray(want).size} values compared, {bad.size} differ from the reference")
    if bad.size:
        g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        raise AssertionError(f"{name}: {bad.size} of {w.size} differ; first at {describe(int(bad[0]))}: device {float(g[bad[0]]).hex()}, "
                             f"reference {float(w[bad[0]]).hex()}")


# ---------------------------------------------------------------------------------------------- pchip, seed_factor
@pytest.mark.parametrize("name", list(sp.profiles()))
def test_pchip_equals_the_reference_bit_for_bit(dev, fixture, name):
    fx = fixture[0][name]
    seed, pts = fx["seed"], fx["pts"]
    for d in range(4):
        x = np.ascontiguousarray(pts[:, d])
        got = dev.pchip(seed.x[d], seed.f[d], x)
        assert_same_bits(f"device pchip_eval, profile {name} axis {d}", got, fx["axis"][:, d], lambda i: f"x = {x[i]!r} ({float(x[i]).hex()})")
        assert_prefixes(f"pchip {name} {d}", lambda n: dev.pchip(seed.x[d], seed.f[d], x[:n]), got)
    assert len(pts) % 256 not in (0, 1) and len(pts) > 256          # more than one work-group, a ragged last one


@pytest.mark.parametrize("name", list(sp.profiles()))
def test_seed_factor_equals_the_reference_bit_for_bit(dev, fixture, name):
    fx = fixture[0][name]
    seed, pts = fx["seed"], fx["pts"]
    got = dev.seed_factor(seed, pts)
    with np.errstate(invalid="ignore", over="ignore"):
        Iv = got[:, None] * np.asarray(seed.f[4])[None, :]          # RayTrace::calc_seed: Iv[k] = f * seed.f[4][k], f[4][1] = 1
    assert seed.f[4][1] == 1.0
    assert_same_bits(f"device seed_factor, profile {name}", Iv, fx["Iv"], lambda i: f"point {pts[i // 3].tolist()}, k = {i % 3}")
    assert_prefixes(f"seed_factor {name}", lambda n: dev.seed_factor(seed, pts[:n]), got)
    # non-finite coordinates: outside the range, f = 0
    bad = ~np.isfinite(pts).all(axis=1)
    assert bad.sum() >= 36 and np.isnan(pts).any() and np.isinf(pts).any()
    assert (got[bad] == 0).all() and not np.signbit(got[bad]).any()
    # nothing negative leaves the clamp (a NaN stays a NaN, as in the reference)
    assert not (got < 0).any()


# ---------------------------------------------------------------------------------------------- seed_tab
def tab_seed(which):
    """A profile whose end nodes lie BESIDE float32 values on two axes (so that rounding a grid value to float crosses
    them) and ON float32 values on the other two.  which = "limiter" or "sign" (negative factors: the clamp)."""
    f32 = lambda v: float(np.float32(v))
    d = 2.0 ** -40
    lo_hi = [(f32(-0.3) - d, f32(0.45) - d), (f32(0.1) + d, f32(0.35) + d), (f32(-0.7), f32(-0.05)), (f32(-0.2), f32(0.6))]
    like = sp.profiles()[which]
    return sp.rescaled(like, like, lo_hi), lo_hi, d


def tab_grids(lo_hi, d, sizes):
    """Four grids of the given sizes: the special entries first (as many as fit), then evenly spread values from below
    the range to above it."""
    out = []
    for a, n in enumerate(sizes):
        lo, hi = lo_hi[a]
        span = hi - lo
        special = [lo, hi,                                             # on the end nodes (axes 2, 3: float values, stay there)
                   lo - d / 2, hi + d / 2,                             # the double outside; its float inside on axis 0 (lo) and 1 (hi)
                   np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf),
                   np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf),
                   lo - 0.1 * span, hi + 0.1 * span, lo - 1e3, hi + 1e3,   # out of range on both sides
                   np.nan, np.inf, -np.inf, 1e300, -1e300]             # (1e300 rounds to the float infinity)
        fill = np.linspace(lo - 0.15 * span, hi + 0.15 * span, max(n - len(special), 0))
        g = np.concatenate([special, fill])[:n] if n > 1 else np.array([lo + 0.37 * span])
        out.append(np.ascontiguousarray(g, dtype=np.float64))
    return out


TAB_SIZES = {4: (1, 1, 1, 1), 255: (100, 60, 50, 45), 257: (100, 60, 50, 47), 3003: (1200, 700, 600, 503)}


@pytest.mark.parametrize("which", ["limiter", "sign"])
@pytest.mark.parametrize("total", sorted(TAB_SIZES))
def test_seed_tab_equals_the_per_point_kernel(dev, which, total):
    seed, lo_hi, d = tab_seed(which)
    sizes = TAB_SIZES[total]
    assert sum(sizes) == total
    grids = tab_grids(lo_hi, d, sizes)
    sf, sin = dev.seed_tab(seed, grids)
    assert sf.shape == sin.shape == (total,)
    if total > 2048:        # 12 work-groups do it in the product's launch; 3 and 1 must walk the entries in the loop
        for n_blocks in (3, 1):
            sf2, sin2 = dev.seed_tab(seed, grids, n_blocks=n_blocks)
            assert sp.same_bits(sf2, sf) and np.array_equal(sin2, sin), f"{n_blocks} work-groups give other tables"
    with np.errstate(over="ignore", invalid="ignore"):
        v = [g.astype(np.float32).astype(np.float64) for g in grids]      # (double)(float) g[i]
    off = np.cumsum([0] + list(sizes))
    crossed = {"in_to_out": 0, "out_to_in": 0, "on_node": 0, "below": 0, "above": 0}
    for a in range(4):
        lo, hi = seed.x[a][0], seed.x[a][-1]
        with np.errstate(invalid="ignore"):
            inside = (v[a] >= lo) & (v[a] <= hi)
            inside_double = (grids[a] >= lo) & (grids[a] <= hi)
        want = np.where(inside, dev.pchip(seed.x[a], seed.f[a], v[a]), 0.0)
        got_sf, got_in = sf[off[a]:off[a + 1]], sin[off[a]:off[a + 1]]
        assert np.array_equal(got_in, inside.astype(np.uint8)), (a, grids[a][got_in != inside], got_in[got_in != inside])
        assert_same_bits(f"rt_seed_tab_kernel, {which}, {total} entries, axis {a}", got_sf, want, lambda i: f"g = {grids[a][i]!r}")
        crossed["in_to_out"] += int((inside_double & ~inside).sum())
        crossed["out_to_in"] += int((~inside_double & inside).sum())
        crossed["on_node"] += int(((v[a] == lo) | (v[a] == hi)).sum())
        crossed["below"] += int((v[a] < lo).sum())
        crossed["above"] += int((v[a] > hi).sum())
        nonfin = ~np.isfinite(v[a])
        assert (got_sf[nonfin] == 0).all() and (got_in[nonfin] == 0).all()
    dm.note(f"rt_seed_tab_kernel, {which}, {total} entries: {crossed}")
    if total > 4:
        assert all(c >= 2 for c in crossed.values()), crossed
    # the product of the tables, as place_ray forms it, against seed_factor at the same float points
    rng = np.random.default_rng(total)
    idx = np.stack([rng.integers(0, n, 2000) for n in sizes], axis=1)
    idx[:min(sizes)] = np.arange(min(sizes))[:, None]                     # the special entries of all four axes together
    with np.errstate(over="ignore", invalid="ignore"):
        f = seed.f0 * sf[off[0] + idx[:, 0]] * sf[off[1] + idx[:, 1]] * sf[off[2] + idx[:, 2]] * sf[off[3] + idx[:, 3]]
        f = np.where(f < 0.0, 0.0, f)
    flags = sin[off[0] + idx[:, 0]] & sin[off[1] + idx[:, 1]] & sin[off[2] + idx[:, 2]] & sin[off[3] + idx[:, 3]]
    f = np.where(flags != 0, f, 0.0)
    pts = np.stack([v[a][idx[:, a]] for a in range(4)], axis=1)
    direct = dev.seed_factor(seed, pts)
    assert_same_bits(f"f0 sf sf sf sf against seed_factor, {which}, {total} entries", f, direct, lambda i: f"point {pts[i].tolist()}")
    if total > 4:
        assert (flags != 0).sum() >= 100 and (flags == 0).sum() >= 100
        if which == "sign":
            raw = seed.f0 * sf[off[0] + idx[:, 0]] * sf[off[1] + idx[:, 1]] * sf[off[2] + idx[:, 2]] * sf[off[3] + idx[:, 3]]
            assert ((raw < 0) & (flags != 0)).sum() >= 50, "the clamp is not reached"


# ---------------------------------------------------------------------------------------------- through the C ABI
@pytest.mark.parametrize("case", sp.E2E_CASES)
def test_profiles_through_the_c_abi(hip, oracle, seed_small, fixture, case):
    p = sp.e2e_problem(seed_small, case)
    p.validate()
    rays = p.build_rays()
    assert len(rays) == 450 and len(rays) % 64 == 2
    # the conditions the case is there for, from the census of its 450 float rays
    tot, n_in, per_axis = sp.ray_census(p.seed, rays)
    dm.note(f"C ABI, profile {case}: {n_in} of 450 rays in range; per axis (in, out) {per_axis}; "
            + ", ".join(f"{k} {tot[k]}" for k in sp.E2E_TARGETS[case]))
    assert n_in >= 90
    for k in sp.E2E_TARGETS[case]:
        assert tot[k] >= 0.1 * n_in, (case, k, tot[k], n_in)
    if case == "narrow":
        assert all(i > 0 and o > 0 for i, o in per_axis), per_axis
    ora = oracle.image_loop(p, rays)
    assert ora["failure_code"] == 0 and np.count_nonzero(ora["image"]) > 0 and np.count_nonzero(ora["I_ang"]) > 0
    counts = counts_from_oracle(oracle, p, rays)
    label = f"C ABI, profile {case}"
    # image mode: the ray grid (seed tables), the same rays as a list (seed_factor per ray), the host-pointer loop
    with hip.Plan(p) as plan:
        grid = plan.set_ray_grid().run().fetch()
        assert plan.n_rays == 450
        lst = plan.set_rays(rays).run().fetch()
        # spectra: list and grid
        plan.enable_spectra().run()
        spec_list = plan.fetch_spectra()
        plan.set_ray_grid().run()
        spec_grid = plan.fetch_spectra()
        plan.enable_spectra(False)
        # step outputs: grid and list
        plan.enable_step().run()
        step_grid = plan.fetch_step()
        assert plan.fetch()["failure_code"] == 0
        plan.set_rays(rays).run()
        step_list = plan.fetch_step()
        assert plan.fetch()["failure_code"] == 0
    loop = hip.image_loop(p, rays)
    for name, out in (("ray grid", grid), ("ray list", lst), ("rt_hip_image_loop", loop)):
        assert out["failure_code"] == 0 and len(out["failed_rays"]) == 0, (label, name)
        assert out["stats"]["cell_steps"] == ora["counters"]["cell_steps"], (label, name)
        gate_outputs(out, ora, p, counts, TIGHT_TIER, f"{label} / {name} against the oracle")
    gate_outputs(grid, lst, p, counts, "reordering", f"{label} / ray grid against ray list")
    probe = oracle.probe(p, rays)
    assert not probe["err"].any()
    for name, out in (("plan, list", spec_list), ("plan, grid", spec_grid), ("rt_hip_calc_rays", hip.calc_rays(p, rays))):
        rows, nzero = check_against(out, probe, f"{label} / spectra / {name}")
        assert rows + nzero == 450 and rows >= n_in - int(tot["product_negative_clamped"]) - int(tot["product_minus_zero"])
        assert nzero >= 450 - n_in
    cube = reduced(hip, p, ora)
    gate_step(step_grid, cube, p, counts, TIGHT_TIER, f"{label} / step, ray grid against the oracle's cube")
    gate_step(step_list, cube, p, counts, TIGHT_TIER, f"{label} / step, ray list against the oracle's cube")
    e2e = fixture[1]
    if case == e2e["case"]:
        for name, out in (("ray grid", grid), ("ray list", lst), ("rt_hip_image_loop", loop)):
            gate_outputs(out, e2e, p, counts, TIGHT_TIER, f"{label} / {name} against the reference's own outputs")


def test_the_stored_case_is_one_of_the_cases(fixture):
    assert fixture[1]["case"] in sp.E2E_CASES
