"""CPU tier of the seed-profile tests: the oracle's seed evaluation (pchip_eval / seed_intensity of oracle/rt_oracle.c,
exported as rt_oracle_calc_seed) against the reference's own RayTrace::calc_seed on the crafted profiles of
tests/seed_profiles.py, as tests/golden/seed_profiles_ref.npz records it (tests/golden/make_golden.py).

  bit equality   every per-axis interpolant and every Iv of the oracle equals the fixture bit for bit (a NaN for a NaN);
                 oracle.image_loop on the stored 450-ray case equals the reference's image / I_ang bit for bit
  census         every branch label of the Python restatement (seed_profiles.pchip / seed_factor) is taken at least 20
                 times over the fixture's points; the shipped profile's census is printed beside it
  sensitivity    every mutant of seed_profiles.MUTANTS moves a fixture value by more than 1e-6 relative
  long double    the reference's double result against the same formula in numpy.longdouble, per value, scaled by
                 max(|fl|, |fr|, |gl|, |gr|) of its interval

Measured (profiles/seed_parity.txt): the reference's double result lies within 2.961e-16 of the long-double evaluation
in that scale (profile plateau, axis 0, x = -0.7187500000000001; 17284 values on the in-range queries of six profiles;
`huge` is left out: fl - fr overflows a double there by design).  The bound asserted is 4 times that figure, 1.2e-15;
it covers nothing but the rounding of about 20 operations."""
from collections import Counter

import numpy as np
import pytest

import seed_profiles as sp
from devmath import note, require_long_double

LONG_DOUBLE_BOUND = 1.2e-15      # 4 x the worst figure measured, 2.961e-16 (docstring)


@pytest.fixture(scope="module")
def fixture():
    return sp.load_fixture()


def test_oracle_equals_the_reference_bit_for_bit(oracle, fixture):
    profs, _ = fixture
    for name, fx in profs.items():
        got = oracle.calc_seed(fx["seed"], fx["pts"])
        for key in ("axis", "Iv"):
            bad = sp.differing(got[key], fx[key])
            note(f"oracle calc_seed, profile {name}, {key}: {fx[key].size} values at {len(fx['pts'])} points, {bad.size} differ from the reference")
            assert bad.size == 0, (name, key, fx["pts"][bad[0] // fx[key].shape[1]], got[key].reshape(-1)[bad[0]], fx[key].reshape(-1)[bad[0]])
        assert fx["Iv"].shape == (len(fx["pts"]), 3) and fx["axis"].shape == (len(fx["pts"]), 4)
        # the restatement that carries the census is the same function
        own = sp.evaluate(fx["seed"], fx["pts"])
        assert sp.same_bits(own["axis"], fx["axis"]) and sp.same_bits(own["Iv"], fx["Iv"]), name


def test_stored_case_bitwise_vs_reference_outputs(oracle, seed_small, fixture):
    _, e2e = fixture
    assert e2e["case"] == sp.E2E_STORED
    p = sp.e2e_problem(seed_small, e2e["case"])
    p.validate()
    out = oracle.image_loop(p)                 # serial: the summation order matters for bit equality
    assert out["failure_code"] == 0 and out["counters"]["n_rays"] == 450
    assert np.array_equal(out["image"], e2e["image"])
    assert np.array_equal(out["I_ang"], e2e["I_ang"])
    assert np.count_nonzero(e2e["image"]) > 0 and np.count_nonzero(e2e["I_ang"]) > 0


def shipped_census(seed_small):
    """The census of the shipped profile at the float-rounded values of its own ray grid (what grid mode evaluates)."""
    T = sp.Tables(seed_small.seed)
    cnt = Counter()
    for d, g in enumerate(seed_small.ray_grid):
        for v in np.asarray(g, dtype=np.float64).astype(np.float32).astype(np.float64):
            pt = [float(T.x[e][1]) for e in range(4)]
            pt[d] = float(v)
            c = Counter()
            sp.seed_factor(T, pt, c)
            if c["in_range"]:                   # the other three coordinates sit on a node: count axis d alone
                sp.pchip(len(T.x[d]), T.x[d], T.f[d], pt[d], cnt)
                cnt["in_range"] += 1
            else:
                cnt += c
    return cnt


def test_census_every_branch_is_taken(fixture, seed_small):
    profs, _ = fixture
    tot, per = Counter(), {}
    for name, fx in profs.items():
        per[name] = Counter()
        sp.evaluate(fx["seed"], fx["pts"], cnt=per[name])
        tot += per[name]
    shipped = shipped_census(seed_small)
    note(f"census over {sum(len(fx['pts']) for fx in profs.values())} points of {len(profs)} profiles | the shipped profile at its "
         f"{sum(len(g) for g in seed_small.ray_grid)} grid values")
    for k in sp.REQUIRED_LABELS:
        note(f"  {k:38s} {tot[k]:7d} | {shipped[k]:5d}")
    assert set(tot) - {k for k in tot if k.startswith("alone_")} <= set(sp.REQUIRED_LABELS), "a label the list does not know"
    low = {k: tot[k] for k in sp.REQUIRED_LABELS if tot[k] < 20}
    assert not low, f"branches taken fewer than 20 times: {low}"
    # what each profile is there for
    assert per["short"]["end_lo_by_n2"] >= 20
    assert per["short"]["interior"] == per["short"]["gl_first_interval"] + per["short"]["gr_last_interval"] >= 40   # dim 3: i <= 1 or i >= n - 1
    assert per["plateau"]["gl_zero_by_fl_eq_fr"] >= 20 and per["plateau"]["gl_zero_by_fl_eq_outer"] >= 20 and per["plateau"]["gr_zero_by_fr_eq_outer"] >= 20
    assert per["sign"]["product_negative_clamped"] >= 20 and per["sign"]["product_positive_of_two_negative"] >= 20 and per["sign"]["product_minus_zero"] >= 20
    for side in ("gl", "gr"):
        assert per["limiter"][f"{side}_limited_pos"] >= 20 and per["limiter"][f"{side}_limited_neg"] >= 20
    assert per["narrow"]["in_on_first_node"] >= 20 and per["narrow"]["in_on_last_node"] >= 20
    for d in range(4):
        ends = profs["narrow"]["seed"].x[d][[0, -1]]
        assert np.array_equal(ends, ends.astype(np.float32).astype(np.float64)), "narrow: an end node is no float32 value"
    # non-uniform axes: neighbouring spacings in ratios from 1/3 to 3, both ends reached
    ratios = np.concatenate([np.diff(profs["nonuniform"]["seed"].x[d])[1:] / np.diff(profs["nonuniform"]["seed"].x[d])[:-1] for d in range(4)])
    assert ratios.min() < 0.3334 and ratios.max() > 2.9999 and ratios.min() > 0.3333 and ratios.max() < 3.0001


def moved(mut, ref):
    """Largest relative move |mut - ref| / max(|mut|, |ref|) over the values; a number against a NaN or an infinity
    against a number counts as infinite."""
    mut, ref = np.asarray(mut).reshape(-1), np.asarray(ref).reshape(-1)
    with np.errstate(all="ignore"):
        rel = np.abs(mut - ref) / np.maximum(np.abs(mut), np.abs(ref))
    rel = np.where((mut == ref) | (np.isnan(mut) & np.isnan(ref)), 0.0, rel)
    rel = np.where(np.isnan(rel), np.inf, rel)
    return float(rel.max()), int(np.argmax(rel))


@pytest.mark.parametrize("mutant", sp.MUTANTS)
def test_every_mutant_moves_a_fixture_value(fixture, mutant):
    profs, _ = fixture
    worst = {}
    for name, fx in profs.items():
        got = sp.evaluate(fx["seed"], fx["pts"], mut=frozenset([mutant]))
        worst[name] = max(moved(got["axis"], fx["axis"])[0], moved(got["Iv"], fx["Iv"])[0])
    note(f"mutant {mutant}: largest relative move per profile: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) > 1e-6, f"the mutant {mutant} survives: the profiles are too weak"


def test_unmutated_restatement_moves_nothing(fixture):
    profs, _ = fixture
    for name, fx in profs.items():
        got = sp.evaluate(fx["seed"], fx["pts"])
        assert moved(got["axis"], fx["axis"])[0] == 0 and moved(got["Iv"], fx["Iv"])[0] == 0, name


def long_double_figures(profs, values):
    """Per profile and axis: (worst |value - long double| / scale, x where, values compared) on the finite in-range
    queries; values(name, d, rows) gives the doubles to judge (the fixture's, or a device's)."""
    require_long_double()
    out = {}
    for name, fx in profs.items():
        if name == "huge":          # fl - fr overflows a double there by design: no rounding figure
            continue
        for d in range(4):
            xs = fx["seed"].x[d]
            q = fx["pts"][:, d]
            rows = np.flatnonzero(np.isfinite(q) & (q >= xs[0]) & (q <= xs[-1]))
            ref, scale = sp.evaluate_long_double(fx["seed"], d, q[rows])
            got = np.asarray(values(name, d, rows), dtype=np.float64).astype(sp.LD)
            assert (scale > 0).all()
            err = (np.abs(got - ref) / scale).astype(np.float64)
            i = int(np.argmax(err))
            out[(name, d)] = (float(err[i]), float(q[rows][i]), len(rows))
    return out


def test_long_double_figure(fixture):
    """The reference's double result against the long-double evaluation of the same formula: worst 2.961e-16 of
    max(|fl|, |fr|, |gl|, |gr|) (measured; the rounding of about 20 operations), asserted below 4 x that = 1.2e-15."""
    profs, _ = fixture
    figs = long_double_figures(profs, lambda name, d, rows: profs[name]["axis"][rows, d])
    for (name, d), (w, x, n) in figs.items():
        note(f"reference pchip against long double, profile {name} axis {d}: {n} values, worst {w:.3e} of max(|fl|, |fr|, |gl|, |gr|) at x = {x!r}")
    w = max(v[0] for v in figs.values())
    note(f"reference pchip against long double: worst {w:.3e} over {sum(v[2] for v in figs.values())} values, bound {LONG_DOUBLE_BOUND:g}")
    assert w <= LONG_DOUBLE_BOUND
    assert w > 1e-17, "no rounding error at all: the long-double evaluation is not one"
