"""The element gate itself (tests/element_gate.py), on the CPU: that its deposit rule is the oracle's, that the
references agree with each other under its tight tier, that it rejects defects which the whole-array rel-L2 gate of
2e-7 lets through by orders of magnitude, and its edge rules."""
import numpy as np
import pytest

from conftest import rel_l2
from element_gate import (DEFAULT_TIER, TIGHT_TIER, assert_elements, contribution_counts, counts_from_oracle,
                          deposit_cells, deposit_index, element_figures, gate_outputs, numpy_deposit, reordering_tol)

WHOLE_ARRAY_GATE = 2e-7


@pytest.fixture(scope="module")
def ase(oracle, ase_small):
    """ASE_small, all rays: the oracle's image loop, its per-ray probe and the counts."""
    rays = ase_small.build_rays()
    return dict(p=ase_small, rays=rays, loop=oracle.image_loop(ase_small, rays), probe=oracle.probe(ase_small, rays),
                counts=contribution_counts(ase_small))


@pytest.fixture(scope="module")
def seeded(oracle, seed_small):
    """seed_small, every 19th ray."""
    rays = seed_small.build_rays(np.arange(0, seed_small.n_rays_total, 19, dtype=np.int64))
    probe = oracle.probe(seed_small, rays)
    return dict(p=seed_small, rays=rays, loop=oracle.image_loop(seed_small, rays), probe=probe,
                counts=contribution_counts(seed_small, rays, probe["ray2"], probe["err"]))


# ---------------------------------------------------------------------------------------------- deposit replay
@pytest.mark.parametrize("which", ["ase", "seeded"])
def test_numpy_deposit_of_the_probe_is_the_oracles_image_loop(which, ase, seeded):
    c = ase if which == "ase" else seeded
    p, counts = c["p"], c["counts"]
    assert c["loop"]["failure_code"] == 0 and not c["probe"]["err"].any()
    image, iang = numpy_deposit(p, c["rays"], c["probe"])
    figs = gate_outputs(dict(image=image, I_ang=iang), c["loop"], p, counts, "reordering", f"deposit replay, {which}")
    assert figs["image"]["count"] == image.size and figs["I_ang"]["count"] == iang.size
    # every ray is accounted for: what does not land on the image is off its grid
    ix, iy, ia, ib = deposit_cells(p, c["rays"], c["probe"]["ray2"])
    assert counts[0].sum() == int(((ix >= 0) & (iy >= 0)).sum()) and counts[1].sum() == int(((ia >= 0) & (ib >= 0)).sum())
    assert counts[0].sum() > 0 and (c["loop"]["image"].reshape(len(counts[0]), -1)[counts[0] == 0] == 0).all()


def test_closed_form_counts_of_an_own_cell_grid_equal_the_counted_ones(ase, oracle):
    p = ase["p"]
    n_img, n_ang = contribution_counts(p, ase["rays"])
    assert np.array_equal(n_img, ase["counts"][0]) and np.array_equal(n_ang, ase["counts"][1])
    assert n_img[0] == p.beam.na * p.beam.nb and n_ang[0] == p.beam.nx * p.beam.ny
    part = ase["rays"][5::7]
    a, b = counts_from_oracle(oracle, p, part, n_threads=3), contribution_counts(p, part)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].sum() == len(part)


def test_deposit_index_is_the_references_rule_at_the_cell_edges():
    g, d = np.array([1.0, 2.0, 3.0, 4.0]), 1.0
    v = np.array([0.49, 0.5, 0.75, 1.5, 1.5000001, 2.5, 2.5000001, 4.5, 4.51, np.nan])
    # v - d/2 == g[0] (v = 1.5) is cell 1: the reference's bisection never tests g[0] (first_not_below in rt_oracle.c)
    assert deposit_index(g, d, v).tolist() == [-1, 0, 0, 1, 1, 1, 2, 3, -1, 3]


# ---------------------------------------------------------------------------------------------- reference agreement
def test_threaded_oracle_and_reference_fixtures_agree_under_the_tight_tier(oracle, ase, seed_small, ase_ref, seed_ref):
    p = ase["p"]
    th = oracle.image_loop(p, ase["rays"], n_threads=8)
    gate_outputs(th, ase["loop"], p, ase["counts"], TIGHT_TIER, "oracle, 8 threads against serial, ASE_small")
    gate_outputs(ase["loop"], ase_ref, p, ase["counts"], TIGHT_TIER, "oracle against ASE_small_ref_cpu.npz")
    whole = oracle.image_loop(seed_small, n_threads=8)
    gate_outputs(whole, seed_ref, seed_small, counts_from_oracle(oracle, seed_small), TIGHT_TIER,
                 "oracle, 8 threads, against seed_small_ref_cpu.npz")


# ---------------------------------------------------------------------------------------------- teeth
def _rejected(got, ref, n_e, label, dims):
    l2 = rel_l2(got, ref)
    fig = element_figures(got, ref, n_e)
    print(f"{label}: whole-array rel-L2 {l2:.3e} (gate {WHOLE_ARRAY_GATE:g} passes), worst element {fig['worst']:.3e}")
    assert l2 < WHOLE_ARRAY_GATE, "the defect must be one that the whole-array gate lets through -- that is the point"
    with pytest.raises(AssertionError, match="fail the element gate"):
        assert_elements(got, ref, n_e, DEFAULT_TIER, label, dims)
    return l2, fig["worst"]


def _dimmest_pixel(image, K):
    rows = image.reshape(-1, K)
    s = rows.sum(axis=1)
    return int(np.argmin(np.where(s > 0, s, np.inf)))


def test_defects_that_pass_the_whole_array_gate_are_rejected_element_by_element(ase, seeded):
    p, probe, ref = ase["p"], ase["probe"], ase["loop"]["image"]
    b = p.beam
    K, dims, n_e = b.nv, (b.ny, b.nx, b.nv), ase["counts"][0]
    ix, iy, ia, ib = deposit_cells(p, ase["rays"])
    pix = _dimmest_pixel(ref, K)
    r = int(np.flatnonzero(ix + iy * b.nx == pix)[0])
    assert probe["Iv"][r].any()
    # (1) one ray of the dimmest pixel is lost
    got = ref.reshape(-1, K).copy()
    got[pix] -= probe["Iv"][r] * p.scale
    l2, worst = _rejected(got, ref, n_e, "a ray of the dimmest pixel dropped", dims)
    assert l2 < 1e-8 and worst > 1e-4
    # ... and I_ang, where the lost ray shows only in one cell of 1500 rays: reported, not required to trip
    ang = ase["loop"]["I_ang"].copy()
    ang[ia[r] + ib[r] * b.na] -= float((probe["Iv"][r] * 2.0 * b.dv).sum())
    print("the same ray missing from I_ang: worst element", element_figures(ang, ase["loop"]["I_ang"], ase["counts"][1])["worst"])
    # (2) the same ray lands in the neighbouring pixel
    nb_pix = pix + 1 if (pix % b.nx) + 1 < b.nx else pix - 1
    got[nb_pix] += probe["Iv"][r] * p.scale
    _rejected(got, ref, n_e, "the same ray deposited into the neighbouring pixel", dims)
    # (3) the last frequency of every pixel is off by 1e-4
    got = ref.reshape(-1, K).copy()
    got[:, K - 1] *= 1.0 + 1e-4
    l2, worst = _rejected(got, ref, n_e, "k = K - 1 of every pixel off by 1e-4", dims)
    assert 0.5e-4 < worst < 2e-4
    # (4) one element of the dimmest decile off by 1e-4: the image of ASE_small, and I_ang of seed_small (the I_ang of
    # ASE_small spans a factor of 20 only, so there the whole-array gate does see one cell)
    sb = seeded["p"].beam
    for c, key, n, dm in ((ase, "image", n_e, dims), (seeded, "I_ang", seeded["counts"][1], (sb.nb, sb.na))):
        want = c["loop"][key]
        nz = np.flatnonzero(want > 0)
        i = nz[np.argsort(want[nz])[len(nz) // 20]]            # the middle of the dimmest decile
        got = want.copy()
        got[i] *= 1.0 + 1e-4
        _rejected(got, want, n, f"one element of the dimmest decile of {key} times 1 + 1e-4", dm)
        # and the tight tier sees a change of 1e-10 there, the reordering tier one of 1e-12
        got[i] = want[i] * (1.0 + 1e-10)
        with pytest.raises(AssertionError):
            assert_elements(got, want, n, TIGHT_TIER, "1e-10 at the tight tier", dm)
        got[i] = want[i] * (1.0 + 1e-12)
        assert_elements(got, want, n, TIGHT_TIER, "1e-12 at the tight tier", dm)
        with pytest.raises(AssertionError):
            assert_elements(got, want, n, reordering_tol(n, c["p"].beam.nv), "1e-12 at the reordering tier", dm)


# ---------------------------------------------------------------------------------------------- edges
def test_edge_rules_of_the_gate():
    ref = np.array([1.0, 0.0, 3.0, 5e-324 * 7, 2.0, 0.0])
    n_e = np.array([4, 0, 2, 3, 1, 2])
    assert_elements(ref.copy(), ref, n_e, DEFAULT_TIER, "identical")
    # a stray value where nothing is deposited
    got = ref.copy()
    got[1] = 1e-300
    with pytest.raises(AssertionError, match="n_e 0"):
        assert_elements(got, ref, n_e, DEFAULT_TIER, "stray value")
    # a NaN on one side only; the same NaN, or the same infinity, on both sides is equal
    got = ref.copy()
    got[2] = np.nan
    with pytest.raises(AssertionError):
        assert_elements(got, ref, n_e, DEFAULT_TIER, "NaN on one side")
    with pytest.raises(AssertionError):
        assert_elements(ref, got, n_e, DEFAULT_TIER, "NaN on the other side")
    assert_elements(got, got.copy(), n_e, DEFAULT_TIER, "NaN on both sides")
    inf = ref.copy()
    inf[4] = np.inf
    assert_elements(inf, inf.copy(), n_e, DEFAULT_TIER, "inf on both sides")
    with pytest.raises(AssertionError):
        assert_elements(inf, ref, n_e, DEFAULT_TIER, "inf on one side")
    # a subnormal element one unit off: a relative difference of 1/7, accepted through the absolute term n_e 2^-1022,
    # as is an underflow to zero of an element that rays are deposited into
    got = ref.copy()
    got[3] = 5e-324 * 8
    got[5] = 5e-324
    fig = assert_elements(got, ref, n_e, TIGHT_TIER, "subnormal, one unit off")
    assert fig["count"] == ref.size and fig["worst"] == 0.0
    # a negative reference is not an input of this gate
    with pytest.raises(AssertionError, match="negative"):
        assert_elements(ref, -ref, n_e, DEFAULT_TIER, "negative reference")
    # per-pixel counts are spread over the K elements of the pixel
    img = np.arange(12.0)
    with pytest.raises(AssertionError, match=r"\(iy 1, ix 0, k 1\)"):
        assert_elements(np.where(np.arange(12) == 7, 7.1, img), img, np.array([1, 1, 1, 1]), 1e-3, "named element", (2, 2, 3))
