"""The choice of the emission update on the device: every regime of tests/update_regimes.py, as a ray list whose tiles hold
stated mixes of small, regular and irregular rays, through every pass that carries the choice -- spectra, image and step
as two kernels, image and step in one launch (on parts of the grid that hold every branch: a list keeps the two kernels), step with ASE
seeds, the length scan and the suffix scan with and without ASE seeds -- in the default mode and with exact emission, at
N = 3 (the tile-wide choice of rt_tile_rec.inc) and N = 5 (the per-slot choice), under both methods; and the gain-only
`need` decision on seed_small (seeded_need).  tests/test_update_regimes_host.py holds the census of every input.

Reference: the CPU oracle, which knows nothing of the choice.  Spectra mode is the sharp instrument: per ray and frequency.
    default mode, finite regimes   per-ray rel-L2 < 1e-6.  With E0 >= 0 every term of the recurrence is non-negative, so a
                                   term's relative error carries into the sum undiluted and unamplified; a term carries at
                                   most 1.2e-7 from the two float products behind rs = es / gs and at most 1.2e-7 (2^-23)
                                   from ase_step_f32: below 3e-7 together, 1e-6 leaves a factor of three
    exact mode                     per-ray rel-L2 < 1e-11 (TIGHT_TIER, what the exact-mode tests of the other passes assert)
    non-finite regimes             the NaN, +inf and -inf elements are the oracle's exactly; the finite elements of every row
                                   pass the 1e-5 gate of tests/test_gpu_spectra.py
    tile-mix invariance            the same rays sorted by class (homogeneous tiles) give the same rows: within 1e-6 in the
                                   default mode (a small ray beside a regular one takes ase_step instead of ase_step_f32),
                                   bit for bit in the exact mode
Image, step and scan passes: gate_outputs / gate_step / gate_records of the neighbouring tests with their tiers
(DEFAULT_TIER emission, TIGHT_TIER exact and gain-only), same_outputs_in_a_failing_run where the oracle's run fails, the
failure code and the reported failing rays the oracle's (as a set: the device reports in the order its waves finish).

Measured figures are printed before every assertion; with UPDATE_REGIMES_PARITY_FILE set they are appended to that file
(profiles/update_regimes_parity.txt)."""
import importlib
import os

import numpy as np
import pytest

import ase_seeds as A
import table_variants as tv
import update_regimes as ur
from element_gate import DEFAULT_TIER, TIGHT_TIER, counts_from_oracle, gate_outputs
from test_gpu_edges import same_outputs_in_a_failing_run
from test_gpu_spectra import GATE, check_against, ray2_bits_equal
from test_gpu_step import _ray_set, gate_step, reduced
import test_gpu_length_scan as LS
import test_gpu_suffix_scan as SS
import test_gpu_scan_ase_seeds as LA
import test_gpu_suffix_ase_seeds as SA

rt = importlib.import_module("raytrace-miniapp_amd")
pytestmark = pytest.mark.gpu

CASES = [(r, N, m) for r in ur.REGIMES for N in (3, 5) for m in (1, 2)]
DEFAULT_BOUND = 1e-6


def note(line):
    print(line)
    path = os.environ.get("UPDATE_REGIMES_PARITY_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def same_failed_rays(out, ora, label):
    """The failure code, and the reported rays as tests/test_gpu_edges.py compares them: the same set where the CPU reports
    fewer than RT_N_FAILED_MAX (the device reports in the order its waves finish), else as many."""
    assert out["failure_code"] == ora["failure_code"], (label, out["failure_code"], ora["failure_code"])
    got, want = _ray_set(out["failed_rays"]), _ray_set(ora["failed_rays"])
    if len(ora["failed_rays"]) < rt.cabi.RT_N_FAILED_MAX:
        assert got == want, label
    else:
        assert len(out["failed_rays"]) == rt.cabi.RT_N_FAILED_MAX, label


# ---------------------------------------------------------------------------------------------- spectra
def row_l2(got, ref):
    """Per-ray rel-L2 over the elements finite in ref (0 for a row without any non-zero finite element, which must then be
    equal)."""
    fin = np.isfinite(ref)
    r = np.where(fin, ref, 0.0)
    top = np.abs(r).max(axis=1, keepdims=True)
    scale = np.where(top > 0, top, 1.0)             # (rows near DBL_MAX: the squares of the norm must not overflow)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(fin, got / scale - r / scale, 0.0)
    r = r / scale
    num, den = np.linalg.norm(d, axis=1), np.linalg.norm(r, axis=1)
    assert not num[den == 0].any(), "a row that is zero on the CPU is not zero here"
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def same_nonfinite(got, ref, label):
    with np.errstate(invalid="ignore"):
        for what, a, b in (("NaN", np.isnan(got), np.isnan(ref)), ("+inf", got == np.inf, ref == np.inf), ("-inf", got == -np.inf, ref == -np.inf)):
            assert np.array_equal(a, b), f"{label}: the {what} elements differ: {int(a.sum())} here, {int(b.sum())} on the CPU, first at {np.argwhere(a != b)[:3].tolist()}"
    return int((~np.isfinite(ref)).sum())


def check_spectra(out, ref, label, bound, finite):
    """err ray by ray, ray2 bit for bit, the gate of tests/test_gpu_spectra.py, and the bound of this module."""
    if finite:
        check_against(out, ref, label)
    else:
        bad = np.flatnonzero(out["err"] != ref["err"])
        assert len(bad) == 0, (f"{label}: {len(bad)} return codes differ, first rays {bad[:4].tolist()}: here {out['err'][bad[:4]].tolist()}, "
                               f"CPU {ref['err'][bad[:4]].tolist()}; gs {ref['gvl'][bad[0]].tolist()}, es {ref['evl'][bad[0]].tolist()}, "
                               f"Iv here {out['Iv'][bad[0]][:8].tolist()}, CPU {ref['Iv'][bad[0]][:8].tolist()}, "
                               f"NaN here at k {np.flatnonzero(np.isnan(out['Iv'][bad[0]])).tolist()}, CPU {np.flatnonzero(np.isnan(ref['Iv'][bad[0]])).tolist()}")
        assert ray2_bits_equal(out["ray2"], ref["ray2"], ref["err"] != -1), label
        n_bad = same_nonfinite(out["Iv"], ref["Iv"], label)
        note(f"{label}: {n_bad} non-finite elements in {int((~np.isfinite(ref['Iv'])).any(axis=1).sum())} rows, as on the CPU; "
             f"return codes {dict(zip(*[v.tolist() for v in np.unique(ref['err'], return_counts=True)]))}")
    l2 = row_l2(out["Iv"], ref["Iv"])
    i = int(np.argmax(l2))
    note(f"{label}: max per-ray rel-L2 over the finite elements {l2[i]:.3e} (ray {i}), bound {bound:g}")
    assert l2[i] < bound, (label, i, float(l2[i]))
    return float(l2[i])


def run_spectra(plan, rays, exact):
    plan.set_rays(rays).set_exact_emission(exact).enable_spectra().run()
    return plan.fetch_spectra()


@pytest.mark.parametrize("regime,N,method", CASES)
def test_spectra_of_the_composed_list_and_of_the_sorted_list(hip, oracle, ase_small, regime, N, method):
    c = ur.case(oracle, ase_small, regime, N, method)
    finite = regime in ur.FINITE
    order = c.sorted_order
    ref_sorted = {k: (v[order] if isinstance(v, np.ndarray) else v) for k, v in c.probe.items()}
    with hip.Plan(c.p) as plan:
        assert plan.table_flags()["gs_cap"] == ur.gs_cap(c.p)
        runs = {(exact, which): run_spectra(plan, c.rays if which == "composed" else c.rays[order], exact)
                for exact in (False, True) for which in ("composed", "sorted")}
    for (exact, which), out in runs.items():
        bound = TIGHT_TIER if exact else (DEFAULT_BOUND if finite else GATE)
        check_spectra(out, c.probe if which == "composed" else ref_sorted, f"spectra / {c.label} / {'exact' if exact else 'default'} / {which} list",
                      bound, finite)
    # tile-mix invariance: a ray's row does not depend on its neighbours
    for exact in (False, True):
        a, b = runs[(exact, "composed")]["Iv"][order], runs[(exact, "sorted")]["Iv"]
        same_nonfinite(a, b, f"tile mix / {c.label}")
        l2 = row_l2(a, b)
        note(f"tile mix / {c.label} / {'exact' if exact else 'default'}: composed against sorted, max per-ray rel-L2 {l2.max():.3e}, "
             f"rows that differ in any bit {int((a.view(np.uint64) != b.view(np.uint64)).any(axis=1).sum())} of {len(a)}")
        if exact:
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), c.label
        else:
            assert l2.max() < DEFAULT_BOUND, (c.label, float(l2.max()))


@pytest.mark.parametrize("N,method", [(N, m) for N in (3, 5) for m in (1, 2)])
def test_cap_exact_on_a_resident_plan_the_device_side_cap_feeds_the_choice(hip, oracle, ase_small, N, method):
    """gs_cap one ulp above the chosen |gs|, equal to it and one ulp below it, applied with update_gain to ONE plan
    (rt_tables.hip derives the cap on the device); a fresh plan of the middle table gives the same bits."""
    c = ur.case(oracle, ase_small, "cap_exact", N, method)
    outs = []
    with hip.Plan(c.tables[0]) as plan:
        for i, q in enumerate(c.tables):
            if i:
                plan.update_gain(tv.as_tables(q))
            cap = plan.table_flags()["gs_cap"]
            assert cap == ur.gs_cap(q), (i, cap)
            out = run_spectra(plan, c.rays, False)
            check_spectra(out, c.probe, f"cap_exact / {c.label} / gs_cap {float(cap)!r} against |gs| {c.chosen[2]!r}", DEFAULT_BOUND, True)
            outs.append(out)
    with hip.Plan(c.tables[1]) as plan:
        assert plan.table_flags()["gs_cap"] == np.float32(c.chosen[2])
        fresh = run_spectra(plan, c.rays, False)
    assert np.array_equal(fresh["Iv"].view(np.uint64), outs[1]["Iv"].view(np.uint64)) and np.array_equal(fresh["err"], outs[1]["err"])
    pos = c.chosen[0]
    bits = [o["Iv"].view(np.uint64) for o in outs]
    note(f"cap_exact / {c.label}: the chosen ray's row, cap above / equal / below: rel-L2 against equal "
         f"{[float(row_l2(o['Iv'][pos:pos + 1], outs[1]['Iv'][pos:pos + 1])[0]) for o in outs]}; rows of the list that differ in "
         f"any bit from equal: above {int((bits[0] != bits[1]).any(axis=1).sum())}, below {int((bits[2] != bits[1]).any(axis=1).sum())}")
    # `<=`: with the cap ON |gs| the slot is regular as with the cap one ulp above -- the whole list, bit for bit; one ulp
    # below, the chosen slot takes ase_update and (N = 3) its tile the per-slot branch: another rounding of the same row
    assert np.array_equal(bits[0], bits[1]), c.label
    assert not np.array_equal(bits[2][pos], bits[1][pos]), c.label


# ---------------------------------------------------------------------------------------------- image and step
def gate_image(out, ora, p, counts, tier, label):
    note(f"{label}: failure_code {out['failure_code']} (oracle {ora['failure_code']}), failed rays {len(out['failed_rays'])}")
    same_failed_rays(out, ora, label)
    if ora["failure_code"]:
        same_outputs_in_a_failing_run(out, ora)
    else:
        figs = gate_outputs(out, ora, p, counts, tier, label)
        note(f"{label}: worst element image {figs['image']['worst']:.3e}, I_ang {figs['I_ang']['worst']:.3e}, tier {tier:g}")


def gate_step_record(hip, step, ora, p, counts, tier, label):
    ref = reduced(hip, p, ora)
    if ora["failure_code"]:
        same_outputs_in_a_failing_run(dict(image=step["nf"], I_ang=step["I_ang"]), dict(image=ref["nf"], I_ang=ref["I_ang"]))
        same_outputs_in_a_failing_run(dict(image=step["E_v"], I_ang=step["I_ang"]), dict(image=ref["E_v"], I_ang=ref["I_ang"]))
    else:
        figs = gate_step(step, ref, p, counts, tier, label)
        note(f"{label}: worst element nf {figs['nf']['worst']:.3e}, E_v {figs['E_v']['worst']:.3e}, I_ang {figs['I_ang']['worst']:.3e}, tier {tier:g}")


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("regime,N,method", CASES)
def test_image_and_step_as_two_kernels_in_one_launch_and_with_ase_seeds(hip, oracle, ase_small, regime, N, method, exact, monkeypatch):
    c = ur.case(oracle, ase_small, regime, N, method)
    p = c.p
    tier = TIGHT_TIER if exact else DEFAULT_TIER
    mode = "exact" if exact else "default"
    # the composed list: two kernels
    ora = oracle.image_loop(p, c.rays)
    counts = counts_from_oracle(oracle, p, c.rays)
    monkeypatch.setenv("RT_HIP_FUSED", "2")
    with hip.Plan(p) as plan:
        plan.set_rays(c.rays).set_exact_emission(exact)
        img = plan.run().fetch()
        assert not plan.last_fused() and img["stats"]["cell_steps"] == ora["counters"]["cell_steps"]
        gate_image(img, ora, p, counts, tier, f"image, two kernels / {c.label} / {mode}")
        plan.enable_step().run()
        step, info = plan.fetch_step(), plan.fetch()
        assert not plan.last_fused()
        same_failed_rays(info, ora, f"step, two kernels / {c.label} / {mode}")
        gate_step_record(hip, step, ora, p, counts, tier, f"step, two kernels / {c.label} / {mode}")
        # step with ASE seeds: record 0 is the emission record, the seeds' records are gain-only on the same march
        seeds = list(A.seeds_of(p))
        plan.set_ase_seeds(seeds, [A.carry(p, s).scale for s in seeds]).run()
        full, info = plan.fetch_full_step(), plan.fetch()
        assert len(full["seeds"]) == 2 and full["ase"]["failure_code"] == ora["failure_code"]
        gate_step_record(hip, full["ase"], ora, p, counts, tier, f"step with ASE seeds, ASE record / {c.label} / {mode}")
        for s, seed in enumerate(seeds):
            q = A.carry(p, seed)
            oq = oracle.image_loop(q, c.rays)
            assert full["seeds"][s]["failure_code"] == oq["failure_code"], (c.label, s)
            gate_step_record(hip, full["seeds"][s], oq, q, counts_from_oracle(oracle, q, c.rays), TIGHT_TIER,
                             f"step with ASE seeds, seed {s} / {c.label} / {mode}")
    monkeypatch.delenv("RT_HIP_FUSED")
    # parts of the grid, each inside one pixel, that hold tiles of the small, the regular and the mixed branch
    # (update_regimes.grid_slices; the census asserts the branches): one launch where the tables leave room for the
    # frequency pass (N = 3), image and step
    if method != 1:
        return          # (the one launch is the backward method's: tests/test_gpu_method_pairs.py)
    monkeypatch.setenv("RT_HIP_FUSED", "1")
    for first, count in c.slices:
        rays = p.build_rays(first + np.arange(count, dtype=np.int64))
        ora = oracle.image_loop(p, rays)
        counts = counts_from_oracle(oracle, p, rays)
        what = f"rays {first} .. {first + count - 1} / {c.label} / {mode}"
        with hip.Plan(p) as plan:
            plan.set_ray_grid(first=first, stride=1, count=count).set_exact_emission(exact)
            img = plan.run().fetch()
            assert plan.last_fused() == (N == 3), c.label
            assert img["stats"]["n_rays"] == count and img["stats"]["cell_steps"] == ora["counters"]["cell_steps"]
            gate_image(img, ora, p, counts, tier, f"image, one launch ({plan.last_fused()}) / {what}")
            plan.enable_step().set_step_one_launch(True).run()
            step, info = plan.fetch_step(), plan.fetch()
            assert plan.last_fused() == (N == 3), c.label
            same_failed_rays(info, ora, f"step, one launch / {what}")
            gate_step_record(hip, step, ora, p, counts, tier, f"step, one launch ({plan.last_fused()}) / {what}")


# ---------------------------------------------------------------------------------------------- scans
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("regime,N,method", CASES)
def test_scans_with_and_without_ase_seeds(hip, oracle, ase_small, regime, N, method, exact):
    """Method 2: the length scan (forward march, rt_step_scan.hip and rt_step_scan_ase_seeds.hip); method 1: the suffix scan
    (backward march, rt_step_rscan.hip and rt_step_rscan_ase_seeds.hip).  Every record against the oracle on its prefix or
    suffix problem."""
    c = ur.case(oracle, ase_small, regime, N, method)
    p = c.p
    kind = "emission_exact" if exact else "emission"
    T, TA = (LS, LA) if method == 2 else (SS, SA)
    key = ("update_regimes", regime, N, method)
    label = f"{'length' if method == 2 else 'suffix'} scan / {c.label} / {'exact' if exact else 'default'}"
    with hip.Plan(p) as plan:
        recs, info = T.run_scan(plan, c.rays, exact=exact)
        assert plan.last_fused() is False and plan.last_march_instance() & (8 << 1)
    T.gate_records(hip, oracle, p, c.rays, recs, info, kind, label, key, False)
    seeds = list(A.seeds_of(p))
    with hip.Plan(p) as plan:
        full, info = TA.run_full_scan(plan, p, seeds, c.rays, exact=exact)
        assert plan.last_fused() is False and plan.last_march_instance() & (8 << 1)
    TA.gate_all(hip, oracle, p, seeds, c.rays, full, info, label + " with ASE seeds", key=key,
                tier0=TIGHT_TIER if exact else DEFAULT_TIER, exact=exact, plans=False)
    note(f"{label}: {len(recs)} records and {len(TA.curves_of(full))} x {len(recs)} with ASE seeds pass gate_records / gate_all, "
         f"failure codes {[r['failure_code'] for r in recs]}")


# ---------------------------------------------------------------------------------------------- gain only: `need`
@pytest.mark.parametrize("method", [1, 2])
def test_seeded_need_through_spectra_image_step_and_the_scan(hip, oracle, seed_small, method, monkeypatch):
    c = ur.seeded_case(oracle, seed_small, method)
    p = c.p
    ora = oracle.image_loop(p, c.rays)
    counts = counts_from_oracle(oracle, p, c.rays)
    assert ora["failure_code"] & (1 << 3)
    with hip.Plan(p) as plan:
        out = plan.set_rays(c.rays).enable_spectra().run().fetch_spectra()
        assert plan.last_fused() is False and not plan.last_march_instance() & (8 << 1)     # the plain march, then rt_spec_kernel
        check_spectra(out, c.probe, f"spectra / {c.label}", TIGHT_TIER, False)
        for name, first, n in c.tiles:
            got, ref = out["Iv"][first:first + n], c.probe["Iv"][first:first + n]
            note(f"   {c.label} / tile '{name}': NaN elements {int(np.isnan(got).sum())} (CPU {int(np.isnan(ref).sum())}), "
                 f"inf {int(np.isinf(got).sum())} (CPU {int(np.isinf(ref).sum())}), non-zero rows {int(got.any(axis=1).sum())}")
        img = plan.enable_spectra(False).run().fetch()
        assert plan.last_fused() is False           # a seeded run keeps the two kernels
        gate_image(img, ora, p, counts, TIGHT_TIER, f"image / {c.label}")
        plan.enable_step().run()
        step, info = plan.fetch_step(), plan.fetch()
        assert plan.last_fused() is False and info["image"] is None
        same_failed_rays(info, ora, f"step / {c.label}")
        gate_step_record(hip, step, ora, p, counts, TIGHT_TIER, f"step / {c.label}")
    T = LS if method == 2 else SS
    with hip.Plan(p) as plan:
        recs, info = T.run_scan(plan, c.rays)
        assert plan.last_fused() is False and plan.last_march_instance() & (8 << 1)         # the scan instance of the march
    T.gate_records(hip, oracle, p, c.rays, recs, info, "seeded", f"{'length' if method == 2 else 'suffix'} scan / {c.label}",
                   ("update_regimes", "seeded_need", method), False)
