"""The populations of tests/test_gpu_march_cell.py, judged on the host: what they reach, what they would catch, and the
records they are gathered from.

  reach     counted from the oracle's outputs (rt_oracle_cell_setup): each escape condition, the first and the last interval of
            either axis, positions exactly on a node, negative py on a mirrored grid, the clamp of E0, the cell step without a
            cross-cell iteration; and, from the float32 restatement of guess_interval, guesses that miss by one cell and by many
  mutants   each named mutant of the restated device rule (march_cell_inputs.restate) changes at least 20 outputs of the
            population -- but `sz * sz < 0.01f` in place of `<=`: no float has 0.01f for its rounded square (the squares of the
            two floats around sqrt(0.01f) are its two neighbours, and the rounded square is monotone), so the two forms are the
            same function of a float sz.  That mutant is asserted to change nothing, with the reason
  records   rh, rw, w, b_lo, b_hi and the mirrored first b_lo of every interval of every test grid, as the product's packing
            function lays them into the blob, equal the oracle's own expressions bit for bit; headers and nodes are the inputs
"""
import numpy as np
import pytest

import march_cell_inputs as mc

F, D = np.float32, np.float64


def u(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def census():
    """per group: the oracle's outputs and the unmutated restatement"""
    return [(g, mc.reference(g.name), mc.restate(g)) for g in mc.groups()]


def test_the_restatement_agrees_with_the_oracle(census):
    """what the restated rule decides equals what the oracle decides, on every case: the mutants below are mutants of the
    right rule"""
    total = 0
    for g, ora, r in census:
        for key in ("escaped", "k1", "k2", "enters"):
            bad = np.flatnonzero(np.asarray(ora[key]) != r[key])
            assert not len(bad), f"{g.name}: {key} differs in {len(bad)} cases, first {bad[0]}: pos {g.pos[bad[0]].tolist()}"
        e = np.flatnonzero((u(ora["E0"]) != u(r["E0"])) & ~(np.isnan(ora["E0"]) & np.isnan(r["E0"])))
        assert not len(e), f"{g.name}: E0 differs in {len(e)} cases"
        total += len(g.ii)
    assert 200_000 <= total <= 900_000, total


def test_what_the_populations_reach(census):
    c = dict(cases=0, esc_x_lo=0, esc_x_hi=0, esc_y_lo=0, esc_y_hi=0, esc_sz=0, k1_first=0, k1_last=0, k2_first=0, k2_last=0,
             tie_x=0, tie_y=0, mirrored_negative_py=0, below_first_node_mirrored=0, clamp=0, minus_zero_E0=0, no_cross_cell=0,
             miss_by_one=0, miss_by_many=0, regather=0, sz2_below=0, sz2_above=0, nan_px=0)
    for g, ora, r in census:
        live = ~ora["escaped"]
        c["cases"] += len(live)
        for k, name in enumerate(("esc_x_lo", "esc_x_hi", "esc_y_lo", "esc_y_hi", "esc_sz")):
            c[name] += int((r["why"][:, k] & ora["escaped"]).sum())
        c["nan_px"] += int(np.isnan(g.pos[:, 0]).sum())
        s2 = (g.pos[:, 2] * g.pos[:, 2]).astype(F)
        c["sz2_below"] += int((s2 == np.nextafter(F(0.01), F(0))).sum())
        c["sz2_above"] += int((s2 == np.nextafter(F(0.01), F(1))).sum())
        for i in range(1, g.N):
            t = g.tables[i]
            m = live & (g.ii == i)
            k1, k2 = ora["k1"][m], ora["k2"][m]
            c["k1_first"] += int((k1 == 1).sum())
            c["k1_last"] += int((k1 == t.Nx - 1).sum())
            c["k2_first"] += int((k2 == 1).sum())
            c["k2_last"] += int((k2 == t.Ny - 1).sum())
            c["tie_x"] += int(np.isin(g.pos[m, 0].astype(D), t.x).sum())
            c["tie_y"] += int(np.isin(r["ya"][m].astype(D), t.y).sum())
            if t.y[0] >= 0:
                c["mirrored_negative_py"] += int((g.pos[m, 1] < 0).sum())
                c["below_first_node_mirrored"] += int((r["ya"][m].astype(D) < t.y[0]).sum())
            d1, d2 = np.abs(r["guess1"][m] - k1), np.abs(r["guess2"][m] - k2)
            c["miss_by_one"] += int(((d1 == 1) | (d2 == 1)).sum())
            c["miss_by_many"] += int(((d1 > 3) | (d2 > 3)).sum())
        c["regather"] += int(r["regather"].sum())
        c["no_cross_cell"] += int((live & ~ora["enters"]).sum())
        if g.use_emis:
            raw = mc.restate(g, "E0_unclamped")["E0"]
            c["clamp"] += int((live & ~(raw >= 0)).sum())
            c["minus_zero_E0"] += int((live & (u(ora["E0"]) == 0x80000000)).sum())
    print("march cell populations reach:", ", ".join(f"{k} {v}" for k, v in c.items()))
    for k, v in c.items():
        assert v >= 20, f"the populations reach {k} in {v} cases only"


@pytest.mark.parametrize("mutant", [m for m in mc.MUTANTS if m != "sz2_lt"])
def test_every_mutant_of_the_device_rule_is_caught(census, mutant):
    n = sum(int(mc.changed(r, mc.restate(g, mutant)).sum()) for g, _, r in census)
    print(f"mutant {mutant}: {n} cases change")
    assert n >= 20, f"mutant {mutant} changes {n} cases only: the populations are too thin there"


def test_the_strict_escape_test_on_sz_is_the_same_function():
    """`sz * sz < 0.01f` against `<=`: they differ only where the rounded square IS 0.01f, and no float squares to it -- the
    floats on either side of sqrt(0.01f) square to the float below and the float above 0.01f, and the rounded square of a
    positive float is monotone.  So this mutant cannot change an output, whatever the population (it changes none here); the
    populations stand on both neighbours instead (sz2_below, sz2_above of the census)."""
    t = F(0.01)
    s = F(np.sqrt(t))
    below, above = np.nextafter(s, F(0)), s
    assert F(below * below) == np.nextafter(t, F(0)) and F(above * above) == np.nextafter(t, F(1))
    assert np.nextafter(below, F(1)) == above  # neighbours: no float between them
    for g in mc.groups():
        assert not mc.changed(mc.restate(g), mc.restate(g, "sz2_lt")).any()


def test_packed_records_are_the_oracles_expressions():
    """every interval of every test grid: rh = 1 / (hi - lo) (the divisor of u and v, Helper.h:482-483), w = (float) (hi - lo)
    and rw = 1 / (double) w (the divisor of cross_cell), b_lo / b_hi the cell box of rt_oracle.c with its 10 % margin, and -b_hi
    for the first interval of a mirrored y axis"""
    n_iv = 0
    for g in mc.groups():
        blob = mc.packed_blob(g)
        hdr = np.frombuffer(blob, mc.BLOB_GAIN, count=g.N)
        for i in range(1, g.N):
            t, h = g.tables[i], hdr[i]
            with np.errstate(over="ignore"):
                lo_y = F(t.y[0])
                mirror = bool(lo_y >= 0)
                want = (F(t.x[0]), F(t.x[-1]), -F(t.y[-1]) if mirror else lo_y, F(t.y[-1]), t.Nx, t.Ny, int(mirror))
            got = (h["lo_x"], h["hi_x"], h["lo_y"], h["hi_y"], h["Nx"], h["Ny"], h["mirror_y"])
            assert got == want, (g.name, i, got, want)
            assert u(h["inv_hxf"]) == u(mc._packed_inv(t.x)) and u(h["inv_hyf"]) == u(mc._packed_inv(t.y))
            nodes = np.frombuffer(blob, mc.NODE, count=t.Nx * t.Ny, offset=int(h["off_node"]))
            assert np.array_equal(u(nodes["n"]), u(t.n)) and np.array_equal(u(nodes["g0"]), u(t.g0))
            assert np.array_equal(u(nodes["E0"]), u(t.E0 if t.E0 is not None else np.zeros(t.Nx * t.Ny, F)))
            for gr, off, mirrored in ((t.x, h["off_ix"], False), (t.y, h["off_iy"], mirror)):
                iv = np.frombuffer(blob, mc.INTERVAL, count=len(gr), offset=int(off))[1:]
                lo, hi = gr[:-1], gr[1:]
                with np.errstate(over="ignore"):
                    hk = hi - lo
                    w = hk.astype(F)
                    b_lo, b_hi = (lo - 0.1 * (hi - lo)).astype(F), (hi + 0.1 * (hi - lo)).astype(F)
                    if mirrored:
                        b_lo[0] = -b_hi[0]
                    rw = 1.0 / w.astype(D)
                for name, a in (("lo", lo), ("hi", hi), ("rh", 1.0 / hk), ("rw", rw), ("w", w), ("b_lo", b_lo), ("b_hi", b_hi)):
                    assert np.array_equal(u(iv[name]), u(a)), f"{g.name}, length {i}: {name} of the packed intervals"
                n_iv += len(iv)
    assert n_iv > 1000
    groups = {g.name: g for g in mc.groups()}
    h = np.frombuffer(mc.packed_blob(groups["non_uniform/degenerate_guess"]), mc.BLOB_GAIN, count=2)[1]
    assert h["inv_hxf"] == 0 and h["inv_hyf"] == 0, "the degenerate-guess grid must pack a zero reciprocal spacing"
