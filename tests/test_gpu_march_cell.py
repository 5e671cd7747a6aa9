"""Block [A2] of the march -- the escape test and the cell set-up, csrc/rt_march_cell.inc -- on a device, against the oracle.

dm_march_cell_kernel (csrc/rt_devmath.hip) includes the fragment exactly as march_wave does and runs one case per lane in
whole waves, in both table instances: `lds` copies the blob to LDS address 0 and gathers with the product's ds_read_b128
sequence straight into the lane-state registers, `global` reads the blob where it lies.  The blob is packed by the function
rt_hip_plan_create packs with (csrc/rt_blob_pack.h).  The yardstick is rt_oracle_cell_setup, the head of the loop body of the
oracle's march (the same static inline function the march calls, so tests/test_oracle_pin.py pins it to the reference):

  every output -- escaped, the new state, c00, mirror, g0, E0, dzrem, the two interval records as the lane keeps them, the four
  corner indices as floats and their four differences, and where the cell step closes without a cross-cell iteration z, gacc,
  eacc, steps, cell_last -- equals the oracle bit for bit (a NaN equals a NaN); an escaping lane leaves its state alone;
  the second-gather flag equals "the restated float guess is not the oracle's interval" on every case.

tests/march_cell_inputs.py builds the populations, tests/test_march_cell_host.py says what they reach.  Every test prints its
census; with DEVMATH_PARITY_FILE set it is appended to that file (profiles/march_cell_parity.txt is such a run on an MI355X).
No case is excepted."""
import numpy as np
import pytest

import devmath as dm
import march_cell_inputs as mc

pytestmark = pytest.mark.gpu
FAMILIES = tuple(dict.fromkeys(g.name.split("/")[0] for g in mc.groups()))


@pytest.fixture(scope="module")
def dev(hip):
    return dm.Device.get()


def differs(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype.kind == "i":
        return got != want
    v = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(v) != want.view(v)) & ~(np.isnan(got) & np.isnan(want))


def describe(g, i, names, got, want):
    cols = [f"{n} {g_!r} != {w!r}" for n, g_, w, d in zip(names, got[i].tolist(), want[i].tolist(), differs(got[i], want[i])) if d]
    return f"case {i} (length {int(g.ii[i])}, px, py, sz, z, z_stop = {[float(v).hex() for v in g.pos[i]]}): " + "; ".join(cols)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("instance", ["lds", "global"])
def test_cell_setup_equals_the_oracle(dev, instance, family):
    failures = []
    for g in (g for g in mc.groups() if g.name.split("/")[0] == family):
        ora = mc.reference(g.name)
        r = mc.restate(g)
        want_i, want_f, want_d = mc.expected(g, ora)
        want_i[:, 4] = ~ora["escaped"] & ((r["guess1"] != ora["k1"]) | (r["guess2"] != ora["k2"]))
        io, fo, do = dev.march_cell(instance == "lds", g.rtgain(), g.use_emis, g.pos, g.ii)
        bad_i, bad_f, bad_d = differs(io, want_i), differs(fo, want_f), differs(do, want_d)
        bad = bad_i.any(axis=1) | bad_f.any(axis=1) | bad_d.any(axis=1)
        live = ~ora["escaped"]
        dm.note(f"cell {g.name} [{instance}]: {len(g.ii)} cases in {g.N - 1} length(s), {int(bad.sum())} differ from the oracle; "
                f"escaped {int(ora['escaped'].sum())}, second gather {int(io[:, 4].sum())}, no cross-cell iteration "
                f"{int((live & ~ora['enters']).sum())}, clamped-or-zero E0 {int((live & (ora['E0'] == 0)).sum())}")
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            per = [f"{n} {int(b.sum())}" for names, bb in ((mc.I_NAMES, bad_i), (mc.F_NAMES, bad_f), (mc.D_NAMES, bad_d))
                   for n, b in zip(names, bb.T) if b.any()]
            failures.append(f"{g.name} [{instance}]: {int(bad.sum())} of {len(g.ii)} ({', '.join(per)}); first: "
                            + describe(g, i, mc.I_NAMES, io, want_i) + " " + describe(g, i, mc.F_NAMES, fo, want_f) + " "
                            + describe(g, i, mc.D_NAMES, do, want_d))
    assert not failures, "\n".join(failures)


def test_bad_arguments_are_refused_before_any_launch(dev):
    g = {g.name: g for g in mc.groups()}["smallest/two_lengths"]
    for ii in (np.zeros_like(g.ii), np.full_like(g.ii, g.N), np.full_like(g.ii, -1)):
        with pytest.raises(dm.DeviceMathError):
            dev.march_cell(False, g.rtgain(), g.use_emis, g.pos, ii)
    # a blob beyond the LDS a work-group may have: refused for the LDS instance, served from global memory
    rng = np.random.default_rng(3)
    t = mc.table(np.linspace(0.0, 1.0, 130), np.linspace(-1.0, 1.0, 100), rng)  # 13 000 nodes of 16 bytes
    big = mc.group("too_big_for_lds", [t], mc.cases(*mc.inside(t, 65, rng)))
    with pytest.raises(dm.DeviceMathError):
        dev.march_cell(True, big.rtgain(), True, big.pos, big.ii)
    io, _, _ = dev.march_cell(False, big.rtgain(), True, big.pos, big.ii)
    ora = mc._oracle().cell_setup(big.rtgain(), True, big.pos, big.ii)
    assert np.array_equal(io[:, 0] != 0, ora["escaped"]) and np.array_equal(io[~ora["escaped"], 2], ora["c00"][~ora["escaped"]])
    # tables that creation refuses are refused here
    bad = mc.Table(t.x.copy(), t.y.copy(), t.n.copy(), t.g0, t.E0)
    bad.n[5] = 2.0 ** 128 - 2.0 ** 103
    with pytest.raises(dm.DeviceMathError):
        dev.march_cell(False, mc.Group("bad", [None, bad], True, big.pos, big.ii).rtgain(), True, big.pos, big.ii)
