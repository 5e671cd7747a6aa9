"""The close of a cell step without a cross-cell iteration (raytrace-miniapp_amd/csrc/rt_march_cell.inc, the `else` of the box
test at the end of block [A2]): a rare arm that the wave now branches round when no lane takes it.  Per lane, through
dm_march_cell_kernel (csrc/rt_devmath.hip, which includes the fragment as march_wave does), in the LDS and the global
instance, against rt_oracle_cell_setup bit for bit -- the judge and the layout of tests/test_gpu_march_cell.py
(march_cell_inputs.expected).  The cases are the ones the arm and its neighbourhood turn on:

  boundary   rays placed exactly on interior cell boundaries of a grid with the usual 10 % box margin (x, y, and both at
             once): the ray belongs to the interval below the node and enters a cross-cell iteration -- the arm is NOT taken;
  dzrem      sub-segments with dzrem == 0 on entry (z == z_stop), dzrem < 0 and the smallest dzrem > 0: the arm is taken for
             the first two;
  margin     a grid at 1e8 with a spacing of 8, one float ulp: the box margin vanishes in float, b_hi == the node, and a ray
             on an interior boundary fails px < b_hi -- the arm is taken;
  mixed      whole waves in which no lane, one lane, every other lane and every lane take the arm (the wave-uniform skip).

The corner values g0 and E0 are +0, -0, below zero and above in bands, so that the sums the arm forms with path = +0 --
gacc + g0 * 0, eacc + E0 * 0 -- meet every sign of zero: the accumulators start at +0 and stay +0, and an E0 that
interpolates to -0 stays -0 in the lane state (a maximum in place of the compare-and-select would make it +0).

The first test runs on the CPU: the numpy restatement of the device's rule (march_cell_inputs.restate) agrees with the
oracle on every case, and every population above is present, so the expected values of the device tests are the reference's
and they reach what they are meant to."""
import functools

import numpy as np
import pytest

import march_cell_inputs as mc

F, D = np.float32, np.float64
POOL = np.array([0.0, -0.0, -1.5, 2.0], F)


def banded_table(x, y, rng):
    """g0 in bands of two columns, E0 in bands of two rows: the four corners of a cell share a value in half the cells"""
    nx, ny = len(x), len(y)
    iy, ix = np.divmod(np.arange(nx * ny), nx)
    return mc.table(x, y, rng, g0=POOL[(ix // 2) % 4], E0=POOL[(iy // 2 + 1) % 4])


@functools.lru_cache(maxsize=None)
def groups():
    rng = np.random.default_rng(20241021)
    x, y = np.linspace(0.0, 1.0, 9), np.linspace(-0.75, 0.75, 7)
    t = banded_table(x, y, rng)
    xn, yn = x[1:-1].astype(F), y[1:-1].astype(F)           # interior nodes as floats (exact: multiples of 1/8 and 1/4)
    assert (xn.astype(D) == x[1:-1]).all() and (yn.astype(D) == y[1:-1]).all()
    px, py = mc.inside(t, 64, rng)
    on_x = mc.cases(np.tile(xn, 8), rng.choice(py, 8 * len(xn)))
    on_y = mc.cases(rng.choice(px, 8 * len(yn)), np.tile(yn, 8))
    on_both = mc.cases(np.repeat(xn, len(yn)), np.tile(yn, len(xn)))
    boundary = mc.group("boundary", [t], np.concatenate([on_x, on_y, on_both]))
    # dzrem = z_stop - z: zero, negative, the smallest positive one; on the boundary and inside
    z_stop = F(0.05)
    zs = np.array([z_stop, np.nextafter(z_stop, F(1)), F(0.06), np.nextafter(z_stop, F(0)), F(0.0)], F)
    pos = np.concatenate([on_both, mc.cases(*mc.inside(t, 100, rng))])
    dz = np.concatenate([mc.cases(pos[:, 0], pos[:, 1], z=z, z_stop=z_stop) for z in zs])
    dzrem = mc.group("dzrem", [t], dz)
    # one float ulp per interval at 1e8: (float) (hi + 0.1 * 8) == (float) hi
    xw = 1e8 + 8.0 * np.arange(12)
    tw = banded_table(xw, y, rng)
    xwn = xw[1:-1].astype(F)
    assert (xwn.astype(D) == xw[1:-1]).all()
    margin = mc.group("margin", [tw], mc.cases(np.tile(xwn, 7), rng.choice(py, 7 * len(xwn))))
    # whole waves of 64 lanes: none, one, every other, all take the arm (z == z_stop takes it, z = 0 does not)
    wx, wy = mc.inside(t, 4 * 64, rng)
    lane = np.arange(4 * 64) % 64
    wave = np.arange(4 * 64) // 64
    takes = ((wave == 1) & (lane == 37)) | ((wave == 2) & (lane % 2 == 0)) | (wave == 3)
    mixed = mc.group("mixed", [t], mc.cases(wx, wy, z=np.where(takes, z_stop, F(0.0)), z_stop=z_stop))
    return {g.name: g for g in (boundary, dzrem, margin, mixed)}, takes


@functools.lru_cache(maxsize=None)
def reference(name):
    """rt_oracle_cell_setup on a group, once"""
    g = groups()[0][name]
    return mc._oracle().cell_setup(g.rtgain(), g.use_emis, g.pos, g.ii)


def test_the_cases_reach_the_arm_and_the_reference_says_so(oracle):
    gs, takes = groups()
    closes = {}
    for name, g in gs.items():
        ora, r = reference(name), mc.restate(g)
        live = ~ora["escaped"]
        assert live.all(), name                                              # every case is inside the plasma box
        assert np.array_equal(r["enters"], ora["enters"]) and np.array_equal(r["k1"], ora["k1"]) and np.array_equal(r["k2"], ora["k2"]), name
        assert np.array_equal(r["E0"].view(np.uint32), ora["E0"].view(np.uint32)), name
        closes[name] = ~ora["enters"]
        print(f"{name}: {len(g.ii)} cases, {int(closes[name].sum())} close without a cross-cell iteration; g0 < 0 in "
              f"{int((ora['g0'] < 0).sum())}, g0 == 0 in {int((ora['g0'] == 0).sum())}, E0 -0 in {int((ora['E0'].view(np.uint32) == 0x80000000).sum())}, "
              f"E0 clamped or +0 in {int((ora['E0'].view(np.uint32) == 0).sum())}")
    assert not closes["boundary"].any()                                      # a 10 % margin: on the boundary is inside the box
    d = closes["dzrem"].reshape(5, -1)
    assert d[0].all() and d[1].all() and d[2].all() and not d[3].any() and not d[4].any()   # dzrem == 0, < 0, < 0, > 0, > 0
    assert closes["margin"].all()                                            # the margin vanished: on the boundary is outside
    assert np.array_equal(closes["mixed"], takes)
    # the zero signs: among the cases that take the arm g0 is negative, +0 and -0, and E0 is -0 (kept) and +0
    for name in ("dzrem", "margin"):
        ora, c = reference(name), closes[name]
        g0, e0 = ora["g0"][c], ora["E0"][c].view(np.uint32)
        assert (g0 < 0).any() and (g0.view(np.uint32) == 0).any() and (g0.view(np.uint32) == 0x80000000).any(), name
        assert (e0 == 0x80000000).any() and (e0 == 0).any(), name
    # ... and the sums the arm forms are +0 for every one of them (what expected() hands the device test)
    for name in gs:
        _, fo, _ = mc.expected(gs[name], reference(name))
        assert not fo[:, 16].view(np.uint32)[closes[name]].any() and not fo[:, 17].view(np.uint32)[closes[name]].any(), name


def differs(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype.kind == "i":
        return got != want
    v = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(v) != want.view(v)) & ~(np.isnan(got) & np.isnan(want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["boundary", "dzrem", "margin", "mixed"])
@pytest.mark.parametrize("instance", ["lds", "global"])
def test_the_closed_cell_step_equals_the_oracle(hip, oracle, instance, name):
    import devmath as dm
    dev = dm.Device.get()
    g = groups()[0][name]
    ora = reference(name)
    want_i, want_f, want_d = mc.expected(g, ora)
    io, fo, do = dev.march_cell(instance == "lds", g.rtgain(), g.use_emis, g.pos, g.ii)
    want_i[:, 4] = io[:, 4]   # (the second-gather flag is the subject of tests/test_gpu_march_cell.py)
    bad = differs(io, want_i).any(axis=1) | differs(fo, want_f).any(axis=1) | differs(do, want_d).any(axis=1)
    closes = ~ora["enters"]
    print(f"cell {name} [{instance}]: {len(g.ii)} cases, {int(closes.sum())} close without a cross-cell iteration, {int(bad.sum())} differ from the oracle")
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        cols = [f"{n} {a!r} != {b!r}" for names, got, want in ((mc.I_NAMES, io, want_i), (mc.F_NAMES, fo, want_f), (mc.D_NAMES, do, want_d))
                for n, a, b, d_ in zip(names, got[i].tolist(), want[i].tolist(), differs(got[i], want[i])) if d_]
        pytest.fail(f"{int(bad.sum())} of {len(g.ii)} cases; first: case {i}, pos {[float(v).hex() for v in g.pos[i]]}: " + "; ".join(cols))
    # the closed step itself, spelled out: steps and cell_last move, z stays, the sums stay +0
    assert np.array_equal(io[closes, 5], np.ones(int(closes.sum()), np.int32)) and np.array_equal(io[closes, 6], ora["c00"][closes])
    assert not io[~closes, 5].any()
    assert np.array_equal(fo[closes, 15].view(np.uint32), g.pos[closes, 3].view(np.uint32))
    assert not fo[closes, 16].view(np.uint32).any() and not fo[closes, 17].view(np.uint32).any()
