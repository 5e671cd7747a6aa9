"""Blocks [A2], [B] and [C] of the march on a device where a zero can carry a sign or a quotient is exactly 0 or 1 --
the populations behind two shortenings of csrc/rt_math.h:

  div_by_recip_pos0   the cell coordinates u, v of [A2] and, in the BOUNDED instances, u, v and the four gradient quotients
                      of [B] go without the sign copy of a zero quotient (csrc/rt_march_cell.inc and rt_march_xsetup.inc
                      argue why it cannot show; [B] is run here in both forms)
  step_factors        1 - ht/3 + ht^2/12 and 1 - ht/2 + ht^2/6 of [C] in nine instructions
                      (tests/test_step_factor_identities.py compares the sequences on every float; here they run in the step)

The kernels are the unit kernels of csrc/rt_devmath.hip, which include the product's fragments as march_wave does:
dm_march_cell_kernel in both table instances, dm_march_xsetup_kernel in both of its, dm_march_step_kernel in its four.  The
yardsticks are rt_oracle_cell_setup, rt_oracle_cross_setup and rt_oracle_linear_step; EVERY output is compared bit for bit
(a NaN equals a NaN), no case is excepted.

What the populations aim at (tests/test_gpu_march_cell.py and test_gpu_march_blocks.py hold the broad ones):
  positions exactly on the lower corner (zero dividend; px = -0 over a grid that starts at +0: the one -0 dividend) and exactly
  on the upper corner (u = 1, v = 1: the factor 1 - v is +0) with corner differences of both signs and of zero in every
  combination, all four corners equal, tables of zeros; mirrored cells entered at py < 0 with a zero y gradient (gyn = -0);
  sx or sy a zero of either sign with gradients that are zeros of either sign, beside a steep gradient of the other axis
  (t of both signs); widths that are a power of two, inexact in 0.1f * w, and 1e-12, the smallest the plan admits;
  ht = h * t from +0 and the subnormals by decades up to 0.05 and the floats around it (t = -0 is not reachable: a0 is
  x + 1e-12f).
Every population is arranged in waves: all 64 lanes special, half of them, one of them, and a ragged last wave."""
import functools

import numpy as np
import pytest

import devmath as dm
import march_block_inputs as mi
import march_cell_inputs as mc
from oracle.binding import Oracle

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
OUT_NAMES = ("n", "rx", "ry", "rz", "sx", "sy", "sz", "hsum")
NO_NTEST = ("prune", "prune_h24")
WIDTHS = (F(2.0 ** -6), F(0.3), F(1e-3), F(1e-12), F(1e3))   # a power of two; 0.1f * w inexact; the smallest; the largest


@pytest.fixture(scope="module")
def dev(hip):
    return dm.Device.get()


@functools.lru_cache(maxsize=None)
def oracle():
    return Oracle()


def differs(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype.kind in "iub":
        return got != want
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want))


def in_waves(special, plain, rng):
    """row indices (is_special, index) arranged in waves of 64: every special case in a wave of specials alone and in a wave
    whose even lanes are special, sixteen waves with a single special lane, and a ragged wave of 37 -> the rows"""
    ns, npl = len(special), len(plain)
    lanes = np.arange(64)
    rows = []
    order = rng.permutation(ns)
    for k in range(0, ns, 64):                                  # all lanes
        rows.append(special[np.resize(order[k:k + 64], 64)])
    for k in range(0, ns, 32):                                  # half of the lanes
        w = plain[rng.integers(0, npl, 64)].copy()
        w[lanes % 2 == 0] = special[np.resize(order[k:k + 32], 32)]
        rows.append(w)
    for k in range(16):                                         # one lane
        w = plain[rng.integers(0, npl, 64)].copy()
        w[(7 * k + 3) % 64] = special[order[k % ns]]
        rows.append(w)
    w = plain[rng.integers(0, npl, 37)].copy()                  # the ragged wave
    w[::3] = special[order[:13]] if ns >= 13 else special[np.resize(order, 13)]
    rows.append(w)
    return np.concatenate(rows)


# ------------------------------------------------------------------------------------------------ [A2] the cell set-up
@functools.lru_cache(maxsize=None)
def cell_groups():
    rng = np.random.default_rng(77001)
    k9 = np.arange(9)
    grids = {
        "two_sided":     (k9 / 64.0, (k9 - 4) / 64.0),
        "mirrored":      (k9 / 64.0, np.arange(7) / 64.0),
        "inexact":       (np.concatenate([[0.0], np.cumsum(D(F(0.3)) * (1 + np.arange(7)))]), np.concatenate([[0.0], np.cumsum(D(F(1e-3)) * (1 + np.arange(5)))])),
        "smallest":      (D(F(1e-12)) * np.array([0, 1, 2, 4, 8, 16.0]), D(F(1e-12)) * np.array([0, 1, 2, 4, 8.0])),
    }
    out = []
    for name, (x, y) in grids.items():
        cells = len(x) * len(y)
        for kind in ("random", "equal_corners"):
            if kind == "random":
                t = mc.table(x, y, rng)
            else:   # one index everywhere, gain and emission tables of zeros: a zero u or v is all that is left of a term
                t = mc.table(x, y, rng, n=np.full(cells, 1.0 - 2.0 ** -12), g0=np.zeros(cells, F), E0=np.zeros(cells, F))
            xs = np.concatenate([x.astype(F), [F(-0.0)]])                       # every node: lower corner (first) or upper; px = -0
            ys = np.concatenate([y.astype(F), -y.astype(F)])                    # (-0 included where y[0] = 0)
            on = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
            special = mc.cases(on[:, 0], on[:, 1])
            plain = mc.cases(*mc.inside(t, 512, rng))
            out.append(mc.group(f"zero_signs/{name}/{kind}", [t], in_waves(special, plain, rng)))
    return tuple(out)


@pytest.mark.parametrize("instance", ["lds", "global"])
def test_cell_setup_on_the_corners(dev, instance):
    failures = []
    for g in cell_groups():
        ora = mc._oracle().cell_setup(g.rtgain(), g.use_emis, g.pos, g.ii)
        r = mc.restate(g)
        want_i, want_f, want_d = mc.expected(g, ora)
        want_i[:, 4] = ~ora["escaped"] & ((r["guess1"] != ora["k1"]) | (r["guess2"] != ora["k2"]))
        io, fo, do = dev.march_cell(instance == "lds", g.rtgain(), g.use_emis, g.pos, g.ii)
        bad = differs(io, want_i).any(axis=1) | differs(fo, want_f).any(axis=1) | differs(do, want_d).any(axis=1)
        live = ~ora["escaped"]
        t = g.tables[1]
        ya = np.abs(g.pos[:, 1]) if ora["mirror"].any() else g.pos[:, 1]
        lower = live & ((g.pos[:, 0].astype(D) == ora["cell"][:, 0]) | (ya.astype(D) == ora["cell"][:, 2]))
        upper = live & ((g.pos[:, 0].astype(D) == ora["cell"][:, 1]) | (ya.astype(D) == ora["cell"][:, 3]))
        neg0 = live & (g.pos[:, 0] == 0) & np.signbit(g.pos[:, 0]) & (t.x[0] == 0)
        dm.note(f"cell {g.name} [{instance}]: {len(g.ii)} cases, {int(bad.sum())} differ from the oracle; live {int(live.sum())}, on a lower "
                f"corner {int(lower.sum())}, on an upper corner {int(upper.sum())}, px = -0 over x[0] = +0 {int(neg0.sum())}, zero g0 {int((live & (ora['g0'] == 0)).sum())}")
        assert lower.sum() >= 64 and upper.sum() >= 64 and neg0.sum() >= 8
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            failures.append(f"{g.name} [{instance}]: {int(bad.sum())} of {len(g.ii)}; first: case {i}, pos {[float(v).hex() for v in g.pos[i]]}: "
                            f"int {io[i].tolist()} / {want_i[i].tolist()}, float {[float(v).hex() for v in fo[i]]} / {[float(v).hex() for v in want_f[i]]}, "
                            f"double {[float(v).hex() for v in do[i]]} / {[float(v).hex() for v in want_d[i]]}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ [B] the cross-cell set-up
@functools.lru_cache(maxsize=None)
def setup_cases():
    """(pos, cell, nc, mirror, is_special): cells [lo, lo + w] with lo in {0, w} -- both corners exact floats --, positions on
    the lower corner, on -0 over lo = +0, on the upper corner, in the 10 % margin on either side; corners b + d {-1, 0, 1}^4:
    every sign pattern of the four edge differences, zero included, and all four equal"""
    rng = np.random.default_rng(77002)
    KINDS = ("lower", "neg0", "upper", "above", "below", "random")

    def axis(kind, w, j, n):
        lo = j * D(w)
        hi = lo + D(w)
        p = {"lower": lo, "neg0": np.where(j == 0, -0.0, lo), "upper": hi, "above": lo + 1.0625 * D(w), "below": lo - 0.0625 * D(w),
             "random": lo + rng.uniform(-0.1, 1.1, n) * D(w)}[kind]
        return p.astype(F), lo, hi

    combos = np.stack(np.meshgrid(*([np.array([-1.0, 0.0, 1.0])] * 4)), -1).reshape(-1, 4)       # 81
    parts = []
    for special in (True, False):
        n = 81 * 30 if special else 2048
        ku = rng.integers(0, 5, n) if special else np.full(n, 5)
        kv = rng.integers(0, 5, n) if special else np.full(n, 5)
        w = np.stack([rng.choice(np.array(WIDTHS), n), rng.choice(np.array(WIDTHS), n)], axis=1)
        j = rng.integers(0, 2, (n, 2))
        mirror = rng.random(n) < 0.5
        pos, cell = np.zeros((n, 2), F), np.zeros((n, 4), D)
        for a, kk in ((0, ku), (1, kv)):
            for k, kind in enumerate(KINDS):
                sel = kk == k
                p, lo, hi = axis(kind, w[:, a], j[:, a], n)
                pos[sel, a], cell[sel, 2 * a], cell[sel, 2 * a + 1] = p[sel], lo[sel], hi[sel]
        neg = mirror & (rng.random(n) < 0.6)                                      # the ray below the axis of a mirrored cell
        pos[:, 1] = np.where(neg, -pos[:, 1], pos[:, 1])
        d = 2.0 ** -rng.integers(3, 30, n).astype(D)
        base = rng.choice(np.array([0.5, 1.0, 1.0 - 2.0 ** -12, 2.5]), n)
        nc = base[:, None] + d[:, None] * (np.resize(combos, (n, 4)) if special else rng.integers(-1, 2, (n, 4)))
        parts.append((pos, cell, nc, mirror.astype(np.uint8)))
    rows = in_waves(np.arange(len(parts[0][0])), -1 - np.arange(len(parts[1][0])), rng)
    pick = lambda k: np.where((rows >= 0)[(...,) + (None,) * (parts[0][k].ndim - 1)], parts[0][k][np.maximum(rows, 0)], parts[1][k][np.maximum(-1 - rows, 0)])
    return pick(0).astype(F), pick(1), pick(2), pick(3).astype(np.uint8), rows >= 0


def xsetup_bounded(dev, pos, lo, w, rw, nc, mirror):
    """Device.march_xsetup through rt_devmath_march_xsetup_bounded: block [B] as the BOUNDED instances of the march compile it"""
    import ctypes
    PF, PD, PB = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_double, ctypes.c_ubyte))
    fn = dev.lib.rt_devmath_march_xsetup_bounded
    fn.restype, fn.argtypes = ctypes.c_int, [PF, PD, PB, PF, ctypes.c_size_t]
    n = len(pos)
    fin = np.ascontiguousarray(np.concatenate([pos, w], axis=1), F)
    din = np.ascontiguousarray(np.stack([lo[:, 0], rw[:, 0], lo[:, 1], rw[:, 1], nc[:, 0], nc[:, 1], nc[:, 2], nc[:, 3]], axis=1), D)
    mirror = np.ascontiguousarray(mirror, np.uint8)
    out = np.empty((n, 3), F)
    dev._check(fn(fin.ctypes.data_as(PF), din.ctypes.data_as(PD), mirror.ctypes.data_as(PB), out.ctypes.data_as(PF), n), "rt_devmath_march_xsetup_bounded")
    return out


@pytest.mark.parametrize("instance", ["bounded", "generic"])
def test_cross_setup_on_the_corners(dev, instance):
    pos, cell, nc, mirror, special = setup_cases()
    # (inside the ranges of the BOUNDED instances, csrc/rt_plan.hip: indices in [0.25, 4], dn / w <= 1e12, w >= 1e-12)
    assert nc.min() >= 0.25 and nc.max() <= 4.0 and (np.abs(np.diff(nc[:, [0, 1, 3, 2, 0]], axis=1)).max(axis=1) / (cell[:, 1::2] - cell[:, ::2]).min(axis=1)).max() <= 1e12
    want = oracle().cross_setup(pos, cell, nc, mirror)
    lo, w, rw = mi.interval_records(cell)
    got = xsetup_bounded(dev, pos, lo, w, rw, nc, mirror) if instance == "bounded" else dev.march_xsetup(pos, lo, w, rw, nc, mirror)
    bad = differs(got, want)
    ya = np.where(mirror != 0, np.abs(pos[:, 1]), pos[:, 1])
    u = (pos[:, 0].astype(D) - cell[:, 0]) / D(1) / (cell[:, 1] - cell[:, 0])
    v = (ya.astype(D) - cell[:, 2]) / (cell[:, 3] - cell[:, 2])
    equal = (nc == nc[:, :1]).all(axis=1)
    dm.note(f"cross set-up [{instance}]: {len(pos)} cases ({int(special.sum())} special), n0 / gxn / gyn differ from the oracle in {[int(b) for b in bad.sum(axis=0)]}; "
            f"u = 0: {int((u == 0).sum())} (dividend -0: {int(((pos[:, 0] == 0) & np.signbit(pos[:, 0]) & (cell[:, 0] == 0)).sum())}), u = 1: {int((u == 1).sum())}, "
            f"v = 0: {int((v == 0).sum())}, v = 1: {int((v == 1).sum())}, outside [0, 1]: {int(((u < 0) | (u > 1) | (v < 0) | (v > 1)).sum())}, equal corners "
            f"{int(equal.sum())}, gradients -0 in the oracle: gxn {int(((want[:, 1] == 0) & np.signbit(want[:, 1])).sum())}, gyn {int(((want[:, 2] == 0) & np.signbit(want[:, 2])).sum())}")
    assert (u == 0).sum() > 200 and (u == 1).sum() > 200 and (v == 0).sum() > 200 and (v == 1).sum() > 200 and equal.sum() >= 30
    assert ((want[:, 2] == 0) & np.signbit(want[:, 2])).sum() > 30, "no -0 gyn in the population"
    if bad.any():
        i = int(np.flatnonzero(bad.any(axis=1))[0])
        raise AssertionError(f"{int(bad.any(axis=1).sum())} of {len(pos)} differ; first: case {i}, pos {[float(x).hex() for x in pos[i]]}, cell "
                             f"{[float(x).hex() for x in cell[i]]}, corners {[float(x).hex() for x in nc[i]]}, mirror {int(mirror[i])}: device "
                             f"{[float(x).hex() for x in got[i]]}, oracle {[float(x).hex() for x in want[i]]}")


# ------------------------------------------------------------------------------------------------ [C] the step
def _pm0(rng, n):
    return np.where(rng.random(n) < 0.5, F(0.0), F(-0.0)).astype(F)


@functools.lru_cache(maxsize=None)
def step_groups():
    """Group(name, c, state) lists, every state inside the ranges of the short forms (march_block_inputs.envelope says which)"""
    rng = np.random.default_rng(77003)
    out = []

    def plain(n, c):
        return mi._benign(rng, n, c)

    def grp(name, c, special, n_plain=512):
        sp = mi._grp(name, c, special).state
        pl = mi._grp(name, c, plain(n_plain, c)).state
        return mi.Group(f"zero_signs/{name}", c, in_waves(sp, pl, rng))

    c = F(0.5)
    # zeros of either sign in sx, sy and in the gradients: every combination, no refraction at all (t = 1e-12 / n > 0)
    n = 1024
    b = plain(n, c)
    kind = rng.integers(0, 3, n)
    sx, sy, sz = b["s"]
    sx = np.where(kind != 1, _pm0(rng, n), sx)
    sy = np.where(kind != 0, _pm0(rng, n), sy)
    b["s"] = list(mi.renorm(sx, sy, sz))
    b["gx"], b["gy"] = _pm0(rng, n), _pm0(rng, n)
    out.append(grp("zero_s_zero_gradient", c, b))
    # ... beside a gradient of the other axis of either sign: t of both signs while q of the zero axis is a zero quotient
    b = plain(n, c)
    kind = rng.integers(0, 2, n)
    sx, sy, sz = b["s"]
    sx = np.where(kind == 0, _pm0(rng, n), sx)
    sy = np.where(kind == 1, _pm0(rng, n), sy)
    b["s"] = list(mi.renorm(sx, sy, sz))
    b["gx"] = np.where(kind == 0, _pm0(rng, n), b["gx"])
    b["gy"] = np.where(kind == 1, _pm0(rng, n), b["gy"])
    out.append(grp("zero_axis_beside_a_gradient", c, b))
    # the widths of the interval records: lim0 = 0.1f * w_x, lim1 = 0.1f * w_y with r on either side of them
    b = plain(n, c)
    b["wx"], b["wy"] = rng.choice(np.array(WIDTHS), n), rng.choice(np.array(WIDTHS), n)
    b["gx"] = np.minimum(np.abs(b["gx"]), F(1.0) / b["wx"]) * np.sign(b["gx"])
    b["gy"] = np.minimum(np.abs(b["gy"]), F(1.0) / b["wy"]) * np.sign(b["gy"])
    lim = [F(0.1) * b["wx"], F(0.1) * b["wy"]]
    near = lambda l: np.select([kind == 0, kind == 1, kind == 2], [l, np.nextafter(l, F(0)), np.nextafter(l, F(np.inf))], l * rng.random(n).astype(F))
    kind = rng.integers(0, 4, n)
    b["r"] = [near(lim[0]) * rng.choice([-1, 1], n).astype(F), near(lim[1]) * rng.choice([-1, 1], n).astype(F), np.zeros(n, F)]
    b["lim2"] = mi.loguniform(rng, 1e-18, 1e-14, n).astype(F)      # steps far too short to move r: the comparison is with r itself
    out.append(grp("widths", c, b))
    # ht by decades: h = dzcap (a short sub-segment) and t from 1e-12 / n up to 1
    for cname, cc in (("c0.5", F(0.5)), ("cmin", mi.C_MIN)):
        b = plain(2048, cc)
        m = 2048
        g = (mi.loguniform(rng, 1e-13, 1.0, m) * rng.choice([-1, 1], m)).astype(F)
        g[rng.random(m) < 0.2] = 0
        b["gx"], b["gy"] = g, np.zeros(m, F)
        b["wx"] = np.minimum(b["wx"], F(1.0))
        b["lim2"] = mi.loguniform(rng, 1e-18, 1e-2, m).astype(F)
        out.append(grp(f"ht_decades_{cname}", cc, b))
    # a0 = +0 exactly (t = 0, ht = +0): sx gx = -1e-12f with a power of two
    b = plain(n, c)
    p = 2.0 ** rng.integers(1, 4, n)
    sx = -1.0 / p
    sz = np.sqrt(1.0 - sx * sx) * rng.choice([-1.0, 1.0], n)
    b["s"] = [sx.astype(F), np.zeros(n, F), sz.astype(F)]
    b["gx"], b["gy"] = (p * D(F(1e-12))).astype(F), np.zeros(n, F)
    out.append(grp("ht_zero", c, b))
    # ... and a few ulps of 1e-12f beside it under the shortest step there is: a0 = +-k 2^-63, ht subnormal
    b = plain(n, mi.C_MIN)
    e12 = np.full(n, F(1e-12))
    for _ in range(3):
        e12 = np.where(rng.random(n) < 0.5, np.nextafter(e12, F(1)), np.nextafter(e12, F(0))).astype(F)
    b["s"] = [sx.astype(F), np.zeros(n, F), sz.astype(F)]
    b["gx"], b["gy"] = (p * e12.astype(D)).astype(F), np.zeros(n, F)
    b["lim2"] = mi.loguniform(rng, 1e-18, 1e-15, n).astype(F)
    out.append(grp("ht_subnormal", mi.C_MIN, b))
    # h = h1 = c 0.1f / |t|: ht on the floats around c 0.1f = 0.05 -- a steep gradient under a long sub-segment
    b = plain(2048, c)
    m = 2048
    b["wx"] = b["wy"] = np.full(m, F(1.0))
    b["gx"] = (rng.uniform(0.5, 3.0, m) * rng.choice([-1, 1], m)).astype(F)
    b["gy"] = np.zeros(m, F)
    sxm = rng.uniform(0.9, 0.99, m)
    b["s"] = list(mi.renorm((sxm * rng.choice([-1, 1], m)).astype(F), np.zeros(m, F), np.sqrt(1 - sxm * sxm).astype(F)))
    b["lim2"] = mi.loguniform(rng, 1.0, 1e6, m).astype(F)
    out.append(grp("ht_at_its_largest", c, b))
    return tuple(out)


def _ht(state, c, ref):
    """ht = h * t of every case as the reference takes it, in float32 (hsum enters at 0: h is the hsum that comes out)"""
    with np.errstate(all="ignore"):
        k = mi.candidates(state, c)
        return (ref["out"][:, 7] - state[:, mi.HS]).astype(F) * k["t"]


@pytest.mark.parametrize("instance", tuple(dm.Device.STEP_INSTANCES))
def test_step_on_zeros_and_over_the_range_of_ht(dev, instance):
    failures, hts = [], []
    for g in step_groups():
        ref = oracle().linear_step(g.state, g.c)
        out, run, cnt = dev.march_step(instance, g.state, g.c)
        want_run = ref["run_geo"] if instance in NO_NTEST else ref["run_full"]
        bad_out = differs(out, ref["out"])
        bad = bad_out.any(axis=1) | (run != want_run)
        ht = _ht(g.state, g.c, ref)
        hts.append(ht)
        neg0 = lambda col: int(((g.state[:, col] == 0) & np.signbit(g.state[:, col])).sum())
        dm.note(f"step {g.name} [{instance}] c = {float(g.c):.9g}: {len(g.state)} cases, {int(bad.sum())} differ from the oracle; -0 in gx {neg0(mi.GX)}, "
                f"gy {neg0(mi.GY)}, sx {neg0(mi.SX)}, sy {neg0(mi.SY)}; t < 0 in {int((mi.candidates(g.state, g.c)['t'] < 0).sum())}; run {int(want_run.sum())}; "
                f"|ht| {float(np.nanmin(np.abs(ht))):.3g} .. {float(np.nanmax(np.abs(ht))):.9g}")
        assert cnt["waves"] == (len(g.state) + 63) // 64
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            per = ", ".join(f"{nm} {int(bad_out[:, k].sum())}" for k, nm in enumerate(OUT_NAMES) if bad_out[:, k].any())
            failures.append(f"{g.name} [{instance}]: {int(bad.sum())} of {len(g.state)} ({per}, run {int((run != want_run).sum())}); first: case {i}, state "
                            f"{[float(v).hex() for v in g.state[i]]}, device {[float(v).hex() for v in out[i]]} run {bool(run[i])}, oracle "
                            f"{[float(v).hex() for v in ref['out'][i]]} run {bool(want_run[i])}")
    # the census of ht over all groups: zero, subnormal, every decade from 1e-30 to 1e-2, the floats around 0.05
    a = np.abs(np.concatenate(hts))
    decades = {e: int(((a >= 10.0 ** e) & (a < 10.0 ** (e + 1))).sum()) for e in range(-30, -1)}
    around = int((np.abs(a.view(np.int32).astype(np.int64) - int(F(0.05).view(np.int32))) <= 4).sum())
    dm.note(f"step [{instance}]: ht = 0 in {int((a == 0).sum())}, subnormal in {int(((a > 0) & (a < 2.0 ** -126)).sum())}, per decade 1e-30 .. 1e-2 "
            f"{list(decades.values())}, within 4 ulp of 0.05f {around}, largest {float(a.max()):.9g}")
    assert (a == 0).sum() >= 64 and ((a > 0) & (a < 2.0 ** -126)).sum() >= 8 and min(decades.values()) >= 8 and around >= 64
    assert not failures, "\n".join(failures)
