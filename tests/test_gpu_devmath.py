"""Device tier of the device-math tests: the float64 building blocks of the frequency pass (exp_tab, exp_tab_vec,
ase_update, ase_step, ase_step_f32, div_fast, deposit_index_fast, deposit_index4 of rt_freq.hip) and the two float kernels
of the march (tanf_flt32_kernel, atanf_flt32_kernel of rt_march.hip), run on a device through csrc/librt_hip_devmath.so
(rt_devmath.hip: one elementwise kernel per function, the exponent tables filled by the product's own RT_FILL_EXP_TABLES)
on the inputs of tests/devmath_inputs.py.

What is asserted:
  tables        every tab[j] within 1 ulp of the correctly rounded 2^(j/256) (the device library's exp2 is not correctly
                rounded); tab[256 + j] = tab[j] with j << 12 taken from its high word, exactly; first work-group = last
  bit equality  exp_tab, exp_tab_vec, ase_step, ase_step_f32 equal tests/devmath_ref.c FED THE DEVICE'S TABLES on every
                input: those are fma / mul / add / ldexp sequences with nothing left to contract, so a difference is a
                finding about the compiler, the inline assembly or the table trick
  bounds        against exp / expm1 / exact quotients in long double (devmath.py): the bounds of the CPU tier
                (test_devmath_host.py) plus 1 ulp for the device's table entries
  div_fast      <= 2 ulp of the exact quotient (the "1-2 ulp" of the header of rt_freq.hip)
  ase_update    the CPU formula in long double, per-branch bounds, and the CPU's branch for every float around 1e-3
  deposit       deposit_index_fast and deposit_index4 equal the reference rule (element_gate.deposit_index, itself checked
                here against the plain bisection) on every input, and each other
  tan / atan    bit-equal to the host libm's tanf up to 1.375 rad / atanf below 0.4375; beyond, within 1 float ulp of the
                correctly rounded value; libm's answers for +-inf and NaN
  E_v wave sum  rt_step_evsum.inc on one work-group of four waves: the accumulator equals numpy's sum over the depositing
                lanes, ==.  The inputs are integers up to 2^20 in doubles and the scale is a power of two, so every
                association of the additions is exact and no tolerance is needed
  nf scan       rt_wave_runs.inc / rt_wave_runscan.inc on one work-group of four waves: nf equals np.add.at over the lanes
                that hold a pixel, ==, on the same kind of input

Every test prints its worst figures and where they occur; with DEVMATH_PARITY_FILE set they are appended to that file
(profiles/devmath_parity.txt is such a run on an MI355X).

Measured on an MI355X: 20 of the 256 table entries lie 1 ulp off the correctly rounded value (6 above, 14 below); no
result of the four sequences differs from the restatement; exp_tab 1.972 ulp, exp_tab_vec 2.193 ulp; e^x - 1 of ase_step
1.4e-13 of e^x (1.0354e-10 of itself for tiny x), of ase_step_f32 1.9e-10 (1.09e-7); div_fast correctly rounded (0.500 ulp)
on all 2.0 M quotients; ase_update at 0.31 / 0.63 of its bounds; every deposit cell equal to the rule; tan / atan equal to the
host libm in the exact ranges and to the correctly rounded float beyond them."""
import numpy as np
import pytest

import devmath as dm
import devmath_inputs as di
from element_gate import deposit_index

pytestmark = pytest.mark.gpu
D = dm.Device


@pytest.fixture(scope="module")
def dev(hip):
    dm.require_long_double()
    return dm.Device.get()


@pytest.fixture(scope="module")
def ref():
    return dm.Ref.get()


@pytest.fixture(scope="module")
def dtabs(dev):
    """(tab, tab2) as the first of 300 work-groups holds them."""
    first, _ = dev.tables(300)
    return first[:dm.EXP_TAB].copy(), first[dm.EXP_TAB:].copy()


def assert_bits_equal(name, got, want, describe):
    a, b = np.asarray(got).view(np.uint64), np.asarray(want).view(np.uint64)
    bad = np.flatnonzero(a != b)
    dm.note(f"{name}: {a.size} results, {bad.size} differ from the restatement fed the device's tables")
    assert bad.size == 0, (f"{name}: {bad.size} of {a.size} differ; first at {describe(int(bad[0]))}: device "
                           f"{float(got[bad[0]]).hex()}, restatement {float(want[bad[0]]).hex()}")


def assert_prefixes(name, run, full, sizes=di.LAUNCH_SIZES):
    """launches of 1, 63 and 65 items give the first items of the whole launch, bit for bit"""
    for n in sizes:
        part = run(n)
        assert part.shape == full[:len(part)].shape
        assert np.array_equal(part.view(np.uint8), full[:len(part)].view(np.uint8)), f"{name}: a launch of {n} differs from the whole one"


# ------------------------------------------------------------------------------------------------------- tables
def test_tables_as_a_wave_sees_them(dev):
    first, last = dev.tables(300)
    one, same = dev.tables(1)
    same_bits = lambda a, b: bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    assert same_bits(first, last), "first and last work-group hold different tables"
    assert same_bits(first, one), "a launch of one work-group holds other tables than one of 300"
    assert same_bits(one, same)
    tab, tab2 = first[:256], first[256:]
    want, _ = dm.correct_tables()
    off = (tab.view(np.int64) - want.view(np.int64))
    dm.note(f"device tables: {int((off != 0).sum())} of 256 entries differ from the correctly rounded 2^(j/256) "
            f"({int((off > 0).sum())} one ulp above, {int((off < 0).sum())} one ulp below), largest |difference| {int(np.abs(off).max())} ulp; "
            f"j = {np.flatnonzero(off).tolist()}")
    assert np.abs(off).max() <= 1
    assert tab[0] == 1.0
    assert np.array_equal(tab2.view(np.uint64), dm.second_table(tab).view(np.uint64)), "second table: high word less j << 12"


# ------------------------------------------------------------------------------------------------------- exponentials
@pytest.mark.parametrize("form", ["exp_tab", "exp_tab_vec"])
def test_exponentials(dev, ref, dtabs, form):
    which, restated, bound = ((D.EXP_TAB, ref.exp_tab, dm.EXP_TAB_ULP) if form == "exp_tab" else
                              (D.EXP_TAB_VEC, ref.exp_tab_vec, dm.EXP_TAB_VEC_ULP))
    x = di.exp_args()
    assert len(x) % 256 == 3 and len(x) % dm.VEC == 3
    got = dev.exp(which, x)
    assert_prefixes(form, lambda n: dev.exp(which, x[:n]), got)
    assert_bits_equal(f"device {form}", got, restated(dtabs[0], x), lambda i: f"x = {x[i]!r} ({float(x[i]).hex()})")
    dm.gate_exp(f"device {form}", got, x, bound, table_ulp=1.0)
    nan = np.isnan(x)
    assert nan.any()
    if form == "exp_tab":
        assert (got[nan] == 0.0).all(), "exp_tab clamps a NaN away and returns 0: callers re-test"
    else:
        assert np.isnan(got[nan]).all(), "exp_tab_vec gives NaN for NaN"


# ------------------------------------------------------------------------------------------------------- step forms
def _form(ref, dtabs, form):
    if form == "ase_step":
        return 708.0, D.STEP_F64, ref.ase_step, dtabs[0], dm.EM1_B_F64, dm.TINY_REL_F64
    return 80.0, D.STEP_F32, ref.ase_step_f32, dtabs[1], dm.EM1_B_F32, dm.TINY_REL_F32


@pytest.mark.parametrize("form", ["ase_step", "ase_step_f32"])
def test_expm1_of_the_step_forms(dev, ref, dtabs, form):
    """Iv = 0, rs = 1, gs = 1: the step returns its e^x - 1 of x = w itself."""
    limit, which, restated, tab, B, tiny = _form(ref, dtabs, form)
    x = di.step_args(limit)
    g = len(x) // dm.VEC
    assert len(x) % dm.VEC == 0 and g % 256 != 0      # whole groups, a ragged last work-group
    Iv, gs, rs = np.zeros(len(x)), np.ones(g, np.float32), np.ones(g)
    got = dev.step(which, Iv, gs, rs, x)
    assert_prefixes(form, lambda n: dev.step(which, Iv[:4 * n], gs[:n], rs[:n], x[:4 * n]), got)
    assert_bits_equal(f"device {form}, e^x - 1", got, restated(tab, Iv, gs, rs, x), lambda i: f"x = {x[i]!r} ({float(x[i]).hex()})")
    dm.gate_em1(f"device {form}", got, x.astype(np.float64), B, tiny, table_ulp=1.0)


@pytest.mark.parametrize("form", ["ase_step", "ase_step_f32"])
def test_step_forms_with_general_intensity_and_source(dev, ref, dtabs, form):
    limit, which, restated, tab, B, _ = _form(ref, dtabs, form)
    Iv, gs, rs, w = di.step_general_args(limit)
    got = dev.step(which, Iv, gs, rs, w)
    assert_bits_equal(f"device {form}, general", got, restated(tab, Iv, gs, rs, w),
                      lambda i: f"Iv = {Iv[i]!r}, gs = {gs[i // 4]!r}, rs = {rs[i // 4]!r}, w = {w[i]!r}")
    dm.gate_step_general(f"device {form}, general", got, Iv, gs, rs, w, B, table_ulp=1.0)


# ------------------------------------------------------------------------------------------------------- update, division
def test_ase_update_against_the_cpu_formula(dev):
    Iv, gs, es, w, near = di.update_args()
    assert len(Iv) % 256 == 3
    got = dev.update(Iv, gs, es, w)
    assert_prefixes("ase_update", lambda n: dev.update(Iv[:n], gs[:n], es[:n], w[:n]), got)
    dm.gate_update("device ase_update", got, Iv, gs, es, w, near)


def test_div_fast_within_two_ulp(dev):
    """The quotient of two floats in long double is exact to 2^-64 relative, 2^-11 ulp of a double."""
    a, b = di.div_args()
    assert len(a) % 256 == 3
    q = dev.div(a, b)
    assert_prefixes("div_fast", lambda n: dev.div(a[:n], b[:n]), q)
    ref = dm.ld(a) / dm.ld(b)
    err = dm.ulp_error(q, ref)
    w, i = dm.worst(err, np.arange(len(a)))
    hist = [int((err > t).sum()) for t in (0.5, 1.0, 1.5)]
    dm.note(f"device div_fast: {len(a)} quotients, worst {w:.3f} ulp at a = {a[i]!r}, b = {b[i]!r}; beyond 0.5 / 1 / 1.5 ulp: "
            f"{hist[0]} / {hist[1]} / {hist[2]}; bound 2 ulp")
    assert not np.isnan(err).any()
    assert w <= 2.0
    assert (q[a == 0] == 0).all()


# ------------------------------------------------------------------------------------------------------- deposit cells
def plain_rule(g, d, v):
    """RayTraceImageCPU.cpp:11-16 with the bisection of Helper.h:101-117, one value at a time.  None where the
    reference's loop would not end: one grid point and v - d/2 == g[0], or NaN."""
    n = len(g)
    if v < g[0] - 0.5 * d or v > g[n - 1] + 0.5 * d:
        return -1
    t = v - 0.5 * d
    if t < g[0]:
        return 0
    if t > g[n - 1]:
        return n
    lo, hi = 0, n - 1
    if hi == lo:
        return None
    while hi - lo != 1:
        mid = (hi + lo) // 2
        if g[mid] >= t:
            hi = mid
        else:
            lo = mid
    return hi


def expected_cells(g, d, v):
    """The reference rule on an array: element_gate.deposit_index.  With ONE grid point the reference's bisection does
    not end for v - d/2 == g[0] and for NaN; rt_freq.hip returns n = 1 there ("if (n < 2) return n"), and so does this."""
    idx = deposit_index(g, d, v)
    if len(g) == 1:
        t = v - 0.5 * d
        idx = np.where((t == g[0]) | np.isnan(v), 1, idx)
    return idx


def test_deposit_cells_equal_the_reference_rule(dev):
    rng = np.random.default_rng(7)
    for c, (grids, d, v) in enumerate(di.deposit_cases()):
        assert len(v) % 256 == 3
        fast = dev.deposit(D.DEPOSIT_FAST, grids, d, v)
        four = dev.deposit(D.DEPOSIT_4, grids, d, v)
        assert_prefixes("deposit_index4", lambda n: dev.deposit(D.DEPOSIT_4, grids, d, v[:n]), four)
        for a in range(4):
            g, dd, va = grids[a], d[a], v[:, a]
            want = expected_cells(g, dd, va)
            # the numpy restatement against the plain bisection: every special value, every value near a cell edge of a
            # small grid, 2000 of the others
            special = np.flatnonzero(~np.isfinite(va) | (np.abs(va) > 1e299))
            pick = np.unique(np.concatenate([special, rng.choice(len(va), 2000, replace=False)]))
            for i in pick:
                r = plain_rule(g, dd, float(va[i]))
                assert (r is None and len(g) == 1 and want[i] == 1) or r == want[i], (len(g), va[i], r, want[i])
            for name, got in (("deposit_index_fast", fast[:, a]), ("deposit_index4", four[:, a])):
                bad = np.flatnonzero(got != want)
                dm.note(f"device {name}: case {c} axis {a} (n = {len(g)}, d = {dd:g}): {len(va)} coordinates, {bad.size} differ "
                        f"from the reference rule; cells hit {np.unique(want).size} of {len(g) + 2}")
                assert bad.size == 0, f"{name}: n = {len(g)}, v = {va[bad[0]]!r} ({float(va[bad[0]]).hex()}): {got[bad[0]]}, rule {want[bad[0]]}"
            assert np.array_equal(fast[:, a], four[:, a])
            # every outcome occurs: -1 and 0 .. n - 1 (n itself needs v - d/2 > g[n-1] with v <= g[n-1] + d/2: by rounding
            # only; with one grid point it is the answer for v - d/2 == g[0])
            assert np.unique(want).size >= len(g) + 1


# ------------------------------------------------------------------------------------------------------- tangent, arctangent
def _ordered(f):
    i = np.asarray(f, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _mp_float32(fn, x):
    import mpmath as mp
    f = {"tan": mp.tan, "atan": mp.atan}[fn]
    with mp.workprec(100):
        return np.array([float(f(mp.mpf(float(v)))) for v in x]).astype(np.float32)


def _float_kernel(dev, ref, which, fn, x, exact_mask, host):
    got = dev.tan(which, x)
    assert_prefixes(fn, lambda n: dev.tan(which, x[:n]), got)
    fin = np.isfinite(x)
    want = host(x)
    # non-finite arguments: libm's answers
    assert np.array_equal(np.isnan(got[~fin]), np.isnan(want[~fin]))
    keep = ~fin & ~np.isnan(want)
    assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32))
    ex = fin & exact_mask
    bad = np.flatnonzero(ex & (got.view(np.uint32) != want.view(np.uint32)))
    dm.note(f"device {fn}f kernel: {int(ex.sum())} floats of the exact range, {bad.size} differ from the host libm")
    assert bad.size == 0, f"{fn}: x = {x[bad[0]]!r} ({float(x[bad[0]]).hex()}): device {got[bad[0]]!r}, host {want[bad[0]]!r}"
    wide = np.flatnonzero(fin & ~exact_mask)
    with np.errstate(all="ignore"):
        exact = getattr(np, "tan" if fn == "tan" else "arctan")(x[wide].astype(dm.LD)).astype(np.float32)
    dist = np.abs(_ordered(got[wide]) - _ordered(exact))
    i = int(np.argmax(dist))
    # the issue's reference, mpmath, on every 64th of them and on everything within 64 floats of FLT_MAX and of the range's start
    ax = np.abs(x[wide])
    sub = np.flatnonzero((np.arange(len(wide)) % 64 == 0) | (ax >= np.float32(3.4028e38)) | (ax <= np.sort(ax)[130]))
    try:
        mpv = _mp_float32(fn, x[wide][sub])
        dist_mp = np.abs(_ordered(got[wide][sub]) - _ordered(mpv))
        ref_gap = int(np.abs(_ordered(exact[sub]) - _ordered(mpv)).max())
        j = int(np.argmax(dist_mp))
        dm.note(f"device {fn}f kernel: {len(sub)} floats beyond the exact range against mpmath: worst {int(dist_mp.max())} ulp at "
                f"x = {x[wide][sub][j]!r}; long double {fn} rounds to another float than mpmath by at most {ref_gap} ulp there")
        assert dist_mp.max() <= 1 and ref_gap == 0
    except ImportError:
        dm.note(f"device {fn}f kernel: mpmath is not importable; long double {fn} alone is the reference beyond the exact range")
    dm.note(f"device {fn}f kernel: {len(wide)} floats beyond the exact range, worst {int(dist.max())} ulp of the correctly "
            f"rounded float at x = {x[wide][i]!r}; {int((dist == 0).sum())} equal it")
    assert dist.max() <= 1, f"{fn}: x = {x[wide][i]!r}: device {got[wide][i]!r}, correctly rounded {exact[i]!r}"


def test_tanf_kernel(dev, ref):
    x = di.tan_args()
    _float_kernel(dev, ref, D.TAN, "tan", x, np.abs(x) <= np.float32(1.375), ref.host_tanf)


def test_atanf_kernel(dev, ref):
    x = di.atan_args()
    _float_kernel(dev, ref, D.ATAN, "atan", x, np.abs(x) < np.float32(0.4375), ref.host_atanf)


# ------------------------------------------------------------------------------------------------------- the step deposit
def _integers(rng, shape):
    """doubles holding integers of magnitude <= 2^20: sums of 256 of them, times a power of two, are exact in any order"""
    return rng.integers(-2 ** 20, 2 ** 20, size=shape, endpoint=True).astype(np.float64)


EV_MASKS = {
    "every lane": np.ones(64, bool),
    "no lane": np.zeros(64, bool),
    "alternating lanes": np.arange(64) % 2 == 0,
    "only lane 0": np.arange(64) == 0,
    "only lane 63": np.arange(64) == 63,
}


@pytest.mark.parametrize("case", list(EV_MASKS))
def test_ev_wave_sum_is_the_sum_over_the_depositing_lanes(dev, case):
    Kp, scale = 8, 2.0 ** -5          # two batches of VEC frequencies: the index of the accumulator entry moves
    assert Kp == 2 * dm.VEC
    rng = np.random.default_rng(11)
    Iv = _integers(rng, (4, 64, Kp))
    deposits = np.broadcast_to(EV_MASKS[case], (4, 64))
    got = dev.ev_sum(Iv, deposits, scale)
    want = scale * (Iv * deposits[:, :, None]).sum(axis=(0, 1))
    dm.note(f"device E_v wave sum, {case}: {int(deposits.sum())} depositing lanes in four waves, {int((got != want).sum())} of {Kp} sums differ")
    assert np.array_equal(got, want), (case, got, want)
    if case == "no lane":
        assert (got == 0.0).all() and not np.signbit(got).any()      # the accumulator stays as it was zeroed


def _lanes(runs):
    """(pixel, lanes) runs -> the 64 pixels of a wave"""
    pix = np.concatenate([np.full(n, p) for p, n in runs])
    assert pix.size == 64
    return pix


NF_PATTERNS = {
    "one run of 64": [(5, 64)],
    "64 runs of one": [(p, 1) for p in range(3, 67)],
    "mixed runs": [(9, 1), (10, 2), (11, 3), (12, 5), (20, 8), (21, 13), (69, 32)],
    "holes inside and at both ends": [(-1, 3), (4, 7), (-1, 1), (5, 2), (-1, 20), (6, 1), (7, 25), (-1, 5)],
    "the same pixel in two runs": [(30, 10), (31, 4), (30, 17), (0, 1), (31, 32)],
    "a run from lane 0, a run to lane 63": [(68, 31), (2, 2), (69, 31)],
}


@pytest.mark.parametrize("case", list(NF_PATTERNS))
def test_nf_segmented_scan_equals_add_at(dev, case):
    n_pix, scale = 70, 2.0 ** 3
    base = _lanes(NF_PATTERNS[case])
    # four waves: the pattern on other pixels (equal pixels stay equal, holes stay holes), so that waves meet in a pixel
    pix = np.stack([np.where(base >= 0, (base + 17 * w) % n_pix, -1) for w in range(4)])
    val = _integers(np.random.default_rng(13), (4, 64))
    got = dev.nf_scan(pix, val, scale, n_pix)
    want = np.zeros(n_pix)
    hold = pix >= 0
    np.add.at(want, pix[hold], val[hold] * scale)
    dm.note(f"device nf scan, {case}: {int(hold.sum())} lanes with a pixel in four waves, {int((got != want).sum())} of {n_pix} pixels differ")
    assert np.array_equal(got, want), (case, np.flatnonzero(got != want))
