"""CPU tier of the device-math tests: the C restatement of the float64 building blocks of rt_freq.hip
(tests/devmath_ref.c, compiled here with `cc -O2 -ffp-contract=off`) with CORRECTLY ROUNDED tables, against exp / expm1 in
long double, on the inputs of tests/devmath_inputs.py.  It asserts the bounds the source states; the device tier
(test_gpu_devmath.py) asserts the same bounds plus the device's table error, and that the device equals this restatement
bit for bit when both use the device's tables.

Measured here (correctly rounded tables, 2.87 M exponent arguments, 2.80 M / 1.54 M step arguments):
    exp_tab        1.957 ulp   (stated: <= 2)
    exp_tab_vec    2.282 ulp   (the comment said <= 2; the vector form drops r^5/120.  Stated now: <= 2.3)
    ase_step       e^x - 1 to 1.4e-13 e^x beyond the rounding of S - 1 (stated 1e-10); tiny x: 1.0354e-10 of e^x - 1
                   (the comment said 1e-10: (ln2/512)^3 / 24 = 1.03e-10 is what the quadratic leaves out.  Stated now: 1.04e-10)
    ase_step_f32   e^x - 1 to 1.9e-10 e^x (stated 3e-10); tiny x: 1.09e-7 of e^x - 1 (2^-23 = 1.19e-7)"""
import numpy as np
import pytest

import devmath as dm
import devmath_inputs as di


@pytest.fixture(scope="module")
def ref():
    dm.require_long_double()
    return dm.Ref.get()


@pytest.fixture(scope="module")
def tabs():
    return dm.correct_tables()


def test_the_reference_agrees_with_40_digit_arithmetic():
    dm.require_long_double()
    x = di.exp_args()
    w = dm.crosscheck_reference("exp", x, dm.exp_ref(x))
    xs = di.step_args(708.0).astype(np.float64)
    w1 = dm.crosscheck_reference("expm1", xs, dm.expm1_ref(xs))
    dm.note(f"host: long double exp / expm1 against 40 digits on 2000 points each: {w:.2e} / {w1:.2e} relative")


def test_correct_tables_are_what_they_say(tabs):
    tab, tab2 = tabs
    assert tab[0] == 1.0 and np.all(np.diff(tab) > 0) and tab[255] < 2.0
    j = np.arange(256)
    # correctly rounded: within half an ulp of 2^(j/256) in long double (whose own error is 2^-11 ulp)
    err = dm.ulp_error(tab, np.exp2(dm.ld(j / 256.0)))
    assert err.max() <= 0.5 + 2.0 ** -10
    hi, lo = tab.view(np.uint64) >> np.uint64(32), tab.view(np.uint64) & np.uint64(0xffffffff)
    hi2, lo2 = tab2.view(np.uint64) >> np.uint64(32), tab2.view(np.uint64) & np.uint64(0xffffffff)
    assert np.array_equal(lo, lo2) and np.array_equal(hi2 + (j.astype(np.uint64) << np.uint64(12)), hi)


def test_exp_tab_within_its_stated_bound(ref, tabs):
    x = di.exp_args()
    got = ref.exp_tab(tabs[0], x)
    dm.gate_exp("host exp_tab", got, x, dm.EXP_TAB_ULP)
    assert (got[np.isnan(x)] == 0.0).all()        # a NaN argument is clamped away: callers re-test


def test_exp_tab_vec_within_its_stated_bound(ref, tabs):
    x = di.exp_args()
    got = ref.exp_tab_vec(tabs[0], x)
    dm.gate_exp("host exp_tab_vec", got, x, dm.EXP_TAB_VEC_ULP)
    assert np.isnan(got[np.isnan(x)]).all() and np.isnan(x).any()


@pytest.mark.parametrize("form", ["ase_step", "ase_step_f32"])
def test_expm1_of_the_step_forms(ref, tabs, form):
    """Iv = 0, rs = 1: the step returns its e^x - 1 itself (fma(em1, 0 + 1, 0) is exact)."""
    limit, fn, tab, B, tiny = ((708.0, ref.ase_step, tabs[0], dm.EM1_B_F64, dm.TINY_REL_F64) if form == "ase_step" else
                               (80.0, ref.ase_step_f32, tabs[1], dm.EM1_B_F32, dm.TINY_REL_F32))
    x = di.step_args(limit)
    g = len(x) // dm.VEC
    got = fn(tab, np.zeros(len(x)), np.ones(g, np.float32), np.ones(g), x)
    dm.gate_em1(f"host {form}", got, x.astype(np.float64), B, tiny)


@pytest.mark.parametrize("form", ["ase_step", "ase_step_f32"])
def test_step_forms_with_general_intensity_and_source(ref, tabs, form):
    limit, fn, tab, B = ((708.0, ref.ase_step, tabs[0], dm.EM1_B_F64) if form == "ase_step" else
                         (80.0, ref.ase_step_f32, tabs[1], dm.EM1_B_F32))
    Iv, gs, rs, w = di.step_general_args(limit)
    dm.gate_step_general(f"host {form}, general", fn(tab, Iv, gs, rs, w), Iv, gs, rs, w, B)


def test_ase_update_against_the_cpu_formula(ref, tabs):
    Iv, gs, es, w, near = di.update_args()
    got, branch = ref.ase_update(tabs[0], Iv, gs, es, w)
    _, small, _, _, _ = dm.update_reference(Iv, gs, es, w)
    assert np.array_equal(branch, small)
    dm.gate_update("host ase_update", got, Iv, gs, es, w, near)
