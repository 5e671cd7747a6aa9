"""Device tier of the unit tests of the march's float32 blocks: one integrator step (csrc/rt_march_step.inc, block [C] of
rt_march.hip) in the four instances the product launches, the cross-cell set-up (csrc/rt_march_xsetup.inc, block [B]) and the
float primitives of csrc/rt_math.h, run on a device through csrc/librt_hip_devmath.so on the inputs of
tests/march_block_inputs.py.  tests/test_march_blocks_host.py asserts on the CPU what those inputs reach.

What is asserted -- bit equality throughout ("the march must take the reference's steps bit for bit"; a NaN equals a NaN):
  step        n, rx, ry, rz, sx, sy, sz, hsum of every case equal rt_oracle_linear_step -- the loop body of the oracle's
              step_linear_medium, true `/`, sqrtf and the `<` chain, compiled by the host compiler; run equals run_full, or
              run_geo in the instances without the index test.  Every population inside the envelope of the short forms in
              every instance; the population outside it in the generic instance (an infinite index apart, where the reference
              takes no step: see that test).  From the counters of the kernel's stand-in
              for MarchDiag: on the threshold population the division of each pruned candidate was skipped by at least one
              wave and executed by at least one; the tiny-dividend block ran.  Launches of 1, 63 and 65 cases give the first
              cases of the whole launch (a padded wave decides for its copies of the last case as well).
  set-up      n0, gxn, gyn equal rt_oracle_cross_setup, the loop head of the oracle's cross_cell (where two quotients of
              dividends below 1e-280 nearly cancel, the zero gradient may carry either sign: see that test)
  primitives  div_by_recip (float, double), div_by_recip_signed, fdiv_nr, fdiv_one_nr equal numpy's IEEE division where
              their comments claim exactness; the TINY_OK double form narrows to the float of the true quotient for dividends
              below 1e-280; fdiv_nr outside its envelope is never a finite value below the IEEE quotient; fmin_nan_drop is C's
              fminf; inv_norm equals (float)(1.0 / (double) sqrtf(q)) on every argument

Every test prints its census; with DEVMATH_PARITY_FILE set it is appended to that file (profiles/march_blocks_parity.txt is
such a run on an MI355X)."""
import functools

import numpy as np
import pytest

import devmath as dm
import devmath_inputs as di
import march_block_inputs as mi
from oracle.binding import Oracle

pytestmark = pytest.mark.gpu
D = dm.Device
F = np.float32
INSTANCES = tuple(D.STEP_INSTANCES)
NO_NTEST = ("prune", "prune_h24")
OUT_NAMES = ("n", "rx", "ry", "rz", "sx", "sy", "sz", "hsum")
FAMILIES = {"trajectory": mi.trajectory, "envelope": mi.envelope, "threshold": lambda: mi.threshold()[0], "specials": mi.specials}


@pytest.fixture(scope="module")
def dev(hip):
    return dm.Device.get()


@functools.lru_cache(maxsize=None)
def oracle():
    return Oracle()


@functools.lru_cache(maxsize=None)
def step_reference(name):
    """the oracle's step of one group, computed once and shared by the instances"""
    g = {g.name: g for g in mi.inside_groups() + mi.outside()}[name]
    return oracle().linear_step(g.state, g.c)


def differs(got, want):
    """elementwise: the bits differ, and not both are NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want))


def check_step(dev, instance, g):
    """runs one group in one instance, notes the census, returns (mismatching cases, counters, the outputs)"""
    ref = step_reference(g.name)
    out, run, cnt = dev.march_step(instance, g.state, g.c)
    want_run = ref["run_geo"] if instance in NO_NTEST else ref["run_full"]
    bad_out = differs(out, ref["out"])
    bad = bad_out.any(axis=1) | (run != want_run)
    share = np.bincount(ref["winner"], minlength=5) / max(1, len(g.state))
    per = ", ".join(f"{n} {int(bad_out[:, i].sum())}" for i, n in enumerate(OUT_NAMES) if bad_out[:, i].any())
    dm.note(f"step {g.name} [{instance}] c = {float(g.c):.9g}: {len(g.state)} cases, {int(bad.sum())} differ from the oracle"
            f"{' (' + per + ', run ' + str(int((run != want_run).sum())) + ')' if bad.any() else ''}; winners dzcap/h1/h2/h3/h4 "
            f"{'/'.join(f'{s:.3f}' for s in share)}; waves {cnt['waves']}, divided h1 in {cnt['prune'][0]}, h2 and h4 in {cnt['prune'][1]}, "
            f"pruning instance in {cnt['prune'][3]}, tiny-dividend block in {cnt['tiny']}")
    return bad, cnt, (out, run)


def describe(g, ref, out, run, i):
    return (f"case {i} of {g.name}: state {[float(v).hex() for v in g.state[i]]}, device {[float(v).hex() for v in out[i]]} run {bool(run[i])}, "
            f"oracle {[float(v).hex() for v in ref['out'][i]]} run_geo {bool(ref['run_geo'][i])} run_full {bool(ref['run_full'][i])} "
            f"winner {int(ref['winner'][i])} candidates {[float(v).hex() for v in ref['cand'][i]]}")


# --------------------------------------------------------------------------------------------------------- the step
@pytest.mark.parametrize("family", tuple(FAMILIES))
@pytest.mark.parametrize("instance", INSTANCES)
def test_step_equals_the_oracle(dev, instance, family):
    failures = []
    for g in FAMILIES[family]():
        bad, cnt, (out, run) = check_step(dev, instance, g)
        assert cnt["waves"] == (len(g.state) + 63) // 64
        if bad.any():
            failures.append(f"{int(bad.sum())} of {len(g.state)}; first: " + describe(g, step_reference(g.name), out, run, int(np.flatnonzero(bad)[0])))
        if family == "threshold" and instance in NO_NTEST:
            # the skip of each pruned candidate was taken by a wave and not taken by another
            which = int(g.name[-1])
            k = 0 if which == 1 else 1
            if which == 1 or instance == "prune_h24":
                assert 0 < cnt["prune"][k] < cnt["waves"], (g.name, cnt)
            assert cnt["prune"][3] == cnt["waves"]
        if instance == "prune":
            assert cnt["prune"][1] == cnt["waves"], "without PRUNE_H24 every wave divides h2 and h4"
        if instance not in NO_NTEST:
            assert cnt["prune"] == [0, 0, 0, 0]
        if g.name in ("specials/tiny_gradient", "specials/zero_gradient"):
            assert cnt["tiny"] == cnt["waves"], "the tiny-dividend block did not run"
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("group", [g.name for g in mi.outside()])
def test_step_outside_the_envelope_in_the_generic_instance(dev, group):
    """Bit equality with the oracle's step on every group but the infinite index.

    outside/n_inf: for n0 = +-inf the loop condition of Helper.h:279-280 is false before the first step -- n = n0 and
    (double) fabsf(inf - inf) < 0.05 compares a NaN -- so the reference takes no step from such a state (it never advances:
    the reason rt_hip_plan_create refuses a non-finite index), and what rt_oracle_linear_step computes from it is a step
    that step_linear_medium never takes.  Block [C] divides by the reciprocal, a0 * (1 / inf) corrected by fma(-inf, 0, a0):
    NaN where a true division gives 0.  Measured on an MI355X: n and run equal the oracle's in all 517 cases, the seven other
    outputs are NaN in all 517 where the oracle's are finite.  Asserted there: n and run -- what the reference defines -- are
    equal, and every other output is the oracle's float or a NaN, never a finite value of its own.  (The plan refuses every
    index that is not finite as a float, a double beyond the largest float included: tests/test_gpu_plan_update.py.)"""
    g = {g.name: g for g in mi.outside()}[group]
    ref = step_reference(g.name)
    bad, cnt, (out, run) = check_step(dev, "ieee", g)
    if group == "outside/n_inf":
        assert np.isinf(g.state[:, mi.N0]).all()
        assert not differs(out[:, 0], ref["out"][:, 0]).any() and not run.any() and not ref["run_full"].any()
        off = differs(out[:, 1:], ref["out"][:, 1:])
        dm.note(f"step {group} [ieee]: n and run equal in all {len(g.state)} cases; of the other outputs {int(off.sum())} differ, "
                f"{int((off & np.isnan(out[:, 1:])).sum())} of them NaN on the device")
        assert np.isnan(out[:, 1:][off]).all()
        return
    assert not bad.any(), f"{int(bad.sum())} of {len(g.state)}; first: " + describe(g, ref, out, run, int(np.flatnonzero(bad)[0]))


@pytest.mark.parametrize("instance", INSTANCES)
def test_step_ragged_launches(dev, instance):
    for g in (mi.envelope()[0], mi.threshold()[0][0], mi.specials()[2]):
        full, full_run, _ = dev.march_step(instance, g.state, g.c)
        for n in di.LAUNCH_SIZES:
            out, run, cnt = dev.march_step(instance, g.state[:n], g.c)
            assert cnt["waves"] == (n + 63) // 64
            assert np.array_equal(out.view(np.uint32), full[:n].view(np.uint32)) and np.array_equal(run, full_run[:n]), \
                f"{g.name} [{instance}]: a launch of {n} differs from the whole one"


# --------------------------------------------------------------------------------------------------------- the set-up
@pytest.mark.parametrize("group", [s.name for s in mi.setup()])
def test_setup_equals_the_oracle(dev, group):
    s = {s.name: s for s in mi.setup()}[group]
    want = oracle().cross_setup(s.pos, s.cell, s.nc, s.mirror)
    lo, w, rw = mi.interval_records(s.cell)
    got = dev.march_xsetup(s.pos, lo, w, rw, s.nc, s.mirror)
    bad = differs(got, want)
    zero_sign = bad & (got == 0) & (want == 0)
    dm.note(f"{group}: {len(s.pos)} cases, n0 / gxn / gyn differ from the oracle in {[int(v) for v in bad.sum(axis=0)]} "
            f"(a zero of the other sign in {[int(v) for v in zero_sign.sum(axis=0)]})")
    for n in di.LAUNCH_SIZES:
        part = dev.march_xsetup(s.pos[:n], lo[:n], w[:n], rw[:n], s.nc[:n], s.mirror[:n])
        assert np.array_equal(part.view(np.uint32), got[:n].view(np.uint32)), f"{group}: a launch of {n} differs from the whole one"
    if group == "setup/tiny_cancelling":
        # Two quotients of dividends below 1e-280 that nearly cancel: div_by_recip<TINY_OK> does not round such a quotient
        # correctly (its residual is subnormal; rt_math.h says so), each narrows to a zero either way, but their SUM is a
        # zero whose sign depends on the last bits: -0 where the correctly rounded quotients cancel to +0, or the reverse.
        # Every dividend of this group is below 1e-280, so every gradient must be a zero; its sign is the one thing left
        # open.  Measured on an MI355X: 29 of 8 197 gxn carry the other sign, no other difference.  (It takes indices of
        # refraction below 1e-235 in magnitude: the index itself is then 0 as a float and the step divides by it.)
        assert (np.abs(s.nc) < 1e-280).all() and (want[:, 1:] == 0).all()
        assert (got[:, 1:] == 0).all() and not bad[:, 0].any()
        return
    if bad.any():
        i = int(np.flatnonzero(bad.any(axis=1))[0])
        raise AssertionError(f"{group}: {int(bad.any(axis=1).sum())} of {len(s.pos)} differ; first: case {i}, pos {[float(v).hex() for v in s.pos[i]]}, "
                             f"cell {[float(v).hex() for v in s.cell[i]]}, corners {[float(v).hex() for v in s.nc[i]]}, mirror {int(s.mirror[i])}: "
                             f"device {[float(v).hex() for v in got[i]]}, oracle {[float(v).hex() for v in want[i]]}")


# --------------------------------------------------------------------------------------------------------- the primitives
def assert_exact(name, got, want, args, sel=None):
    bad = differs(got, want)
    if sel is not None:
        bad &= sel
    n = int(got.size if sel is None else sel.sum())
    dm.note(f"{name}: {n} results, {int(bad.sum())} differ from the IEEE result")
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {n} differ; first at {[float(a[i]).hex() for a in args]}: device {float(got[i]).hex()}, "
                             f"IEEE {float(want[i]).hex()}")


def test_float_div_by_recip(dev):
    a, b, y = mi.prim_div_f32()
    with np.errstate(all="ignore"):
        want = a / b
    assert_exact("div_by_recip (float)", dev.f32(D.DIV_BY_RECIP, a, b, y), want, (a, b, y))
    # the unguarded form: its callers keep non-zero dividends below 1e-29 away from it
    sel = ~((np.abs(a) < F(1e-29)) & (a != 0))
    assert_exact("div_by_recip_signed", dev.f32(D.DIV_BY_RECIP_SIGNED, a, b, y), want, (a, b, y), sel)


def test_double_div_by_recip(dev):
    a, b, y = mi.prim_div_f64()
    with np.errstate(all="ignore"):
        want = a / b
    assert_exact("div_by_recip (double)", dev.f64_div(D.F64_DIV_BY_RECIP, a, b, y), want, (a, b, y))
    got = dev.f64_div(D.F64_DIV_BY_RECIP_TINY_OK, a, b, y)
    tiny = (np.abs(a) < 1e-280) & (a != 0)
    assert tiny.sum() > 1000
    assert_exact("div_by_recip<TINY_OK> (double), dividends of at least 1e-280 and zeros", got, want, (a, b, y), ~tiny)
    # below: "narrows to a zero of the right sign either way"
    with np.errstate(all="ignore"):
        assert_exact("div_by_recip<TINY_OK> (double) narrowed to float, dividends below 1e-280", got.astype(F), want.astype(F), (a, b, y), tiny)


def test_fdiv_nr_inside_its_envelope(dev):
    a, b = mi.prim_fdiv_inside()
    with np.errstate(all="ignore"):
        want = a / b
    assert_exact("fdiv_nr inside its envelope", dev.f32(D.FDIV_NR, a, b), want, (a, b))
    b1 = mi.prim_fdiv_one()
    assert_exact("fdiv_one_nr inside its envelope", dev.f32(D.FDIV_ONE_NR, None, b1), F(1) / b1, (b1,))


def test_fdiv_nr_outside_its_envelope_is_never_small(dev):
    """what the step relies on where a candidate leaves the envelope: huge, infinite or NaN -- never a finite value below
    the quotient, which could be taken for the minimum"""
    a, b = mi.prim_fdiv_outside()
    with np.errstate(all="ignore"):
        want = a / b
    got = dev.f32(D.FDIV_NR, a, b)
    bad = np.isfinite(got) & (got < want)
    dm.note(f"fdiv_nr outside its envelope: {a.size} pairs, {int(np.isnan(got).sum())} NaN, {int(np.isinf(got).sum())} infinite, "
            f"{int((np.isfinite(got) & ~differs(got, want)).sum())} finite and equal to the IEEE quotient, {int(bad.sum())} finite and below it")
    assert not bad.any(), (float(a[bad][0]).hex(), float(b[bad][0]).hex(), float(got[bad][0]).hex())


def test_fmin_nan_drop_is_fminf(dev):
    a, b = mi.prim_fmin()
    got = dev.f32(D.FMIN_NAN_DROP, a, b)
    want = np.fmin(a, b)
    # C leaves the sign of fminf(+0, -0) open; any zero is fminf there
    zeros = (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))
    bad = np.where(zeros, got != 0, differs(got, want))
    dm.note(f"fmin_nan_drop: {a.size} pairs, {int(bad.sum())} differ from fminf; of +0 and -0 it returns "
            f"{sorted(set(float(v).hex() for v in got[zeros]))}")
    assert not bad.any(), (float(a[bad][0]).hex(), float(b[bad][0]).hex(), float(got[bad][0]).hex())
    both = np.isnan(a) & np.isnan(b)
    assert np.isnan(got[both]).all() and not np.isnan(got[~both]).any()


def test_inv_norm(dev):
    q = mi.prim_inv_norm()
    with np.errstate(all="ignore"):
        want = (1.0 / np.sqrt(q).astype(np.float64)).astype(F)
    got = dev.f32(D.INV_NORM, q)
    assert_exact("inv_norm", got, want, (q,))
    for n in di.LAUNCH_SIZES:
        assert np.array_equal(dev.f32(D.INV_NORM, q[:n]).view(np.uint32), got[:n].view(np.uint32))
