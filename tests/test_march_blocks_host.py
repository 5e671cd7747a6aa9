"""CPU tier of the unit tests of the march's float32 blocks: what the populations of tests/march_block_inputs.py reach, asserted
from the oracle's own outputs, so that an empty population cannot hide behind a green device tier
(tests/test_gpu_march_blocks.py); the two checks that the threshold population straddles the pruning constant; and that the
step the oracle exports, iterated, is the step of its march.

Coverage, over the populations inside the envelope of the short forms (trajectory, envelope, threshold, specials):
  every one of dzcap, h1, h2, h3, h4 sets at least 1 000 steps by the reference's `<` chain;
  each of h1, h2, h4 has at least 1 000 cases on either side of K dzcap within 400 x 2^-23 of it (K = 1.00002f);
  at least 50 waves (64 consecutive cases of a launch) all of whose lanes pass the division-free test, per pruned candidate;
  at least 1 000 cases with a non-finite reference candidate, 1 000 with a tiny non-zero dividend (|gx|, |gy| or |a0| below
  1e-29), 1 000 in which the geometric loop tests and the full loop condition differ."""
import functools

import numpy as np

import march_block_inputs as mi
import march_steps
from oracle.binding import Oracle

F = np.float32
WINDOW = 400 * mi.EPS


@functools.lru_cache(maxsize=None)
def oracle():
    return Oracle()


@functools.lru_cache(maxsize=None)
def census():
    """per group inside the envelope: the oracle's step and the numerators / denominators of the pruned candidates"""
    out = []
    for g in mi.inside_groups():
        out.append((g, oracle().linear_step(g.state, g.c), mi.candidates(g.state, g.c)))
    return out


def test_the_numpy_candidates_are_the_oracles():
    # (the division-free test below is evaluated on them)
    for g, o, cd in census():
        for j, k in ((0, 0), (1, 1), (2, 3)):
            a, b = cd["quo"][j], o["cand"][:, k]
            same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
            assert same.all(), (g.name, j, int((~same).sum()))


def test_every_candidate_sets_steps():
    winners = sum(np.bincount(o["winner"], minlength=5) for _, o, _ in census())
    print("steps set by dzcap, h1, h2, h3, h4:", winners)
    assert (winners >= 1000).all(), winners


def test_candidates_straddle_the_pruning_constant():
    K = float(mi.K_PRUNE)
    below, above = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for g, o, cd in census():
        dz = g.state[:, mi.DZCAP].astype(np.float64)
        for j, k in ((0, 0), (1, 1), (2, 3)):
            with np.errstate(all="ignore"):
                ratio = o["cand"][:, k].astype(np.float64) / dz
            below[j] += int(((ratio < K) & (ratio >= K - WINDOW)).sum())
            above[j] += int(((ratio >= K) & (ratio <= K + WINDOW)).sum())
    print("h1, h2, h4 within 400 x 2^-23 below K dzcap:", below, "at or above:", above)
    assert (below >= 1000).all() and (above >= 1000).all(), (below, above)


def test_whole_waves_pass_the_division_free_test():
    waves = np.zeros(3, np.int64)
    both = 0
    for g, o, cd in census():
        m = len(g.state) // mi.WAVE * mi.WAVE
        ok = [mi.prunable(cd["num"][j], cd["den"][j], g.state[:, mi.DZCAP])[:m].reshape(-1, mi.WAVE).all(axis=1) for j in range(3)]
        if not g.name.startswith("threshold/"):
            continue                                   # (counted where the waves were arranged for it)
        waves += [int(v.sum()) for v in ok]
        both += int((ok[1] & ok[2]).sum())
    print("waves all of whose lanes may skip h1, h2, h4:", waves, "h2 and h4 together:", both)
    assert (waves >= 50).all() and both >= 50, (waves, both)
    groups, kinds = mi.threshold()
    for g in groups:
        assert len(g.state) % mi.WAVE == 0 and len(kinds[g.name]) == len(g.state) // mi.WAVE
        which = int(g.name[-1])
        cd = mi.candidates(g.state, g.c)
        dz = g.state[:, mi.DZCAP]
        if which == 1:
            skip = mi.prunable(cd["num"][0], cd["den"][0], dz)
        else:
            skip = mi.prunable(cd["num"][1], cd["den"][1], dz) & mi.prunable(cd["num"][2], cd["den"][2], dz)
        fails = (~skip).reshape(-1, mi.WAVE).sum(axis=1)
        kd = np.array(kinds[g.name])
        assert (kd == "all").sum() >= 50 and (kd == "one").sum() >= 50 and (kd == "mixed").sum() >= 50
        assert (fails[kd == "all"] == 0).all() and (fails[kd == "one"] == 1).all() and (fails[kd == "mixed"] == 32).all(), g.name


def test_non_finite_candidates_tiny_dividends_and_the_index_test():
    nonfinite = tiny = differ = 0
    for g, o, cd in census():
        nonfinite += int((~np.isfinite(o["cand"])).any(axis=1).sum())
        mags = [np.abs(g.state[:, mi.GX]), np.abs(g.state[:, mi.GY]), np.abs(cd["a0"])]
        tiny += int(np.any([(m < F(1e-29)) & (m != 0) for m in mags], axis=0).sum())
        differ += int((o["run_geo"] != o["run_full"]).sum())
    print(f"non-finite candidate: {nonfinite}, tiny non-zero dividend: {tiny}, run_geo != run_full: {differ}")
    assert nonfinite >= 1000 and tiny >= 1000 and differ >= 1000


def test_a0_is_never_a_tiny_non_zero_dividend():
    """x + 1e-12f is zero or at least 2^-64 in magnitude: below 2^-41 the sum is exact (Sterbenz), a multiple of the ulp of
    the smaller operand, which is at least 2^-64 for operands that nearly cancel 1e-12f -- so of the three dividends of the
    merged guard of block [C] only the two gradients can be non-zero below 1e-29."""
    rng = np.random.default_rng(3)
    x = -(F(1e-12) * (1 + rng.uniform(-1e-3, 1e-3, 500_000))).astype(F)
    x = np.concatenate([x, mi._neighbours(np.array([-1e-12], F), 2000)])
    a0 = x + F(1e-12)
    nz = np.abs(a0[a0 != 0])
    assert nz.size and nz.min() >= 2.0 ** -64
    for _, _, cd in census():
        m = np.abs(cd["a0"])
        assert not ((m < F(1e-29)) & (m != 0)).any()


def test_threshold_population_straddles_the_constant():
    """The pruning rule of march_steps.py, num > RN(RN(K dzcap) den), over the threshold population: with K = 1.00002f it
    prunes no case whose float quotient is below dzcap.

    The population resolves the boundary of the rule to the ulp: with the largest float below one, K = 1 - 2^-24, the rule
    prunes cases whose float quotient is below dzcap, and K = 1.0f prunes thousands of cases that K = 1.00002f divides.
    K = 1.0f itself prunes no such case, and cannot on any input: RN(K dzcap) = dzcap is then exact, p = RN(dzcap den) is the
    float nearest the exact product x, no float lies strictly between p and x, so num > p gives num >= x, num / den >= dzcap
    and a correctly rounded quotient of at least dzcap.  (The margin K - 1 = 168 x 2^-23 pays for the second rounding only
    when K is not 1; it costs the divisions of the candidates in between.)"""
    below_one = np.nextafter(F(1), F(0))
    wrong, pruned = {}, {}
    for K in (F(1.00002), F(1.0), below_one):
        wrong[K] = pruned[K] = 0
        for g in mi.threshold()[0]:
            cd = mi.candidates(g.state, g.c)
            dz = g.state[:, mi.DZCAP]
            for j in range(3):
                pr = mi.prunable(cd["num"][j], cd["den"][j], dz, K=K)
                pruned[K] += int(pr.sum())
                wrong[K] += int((pr & (cd["quo"][j] < dz)).sum())
    print("pruned:", pruned, "of them with a float quotient below dzcap:", wrong)
    assert pruned[F(1.00002)] > 1000
    assert wrong[F(1.00002)] == 0
    assert wrong[F(1.0)] == 0
    assert pruned[F(1.0)] - pruned[F(1.00002)] >= 1000
    assert wrong[below_one] >= 1


def test_the_exported_step_iterated_is_the_step_of_the_march():
    """march_steps.steps on a BINDING_CASES problem with every integrator step taken by rt_oracle_linear_step: the same count
    of integrator steps, the same winners and the same end state of every ray as with its own numpy statement of the loop --
    and one call per pass of the loop, from the cell entry r = 0 to the step whose run_full is false"""
    p = march_steps.BINDING_CASES["y_dominated"][0]()
    rays = p.build_rays()
    own = march_steps.steps(p, rays, want_state=True)
    exp = march_steps.steps(p, rays, want_state=True, step_fn=lambda st, c: oracle().linear_step(st, c))
    assert own["inner"] == exp["inner"] > 10_000
    assert own["cells"] == exp["cells"] and own["n_exit"] == exp["n_exit"]
    assert np.array_equal(own["winner"], exp["winner"])
    assert np.array_equal(own["end_state"].view(np.uint32), exp["end_state"].view(np.uint32))


def test_entry_state_sampling_leaves_the_counts_alone():
    p = march_steps.BINDING_CASES["weak_wide"][0]()
    rays = p.build_rays()
    a = march_steps.steps(p, rays)
    b = march_steps.steps(p, rays, sample=(500, 3))
    assert set(a) | {"entry_states"} == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert 0 < len(b["entry_states"]) <= 500 and b["entry_states"].shape[1] == 14
    assert (b["entry_states"][:, mi.RX] != 0).any()
    # (x_steep leaves its box with every step: its entry states all have r = 0; the other two hold thousands that have not)
    moved = {g.name: int((g.state[:, mi.RX] != 0).sum()) for g in mi.trajectory()}
    assert all(len(g.state) > 300 for g in mi.trajectory()) and sum(moved.values()) > 10_000, moved


def test_the_setup_and_primitive_populations_hold_what_they_name():
    for s in mi.setup():
        assert len(s.pos) == len(s.cell) == len(s.nc) == len(s.mirror) > 1000
        lo, w, rw = mi.interval_records(s.cell)
        assert (w >= F(1e-12)).all() and (w <= F(1.1e3)).all()
    env = mi.setup()[0]
    lo, w, rw = mi.interval_records(env.cell)
    hk = np.stack([env.cell[:, 1] - env.cell[:, 0], env.cell[:, 3] - env.cell[:, 2]], axis=1)
    assert (w.astype(np.float64) != hk).sum() > 1000                      # widths whose float rounding differs from the double
    assert ((env.mirror != 0) & (env.pos[:, 1] < 0)).sum() > 1000
    assert (env.nc == env.nc[:, :1]).all(axis=1).sum() > 1000             # equal corners
    a, b, y = mi.prim_div_f32()
    assert ((np.abs(a) < F(1e-29)) & (a != 0)).sum() > 1000 and (a == 0).any() and np.signbit(a[a == 0]).any()
    with np.errstate(all="ignore"):
        q = a / b
    assert ((np.abs(q) < F(1.1754944e-38)) & (q != 0)).sum() > 1000       # quotients that land subnormal
    a, b = mi.prim_fdiv_inside()
    ea, eb = np.frexp(a)[1], np.frexp(b)[1]
    assert np.abs(ea - eb).max() == 95 and (np.abs(a) >= 2.0 ** -102).all() and (np.abs(b) < 2.0 ** 126).all()
    assert (np.abs(a) == F(2.0 ** -102)).any() and (np.abs(b) == np.nextafter(F(2.0 ** 126), F(0))).any()
    q = mi.prim_inv_norm()
    for v in (0.9375, 1.0, 1.0625):
        for k in (-64, 64):
            assert (q == (np.array([v], F).view(np.uint32) + np.uint32(k & 0xffffffff)).view(F)[0]).any()
