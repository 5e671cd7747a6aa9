"""Inputs of the unit tests of the march's float32 blocks, shared by the CPU tier (test_march_blocks_host.py) and the device
tier (test_gpu_march_blocks.py).  Every generator has a fixed default_rng seed and is cached: both tiers, and every test of
a tier, see the same arrays (treat them as read-only).

A step case is one row of 14 float32: n0, gx, gy, rx, ry, rz, sx, sy, sz, hsum, w_x, w_y, lim2, dzcap -- the state of a lane
at the entry of block [C] of csrc/rt_march.hip (csrc/rt_march_step.inc), which is what Oracle.linear_step and
Device.march_step take; the step factor c belongs to a launch, so a population is a list of Group(name, c, state).
dzcap = RN(RN(c 1.00001f) lim2) in every case, as block [B] leaves it.

  trajectory()   entry states harvested from march_steps.steps on its three BINDING_CASES: real r != 0 states
  envelope()     log-uniform over the ranges under which the plan selects the short forms (csrc/rt_plan.hip): 0.25 <= n <= 4,
                 |g| in {0} u [1e-30, min(1.3e12, 4.5 / w)] (1.3 dn / w with dn <= 3.75, and |g| w <= 1.2 dn), w in [1e-12, 1e3],
                 lim2 in [1e-18, 1e6], unit s with |sz| >= 0.1, r zero or a fraction of the limits, four step factors
  threshold()    each of h1, h2, h4 within 400 x 2^-23 of dzcap, on a lattice of the quotient's ratio to dzcap and at single ulps
                 around each lattice point, on states in which that candidate is the smallest of the four quotients (so a
                 division skipped wrongly shows in the step); arranged in waves of 64: all lanes prunable / mixed / all but one
  specials()     what the source's comments argue by hand, one group each (see the functions)
  outside()      beyond the envelope, for the generic instance only
  setup()        the cross-cell set-up [B]
  prim_*()       the float and double primitives of csrc/rt_math.h

candidates(state, c) restates the head of the step in numpy float32 (as march_steps.py does) far enough to give the
numerators and denominators of the four quotients: the division-free test of block [C] is evaluated on them."""
import collections
import functools

import numpy as np

F = np.float32
D = np.float64
WAVE = 64
EPS = 2.0 ** -23
K_PRUNE = F(1.00002)
N0, GX, GY, RX, RY, RZ, SX, SY, SZ, HS, WX, WY, LIM2, DZCAP = range(14)
STEP_FACTORS_NAMES = ("c0.5", "c1", "c0.05", "cmin")

Group = collections.namedtuple("Group", "name c state")


def _smallest_c():
    """the smallest float c with RN(c 0.05f) >= 1e-8f (csrc/rt_run_shape.h: the short forms need c_h3 >= 1e-8f)"""
    c = F(1e-8) / F(0.05)
    while F(c * F(0.05)) >= F(1e-8):
        c = np.nextafter(c, F(0))
    while F(c * F(0.05)) < F(1e-8):
        c = np.nextafter(c, F(1))
    return c


C_MIN = _smallest_c()
STEP_FACTORS = (F(0.5), F(1.0), F(0.05), C_MIN)


def c_cap(c):
    return F(F(c) * F(1.00001))


def renorm(sx, sy, sz):
    """the reference's renormalisation (Helper.h:73-89)"""
    q = sx * sx + sy * sy + sz * sz
    inv = (1.0 / np.sqrt(q).astype(D)).astype(F)
    return sx * inv, sy * inv, sz * inv


def unit_s(rng, n, sz_min=0.1):
    """unit vectors with |sz| >= sz_min, renormalised the reference's way: |s|^2 within ulps of 1"""
    sz = rng.uniform(sz_min, 1.0, n) * rng.choice([-1.0, 1.0], n)
    rho = np.sqrt(np.maximum(0.0, 1.0 - sz * sz))
    phi = rng.uniform(0, 2 * np.pi, n)
    return renorm((rho * np.cos(phi)).astype(F), (rho * np.sin(phi)).astype(F), sz.astype(F))


def loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def pack(c, n0, gx, gy, r, s, hs, wx, wy, lim2):
    n = len(np.atleast_1d(lim2))
    st = np.zeros((n, 14), F)
    for col, v in ((N0, n0), (GX, gx), (GY, gy), (RX, r[0]), (RY, r[1]), (RZ, r[2]), (SX, s[0]), (SY, s[1]), (SZ, s[2]), (HS, hs),
                   (WX, wx), (WY, wy), (LIM2, lim2)):
        st[:, col] = np.asarray(v, dtype=F)
    st[:, DZCAP] = c_cap(c) * st[:, LIM2]
    return st


def candidates(state, c):
    """dict(n, a0, t, num [3][m], den [3][m], quo [3][m]) for the pruned candidates h1, h2, h4 of every case, every operation a
    float32 operation in the order of the reference (oracle/rt_oracle.c, linear_step)"""
    st = np.asarray(state, dtype=F)
    c = F(c)
    with np.errstate(all="ignore"):
        n = st[:, N0] + st[:, RX] * st[:, GX] + st[:, RY] * st[:, GY]
        a0 = st[:, SX] * st[:, GX] + st[:, SY] * st[:, GY] + F(1e-12)
        t = a0 / n
        fy = st[:, GY] / n - st[:, SY] * t
        num = [np.full(len(st), c * F(0.1), F), F(1.0001) * (st[:, LIM2] - np.abs(st[:, RZ])), c * F(0.05) * (np.abs(st[:, SY]) + F(5e-4))]
        den = [np.abs(t), np.abs(st[:, SZ]), np.abs(fy) + F(1e-8)]
        quo = [a / b for a, b in zip(num, den)]
    return dict(n=n, a0=a0, t=t, num=num, den=den, quo=quo)


def prunable(num, den, dzcap, K=K_PRUNE):
    """the division-free test of block [C]: num > RN(RN(K dzcap) den)"""
    with np.errstate(all="ignore"):
        return num > (F(K) * dzcap) * den


# ------------------------------------------------------------------------------------------------ trajectory
@functools.lru_cache(maxsize=None)
def trajectory():
    import march_steps
    groups = []
    for name, (make, _, _) in march_steps.BINDING_CASES.items():
        p = make()
        res = march_steps.steps(p, p.build_rays(), sample=(60_000, 7))
        groups.append(Group(f"trajectory/{name}", F(0.5), res["entry_states"]))
    return tuple(groups)


# ------------------------------------------------------------------------------------------------ envelope
@functools.lru_cache(maxsize=None)
def envelope(n_per_c=48_000 + 37):
    rng = np.random.default_rng(20240611)
    groups = []
    for label, c in zip(STEP_FACTORS_NAMES, STEP_FACTORS):
        n = n_per_c
        wx, wy = loguniform(rng, 1e-12, 1e3, n).astype(F), loguniform(rng, 1e-12, 1e3, n).astype(F)
        g = []
        for w in (wx, wy):
            hi = np.minimum(1.3e12, 4.5 / w.astype(D))
            mag = np.exp(rng.uniform(np.log(1e-30), np.log(hi)))
            mag = np.where(rng.random(n) < 0.1, 0.0, mag)
            # (a tenth at the largest gradient the widths allow)
            mag = np.where(rng.random(n) < 0.1, hi, mag)
            g.append((mag * rng.choice([-1.0, 1.0], n)).astype(F))
        lim2 = loguniform(rng, 1e-18, 1e6, n).astype(F)
        zero_r = rng.random(n) < 0.3
        fr = rng.uniform(-1.0, 1.0, (3, n))
        r = [np.where(zero_r, 0.0, fr[0] * 0.1 * wx).astype(F), np.where(zero_r, 0.0, fr[1] * 0.1 * wy).astype(F),
             np.where(zero_r, 0.0, fr[2] * lim2).astype(F)]
        # keep |r| strictly inside the limits as a lane that stays in [C] has it
        lim0, lim1 = F(0.1) * wx, F(0.1) * wy
        r[0] = np.where(np.abs(r[0]) < lim0, r[0], F(0))
        r[1] = np.where(np.abs(r[1]) < lim1, r[1], F(0))
        r[2] = np.where(np.abs(r[2]) < lim2, r[2], F(0))
        n_t = loguniform(rng, 0.25, 4.0, n)
        delta = r[0].astype(D) * g[0] + r[1].astype(D) * g[1]
        n0 = (n_t - delta).astype(F)
        seen = n0 + r[0] * g[0] + r[1] * g[1]
        bad = ~((n0 >= 0.25) & (n0 <= 4.0) & (seen >= 0.25) & (seen <= 4.0))
        n0 = np.where(bad, n_t.astype(F), n0)
        r[0], r[1] = np.where(bad, F(0), r[0]), np.where(bad, F(0), r[1])
        s = unit_s(rng, n)
        hs = (rng.uniform(0, 3, n) * lim2).astype(F)
        groups.append(Group(f"envelope/{label}", c, pack(c, n0, g[0], g[1], r, s, hs, wx, wy, lim2)))
    return tuple(groups)


# ------------------------------------------------------------------------------------------------ threshold
LATTICE = np.arange(-400, 401, 4)
MOVES = np.arange(-2, 3)


def _threshold_bases(which, rng, n):
    """states in which candidate `which` (1, 2, 4) is the smallest of the four quotients whatever dzcap is: r = 0, the
    other three candidates far above it (module docstring)"""
    n0 = rng.uniform(0.5, 3.0, n).astype(F)
    sign = rng.choice([-1.0, 1.0], (3, n))
    z = np.zeros(n, F)
    if which == 1:
        # gradient along x, sx^2 > 2/3 and no y component: h3 / h1 = 0.5 sx^2 / (1 - sx^2) > 1, h4 = 2500 c
        sx = rng.uniform(0.85, 0.99, n)
        s = renorm((sign[0] * sx).astype(F), z, (sign[2] * np.sqrt(1 - sx * sx)).astype(F))
        g = (loguniform(rng, 1e-2, 1e3, n) * sign[1]).astype(F)
        return n0, g, z, s
    if which == 4:
        # gradient along y, sy^2 < 1/2: h4 below h1 (sy^2 < 2/3) and below h3 (sy^2 < 1 - sy^2)
        sy = rng.uniform(0.25, 0.65, n)
        rest = np.sqrt(1 - sy * sy)
        sz = rng.uniform(0.3, 0.9, n) * rest
        sx = np.sqrt(np.maximum(0.0, rest * rest - sz * sz))
        s = renorm((sign[0] * sx).astype(F), (sign[1] * sy).astype(F), (sign[2] * sz).astype(F))
        g = (loguniform(rng, 1e-2, 1e3, n) * rng.choice([-1.0, 1.0], n)).astype(F)
        return n0, z, g, s
    # h2: no gradient, so h1 = 0.1 c n / 1e-12 and h3, h4 >= 2500 c while h2 is about lim2 <= 1
    return n0, z, z, unit_s(rng, n, 0.2)


def _threshold_pool(which, c, rng, n_base):
    n0, gx, gy, s = _threshold_bases(which, rng, n_base)
    wx = wy = np.full(n_base, 10.0, F)
    idx = np.repeat(np.arange(n_base), len(LATTICE))
    k = np.tile(LATTICE, n_base).astype(D)
    n0, gx, gy, s, wx, wy = n0[idx], gx[idx], gy[idx], [v[idx] for v in s], wx[idx], wy[idx]
    m = len(idx)
    z = np.zeros(m, F)
    cc = D(c_cap(c))
    if which == 2:
        # 1.0001f (lim2 - |rz|) / |sz| = (1 + k eps) c_cap lim2, solved for rz in double; the single ulps are those of rz, which
        # move the numerator by at least as much
        lim2 = loguniform(rng, 1e-6, 1.0, n_base).astype(F)[idx]
        rz = lim2.astype(D) * (1.0 - np.abs(s[2]).astype(D) * cc * (1.0 + k * EPS) / D(F(1.0001)))
        rz = (rz * rng.choice([-1.0, 1.0], n_base)[idx]).astype(F)
        out = []
        for mv in MOVES:
            r2 = rz.copy()
            for _ in range(abs(mv)):
                r2 = np.nextafter(r2, np.where(r2 < 0, F(-np.inf), F(np.inf)) if mv > 0 else F(0)).astype(F)
            out.append(pack(c, n0, gx, gy, (z, z, r2), s, z, wx, wy, lim2))
        return np.concatenate(out)
    # h1, h4: the numerator is a constant of the launch (c 0.1f) or a function of s; the quotient stays and dzcap moves:
    # lim2 = quotient / ((1 + k eps) c_cap) in double, then lim2 by single ulps (one ulp of lim2 is one ulp of dzcap)
    probe = pack(c, n0, gx, gy, (z, z, z), s, z, wx, wy, np.ones(m, F))
    cd = candidates(probe, c)
    j = {1: 0, 4: 2}[which]
    quo = cd["num"][j].astype(D) / cd["den"][j].astype(D)
    lim2 = (quo / ((1.0 + k * EPS) * cc)).astype(F)
    out = []
    for mv in MOVES:
        l2 = lim2.copy()
        for _ in range(abs(mv)):
            l2 = np.nextafter(l2, F(np.inf) if mv > 0 else F(0)).astype(F)
        out.append(pack(c, n0, gx, gy, (z, z, z), s, z, wx, wy, l2))
    return np.concatenate(out)


def _waves(pool, can_skip, rng, n_each=64):
    """Arranges cases in waves of 64: n_each waves whose lanes all pass the division-free test, n_each in which exactly one lane
    (at a random place) fails it, the rest mixed, in turn.  Every case is used at most once."""
    A, B = list(rng.permutation(np.flatnonzero(can_skip))), list(rng.permutation(np.flatnonzero(~can_skip)))
    order, kinds = [], []
    for w in range(n_each):
        if len(A) < 2 * WAVE + 32 or len(B) < 33:
            break
        order += [A.pop() for _ in range(WAVE)]
        kinds.append("all")
        mixed = [A.pop() for _ in range(32)] + [B.pop() for _ in range(32)]
        order += list(rng.permutation(mixed))
        kinds.append("mixed")
        one = [A.pop() for _ in range(WAVE - 1)]
        one.insert(int(rng.integers(0, WAVE)), B.pop())
        order += one
        kinds.append("one")
    rest = list(rng.permutation(A + B))
    rest = rest[:len(rest) // WAVE * WAVE]
    order += rest
    kinds += ["rest"] * (len(rest) // WAVE)
    return pool[np.array(order)], kinds


@functools.lru_cache(maxsize=None)
def threshold():
    """Groups threshold/h1, /h2, /h4 at c = 1 and c = 0.5 alternately -> (groups, {name: wave kinds})"""
    rng = np.random.default_rng(777)
    groups, kinds = [], {}
    for which, c, n_base in ((1, F(0.5), 52), (2, F(1.0), 52), (4, F(0.5), 52)):
        pool = _threshold_pool(which, c, rng, n_base)
        cd = candidates(pool, c)
        skip_h1 = prunable(cd["num"][0], cd["den"][0], pool[:, DZCAP])
        skip_h24 = prunable(cd["num"][1], cd["den"][1], pool[:, DZCAP]) & prunable(cd["num"][2], cd["den"][2], pool[:, DZCAP])
        state, kd = _waves(pool, skip_h1 if which == 1 else skip_h24, rng)
        name = f"threshold/h{which}"
        groups.append(Group(name, c, state))
        kinds[name] = kd
    return tuple(groups), kinds


# ------------------------------------------------------------------------------------------------ specials
def _benign(rng, n, c):
    """a state well inside every range: the specials change one thing of it each"""
    wx, wy = loguniform(rng, 1e-4, 1.0, n).astype(F), loguniform(rng, 1e-4, 1.0, n).astype(F)
    return dict(n0=rng.uniform(0.5, 3.0, n).astype(F), gx=(rng.uniform(-3, 3, n)).astype(F), gy=(rng.uniform(-3, 3, n)).astype(F),
                r=[np.zeros(n, F)] * 3, s=list(unit_s(rng, n)), hs=np.zeros(n, F), wx=wx, wy=wy,
                lim2=loguniform(rng, 1e-6, 1.0, n).astype(F))


def _grp(name, c, b):
    return Group(f"specials/{name}", c, pack(c, b["n0"], b["gx"], b["gy"], b["r"], b["s"], b["hs"], b["wx"], b["wy"], b["lim2"]))


def _subnormals(rng, n):
    return (rng.integers(1, 1 << 23, n).astype(np.uint32)).view(F)


@functools.lru_cache(maxsize=None)
def specials():
    rng = np.random.default_rng(4242)
    c = F(0.5)
    out = []
    n = 1024 + 5

    # a medium without refraction
    b = _benign(rng, n, c)
    b["gx"] = b["gy"] = np.zeros(n, F)
    out.append(_grp("zero_gradient", c, b))

    # sx gx + sy gy == -1e-12f exactly: a0 = +0, t = 0, h1 = c 0.1f / 0.  Products of a power of two with RN(1e-12) are exact.
    n = 2048 + 11
    b = _benign(rng, n, c)
    e12 = F(1e-12)
    kind = rng.integers(0, 4, n)
    p = 2.0 ** rng.integers(1, 4, n)                                   # 2, 4, 8
    sx = np.where(kind == 0, -1.0 / p, np.where(kind == 2, -0.5, np.where(kind == 3, 0.5, 0.0)))
    sy = np.where(kind == 1, -1.0 / p, np.where(kind == 2, -0.5, np.where(kind == 3, -0.25, 0.0)))
    gx = np.where(kind == 0, p * D(e12), np.where(kind == 2, D(e12), np.where(kind == 3, 2 * D(e12), 0.0)))   # kind 3: e12 - 2 e12
    gy = np.where(kind == 1, p * D(e12), np.where(kind == 2, D(e12), np.where(kind == 3, 8 * D(e12), 0.0)))
    sz = np.sqrt(1.0 - sx * sx - sy * sy) * rng.choice([-1.0, 1.0], n)
    b["s"] = [sx.astype(F), sy.astype(F), sz.astype(F)]                # (|s|^2 within ulps of 1; not renormalised: sx, sy stay exact)
    b["gx"], b["gy"] = gx.astype(F), gy.astype(F)
    out.append(_grp("a0_zero", c, b))

    # |gx| or |gy| non-zero below 1e-29, subnormals included, alone and next to exact zeros in the same wave
    n = 4096 + 29
    b = _benign(rng, n, c)
    tiny = np.where(rng.random(n) < 0.3, _subnormals(rng, n), loguniform(rng, 1.2e-38, 1e-29, n).astype(F)) * rng.choice([-1, 1], n).astype(F)
    tiny2 = np.where(rng.random(n) < 0.3, _subnormals(rng, n), loguniform(rng, 1.2e-38, 1e-29, n).astype(F)) * rng.choice([-1, 1], n).astype(F)
    edge = np.array([1e-29, np.nextafter(F(1e-29), F(0)), np.nextafter(F(1e-29), F(1)), 1.4e-45, 1.1754942e-38, 1.17549435e-38], F)
    tiny[:len(edge)] = edge
    kind = rng.integers(0, 6, n)
    b["gx"] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [tiny, np.zeros(n, F), tiny, b["gx"], tiny], np.zeros(n, F)).astype(F)
    b["gy"] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [np.zeros(n, F), tiny, tiny2, tiny, b["gy"]], np.zeros(n, F)).astype(F)
    out.append(_grp("tiny_gradient", c, b))

    # |sz| from 0.1 down through 2^-78 to subnormal and zero
    n = 2048 + 3
    b = _benign(rng, n, c)
    mag = np.concatenate([[0.1, 2.0 ** -78, 2.0 ** -79, 2.0 ** -100, 2.0 ** -126, 2.0 ** -127, 2.0 ** -149, 0.0],
                          loguniform(rng, 1e-45, 0.1, n - 8)]).astype(F)
    sz = mag * rng.choice([-1, 1], n).astype(F)
    phi = rng.uniform(0, 2 * np.pi, n)
    rho = np.sqrt(1.0 - sz.astype(D) ** 2)
    b["s"] = list(renorm((rho * np.cos(phi)).astype(F), (rho * np.sin(phi)).astype(F), sz))
    out.append(_grp("small_sz", c, b))

    # lim2 - |rz| zero and negative
    n = 1024 + 7
    b = _benign(rng, n, c)
    l2 = b["lim2"]
    kind = rng.integers(0, 4, n)
    rz = np.select([kind == 0, kind == 1, kind == 2], [l2, np.nextafter(l2, F(np.inf)), F(2) * l2], l2 * rng.uniform(1.0, 1.5, n).astype(F))
    b["r"] = [np.zeros(n, F), np.zeros(n, F), (rz * rng.choice([-1, 1], n)).astype(F)]
    out.append(_grp("h2_numerator_not_positive", c, b))

    # fx or fy exactly zero: no gradient and no direction component along that axis
    n = 1024 + 13
    b = _benign(rng, n, c)
    kind = rng.integers(0, 3, n)
    sx, sy, sz = b["s"]
    sx = np.where(kind != 1, F(0), sx)
    sy = np.where(kind != 0, F(0), sy)
    b["s"] = list(renorm(sx, sy, sz))
    b["gx"] = np.where(kind != 1, F(0), b["gx"])
    b["gy"] = np.where(kind != 0, F(0), b["gy"])
    out.append(_grp("f_zero", c, b))

    # |s|^2 = q with an all-ones root significand (q just below 1); no refraction, so the step leaves s as it is
    m = 100_000
    s = unit_s(rng, m)
    shrink = rng.choice(np.array([1.0 - 2.0 ** -24, 1.0 - 2.0 ** -23, 1.0 - 2.0 ** -22], F), m)
    s = [v * shrink for v in s]
    q = s[0] * s[0] + s[1] * s[1] + s[2] * s[2]
    ones = (np.sqrt(q).view(np.uint32) & 0x7fffff) == 0x7fffff
    pick = np.flatnonzero(ones)[:2048 + 17]
    b = _benign(rng, len(pick), c)
    b["gx"] = b["gy"] = np.zeros(len(pick), F)
    b["s"] = [v[pick] for v in s]
    out.append(_grp("all_ones_root", c, b))

    # |s|^2 outside [0.9375, 1.0625): the general branch of inv_norm, in waves that also hold lanes inside
    n = 2048 + 19
    b = _benign(rng, n, c)
    scale = rng.choice(np.array([1.0, 0.5, 0.9, 0.968, 0.9682458, 0.96825, 1.0307, 1.0307764, 1.031, 1.1, 2.0]), n).astype(F)
    b["s"] = [v * scale for v in b["s"]]
    out.append(_grp("inv_norm_general", c, b))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ outside
@functools.lru_cache(maxsize=None)
def outside():
    """beyond the ranges of the short forms: for the generic instance only"""
    rng = np.random.default_rng(99)
    c = F(0.5)
    out = []
    n = 4096 + 21
    b = _benign(rng, n, c)
    b["n0"] = loguniform(rng, 1e-6, 0.25, n).astype(F)
    out.append(Group("outside/n_low", c, _grp("", c, b).state))
    b = _benign(rng, n, c)
    b["n0"] = loguniform(rng, 4.0, 1e6, n).astype(F)
    b["n0"][0] = F(1e6)
    out.append(Group("outside/n_high", c, _grp("", c, b).state))
    b = _benign(rng, n, c)
    b["gx"] = (loguniform(rng, 1e12, 1e30, n) * rng.choice([-1, 1], n)).astype(F)
    b["gy"] = np.where(rng.random(n) < 0.5, b["gy"], (loguniform(rng, 1e12, 1e30, n) * rng.choice([-1, 1], n)).astype(F))
    out.append(Group("outside/steep", c, _grp("", c, b).state))
    b = _benign(rng, 512 + 5, c)
    b["n0"] = np.full(512 + 5, np.nan, F)
    out.append(Group("outside/n_nan", c, _grp("", c, b).state))
    b = _benign(rng, 512 + 5, c)
    b["n0"] = (np.inf * rng.choice([-1, 1], 512 + 5)).astype(F)
    out.append(Group("outside/n_inf", c, _grp("", c, b).state))
    return tuple(out)


def inside_groups():
    """every population the four instances must agree on"""
    return trajectory() + envelope() + threshold()[0] + specials()


# ------------------------------------------------------------------------------------------------ the cross-cell set-up
Setup = collections.namedtuple("Setup", "name pos cell nc mirror")


def _neighbours(x, k=2):
    """x and its k float neighbours on either side"""
    out = [x]
    up = down = x
    for _ in range(k):
        up, down = np.nextafter(up, F(np.inf)), np.nextafter(down, F(-np.inf))
        out += [up, down]
    return np.concatenate(out)


def _setup_geometry(rng, n, mirror=None):
    """cells of width 1e-12 .. 1e3 whose lower corner lies within 100 widths of the origin (so that a float position
    resolves the cell; mirror: at y >= 0), positions at u, v in {0, 1, -0.1, 1.1, random} and their float neighbours"""
    hk = loguniform(rng, 1e-12, 1e3, (n, 2))
    lo = hk * np.where(rng.random((n, 2)) < 0.3, 0.0, rng.integers(-100, 101, (n, 2)).astype(D) + rng.random((n, 2)))
    if mirror is not None:
        lo[:, 1] = np.where(mirror, np.abs(lo[:, 1]), lo[:, 1])
    hi = lo + hk
    hk = hi - lo                                                        # the width as the plan computes it
    edge = rng.choice(np.array([0.0, 1.0, -0.1, 1.1, np.nan]), (n, 2))
    uv = np.where(np.isnan(edge), rng.uniform(-0.1, 1.1, (n, 2)), edge)
    pos = (lo + uv * hk).astype(F)
    step = rng.integers(-2, 3, (n, 2))
    for _ in range(2):
        pos = np.where(step > 0, np.nextafter(pos, F(np.inf)), np.where(step < 0, np.nextafter(pos, F(-np.inf)), pos)).astype(F)
        step = step - np.sign(step)
    return pos, np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1]], axis=1), hk


@functools.lru_cache(maxsize=None)
def setup():
    rng = np.random.default_rng(31337)
    out = []

    def corners(base, d):
        return base[:, None] + d

    # corner differences from 0 to the envelope's largest (dn <= 3.75, dn / w <= 1e12), equal corners included
    n = 60_000 + 41
    mirror = rng.random(n) < 0.5
    pos, cell, hk = _setup_geometry(rng, n, mirror)
    dn_max = np.minimum(3.0, 1e12 * hk.min(axis=1))
    d = loguniform(rng, 1e-17, 1.0, (n, 4)) * dn_max[:, None] * rng.choice([-1.0, 1.0], (n, 4))
    d[rng.random((n, 4)) < 0.15] = 0.0
    d[rng.random(n) < 0.05] = 0.0                                        # equal corners
    base = rng.uniform(0.5, 3.5, n)
    nc = np.clip(base[:, None] + d, 0.25, 4.0)
    # mirrored: the cell lies at y >= 0 and the ray on either side of y = 0
    flip = mirror & (rng.random(n) < 0.5)
    pos[:, 1] = np.where(flip, -pos[:, 1], pos[:, 1])
    out.append(Setup("setup/envelope", pos, cell, nc, mirror.astype(np.uint8)))

    # corner differences down to 1e-300 and below (dividends below 1e-280, double subnormals included): indices next to 0
    n = 20_000 + 9
    pos, cell, hk = _setup_geometry(rng, n)
    d = loguniform(rng, 1e-323, 1e-250, (n, 4)) * rng.choice([-1.0, 1.0], (n, 4))
    d[rng.random((n, 4)) < 0.2] = 0.0
    out.append(Setup("setup/tiny_differences", pos, cell, d, (rng.random(n) < 0.3).astype(np.uint8)))

    # ... whose two quotients nearly cancel in the sum: v = 0.5 exactly, n10 - n00 = X, n11 - n01 = -X (1 + j 2^-52) or X's
    # neighbours in the subnormal range
    n = 8192 + 5
    pos, cell, hk = _setup_geometry(rng, n)
    cell[:, 2], cell[:, 3] = 0.0, 2.0 ** rng.integers(-30, 8, n).astype(D)
    pos[:, 1] = (0.5 * cell[:, 3]).astype(F)
    X = loguniform(rng, 1e-322, 1e-285, n)
    Y = X.copy()
    for _ in range(3):
        Y = np.where(rng.random(n) < 0.5, np.nextafter(Y, np.inf), Y)
    nc = np.stack([np.zeros(n), X, np.zeros(n), -Y], axis=1)           # dnx0 = X, dnx1 = -Y
    out.append(Setup("setup/tiny_cancelling", pos, cell, nc, np.zeros(n, np.uint8)))
    return tuple(out)


def interval_records(cell):
    """(lo [n][2], w [n][2] float32, rw [n][2]) of the cells as rt_plan.hip packs an interval: hk = hi - lo, w = (float) hk,
    rw = 1.0 / (double) (float) hk"""
    lo = np.stack([cell[:, 0], cell[:, 2]], axis=1)
    hk = np.stack([cell[:, 1] - cell[:, 0], cell[:, 3] - cell[:, 2]], axis=1)
    w = hk.astype(F)
    return lo, w, 1.0 / w.astype(D)


# ------------------------------------------------------------------------------------------------ primitives
def _f32_bits(u):
    return np.asarray(u, dtype=np.uint32).view(F)


def _pow2(lo, hi):
    return (2.0 ** np.arange(lo, hi + 1, dtype=D)).astype(F)


@functools.lru_cache(maxsize=None)
def prim_div_f32():
    """(a, b, y = RN(1 / b)) for the float div_by_recip forms: divisors an index of refraction in [0.25, 4] or one of the
    constants 3, 6, 12 of the integrator step; dividends +-0, subnormal, tiny ones straddling 1e-29, powers of two, any
    normal, and those whose quotient lands subnormal"""
    rng = np.random.default_rng(11)
    e29 = F(1e-29)
    a = [np.array([0.0, -0.0], F), _subnormals(rng, 4000), loguniform(rng, 1e-38, 1e-25, 8000).astype(F), _neighbours(np.array([e29]), 40),
         _pow2(-149, 120), _f32_bits(rng.integers(0x00800000, 0x7d000000, 40000)),    # (no quotient overflows)
         loguniform(rng, 1.2e-38, 4.5e-38, 4000).astype(F)]
    a = np.concatenate(a)
    a = np.concatenate([a, -a])
    b = np.where(rng.random(a.size) < 0.2, rng.choice(np.array([3.0, 6.0, 12.0, 0.25, 0.5, 1.0, 2.0, 4.0], F), a.size),
                 loguniform(rng, 0.25, 4.0, a.size).astype(F)).astype(F)
    return a, b, (F(1) / b).astype(F)


@functools.lru_cache(maxsize=None)
def prim_div_f64():
    """(a, b, y = RN(1 / b)) for the double div_by_recip forms: divisors a cell width (float-valued, 1e-12 .. 1e3, as the
    cross-cell set-up divides); dividends +-0, subnormal, tiny ones straddling 1e-280, powers of two, any normal"""
    rng = np.random.default_rng(12)
    sub = rng.integers(1, 1 << 52, 4000).astype(np.uint64).view(D)
    a = [np.array([0.0, -0.0]), sub, loguniform(rng, 1e-307, 1e-270, 8000), np.array([1e-280, np.nextafter(1e-280, 0), np.nextafter(1e-280, 1)]),
         2.0 ** np.arange(-1074, 1000, 7, dtype=D), loguniform(rng, 1e-200, 1e200, 40000)]
    a = np.concatenate(a)
    a = np.concatenate([a, -a])
    b = loguniform(rng, 1e-12, 1e3, a.size).astype(F).astype(D)
    b[::17] = 2.0 ** rng.integers(-39, 10, len(b[::17]))
    return a, b, 1.0 / b


def _pair(ea, eb, rng):
    n = len(ea)
    ma, mb = rng.integers(0, 1 << 23, n), rng.integers(0, 1 << 23, n)
    first = rng.random(n) < 0.2                                           # a fifth with the smallest significands: the limits exactly
    ma, mb = np.where(first, 0, ma), np.where(first, 0, mb)
    return _f32_bits(((ea + 127) << 23) | ma), _f32_bits(((eb + 127) << 23) | mb)


@functools.lru_cache(maxsize=None)
def prim_fdiv_inside():
    """pairs inside the envelope the comment of fdiv_nr states: normal operands whose exponents differ by less than 96, a
    dividend of at least 2^-102, a divisor below 2^126, a normal quotient -- the limits of the distance, the dividend and the divisor hit exactly"""
    rng = np.random.default_rng(13)
    n = 120_000
    ea = rng.integers(-102, 128, n)
    eb = np.clip(ea + rng.integers(-95, 96, n), -126, 125)
    edge = rng.random(n) < 0.2                                            # the exponent distance at its limit, either way
    eb = np.where(edge, np.clip(ea + rng.choice([-95, 95], n), -126, 125), eb)
    a, b = _pair(ea, eb, rng)
    with np.errstate(all="ignore"):
        q = a.astype(D) / b.astype(D)
    keep = (np.abs(ea - eb) <= 95) & (q >= 2.0 ** -126) & (q < 2.0 ** 128)
    a, b = a[keep], b[keep]
    # the limits themselves: quotient 2^-126, dividend 2^-102, divisor just below 2^126, distance 95
    # (a normal quotient follows from the other limits: a >= 2^-102 and a distance below 96 keep it within 2^-96 .. 2^96)
    xa = np.array([2.0 ** -102, 2.0 ** -102, 2.0 ** -31, 2.0 ** 30, 2.0 ** 127, 2.0 ** 30], F)
    xb = np.array([2.0 ** -126, 2.0 ** -7, 2.0 ** 64, np.nextafter(F(2.0 ** 126), F(0)), 2.0 ** 32, 2.0 ** -65], F)
    sign = rng.choice([-1, 1], (2, len(a) + len(xa))).astype(F)
    return np.concatenate([a, xa]) * sign[0], np.concatenate([b, xb]) * sign[1]


@functools.lru_cache(maxsize=None)
def prim_fdiv_outside():
    """Pairs outside that envelope in the ways the integrator step can leave it.  Its numerators are normal and at most
    about 1e6 (c 0.1f, c 0.05f (|s| + 5e-4f), 1.0001f (lim2 - |rz|)); its divisors |t|, |sz|, |f| + 1e-8f are bounded above by
    the gradients (1e13) but not below: a divisor that is zero, subnormal, or more than 2^95 below the dividend.  Positive
    operands."""
    rng = np.random.default_rng(14)
    n = 20_000
    a = loguniform(rng, 1e-30, 1e7, n).astype(F)
    kind = rng.integers(0, 3, n)
    far = (a.astype(D) * 2.0 ** -rng.uniform(96, 150, n))
    b = np.select([kind == 0, kind == 1], [np.zeros(n), _subnormals(rng, n).astype(D)], far).astype(F)
    return a, b


@functools.lru_cache(maxsize=None)
def prim_fdiv_one():
    """divisors of fdiv_one_nr inside the envelope (2^-96 < b < 2^96 for the dividend 1), the limits included"""
    rng = np.random.default_rng(15)
    e = rng.integers(-95, 96, 60_000)
    _, b = _pair(e, e, rng)
    b = np.concatenate([b, loguniform(rng, 0.25, 4.0, 20_000).astype(F), _pow2(-95, 95)])
    return b * rng.choice([-1, 1], b.size).astype(F)


@functools.lru_cache(maxsize=None)
def prim_fmin():
    """every ordered pair of a set that holds NaNs of both signs, +-0, +-inf, subnormals and ordinary numbers"""
    v = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 1.4e-45, -1.4e-45, 1.0, -1.0, 3.5, 1e-30, 1e30, -1e30, 3.4028235e38], F)
    v = np.concatenate([v, _f32_bits([0x7fc00001, 0xffc12345])])               # quiet NaNs with payloads
    a, b = np.meshgrid(v, v)
    return a.reshape(-1).copy(), b.reshape(-1).copy()


@functools.lru_cache(maxsize=None)
def prim_inv_norm():
    """q: every float within 64 ulp of 0.9375, 1 and 1.0625; all-ones roots; 0, subnormal, inf, NaN and negative arguments;
    random ones inside the shortcut's range and anywhere"""
    rng = np.random.default_rng(16)
    near = np.concatenate([_neighbours(np.array([v], F), 64) for v in (0.9375, 1.0, 1.0625)])
    # all-ones roots: the floats q whose correctly rounded root has the significand 0x7fffff, over 20 binades
    root = _f32_bits((np.arange(117, 137, dtype=np.uint32) << 23) | 0x7fffff)
    sq = (root.astype(D) ** 2).astype(F)
    cand = _neighbours(sq, 3)
    ones = cand[(np.sqrt(cand).view(np.uint32) & 0x7fffff) == 0x7fffff]
    inside = rng.uniform(0.9375, 1.0625, 60_000).astype(F)
    ones_in = inside[(np.sqrt(inside).view(np.uint32) & 0x7fffff) == 0x7fffff]
    edge = np.array([0.0, -0.0, 1.4e-45, 1e-40, 1.1754944e-38, np.inf, -np.inf, np.nan, -1.0, -1e-30, 3.4028235e38], F)
    wide = loguniform(rng, 1e-44, 3e38, 30_000).astype(F)
    return np.concatenate([near, ones, ones_in, inside, edge, wide, _subnormals(rng, 2000)])
