"""Inputs of the device-math tests, shared by the CPU tier (test_devmath_host.py) and the device tier
(test_gpu_devmath.py).  Every generator has a fixed default_rng seed and is cached: both tiers, and every test of a
tier, see the same arrays (treat them as read-only).

Exponent arguments are built around the range reduction of rt_freq.hip: x = (256 m + j) ln2/256 + r with every table
index j, both signs of m and r in {0, just inside +-ln2/512, random}; plus arguments whose x 256/ln2 lies within a few
ulp of a half-integer (where rint must break the tie the same way everywhere), tiny arguments, and the edges of the
double range.  Array lengths end in a ragged last work-group (len mod 256 == 3)."""
import functools
import math

import numpy as np

LN2_256 = math.log(2.0) / 256.0
HALF = 0.4999 * LN2_256                      # "just inside" +-ln2/512
WORST_VEC = -502.54930561685239               # where the host restatement of exp_tab_vec was first seen beyond 2 ulp
FLT_MAX = float(np.finfo(np.float32).max)

EXP_EDGES = np.array([0.0, -0.0, 709.78, 709.782712893384, 709.79, -708.4, -745.13, -745.14, 1100.0, -1100.0,
                      1e308, -1e308, np.inf, -np.inf, np.nan, WORST_VEC])
LAUNCH_SIZES = (1, 63, 65)                    # besides the whole array: one thread, a ragged wave, one wave + 1


def ragged(a, fill=0.0):
    """a, padded with `fill` until len mod 256 == 3: the last work-group of a launch is ragged."""
    pad = (3 - len(a)) % 256
    return np.concatenate([a, np.full(pad, fill, dtype=a.dtype)])


def _lattice(m_lo, m_hi, n_rand, rng):
    """(256 m + j) ln2/256 + r for every j, m in [m_lo, m_hi], r in {0, +HALF, -HALF, n_rand random in (-HALF, HALF)}"""
    m = np.arange(m_lo, m_hi + 1, dtype=np.float64)
    j = np.arange(256, dtype=np.float64)
    base = ((256.0 * m[:, None] + j[None, :]) * LN2_256).reshape(-1)
    parts = [base, base + HALF, base - HALF]
    for _ in range(n_rand):
        parts.append(base + rng.uniform(-HALF, HALF, base.size))
    return np.concatenate(parts)


def _ties(k_max, n, rng, dtype):
    """arguments with x 256/ln2 within a few ulp (of dtype) of a half-integer"""
    k = rng.integers(-k_max, k_max, n).astype(np.float64)
    x = ((k + 0.5) * LN2_256).astype(dtype)
    out = [x]
    up, down = x, x
    for _ in range(3):
        up = np.nextafter(up, dtype(np.inf))
        down = np.nextafter(down, dtype(-np.inf))
        out += [up, down]
    return np.concatenate(out).astype(np.float64)


def _tiny(n, rng):
    mag = 10.0 ** rng.uniform(-44.0, -2.0, n)
    edge = np.array([HALF, LN2_256 / 2, np.nextafter(LN2_256 / 2, 0.0), 1e-44, 1e-2, 1e-3])
    mag = np.concatenate([mag, edge])
    return np.concatenate([mag, -mag])


@functools.lru_cache(maxsize=None)
def exp_args():
    """float64 arguments of exp_tab / exp_tab_vec: m over the whole double range and beyond both ends (2.7 M of the
    lattice), ties, the worst point of the vector form, tiny arguments, the edges."""
    rng = np.random.default_rng(101)
    x = np.concatenate([EXP_EDGES, _lattice(-1080, 1024, 2, rng), _ties(270_000, 20_000, rng, np.float64),
                        _tiny(20_000, rng)])
    return ragged(x)


@functools.lru_cache(maxsize=None)
def step_args(limit):
    """float32 arguments x = gs * w of a step form with |x| <= limit (708: ase_step, 80: ase_step_f32), as float32: the
    lattice rounded to float (ulp(700) = 6e-5 against ln2/256 = 2.7e-3: still every j and both halves of the reduced
    range), float ties, tiny floats down to the denormals, +-0 and +-limit.  Length a multiple of VEC = 4 and ragged."""
    rng = np.random.default_rng(202 + int(limit))
    m_max = int(limit / math.log(2.0)) + 1
    n_rand = 2 if limit > 100 else 20
    x = np.concatenate([np.array([0.0, -0.0, limit, -limit, WORST_VEC if limit > 600 else -limit / 3]),
                        _lattice(-m_max, m_max, n_rand, rng),
                        _ties(int(limit / LN2_256) - 1, 20_000, rng, np.float32), _tiny(20_000, rng)])
    x = x.astype(np.float32)
    x = x[np.abs(x) <= np.float32(limit)]
    x = ragged(x, np.float32(0.0))
    return np.concatenate([x, np.zeros((-len(x)) % 4, np.float32)])      # 259 -> 260: whole groups, still ragged


def _signed_log(rng, n, lo, hi):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)


@functools.lru_cache(maxsize=None)
def step_general_args(limit):
    """(Iv [4 g], gs [g], rs [g], w [4 g]) for a step form with |gs w| <= limit: Iv in {0, 10^[-300, 300]}, both signs of
    gs, es >= 0 (rs = es / gs), w in [2e-3, 1] and negative."""
    rng = np.random.default_rng(303 + int(limit))
    g = 100_000
    gs = _signed_log(rng, g, -6.0, math.log10(limit)).astype(np.float32)
    gs = np.where(np.abs(gs) > np.float32(limit), np.float32(limit), gs).astype(np.float32)
    es = (np.abs(gs.astype(np.float64)) * 10.0 ** rng.uniform(-8.0, 2.0, g)).astype(np.float32)
    es[rng.random(g) < 0.1] = 0.0
    rs = es.astype(np.float64) / gs.astype(np.float64)
    w = rng.uniform(2e-3, 1.0, 4 * g).astype(np.float32)
    w[rng.random(4 * g) < 0.15] *= np.float32(-1.0)
    Iv = 10.0 ** rng.uniform(-300.0, 300.0, 4 * g)
    Iv[rng.random(4 * g) < 0.2] = 0.0
    return Iv, gs, rs, w


@functools.lru_cache(maxsize=None)
def update_args():
    """(Iv, gs, es, w) of ase_update: general cases with |gs w| up to 750 (beyond the range of exp), then the blocks the
    CPU's branch depends on: every float within 300 ulp of +-1e-3 (as gs w with gs = 1, and as a product of two
    floats), gs = 0 with es != 0, denormal gs w.  Returns also `near`, the mask of the +-1e-3 block."""
    rng = np.random.default_rng(404)
    n = 400_000
    gs = _signed_log(rng, n, -8.0, math.log10(750.0)).astype(np.float32)
    es = (np.abs(gs.astype(np.float64)) * 10.0 ** rng.uniform(-8.0, 2.0, n)).astype(np.float32)
    es[rng.random(n) < 0.1] = 0.0
    w = rng.uniform(2e-3, 1.0, n).astype(np.float32)
    w[rng.random(n) < 0.15] *= np.float32(-1.0)
    Iv = 10.0 ** rng.uniform(-300.0, 300.0, n)
    Iv[rng.random(n) < 0.2] = 0.0
    blocks = [(Iv, gs, es, w, np.zeros(n, bool))]
    # floats on both sides of |gl| = 1e-3
    c = int(np.float32(1e-3).view(np.uint32))
    near = np.arange(c - 300, c + 301, dtype=np.uint32).view(np.float32)
    for sign in (1.0, -1.0):
        for gs0 in (1.0, 0.5, 3.0, 1e-3, 0.37):       # gs w = (near / gs0 rounded) * gs0: products that land around 1e-3
            wv = (near.astype(np.float64) / gs0).astype(np.float32)
            k = len(wv)
            blocks.append((np.full(k, 0.25), np.full(k, sign * gs0, np.float32), np.full(k, 0.7, np.float32), wv, np.ones(k, bool)))
            blocks.append((np.zeros(k), np.full(k, sign * gs0, np.float32), np.full(k, 2.0, np.float32), wv, np.ones(k, bool)))
    # gs = 0 with es != 0; denormal gs w (and gs w that underflows to zero)
    k = 2000
    blocks.append((10.0 ** rng.uniform(-10, 10, k), np.zeros(k, np.float32), (10.0 ** rng.uniform(-6, 3, k)).astype(np.float32),
                   rng.uniform(2e-3, 1.0, k).astype(np.float32), np.zeros(k, bool)))
    blocks.append((10.0 ** rng.uniform(-10, 10, k), _signed_log(rng, k, -36.0, -30.0).astype(np.float32),
                   (10.0 ** rng.uniform(-30, 3, k)).astype(np.float32), (10.0 ** rng.uniform(-12, 0, k)).astype(np.float32),
                   np.zeros(k, bool)))
    Iv, gs, es, w, near = (np.concatenate([b[i] for b in blocks]) for i in range(5))
    pad = (3 - len(Iv)) % 256
    z32 = np.zeros(pad, np.float32)
    return (np.concatenate([Iv, np.zeros(pad)]), np.concatenate([gs, z32]), np.concatenate([es, z32]),
            np.concatenate([w, z32]), np.concatenate([near, np.zeros(pad, bool)]))


@functools.lru_cache(maxsize=None)
def div_args():
    """(a, b) of div_fast as float64: a = any finite float widened (0 and the float denormals among them), b = a float
    with |b| in [1e-30, FLT_MAX], both signs -- the domain RT_RS_MIN and gs_cap leave the divisor."""
    rng = np.random.default_rng(505)
    n = 2_000_000
    a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    a = a[np.isfinite(a)]
    den = rng.integers(1, 0x00800000, 20_000, dtype=np.uint32).view(np.float32)          # float denormals
    a = np.concatenate([a, den, -den])
    lo, hi = int(np.float32(1e-30).view(np.uint32)), int(np.float32(FLT_MAX).view(np.uint32))
    b = rng.integers(lo, hi + 1, len(a), dtype=np.uint32).view(np.float32)
    b = np.where(rng.random(len(a)) < 0.5, -b, b)
    sa = np.float32([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 1.0, 3.0, FLT_MAX, -FLT_MAX, 1e-30, 0.1])
    sb = np.float32([1e-30, -1e-30, FLT_MAX, -FLT_MAX, 1.0, 3.0, -7.0, 0.5, 1.0000001, 1.9999999, 1e30, 1.0000000e-30])
    A, B = np.meshgrid(sa, sb)
    a = np.concatenate([A.ravel(), a]).astype(np.float64)
    b = np.concatenate([B.ravel(), b]).astype(np.float64)
    pad = (3 - len(a)) % 256
    return np.concatenate([a, np.ones(pad)]), np.concatenate([b, np.full(pad, 3.0)])


def _moved(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def _axis_values(g, d, rng, n_rand):
    """coordinates that try a deposit axis: every cell edge g[i] +- d/2 moved by 0, +-1, +-2 ulp, the grid points, just
    inside and outside both ends, far outside, non-finite, and random ones over a little more than the axis."""
    g = np.asarray(g, dtype=np.float64)
    out = [g]
    for edge in (g + 0.5 * d, g - 0.5 * d, g[:1] - 0.5 * d, g[-1:] + 0.5 * d, g + d, g - d):
        out += [_moved(edge, k) for k in (0, 1, -1, 2, -2)]
    out.append(np.array([1e300, -1e300, np.inf, -np.inf, np.nan]))
    span = g[-1] - g[0] + 2.0 * d
    out.append(rng.uniform(g[0] - 0.75 * d - 0.02 * span, g[-1] + 0.75 * d + 0.02 * span, n_rand))
    return np.concatenate(out)


def uniform_grid(n, g0, d):
    return g0 + d * np.arange(n, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def deposit_cases():
    """[(grids, d, v [n][4])]: uniform grids of 1, 2, 3, 64 and 1000 points (origins and spacings that are no round
    binary numbers, so that g0 + i d, v - d/2 and (t - g0) / d all round) and one mildly non-uniform grid whose points lie
    up to 0.3 d off the uniform ones -- the arithmetic guess is then wrong for part of the axis and the bisection runs."""
    rng = np.random.default_rng(606)
    g64 = uniform_grid(64, -0.63, 0.02)
    bumpy = uniform_grid(64, -3.15, 0.1) + 0.03 * np.sin(np.arange(64) * 1.7)
    sets = [
        ([uniform_grid(1, 0.3, 0.5), uniform_grid(2, -0.1, 0.2), uniform_grid(3, 1e-3, 0.7), g64], [0.5, 0.2, 0.7, 0.02], 50_000),
        ([uniform_grid(1000, -49.95, 0.1), bumpy, uniform_grid(64, 0.0, 1.0 / 3.0), uniform_grid(3, -1.0, 1.0)],
         [0.1, 0.1, 1.0 / 3.0, 1.0], 300_000),
    ]
    cases = []
    for grids, d, n_rand in sets:
        cols = [_axis_values(g, dd, rng, n_rand) for g, dd in zip(grids, d)]
        n = max(len(c) for c in cols)
        n += (3 - n) % 256
        v = np.empty((n, 4))
        for a, c in enumerate(cols):       # shorter columns: filled up with random coordinates of that axis
            g, dd = grids[a], d[a]
            fill = rng.uniform(g[0] - dd, g[-1] + dd, n - len(c))
            v[:, a] = rng.permutation(np.concatenate([c, fill]))
        cases.append((tuple(grids), tuple(d), v))
    return cases


def _around(bits, k=64):
    lo = max(int(bits) - k, 0)
    hi = min(int(bits) + k, 0x7f7fffff)
    return np.arange(lo, hi + 1, dtype=np.uint32)


def _float_args(branch_floats):
    u = [np.arange(0, 0x7f800000, 1021, dtype=np.uint32)]
    u += [_around(np.float32(b).view(np.uint32)) for b in branch_floats]
    x = np.unique(np.concatenate(u)).view(np.float32)
    x = np.concatenate([x, -x, np.float32([np.inf, -np.inf, np.nan])])
    return ragged(x, np.float32(0.0))


@functools.lru_cache(maxsize=None)
def tan_args():
    """every 1021st float of [0, FLT_MAX], both signs; +-64 floats around the branch points of tanf_flt32_kernel,
    tanf_flt32_wide and ktanf_flt32 as the source has them (2^-13, 0.2, 0.6744 = 0x3f2ca140, pi/4 = 0x3f490fda, the
    0x3fc90fd0 block, 1.375, FLT_MAX); +-0, +-inf, NaN."""
    pts = [2.0 ** -13, 0.2, 1.375, FLT_MAX] + [np.uint32(b).view(np.float32) for b in (0x3f2ca140, 0x3f490fda, 0x3fc90fd0, 0x3fc90fdf)]
    return _float_args(pts)


@functools.lru_cache(maxsize=None)
def atan_args():
    """likewise for atanf_flt32_kernel: 2^-29, 0.4375, FLT_MAX."""
    return _float_args([2.0 ** -29, 0.4375, FLT_MAX])
