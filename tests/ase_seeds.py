"""Inputs and helpers of the ASE-seed tests (a plain helper module: `from ase_seeds import ...`).  Nothing here touches a
device; tests/test_ase_seeds_host.py asserts the census of every input on the CPU oracle, tests/test_gpu_ase_seeds.py runs
them.

    base(ase_small, method, N=3, dark=False)
                    with_method(regrid_beam(ASE_small, 12, 6, 5, 4), method): an emission problem of 1 440 rays on the
                    beam's own grid; N = 5 through length_scan.scan_problem (no two lengths share a table); `dark`
                    multiplies g0 and E0 of every length by (ix < int(0.7 Nx)): rays that stay in the dark part have all
                    march sums zero, which the emission march marks (F_SKIP)
    wide(p)         a seed that covers the beam's grid and 0.6 spans beyond either end of every axis
    narrow(p)       a seed whose support leaves part of the grid out on every axis
    negative(seed)  the seed with f[4][3] negated: every in-range ray fails with error -2 under it
    carry(p, seed)  the SAME PROBLEM CREATED WITH THE SEED: p's tables (E0 present, unused), rays and method, the seed, and the
                    beam's own grids as seed_beam; its scale is da db -- the tests pass it as scales[s], so that the stock
                    oracle on carry(p, seed) is the reference of record 1 + s

Census of the 1 440 rays on the CPU oracle (tests/test_ase_seeds_host.py asserts what the tests need of it):
    input    escaped (m1 / m2)    in range, wide (m1 / m2)    in range, narrow (m1 / m2)
    N = 3    368 / 51             1 072 / 1 389               60 / 48
    N = 5    690 / 152            750 / 1 288                 49 / 48
    dark variant (N = 3): 459 / 432 rays have all sums zero, 304 / 384 of them in range of `wide`; N = 5: 423 / 360 and
    151 / 257; 6 (N = 5: 4 / 2) of the 23 tiles lie wholly in the dark.
No failure anywhere, no escaped ray is in range, every record is non-zero."""
import copy
import dataclasses
import importlib

import numpy as np

import length_scan as ls
import method_pairs as mp

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")

_built = {}


def base(ase_small, method, N=3, dark=False):
    """One object per (method, N, dark) and session (counts_from_oracle keys on identity)."""
    key = ("base", method, N, dark)
    if key not in _built:
        p = mp.with_method(problem_mod.regrid_beam(ase_small, nx=12, ny=6, na=5, nb=4), method)
        if N != 3:
            p = mp.with_method(ls.scan_problem(p, N), method)
        if dark:
            def darkened(g):
                lit = np.tile(np.arange(g.Nx) < int(0.7 * g.Nx), g.Ny).astype(np.float32)
                return dataclasses.replace(g, g0=g.g0 * lit, E0=g.E0 * lit)
            q = copy.copy(p)
            q.gain = [p.gain[0]] + [darkened(g) for g in p.gain[1:]]
            q.golden_image = q.golden_I_ang = None
            q.label = f"{p.label} / dark beyond 0.7 Nx"
            p = q
        assert p.seed is None and p.use_emis and p.method == method and p.N == N and p.n_rays_total == 1440
        _built[key] = p
    return _built[key]


def _spatial(p, lo, hi):
    b = p.beam
    xs = []
    for g in (b.x, b.y, b.a, b.b):
        span = g[-1] - g[0]
        xs.append(np.linspace(g[0] + lo * span, g[-1] + hi * span, 9))
    f = 0.2 + np.sin(np.pi * np.linspace(0.0, 1.0, 9)) ** 2
    return xs, [f.copy() for _ in range(4)]


def wide(p):
    nv = p.beam.nv
    xs, fs = _spatial(p, -0.6, 0.6)
    k = np.arange(nv, dtype=np.float64)
    return rt.Seed(xs + [k], fs + [np.exp(-((k - 0.4 * nv) / (0.2 * nv)) ** 2)], 3e-3)


def narrow(p):
    nv = p.beam.nv
    xs, fs = _spatial(p, 0.22, -0.27)
    k = np.arange(nv, dtype=np.float64)
    return rt.Seed(xs + [k], fs + [(1.0 + k) / nv], 1.1e-3)


def negative(seed):
    f4 = seed.f[4].copy()
    f4[3] = -f4[3]
    return rt.Seed(list(seed.x), list(seed.f[:4]) + [f4], seed.f0)


_carried = {}


def carry(p, seed):
    """One object per (p, seed) and session."""
    key = (id(p), id(seed))
    if key not in _carried:
        b = p.beam
        q = copy.copy(p)
        q.seed = seed
        q.seed_beam = problem_mod.SeedBeam(b.x, b.y, b.a, b.b, b.dx, b.dy, b.da, b.db)
        q.golden_image = q.golden_I_ang = None
        q = mp.with_method(q, p.method)
        q.label = f"{p.label} / carrying a seed"
        assert q.seed is seed and not q.use_emis and q.gain[1].E0 is not None and q.method == p.method
        assert abs(q.scale - b.da * b.db) <= 1e-12 * b.da * b.db
        _carried[key] = (p, seed, q)
    return _carried[key][2]


_seeds = {}


def seeds_of(p):
    """(wide(p), narrow(p)), one pair of objects per p and session."""
    if id(p) not in _seeds:
        _seeds[id(p)] = (p, (wide(p), narrow(p)))
    return _seeds[id(p)][1]


def in_range(seed, rays):
    """Per ray: inside the support of the seed on all four axes (Helper.h:233-236; the float coordinates widen exactly)."""
    ok = np.ones(len(rays), dtype=bool)
    for d, k in enumerate("xyab"):
        v = rays[k].astype(np.float64)
        ok &= (v >= seed.x[d][0]) & (v <= seed.x[d][-1])
    return ok


def seed_points(p, probe, rays):
    """The rays at which the seed factor is taken: the launch rays (method 2) or the exit rays (method 1)."""
    return probe["ray2"] if p.method == 1 else rays
