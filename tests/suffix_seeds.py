"""Inputs and references of the suffix-seed tests (a plain helper module: `from suffix_seeds import ...`).  Nothing here
touches a device; tests/test_suffix_seeds_host.py asserts the census on the CPU oracle, tests/test_gpu_suffix_seeds.py runs
the inputs.

The input is suffix_scan.seeded_backward(seed_small, N): the backward method, 1 350 rays (21 tiles and a ragged one of 6), nv 82,
no two lengths sharing a table.
    seed 0   the problem's own seed
    seed 1   seed_scan.primed of the `narrow` profile of seed_profiles.e2e_problem: a narrower support (its in-range count at
             the exit ray differs from n to n), f[4] reversed in k and another f0 -- a kernel that reads seed 0's table, or takes
             the factor at the wrong state, cannot pass
The reference of record (s, n) is the oracle on seed_scan.with_seed(suffix_scan.suffix(p, n), seed_s, ...): the suffix problem
of the last n lengths created with seed s.

    seeds_of(p, seed_small)   (seed 0, seed 1)
    problems(p, seeds)        per seed s: {n: the problem whose step run is the reference of (s, n)}
    carry(p, seed)            p created with `seed`: the single-seed plan a seed's curve is held against
    failing(p, seed_small)    tv.crafted_nan_lineshape(p, i=1) with the seeds (own, seed 1 with f[4][3] negated): a NaN in the table
                              of length 1, which only the run of all N lengths reaches, and a negative f[4] entry under seed 1"""
import importlib

import numpy as np

import seed_profiles as sp
import seed_scan as sc
import suffix_scan as ss
import table_variants as tv

rt = importlib.import_module("raytrace-miniapp_amd")

_built = {}


def seeds_of(p, seed_small):
    key = ("seeds", id(p))
    if key not in _built:
        _built[key] = (p, (p.seed, sc.primed(sp.e2e_problem(seed_small, "narrow").seed)))
    return _built[key][1]


def carry(p, seed):
    """One object per (p, seed) and session (counts_from_oracle and suffix_scan.suffix key on identity)."""
    key = ("carry", id(p), id(seed))
    if key not in _built:
        _built[key] = (p, seed, sc.with_seed(p, seed, "seed 0 (own)" if seed is p.seed else "another seed"))
    return _built[key][2]


def problems(p, seeds):
    key = ("problems", id(p), tuple(id(s) for s in seeds))
    if key not in _built:
        rows = [{n: sc.with_seed(ss.suffix(p, n), seed, f"seed {s}") for n in range(2, p.N + 1)} for s, seed in enumerate(seeds)]
        _built[key] = (p, seeds, rows)
    return _built[key][2]


def negated(seed, k=3):
    """`seed` with f[4][k] negated."""
    f4 = seed.f[4].copy()
    f4[k] = -f4[k]
    return rt.Seed(list(seed.x), list(seed.f[:4]) + [f4], seed.f0)


def failing(p, seed_small):
    """(the problem with a NaN in the lineshape table of length 1, (own seed, seed 1 with f[4][3] negated))"""
    key = ("failing", id(p))
    if key not in _built:
        s0, s1 = seeds_of(p, seed_small)
        _built[key] = (p, tv.crafted_nan_lineshape(p, i=1), (s0, negated(s1, 3)))
    return _built[key][1:]


def in_range(seed, rays):
    return sc.in_range(seed, rays)


WANT_CODES = [[0, 0, 0, 0, 8], [4, 4, 4, 4, 12]]     # per seed, n = 2 .. 6, of failing(seeded_backward(N = 6))
ESCAPED_6 = [0, 6, 61, 107, 170]                      # escaped by the end of the run of the last n = 2 .. 6 lengths
IN_RANGE_6 = [[1300, 1215, 1124, 1051, 967], [44, 49, 69, 61, 56]]   # per seed: in range at the exit ray and not escaped
