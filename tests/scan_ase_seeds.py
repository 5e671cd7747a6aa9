"""Inputs and references of the scan-ASE-seed tests (a plain helper module: `from scan_ase_seeds import ...`).  Nothing here
touches a device; tests/test_scan_ase_seeds_host.py asserts the census on the CPU oracle, tests/test_gpu_scan_ase_seeds.py runs
the inputs.

The input is ase_seeds.base(ase_small, 2, N, dark): 1 440 rays, 23 tiles, the last holding 32 rays, nv 52, no two lengths
sharing a table; the seeds are ase_seeds.seeds_of(p).  The reference of record (0, n) is the oracle on length_scan.prefix(p, n),
of (1 + s, n) the oracle on ase_seeds.carry(length_scan.prefix(p, n), seed_s), whose scale the tests pass as scales[s].

    problems(p, seeds)   per record r = 0 .. len(seeds): {n: the problem whose step run is the reference of (r, n)}
    dark_first(zero)     the ray order that puts the rays the march marks first: whole dark tiles on a list
    failing(p)           tv.crafted_nan_lineshape(p, i=3) with the seeds (wide, negative(narrow)): a NaN in the table of length 3
                         and a negative f[4] entry under seed 1 -- the failure matrix"""
import ase_seeds as A
import length_scan as ls
import table_variants as tv

_built = {}


def problems(p, seeds):
    """One object per (p, seeds, r, n) and session (counts_from_oracle keys on identity)."""
    key = ("problems", id(p), tuple(id(s) for s in seeds))
    if key not in _built:
        rows = [{n: ls.prefix(p, n) for n in range(2, p.N + 1)}]
        for seed in seeds:
            rows.append({n: A.carry(ls.prefix(p, n), seed) for n in range(2, p.N + 1)})
        _built[key] = (p, seeds, rows)
    return _built[key][2]


def scales_of(p, seeds):
    return [A.carry(ls.prefix(p, p.N), s).scale for s in seeds]


def dark_first(zero_all):
    """The order of the rays with the marked ones (all sums zero over the whole run) first, each group in grid order: as a
    list the first tiles then hold marked rays only -- no ray of theirs is live for the ASE records, all are for the seeds'."""
    import numpy as np
    return np.argsort(~np.asarray(zero_all), kind="stable")


def failing(p):
    """(the problem with a NaN in the lineshape table of length 3, (wide, negated narrow))"""
    key = ("failing", id(p))
    if key not in _built:
        w, n = A.seeds_of(p)
        _built[key] = (p, tv.crafted_nan_lineshape(p, i=3), (w, A.negative(n)))
    return _built[key][1:]


WANT_CODES = [[0, 0, 8, 8, 8], [0, 0, 8, 8, 8], [4, 4, 12, 12, 12]]     # per record, n = 2 .. 6, of failing(base(N = 6))
