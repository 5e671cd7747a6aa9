"""Inputs and references of the suffix-ASE-seed tests (a plain helper module: `from suffix_ase_seeds import ...`).  Nothing
here touches a device; tests/test_suffix_ase_seeds_host.py asserts the census on the CPU oracle,
tests/test_gpu_suffix_ase_seeds.py runs the inputs.

The input is ase_seeds.base(ase_small, 1, N, dark): the backward method, 1 440 rays, 22.5 tiles, nv 52, no two lengths sharing
a table; the seeds are ase_seeds.seeds_of(p).  The reference of record (0, n) is the oracle on suffix_scan.suffix(p, n), of
(1 + s, n) the oracle on ase_seeds.carry(suffix_scan.suffix(p, n), seed_s), whose scale the tests pass as scales[s].

    problems(p, seeds)   per record r = 0 .. len(seeds): {n: the problem whose step run is the reference of (r, n)}
    failing(p)           tv.crafted_nan_lineshape(p, i=1) with the seeds (wide, negative(narrow)): a NaN in the table of length 1,
                         which only the run of all N lengths reaches, and a negative f[4] entry under seed 1 -- the failure
                         matrix.  (i = 1, not i = 3: at N = 6 the matrix of i = 3 is the same for prefixes and suffixes.)"""
import ase_seeds as A
import suffix_scan as ss
import table_variants as tv

_built = {}


def problems(p, seeds):
    """One object per (p, seeds, r, n) and session (counts_from_oracle keys on identity)."""
    key = ("problems", id(p), tuple(id(s) for s in seeds))
    if key not in _built:
        rows = [{n: ss.suffix(p, n) for n in range(2, p.N + 1)}]
        for seed in seeds:
            rows.append({n: A.carry(ss.suffix(p, n), seed) for n in range(2, p.N + 1)})
        _built[key] = (p, seeds, rows)
    return _built[key][2]


def scales_of(p, seeds):
    return [A.carry(ss.suffix(p, p.N), s).scale for s in seeds]


def failing(p):
    """(the problem with a NaN in the lineshape table of length 1, (wide, negated narrow))"""
    key = ("failing", id(p))
    if key not in _built:
        w, n = A.seeds_of(p)
        _built[key] = (p, tv.crafted_nan_lineshape(p, i=1), (w, A.negative(n)))
    return _built[key][1:]


WANT_CODES = [[0, 0, 0, 0, 8], [0, 0, 0, 0, 8], [4, 4, 4, 4, 12]]     # per record, n = 2 .. 6, of failing(base(N = 6))
