"""Inputs and references of the spectra-seed tests (a plain helper module: `from spectra_seeds import ...`).  Nothing here
touches a device; tests/test_spectra_seeds_host.py asserts the census on the CPU oracle, tests/test_gpu_spectra_seeds.py runs
the inputs.

The inputs are those of the scan tests: length_scan.seeded_forward(seed_small, N) and suffix_scan.seeded_backward(seed_small, N)
-- 1 350 rays (21 tiles and a ragged one of 6), K = 82 (five groups of 16 and a left-over of two).
    seed 0   the problem's own seed
    seed 1   seed_scan.primed of the `narrow` profile (suffix_seeds.seeds_of): another support, f[4] reversed in k, another f0
The reference of (s, n) is the oracle's probe on seed_scan.with_seed(sub-problem of n lengths, seed_s); of spectra mode the
probe on the problem itself with seed_s.

    problem_of(seed_small, method, N)   the forward (2) or backward (1) problem
    sub(p, n)                           prefix or suffix of n lengths, by the method
    failing(p, seed_small)              (the problem with a NaN in a lineshape table, (own seed, seed 1 with f[4][3] negated)):
                                        backward suffix_seeds.failing (NaN at length 1, which only n = N reaches), forward its
                                        twin built the same way with the NaN at length 3 (read by n >= 4)
    probe_of(oracle, q, seed, rays)     the oracle's probe of q created with `seed`
    WANT_CODES[method]                  per seed, n = 2 .. 6: the OR of the codes of failing(N = 6), from the oracle"""
import length_scan as ls
import seed_scan as sc
import suffix_scan as sx
import suffix_seeds as sfx
import table_variants as tv

_built = {}


def problem_of(seed_small, method, N=6):
    return sx.seeded_backward(seed_small, N) if method == 1 else ls.seeded_forward(seed_small, N)


def sub(p, n):
    return ls.prefix(p, n) if p.method == 2 else sx.suffix(p, n)


def seeds_of(p, seed_small):
    return sfx.seeds_of(p, seed_small)


def failing(p, seed_small):
    if p.method == 1:
        return sfx.failing(p, seed_small)
    key = ("failing forward", id(p))
    if key not in _built:
        s0, s1 = seeds_of(p, seed_small)
        _built[key] = (p, tv.crafted_nan_lineshape(p, i=3), (s0, sfx.negated(s1, 3)))
    return _built[key][1:]


def probe_of(oracle, q, seed, rays):
    return oracle.probe(sc.with_seed(q, seed, "a spectra seed"), rays, want_Iv=True)


def code_of(err):
    code = 0
    for e in (-1, -2, -3):
        if (err == e).any():
            code |= 1 << -e
    return code


CLEAN_6 = {2: [[1350, 1344, 1289, 1243, 1180], [80, 80, 80, 80, 80]],      # per method and seed: clean non-zero rows at n = 2 .. 6
           1: [[1300, 1215, 1124, 1051, 967], [44, 49, 69, 61, 56]]}
WANT_CODES = {2: [[0, 0, 8, 8, 8], [4, 4, 12, 12, 12]], 1: sfx.WANT_CODES}
