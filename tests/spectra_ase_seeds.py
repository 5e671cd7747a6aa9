"""Inputs and references of the tests of spectra mode with ASE seeds (a plain helper module: `from spectra_ase_seeds import
...`).  Nothing here touches a device; tests/test_spectra_ase_seeds_host.py asserts the census on the CPU oracle,
tests/test_gpu_spectra_ase_seeds.py runs the inputs.

The inputs are those of the ASE-seed tests (tests/ase_seeds.py): ase_seeds.base(ase_small, method, N) -- an emission problem of
1 440 rays on the beam's own grid (22 full tiles and a ragged one of 32), K = 52 (three groups of 16 and a left-over of 4);
N = 3 takes rt_spec_ase_seeds_kernel<6>, N = 5 <0>; the seeds `wide` and `narrow`.
    block 0       the oracle's probe of p
    block 1 + s   the oracle's probe of ase_seeds.carry(p, seed_s): the same problem created with the seed

    problem_of(ase_small, method, N, dark)   ase_seeds.base
    seeds_of(p)                              (wide(p), narrow(p))
    refs(oracle, p, seeds, rays, key)        [probe of p, probe of carry(p, seed) per seed], once per key, left unchanged
    all_zero_sums(probe)                     per ray: every gvl and evl sum is zero -- what the emission march marks (F_SKIP)
    negative_pair(p)                         (wide, negative(narrow)): -2 under seed 1 only
    nan_tables(p)                            table_variants.crafted_nan_lineshape(p): -3 where a ray reads the NaN, per block
    odd_k(ase_small, method)                 the problem resampled to 51 frequencies
    steep(rays)                              the rays with ray 7 launched almost perpendicular to z (error -1)
    code_of(err)                             the OR of the codes of an err array"""
import importlib

import numpy as np

import ase_seeds as A
import table_variants as tv

problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")

TILE = 64
_refs, _built = {}, {}


def problem_of(ase_small, method, N=3, dark=False):
    return A.base(ase_small, method, N, dark)


def seeds_of(p):
    return A.seeds_of(p)


def refs(oracle, p, seeds, rays, key):
    if key not in _refs:
        _refs[key] = (p, [oracle.probe(p, rays, want_Iv=True)] + [oracle.probe(A.carry(p, sd), rays, want_Iv=True) for sd in seeds])
    return _refs[key][1]


def all_zero_sums(probe):
    return ~probe["gvl"].any(axis=1) & ~probe["evl"].any(axis=1)


def dark_tiles(zero):
    """First rays of the 64-ray tiles all of whose rays have all sums zero."""
    return [t for t in range(0, len(zero), TILE) if zero[t:t + TILE].all()]


def negative_pair(p):
    key = ("negative", id(p))
    if key not in _built:
        w, n = A.seeds_of(p)
        _built[key] = (p, (w, A.negative(n)))
    return _built[key][1]


def nan_tables(p):
    key = ("nan", id(p))
    if key not in _built:
        _built[key] = (p, tv.crafted_nan_lineshape(p))
    return _built[key][1]


def odd_k(ase_small, method, nv=51):
    key = ("nv", method, nv)
    if key not in _built:
        _built[key] = (None, problem_mod.resample_frequency(A.base(ase_small, method, 3), nv))
    return _built[key][1]


def steep(rays, i=7):
    bad = rays.copy()
    bad["a"][i] = 1500.0
    return bad


def code_of(err):
    code = 0
    for e in (-1, -2, -3):
        if (np.asarray(err) == e).any():
            code |= 1 << -e
    return code
