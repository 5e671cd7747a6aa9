"""Inputs of the suffix-scan tests (a plain helper module: `from suffix_scan import ...`).  Nothing here touches a device.

The two backward problems of tests/test_gpu_suffix_scan.py and tests/test_suffix_scan_host.py, built once per session
(counts_from_oracle keys on identity), at N lengths with no two lengths sharing a table (length_scan.scan_problem):
    emission backward  scan_problem(regrid_beam(ASE_small, 12, 6, 5, 4), N)                          1 440 rays
    seeded backward    scan_problem(regrid_seed_beam(seed_backward(seed_small), 9, 5, 6, 5), N)      1 350 rays
1 440 rays are 22.5 tiles; at N = 6 the five records are a full chunk and a rest in both modes of rt_step_rscan_kernel.
"""
import importlib

import length_scan as ls
import method_pairs as mp

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")

_built = {}


def emission_backward(ase_small, N=6):
    if ("ase", N) not in _built:
        _built[("ase", N)] = ls.scan_problem(problem_mod.regrid_beam(ase_small, nx=12, ny=6, na=5, nb=4), N)
    return _built[("ase", N)]


def seeded_backward(seed_small, N=6):
    if ("seed", N) not in _built:
        _built[("seed", N)] = ls.scan_problem(problem_mod.regrid_seed_beam(mp.seed_backward(seed_small), nx=9, ny=5, na=6, nb=5), N)
    return _built[("seed", N)]


_suffixes = {}


def suffix(p, n):
    """problem.suffix_lengths(p, n), one object per (p, n) and session."""
    if (id(p), n) not in _suffixes:
        _suffixes[(id(p), n)] = (p, problem_mod.suffix_lengths(p, n))
    return _suffixes[(id(p), n)][1]


_census = {}


def census(oracle, p, rays, key):
    """Per n = 2 .. N the oracle's probe of the suffix problem (flags bit 0 = escaped, err, ray2, Iv), once per key."""
    if key not in _census:
        _census[key] = {n: oracle.probe(suffix(p, n), rays, want_Iv=True) for n in range(2, p.N + 1)}
    return _census[key]
