"""Inputs of the length-scan tests (a plain helper module: `from length_scan import ...`).  Nothing here touches a device.

scan_problem(p, N)   p with N lengths: the tables repeated as with_lengths of tests/test_gpu_method_pairs.py repeats them
                     (gain[0], then gain[1], gain[2], gain[1], ...), and g0 of length i scaled by 1 + 0.1 i, so that no
                     two lengths share a table -- a kernel that reads the table of another length cannot pass.
The two problems of tests/test_gpu_length_scan.py, built once per session (counts_from_oracle keys on identity):
    seeded forward    regrid_seed_beam(seed_small, 9, 5, 6, 5)              1 350 rays
    emission forward  regrid_beam(ase_forward(ASE_small), 12, 6, 5, 4)      1 440 rays
"""
import copy
import dataclasses
import importlib

import numpy as np

import method_pairs as mp

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")


def scan_problem(p, N, scale_g0=True):
    q = copy.copy(p)
    g = p.gain
    q.gain = [g[0]] + [g[1 + (i % 2)] for i in range(N - 1)]
    if scale_g0:
        q.gain = [q.gain[0]] + [dataclasses.replace(t, g0=t.g0 * np.float32(1.0 + 0.1 * i)) for i, t in enumerate(q.gain) if i > 0]
    q.golden_image = q.golden_I_ang = None
    q.label = f"{p.label} / {N} lengths"
    return q


_built = {}


def seeded_forward(seed_small, N=6):
    if ("seed", N) not in _built:
        _built[("seed", N)] = scan_problem(problem_mod.regrid_seed_beam(seed_small, nx=9, ny=5, na=6, nb=5), N)
    return _built[("seed", N)]


def emission_forward(ase_small, N=6):
    if ("ase", N) not in _built:
        _built[("ase", N)] = scan_problem(problem_mod.regrid_beam(mp.ase_forward(ase_small), nx=12, ny=6, na=5, nb=4), N)
    return _built[("ase", N)]


_prefixes = {}


def prefix(p, n):
    """problem.prefix_lengths(p, n), one object per (p, n) and session."""
    if (id(p), n) not in _prefixes:
        _prefixes[(id(p), n)] = (p, problem_mod.prefix_lengths(p, n))
    return _prefixes[(id(p), n)][1]


def escape_census(oracle, p, rays):
    """Per n = 2 .. N: (escaped rays of the prefix run, exit rays of it) from the oracle's probe; flag bit 0 = escaped."""
    out = {}
    for n in range(2, p.N + 1):
        pr = oracle.probe(prefix(p, n), rays, want_Iv=False)
        out[n] = ((pr["flags"] & 1) != 0, pr["ray2"])
    return out
