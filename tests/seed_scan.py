"""Inputs and helpers of the scan-seed tests (a plain helper module: `from seed_scan import ...`).  Nothing here touches a
device; tests/test_seed_scan_host.py asserts the census of every input on the CPU oracle, tests/test_gpu_seed_scan.py runs
them.

The inputs, each a pair (problem carrying seed 0, the same problem carrying seed 1), built once per session
(counts_from_oracle and length_scan.prefix key on identity):
    p450(seed_small, N=6)   scan_problem(e2e_problem(seed_small, "limiter"), N); seed A = its own, seed B = primed of the
                            "narrow" profile.  450 rays, seven tiles and a ragged one; N = 10 reaches beyond the first chunk.
    p1350(seed_small)       length_scan.seeded_forward(seed_small); seeds own and primed(own).  1 350 rays, all in range.
    f1350(seed_small)       crafted_nan_lineshape(P1350, i=3); seed 0 = own, seed 1 = primed(own) with f[4][1] = -|f[4][1]|.
primed(seed): f[4] reversed in k and f0 x 0.37, as in tests/test_gpu_seed_set.py -- a kernel that reads seed 0's f[4] or f0
for seed 1 cannot pass."""
import copy
import importlib

import numpy as np

import length_scan as ls
import seed_profiles as sp
import table_variants as tv

rt = importlib.import_module("raytrace-miniapp_amd")


def primed(seed):
    """The second seed of a pair: f[4] reversed in k, f0 x 0.37."""
    return rt.Seed(list(seed.x), list(seed.f[:4]) + [np.ascontiguousarray(seed.f[4][::-1])], seed.f0 * 0.37)


def with_seed(p, seed, label):
    q = copy.copy(p)
    q.seed = seed
    q.golden_image = q.golden_I_ang = None
    q.label = f"{p.label} / {label}"
    return q


_built = {}


def p450(seed_small, N=6):
    if ("p450", N) not in _built:
        base = ls.scan_problem(sp.e2e_problem(seed_small, "limiter"), N)
        b_seed = primed(sp.e2e_problem(seed_small, "narrow").seed)
        _built[("p450", N)] = (with_seed(base, base.seed, "seed A (limiter)"), with_seed(base, b_seed, "seed B (narrow')"))
    return _built[("p450", N)]


def p1350(seed_small):
    if "p1350" not in _built:
        base = ls.seeded_forward(seed_small)
        _built["p1350"] = (base, with_seed(base, primed(base.seed), "primed seed"))
    return _built["p1350"]


def f1350(seed_small):
    if "f1350" not in _built:
        base = tv.crafted_nan_lineshape(p1350(seed_small)[0], i=3)
        s1 = primed(base.seed)
        f4 = s1.f[4].copy()
        f4[1] = -abs(f4[1])
        s1 = rt.Seed(list(s1.x), list(s1.f[:4]) + [f4], s1.f0)
        _built["f1350"] = (base, with_seed(base, s1, "primed seed, f[4][1] negative"))
    return _built["f1350"]


def in_range(seed, rays):
    return np.array([sp.ray_census(seed, rays[i:i + 1])[1] for i in range(len(rays))], dtype=bool)


def escaped(oracle, p, rays):
    """{n: bool per ray, escaped in the run of n lengths} for n = 2 .. N (the march does not depend on the seed)."""
    return {n: e for n, (e, _) in ls.escape_census(oracle, p, rays).items()}


def error_counts(oracle, p, rays):
    """{n: (failure code of the oracle's run of n lengths, {-1: .., -2: .., -3: ..} rays per return code)}, n = 2 .. N."""
    out = {}
    for n in range(2, p.N + 1):
        q = ls.prefix(p, n)
        err = np.asarray(oracle.exit_rays(q, rays)[1])
        out[n] = (oracle.image_loop(q, rays)["failure_code"], {c: int((err == c).sum()) for c in (-1, -2, -3)})
    return out
