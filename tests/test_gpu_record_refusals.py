"""Every refusal of the record entry points of the C ABI, by its full text.

The installers (rt_hip_plan_set_*seeds), the two scan switches (rt_hip_plan_enable_*_scan) and the accessors
(rt_hip_plan_fetch_*_step / rt_hip_plan_*_step_ptrs) are called through the raw C ABI -- the Python checks of backend.Plan are
not in the way -- against every plan state they refuse, and rt_hip_last_error() is compared, whole, with a literal written
here.  Every refusal is RT_ERR_ARG before any launch; nothing here provokes a failure code or a fault.

Plans: ASE_small (emission) and seed_small (seeded), both at N = 3, each forward (method 2) and backward (method 1), and
ASE_small at N = RT_N_SCAN_MAX + 2 for the length limit (never run).  Rays: a list of 64.  Eight step runs in all, one per
record kind and a plain one; after each the accessors of the other kinds refuse, those of its own kind refuse every index
one outside the set and serve every index inside it: pointers = block 0's + block * stride, the fetch bit for bit what a
read of those pointers gives (the pattern of tests/test_gpu_record_access.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import ase_seeds as A
import length_scan as ls
import method_pairs as mp
import seed_scan as ss

rt = importlib.import_module("raytrace-miniapp_amd")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

KEYS = ("E_v", "nf", "I_ang")
N_RAYS = 64

# accessor pair -> (number of indices, what both say after a run of another kind)
PAIRS = {
    "seed_step": (1, "the last run was not a step run with a seed set"),
    "length_step": (1, "the last run was not a step run with the length scan on"),
    "full_step": (1, "the last run was not a step run of an emission plan with ASE seeds"),
    "full_length_step": (2, "the last run was not a step run of a length scan with ASE seeds"),
    "seed_length_step": (2, "the last run was not a step run of a length scan with scan seeds"),
}
NO_SEED = "no such seed in the set of the last run"
NO_SCAN_SEED = "no such seed among the scan seeds of the last run"
BAD_R = "r must be 0 (ASE) .. n_seed of the last run"
BAD_N = "n must be 2 .. N of the last run"
VALIDATE = (": n_seed must be 0 .. RT_N_SEED_MAX", ": NULL seeds", ": incomplete seed table", ": seed.dim[4] != beam.nv")


def entries(pair):
    return "rt_hip_plan_fetch_" + pair, "rt_hip_plan_" + pair + "_ptrs"


def ptrs_of(plan, pair, *index):
    e, n, a = C.c_void_p(), C.c_void_p(), C.c_void_p()
    lib = plan.hl.lib
    rc = getattr(lib, entries(pair)[1])(plan._h, *index, C.byref(e), C.byref(n), C.byref(a))
    return rc, (int(e.value or 0), int(n.value or 0), int(a.value or 0)), lib.rt_hip_last_error().decode()


def fetch_of(plan, pair, *index):
    b = plan.problem.beam
    out = dict(E_v=np.full(b.nv, np.nan), nf=np.full(b.nx * b.ny, np.nan), I_ang=np.full(b.na * b.nb, np.nan))
    code = C.c_uint(0xffffffff)
    lib = plan.hl.lib
    rc = getattr(lib, entries(pair)[0])(plan._h, *index, cabi._dp(out["E_v"]), cabi._dp(out["nf"]), cabi._dp(out["I_ang"]), C.byref(code))
    out["failure_code"] = code.value
    return rc, out, lib.rt_hip_last_error().decode()


def access_refused(plan, pair, index, text):
    for name, (rc, _, err) in zip(entries(pair), (fetch_of(plan, pair, *index), ptrs_of(plan, pair, *index))):
        assert rc == cabi.RT_ERR_ARG and err == f"{name}: {text}", (pair, index, rc, err)


class _Dev:  # the CUDA array interface, which torch.as_tensor reads
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="<f8", data=(ptr, False), version=2, strides=None)


def read_device(plan, ptrs):
    import torch

    b = plan.problem.beam
    sizes = (b.nv, b.nx * b.ny, b.na * b.nb)
    return {k: torch.as_tensor(_Dev(p, n), device=torch.device("cuda", plan.device)).cpu().numpy() for k, p, n in zip(KEYS, ptrs, sizes)}


def block_layout(b):
    """(nf offset, I_ang offset, stride) of a block in bytes: E_v [nv] | pad to 256 bytes | nf [nx * ny] | I_ang [na * nb],
    the block padded to 256 bytes (no axis of these inputs has one point)."""
    assert min(b.nx, b.ny, b.na, b.nb) >= 2
    nf_off = (b.nv * 8 + 255) // 256 * 256
    ang_off = nf_off + b.nx * b.ny * 8
    return nf_off, ang_off, (ang_off + b.na * b.nb * 8 + 255) // 256 * 256


def serves(plan, pair, valid):
    """Every index of `valid` ({index: block}) is served: the pointers are block 0's + block * stride, the fetch is a read of them."""
    nf_off, ang_off, stride = block_layout(plan.problem.beam)
    rc, base, err = ptrs_of(plan, pair, *min(valid, key=valid.get))
    assert rc == cabi.RT_OK and min(valid.values()) == 0 and base[0] % 256 == 0, (pair, err)
    for index, block in valid.items():
        rc, ptrs, err = ptrs_of(plan, pair, *index)
        assert rc == cabi.RT_OK, (pair, index, err)
        at = base[0] + block * stride
        assert ptrs == (at, at + nf_off, at + ang_off), (pair, index, block)
        rc, rec, err = fetch_of(plan, pair, *index)
        assert rc == cabi.RT_OK and rec["failure_code"] != 0xffffffff, (pair, index, err)
        dev = read_device(plan, ptrs)
        for key in KEYS:
            assert np.array_equal(rec[key], dev[key], equal_nan=True), (pair, index, key)


def check_accessors(plan, own, n_seed):
    """After a run whose records the pairs `own` serve ({pair: ({index: block}, [(index outside, text)])}): every other pair
    refuses by the kind, the own ones refuse outside the set and serve the set."""
    for pair, (n_index, text) in PAIRS.items():
        if pair not in own:
            access_refused(plan, pair, (0, 2)[:n_index] if n_index == 2 else ((2,) if pair == "length_step" else (0,)), text)
    for pair, (valid, outside) in own.items():
        for index, text in outside:
            access_refused(plan, pair, index, text)
        serves(plan, pair, valid)


def rays_of(p):
    ids = np.arange(N_RAYS, dtype=np.int64) * (p.n_rays_total // N_RAYS)
    rays = p.build_rays(ids)
    assert len(rays) == N_RAYS
    return rays


def seed_array(seeds):
    keep = []
    arr = (cabi.RtSeed * max(1, len(seeds)))()
    for i, sd in enumerate(seeds):
        arr[i] = cabi.seed_record(sd, keep)
    return arr, keep


class Caller:
    """The installers and switches of one plan through the raw C ABI, with the text of a refusal."""

    def __init__(self, plan, seeds):
        self.plan, self.lib, self.h = plan, plan.hl.lib, plan._h
        self.seeds = list(seeds)
        self.arr, self._keep = seed_array(self.seeds)
        self.scales = np.array([0.5, 0.25])

    def _text(self, rc):
        return rc, self.lib.rt_hip_last_error().decode()

    def set(self, name, n_seed=None, arr="own"):
        fn = getattr(self.lib, "rt_hip_plan_set_" + name)
        n_seed = len(self.seeds) if n_seed is None else n_seed
        a = (self.arr if n_seed > 0 else None) if isinstance(arr, str) else arr
        if "ase" in name:
            return self._text(fn(self.h, n_seed, a, cabi._dp(self.scales) if n_seed > 0 else None))
        return self._text(fn(self.h, n_seed, a))

    def enable(self, name, on=1):
        return self._text(getattr(self.lib, "rt_hip_plan_enable_" + name)(self.h, on))

    def ok(self, rc_err):
        assert rc_err[0] == cabi.RT_OK, rc_err
        return self

    def refuses(self, rc_err, text):
        assert rc_err == (cabi.RT_ERR_ARG, text), (rc_err, text)
        return self

    def validates(self, name):
        """The four refusals of the seed tables, as every installer words them behind its own name."""
        who = "rt_hip_plan_set_" + name
        self.refuses(self.set(name, -1), who + VALIDATE[0])
        if name != "suffix_ase_seeds":   # (it has a text of its own for too many)
            self.refuses(self.set(name, cabi.RT_N_SEED_MAX + 1), who + VALIDATE[0])
        self.refuses(self.set(name, 1, None), who + VALIDATE[1])
        short, keep = seed_array(self.seeds[:1])
        short[0].dim[0] = 1
        self.refuses(self.set(name, 1, short), who + VALIDATE[2])
        nv, keep2 = seed_array(self.seeds[:1])
        nv[0].dim[4] = nv[0].dim[4] - 1
        self.refuses(self.set(name, 1, nv), who + VALIDATE[3])
        return self


def emission(ase_small, method, N=3):
    p = mp.with_method(ase_small, method)
    if N != 3:
        p = mp.with_method(ls.scan_problem(p, N), method)
    assert p.seed is None and p.use_emis and p.method == method and p.N == N
    return p


def seeded(seed_small, method):
    p = mp.with_method(seed_small, method)
    assert p.seed is not None and p.method == method and p.N == 3
    return p


def run_step(plan, rays):
    plan.set_rays(rays).enable_step().run()
    info = plan.fetch()
    assert info["stats"]["n_rays"] == N_RAYS
    return info


OUT_N = lambda N: [((1,), BAD_N), ((N + 1,), BAD_N)]


def test_forward_emission_plan(hip, ase_small):
    p = emission(ase_small, 2)
    N, L, ns = p.N, p.N - 1, 2
    rays = rays_of(p)
    with hip.Plan(p) as plan:
        c = Caller(plan, [A.wide(p), A.narrow(p)])
        check_accessors(plan, {}, 0)                      # no run yet
        # wrong flavour, wrong method, scan off
        c.refuses(c.set("seeds"), "rt_hip_plan_set_seeds: the plan was created without a seed (a set needs the gain-only mode)")
        c.refuses(c.set("scan_seeds"), "rt_hip_plan_set_scan_seeds: the plan was created without a seed (scan seeds need the gain-only mode)")
        c.refuses(c.set("scan_ase_seeds"), "rt_hip_plan_set_scan_ase_seeds: the length scan is off (rt_hip_plan_enable_length_scan first)")
        c.refuses(c.set("suffix_ase_seeds"),
                  "rt_hip_plan_set_suffix_ase_seeds: the plan's method is not 1 (a forward plan takes rt_hip_plan_set_scan_ase_seeds)")
        for on in (0, 1):
            c.refuses(c.enable("suffix_scan", on), "rt_hip_plan_enable_suffix_scan: the plan's method is not 1 "
                      "(only the backward march of N lengths begins with the marches of the last n)")
        c.validates("ase_seeds")
        # path or spectra enabled
        for mode in ("path", "spectra"):
            c.ok(c.enable(mode))
            c.refuses(c.set("ase_seeds"), "rt_hip_plan_set_ase_seeds: the path tracer or spectra mode is enabled (ASE seeds run in step mode only)")
            c.refuses(c.enable("length_scan"), "rt_hip_plan_enable_length_scan: the path tracer or spectra mode is enabled (the scan runs in step mode only)")
            c.ok(c.set("ase_seeds", 0)).ok(c.enable("length_scan", 0)).ok(c.enable(mode, 0))
        # a plain step run: every accessor refuses by the kind
        run_step(plan, rays)
        check_accessors(plan, {}, 0)
        # ASE seeds: held, they refuse the scan
        c.ok(c.set("ase_seeds"))
        c.refuses(c.enable("length_scan"), "rt_hip_plan_enable_length_scan: the plan holds a seed set (a seed set and a length scan exclude each other)")
        plan.run()
        check_accessors(plan, {"full_step": ({(r,): r for r in range(1 + ns)}, [((-1,), BAD_R), ((ns + 1,), BAD_R)])}, ns)
        c.ok(c.set("ase_seeds", 0))
        # the length scan: on, it refuses ASE seeds (even none) and takes its own
        c.ok(c.enable("length_scan"))
        for n_seed in (0, ns):
            c.refuses(c.set("ase_seeds", n_seed), "rt_hip_plan_set_ase_seeds: the length scan is on (ASE seeds and a length scan exclude each other)")
        c.validates("scan_ase_seeds")
        plan.run()
        check_accessors(plan, {"length_step": ({(n,): n - 2 for n in range(2, N + 1)}, OUT_N(N))}, 0)
        c.ok(c.set("scan_ase_seeds"))
        plan.run()
        full = {(r, n): r * L + n - 2 for r in range(1 + ns) for n in range(2, N + 1)}
        check_accessors(plan, {"length_step": ({(n,): n - 2 for n in range(2, N + 1)}, OUT_N(N)),
                               "full_length_step": (full, [((-1, 2), BAD_R), ((ns + 1, 2), BAD_R), ((0, 1), BAD_N), ((0, N + 1), BAD_N)])}, ns)
        # the scan off drops its seeds: the plain record again
        c.ok(c.enable("length_scan", 0))
        plan.run()
        check_accessors(plan, {}, 0)


def test_backward_emission_plan(hip, ase_small):
    p = emission(ase_small, 1)
    N, L, ns = p.N, p.N - 1, 2
    rays = rays_of(p)
    with hip.Plan(p) as plan:
        c = Caller(plan, [A.wide(p), A.narrow(p)])
        c.refuses(c.enable("length_scan"), "rt_hip_plan_enable_length_scan: the plan's method is not 2 "
                  "(only the forward march of N lengths holds the marches of fewer)")
        c.ok(c.enable("length_scan", 0))                  # (off on a plan whose scans are off: nothing to do)
        c.refuses(c.set("suffix_ase_seeds"), "rt_hip_plan_set_suffix_ase_seeds: the suffix scan is off (rt_hip_plan_enable_suffix_scan first)")
        c.refuses(c.set("scan_ase_seeds"), "rt_hip_plan_set_scan_ase_seeds: the length scan is off (rt_hip_plan_enable_length_scan first)")
        for mode in ("path", "spectra"):
            c.ok(c.enable(mode))
            c.refuses(c.enable("suffix_scan"), "rt_hip_plan_enable_suffix_scan: the path tracer or spectra mode is enabled (the scan runs in step mode only)")
            c.ok(c.enable("suffix_scan", 0)).ok(c.enable(mode, 0))
        # ASE seeds held
        c.ok(c.set("ase_seeds"))
        c.refuses(c.enable("suffix_scan"), "rt_hip_plan_enable_suffix_scan: the plan holds ASE seeds (ASE seeds and a suffix scan exclude each other)")
        c.ok(c.set("ase_seeds", 0))
        # the suffix scan on
        c.ok(c.enable("suffix_scan"))
        c.refuses(c.enable("length_scan", 0), "rt_hip_plan_enable_length_scan: the suffix scan is on (rt_hip_plan_enable_suffix_scan switches it off)")
        for n_seed in (0, ns):
            c.refuses(c.set("ase_seeds", n_seed), "rt_hip_plan_set_ase_seeds: the suffix scan is on (ASE seeds and a suffix scan exclude each other)")
        c.refuses(c.set("scan_ase_seeds"), "rt_hip_plan_set_scan_ase_seeds: the suffix scan is on (it takes no ASE seeds)")
        c.refuses(c.set("suffix_ase_seeds", cabi.RT_N_SEED_MAX + 1), "rt_hip_plan_set_suffix_ase_seeds: more than RT_N_SEED_MAX seeds")
        c.validates("suffix_ase_seeds")
        run_step(plan, rays)
        check_accessors(plan, {"length_step": ({(n,): n - 2 for n in range(2, N + 1)}, OUT_N(N))}, 0)
        c.ok(c.set("suffix_ase_seeds"))
        plan.run()
        full = {(r, n): r * L + n - 2 for r in range(1 + ns) for n in range(2, N + 1)}
        check_accessors(plan, {"length_step": ({(n,): n - 2 for n in range(2, N + 1)}, OUT_N(N)),
                               "full_length_step": (full, [((-1, 2), BAD_R), ((ns + 1, 2), BAD_R), ((0, 1), BAD_N), ((0, N + 1), BAD_N)])}, ns)


def test_forward_seeded_plan(hip, seed_small):
    p = seeded(seed_small, 2)
    N, L, ns = p.N, p.N - 1, 2
    rays = rays_of(p)
    with hip.Plan(p) as plan:
        c = Caller(plan, [p.seed, ss.primed(p.seed)])
        c.refuses(c.set("ase_seeds"), "rt_hip_plan_set_ase_seeds: not an emission plan (created without a seed, tables with E0)")
        c.refuses(c.set("scan_ase_seeds"), "rt_hip_plan_set_scan_ase_seeds: not an emission plan (created without a seed, tables with E0)")
        c.refuses(c.set("scan_seeds"), "rt_hip_plan_set_scan_seeds: the length scan is off (rt_hip_plan_enable_length_scan first)")
        c.validates("seeds")
        for mode in ("path", "spectra"):
            c.ok(c.enable(mode))
            c.refuses(c.set("seeds"), "rt_hip_plan_set_seeds: the path tracer or spectra mode is enabled (a set runs in step mode only)")
            c.ok(c.set("seeds", 0)).ok(c.enable(mode, 0))
        # a set held
        c.ok(c.set("seeds"))
        c.refuses(c.enable("length_scan"), "rt_hip_plan_enable_length_scan: the plan holds a seed set (a seed set and a length scan exclude each other)")
        run_step(plan, rays)
        check_accessors(plan, {"seed_step": ({(s,): s for s in range(ns)}, [((-1,), NO_SEED), ((ns,), NO_SEED)])}, ns)
        c.ok(c.set("seeds", 0))
        # the length scan on
        c.ok(c.enable("length_scan"))
        c.refuses(c.set("seeds"), "rt_hip_plan_set_seeds: the length scan is on (a seed set and a length scan exclude each other)")
        c.ok(c.set("seeds", 0))                           # (no set to remove: accepted, as before)
        c.validates("scan_seeds")
        c.ok(c.set("scan_seeds"))
        c.ok(c.set("seeds", 0))                           # (the seeds of the scan are not a set: they stay)
        plan.run()
        both = {(s, n): s * L + n - 2 for s in range(ns) for n in range(2, N + 1)}
        check_accessors(plan, {"length_step": ({(n,): n - 2 for n in range(2, N + 1)}, OUT_N(N)),
                               "seed_length_step": (both, [((-1, 2), NO_SCAN_SEED), ((ns, 2), NO_SCAN_SEED), ((0, 1), BAD_N), ((0, N + 1), BAD_N)])}, ns)


def test_backward_seeded_plan(hip, seed_small):
    p = seeded(seed_small, 1)
    N = p.N
    rays = rays_of(p)
    with hip.Plan(p) as plan:
        c = Caller(plan, [p.seed, ss.primed(p.seed)])
        c.refuses(c.set("suffix_ase_seeds"), "rt_hip_plan_set_suffix_ase_seeds: the plan was created with a seed (the ASE record needs an emission plan)")
        c.ok(c.set("seeds"))
        c.refuses(c.enable("suffix_scan"), "rt_hip_plan_enable_suffix_scan: the plan holds a seed set (a seed set and a suffix scan exclude each other)")
        c.ok(c.set("seeds", 0))
        c.ok(c.enable("suffix_scan"))
        c.refuses(c.set("seeds"), "rt_hip_plan_set_seeds: the suffix scan is on (a seed set and a suffix scan exclude each other)")
        c.refuses(c.set("scan_seeds"), "rt_hip_plan_set_scan_seeds: the suffix scan is on (it takes no scan seeds)")
        run_step(plan, rays)
        check_accessors(plan, {"length_step": ({(n,): n - 2 for n in range(2, N + 1)}, OUT_N(N))}, 0)


@pytest.mark.parametrize("method, scan", [(2, "length_scan"), (1, "suffix_scan")])
def test_more_lengths_than_a_scan_takes(hip, ase_small, method, scan):
    """The smallest N beyond RT_N_SCAN_MAX + 1; the plan is created and never run."""
    p = emission(ase_small, method, N=cabi.RT_N_SCAN_MAX + 2)
    with hip.Plan(p) as plan:
        c = Caller(plan, [])
        c.refuses(c.enable(scan), f"rt_hip_plan_enable_{scan}: more than RT_N_SCAN_MAX lengths")
        c.ok(c.enable(scan, 0))
