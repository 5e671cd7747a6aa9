"""The accessors of the records of a step run (rt_hip_plan_fetch_*_step / rt_hip_plan_*_step_ptrs), every pair against
every kind of last run.  The kind test and the index -> block mapping live in one place (csrc/rt_records.h, RecordSet);
this is its matrix on the device.

Inputs: seed_scan.p450(seed_small, N=4) -- 450 rays, THREE lengths and TWO seeds, so that s * L and s * n_seed differ and a
transposed mapping cannot pass -- and ase_seeds.base(ase_small, 2, N=3) with ase_seeds.seeds_of (1 440 rays).

After every run, for the four accessor pairs:
    * a pair of another kind answers RT_ERR_ARG with its "the last run was not ..." text -- but for length_step after a scan
      with seeds, which is seed_length_step(0, n) in pointers, bits and code;
    * the pair of the run's own kind answers RT_ERR_ARG for every index just outside the set;
    * for every valid index the pointers are block 0's + block * stride (block numbers: seed s -> s, length n -> n - 2,
      (s, n) -> s L + n - 2, ASE record r -> r; offsets and stride worked out here from the beam's sizes), and what the fetch
      returns is bit for bit what a torch read of those pointers gives afterwards;
    * step_ptrs() and fetch_step() are the primary record: block 0 of a set and of ASE seeds, block L - 1 of a scan.
Nothing here provokes a failure code."""
import ctypes as C
import importlib

import numpy as np
import pytest

import ase_seeds as A
import seed_scan as ss

rt = importlib.import_module("raytrace-miniapp_amd")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

KEYS = ("E_v", "nf", "I_ang")
# pair -> (fetch entry, pointer entry, what both say after a run of another kind, an index that a run of its kind has)
PAIRS = {
    "seed": ("rt_hip_plan_fetch_seed_step", "rt_hip_plan_seed_step_ptrs", "the last run was not a step run with a seed set", (0,)),
    "length": ("rt_hip_plan_fetch_length_step", "rt_hip_plan_length_step_ptrs", "the last run was not a step run with the length scan on", (2,)),
    "full": ("rt_hip_plan_fetch_full_step", "rt_hip_plan_full_step_ptrs",
             "the last run was not a step run of an emission plan with ASE seeds", (0,)),
    "seed_length": ("rt_hip_plan_fetch_seed_length_step", "rt_hip_plan_seed_length_step_ptrs",
                    "the last run was not a step run of a length scan with scan seeds", (0, 2)),
}


def ptrs_of(plan, pair, *index):
    """(status, (E_v, nf, I_ang) device pointers, error text)"""
    e, n, a = C.c_void_p(), C.c_void_p(), C.c_void_p()
    lib = plan.hl.lib
    rc = getattr(lib, PAIRS[pair][1])(plan._h, *index, C.byref(e), C.byref(n), C.byref(a))
    return rc, (int(e.value or 0), int(n.value or 0), int(a.value or 0)), lib.rt_hip_last_error().decode()


def fetch_of(plan, pair, *index):
    """(status, dict(E_v, nf, I_ang, failure_code), error text)"""
    b = plan.problem.beam
    out = dict(E_v=np.full(b.nv, np.nan), nf=np.full(b.nx * b.ny, np.nan), I_ang=np.full(b.na * b.nb, np.nan))
    code = C.c_uint(0xffffffff)
    lib = plan.hl.lib
    rc = getattr(lib, PAIRS[pair][0])(plan._h, *index, cabi._dp(out["E_v"]), cabi._dp(out["nf"]), cabi._dp(out["I_ang"]), C.byref(code))
    out["failure_code"] = code.value
    return rc, out, lib.rt_hip_last_error().decode()


class _Dev:  # the CUDA array interface, which torch.as_tensor reads
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="<f8", data=(ptr, False), version=2, strides=None)


def read_device(plan, ptrs):
    """E_v, nf and I_ang as a torch read of the three pointers gives them"""
    import torch

    b = plan.problem.beam
    sizes = (b.nv, b.nx * b.ny, b.na * b.nb)
    return {k: torch.as_tensor(_Dev(p, n), device=torch.device("cuda", plan.device)).cpu().numpy() for k, p, n in zip(KEYS, ptrs, sizes)}


def block_layout(b):
    """(nf offset, I_ang offset, stride) of a block in bytes: E_v [nv] | pad to 256 bytes | nf [nx * ny] | I_ang [na * nb],
    the block padded to 256 bytes; an axis of one point brings spare cells (none of these inputs has one)."""
    assert min(b.nx, b.ny, b.na, b.nb) >= 2
    nf_off = (b.nv * 8 + 255) // 256 * 256
    ang_off = nf_off + b.nx * b.ny * 8
    return nf_off, ang_off, (ang_off + b.na * b.nb * 8 + 255) // 256 * 256


def refused(plan, pair, index, text):
    for rc, _, err in (ptrs_of(plan, pair, *index), fetch_of(plan, pair, *index)):
        assert rc == cabi.RT_ERR_ARG and text in err, (pair, index, rc, err)


def check_accessors(plan, own, n_seed, N):
    """The whole matrix after a run of kind `own` (None: a plain step run) with n_seed seeds and N - 1 lengths."""
    L = N - 1
    valid = {None: {},
             "seed": {(s,): s for s in range(n_seed)},
             "full": {(r,): r for r in range(1 + n_seed)},
             "length": {(n,): n - 2 for n in range(2, N + 1)},
             "seed_length": {(s, n): s * L + n - 2 for s in range(n_seed) for n in range(2, N + 1)}}[own]
    outside = {None: [], "seed": [(-1,), (n_seed,)], "full": [(-1,), (n_seed + 1,)], "length": [(1,), (N + 1,)],
               "seed_length": [(-1, 2), (n_seed, 2), (0, 1), (0, N + 1)]}[own]
    primary = L - 1 if own in ("length", "seed_length") else 0
    # 1. the pairs of the other kinds
    for pair, (_, _, text, index) in PAIRS.items():
        if pair != own and not (pair == "length" and own == "seed_length"):
            refused(plan, pair, index, text)
    # 2. its own pair: outside the set
    for index in outside:
        word = "r must be" if own == "full" else "no such seed" if own == "seed" or (own == "seed_length" and index[1] == 2) else "n must be"
        refused(plan, own, index, word)
    # 3. ... and every record of the set
    nf_off, ang_off, stride = block_layout(plan.problem.beam)
    base, fetched = None, {}
    for index, block in sorted(valid.items(), key=lambda kv: kv[1]):
        rc, ptrs, err = ptrs_of(plan, own, *index)
        assert rc == cabi.RT_OK, (own, index, err)
        if base is None:
            assert block == 0
            base = ptrs[0]
            assert base % 256 == 0
        assert ptrs == (base + block * stride, base + block * stride + nf_off, base + block * stride + ang_off), (own, index, block)
        rc, rec, err = fetch_of(plan, own, *index)
        assert rc == cabi.RT_OK and rec["failure_code"] == 0, (own, index, err, rec["failure_code"])
        dev = read_device(plan, ptrs)
        for key in KEYS:
            assert np.array_equal(rec[key], dev[key]) and np.isfinite(rec[key]).all(), (own, index, key)
        assert rec["E_v"].any() and rec["nf"].any() and rec["I_ang"].any(), (own, index)
        fetched[block] = (ptrs, rec)
    assert len(fetched) == len(valid) and (own is None or sorted(fetched) == list(range(len(valid))))
    for i in fetched:   # no two blocks hold the same record: a mapping that serves one block twice cannot pass
        for j in fetched:
            assert i >= j or not np.array_equal(fetched[i][1]["E_v"], fetched[j][1]["E_v"]), (own, i, j)
    # 4. a length alone after a scan with seeds: seed 0's curve
    if own == "seed_length":
        for n in range(2, N + 1):
            want_ptrs, want = fetched[n - 2]
            rc, ptrs, err = ptrs_of(plan, "length", n)
            assert rc == cabi.RT_OK and ptrs == want_ptrs, (n, err)
            rc, rec, err = fetch_of(plan, "length", n)
            assert rc == cabi.RT_OK and rec["failure_code"] == want["failure_code"], (n, err)
            for key in KEYS:
                assert np.array_equal(rec[key], want[key]), (n, key)
        for index in [(1,), (N + 1,)]:
            refused(plan, "length", index, "n must be")
    # 5. step_ptrs() and fetch_step(): the primary record
    step = plan.fetch_step()
    if own is None:
        dev = read_device(plan, plan.step_ptrs() + (plan.iang_ptr,))
        for key in KEYS:
            assert np.array_equal(step[key], dev[key]) and step[key].any(), key
    else:
        ptrs, rec = fetched[primary]
        assert plan.step_ptrs() == ptrs[:2]
        for key in KEYS:
            assert np.array_equal(step[key], rec[key]), (own, key)
        assert np.array_equal(plan.fetch()["I_ang"], rec["I_ang"])


def run_p450(plan, pa, pb, kind):
    plan.set_ray_grid().enable_step()
    if kind in ("length", "seed_length"):
        plan.enable_length_scan()
    if kind == "seed_length":
        plan.set_scan_seeds([pa.seed, pb.seed])
    if kind == "seed":
        plan.set_seeds([pa.seed, pb.seed])
    plan.run()
    info = plan.fetch()
    assert info["failure_code"] == 0 and info["stats"]["n_rays"] == 450


@pytest.mark.parametrize("kind", [None, "seed", "length", "seed_length"])
def test_accessors_after_a_run_of_every_kind_on_a_seeded_plan(hip, seed_small, kind):
    pa, pb = ss.p450(seed_small, N=4)
    assert pa.N == 4 and pa.n_rays_total == 450
    with hip.Plan(pa) as plan:
        run_p450(plan, pa, pb, kind)
        check_accessors(plan, kind, 2 if kind in ("seed", "seed_length") else 0, pa.N)


def test_accessors_after_a_run_with_ase_seeds(hip, ase_small):
    p = A.base(ase_small, 2, N=3)
    seeds = A.seeds_of(p)
    with hip.Plan(p) as plan:
        plan.set_ray_grid().set_ase_seeds(seeds, [A.carry(p, s).scale for s in seeds]).enable_step().run()
        info = plan.fetch()
        assert info["failure_code"] == 0 and info["stats"]["n_rays"] == 1440
        check_accessors(plan, "full", 2, p.N)


def test_accessors_follow_the_last_run(hip, seed_small):
    """One plan: a scan with seeds, then the scan off and a seed set installed."""
    pa, pb = ss.p450(seed_small, N=4)
    with hip.Plan(pa) as plan:
        run_p450(plan, pa, pb, "seed_length")
        check_accessors(plan, "seed_length", 2, pa.N)
        plan.enable_length_scan(False).set_seeds([pa.seed, pb.seed]).run()
        assert plan.fetch()["failure_code"] == 0
        check_accessors(plan, "seed", 2, pa.N)
