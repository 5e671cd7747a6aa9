"""Every refusal of the per-ray spectra entry points of the C ABI, by its full text, and the rows they serve, by address.

The two switches (rt_hip_plan_enable_spectra, rt_hip_plan_enable_length_spectra), the two installers
(rt_hip_plan_set_spectra_seeds, rt_hip_plan_set_spectra_ase_seeds) and the five accessor pairs (rt_hip_plan_fetch_spectra /
rt_hip_plan_spectra_ptr, rt_hip_plan_fetch_<pair> / rt_hip_plan_<pair>_ptrs for seed_spectra, full_spectra, length_spectra and
seed_length_spectra) are called through the raw C ABI -- the Python checks of backend.Plan are not in the way -- and
rt_hip_last_error() is compared, whole, with a literal written here (the pattern of tests/test_gpu_record_refusals.py).  Every
refusal is RT_ERR_ARG before any launch; nothing here provokes a fault.

Plans: ASE_small (emission; on the 12 x 6 x 5 x 4 beam of tests/spectra_ase_seeds.py, K = 52) and seed_small (seeded, K = 82),
both at N = 3: L = 2, lengths n = 2, 3.  Rays: a list of 70 -- one full tile and a ragged one; a block stride of 70 cannot be
mistaken for 64 or 128.  Two seeds where seeds are installed: `wide` and `narrow` of tests/ase_seeds.py on the emission plan, the
plan's own seed and the `narrow` profile of tests/seed_profiles.py on the seeded one.  Seven runs, one per kind of rows:

    plain spectra (emission)   plain spectra (seeded)   spectra seeds   ASE seeds
    length spectra (emission, forward)   length spectra (seeded, backward)   length spectra with seeds

After each: the pairs of the other kinds refuse, the own ones refuse every index one outside the set -- in the order the
checks are made -- and serve every index inside it: the pointers are block 0's + block x stride (ray2: one block in spectra
mode, one per length in length spectra), block 0 lies as the allocation of the run lays it out, and a fetch is bit for bit a
read of those pointers, with every output NULL in turn.

Recorded here, because it is what callers rely on today: rt_hip_plan_fetch_spectra / rt_hip_plan_spectra_ptr serve block 0 of
all three spectra-mode kinds and refuse after length spectra; rt_hip_plan_fetch_length_spectra serves seed 0 of a length-spectra
run with seeds."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import ase_seeds as A
import length_scan as ls
import method_pairs as mp
import seed_profiles as SP
import seed_scan as sc
import spectra_ase_seeds as S

rt = importlib.import_module("raytrace-miniapp_amd")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

N_RAYS = 70
RAY_BYTES = 16      # sizeof(rt_ray): four floats
KEYS = ("Iv", "ray2", "err")

# accessor pair -> (number of indices, what both say after a run of another kind)
NOT_LENGTH = "the last run was not a length-spectra run (or length spectra have been switched off since)"
PAIRS = {
    "spectra": (0, "the last run was not a spectra run"),
    "seed_spectra": (1, "the last run was not a spectra run with spectra seeds"),
    "full_spectra": (1, "the last run was not a spectra run with ASE seeds"),
    "length_spectra": (1, NOT_LENGTH),
    "seed_length_spectra": (2, NOT_LENGTH),
}
BAD_S = "s must be 0 .. n_seed - 1 of the last run"
BAD_R = "r must be 0 .. n_seed of the last run"
BAD_N = "n must be 2 .. N of the last run"
NO_SEEDS = "the last run carried no spectra seeds"
VALIDATE = (": n_seed must be 0 .. RT_N_SEED_MAX", ": NULL seeds", ": incomplete seed table", ": seed.dim[4] != beam.nv")
NEITHER_ON = ("rt_hip_plan_set_spectra_seeds: neither spectra mode nor length spectra are on "
              "(rt_hip_plan_enable_spectra or rt_hip_plan_enable_length_spectra first)")


# ---------------------------------------------------------------------------------------------- the raw calls
def entries(pair):
    return "rt_hip_plan_fetch_" + pair, ("rt_hip_plan_spectra_ptr" if pair == "spectra" else "rt_hip_plan_" + pair + "_ptrs")


def ptrs_of(plan, pair, index):
    """(rc, (Iv, ray2, err) device addresses, text); rt_hip_plan_spectra_ptr answers Iv alone, NULL where it refuses."""
    lib = plan.hl.lib
    if pair == "spectra":
        iv = int(lib.rt_hip_plan_spectra_ptr(plan._h) or 0)
        return (cabi.RT_OK if iv else cabi.RT_ERR_ARG), (iv, 0, 0), None
    iv, r2, er = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = getattr(lib, entries(pair)[1])(plan._h, *index, C.byref(iv), C.byref(r2), C.byref(er))
    return rc, (int(iv.value or 0), int(r2.value or 0), int(er.value or 0)), lib.rt_hip_last_error().decode()


def sentinel_rows(K, n):
    return dict(Iv=np.full((n, K), -7.5), ray2=np.full((n, 4), -7.5, np.float32).view(cabi.RAY_DTYPE).reshape(n), err=np.full(n, -77, np.int32))


def fetch_of(plan, pair, index, skip=None, n=N_RAYS):
    """(rc, rows, text) of the fetch into buffers of n rows filled with a sentinel; the output `skip` is passed as NULL."""
    out = sentinel_rows(plan.problem.beam.nv, n)
    args = (cabi._dp(out["Iv"]), cabi.rays_ptr(out["ray2"]), out["err"].ctypes.data_as(C.POINTER(C.c_int32)))
    args = [None if k == skip else a for k, a in zip(KEYS, args)]
    lib = plan.hl.lib
    rc = getattr(lib, entries(pair)[0])(plan._h, *index, *args)
    return rc, out, lib.rt_hip_last_error().decode()


def access_refused(plan, pair, index, text):
    fetch, ptrs = entries(pair)
    rc, _, err = fetch_of(plan, pair, index)
    assert rc == cabi.RT_ERR_ARG and err == f"{fetch}: {text}", (pair, index, rc, err)
    rc, got, err = ptrs_of(plan, pair, index)
    assert rc == cabi.RT_ERR_ARG and (err is None or err == f"{ptrs}: {text}"), (pair, index, rc, err)
    assert pair != "spectra" or got[0] == 0


class _Dev:  # the CUDA array interface, which torch.as_tensor reads
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=2, strides=None)


def read_device(plan, ptrs, n=N_RAYS):
    import torch

    K = plan.problem.beam.nv
    dev = torch.device("cuda", plan.device)
    shapes = dict(Iv=((n, K), "<f8"), ray2=((n, 4), "<f4"), err=((n,), "<i4"))
    got = {k: torch.as_tensor(_Dev(p, *shapes[k]), device=dev).cpu().numpy() for k, p in zip(KEYS, ptrs)}
    got["ray2"] = np.ascontiguousarray(got["ray2"]).view(cabi.RAY_DTYPE).reshape(n)
    return got


def same_rows(a, b, keys=KEYS):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


# ---------------------------------------------------------------------------------------------- layout and service
def align_up(v, a):
    return (v + a - 1) // a * a


def block0_layout(K, n_blocks, n_ray2_blocks, n=N_RAYS):
    """(ray2 - Iv, err - Iv) in bytes of the allocation of a run: Iv [n_blocks][n][K] | ray2 [n_ray2_blocks][n] | err [n_blocks][n],
    the first two padded by 16 bytes and to 256.  (Spectra mode keeps room for n_blocks blocks of ray2 and writes one: the
    callers below pass n_blocks for both.)"""
    iv_bytes = align_up(n_blocks * n * K * 8 + 16, 256)
    return iv_bytes, iv_bytes + align_up(n_ray2_blocks * n * RAY_BYTES + 16, 256)


def block0_of(plan, n_blocks, n_ray2_blocks, pair, index):
    """Block 0 of the last run: (Iv, ray2, err) from `pair` at `index` (the spectra pair: Iv, the others by the layout)."""
    K = plan.problem.beam.nv
    r2_off, err_off = block0_layout(K, n_blocks, n_ray2_blocks)
    rc, base, err = ptrs_of(plan, pair, index)
    assert rc == cabi.RT_OK and base[0] and base[0] % 256 == 0, (pair, index, err)
    if pair == "spectra":
        base = (base[0], base[0] + r2_off, base[0] + err_off)
    assert (base[1] - base[0], base[2] - base[0]) == (r2_off, err_off), (pair, index, base)
    return base


def serves(plan, pair, valid, base, lengths):
    """Every index of `valid` ({index: block}) is served: the pointers are block 0's + block x stride, the fetch a read of them."""
    K = plan.problem.beam.nv
    for index, block in valid.items():
        want = (base[0] + block * N_RAYS * K * 8, base[1] + ((index[-1] - 2) * N_RAYS * RAY_BYTES if lengths else 0), base[2] + block * N_RAYS * 4)
        rc, ptrs, err = ptrs_of(plan, pair, index)
        assert rc == cabi.RT_OK, (pair, index, err)
        assert ptrs == (want if pair != "spectra" else (want[0], 0, 0)), (pair, index, block)
        if pair != "spectra":                               # any pointer may be NULL
            assert getattr(plan.hl.lib, entries(pair)[1])(plan._h, *index, None, None, None) == cabi.RT_OK
        dev = read_device(plan, want)
        rc, rows, err = fetch_of(plan, pair, index)
        assert rc == cabi.RT_OK and same_rows(rows, dev), (pair, index, err)
        assert not (rows["err"] == -77).any()
        for skip in KEYS:                                   # a NULL output is skipped, the others are written
            rc, rows, err = fetch_of(plan, pair, index, skip)
            assert rc == cabi.RT_OK and same_rows(rows, dev, [k for k in KEYS if k != skip]), (pair, index, skip, err)


def check_accessors(plan, own, base=None, lengths=False):
    """After a run whose rows the pairs `own` serve ({pair: ({index: block}, [(index outside, text)])}): every other pair
    refuses by the kind, the own ones refuse outside the set, in this order, and serve the set."""
    for pair, (n_index, text) in PAIRS.items():
        if pair not in own:
            access_refused(plan, pair, ((), (0,), (0, 2))[n_index] if pair != "length_spectra" else (2,), text)
    for pair, (valid, outside) in own.items():
        for index, text in outside:
            access_refused(plan, pair, index, text)
        serves(plan, pair, valid, base, lengths)


def spectra_mode_blocks(plan, n_blocks, pair=None, outside=()):
    """The three spectra-mode kinds: the plain pair serves block 0, `pair` every block."""
    own = {"spectra": ({(): 0}, [])}
    if pair:
        own[pair] = ({(b,): b for b in range(n_blocks)}, list(outside))
    base = block0_of(plan, n_blocks, n_blocks, pair or "spectra", (0,) if pair else ())
    assert base[0] == block0_of(plan, n_blocks, n_blocks, "spectra", ())[0]
    check_accessors(plan, own, base)


def length_blocks(plan, N, n_seed):
    """The two length kinds: n alone serves seed 0 (block n - 2), (s, n) block s L + n - 2 where the run carried seeds."""
    L = N - 1
    out_n = [((1,), BAD_N), ((N + 1,), BAD_N)]
    both = {(s, n): s * L + n - 2 for s in range(n_seed) for n in range(2, N + 1)}
    # a bad n is reported before a bad s, "no spectra seeds" before the range of s
    outside = [((0, 1), BAD_N), ((0, N + 1), BAD_N), ((-1, 1), BAD_N), ((n_seed, N + 1), BAD_N)]
    outside += [((-1, 2), BAD_S), ((n_seed, 2), BAD_S), ((n_seed, N), BAD_S)] if n_seed else [((0, 2), NO_SEEDS), ((-1, 2), NO_SEEDS), ((0, N), NO_SEEDS)]
    base = block0_of(plan, max(n_seed, 1) * L, L, "length_spectra", (2,))
    check_accessors(plan, {"length_spectra": ({(n,): n - 2 for n in range(2, N + 1)}, out_n), "seed_length_spectra": (both, outside)}, base, True)


# ---------------------------------------------------------------------------------------------- inputs
def emission(ase_small, method, N=3):
    p = S.problem_of(ase_small, method, 3)
    if N == 2:
        p = mp.with_method(ls.prefix(p, 2), method)
    elif N != 3:
        p = mp.with_method(ls.scan_problem(p, N), method)
    assert p.seed is None and p.use_emis and p.method == method and p.N == N
    return p


def seeded(seed_small, method):
    p = mp.with_method(seed_small, method)
    assert p.seed is not None and not p.use_emis and p.method == method and p.N == 3
    return p


def seeded_seeds(p, seed_small):
    return [p.seed, sc.primed(SP.e2e_problem(seed_small, "narrow").seed)]


def rays_of(p, n=N_RAYS):
    rays = p.build_rays(np.arange(n, dtype=np.int64) * (p.n_rays_total // n))
    assert len(rays) == n
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

    def _text(self, rc):
        return rc, self.lib.rt_hip_last_error().decode()

    def set(self, name, n_seed=None, arr="own"):
        fn = getattr(self.lib, "rt_hip_plan_set_" + name)
        n_seed = len(self.seeds) if n_seed is None else n_seed
        a = (self.arr if n_seed > 0 else None) if isinstance(arr, str) else arr
        if name in ("ase_seeds", "scan_ase_seeds", "suffix_ase_seeds"):
            return self._text(fn(self.h, n_seed, a, None))
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
        """The refusals of the seed tables, as both installers word them behind their own names (too many seeds has a text of
        its own, before the tables are looked at)."""
        who = "rt_hip_plan_set_" + name
        self.refuses(self.set(name, cabi.RT_N_SEED_MAX + 1), who + ": more than RT_N_SEED_MAX seeds")
        self.refuses(self.set(name, -1), who + VALIDATE[0])
        self.refuses(self.set(name, 1, None), who + VALIDATE[1])
        short, keep = seed_array(self.seeds[:1])
        short[0].dim[0] = 1
        self.refuses(self.set(name, 1, short), who + VALIDATE[2])
        nv, keep2 = seed_array(self.seeds[:1])
        nv[0].dim[4] = nv[0].dim[4] - 1
        self.refuses(self.set(name, 1, nv), who + VALIDATE[3])
        return self


def run(plan):
    plan.run()
    info = plan.fetch(want_image=False)
    assert info["stats"]["n_rays"] == N_RAYS
    return info


# ---------------------------------------------------------------------------------------------- 1 - 6: the seven runs
def test_emission_plan(hip, ase_small):
    """Plain spectra, spectra with ASE seeds and length spectra (forward) on one emission plan, with the switches and the
    installer of ASE seeds on the way."""
    p = emission(ase_small, 2)
    N, ns = p.N, 2
    with hip.Plan(p) as plan:
        c = Caller(plan, S.seeds_of(p))
        plan.set_rays(rays_of(p))
        check_accessors(plan, {})                          # no run yet
        # the installers on a plan whose modes are off, and the one a seeded plan takes
        c.refuses(c.set("spectra_ase_seeds"), "rt_hip_plan_set_spectra_ase_seeds: spectra mode is off (rt_hip_plan_enable_spectra first)")
        c.refuses(c.set("spectra_ase_seeds", 0), "rt_hip_plan_set_spectra_ase_seeds: spectra mode is off (rt_hip_plan_enable_spectra first)")
        c.refuses(c.set("spectra_seeds"), "rt_hip_plan_set_spectra_seeds: the plan was created without a seed "
                  "(an emission plan: per-ray spectra with ASE seeds are not built)")
        # the switches against every other mode
        c.ok(c.enable("path"))
        c.refuses(c.enable("spectra"), "rt_hip_plan_enable_spectra: the path tracer is enabled (one per-ray output at a time)")
        c.refuses(c.enable("length_spectra"), "rt_hip_plan_enable_length_spectra: the path tracer is enabled (one per-ray output at a time)")
        c.ok(c.enable("spectra", 0)).ok(c.enable("length_spectra", 0)).ok(c.enable("path", 0))
        c.ok(c.enable("step"))
        c.refuses(c.enable("spectra"), "rt_hip_plan_enable_spectra: the plan is in step mode (one output mode at a time)")
        c.refuses(c.enable("length_spectra"), "rt_hip_plan_enable_length_spectra: the plan is in step mode (one output mode at a time)")
        c.ok(c.enable("step", 0))
        c.ok(c.set("ase_seeds"))                           # ASE seeds of step mode held
        c.refuses(c.enable("spectra"), "rt_hip_plan_enable_spectra: the plan holds a seed set (step mode only)")
        c.refuses(c.enable("length_spectra"), "rt_hip_plan_enable_length_spectra: the plan holds ASE seeds (length spectra take the creation seed alone)")
        c.ok(c.set("ase_seeds", 0))
        c.ok(c.enable("length_scan"))
        c.refuses(c.enable("spectra"), "rt_hip_plan_enable_spectra: the length scan is on (step mode only)")
        c.refuses(c.enable("length_spectra"), "rt_hip_plan_enable_length_spectra: the length scan is on (it leaves step records, not spectra)")
        c.ok(c.enable("length_scan", 0))
        # run 1: plain spectra
        c.ok(c.enable("spectra"))
        c.refuses(c.enable("length_spectra"), "rt_hip_plan_enable_length_spectra: the plan is in spectra mode (length spectra are a mode of their own)")
        run(plan)
        spectra_mode_blocks(plan, 1)
        # run 4: spectra with ASE seeds
        c.validates("spectra_ase_seeds")
        c.ok(c.set("spectra_ase_seeds"))
        run(plan)
        spectra_mode_blocks(plan, 1 + ns, "full_spectra", [((-1,), BAD_R), ((ns + 1,), BAD_R)])
        # spectra mode off: its seeds are gone with it
        c.ok(c.enable("spectra", 0))
        c.refuses(c.set("spectra_ase_seeds", 0), "rt_hip_plan_set_spectra_ase_seeds: spectra mode is off (rt_hip_plan_enable_spectra first)")
        c.ok(c.enable("spectra"))
        run(plan)                                          # the plain plan again: one block
        access_refused(plan, "full_spectra", (0,), PAIRS["full_spectra"][1])
        assert fetch_of(plan, "spectra", ())[0] == cabi.RT_OK
        c.ok(c.enable("spectra", 0))
        # run 5: length spectra, forward
        c.ok(c.enable("length_spectra"))
        c.refuses(c.enable("spectra"), "rt_hip_plan_enable_spectra: length spectra are on (a mode of their own: rt_hip_plan_enable_length_spectra switches them off)")
        c.refuses(c.set("spectra_ase_seeds"), "rt_hip_plan_set_spectra_ase_seeds: length spectra are on (per-ray ASE seeds at every length are not built)")
        before = run(plan)
        length_blocks(plan, N, 0)
        # switched off: the rows are gone, the report and the counters of that run are not
        c.ok(c.enable("length_spectra", 0))
        check_accessors(plan, {})
        after = plan.fetch(want_image=False)
        counters = lambda info: {k: v for k, v in info["stats"].items() if not k.endswith("_ms")}    # (total_ms is the wall clock)
        assert after["failure_code"] == before["failure_code"] and counters(after) == counters(before)
        assert after["failed_rays"].tobytes() == before["failed_rays"].tobytes()


def test_seeded_plans(hip, seed_small):
    """Plain spectra and spectra with spectra seeds on the forward plan; length spectra and length spectra with seeds on the
    backward one."""
    p = seeded(seed_small, 2)
    N, ns = p.N, 2
    with hip.Plan(p) as plan:
        c = Caller(plan, seeded_seeds(p, seed_small))
        plan.set_rays(rays_of(p))
        c.refuses(c.set("spectra_seeds"), NEITHER_ON)
        c.refuses(c.set("spectra_seeds", 0), NEITHER_ON)
        c.refuses(c.set("spectra_ase_seeds"), "rt_hip_plan_set_spectra_ase_seeds: the plan was created with a seed (a seeded plan takes rt_hip_plan_set_spectra_seeds)")
        c.ok(c.set("seeds"))                               # a seed set held
        c.refuses(c.enable("spectra"), "rt_hip_plan_enable_spectra: the plan holds a seed set (step mode only)")
        c.refuses(c.enable("length_spectra"), "rt_hip_plan_enable_length_spectra: the plan holds a seed set (length spectra take the creation seed alone)")
        c.ok(c.set("seeds", 0))
        # run 2: plain spectra
        c.ok(c.enable("spectra"))
        run(plan)
        spectra_mode_blocks(plan, 1)
        # run 3: spectra with spectra seeds
        c.validates("spectra_seeds")
        c.ok(c.set("spectra_seeds"))
        run(plan)
        spectra_mode_blocks(plan, ns, "seed_spectra", [((-1,), BAD_S), ((ns,), BAD_S)])
        c.ok(c.enable("spectra", 0))                       # the seeds are gone with the mode
        c.refuses(c.set("spectra_seeds", 0), NEITHER_ON)
    p = seeded(seed_small, 1)
    with hip.Plan(p) as plan:
        c = Caller(plan, seeded_seeds(p, seed_small))
        plan.set_rays(rays_of(p))
        c.ok(c.enable("suffix_scan"))
        c.refuses(c.enable("spectra"), "rt_hip_plan_enable_spectra: the suffix scan is on (step mode only)")
        c.refuses(c.enable("length_spectra"), "rt_hip_plan_enable_length_spectra: the suffix scan is on (it leaves step records, not spectra)")
        c.ok(c.enable("suffix_scan", 0))
        # run 6: length spectra, backward
        c.ok(c.enable("length_spectra"))
        run(plan)
        length_blocks(plan, N, 0)
        # run 7: length spectra with seeds
        c.ok(c.set("spectra_seeds"))
        run(plan)
        length_blocks(plan, N, ns)
        c.ok(c.enable("length_spectra", 0))                # the rows and the seeds are gone with the mode
        check_accessors(plan, {})
        c.refuses(c.set("spectra_seeds", 0), NEITHER_ON)
        c.ok(c.enable("length_spectra"))
        run(plan)
        length_blocks(plan, N, 0)                          # the creation seed alone again


def test_null_plans_and_tables_without_E0(hip, ase_small):
    lib = hip.HipLibrary.get().lib
    for name, args in (("enable_spectra", (1,)), ("enable_length_spectra", (1,)), ("set_spectra_seeds", (0, None)), ("set_spectra_ase_seeds", (0, None))):
        assert getattr(lib, "rt_hip_plan_" + name)(None, *args) == cabi.RT_ERR_ARG
        assert lib.rt_hip_last_error().decode() == f"rt_hip_plan_{name}: NULL plan"
    p = emission(ase_small, 2)
    q = copy.copy(p)
    q.gain = [rt.Gain(g.x, g.y, g.n, g.g0, None, g.gv, g.Nv) for g in p.gain]
    q = mp.with_method(q, 2)
    assert not q.use_emis and q.seed is None
    with hip.Plan(q) as plan:                              # neither a seed nor E0
        c = Caller(plan, S.seeds_of(p))
        c.ok(c.enable("spectra"))
        c.refuses(c.set("spectra_ase_seeds"), "rt_hip_plan_set_spectra_ase_seeds: not an emission plan (tables without E0)")


@pytest.mark.parametrize("N, text", [(2, "N < 3 (one length: spectra mode is the whole curve)"), (cabi.RT_N_SCAN_MAX + 2, "more than RT_N_SCAN_MAX lengths")])
def test_lengths_that_length_spectra_do_not_take(hip, ase_small, N, text):
    """One length, and the smallest N beyond RT_N_SCAN_MAX + 1; the plans are created and never run."""
    with hip.Plan(emission(ase_small, 2, N)) as plan:
        c = Caller(plan, [])
        c.refuses(c.enable("length_spectra"), "rt_hip_plan_enable_length_spectra: " + text)
        c.ok(c.enable("length_spectra", 0))


# ---------------------------------------------------------------------------------------------- 7. the report
def pick(fail, n_bad=40, n=N_RAYS):
    """Indices of n_bad failing and n - n_bad clean candidates, a clean one before each of the first failing ones: more failing
    rays than the report holds, and the first of them are not simply the first rays of the list."""
    bad, good = np.flatnonzero(fail), np.flatnonzero(~fail)
    assert len(bad) >= n_bad and len(good) >= n - n_bad, (len(bad), len(good))
    n_good = n - n_bad
    take = np.concatenate([np.stack([good[:n_good], bad[:n_good]], axis=1).reshape(-1), bad[n_good:n_bad]])
    assert len(take) == n and len(set(take.tolist())) == n
    return take


def check_report(info, err_blocks, rays):
    """The first RT_N_FAILED_MAX failing rays in list order; a ray fails if any block holds a non-zero code."""
    failing = np.zeros(len(rays), bool)
    for err in err_blocks:
        failing |= err != 0
    print(f"failing rays {int(failing.sum())} of {len(rays)}, reported {len(info['failed_rays'])}")
    assert int(failing.sum()) > cabi.RT_N_FAILED_MAX and not failing.all()
    assert not failing[:cabi.RT_N_FAILED_MAX].all()                                             # (not simply the first rays of the list)
    assert info["failed_rays"].tobytes() == rays[failing][:cabi.RT_N_FAILED_MAX].tobytes()


def test_report_order_after_spectra_with_ase_seeds(hip, ase_small):
    """negative(narrow): -2 under seed 1 only, i.e. in the LAST block of three."""
    p = emission(ase_small, 1)
    seeds = S.negative_pair(p)
    every = p.build_rays()
    with hip.Plan(p) as plan:
        plan.set_rays(every).enable_spectra().set_spectra_ase_seeds(seeds).run()
        full = plan.fetch_full_spectra()
        fail = np.zeros(len(every), bool)
        for blk in [full["ase"]] + full["seeds"]:
            fail |= blk["err"] != 0
        rays = np.ascontiguousarray(every[pick(fail)])
        plan.set_rays(rays).run()
        info = plan.fetch()
        blocks = [fetch_of(plan, "full_spectra", (r,)) for r in range(3)]
        assert all(rc == cabi.RT_OK for rc, _, _ in blocks)
        assert not blocks[0][1]["err"].any() and not blocks[1][1]["err"].any()
        check_report(info, [rows["err"] for _, rows, _ in blocks], rays)


def test_report_order_after_length_spectra_with_seeds(hip, seed_small):
    """The `narrow` profile with f[4][3] negated as seed 1: -2 in the blocks of seed 1 only, the last L of 2 L."""
    p = seeded(seed_small, 1)
    s0, s1 = seeded_seeds(p, seed_small)
    seeds = [s0, A.negative(s1)]
    cand = rays_of(p, 8192)
    with hip.Plan(p) as plan:
        plan.set_rays(cand).enable_length_spectra().set_spectra_seeds(seeds).run()
        fail = np.zeros(len(cand), bool)
        for per_seed in plan.fetch_seed_length_spectra():
            for rows in per_seed:
                fail |= rows["err"] != 0
        rays = np.ascontiguousarray(cand[pick(fail)])
        plan.set_rays(rays).run()
        info = plan.fetch()
        blocks = [fetch_of(plan, "seed_length_spectra", (s, n)) for s in range(2) for n in range(2, p.N + 1)]
        assert all(rc == cabi.RT_OK for rc, _, _ in blocks)
        assert not any(rows["err"].any() for _, rows, _ in blocks[:p.N - 1])
        check_report(info, [rows["err"] for _, rows, _ in blocks], rays)


# ---------------------------------------------------------------------------------------------- 8. the ray count of the run
def test_fetch_spectra_takes_the_ray_count_of_the_run_not_of_the_plan(hip, ase_small):
    """This test fails on the parent commit, which sizes the copies of rt_hip_plan_fetch_spectra by the plan's CURRENT ray
    count: after rt_hip_plan_set_rays with a longer list (and no run) it copies 140 rows, or fails in the copy, where the last
    run left 70.  The host buffers hold 140 rows, so neither version writes outside them."""
    p = emission(ase_small, 2)
    with hip.Plan(p) as plan:
        plan.set_rays(rays_of(p))
        c = Caller(plan, [])
        c.ok(c.enable("spectra"))
        run(plan)
        rc, first, err = fetch_of(plan, "spectra", ())
        assert rc == cabi.RT_OK, err
        ptr = ptrs_of(plan, "spectra", ())[1]
        plan.set_rays(rays_of(p, 2 * N_RAYS))              # a longer list, and no run
        rc, rows, err = fetch_of(plan, "spectra", (), n=2 * N_RAYS)
        assert rc == cabi.RT_OK, err
        untouched = sentinel_rows(p.beam.nv, N_RAYS)
        for k in KEYS:
            assert rows[k][:N_RAYS].tobytes() == first[k].tobytes(), k
            assert rows[k][N_RAYS:].tobytes() == untouched[k].tobytes(), k
        assert ptrs_of(plan, "spectra", ())[1] == ptr
