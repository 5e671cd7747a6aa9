"""The device-resident step history (include/rt_hip.h, rt_hip_plan_history_*; csrc/rt_history.hip) on the GPU.

Inputs, small on purpose (every one a time loop of 4 steps over the tables of p and table_variants.tables_b(p), alternating):
    a    ase_seeds.base(ASE_small, method): 1 440 rays, nx ny = 72 (one wave of pixels and a ragged 8), ASE seeds: 3 records
    b    one ray per pixel on a grid of more than two chunks of pixels and no whole number of them (chunk: the debug layout)
    c    a beam with ONE x point, rays at x = g[0] + dx/2 exactly: the reference's getIndex answers 1 there, so the top
         pixel row deposits into the spare cell behind nf -- which is neither copied nor summed
    d    the length scan of N = 3: 2 records
    e    a plain step plan writing E_v, nf (lent buffers, nf 8-byte aligned only) and I_ang into the caller's memory

1. copies bit for bit against a second plan that fetches every step (RT_HIP_STEP_SERIAL=1 on both: the sums of the step
   pass in a fixed order), and against that plan's own history (fetch before append); unused slots zero
2. E_sum within gamma_{n-1} of math.fsum (the bound of a sum of n non-negative doubles in ANY order); the spare cell of c
3. E_sum is the same double in every slot, on every plan, as block 0 of a set and as a plain record
4. codes and flags around a step with a NaN in the lineshape table (data, not a fault: every kernel handles it)
5. the running sum against the host fold over the device's own slabs
6. refusals leave the history as it was; release and re-create
7. history_append returns while the run is in flight
8. an append on another stream, the next run on the first
9. backend.step_history_loop against the explicit loop
The figures are printed before every assertion (ELEMENT_PARITY_FILE appends them to a file: profiles/history_parity.txt)."""
import copy
import importlib
import math
import os

import numpy as np
import pytest

import ase_seeds as A
import method_pairs as mp
import step_history as H
import table_variants as tv
from element_gate import note

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
pytestmark = pytest.mark.gpu

N_STEPS = 4
N_SLOTS = 5     # one slot more than steps: it is never appended


# ---------------------------------------------------------------------------------------------- inputs
_problems = {}


def problem_of(hip, name, ase_small, method=2):
    """(problem, kind) of a case; kind: how the plan is set up and fetched.  One object per case and session."""
    key = (name, method)
    if key in _problems:
        return _problems[key]
    if name == "a":
        out = A.base(ase_small, method), "ase"
    elif name == "b":
        chunk = H.layout(hip.HipLibrary.get(), 1, 1, 1, 1, 1, 1, 1)["chunk"]
        n = math.isqrt(2 * chunk) + 1
        p = problem_mod.regrid_beam(ase_small, nx=n, ny=n, na=1, nb=1)
        assert p.n_rays_total == n * n > 2 * chunk and (n * n) % chunk
        out = p, "plain"
    elif name == "c":
        p = mp.with_method(problem_mod.regrid_beam(ase_small, nx=1, ny=6, na=5, nb=4), 1)
        b = copy.copy(p.beam)
        # dx a power of two and x[0] a multiple of dx / 2: x[0] + dx / 2 is a float, and (x[0] + dx / 2) - dx / 2 == x[0]
        d = 2.0 ** math.floor(math.log2(b.dx))
        c = round(float(b.x[0]) / (0.5 * d)) * (0.5 * d)
        assert float(np.float32(c)) == c and float(np.float32(c + 0.5 * d)) == c + 0.5 * d and (c + 0.5 * d) - 0.5 * d == c
        b.x, b.dx = np.array([c]), d
        p = copy.copy(p)
        p.beam = b
        p.golden_image = p.golden_I_ang = None
        out = p, "spare"
    elif name == "d":
        out = A.base(ase_small, 2), "scan"
    elif name == "e":
        out = A.base(ase_small, method), "lent"
    else:
        raise KeyError(name)
    _problems[key] = out
    return out


def snapshots(p, n=N_STEPS):
    b = tv.tables_b(p)
    return [p if i % 2 == 0 else b for i in range(n)]


class Loop:
    """A plan of a case, set up for step runs; run() is one step, fetch_records() its records as [dict(E_v, nf, I_ang,
    failure_code)] by the per-record fetch calls."""

    def __init__(self, hip, p, kind, n_slots):
        import torch

        self.kind, self.p = kind, p
        self.plan = hip.Plan(p)
        self.kw = {}
        b = p.beam
        if kind == "spare":     # rays ON the edge x[0] + dx / 2 beside the grid point itself
            self.plan.set_ray_grid(first=0, stride=1, grids=(np.array([b.x[0], b.x[0] + 0.5 * b.dx]), b.y, b.a, b.b))
        else:
            self.plan.set_ray_grid()
        self.plan.enable_step()
        if kind == "ase":
            self.plan.set_ase_seeds(list(A.seeds_of(p)))
        if kind == "scan":
            self.plan.enable_length_scan()
        if kind == "lent":      # one tensor: E_v | one double | nf (8-byte aligned only) | I_ang
            npix = b.nx * b.ny
            self.buf = torch.zeros(b.nv + (b.nv % 2 == 0) + npix + b.na * b.nb, dtype=torch.float64, device="cuda")
            nf_at = b.nv + (b.nv % 2 == 0)
            ptr = self.buf.data_ptr()
            assert (ptr + 8 * nf_at) % 16 == 8
            self.plan.set_step_buffers(ptr, ptr + 8 * nf_at)
            self.kw = dict(iang_ptr=ptr + 8 * (nf_at + npix))
        self.plan.enable_history(n_slots)

    def run(self, tables=None):
        if tables is not None:
            self.plan.update_gain(tables)
        self.plan.run(**self.kw)
        return self

    def fetch_records(self):
        plan = self.plan
        if self.kind == "ase":
            full = plan.fetch_full_step()
            return [full["ase"]] + full["seeds"]
        if self.kind == "scan":
            return plan.fetch_length_steps()
        rec = plan.fetch_step()
        rec["failure_code"] = plan.fetch(want_image=False)["failure_code"]
        return [rec]

    def spare_cells(self):
        """the doubles behind nf of a plain step run on a one-point axis (nx + 2 of them)"""
        b = self.p.beam
        nf_ptr = self.plan.step_ptrs()[1]
        return hip_view(nf_ptr, b.nx * b.ny + b.nx + 2, self.plan.device)[b.nx * b.ny:]

    def close(self):
        self.plan.close()


def hip_view(ptr, n, device):
    backend = importlib.import_module("raytrace-miniapp_amd.backend")
    return backend._view(ptr, (n,), device).cpu().numpy()


class serial:
    """RT_HIP_STEP_SERIAL=1 for the runs inside: every step pass as one wave, its sums in a fixed order (every run reads it)."""

    def __enter__(self):
        self.old = os.environ.get("RT_HIP_STEP_SERIAL")
        os.environ["RT_HIP_STEP_SERIAL"] = "1"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["RT_HIP_STEP_SERIAL"]
        else:
            os.environ["RT_HIP_STEP_SERIAL"] = self.old


_results = {}


def result_of(hip, name, ase_small, method=2):
    """Both loops of a case, once per session and left unchanged: the appending loop (history, sums, tensors) and the
    fetching loop on a second plan (per-step records, and its own history with every fetch before its append)."""
    key = (name, method)
    if key in _results:
        return _results[key]
    p, kind = problem_of(hip, name, ase_small, method)
    snaps = snapshots(p)
    with serial():
        one = Loop(hip, p, kind, N_SLOTS)
        spare = []
        for i, tables in enumerate(snaps):
            one.run(tables).plan.history_append(i, H.WEIGHTS[i], accumulate=True)
            if kind == "spare":
                spare.append(one.spare_cells())
        hist, sums, info = one.plan.fetch_history(), one.plan.fetch_history_sum(), one.plan.history_info()
        views = [{k: v.cpu().numpy() for k, v in rec.items()} for rec in one.plan.history_tensors()]
        sum_views = [{k: v.cpu().numpy() for k, v in rec.items()} for rec in one.plan.history_sum_tensors()]
        one.close()
        two = Loop(hip, p, kind, N_STEPS)
        steps = []
        for i, tables in enumerate(snaps):
            steps.append(two.run(tables).fetch_records())
            two.plan.history_append(i)
        hist2 = two.plan.fetch_history()
        two.close()
    out = dict(p=p, kind=kind, hist=hist, sums=sums, info=info, views=views, sum_views=sum_views, steps=steps, hist2=hist2, spare=spare)
    _results[key] = out
    return out


CASES = [("a", 1), ("a", 2), ("b", 2), ("c", 1), ("d", 2), ("e", 2)]
N_REC = dict(a=3, b=1, c=1, d=2, e=1)


# ---------------------------------------------------------------------------------------------- 1. copies
@pytest.mark.parametrize("name,method", CASES)
def test_copies_are_bit_equal(hip, ase_small, name, method):
    R = result_of(hip, name, ase_small, method)
    b = R["p"].beam
    hist, hist2, steps = R["hist"], R["hist2"], R["steps"]
    assert R["info"] == dict(n_steps=N_SLOTS, n_rec=N_REC[name], n_filled=N_STEPS)
    assert len(hist) == len(hist2) == N_REC[name] and all(len(s) == N_REC[name] for s in steps)
    for r, h in enumerate(hist):
        assert h["E_v"].shape == (N_SLOTS, b.nv) and h["nf"].shape == (N_SLOTS, b.nx * b.ny) and h["I_ang"].shape == (N_SLOTS, b.na * b.nb)
        assert h["filled"].tolist() == [1] * N_STEPS + [0]
        for i in range(N_STEPS):
            rec = steps[i][r]
            assert rec["nf"].any() and rec["E_v"].any() and rec["I_ang"].any()
            for k in H.KEYS:
                assert np.array_equal(h[k][i], rec[k]), (name, r, i, k)             # append straight behind the run
                assert np.array_equal(hist2[r][k][i], rec[k]), (name, r, i, k)     # fetch before append, the plan's own records
            assert h["failure_code"][i] == hist2[r]["failure_code"][i] == rec["failure_code"] == 0
            assert h["flags"][i] == hist2[r]["flags"][i] == 0
            assert h["E_sum"][i] == hist2[r]["E_sum"][i]
        assert not np.array_equal(h["nf"][0], h["nf"][1]) and np.array_equal(h["nf"][0], h["nf"][2])   # tables A, B, A, B
        for k in H.KEYS + ("E_sum", "failure_code", "flags"):       # the slot never appended
            assert not h[k][N_STEPS:].any(), (name, r, k)
        # the torch views are the arrays the fetch copies
        v = R["views"][r]
        assert np.array_equal(v["E_v"], h["E_v"]) and np.array_equal(v["nf"].reshape(N_SLOTS, -1), h["nf"])
        assert np.array_equal(v["I_ang"].reshape(N_SLOTS, -1), h["I_ang"]) and np.array_equal(v["E_sum"], h["E_sum"])
        assert np.array_equal(v["failure_code"].astype(np.uint32), h["failure_code"]) and np.array_equal(v["flags"].astype(np.uint32), h["flags"])


# ---------------------------------------------------------------------------------------------- 2. E_sum
@pytest.mark.parametrize("name,method", CASES)
def test_e_sum_within_the_reordering_bound(hip, ase_small, name, method):
    R = result_of(hip, name, ase_small, method)
    worst = 0.0
    for r, h in enumerate(R["hist"]):
        for i in range(N_STEPS):
            assert (h["nf"][i] >= 0).all()
            ratio, bound = H.esum_ratio(h["E_sum"][i], h["nf"][i])
            worst = max(worst, ratio / bound if bound > 0 else ratio)
            ok = ratio <= bound
            if not ok:
                note(f"history: case {name} method {method} record {r} step {i}: |E_sum - fsum| / fsum = {ratio:.3e} > gamma = {bound:.3e}")
            assert ok, (name, r, i, ratio, bound)
    n = R["p"].beam.nx * R["p"].beam.ny
    note(f"history: case {name} method {method}: n = {n} pixels, worst |E_sum - fsum(nf)| / fsum(nf) = {worst:.3f} of gamma_{n - 1} = {H.gamma(n - 1):.3e}"
         f" over {len(R['hist'])} records x {N_STEPS} steps")


def test_spare_cells_are_neither_copied_nor_summed(hip, ase_small):
    R = result_of(hip, "c", ase_small, 1)
    b = R["p"].beam
    assert b.nx == 1 and len(R["spare"]) == N_STEPS
    h = R["hist"][0]
    for i, spare in enumerate(R["spare"]):
        note(f"history: case c step {i}: spare cells behind nf = {spare.tolist()}, E_sum = {h['E_sum'][i]!r}, sum of the {b.ny} pixels = {math.fsum(h['nf'][i])!r}")
        assert spare[0] > 0                    # the top row's rays on the edge x[0] + dx / 2 deposited one past the image
        ratio, bound = H.esum_ratio(h["E_sum"][i], h["nf"][i])
        assert ratio <= bound                  # ... and E_sum is the sum of the nx ny fetched pixels alone
        assert abs(h["E_sum"][i] - math.fsum(h["nf"][i])) < 0.5 * spare[0]


# ---------------------------------------------------------------------------------------------- 3. determinism
def test_e_sum_is_the_same_double_everywhere(hip, ase_small):
    p, _ = problem_of(hip, "a", ase_small, 2)
    with serial():
        sums, nf0 = [], []
        for _ in range(2):      # two plans, two slots each
            loop = Loop(hip, p, "ase", 3)
            loop.run().plan.history_append(0).history_append(2)
            h = loop.plan.fetch_history()
            loop.close()
            assert [r["filled"].tolist() for r in h] == [[1, 0, 1]] * 3
            for r in h:
                assert r["E_sum"][0] == r["E_sum"][2] != 0 and np.array_equal(r["nf"][0], r["nf"][2])
            sums.append([float(r["E_sum"][0]) for r in h])
            nf0.append(h[0]["nf"][0])
        assert sums[0] == sums[1]
        plain = Loop(hip, p, "plain", 2)    # the same problem as a plain emission plan: its record is block 0 of the set
        plain.run().plan.history_append(1)
        hp = plain.plan.fetch_history()
        plain.close()
    assert len(hp) == 1 and np.array_equal(hp[0]["nf"][1], nf0[0])
    note(f"history: E_sum of the ASE record in two slots of two plans and as a plain record: {sums[0][0]!r} {sums[1][0]!r} {float(hp[0]['E_sum'][1])!r}")
    assert float(hp[0]["E_sum"][1]) == sums[0][0]
    assert float(R_a(hip, ase_small)["hist"][0]["E_sum"][0]) == sums[0][0]      # ... and in the time loop of case a


def R_a(hip, ase_small):
    return result_of(hip, "a", ase_small, 2)


# ---------------------------------------------------------------------------------------------- 4. codes and flags
def test_codes_and_flags_around_a_failing_step(hip, ase_small):
    p, _ = problem_of(hip, "e", ase_small, 2)
    bad = tv.crafted_nan_lineshape(p)
    with serial():      # (for the last line alone: steps 0 and 3 are the same tables)
        loop = Loop(hip, p, "plain", 4)
        plan = loop.plan
        loop.run(p).plan.history_append(0)
        loop.run(bad).plan.history_append(1)            # straight behind the run: the unchecked record
        loop.run(bad)
        checked = loop.fetch_records()[0]               # the checking repeat, then the append
        plan.history_append(2)
        loop.run(p).plan.history_append(3)
        h = plan.fetch_history()[0]
        loop.close()
    note(f"history: NaN lineshape step: codes {h['failure_code'].tolist()} flags {h['flags'].tolist()} fetched code {checked['failure_code']}")
    assert h["failure_code"][1] & (1 << 3) and h["flags"][1] & 2
    assert h["failure_code"][2] == checked["failure_code"] and checked["failure_code"] & (1 << 3)
    for k in H.KEYS:
        assert np.array_equal(h[k][2], checked[k]), k
    assert h["flags"][2] == H.flags_of(checked)
    assert h["failure_code"][0] == h["failure_code"][3] == 0 and h["flags"][0] == h["flags"][3] == 0
    assert np.array_equal(h["nf"][0], h["nf"][3]) and h["nf"][0].any()


# ---------------------------------------------------------------------------------------------- 5. running sum
@pytest.mark.parametrize("name,method", CASES)
def test_running_sum_is_the_host_fold(hip, ase_small, name, method):
    R = result_of(hip, name, ase_small, method)
    b = R["p"].beam
    host = H.new_history(N_SLOTS, len(R["hist"]), b.nv, b.nx * b.ny, b.na * b.nb)
    for i in range(N_STEPS):    # the fold over the device's own slabs (pinned by test 1)
        H.file_step(host, i, [{k: h[k][i] for k in H.KEYS} for h in R["hist"]], [0] * len(R["hist"]), weight=H.WEIGHTS[i])
    for r, (h, s) in enumerate(zip(R["hist"], R["sums"])):
        for k in H.KEYS:
            assert s[k].any() and np.array_equal(s[k], host["records"][r]["acc"][k]), (name, r, k)
            assert np.array_equal(R["sum_views"][r][k].ravel(), s[k])
        es = 0.0
        for i in range(N_STEPS):    # E_sum_acc folds the DEVICE's E_sum[i]
            es = es + H.WEIGHTS[i] * float(h["E_sum"][i])
        assert s["E_sum"] == es == float(R["sum_views"][r]["E_sum"][0]), (name, r)


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_history_as_it_was(hip, ase_small, seed_small):
    p, _ = problem_of(hip, "a", ase_small, 2)
    seeds = list(A.seeds_of(p))
    with hip.Plan(p) as plan:
        plan.set_ray_grid()
        with pytest.raises(hip.RayTraceError, match="no history"):
            plan.history_append(0)
        plan.enable_history(3)
        assert plan.history_info() == dict(n_steps=3, n_rec=0, n_filled=0)
        with pytest.raises(hip.RayTraceError, match="not a step run"):       # nothing has run
            plan.history_append(0)
        plan.run()                                                           # an image run
        with pytest.raises(hip.RayTraceError, match="not a step run"):
            plan.history_append(0)
        empty = plan.fetch_history()
        assert len(empty) == 1 and not any(empty[0][k].any() for k in empty[0])
        plan.enable_step().set_ase_seeds(seeds).run().history_append(1)
        before = plan.fetch_history()
        for step in (-1, 3, 1 << 20):
            with pytest.raises(hip.RayTraceError, match="step must be"):
                plan.history_append(step)
        plan.set_ase_seeds([]).run()                                         # another record set: one plain record
        with pytest.raises(hip.RayTraceError, match="bound to"):
            plan.history_append(2)
        with pytest.raises(hip.RayTraceError, match="n_steps"):
            plan.hl.check(plan.hl.lib.rt_hip_plan_history_create(plan._h, -1), "rt_hip_plan_history_create")
        after = plan.fetch_history()
        assert plan.history_info() == dict(n_steps=3, n_rec=3, n_filled=1)
        for x, y in zip(before, after):
            assert x["filled"].tolist() == [0, 1, 0]
            for k in x:
                assert np.array_equal(x[k], y[k]), k
        plan.enable_history(0)                                               # release ...
        assert plan.history_info() == dict(n_steps=0, n_rec=0, n_filled=0)
        with pytest.raises(hip.RayTraceError, match="no history"):
            plan.history_append(0)
        with pytest.raises(hip.RayTraceError, match="no history"):
            plan.fetch_history()
        plan.enable_history(2).history_append(0)                             # ... and create again: bound to the plain record now
        again = plan.fetch_history()
        assert len(again) == 1 and again[0]["filled"].tolist() == [1, 0] and again[0]["nf"][0].any() and not again[0]["nf"][1].any()
        assert np.array_equal(again[0]["nf"][0], plan.fetch_step()["nf"])


# ---------------------------------------------------------------------------------------------- 7. no host wait
def test_append_returns_while_the_run_is_in_flight(hip, seed_small):
    import torch

    with hip.Plan(seed_small) as plan:
        plan.set_ray_grid().enable_step().enable_history(1)
        plan.run().history_append(0)                    # (a warm-up: the allocation of the history happens here)
        torch.cuda.synchronize()
        plan.run().history_append(0)
        ev = torch.cuda.Event()
        ev.record()                                     # (the null stream, where run and append were queued)
        done = ev.query()
        print(f"history: the event behind run + append had {'completed' if done else 'NOT completed'} when history_append returned")
        h = plan.fetch_history()[0]
        rec = plan.fetch_step()
        code = plan.fetch(want_image=False)["failure_code"]
    assert h["filled"].tolist() == [1] and h["failure_code"][0] == code == 0 and h["flags"][0] == 0
    for k in H.KEYS:
        assert rec[k].any() and np.array_equal(h[k][0], rec[k]), k
    ratio, bound = H.esum_ratio(h["E_sum"][0], h["nf"][0])
    assert ratio <= bound


# ---------------------------------------------------------------------------------------------- 8. another stream
def test_append_on_a_second_stream(hip, ase_small):
    import torch

    R = R_a(hip, ase_small)
    p = R["p"]
    side = torch.cuda.Stream()
    with serial():
        loop = Loop(hip, p, "ase", N_SLOTS)
        for i, tables in enumerate(snapshots(p)):       # the run on the null stream, the append on `side`, the next run on the null stream again
            loop.run(tables).plan.history_append(i, H.WEIGHTS[i], accumulate=True, stream=side.cuda_stream)
        hist, sums = loop.plan.fetch_history(), loop.plan.fetch_history_sum()
        loop.close()
    for h, ref, s, sref in zip(hist, R["hist"], sums, R["sums"]):
        for k in ref:
            assert np.array_equal(h[k], ref[k]), k
        for k in sref:
            assert np.array_equal(s[k], sref[k]), k


# ---------------------------------------------------------------------------------------------- 9. the convenience loop
def test_step_history_loop_is_the_explicit_loop(hip, ase_small):
    R = R_a(hip, ase_small)
    p = R["p"]
    with serial():
        out = hip.step_history_loop(p, snapshots(p), seeds=list(A.seeds_of(p)), accumulate=True, weights=H.WEIGHTS)
        plain = hip.step_history_loop(p, snapshots(p, 2))
    assert out["filled"].tolist() == [1] * N_STEPS and len(out["records"]) == 3 and plain["sums"] is None and len(plain["records"]) == 1
    for h, ref, s, sref in zip(out["records"], R["hist"], out["sums"], R["sums"]):
        for k in ref:
            assert np.array_equal(h[k], ref[k][:N_STEPS]), k
        for k in sref:
            assert np.array_equal(s[k], sref[k]), k
    for k in H.KEYS + ("E_sum",):                      # without seeds: the plain emission record, block 0 of the set
        assert np.array_equal(plain["records"][0][k], R["hist"][0][k][:2]), k
