"""The step history without a device (include/rt_hip.h, rt_hip_plan_history_*; csrc/rt_history.hip).

1. Layout: the arrays rt_hip_debug_history_layout reports -- the function rt_hip_plan_history_append itself lays the
   allocation out with -- do not overlap, are aligned to 8 bytes (the record-shaped blocks to 256), fit the reported size;
   the chunks of the work-groups tile [0, nx ny) exactly once.
2. The host restatement (tests/step_history.py: file_step): on the oracle's reduced records of tests/ase_seeds.py's problem
   E_sum is within the reordering bound of math.fsum, the flags are clean, and one planted negative value / one planted NaN
   sets its bit.
3. The entry points are declared, listed and bound; the Python face validates; without a device the new calls fail loudly."""
import ctypes
import importlib
import math
import re
from pathlib import Path

import numpy as np
import pytest

import ase_seeds as A
import step_history as H
import table_variants as tv

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
cabi = rt.cabi
HEADER = Path(__file__).resolve().parents[1] / "include" / "rt_hip.h"
NEW = ["rt_hip_plan_history_create", "rt_hip_plan_history_append", "rt_hip_plan_history_ptrs", "rt_hip_plan_history_sum_ptrs",
       "rt_hip_plan_history_fetch", "rt_hip_plan_history_fetch_sum", "rt_hip_plan_history_info", "rt_hip_debug_history_layout"]


@pytest.fixture(scope="module")
def hl(hip):
    backend.build_library()
    return backend.HipLibrary.get()


# ---------------------------------------------------------------------------------------------- 1. layout
def extents(L, n_rec, n_steps, accumulate):
    """[(name, first byte, bytes, alignment asked)] of every array of every block, the scratch included."""
    out = []
    for r in range(n_rec):
        for k in ("E_v", "nf", "I_ang"):
            out.append((f"{k}[{r}]", L[f"off_{k}"] + r * L[f"rec_{k}"], n_steps * L[f"step_{k}"], 256))
            if accumulate:
                out.append((f"acc_{k}[{r}]", L[f"off_acc_{k}"] + r * L[f"rec_acc_{k}"], L[f"step_{k}"], 256))
        out.append((f"E_sum[{r}]", L["off_E_sum"] + r * L["rec_E_sum"], 8 * n_steps, 8))
        out.append((f"code[{r}]", L["off_code"] + r * L["rec_code"], 4 * n_steps, 8))
        out.append((f"flags[{r}]", L["off_flags"] + r * L["rec_flags"], 4 * n_steps, 8))
    if accumulate:
        out.append(("acc_E_sum", L["off_acc_E_sum"], 8 * n_rec, 8))
    out.append(("filled", L["off_filled"], n_steps, 8))
    out.append(("part", L["off_part"], 8 * n_rec * L["wg_per_rec"], 8))
    out.append(("pflag", L["off_pflag"], 4 * n_rec * L["wg_per_rec"], 8))
    return out


def pixel_shapes(chunk):
    return [(1, 1), (63, 1), (64, 1), (65, 1), (12, 6), (chunk - 1, 1), (chunk, 1), (chunk + 1, 1), (2 * chunk + 7, 1)]


def test_layout_arrays_are_disjoint_aligned_and_inside(hl):
    chunk = H.layout(hl, 1, 1, 1, 1, 1, 1, 1)["chunk"]
    assert chunk >= 64 and chunk % 2 == 0
    n = 0
    for nx, ny in pixel_shapes(chunk):
        for nv in (1, 5, 52):
            for na, nb in ((1, 1), (5, 4)):
                for n_rec in (1, 3, 6):
                    for n_steps, acc in ((1, 1), (4, 1), (5, 0)):
                        L = H.layout(hl, nv, nx, ny, na, nb, n_rec, n_steps, acc)
                        label = f"nv {nv} nx {nx} ny {ny} na {na} nb {nb} n_rec {n_rec} n_steps {n_steps} acc {acc}"
                        ext = sorted(extents(L, n_rec, n_steps, acc), key=lambda e: e[1])
                        for name, first, size, align in ext:
                            assert first % align == 0, (label, name)
                            assert first + size <= L["bytes"], (label, name)
                        for (na_, fa, sa, _), (nb_, fb, _, _) in zip(ext, ext[1:]):
                            assert fa + sa <= fb, (label, na_, nb_)
                        assert L["off_part"] + L["scratch_bytes"] == L["bytes"] and L["off_pflag"] >= L["off_part"] + 8 * n_rec * L["wg_per_rec"], label
                        assert (L["step_E_v"], L["step_nf"], L["step_I_ang"]) == (8 * nv, 8 * nx * ny, 8 * na * nb), label
                        if not acc:
                            assert L["off_acc_E_v"] == L["off_acc_nf"] == L["off_acc_I_ang"] == L["off_acc_E_sum"] == 0, label
                        n += 1
    assert n == 9 * 3 * 2 * 3 * 3


def test_layout_chunks_tile_the_pixels_exactly_once(hl):
    chunk = H.layout(hl, 1, 1, 1, 1, 1, 1, 1)["chunk"]
    for nx, ny in pixel_shapes(chunk):
        for n_rec in (1, 3, 6):
            L = H.layout(hl, 5, nx, ny, 5, 4, n_rec, 4)
            npix = nx * ny
            assert L["chunk"] == chunk          # a constant of the layout, whatever the shape
            covered = np.zeros(npix, np.int64)
            for w in range(L["pix_wg"]):        # work-group w of a block: pixels [w chunk, (w + 1) chunk) of it
                assert w * chunk < npix          # (no work-group without a pixel)
                covered[w * chunk:min((w + 1) * chunk, npix)] += 1
            assert (covered == 1).all(), (nx, ny)
            assert L["aux_wg"] >= 1 and L["wg_per_rec"] == L["pix_wg"] + L["aux_wg"] and L["grid"] == n_rec * L["wg_per_rec"]
            assert L["wg_threads"] * 4 == chunk  # two pairs of pixels per thread


def test_layout_refuses_nonsense(hl):
    f, out = cabi.RtHistoryFacts(), cabi.RtHistoryLayout()
    f.size, out.size = ctypes.sizeof(f), ctypes.sizeof(out)
    f.nv = f.nx = f.ny = f.na = f.nb = f.n_rec = f.n_steps = 1
    assert hl.lib.rt_hip_debug_history_layout(ctypes.byref(f), ctypes.byref(out)) == cabi.RT_OK
    for name in ("nv", "nx", "ny", "na", "nb", "n_rec", "n_steps"):
        setattr(f, name, 0)
        assert hl.lib.rt_hip_debug_history_layout(ctypes.byref(f), ctypes.byref(out)) != cabi.RT_OK, name
        setattr(f, name, 1)
    out.size += 4
    assert hl.lib.rt_hip_debug_history_layout(ctypes.byref(f), ctypes.byref(out)) != cabi.RT_OK
    assert hl.lib.rt_hip_debug_history_layout(None, None) != cabi.RT_OK


# ---------------------------------------------------------------------------------------------- 2. the restatement
_records = {}


def oracle_records(oracle, ase_small):
    """The oracle's records of base(ASE_small, 2) and of its B tables, reduced to E_v, nf, I_ang (once per session)."""
    if not _records:
        p = A.base(ase_small, 2)
        for name, q in (("A", p), ("B", tv.tables_b(p))):
            out = oracle.image_loop(q, q.build_rays())
            assert out["failure_code"] == 0
            rec = backend.step_outputs_from_image(q, out["image"])
            _records[name] = dict(E_v=np.asarray(rec["E_v"]), nf=np.asarray(rec["nf"]).ravel(), I_ang=np.asarray(out["I_ang"]).ravel())
    return _records


def test_restatement_on_the_oracles_records(oracle, ase_small):
    recs = oracle_records(oracle, ase_small)
    a, b = recs["A"], recs["B"]
    nv, npix, nab = len(a["E_v"]), len(a["nf"]), len(a["I_ang"])
    assert npix == 72 and a["nf"].any() and not np.array_equal(a["nf"], b["nf"])
    hist = H.new_history(4, 2, nv, npix, nab)
    for i, w in enumerate(H.WEIGHTS):
        H.file_step(hist, i, [a, b] if i % 2 == 0 else [b, a], [0, 0], weight=w)
    assert hist["filled"].tolist() == [1, 1, 1, 1]
    for r, h in enumerate(hist["records"]):
        for i in range(4):
            src = (a, b)[(i + r) % 2]
            for k in H.KEYS:
                assert np.array_equal(h[k][i], src[k])
            ratio, bound = H.esum_ratio(h["E_sum"][i], h["nf"][i])
            print(f"restatement: record {r} step {i}: |E_sum - fsum| / fsum = {ratio:.3e} (bound gamma_{npix - 1} = {bound:.3e})")
            assert (src["nf"] >= 0).all() and ratio <= bound
            assert h["flags"][i] == 0 and h["failure_code"][i] == 0
        # the running sum: the fold written out once more, element by element
        for k in H.KEYS:
            acc = np.zeros_like(h[k][0])
            for i, w in enumerate(H.WEIGHTS):
                acc = acc + np.float64(w) * h[k][i]
            assert np.array_equal(h["acc"][k], acc)
        es = 0.0
        for i, w in enumerate(H.WEIGHTS):
            es = es + w * float(h["E_sum"][i])
        assert h["acc"]["E_sum"] == es


@pytest.mark.parametrize("key", H.KEYS)
def test_restatement_flags_a_planted_value(oracle, ase_small, key):
    a = oracle_records(oracle, ase_small)["A"]
    for value, bit in ((-1e-300, 1), (np.nan, 2)):
        rec = {k: v.copy() for k, v in a.items()}
        rec[key][len(rec[key]) // 2] = value
        hist = H.file_step(H.new_history(2, 1, len(a["E_v"]), len(a["nf"]), len(a["I_ang"])), 1, [rec], [8])
        h = hist["records"][0]
        assert h["flags"].tolist() == [0, bit] and h["failure_code"].tolist() == [0, 8] and hist["filled"].tolist() == [0, 1]
        if key == "nf" and bit == 2:
            assert math.isnan(h["E_sum"][1])


# ---------------------------------------------------------------------------------------------- 3. header, binding, Python face
def test_entry_points_are_declared_listed_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(rt_hip_[a-z_0-9]+)\s*\(", text))
    lib = backend.HipLibrary.get().lib
    for name in NEW:
        assert name in cabi.HIP_API_SYMBOLS and name in declared, name
        assert getattr(lib, name).restype is ctypes.c_int, name
    assert re.search(r"int\s+rt_hip_plan_history_append\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+step,\s*double\s+weight,\s*int\s+accumulate,"
                     r"\s*void\s*\*\s*stream\s*\)", text)
    for method in ("enable_history", "history_append", "fetch_history", "fetch_history_sum", "history_tensors", "history_sum_tensors",
                   "history_info"):
        assert callable(getattr(backend.Plan, method)), method
    assert callable(backend.step_history_loop)


class _NoNativeCalls:
    def __getattr__(self, name):
        raise AssertionError(f"the native library ({name}) was reached before the arguments were refused")


def test_python_face_refuses_before_any_native_call(ase_small):
    plan = backend.Plan.__new__(backend.Plan)
    plan.hl = _NoNativeCalls()
    plan._h = None
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError, match="n_steps"):
            plan.enable_history(bad)
    with pytest.raises(AssertionError, match="native library"):
        plan.enable_history(4)
    with pytest.raises(ValueError, match="no snapshots"):
        backend.step_history_loop(ase_small, [])
    with pytest.raises(ValueError, match="weights"):
        backend.step_history_loop(ase_small, [ase_small], weights=[1.0, 2.0])


def test_no_silent_fallback_without_a_device(ase_small):
    lib = backend.HipLibrary.get()
    p = A.base(ase_small, 2)
    if lib.device_count() > 0:      # (what the loop files: tests/test_gpu_step_history.py)
        out = backend.step_history_loop(p, [p, tv.tables_b(p)])
        assert out["filled"].tolist() == [1, 1] and len(out["records"]) == 1 and out["records"][0]["E_sum"].all()
        return
    with pytest.raises(backend.RayTraceError, match="no HIP device"):
        backend.step_history_loop(p, [p, tv.tables_b(p)])
    # a NULL plan is an argument error of every new plan call, not a crash
    for name, args in (("rt_hip_plan_history_create", (4,)), ("rt_hip_plan_history_append", (0, 1.0, 0, None)),
                       ("rt_hip_plan_history_info", (None, None, None)), ("rt_hip_plan_history_ptrs", (0,) + (None,) * 6),
                       ("rt_hip_plan_history_sum_ptrs", (0,) + (None,) * 4), ("rt_hip_plan_history_fetch", (0,) + (None,) * 7),
                       ("rt_hip_plan_history_fetch_sum", (0,) + (None,) * 4)):
        assert getattr(lib.lib, name)(None, *args) == cabi.RT_ERR_ARG, name
        with pytest.raises(backend.RayTraceError, match=name):
            lib.check(getattr(lib.lib, name)(None, *args), name)
