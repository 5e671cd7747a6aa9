"""Plan.update_gain without a device: the record type, the marshalling and its ValueErrors (all raised before the library
is reached), the declared symbols, and the table helpers of tests/table_variants.py checked in numpy.  The device side
is tests/test_gpu_plan_update.py."""
import ctypes
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import table_variants as tv

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
cabi = rt.cabi
ROOT = Path(__file__).resolve().parents[1]


def shapes(p):
    return [(g.Nx, g.Ny) for g in p.gain]


def test_record_layout():
    assert ctypes.sizeof(cabi.RtGainValues) == 32
    assert [f for f, _ in cabi.RtGainValues._fields_] == ["n", "g0", "E0", "gv"]


def test_the_three_symbols_are_declared():
    for s in ("rt_hip_plan_update_gain", "rt_hip_plan_update_gain_dev", "rt_hip_plan_table_flags"):
        assert s in cabi.HIP_API_SYMBOLS
    header = (ROOT / "include" / "rt_hip.h").read_text()
    assert re.search(r"typedef struct rt_gain_values \{[^}]*\bn;[^}]*\bg0;[^}]*\bE0;[^}]*\bgv;[^}]*\} rt_gain_values;", header, re.S)
    assert hasattr(backend.Plan, "update_gain") and hasattr(backend.Plan, "table_flags")


def test_marshalling_points_into_the_arrays_it_keeps(ase_small):
    b = tv.tables_b(ase_small)
    for form in (b, b.gain, tv.as_tables(b), [None] + [dict(n=g.n, g0=g.g0, E0=g.E0, gv=g.gv) for g in b.gain[1:]]):
        m = cabi.GainValues(form, shapes(ase_small), ase_small.beam.nv)
        assert m.N == 3 and not m.on_device
        for i in (1, 2):
            g = b.gain[i]
            for name in ("n", "g0", "E0", "gv"):
                assert ctypes.cast(getattr(m.vals[i], name), ctypes.c_void_p).value == getattr(g, name).ctypes.data
                assert any(a is getattr(g, name) for a in m._keep)
        assert not m.vals[0].n and not m.vals[0].gv            # entry 0 is ignored
    # the natural multi-dimensional shapes are accepted too
    g = b.gain[1]
    nd = [None] + [(g.n.reshape(g.Ny, g.Nx), g.g0.reshape(g.Ny, g.Nx), g.E0, g.gv.reshape(g.Ny, g.Nx, g.Nv))] + tv.as_tables(b)[2:]
    assert cabi.GainValues(nd, shapes(ase_small), ase_small.beam.nv).N == 3


def test_a_missing_E0_is_a_null_pointer(ase_small):
    q = tv.crafted_no_e0(ase_small)
    m = cabi.GainValues(q, shapes(ase_small), ase_small.beam.nv)
    assert not m.vals[2].E0 and m.vals[1].E0 and m.vals[2].n and m.vals[2].g0 and m.vals[2].gv
    assert m.tables[2][2] is None


def test_value_errors_are_raised_before_the_library(ase_small):
    import torch

    p, K = ase_small, ase_small.beam.nv
    good = tv.as_tables(p)

    def swap(i, k, a):
        t = list(good)
        e = list(t[i])
        e[k] = a
        t[i] = tuple(e)
        return t

    g = p.gain[1]
    cases = [
        (good[:2], "N = 3"),                                                       # wrong N
        (good + good[1:2], "N = 3"),
        (swap(1, 0, g.n[:-1].copy()), r"n has shape"),                             # wrong shapes
        (swap(2, 3, p.gain[2].gv.reshape(-1, K)[:, :-1].copy()), r"gv has shape"),
        (swap(1, 3, g.gv.reshape(g.Nx, g.Ny, K)), r"gv has shape"),
        (swap(1, 0, g.n.astype(np.float32)), "n has dtype float32, expected float64"),
        (swap(1, 1, g.g0.astype(np.float64)), "g0 has dtype float64, expected float32"),
        (swap(1, 3, np.asfortranarray(g.gv.reshape(-1, K))), "gv is not contiguous"),
        (swap(2, 1, None), "g0 is missing"),
        (swap(1, 0, g.n.tolist()), "neither a numpy array nor a torch tensor"),
        (swap(1, 1, torch.from_numpy(g.g0)), "torch tensor on the CPU"),           # a CPU tensor, alone or among numpy arrays
        (tv.as_tables(p, torch.from_numpy), "torch tensor on the CPU"),
        ([None, 7, good[2]], "expected a Gain, a dict or a tuple"),
    ]
    for tables, text in cases:
        with pytest.raises(ValueError, match=text):
            cabi.GainValues(tables, shapes(p), K)


def test_host_and_device_arrays_do_not_mix(ase_small):
    """No device here: a stand-in with the two attributes the marshalling asks a tensor for."""
    class OnDevice:
        is_cuda, dtype, shape = True, "torch.float32", (ase_small.gain[1].Nx * ase_small.gain[1].Ny,)
        device = type("D", (), dict(index=0))()

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 4096

    t = tv.as_tables(ase_small)
    t[1] = (t[1][0], OnDevice(), t[1][2], t[1][3])
    with pytest.raises(ValueError, match="mixed"):
        cabi.GainValues(t, shapes(ase_small), ase_small.beam.nv)
    OnDevice.device = type("D", (), dict(index=1, __str__=lambda s: "cuda:1"))()
    with pytest.raises(ValueError, match="the plan on device 0"):
        cabi.GainValues(t, shapes(ase_small), ase_small.beam.nv)


# ------------------------------------------------------------------------------------------ the helpers, in numpy
def test_tables_b_is_a_finite_non_negative_snapshot_on_the_same_grids(ase_small, seed_small):
    for p in (ase_small, seed_small):
        b = tv.tables_b(p)
        assert b.gain[0] is p.gain[0] and b.N == p.N and b.use_emis == p.use_emis
        for ga, gb in zip(p.gain[1:], b.gain[1:]):
            assert gb.x is ga.x and gb.y is ga.y and gb.Nv == ga.Nv
            assert np.array_equal(gb.g0, ga.g0 * np.float32(0.5)) and np.array_equal(gb.gv, ga.gv * np.float32(0.75))
            assert np.array_equal(gb.n, 1.0 + 1.1 * (ga.n - 1.0)) and not np.array_equal(gb.n, ga.n)
            if ga.E0 is not None:
                assert np.array_equal(gb.E0, ga.E0 * np.float32(2.0))
            for a in (gb.n, gb.g0, gb.gv) + (() if gb.E0 is None else (gb.E0,)):
                assert np.isfinite(a).all() and (a >= 0).all()
        assert tv.expected_flags(b)["bounded"] == 1 and tv.expected_flags(b)["gv_nonfinite"] == 0


def test_row_wrap_table(ase_small):
    q = tv.crafted_row_wrap(ase_small)
    g = q.gain[1]
    assert g.Nx >= 40
    dn = tv.neighbour_dn(g)
    assert abs(dn - 0.001) < 1e-15, "horizontal neighbours differ by 0.001, vertical ones by nothing"
    across_the_wrap = float(np.abs(np.diff(g.n)).max())       # what a scan over the flat array would see
    assert across_the_wrap >= 0.039 and abs(across_the_wrap - 0.001 * (g.Nx - 1)) < 1e-12
    f = tv.expected_flags(q)
    assert f["bounded"] == 1 and f["ntest_proven"] == 1
    # ... and with the wrap's difference the proof of the |n - n0| test would be lost: 8 x 0.1 x 2.4 x dn against 0.05 - 1e-5
    assert 8.0 * 0.1 * 2.4 * dn <= 0.05 - 1e-5 < 8.0 * 0.1 * 2.4 * 0.039


def test_crafted_flags(ase_small, seed_small):
    a = tv.expected_flags(ase_small)
    assert a == dict(bounded=1, ntest_proven=1, gv_nonfinite=0, gs_cap=a["gs_cap"]) and 0 < a["gs_cap"] < np.finfo(np.float32).max
    u = tv.expected_flags(tv.crafted_unbounded(ase_small))
    assert u["bounded"] == 0 and u["ntest_proven"] == 0 and u["gs_cap"] == a["gs_cap"]
    h = tv.expected_flags(tv.crafted_huge_lineshape(ase_small))
    assert h["gs_cap"] == np.float32(708.0) / np.float32(1e30) and h["gv_nonfinite"] == 0 and h["bounded"] == 1
    e = tv.expected_flags(tv.crafted_no_e0(ase_small))
    assert e == a and tv.crafted_no_e0(ase_small).use_emis
    for value in (np.nan, np.inf):
        n = tv.expected_flags(tv.crafted_nan_lineshape(ase_small, value=value))
        assert n["gv_nonfinite"] == 1 and n["gs_cap"] == a["gs_cap"], "a non-finite value does not enter the maximum"
    assert not np.isfinite(tv.crafted_nan_index(ase_small).gain[2].n).all()
    # the gain-only mode scans no lineshape
    s = tv.expected_flags(seed_small)
    assert s["gv_nonfinite"] == 0 and s["gs_cap"] == np.finfo(np.float32).max


def test_four_lengths(ase_small):
    q = tv.four_lengths(ase_small)
    g2, sub = ase_small.gain[2], q.gain[2]
    assert q.N == 4 and sub.Nx == (g2.Nx + 1) // 2 and sub.Ny == g2.Ny
    assert np.array_equal(sub.n.reshape(sub.Ny, sub.Nx), g2.n.reshape(g2.Ny, g2.Nx)[:, ::2])
    assert np.array_equal(sub.gv.reshape(sub.Ny, sub.Nx, -1), g2.gv.reshape(g2.Ny, g2.Nx, -1)[:, ::2])
    q.validate()


def test_row_padding_shapes(ase_small, seed_small):
    """Kp = K rounded up to four: the three shapes of the row-padding test on the device."""
    assert seed_small.beam.nv == 82                                        # Kp = 84
    assert problem_mod.resample_frequency(ase_small, 5).beam.nv == 5       # Kp = 8
    assert ase_small.beam.nv % 4 == 0                                      # Kp = K: the straight copy
