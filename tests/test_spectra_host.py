"""Spectra mode (RayTrace::calc_ray on the GPU), the parts that need no device: the C ABI carries the four entry
points, the code object carries the kernel, there is no fallback without a device, and the [n][4] float64 form of a
ray list rounds as the C cast does."""
import importlib

import numpy as np
import pytest

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
cabi = rt.cabi

NEW = ["rt_hip_plan_enable_spectra", "rt_hip_plan_fetch_spectra", "rt_hip_plan_spectra_ptr", "rt_hip_calc_rays"]


def test_entry_points_are_declared_bound_and_exported():
    hl = backend.HipLibrary.get()
    for name in NEW:
        assert name in cabi.HIP_API_SYMBOLS
        fn = getattr(hl.lib, name)          # exported by the built library
        assert fn.argtypes is not None, name  # bound by declare_hip_api
    assert len(hl.lib.rt_hip_calc_rays.argtypes) == 13
    for method in ("enable_spectra", "fetch_spectra", "spectra_ptr"):
        assert callable(getattr(backend.Plan, method))
    assert callable(backend.calc_rays) and callable(backend.calc_ray)


def test_code_object_holds_the_spectra_kernel():
    blob = backend.LIB_PATH.read_bytes()
    assert b"rt_spec_kernel" in blob
    assert b"gfx950" in blob


def test_calc_rays_without_a_device_is_an_error(ase_small):
    hl = backend.HipLibrary.get()
    if hl.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(backend.RayTraceError, match="no HIP device"):
        backend.calc_rays(ase_small, ase_small.build_rays(np.arange(10)))
    with pytest.raises(backend.RayTraceError, match="no HIP device"):
        backend.calc_ray(ase_small, (0.0, 0.0, 0.0, 0.0))


def test_ray_array_conversion_rounds_as_the_float_cast(ase_small, seed_small):
    for p in (ase_small, seed_small):
        ids = np.arange(0, p.n_rays_total, 4001, dtype=np.int64)
        rays = p.build_rays(ids)
        gx, gy, ga, gb = p.ray_grid
        nb, na, ny = len(gb), len(ga), len(gy)
        full = np.stack([gx[ids // (ny * na * nb)], gy[(ids // (na * nb)) % ny], ga[(ids // nb) % na], gb[ids % nb]], axis=1)
        assert full.dtype == np.float64
        got = cabi.rays_from_array(full)
        assert got.dtype == cabi.RAY_DTYPE
        for key in "xyab":
            assert np.array_equal(got[key].view(np.uint32), rays[key].view(np.uint32))
        back = cabi.rays_to_array(got)
        assert back.dtype == np.float64 and back.shape == (len(ids), 4)
        assert np.array_equal(cabi.rays_from_array(back).view(np.uint32), rays.view(np.uint32))
    # ties and values no float holds: round to nearest even, as (float) does
    v = np.array([[1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 0.1, -1e-50]])
    r = cabi.rays_from_array(v)
    assert r["x"][0] == np.float32(1.0) and r["y"][0] == np.float32(1.0 + 2.0 ** -22)
    assert r["a"][0] == np.float32(0.1) and r["b"][0] == 0.0 and np.signbit(r["b"][0])
    with pytest.raises(ValueError):
        cabi.rays_from_array(np.zeros((3, 3)))
    assert cabi.rays_to_array(np.zeros(0, cabi.RAY_DTYPE)).shape == (0, 4)
