"""The C-ABI shared library loads (no GPU needed) and exports exactly what
include/rt_hip.h declares; entry points fail loudly without a device."""
import ctypes
import importlib
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib(hip):
    # through the `hip` fixture: torch's HIP runtime must be loaded before this library's, or a GPU test later in the
    # same session finds no device through torch and RCCL cannot initialise
    backend.build_library()
    return backend.HipLibrary.get()


def declared_symbols():
    text = (ROOT / "include" / "rt_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_hip_[a-z_0-9]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert declared_symbols() == sorted(rt.cabi.HIP_API_SYMBOLS)


def test_library_exports_every_declared_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib.path)], capture_output=True, text=True, check=True).stdout
    # a closed export surface (csrc/rt_hip.map): every defined dynamic symbol is a declared entry point -- no runtime
    # internals, no kernel host stubs, no C++ library symbols
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert exported == set(declared_symbols()), sorted(exported ^ set(declared_symbols()))
    for s in declared_symbols():
        assert getattr(lib.lib, s) is not None


def test_code_object_is_gfx950(lib):
    blob = lib.path.read_bytes()
    assert b"gfx950" in blob and b"rt_march_kernel" in blob and b"rt_freq_kernel" in blob


def test_struct_layouts_match_the_header():
    c = rt.cabi
    assert ctypes.sizeof(c.RtRay) == 16 and c.RAY_DTYPE.itemsize == 16
    assert ctypes.sizeof(c.RtBeam) == 5 * 4 + 4 + 5 * 8 + 5 * 8     # ints, pad, doubles, pointers
    assert ctypes.sizeof(c.RtGain) == 3 * 4 + 4 + 6 * 8
    assert ctypes.sizeof(c.RtSeed) == 5 * 4 + 4 + 10 * 8 + 8
    assert ctypes.sizeof(c.RtStats) == 4 * 8 + 4 * 4


def test_no_silent_fallback_without_a_device(lib, ase_small):
    if lib.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(backend.RayTraceError, match="no HIP device"):
        backend.Plan(ase_small)
    with pytest.raises(backend.RayTraceError):
        backend.image_loop(ase_small, ase_small.build_rays(np.arange(10)))
    with pytest.raises(backend.RayTraceError, match="Unknown method"):
        backend.create_image(ase_small, "cpu")


def test_missing_library_is_loud(tmp_path):
    with pytest.raises(backend.RayTraceError, match="not built"):
        backend.HipLibrary(tmp_path / "librt_hip.so")


def test_product_never_imports_the_oracle():
    pkg = ROOT / "raytrace-miniapp_amd"
    for f in list(pkg.rglob("*.py")) + list(pkg.rglob("*.hip")) + list(pkg.rglob("*.h")) + list(pkg.rglob("*.cpp")):
        text = f.read_text()
        assert "rt_oracle" not in text and "from oracle" not in text and "import oracle" not in text, f
