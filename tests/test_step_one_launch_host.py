"""Step mode in one launch (rt_hip_plan_set_step_one_launch), the parts that need no device: the C ABI carries the entry
point -- declared in the header, bound in cabi, covered by the export map -- and Plan.set_step_one_launch refuses a bad
argument before any native call."""
import fnmatch
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
cabi = rt.cabi

NAME = "rt_hip_plan_set_step_one_launch"
ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_hip.h"
MAP = ROOT / "raytrace-miniapp_amd" / "csrc" / "rt_hip.map"


def test_entry_point_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"int\s+" + NAME + r"\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+on\s*\)", text)
    assert NAME in cabi.HIP_API_SYMBOLS
    # the export map: what it lists under `global:` names the symbol (a pattern or the name itself)
    body = re.sub(r"/\*.*?\*/", "", MAP.read_text(), flags=re.S)
    exported = re.search(r"global:(.*?)local:", body, flags=re.S).group(1)
    patterns = [s.strip() for s in exported.split(";") if s.strip()]
    assert any(fnmatch.fnmatchcase(NAME, pat) for pat in patterns), patterns
    assert callable(backend.Plan.set_step_one_launch)
    lib = backend.HipLibrary.get().lib         # the built library carries it, with the prototype cabi declares
    fn = getattr(lib, NAME)
    assert fn.restype is cabi.C.c_int and list(fn.argtypes) == [cabi.C.c_void_p, cabi.C.c_int]
    # the environment switch is documented where the other switches are
    assert "RT_HIP_STEP_ONE_LAUNCH" in (ROOT / "INTEGRATION.md").read_text()


class _NoNativeCalls:
    """Stands where Plan.hl stands: any use of the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"Plan.set_step_one_launch reached the native library ({name}) before it refused its argument")


def _bare_plan():
    plan = backend.Plan.__new__(backend.Plan)
    plan.hl = _NoNativeCalls()
    plan._h = None          # (close() has nothing to destroy)
    return plan


def test_set_step_one_launch_refuses_in_python_before_any_native_call():
    plan = _bare_plan()
    for bad in (2, -1, "1", None, 0.5, 1.0, [True], np.int64(3)):
        with pytest.raises(ValueError, match="set_step_one_launch"):
            plan.set_step_one_launch(bad)
    for good in (True, False, 1, 0, np.int32(1)):   # (what is acceptable does go on to the library)
        with pytest.raises(AssertionError, match="native library"):
            plan.set_step_one_launch(good)
