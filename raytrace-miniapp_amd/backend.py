"""Host-side binding of the HIP backend (csrc/librt_hip.so) and the Python
mirror of the reference's operator interface for this path.

  HipLibrary            loads the in-tree shared library; fails loudly when it
                        is missing -- there is NO CPU fallback in the product.
  Plan                  device-resident problem (rt_hip_plan_* of include/rt_hip.h)
  image_loop(...)       the back-end loop, same meaning as RayTraceImageCudaLoop
                        (src/RayTraceImageCuda.cu:145-221) behind the signature of
                        src/RayTraceImage.cpp:47-75
  step_loop(...)        the same loop with the application's per-step record in place of the image cube: E_v, nf, I_ang
  step_history_loop(...) a time loop over gain tables with every step's records filed on the device (Plan.history_append)
  multi_step_loop(...)  step_loop on all devices of the node: strided ray grid per device, one sum-reduce of the record
  seed_step_loop(...)   the step records of up to RT_N_SEED_MAX seed beams from one march (Plan.set_seeds)
  full_step_loop(...)   the ASE record and the records of up to RT_N_SEED_MAX seed beams from one march (Plan.set_ase_seeds)
  length_scan_loop(...) the step record at every plasma length n = 2 .. N from one forward march (Plan.enable_length_scan)
  suffix_scan_loop(...)  the step record of the last n lengths, n = 2 .. N, from one backward march (Plan.enable_suffix_scan)
  seed_length_scan_loop(...) ... of up to RT_N_SEED_MAX seed beams at every length, from that one march (Plan.set_scan_seeds)
  step_outputs_from_image  their definition as reductions of a cube, in numpy (no device)
  calc_rays / calc_ray  RayTrace::calc_ray (src/RayTraceImage.cpp:189-204), batched: per-ray spectrum, exit ray, code
  create_image(p, method)
                        mirror of RayTrace::create_image (src/RayTraceImage.cpp:227-434):
                        checks, mode select, ray list, dispatch on the method
                        string ("hip", "hip-multigpu", "auto"), failure handling.
"""
from __future__ import annotations

import ctypes as C
import subprocess
import time
from pathlib import Path

import numpy as np

from . import cabi
from .problem import Problem, Seed

CSRC = Path(__file__).resolve().parent / "csrc"
LIB_PATH = CSRC / "librt_hip.so"


class RayTraceError(RuntimeError):
    """Raised where the reference calls RAY_ERROR (utilities/RayUtilityMacros.h:88-91)."""


def build_library(force: bool = False) -> Path:
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    if force and LIB_PATH.exists():
        LIB_PATH.unlink()
    subprocess.run(["make", "-s", "-C", str(CSRC)], check=True)
    return LIB_PATH


class HipLibrary:
    _instance = None

    def __init__(self, path: Path = LIB_PATH):
        if not Path(path).exists():
            raise RayTraceError(
                f"HIP backend library {path} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        self.path = Path(path)
        self.lib = C.CDLL(str(path))
        cabi.declare_hip_api(self.lib)

    @classmethod
    def get(cls) -> "HipLibrary":
        if cls._instance is None:
            if not LIB_PATH.exists():
                # a fresh checkout (built files are not in history): compile in-tree with hipcc;
                # if that is impossible the constructor below raises -- there is no other path
                try:
                    build_library()
                except Exception as exc:  # noqa: BLE001
                    raise RayTraceError(f"HIP backend library {LIB_PATH} is missing and could not be built: {exc}") from exc
            cls._instance = HipLibrary()
        return cls._instance

    def device_count(self) -> int:
        return int(self.lib.rt_hip_device_count())

    def selftest(self, device: int = 0) -> tuple[int, int]:
        """(values checked, mismatches) of the on-device known-answer test of the march's exact shortcuts."""
        n, bad = C.c_ulonglong(0), C.c_ulonglong(0)
        self.check(self.lib.rt_hip_selftest(device, C.byref(n), C.byref(bad)), "rt_hip_selftest")
        return int(n.value), int(bad.value)

    def check(self, rc: int, what: str) -> None:
        if rc != cabi.RT_OK:
            msg = self.lib.rt_hip_last_error().decode(errors="replace")
            raise RayTraceError(f"{what} failed (status {rc}): {msg}")


class _View:  # the CUDA array interface, which torch.as_tensor reads
    def __init__(self, ptr: int, shape: tuple, typestr: str = "<f8"):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=2, strides=None)


def _view(ptr: int, shape: tuple, device: int):
    """torch view (float64, on `device`, no copy) of the doubles at device pointer ptr."""
    import torch

    return torch.as_tensor(_View(ptr, shape), device=torch.device("cuda", device))


def _seed_array(seeds, who: str, what: str) -> tuple:
    """(seeds as a list, their RtSeed array, what the array points into) for `who`; more than RT_N_SEED_MAX of them (`what`:
    where they would have to fit) or an entry that is not a Seed is a ValueError."""
    seeds = list(seeds)
    if len(seeds) > cabi.RT_N_SEED_MAX:
        raise ValueError(f"{who}: {len(seeds)} seeds given, at most RT_N_SEED_MAX = {cabi.RT_N_SEED_MAX} fit into {what}")
    for i, sd in enumerate(seeds):
        if not isinstance(sd, Seed):
            raise ValueError(f"{who}: entry {i} is a {type(sd).__name__}, not a Seed")
    keep = []
    arr = (cabi.RtSeed * max(1, len(seeds)))()
    for i, sd in enumerate(seeds):
        arr[i] = cabi.seed_record(sd, keep)
    return seeds, arr, keep


def _taken_seeds(who: str, seeds) -> list:
    """`seeds` as a list for a loop that takes 1 .. RT_N_SEED_MAX of them, every entry a Seed; anything else is a ValueError."""
    seeds = list(seeds)
    if not 1 <= len(seeds) <= cabi.RT_N_SEED_MAX:
        raise ValueError(f"{who}: {len(seeds)} seeds given, 1 .. RT_N_SEED_MAX = {cabi.RT_N_SEED_MAX} are taken")
    for i, sd in enumerate(seeds):
        if not isinstance(sd, Seed):
            raise ValueError(f"{who}: entry {i} is a {type(sd).__name__}, not a Seed")
    return seeds


def _scales_arg(who: str, scales, n: int):
    """`scales` as a float64 array of n entries (None stays None: the plan's scale); another length is a ValueError."""
    if scales is None:
        return None
    sc = np.ascontiguousarray(scales, dtype=np.float64)
    if sc.shape != (n,):
        raise ValueError(f"{who}: {sc.size} scales for {n} seeds")
    return sc


def _on_arg(who: str, on) -> int:
    """`on` as 0 / 1; anything but a bool or 0 / 1 is a ValueError."""
    if isinstance(on, bool):
        on = int(on)
    if not isinstance(on, (int, np.integer)) or on not in (0, 1):
        raise ValueError(f"{who}: on is True / False (or 1 / 0), not {on!r}")
    return int(on)


def _scan_takes(who: str, problem: Problem, method: int, only: str) -> None:
    """The loops of a scan: another method than the scan's, N < 3 or more than RT_N_SCAN_MAX lengths is a ValueError."""
    if problem.method != method:
        raise ValueError(f"{who}: the problem's method is {problem.method}; {only}")
    if problem.N < 3 or problem.N - 1 > cabi.RT_N_SCAN_MAX:
        raise ValueError(f"{who}: N = {problem.N}; a scan takes 3 <= N <= RT_N_SCAN_MAX + 1 = {cabi.RT_N_SCAN_MAX + 1}")


class Plan:
    """A problem resident in HBM: tables uploaded once, runnable many times."""

    # What the plan has been switched to, as the methods below record it.  Class-level defaults: they hold for a plan of any
    # making (the host tests build one without a device, around __init__).
    _spectra = _step = False    # the output mode (enable_spectra, enable_step)
    _length_spectra = False     # length spectra are on (enable_length_spectra): a run without image and I_ang, as a spectra run
    _ring = 0                   # runs of the timing ring (set_timing_ring)
    _scan = False               # the length scan or the suffix scan is on (enable_length_scan, enable_suffix_scan)
    _n_seed = 0                 # seeds of the set (set_seeds)
    _n_spec_seed = 0            # seeds of spectra mode or of length spectra (set_spectra_seeds)
    _n_spec_ase_seed = 0        # ASE seeds of spectra mode (set_spectra_ase_seeds)
    _n_lspec_ase_seed = 0       # ASE seeds of length spectra (set_length_spectra_ase_seeds)
    _n_scan_seed = 0            # seeds of the length scan or of the suffix scan (set_scan_seeds, set_suffix_seeds)
    _n_ase_seed = 0             # ASE seeds (set_ase_seeds)
    _n_scan_ase_seed = 0        # ASE seeds of the length scan or of the suffix scan (set_scan_ase_seeds, set_suffix_ase_seeds)

    def __init__(self, problem: Problem, device: int = 0, lib: HipLibrary | None = None,
                 method: int | None = None):
        self.hl = lib or HipLibrary.get()
        self.problem = problem
        self.device = device
        self._m = cabi.Marshalled(problem)
        self._h = C.c_void_p()
        rc = self.hl.lib.rt_hip_plan_create(C.byref(self._h), device, self._m.N, C.byref(self._m.beam),
                                            self._m.gain, self._m.seed_ref,
                                            problem.method if method is None else method, problem.scale)
        self.hl.check(rc, "rt_hip_plan_create")
        self.n_rays = 0

    # -- rays ---------------------------------------------------------------
    def set_rays(self, rays: np.ndarray) -> "Plan":
        rays = np.ascontiguousarray(rays, dtype=cabi.RAY_DTYPE)
        self.hl.check(self.hl.lib.rt_hip_plan_set_rays(self._h, cabi.rays_ptr(rays), len(rays)),
                      "rt_hip_plan_set_rays")
        self.n_rays = len(rays)
        return self

    def set_ray_grid(self, first: int | None = None, stride: int | None = None,
                     count: int | None = None, grids=None) -> "Plan":
        """Rays generated on the device from the problem's ray grid
        (RayTraceImage.cpp:300-328); defaults follow N_start / N_parallel.
        `grids` = (x, y, a, b) overrides the problem's ray grid."""
        p = self.problem
        gx, gy, ga, gb = p.ray_grid if grids is None else [np.ascontiguousarray(g, np.float64) for g in grids]
        first = p.N_start if first is None else first
        stride = p.N_parallel if stride is None else stride
        if count is None:
            nt = len(gx) * len(gy) * len(ga) * len(gb)
            count = 0 if first >= nt else (nt - first + stride - 1) // stride
        self._grids = (gx, gy, ga, gb)
        self.hl.check(self.hl.lib.rt_hip_plan_set_ray_grid(
            self._h, cabi._dp(gx), len(gx), cabi._dp(gy), len(gy), cabi._dp(ga), len(ga),
            cabi._dp(gb), len(gb), first, stride, count), "rt_hip_plan_set_ray_grid")
        self.n_rays = count
        return self

    # -- run ----------------------------------------------------------------
    def enable_probe(self, on: bool = True) -> "Plan":
        self.hl.check(self.hl.lib.rt_hip_plan_enable_probe(self._h, int(on)), "rt_hip_plan_enable_probe")
        return self

    def run(self, stream: int = 0, image_ptr: int = 0, iang_ptr: int = 0) -> "Plan":
        """Asynchronous: zero outputs + trace kernel on `stream` (a hipStream_t value)."""
        self.hl.check(self.hl.lib.rt_hip_plan_run(self._h, C.c_void_p(stream), C.c_void_p(image_ptr),
                                                  C.c_void_p(iang_ptr)), "rt_hip_plan_run")
        return self

    def fetch(self, want_image: bool = True) -> dict:
        b = self.problem.beam
        want_image = want_image and not self._spectra and not self._length_spectra  # a spectra run has no image
        want_iang = want_image
        want_image = want_image and not self._step     # ... and a step run has I_ang only
        image = np.empty(b.nx * b.ny * b.nv) if want_image else None
        iang = np.empty(b.na * b.nb) if want_iang else None
        code = C.c_uint(0)
        nf = C.c_int(0)
        failed = np.zeros(cabi.RT_N_FAILED_MAX, dtype=cabi.RAY_DTYPE)
        st = cabi.RtStats()
        rc = self.hl.lib.rt_hip_plan_fetch(
            self._h, cabi._dp(image) if want_image else None, cabi._dp(iang) if want_iang else None,
            C.byref(code), cabi.rays_ptr(failed), cabi.RT_N_FAILED_MAX, C.byref(nf), C.byref(st))
        self.hl.check(rc, "rt_hip_plan_fetch")
        return dict(image=image, I_ang=iang, failure_code=code.value, failed_rays=failed[:nf.value].copy(),
                    stats={k: getattr(st, k) for k, _ in cabi.RtStats._fields_})

    def set_exact_emission(self, on: bool = True) -> "Plan":
        """Emission mode: the CPU's per-frequency el/gl instead of the per-sub-segment ratio (include/rt_hip.h)."""
        self.hl.check(self.hl.lib.rt_hip_plan_set_exact_emission(self._h, int(on)), "rt_hip_plan_set_exact_emission")
        return self

    def set_step_factor(self, c: float) -> "Plan":
        self.hl.check(self.hl.lib.rt_hip_plan_set_step_factor(self._h, float(c)), "rt_hip_plan_set_step_factor")
        return self

    def set_debug(self, bits: int) -> "Plan":
        """Profiling aid: bit 0 skips the frequency kernel, bit 1 skips the march, bit 2 the I_ang flush (include/rt_hip.h)."""
        self.hl.check(self.hl.lib.rt_hip_plan_set_debug(self._h, int(bits)), "rt_hip_plan_set_debug")
        return self

    def enable_path(self, on: bool = True) -> "Plan":
        self.hl.check(self.hl.lib.rt_hip_plan_enable_path(self._h, int(on)), "rt_hip_plan_enable_path")
        return self

    def fetch_path(self) -> dict:
        """{x, y, I}: [n_rays][3(N-1)+1] float arrays, err: [n_rays] return codes."""
        n = self.n_rays
        N2 = (self.problem.N - 1) * cabi.RT_N_SUB + 1
        path = np.zeros((n, N2, 3), np.float32)
        err = np.zeros(n, np.int32)
        self.hl.check(self.hl.lib.rt_hip_plan_fetch_path(self._h, cabi._fp(path), err.ctypes.data_as(C.POINTER(C.c_int32))),
                      "rt_hip_plan_fetch_path")
        return dict(x=path[:, :, 0].copy(), y=path[:, :, 1].copy(), I=path[:, :, 2].copy(), err=err)

    def enable_spectra(self, on: bool = True) -> "Plan":
        """Spectra mode (RayTrace::calc_ray for every ray): a run produces Iv, ray2, err per ray instead of the image."""
        self.hl.check(self.hl.lib.rt_hip_plan_enable_spectra(self._h, int(on)), "rt_hip_plan_enable_spectra")
        if self._spectra and not on:
            self._n_spec_seed = 0   # (switching the mode off drops its seeds)
            self._n_spec_ase_seed = 0
        self._spectra = bool(on)
        return self

    def fetch_spectra(self) -> dict:
        """Iv [n_rays][K] float64, ray2 [n_rays] (RAY_DTYPE), err [n_rays] int32 (0, -1, -2, -3) of the last run."""
        n, K = self.n_rays, self.problem.beam.nv
        Iv = np.empty((n, K))
        ray2 = np.zeros(n, cabi.RAY_DTYPE)
        err = np.zeros(n, np.int32)
        self.hl.check(self.hl.lib.rt_hip_plan_fetch_spectra(self._h, cabi._dp(Iv), cabi.rays_ptr(ray2),
                                                            err.ctypes.data_as(C.POINTER(C.c_int32))),
                      "rt_hip_plan_fetch_spectra")
        return dict(Iv=Iv, ray2=ray2, err=err)

    def spectra_ptr(self) -> int:
        """Device pointer of Iv [n_rays][K] of the last spectra run (for torch views), 0 if there is none."""
        return int(self.hl.lib.rt_hip_plan_spectra_ptr(self._h) or 0)

    def spectra_tensor(self):
        """torch view [n_rays][K] (float64, on the plan's device) of Iv of the last spectra run: no copy, valid until
        the plan's next run."""
        import torch

        ptr = self.spectra_ptr()
        if not ptr or not self.n_rays:
            return torch.empty((0, self.problem.beam.nv), dtype=torch.float64, device=torch.device("cuda", self.device))
        return _view(ptr, (self.n_rays, self.problem.beam.nv), self.device)

    def enable_length_spectra(self, on: bool = True) -> "Plan":
        """Length spectra (include/rt_hip.h, rt_hip_plan_enable_length_spectra): a run marches once and leaves Iv, ray2
        and err per ray at EVERY plasma length n = 2 .. N -- calc_ray on prefix_lengths(n) of a forward plan, on
        suffix_lengths(n) of a backward one.  A mode of its own: not together with spectra, step, path, a scan or seeds."""
        on = _on_arg("enable_length_spectra", on)
        self.hl.check(self.hl.lib.rt_hip_plan_enable_length_spectra(self._h, on), "rt_hip_plan_enable_length_spectra")
        if self._length_spectra and not on:
            self._n_spec_seed = 0   # (switching the mode off drops its seeds)
            self._n_lspec_ase_seed = 0
        self._length_spectra = bool(on)   # (fetch() reads it; spectra mode keeps its own flag: switching this off on a plan in spectra mode changes nothing)
        return self

    def fetch_length_spectra(self) -> list:
        """[dict(n, Iv [n_rays][K], ray2 (RAY_DTYPE), err [n_rays] int32)] for n = 2 .. N of the last length-spectra run."""
        nr, K = self.n_rays, self.problem.beam.nv
        out = []
        for n in range(2, self.problem.N + 1):
            Iv = np.empty((nr, K))
            ray2 = np.zeros(nr, cabi.RAY_DTYPE)
            err = np.zeros(nr, np.int32)
            self.hl.check(self.hl.lib.rt_hip_plan_fetch_length_spectra(self._h, n, cabi._dp(Iv), cabi.rays_ptr(ray2),
                                                                       err.ctypes.data_as(C.POINTER(C.c_int32))),
                          "rt_hip_plan_fetch_length_spectra")
            out.append(dict(n=n, Iv=Iv, ray2=ray2, err=err))
        return out

    def length_spectra_ptrs(self, n: int) -> tuple:
        """Device pointers (Iv, ray2, err) of the rows of length n of the last length-spectra run."""
        iv, r2, er = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.hl.check(self.hl.lib.rt_hip_plan_length_spectra_ptrs(self._h, int(n), C.byref(iv), C.byref(r2), C.byref(er)),
                      "rt_hip_plan_length_spectra_ptrs")
        return int(iv.value or 0), int(r2.value or 0), int(er.value or 0)

    def length_spectra_tensors(self) -> dict:
        """torch views of the last length-spectra run, length-major and without a copy: Iv [N-1][n_rays][K] float64, ray2
        [N-1][n_rays][4] float32 (x, y, a, b), err [N-1][n_rays] int32; block n - 2 is length n.  Valid until the plan's
        next run or a change of its ray set."""
        import torch

        L, nr, K = self.problem.N - 1, self.n_rays, self.problem.beam.nv
        dev = torch.device("cuda", self.device)
        if not nr:
            return dict(Iv=torch.empty((L, 0, K), dtype=torch.float64, device=dev), ray2=torch.empty((L, 0, 4), dtype=torch.float32, device=dev),
                        err=torch.empty((L, 0), dtype=torch.int32, device=dev))
        iv, r2, er = self.length_spectra_ptrs(2)   # (block 0: the arrays are length-major)

        return dict(Iv=_view(iv, (L, nr, K), self.device), ray2=torch.as_tensor(_View(r2, (L, nr, 4), "<f4"), device=dev),
                    err=torch.as_tensor(_View(er, (L, nr), "<i4"), device=dev))

    # -- spectra seeds: the per-ray outputs of several seed beams from one march --
    def set_spectra_seeds(self, seeds) -> "Plan":
        """Spectra seeds (include/rt_hip.h, rt_hip_plan_set_spectra_seeds): up to RT_N_SEED_MAX Seed records on a plan created
        with a seed whose spectra mode or length spectra are on.  A run then leaves Iv and err once per seed, seed-major, from
        one march (ray2 does not depend on the seed); the creation seed is not among them.  [] removes the seeds.  More
        seeds than that, or anything that is not a Seed, is a ValueError raised here, before any native call."""
        self._n_spec_seed = self._install_seeds("set_spectra_seeds", seeds, "spectra mode")
        return self

    def _spec_rows(self, name: str, *index) -> dict:
        nr, K = self.n_rays, self.problem.beam.nv
        Iv = np.empty((nr, K))
        ray2 = np.zeros(nr, cabi.RAY_DTYPE)
        err = np.zeros(nr, np.int32)
        self.hl.check(getattr(self.hl.lib, name)(self._h, *index, cabi._dp(Iv), cabi.rays_ptr(ray2), err.ctypes.data_as(C.POINTER(C.c_int32))), name)
        return dict(Iv=Iv, ray2=ray2, err=err)

    def fetch_seed_spectra(self) -> list:
        """[dict(Iv [n_rays][K], ray2 (RAY_DTYPE), err [n_rays] int32)] per spectra seed of the last spectra-mode run."""
        return [self._spec_rows("rt_hip_plan_fetch_seed_spectra", s) for s in range(self._n_spec_seed)]

    def fetch_seed_length_spectra(self) -> list:
        """Per spectra seed of the last length-spectra run: [dict(n, Iv [n_rays][K], ray2 (RAY_DTYPE), err [n_rays] int32)]
        for n = 2 .. N."""
        return [[dict(n=n, **self._spec_rows("rt_hip_plan_fetch_seed_length_spectra", s, n)) for n in range(2, self.problem.N + 1)]
                for s in range(self._n_spec_seed)]

    def _spec_ptrs(self, name: str, *index) -> tuple:
        iv, r2, er = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.hl.check(getattr(self.hl.lib, name)(self._h, *(int(i) for i in index), C.byref(iv), C.byref(r2), C.byref(er)), name)
        return int(iv.value or 0), int(r2.value or 0), int(er.value or 0)

    def seed_spectra_ptrs(self, s: int) -> tuple:
        """Device pointers (Iv, ray2, err) of the rows of spectra seed s of the last spectra-mode run with seeds."""
        return self._spec_ptrs("rt_hip_plan_seed_spectra_ptrs", s)

    def seed_length_spectra_ptrs(self, s: int, n: int) -> tuple:
        """Device pointers (Iv, ray2, err) of the rows of (spectra seed s, length n) of the last length-spectra run with seeds."""
        return self._spec_ptrs("rt_hip_plan_seed_length_spectra_ptrs", s, n)

    def seed_spectra_tensors(self) -> dict:
        """torch views of the last spectra-mode run with spectra seeds, seed-major and without a copy: Iv [n_seed][n_rays][K]
        float64, err [n_seed][n_rays] int32, ray2 [n_rays][4] float32 (x, y, a, b: the same for every seed).  Valid until
        the plan's next run or a change of its ray set."""
        import torch

        ns, nr, K = self._n_spec_seed, self.n_rays, self.problem.beam.nv
        dev = torch.device("cuda", self.device)
        if not nr or not ns:
            return dict(Iv=torch.empty((ns, 0, K), dtype=torch.float64, device=dev), ray2=torch.empty((0, 4), dtype=torch.float32, device=dev),
                        err=torch.empty((ns, 0), dtype=torch.int32, device=dev))
        iv, r2, er = self.seed_spectra_ptrs(0)   # (block 0: the arrays are seed-major)
        return dict(Iv=_view(iv, (ns, nr, K), self.device), ray2=torch.as_tensor(_View(r2, (nr, 4), "<f4"), device=dev),
                    err=torch.as_tensor(_View(er, (ns, nr), "<i4"), device=dev))

    def seed_length_spectra_tensors(self) -> dict:
        """torch views of the last length-spectra run with spectra seeds, seed-major then length-major and without a copy:
        Iv [n_seed][N-1][n_rays][K] float64, err [n_seed][N-1][n_rays] int32, ray2 [N-1][n_rays][4] float32; block n - 2 is
        length n.  Valid until the plan's next run or a change of its ray set."""
        import torch

        ns, L, nr, K = self._n_spec_seed, self.problem.N - 1, self.n_rays, self.problem.beam.nv
        dev = torch.device("cuda", self.device)
        if not nr or not ns:
            return dict(Iv=torch.empty((ns, L, 0, K), dtype=torch.float64, device=dev), ray2=torch.empty((L, 0, 4), dtype=torch.float32, device=dev),
                        err=torch.empty((ns, L, 0), dtype=torch.int32, device=dev))
        iv, r2, er = self.seed_length_spectra_ptrs(0, 2)   # (block (0, 0))
        return dict(Iv=_view(iv, (ns, L, nr, K), self.device), ray2=torch.as_tensor(_View(r2, (L, nr, 4), "<f4"), device=dev),
                    err=torch.as_tensor(_View(er, (ns, L, nr), "<i4"), device=dev))

    # -- spectra mode with ASE seeds: the ASE rows and the seeded rows of an emission plan from one march --
    def set_spectra_ase_seeds(self, seeds) -> "Plan":
        """ASE seeds of spectra mode (include/rt_hip.h, rt_hip_plan_set_spectra_ase_seeds): up to RT_N_SEED_MAX Seed records on
        an EMISSION plan (created without a seed, tables with E0) whose spectra mode is on.  A run then leaves, from one march,
        the plan's own ASE rows (block 0) and per seed the rows of the same problem created with that seed (block 1 + s); ray2
        does not depend on the block.  There are no scales: calc_ray has none.  [] removes the seeds.  More seeds than that,
        or anything that is not a Seed, is a ValueError raised here, before any native call."""
        self._n_spec_ase_seed = self._install_seeds("set_spectra_ase_seeds", seeds, "spectra mode")
        return self

    def fetch_full_spectra(self) -> dict:
        """dict(ase=rows, seeds=[rows ...]) of the last spectra-mode run with ASE seeds; every rows is dict(Iv [n_rays][K],
        ray2 (RAY_DTYPE), err [n_rays] int32)."""
        return dict(ase=self._spec_rows("rt_hip_plan_fetch_full_spectra", 0),
                    seeds=[self._spec_rows("rt_hip_plan_fetch_full_spectra", 1 + s) for s in range(self._n_spec_ase_seed)])

    def full_spectra_ptrs(self, r: int) -> tuple:
        """Device pointers (Iv, ray2, err) of block r of the last spectra-mode run with ASE seeds: r = 0 the ASE rows, 1 + s
        those of seed s."""
        return self._spec_ptrs("rt_hip_plan_full_spectra_ptrs", r)

    def full_spectra_tensors(self) -> dict:
        """torch views of the last spectra-mode run with ASE seeds, block-major and without a copy: Iv [1 + n_seed][n_rays][K]
        float64, err [1 + n_seed][n_rays] int32, ray2 [n_rays][4] float32 (x, y, a, b: the same for every block); block 0 is
        the ASE block.  Valid until the plan's next run or a change of its ray set."""
        import torch

        nb, nr, K = 1 + self._n_spec_ase_seed, self.n_rays, self.problem.beam.nv
        dev = torch.device("cuda", self.device)
        if not nr:
            return dict(Iv=torch.empty((nb, 0, K), dtype=torch.float64, device=dev), ray2=torch.empty((0, 4), dtype=torch.float32, device=dev),
                        err=torch.empty((nb, 0), dtype=torch.int32, device=dev))
        iv, r2, er = self.full_spectra_ptrs(0)   # (block 0: the arrays are block-major)
        return dict(Iv=_view(iv, (nb, nr, K), self.device), ray2=torch.as_tensor(_View(r2, (nr, 4), "<f4"), device=dev),
                    err=torch.as_tensor(_View(er, (nb, nr), "<i4"), device=dev))

    # -- length spectra with ASE seeds: the ASE curve and the seeded curves of an emission plan, per ray, from one march --
    def set_length_spectra_ase_seeds(self, seeds) -> "Plan":
        """ASE seeds of length spectra (include/rt_hip.h, rt_hip_plan_set_length_spectra_ase_seeds): up to RT_N_SEED_MAX Seed
        records on an EMISSION plan (created without a seed, tables with E0) whose length spectra are on.  A run then leaves,
        from one scan march, at every length n = 2 .. N the plan's own ASE rows (curve 0) and per seed the rows of the same
        problem created with that seed (curve 1 + s); ray2 does not depend on the curve.  There are no scales: calc_ray has
        none.  [] removes the seeds.  More seeds than that, or anything that is not a Seed, is a ValueError raised here, before
        any native call."""
        self._n_lspec_ase_seed = self._install_seeds("set_length_spectra_ase_seeds", seeds, "length spectra")
        return self

    def fetch_full_length_spectra(self) -> dict:
        """dict(ase=[rows per n], seeds=[[rows per n] per seed]) of the last length-spectra run with ASE seeds, n = 2 .. N;
        every rows is dict(n, Iv [n_rays][K], ray2 (RAY_DTYPE), err [n_rays] int32)."""
        curve = lambda r: [dict(n=n, **self._spec_rows("rt_hip_plan_fetch_full_length_spectra", r, n)) for n in range(2, self.problem.N + 1)]
        return dict(ase=curve(0), seeds=[curve(1 + s) for s in range(self._n_lspec_ase_seed)])

    def full_length_spectra_ptrs(self, r: int, n: int) -> tuple:
        """Device pointers (Iv, ray2, err) of block (r, n) of the last length-spectra run with ASE seeds: r = 0 the ASE curve,
        1 + s that of seed s; n = 2 .. N."""
        return self._spec_ptrs("rt_hip_plan_full_length_spectra_ptrs", r, n)

    def full_length_spectra_tensors(self) -> dict:
        """torch views of the last length-spectra run with ASE seeds, curve-major then length-major and without a copy: Iv
        [1 + n_seed][N-1][n_rays][K] float64, err [1 + n_seed][N-1][n_rays] int32, ray2 [N-1][n_rays][4] float32 (x, y, a, b: the
        same for every curve); curve 0 is the ASE curve, block n - 2 length n.  Valid until the plan's next run or a change
        of its ray set."""
        import torch

        nb, L, nr, K = 1 + self._n_lspec_ase_seed, self.problem.N - 1, self.n_rays, self.problem.beam.nv
        dev = torch.device("cuda", self.device)
        if not nr:
            return dict(Iv=torch.empty((nb, L, 0, K), dtype=torch.float64, device=dev), ray2=torch.empty((L, 0, 4), dtype=torch.float32, device=dev),
                        err=torch.empty((nb, L, 0), dtype=torch.int32, device=dev))
        iv, r2, er = self.full_length_spectra_ptrs(0, 2)   # (block (0, 0))
        return dict(Iv=_view(iv, (nb, L, nr, K), self.device), ray2=torch.as_tensor(_View(r2, (L, nr, 4), "<f4"), device=dev),
                    err=torch.as_tensor(_View(er, (nb, L, nr), "<i4"), device=dev))

    def enable_step(self, on: bool = True) -> "Plan":
        """Step mode (include/rt_hip.h): a run produces E_v, nf and I_ang -- the image cube reduced on the way, never
        allocated.  run() then takes no image_ptr."""
        self.hl.check(self.hl.lib.rt_hip_plan_enable_step(self._h, int(on)), "rt_hip_plan_enable_step")
        self._step = bool(on)
        return self

    def set_step_buffers(self, E_v_ptr: int = 0, nf_ptr: int = 0) -> "Plan":
        """E_v [nv] and nf [nx * ny] of the following step runs in the caller's device memory (8-byte aligned; include/rt_hip.h),
        e.g. views of the tensor whose tail is handed to run(iang_ptr=...); (0, 0) restores the plan's own buffers."""
        self.hl.check(self.hl.lib.rt_hip_plan_set_step_buffers(self._h, C.c_void_p(E_v_ptr or None), C.c_void_p(nf_ptr or None)),
                      "rt_hip_plan_set_step_buffers")
        return self

    def set_step_one_launch(self, on: bool = True) -> "Plan":
        """Step runs as ONE launch where that applies (include/rt_hip.h, rt_hip_plan_set_step_one_launch): emission on a ray
        grid of the beam, tables in LDS; everything else keeps the march and the step kernel.  Off by default.  Anything
        but a bool or 0 / 1 is a ValueError raised here, before any native call."""
        on = _on_arg("set_step_one_launch", on)
        self.hl.check(self.hl.lib.rt_hip_plan_set_step_one_launch(self._h, on), "rt_hip_plan_set_step_one_launch")
        return self

    def fetch_step(self) -> dict:
        """E_v [nv], nf [nx * ny] (p = ix + iy nx), I_ang [na * nb] of the last step run (waits for it)."""
        b = self.problem.beam
        E_v, nf, iang = np.empty(b.nv), np.empty(b.nx * b.ny), np.empty(b.na * b.nb)
        self.hl.check(self.hl.lib.rt_hip_plan_fetch_step(self._h, cabi._dp(E_v), cabi._dp(nf), cabi._dp(iang)),
                      "rt_hip_plan_fetch_step")
        return dict(E_v=E_v, nf=nf, I_ang=iang)

    def step_ptrs(self) -> tuple:
        """Device pointers (E_v, nf) of the last step run."""
        e, n = C.c_void_p(), C.c_void_p()
        self.hl.check(self.hl.lib.rt_hip_plan_step_ptrs(self._h, C.byref(e), C.byref(n)), "rt_hip_plan_step_ptrs")
        return int(e.value or 0), int(n.value or 0)

    def step_tensors(self) -> dict:
        """torch views (float64, on the plan's device, no copy) of E_v [nv], nf [ny][nx] and I_ang [nb][na] (the plan's own
        buffer; None if every run was handed the caller's) of the last step run: valid until the plan's next run; read
        them on the run's stream or after a fetch."""
        e, n = self.step_ptrs()
        return self._record_views((e, n, self.iang_ptr))

    # -- the records of a run that leaves several (a seed set, ASE seeds, a length scan, the seeds of a scan) --
    def _fetch_record(self, name: str, *index) -> dict:
        """dict(E_v [nv], nf [nx * ny], I_ang [na * nb], failure_code) by the C entry point `name` at `index`."""
        b = self.problem.beam
        E_v, nf, iang = np.empty(b.nv), np.empty(b.nx * b.ny), np.empty(b.na * b.nb)
        code = C.c_uint(0)
        self.hl.check(getattr(self.hl.lib, name)(self._h, *index, cabi._dp(E_v), cabi._dp(nf), cabi._dp(iang), C.byref(code)), name)
        return dict(E_v=E_v, nf=nf, I_ang=iang, failure_code=code.value)

    def _record_ptrs(self, name: str, *index) -> tuple:
        """Device pointers (E_v, nf, I_ang) by the C entry point `name` at `index`."""
        e, n, a = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.hl.check(getattr(self.hl.lib, name)(self._h, *(int(i) for i in index), C.byref(e), C.byref(n), C.byref(a)), name)
        return int(e.value or 0), int(n.value or 0), int(a.value or 0)

    def _record_views(self, ptrs: tuple) -> dict:
        """torch views of E_v [nv], nf [ny][nx] and I_ang [nb][na] (None without a pointer) at the pointers of a record."""
        b = self.problem.beam
        e, n, a = ptrs
        return dict(E_v=_view(e, (b.nv,), self.device), nf=_view(n, (b.ny, b.nx), self.device),
                    I_ang=_view(a, (b.nb, b.na), self.device) if a else None)

    # -- seed set -----------------------------------------------------------
    def set_seeds(self, seeds) -> "Plan":
        """A seed set (include/rt_hip.h, rt_hip_plan_set_seeds): up to RT_N_SEED_MAX Seed records whose step records one
        run leaves, from one march; [] removes the set.  The plan must have been created with a seed.  More seeds than
        that, or anything that is not a Seed, is a ValueError raised here, before any native call."""
        self._n_seed = self._install_seeds("set_seeds", seeds, "a set")
        return self

    def _install_seeds(self, who: str, seeds, what: str) -> int:
        """set_seeds, set_scan_seeds and set_suffix_seeds behind their own checks: the seeds, checked and marshalled, through
        rt_hip_plan_<who>; returns how many were installed."""
        seeds, arr, _keep = _seed_array(seeds, who, what)
        self.hl.check(getattr(self.hl.lib, "rt_hip_plan_" + who)(self._h, len(seeds), arr if seeds else None), "rt_hip_plan_" + who)
        return len(seeds)

    def fetch_seed_steps(self) -> list:
        """[dict(E_v [nv], nf [nx * ny], I_ang [na * nb], failure_code)] per seed of the set of the last step run (waits for
        it; a failing run is repeated in the checking mode first)."""
        return [self._fetch_record("rt_hip_plan_fetch_seed_step", s) for s in range(self._n_seed)]

    def seed_step_ptrs(self, s: int) -> tuple:
        """Device pointers (E_v, nf, I_ang) of the record of seed s of the last step run with a set."""
        return self._record_ptrs("rt_hip_plan_seed_step_ptrs", s)

    def seed_step_tensors(self) -> list:
        """Per seed of the set: torch views (float64, on the plan's device, no copy) of E_v [nv], nf [ny][nx] and I_ang
        [nb][na] of the last step run -- blocks of one allocation, valid until the plan's next run; read them on the
        run's stream or after a fetch."""
        return [self._record_views(self.seed_step_ptrs(s)) for s in range(self._n_seed)]

    # -- ASE seeds ----------------------------------------------------------
    def set_ase_seeds(self, seeds, scales=None) -> "Plan":
        """ASE seeds (include/rt_hip.h, rt_hip_plan_set_ase_seeds): up to RT_N_SEED_MAX Seed records on an EMISSION plan
        (created without a seed, tables with E0).  A step run then leaves the plan's own emission record and, from the same
        march, the gain-only record of the same problem created with each seed, scale scales[s] (None: the plan's scale);
        [] removes them.  More seeds than that, anything that is not a Seed, or scales of another length is a ValueError
        raised here, before any native call."""
        self._n_ase_seed = self._install_ase_seeds("set_ase_seeds", seeds, scales)
        return self

    def _install_ase_seeds(self, who: str, seeds, scales) -> int:
        """set_ase_seeds, set_scan_ase_seeds and set_suffix_ase_seeds behind their own checks: the seeds and their scales,
        checked and marshalled, through rt_hip_plan_<who>; returns how many were installed."""
        seeds, arr, _keep = _seed_array(seeds, who, "a step record")
        sc = _scales_arg(who, scales, len(seeds))
        self.hl.check(getattr(self.hl.lib, "rt_hip_plan_" + who)(self._h, len(seeds), arr if seeds else None,
                                                                 cabi._dp(sc) if sc is not None and len(seeds) else None),
                      "rt_hip_plan_" + who)
        return len(seeds)

    def fetch_full_step(self) -> dict:
        """dict(ase=rec, seeds=[rec ...]) of the last step run with ASE seeds (waits for it; a failing run is repeated in
        the checking mode first); every rec is dict(E_v [nv], nf [nx * ny], I_ang [na * nb], failure_code)."""
        recs = [self._fetch_record("rt_hip_plan_fetch_full_step", r) for r in range(1 + self._n_ase_seed)]
        return dict(ase=recs[0], seeds=recs[1:])

    def full_step_ptrs(self, r: int) -> tuple:
        """Device pointers (E_v, nf, I_ang) of record r (0: ASE, 1 + s: seed s) of the last step run with ASE seeds."""
        return self._record_ptrs("rt_hip_plan_full_step_ptrs", r)

    def full_step_tensors(self) -> dict:
        """dict(ase=views, seeds=[views ...]): torch views (float64, on the plan's device, no copy) of E_v [nv], nf [ny][nx]
        and I_ang [nb][na] of every record of the last step run with ASE seeds -- blocks of one allocation, valid until the
        plan's next run; read them on the run's stream or after a fetch."""
        recs = [self._record_views(self.full_step_ptrs(r)) for r in range(1 + self._n_ase_seed)]
        return dict(ase=recs[0], seeds=recs[1:])

    # -- length scan --------------------------------------------------------
    def enable_length_scan(self, on: bool = True) -> "Plan":
        """The length scan (include/rt_hip.h, rt_hip_plan_enable_length_scan): a step run then leaves the step record at
        every plasma length n = 2 .. N -- record n is what a step run of problem.prefix_lengths(p, n) leaves -- from ONE
        march.  Forward method only, 3 <= N <= RT_N_SCAN_MAX + 1.  Anything else, or an `on` that is not a bool or 0 / 1, is
        a ValueError raised here, before any native call."""
        return self._enable_scan("enable_length_scan", on, 2, "forward method (2) has the marches of fewer lengths as prefixes of its own")

    def _enable_scan(self, who: str, on, method: int, only: str) -> "Plan":
        """enable_length_scan (method 2, which it asks for when switching on) and enable_suffix_scan (method 1, always)."""
        on = _on_arg(who, on)
        p = self.problem
        if (on or method == 1) and p.method != method:
            raise ValueError(f"{who}: the problem's method is {p.method}; only the {only}")
        if on:
            if p.N < 3:
                raise ValueError(f"{who}: N = {p.N}; a scan needs at least two lengths (N >= 3)")
            if p.N - 1 > cabi.RT_N_SCAN_MAX:
                raise ValueError(f"{who}: N - 1 = {p.N - 1} lengths, at most RT_N_SCAN_MAX = {cabi.RT_N_SCAN_MAX} fit into a scan")
        self.hl.check(getattr(self.hl.lib, "rt_hip_plan_" + who)(self._h, on), "rt_hip_plan_" + who)
        self._scan = bool(on)   # (the records of either scan are the length scan's: _scan_seed_range counts them)
        if not on:
            self._n_scan_seed = self._n_scan_ase_seed = 0   # (switching the scan off drops its seeds)
        return self

    def fetch_length_steps(self) -> list:
        """[dict(n, E_v [nv], nf [nx * ny], I_ang [na * nb], failure_code)] for n = 2 .. N lengths of the last step run with
        the scan on (waits for it; a failing run is repeated in the checking mode first)."""
        return [dict(n=n, **self._fetch_record("rt_hip_plan_fetch_length_step", n)) for n in self._scan_seed_range()[1]]

    def length_step_ptrs(self, n: int) -> tuple:
        """Device pointers (E_v, nf, I_ang) of the record of n lengths of the last step run with the scan on."""
        return self._record_ptrs("rt_hip_plan_length_step_ptrs", n)

    def length_step_tensors(self) -> list:
        """Per n = 2 .. N: dict(n, E_v [nv], nf [ny][nx], I_ang [nb][na]) of torch views (float64, on the plan's device, no
        copy) of the last step run with the scan on -- blocks of one allocation, valid until the plan's next run; read them
        on the run's stream or after a fetch."""
        return [dict(n=n, **self._record_views(self.length_step_ptrs(n))) for n in self._scan_seed_range()[1]]

    # -- suffix scan --------------------------------------------------------
    def enable_suffix_scan(self, on: bool = True) -> "Plan":
        """The suffix scan (include/rt_hip.h, rt_hip_plan_enable_suffix_scan): a step run then leaves the step record of the
        run of the LAST n lengths, n = 2 .. N -- record n is what a step run of problem.suffix_lengths(p, n) leaves -- from
        ONE backward march; fetch_length_steps, length_step_ptrs and length_step_tensors serve the records.  Backward method
        only, 3 <= N <= RT_N_SCAN_MAX + 1.  Anything else, or an `on` that is not a bool or 0 / 1, is a ValueError raised here,
        before any native call."""
        return self._enable_scan("enable_suffix_scan", on, 1, "backward method (1) begins with the marches of the last lengths")

    def set_suffix_ase_seeds(self, seeds, scales=None) -> "Plan":
        """The ASE seeds of the suffix scan (include/rt_hip.h, rt_hip_plan_set_suffix_ase_seeds): up to RT_N_SEED_MAX Seed
        records on a backward EMISSION plan (created without a seed, tables with E0) whose suffix scan is on.  A step run
        then leaves, from one backward march, the plan's emission record and the gain-only record of the same problem created
        with each seed, scale scales[s] (None: the plan's scale), of the run of the last n lengths for n = 2 .. N;
        fetch_full_length_steps, full_length_step_ptrs and full_length_step_tensors serve them; [] removes the seeds.  A
        forward problem, a problem with a seed, a plan whose suffix scan is off or that holds ASE seeds or a seed set, more
        seeds than that, anything that is not a Seed, or scales of another length is a ValueError raised here, before any
        native call."""
        p = self.problem
        if p.method != 1:
            raise ValueError(f"set_suffix_ase_seeds: the problem's method is {p.method}; the suffix scan takes the backward "
                             "method (1) only (a forward plan takes set_scan_ase_seeds)")
        if p.seed is not None:
            raise ValueError("set_suffix_ase_seeds: the plan was created with a seed; the ASE record needs an emission plan")
        if not self._scan:
            raise ValueError("set_suffix_ase_seeds: the suffix scan is off (enable_suffix_scan first)")
        if self._n_ase_seed > 0 or self._n_seed > 0:
            raise ValueError("set_suffix_ase_seeds: the plan holds ASE seeds or a seed set; they and a suffix scan exclude each other")
        # (the records are those of a length scan with ASE seeds: _full_length_range counts them)
        self._n_scan_ase_seed = self._install_ase_seeds("set_suffix_ase_seeds", seeds, scales)
        return self

    # -- the seeds of a scan ------------------------------------------------
    def set_scan_seeds(self, seeds) -> "Plan":
        """The seeds of the length scan (include/rt_hip.h, rt_hip_plan_set_scan_seeds): up to RT_N_SEED_MAX Seed records; a
        step run with the scan on then leaves one record per seed and length n = 2 .. N from one march; [] removes them.
        The scan must be on and the plan created with a seed.  More seeds than that, or anything that is not a Seed, is a
        ValueError raised here, before any native call."""
        self._n_scan_seed = self._install_seeds("set_scan_seeds", seeds, "a scan")
        return self

    def set_suffix_seeds(self, seeds) -> "Plan":
        """The seeds of the suffix scan (include/rt_hip.h, rt_hip_plan_set_suffix_seeds): up to RT_N_SEED_MAX Seed records on
        a backward plan created with a seed whose suffix scan is on.  A step run then leaves, from one backward march, one
        record per seed of the run of the last n lengths for n = 2 .. N; fetch_seed_length_steps, seed_length_step_ptrs and
        seed_length_step_tensors serve them, fetch_length_steps seed 0's curve; [] removes the seeds.  A forward problem, a
        problem without a seed, a plan whose suffix scan is off, more seeds than that, or anything that is not a Seed is a
        ValueError raised here, before any native call."""
        p = self.problem
        if p.method != 1:
            raise ValueError(f"set_suffix_seeds: the problem's method is {p.method}; the suffix scan takes the backward "
                             "method (1) only (a forward plan takes set_scan_seeds)")
        if p.seed is None:
            raise ValueError("set_suffix_seeds: the plan was created without a seed (an emission plan takes set_suffix_ase_seeds)")
        if not self._scan:
            raise ValueError("set_suffix_seeds: the suffix scan is off (enable_suffix_scan first)")
        # (the records are those of a length scan with scan seeds: _scan_seed_range counts them)
        self._n_scan_seed = self._install_seeds("set_suffix_seeds", seeds, "a scan")
        return self

    def _scan_seed_range(self):
        on = self._scan
        return range(self._n_scan_seed if on else 0), range(2, self.problem.N + 1 if on else 2)

    def fetch_seed_length_steps(self) -> list:
        """Per scan seed: [dict(n, E_v [nv], nf [nx * ny], I_ang [na * nb], failure_code)] for n = 2 .. N lengths of the last
        step run (waits for it; a failing run is repeated in the checking mode first)."""
        seeds, lengths = self._scan_seed_range()
        return [[dict(n=n, **self._fetch_record("rt_hip_plan_fetch_seed_length_step", s, n)) for n in lengths] for s in seeds]

    def seed_length_step_ptrs(self, s: int, n: int) -> tuple:
        """Device pointers (E_v, nf, I_ang) of the record of scan seed s at n lengths of the last step run."""
        return self._record_ptrs("rt_hip_plan_seed_length_step_ptrs", s, n)

    def seed_length_step_tensors(self) -> list:
        """Per scan seed, per n = 2 .. N: dict(n, E_v [nv], nf [ny][nx], I_ang [nb][na]) of torch views (float64, on the plan's
        device, no copy) of the last step run -- blocks of one allocation, valid until the plan's next run; read them on the
        run's stream or after a fetch."""
        seeds, lengths = self._scan_seed_range()
        return [[dict(n=n, **self._record_views(self.seed_length_step_ptrs(s, n))) for n in lengths] for s in seeds]

    # -- the ASE seeds of a scan --------------------------------------------
    def set_scan_ase_seeds(self, seeds, scales=None) -> "Plan":
        """The ASE seeds of the length scan (include/rt_hip.h, rt_hip_plan_set_scan_ase_seeds): up to RT_N_SEED_MAX Seed records
        on an EMISSION plan (created without a seed, tables with E0) whose scan is on.  A step run then leaves, from one
        forward march, the plan's emission record and the gain-only record of the same problem created with each seed, scale
        scales[s] (None: the plan's scale), at every length n = 2 .. N; [] removes them.  More seeds than that, anything that is
        not a Seed, or scales of another length is a ValueError raised here, before any native call."""
        self._n_scan_ase_seed = self._install_ase_seeds("set_scan_ase_seeds", seeds, scales)
        return self

    def _full_length_range(self):
        on = self._scan and self._n_scan_ase_seed > 0
        return range(1 + self._n_scan_ase_seed if on else 0), range(2, self.problem.N + 1 if on else 2)

    def fetch_full_length_steps(self) -> dict:
        """dict(ase=[rec per n], seeds=[[rec per n] per seed]) for n = 2 .. N lengths of the last step run of a scan with ASE
        seeds (waits for it; a failing run is repeated in the checking mode first); every rec is dict(n, E_v [nv], nf
        [nx * ny], I_ang [na * nb], failure_code)."""
        recs, lengths = self._full_length_range()
        curves = [[dict(n=n, **self._fetch_record("rt_hip_plan_fetch_full_length_step", r, n)) for n in lengths] for r in recs]
        return dict(ase=curves[0] if curves else [], seeds=curves[1:])

    def full_length_step_ptrs(self, r: int, n: int) -> tuple:
        """Device pointers (E_v, nf, I_ang) of record r (0: ASE, 1 + s: seed s) at n lengths of the last step run of a scan
        with ASE seeds."""
        return self._record_ptrs("rt_hip_plan_full_length_step_ptrs", r, n)

    def full_length_step_tensors(self) -> dict:
        """dict(ase=[views per n], seeds=[[views per n] per seed]): torch views (float64, on the plan's device, no copy) of E_v
        [nv], nf [ny][nx] and I_ang [nb][na] of every record of the last step run of a scan with ASE seeds -- blocks of one
        allocation, valid until the plan's next run; read them on the run's stream or after a fetch."""
        recs, lengths = self._full_length_range()
        curves = [[dict(n=n, **self._record_views(self.full_length_step_ptrs(r, n))) for n in lengths] for r in recs]
        return dict(ase=curves[0] if curves else [], seeds=curves[1:])

    # -- step history -------------------------------------------------------
    def enable_history(self, n_steps: int) -> "Plan":
        """A device-resident step history of n_steps slots (include/rt_hip.h, rt_hip_plan_history_create); 0 releases it.  The
        memory is taken at the first history_append, which binds the history to that run's record set."""
        if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 0:
            raise ValueError(f"enable_history: n_steps is an int >= 0, not {n_steps!r}")
        self.hl.check(self.hl.lib.rt_hip_plan_history_create(self._h, int(n_steps)), "rt_hip_plan_history_create")
        return self

    def history_append(self, step: int, weight: float = 1.0, accumulate: bool = False, stream: int | None = None) -> "Plan":
        """File every record of the last step run into slot `step` of the history, with E_sum, the valid() flags and the
        failure codes, on the device and in stream order: the call only enqueues.  accumulate: add weight * record to the
        running sum as well.  stream: a hipStream_t value; None: the stream of the last run."""
        self.hl.check(self.hl.lib.rt_hip_plan_history_append(self._h, int(step), float(weight), int(bool(accumulate)),
                                                             C.c_void_p(stream or None)), "rt_hip_plan_history_append")
        return self

    def history_info(self) -> dict:
        """dict(n_steps, n_rec (0 before the first append), n_filled (slots an append was queued for))."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self.hl.check(self.hl.lib.rt_hip_plan_history_info(self._h, C.byref(a), C.byref(b), C.byref(c)), "rt_hip_plan_history_info")
        return dict(n_steps=a.value, n_rec=b.value, n_filled=c.value)

    def fetch_history(self) -> list:
        """One dict per record block of the history (waits for the last append): E_v [n_steps][nv], nf [n_steps][nx * ny],
        I_ang [n_steps][na * nb], E_sum [n_steps], failure_code [n_steps] and flags [n_steps] (uint32; bit 0 a negative value,
        bit 1 a NaN) and filled [n_steps] (uint8, the same in every dict).  Slots never appended read zero."""
        b, info = self.problem.beam, self.history_info()
        T, out = info["n_steps"], []
        for r in range(max(1, info["n_rec"])):
            E_v, nf, iang, es = np.empty((T, b.nv)), np.empty((T, b.nx * b.ny)), np.empty((T, b.na * b.nb)), np.empty(T)
            code, flags, filled = np.empty(T, np.uint32), np.empty(T, np.uint32), np.empty(T, np.uint8)
            U, B = C.POINTER(C.c_uint), C.POINTER(C.c_ubyte)
            self.hl.check(self.hl.lib.rt_hip_plan_history_fetch(
                self._h, r, cabi._dp(E_v), cabi._dp(nf), cabi._dp(iang), cabi._dp(es), code.ctypes.data_as(U),
                flags.ctypes.data_as(U), filled.ctypes.data_as(B)), "rt_hip_plan_history_fetch")
            out.append(dict(E_v=E_v, nf=nf, I_ang=iang, E_sum=es, failure_code=code, flags=flags, filled=filled))
        return out

    def fetch_history_sum(self) -> list:
        """One dict per record block: the running sum E_v [nv], nf [nx * ny], I_ang [na * nb] and E_sum (a float) of the
        appends that asked for it (waits for the last append)."""
        b, out = self.problem.beam, []
        for r in range(max(1, self.history_info()["n_rec"])):
            E_v, nf, iang, es = np.empty(b.nv), np.empty(b.nx * b.ny), np.empty(b.na * b.nb), np.empty(1)
            self.hl.check(self.hl.lib.rt_hip_plan_history_fetch_sum(self._h, r, cabi._dp(E_v), cabi._dp(nf), cabi._dp(iang),
                                                                    cabi._dp(es)), "rt_hip_plan_history_fetch_sum")
            out.append(dict(E_v=E_v, nf=nf, I_ang=iang, E_sum=float(es[0])))
        return out

    def history_tensors(self) -> list:
        """One dict per record block: torch views (on the plan's device, no copy) of E_v [n_steps][nv], nf [n_steps][ny][nx],
        I_ang [n_steps][nb][na], E_sum [n_steps] (float64), failure_code and flags [n_steps] (int32 views of the 32-bit words);
        after the first append, valid until enable_history is called again; read them on the append's stream."""
        import torch

        b, info, out = self.problem.beam, self.history_info(), []
        T = info["n_steps"]
        for r in range(info["n_rec"]):
            q = [C.c_void_p() for _ in range(6)]
            self.hl.check(self.hl.lib.rt_hip_plan_history_ptrs(self._h, r, *(C.byref(x) for x in q)), "rt_hip_plan_history_ptrs")
            e, n, a, s, c, f = (int(x.value or 0) for x in q)
            words = lambda ptr: _view(ptr, (T // 2 + T % 2,), self.device).view(torch.int32)[:T]   # (blocks of words are padded to 8 bytes)
            out.append(dict(E_v=_view(e, (T, b.nv), self.device), nf=_view(n, (T, b.ny, b.nx), self.device),
                            I_ang=_view(a, (T, b.nb, b.na), self.device), E_sum=_view(s, (T,), self.device),
                            failure_code=words(c), flags=words(f)))
        return out

    def history_sum_tensors(self) -> list:
        """One dict per record block: torch views of the running sum, E_v [nv], nf [ny][nx], I_ang [nb][na], E_sum [1]."""
        out = []
        for r in range(self.history_info()["n_rec"]):
            q = [C.c_void_p() for _ in range(4)]
            self.hl.check(self.hl.lib.rt_hip_plan_history_sum_ptrs(self._h, r, *(C.byref(x) for x in q)), "rt_hip_plan_history_sum_ptrs")
            e, n, a, s = (int(x.value or 0) for x in q)
            out.append(dict(**self._record_views((e, n, a)), E_sum=_view(s, (1,), self.device)))
        return out

    # -- tables -------------------------------------------------------------
    def update_gain(self, gain, stream: int | None = None) -> "Plan":
        """New n, g0, E0 and gv on the plan's grids (include/rt_hip.h, rt_hip_plan_update_gain): everything else about the
        plan stays -- rays, output mode, lent buffers, probe.  `gain`: a Problem, a list of Gain, or a list of per-length
        dicts / tuples (n, g0, E0, gv); entry 0 is ignored.  numpy arrays take the host call; torch tensors on the plan's
        device take the device call on `stream` (a hipStream_t value; default: torch's current stream, so that the
        allocator's ordering holds) and must stay unchanged until the work on that stream has completed.  Shapes, dtypes
        and contiguity are checked here (ValueError); a table the scan rejects -- a non-finite index of refraction -- raises
        RayTraceError and leaves the plan as it was.  With host arrays, self.problem is replaced by one that carries the
        new tables."""
        import copy
        import dataclasses

        old = self.problem.gain
        gv = cabi.GainValues(gain, [(g.Nx, g.Ny) for g in old], self.problem.beam.nv, self.device)
        if gv.on_device:
            if stream is None:
                import torch
                stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = self.hl.lib.rt_hip_plan_update_gain_dev(self._h, gv.N, gv.vals, C.c_void_p(stream))
            self.hl.check(rc, "rt_hip_plan_update_gain_dev")
            self._gain_dev = gv           # (the tensors live at least until the next update)
        else:
            self.hl.check(self.hl.lib.rt_hip_plan_update_gain(self._h, gv.N, gv.vals), "rt_hip_plan_update_gain")
            q = copy.copy(self.problem)
            q.gain = [old[0]] + [dataclasses.replace(old[i], n=t[0], g0=t[1], E0=t[2], gv=t[3]) for i, t in enumerate(gv.tables) if i]
            q.golden_image = q.golden_I_ang = None
            self.problem = q
        return self

    def table_flags(self) -> dict:
        """The four facts of the tables every run is chosen by (rt_hip_plan_table_flags): bounded, ntest_proven,
        gv_nonfinite (0 / 1) and gs_cap (numpy float32)."""
        b, t, g, cap = C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0)
        self.hl.check(self.hl.lib.rt_hip_plan_table_flags(self._h, C.byref(b), C.byref(t), C.byref(g), C.byref(cap)),
                      "rt_hip_plan_table_flags")
        return dict(bounded=b.value, ntest_proven=t.value, gv_nonfinite=g.value, gs_cap=np.float32(cap.value))

    def kernel_ms(self) -> float:
        """Device time of the last run's trace kernel (waits for it)."""
        ms = C.c_float(0)
        self.hl.check(self.hl.lib.rt_hip_plan_kernel_ms(self._h, C.byref(ms)), "rt_hip_plan_kernel_ms")
        return float(ms.value)

    def kernel_times(self) -> tuple:
        """(march_ms, freq_ms) of the last run (waits for it)."""
        a, f = C.c_float(0), C.c_float(0)
        self.hl.check(self.hl.lib.rt_hip_plan_kernel_times(self._h, C.byref(a), C.byref(f)),
                      "rt_hip_plan_kernel_times")
        return float(a.value), float(f.value)

    def last_fused(self) -> bool:
        """The last run took the whole path in one launch (rt_fused.hip): kernel_times() = (launch, 0)."""
        return bool(self.hl.lib.rt_hip_plan_last_fused(self._h))

    def last_march_instance(self) -> int:
        """Bits of the march instance of the last run (include/rt_hip.h): 1 short divisions, 2 h1 pruned, 4 no |n - n0| test,
        8 h2 and h4 pruned."""
        return int(self.hl.lib.rt_hip_plan_last_march_instance(self._h))

    def set_timing_ring(self, n_runs: int) -> "Plan":
        """Keep the kernel-event triples of the last n_runs runs (include/rt_hip.h)."""
        self.hl.check(self.hl.lib.rt_hip_plan_set_timing_ring(self._h, int(n_runs)), "rt_hip_plan_set_timing_ring")
        self._ring = int(n_runs)
        return self

    def ring_times(self) -> list:
        """[(march_ms, freq_ms)] of the most recent runs, oldest first (waits for the last run)."""
        n = self._ring
        if n < 1:
            return []
        a = np.zeros(n, np.float32)
        f = np.zeros(n, np.float32)
        got = C.c_int(0)
        self.hl.check(self.hl.lib.rt_hip_plan_ring_times(self._h, cabi._fp(a), cabi._fp(f), n, C.byref(got)),
                      "rt_hip_plan_ring_times")
        return [(float(a[i]), float(f[i])) for i in range(got.value)]

    def fetch_probe(self) -> dict:
        n = self.n_rays
        S = (self.problem.N - 1) * cabi.RT_N_SUB
        out = dict(gvl=np.zeros((n, S), np.float32), evl=np.zeros((n, S), np.float32),
                   ivl=np.zeros((n, S), np.int32), ray2=np.zeros(n, cabi.RAY_DTYPE),
                   flags=np.zeros(n, np.uint32), steps=np.zeros(n, np.uint32))
        P = C.POINTER
        rc = self.hl.lib.rt_hip_plan_fetch_probe(
            self._h, cabi._fp(out["gvl"]), cabi._fp(out["evl"]), out["ivl"].ctypes.data_as(P(C.c_int32)),
            cabi.rays_ptr(out["ray2"]), out["flags"].ctypes.data_as(P(C.c_uint32)),
            out["steps"].ctypes.data_as(P(C.c_uint32)))
        self.hl.check(rc, "rt_hip_plan_fetch_probe")
        return out

    @property
    def image_ptr(self) -> int:
        return int(self.hl.lib.rt_hip_plan_image_ptr(self._h) or 0)

    @property
    def iang_ptr(self) -> int:
        return int(self.hl.lib.rt_hip_plan_iang_ptr(self._h) or 0)

    def close(self) -> None:
        if self._h:
            self.hl.lib.rt_hip_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_loop(entry: str, problem: Problem, rays, device: int, lead: tuple = (), seeds=None, scales=None, ase: bool = False,
               image: bool = False) -> dict:
    """One call of the host-pointer entry point `entry` of the C ABI: the problem, the rays (None: the problem's ray grid as a
    list) and the seeds (None: the entry point takes none; `ase`: an entry point of ASE seeds -- no creation seed, `scales`
    behind the seeds) marshalled, the outputs allocated -- `image`: the cube and I_ang; else E_v, nf and I_ang with the leading
    shape `lead` of the rows: (), (L,), (ns, L), (nr,) or (nr, L) --, the call timed and checked.  Returns dict(outs = the
    output arrays, codes = the failure codes [lead], failure_code = their OR, failed_rays, stats, call_ms = the C call alone
    (what a C++ caller of the adapter waits for))."""
    hl = HipLibrary.get()
    m = cabi.Marshalled(problem)
    if rays is None:
        rays = problem.build_rays()
    rays = np.ascontiguousarray(rays, dtype=cabi.RAY_DTYPE)
    b = problem.beam
    sizes = (b.nx * b.ny * b.nv, b.na * b.nb) if image else (b.nv, b.nx * b.ny, b.na * b.nb)
    outs = [np.zeros(lead + (n,)) for n in sizes]
    codes = np.zeros(lead, np.uint32)
    nfail = C.c_int(0)
    failed = np.zeros(cabi.RT_N_FAILED_MAX, dtype=cabi.RAY_DTYPE)
    st = cabi.RtStats()
    args = [device, m.N, C.byref(m.beam), m.gain] + ([] if ase else [m.seed_ref])
    args += [problem.method, cabi.rays_ptr(rays), len(rays), problem.scale]
    if seeds is not None:
        _, arr, _keep = _seed_array(seeds, entry, "a call")   # (checked by the caller: marshalled only)
        args += [len(seeds), arr] + ([cabi._dp(scales) if scales is not None else None] if ase else [])
    args += [cabi._dp(o) for o in outs] + [codes.ctypes.data_as(C.POINTER(C.c_uint)), cabi.rays_ptr(failed), cabi.RT_N_FAILED_MAX,
                                          C.byref(nfail), C.byref(st)]
    t0 = time.perf_counter()
    rc = getattr(hl.lib, entry)(*args)
    call_ms = (time.perf_counter() - t0) * 1e3
    hl.check(rc, entry)
    return dict(outs=outs, codes=codes, failure_code=int(np.bitwise_or.reduce(codes, axis=None)), failed_rays=failed[:nfail.value].copy(),
                stats={k: getattr(st, k) for k, _ in cabi.RtStats._fields_}, call_ms=call_ms)


def _rec(out: dict, index: tuple, **first) -> dict:
    """Row `index` of the outputs of a _host_loop as a record: dict(**first, E_v, nf, I_ang, failure_code)."""
    E_v, nf, iang = out["outs"]
    return dict(**first, E_v=E_v[index].copy(), nf=nf[index].copy(), I_ang=iang[index].copy(), failure_code=int(out["codes"][index]))


def _curve(out: dict, L: int, *row) -> list:
    """The records of row `row` at n = 2 .. L + 1 lengths: [dict(n, E_v, nf, I_ang, failure_code)]."""
    return [_rec(out, row + (i,), n=i + 2) for i in range(L)]


def _tail(out: dict, *keys) -> dict:
    """What every loop returns behind its outputs: failure_code, failed_rays, stats, and of `keys` what the loop has always had."""
    return {k: out[k] for k in ("failure_code", "failed_rays", "stats") + keys}


def image_loop(problem: Problem, rays: np.ndarray | None = None, device: int = 0) -> dict:
    """RayTraceImageHipLoop through the host-pointer entry point
    (rt_hip_image_loop): upload, trace, download.  Returns image, I_ang,
    failure_code, failed_rays, stats."""
    out = _host_loop("rt_hip_image_loop", problem, rays, device, image=True)
    return dict(image=out["outs"][0], I_ang=out["outs"][1], **_tail(out, "call_ms"))


def step_loop(problem: Problem, rays: np.ndarray | None = None, device: int = 0) -> dict:
    """image_loop with the small outputs (rt_hip_step_loop): E_v [nv], nf [nx * ny], I_ang, failure_code, failed_rays,
    stats -- the image cube is never built."""
    out = _host_loop("rt_hip_step_loop", problem, rays, device)
    return dict(zip(("E_v", "nf", "I_ang"), out["outs"]), **_tail(out, "call_ms"))


def step_history_loop(p: Problem, snapshots, seeds=None, scales=None, accumulate: bool = False, weights=None, device: int = 0) -> dict:
    """A time loop over the gain tables `snapshots` (what Plan.update_gain takes, one entry per step) with the step records
    filed on the device: one plan of `p` in step mode on its ray grid (with ASE seeds when `seeds` is given: Plan.set_ase_seeds
    with `scales`), per snapshot update_gain -> run -> history_append(i, weights[i], accumulate), and ONE fetch at the end.
    A convenience over the plan API.  Returns dict(records=Plan.fetch_history(), sums=Plan.fetch_history_sum() or None,
    filled)."""
    snapshots = list(snapshots)
    if not snapshots:
        raise ValueError("step_history_loop: no snapshots")
    weights = [1.0] * len(snapshots) if weights is None else [float(w) for w in weights]
    if len(weights) != len(snapshots):
        raise ValueError(f"step_history_loop: {len(weights)} weights for {len(snapshots)} snapshots")
    with Plan(p, device=device) as plan:
        plan.set_ray_grid().enable_step()
        if seeds is not None:
            plan.set_ase_seeds(seeds, scales)
        plan.enable_history(len(snapshots))
        for i, tables in enumerate(snapshots):
            plan.update_gain(tables).run().history_append(i, weights[i], accumulate)
        recs = plan.fetch_history()
        return dict(records=recs, sums=plan.fetch_history_sum() if accumulate else None, filled=recs[0]["filled"])


def multi_step_loop(problem: Problem, rays: np.ndarray | None = None, n_devices: int = 0) -> dict:
    """step_loop on all devices of the node (rt_hip_multi_step_loop): every device traces its share of the rays on the
    full beam into one buffer (E_v | nf | I_ang), ONE RCCL sum-reduce assembles them (include/rt_hip.h).  n_devices <= 0:
    every device.  Returns what step_loop returns plus `mode` (3 = strided ray grid, 2 = chunks of the list)."""
    out = _host_loop("rt_hip_multi_step_loop", problem, rays, n_devices)
    return dict(zip(("E_v", "nf", "I_ang"), out["outs"]), **_tail(out), mode=int(HipLibrary.get().lib.rt_hip_multi_last_mode()),
                call_ms=out["call_ms"])


def seed_step_loop(problem: Problem, seeds, rays: np.ndarray | None = None, device: int = 0) -> dict:
    """The step records of the seed beams `seeds` (a list of Seed, at most RT_N_SEED_MAX) from ONE march of the
    problem's rays (rays None: the problem's ray grid, generated on the device): a convenience over a Plan in step mode
    with a seed set.  The problem must carry a seed -- it decides the gain-only mode and the method; it is not part of
    the set.  Returns dict(records = [dict(E_v, nf, I_ang, failure_code)] per seed, failure_code = their OR,
    failed_rays = the rays that fail under any seed, stats)."""
    with Plan(problem, device) as plan:   # (without a device: RayTraceError, "no HIP device", as the other entries)
        plan.set_seeds(seeds)
        if rays is None:
            plan.set_ray_grid()
        else:
            plan.set_rays(rays)
        plan.enable_step().run()
        records = plan.fetch_seed_steps()
        info = plan.fetch()
    return dict(records=records, failure_code=info["failure_code"], failed_rays=info["failed_rays"], stats=info["stats"])


def _ase_loop_args(who: str, problem: Problem, seeds, scales) -> tuple:
    """(seeds, scales) of a loop with ASE seeds, checked: 1 .. RT_N_SEED_MAX Seeds, an emission problem, one scale per seed."""
    seeds = _taken_seeds(who, seeds)
    if problem.seed is not None:
        raise ValueError(f"{who}: the problem carries a seed; the ASE record needs an emission problem")
    return seeds, _scales_arg(who, scales, len(seeds))


def full_step_loop(problem: Problem, seeds, scales=None, rays: np.ndarray | None = None, device: int = 0) -> dict:
    """The whole per-step record from ONE march of the problem's rays (rt_hip_full_step_loop, host pointers; rays None: the
    problem's ray grid as a list): the emission record of `problem`, which must carry no seed and tables with E0, and the
    gain-only record of the same problem under each Seed of `seeds` (1 .. RT_N_SEED_MAX) with scale scales[s] (None: the
    problem's scale).  Returns dict(ase = rec, seeds = [rec ...], failure_code = the OR of the codes, failed_rays, stats),
    every rec dict(E_v, nf, I_ang, failure_code).  No seed or too many, an entry that is not a Seed, scales of another
    length or a problem with a seed is a ValueError raised here, before any native call."""
    seeds, sc = _ase_loop_args("full_step_loop", problem, seeds, scales)
    out = _host_loop("rt_hip_full_step_loop", problem, rays, device, (1 + len(seeds),), seeds, sc, ase=True)
    recs = [_rec(out, (r,)) for r in range(1 + len(seeds))]
    return dict(ase=recs[0], seeds=recs[1:], **_tail(out))


def full_length_scan_loop(problem: Problem, seeds, scales=None, rays: np.ndarray | None = None, device: int = 0) -> dict:
    """The whole per-step record at every plasma length n = 2 .. N from ONE forward march of the problem's rays
    (rt_hip_full_length_scan_loop, host pointers; rays None: the problem's ray grid as a list): the emission record of
    `problem`, which must carry no seed and tables with E0, and the gain-only record of the same problem under each Seed of
    `seeds` (1 .. RT_N_SEED_MAX) with scale scales[s] (None: the problem's scale).  Returns dict(ase = [rec per n], seeds =
    [[rec per n] per seed], failure_code = the OR of the codes, failed_rays, stats), every rec dict(n, E_v, nf, I_ang,
    failure_code).  What the scan does not take, no seed or too many, an entry that is not a Seed, scales of another length
    or a problem with a seed is a ValueError raised here, before any native call."""
    return _full_scan_loop("full_length_scan_loop", 2, "the scan takes the forward method (2) only", problem, seeds, scales, rays, device)


def full_suffix_scan_loop(problem: Problem, seeds, scales=None, rays: np.ndarray | None = None, device: int = 0) -> dict:
    """The whole per-step record of the run of the LAST n lengths, n = 2 .. N, from ONE backward march of the problem's rays
    (rt_hip_full_suffix_scan_loop, host pointers; rays None: the problem's ray grid as a list): the emission record of
    problem.suffix_lengths(problem, n) and the gain-only record of that problem under each Seed of `seeds`
    (1 .. RT_N_SEED_MAX) with scale scales[s] (None: the problem's scale).  Returns what full_length_scan_loop returns.  The
    forward method, N < 3 or more than RT_N_SCAN_MAX lengths, no seed or too many, an entry that is not a Seed, scales of
    another length or a problem with a seed is a ValueError raised here, before any native call."""
    return _full_scan_loop("full_suffix_scan_loop", 1, "the suffix scan takes the backward method (1) only", problem, seeds, scales, rays, device)


def _full_scan_loop(who: str, method: int, method_text: str, problem: Problem, seeds, scales, rays, device: int) -> dict:
    """full_length_scan_loop (method 2) and full_suffix_scan_loop (method 1): the checks, the call and the rows."""
    _scan_takes(who, problem, method, method_text)
    seeds, sc = _ase_loop_args(who, problem, seeds, scales)
    L, nr = problem.N - 1, 1 + len(seeds)
    out = _host_loop("rt_hip_" + who, problem, rays, device, (nr, L), seeds, sc, ase=True)
    curves = [_curve(out, L, r) for r in range(nr)]
    return dict(ase=curves[0], seeds=curves[1:], **_tail(out))


def _scan_loop(who: str, method: int, method_text: str, problem: Problem, rays, device: int) -> dict:
    """length_scan_loop (method 2) and suffix_scan_loop (method 1): the checks, the call and the rows."""
    _scan_takes(who, problem, method, method_text)
    out = _host_loop("rt_hip_" + who, problem, rays, device, (problem.N - 1,))
    return dict(records=_curve(out, problem.N - 1), **_tail(out))


def length_scan_loop(problem: Problem, rays: np.ndarray | None = None, device: int = 0) -> dict:
    """The step record at every plasma length n = 2 .. N from ONE forward march of the problem's rays
    (rt_hip_length_scan_loop; rays None: the problem's ray grid as a list, which the library recognises).  Returns
    dict(records = [dict(n, E_v, nf, I_ang, failure_code)], failure_code = the OR of the codes, failed_rays = the rays
    that fail at any length, stats).  A problem the scan does not take (backward method, N < 3, more than RT_N_SCAN_MAX
    lengths) is a ValueError raised here, before any native call."""
    return _scan_loop("length_scan_loop", 2, "the scan takes the forward method (2) only", problem, rays, device)


def suffix_scan_loop(problem: Problem, rays: np.ndarray | None = None, device: int = 0) -> dict:
    """The step record of the run of the last n lengths, n = 2 .. N, from ONE backward march of the problem's rays
    (rt_hip_suffix_scan_loop; rays None: the problem's ray grid as a list, which the library recognises).  Returns
    dict(records = [dict(n, E_v, nf, I_ang, failure_code)], failure_code = the OR of the codes, failed_rays = the rays
    that fail under any record, stats).  A problem the scan does not take (forward method, N < 3, more than RT_N_SCAN_MAX
    lengths) is a ValueError raised here, before any native call."""
    return _scan_loop("suffix_scan_loop", 1, "the scan takes the backward method (1) only", problem, rays, device)


def seed_length_scan_loop(problem: Problem, seeds, rays: np.ndarray | None = None, device: int = 0) -> dict:
    """The step record of every seed beam of `seeds` (a list of Seed, 1 .. RT_N_SEED_MAX) at every plasma length n = 2 .. N
    from ONE forward march of the problem's rays (rt_hip_seed_length_scan_loop; rays None: the problem's ray grid as a list,
    which the library recognises).  The problem must carry a seed -- it decides the gain-only mode and the method; it is not
    part of the set.  Returns dict(records = per seed [dict(n, E_v, nf, I_ang, failure_code)], failure_code = the OR of the
    codes, failed_rays = the rays that fail anywhere, stats).  What the scan does not take (backward method, N < 3, more than
    RT_N_SCAN_MAX lengths), no seed or more than RT_N_SEED_MAX, or an entry that is not a Seed is a ValueError raised here,
    before any native call."""
    return _seed_scan_loop("seed_length_scan_loop", 2, "the scan takes the forward method (2) only", problem, seeds, rays, device)


def seed_suffix_scan_loop(problem: Problem, seeds, rays: np.ndarray | None = None, device: int = 0) -> dict:
    """The step record of every seed beam of `seeds` (a list of Seed, 1 .. RT_N_SEED_MAX) of the run of the last n lengths,
    n = 2 .. N, from ONE backward march of the problem's rays (rt_hip_seed_suffix_scan_loop; rays None: the problem's ray
    grid as a list).  The problem must carry a seed, which is not part of `seeds`.  Returns what seed_length_scan_loop
    returns, records[s][n - 2] the record of seed s of the last n lengths.  What the scan does not take (forward method,
    N < 3, more than RT_N_SCAN_MAX lengths), no seed or more than RT_N_SEED_MAX, or an entry that is not a Seed is a
    ValueError raised here, before any native call."""
    return _seed_scan_loop("seed_suffix_scan_loop", 1, "the suffix scan takes the backward method (1) only", problem, seeds, rays, device)


def _seed_scan_loop(who: str, method: int, method_text: str, problem: Problem, seeds, rays, device: int) -> dict:
    """seed_length_scan_loop (method 2) and seed_suffix_scan_loop (method 1): the checks, the call and the rows."""
    _scan_takes(who, problem, method, method_text)
    seeds = _taken_seeds(who, seeds)
    L = problem.N - 1
    out = _host_loop("rt_hip_" + who, problem, rays, device, (len(seeds), L), seeds)
    return dict(records=[_curve(out, L, s) for s in range(len(seeds))], **_tail(out))


def step_outputs_from_image(problem: Problem, image) -> dict:
    """The definition of the step outputs as reductions of an image cube [ny * nx * nv] (k fastest, p = ix + iy nx):
    E_v[k] = sum_p image[k + nv p], nf[p] = sum_k 2 dv[k] image[k + nv p] -- accumulated in np.longdouble, returned as
    float64.  Needs no device."""
    b = problem.beam
    cube = np.asarray(image, dtype=np.float64).reshape(b.nx * b.ny, b.nv)
    w = (2.0 * np.asarray(b.dv, dtype=np.float64)).astype(np.longdouble)   # (2 dv is exact: RayTraceImageCPU.cpp:66)
    E_v = np.zeros(b.nv, np.longdouble)
    nf = np.empty(b.nx * b.ny)
    step = max(1, (1 << 22) // b.nv)                      # pixels per block: the long-double copy stays at 64 MB
    for lo in range(0, b.nx * b.ny, step):
        part = cube[lo:lo + step].astype(np.longdouble)
        E_v += part.sum(axis=0)
        nf[lo:lo + step] = (part * w[None, :]).sum(axis=1)
    return dict(E_v=E_v.astype(np.float64), nf=nf)


def multi_image_loop(problem: Problem, rays: np.ndarray | None = None, n_devices: int = 0) -> dict:
    """RayTraceImageHipMultiGPULoop through rt_hip_multi_image_loop: all devices of the node, one RCCL
    collective per image (include/rt_hip.h).  n_devices <= 0: every device.  Returns what image_loop
    returns plus `mode` (1 = pixel-column tiles + gather, 2 = ray chunks + sum-reduce)."""
    out = _host_loop("rt_hip_multi_image_loop", problem, rays, n_devices, image=True)
    return dict(image=out["outs"][0], I_ang=out["outs"][1], **_tail(out), mode=int(HipLibrary.get().lib.rt_hip_multi_last_mode()),
                call_ms=out["call_ms"])


def ray_list_grid_dims(rays: np.ndarray):
    """(nx, ny, na, nb) if the list is a whole tensor grid in create_image's order, else None (host only)."""
    hl = HipLibrary.get()
    rays = np.ascontiguousarray(rays, dtype=cabi.RAY_DTYPE)
    dims = (C.c_int * 4)()
    ok = hl.lib.rt_hip_ray_list_grid_dims(cabi.rays_ptr(rays), len(rays), C.byref(dims))
    return tuple(dims) if ok else None


_FAILURE_TEXT = {1: "Invalid ray detected", 2: "Negitive intensity detected", 3: "NaNs detected in intensity"}


def create_image(problem: Problem, method: str = "auto", device: int = 0, device_rays: bool = True) -> dict:
    """Mirror of RayTrace::create_image (src/RayTraceImage.cpp:227-434) with the
    arms this backend adds: "hip" (one device) and "hip-multigpu" (all devices of
    the node behind rt_hip_multi_image_loop: pixel-column tiles + RCCL gather for
    ASE, ray chunks + RCCL sum-reduce otherwise).  "auto" resolves to "hip".  Any other method string
    is an error -- the CPU/OpenMP/CUDA arms belong to the reference.

    Returns dict(image [ny][nx][nv] flat, I_ang, stats)."""
    problem.validate()
    m = method.lower()
    if m == "auto":
        m = "hip"
    if m == "hip":
        with Plan(problem, device) as plan:
            if device_rays:
                plan.set_ray_grid()
            else:
                plan.set_rays(problem.build_rays())
            out = plan.run().fetch()
    elif m == "hip-multigpu":
        out = multi_image_loop(problem)
    else:
        raise RayTraceError("Unknown method: " + m)
    if out["failure_code"] != 0:
        msgs = [t for bit, t in _FAILURE_TEXT.items() if out["failure_code"] & (1 << bit)]
        raise RayTraceError("Some rays failed: " + "; ".join(msgs))
    return out


def calc_rays(problem: Problem, rays, method: int | None = None, device: int = 0) -> dict:
    """n calls of RayTrace::calc_ray (src/RayTraceImage.cpp:189-204) in one, through rt_hip_calc_rays: host arrays
    in, host arrays out, device memory bounded for any n.  `rays`: RAY_DTYPE records or an [n][4] float64 array of
    (x, y, a, b), rounded to float as calc_ray rounds its arguments.

    Returns dict(Iv [n][K], ray2 (RAY_DTYPE), err [n] int32, stats)."""
    hl = HipLibrary.get()
    m = cabi.Marshalled(problem)
    rays = np.asarray(rays)
    r4 = cabi.rays_to_array(rays) if rays.dtype == cabi.RAY_DTYPE else cabi.rays_to_array(cabi.rays_from_array(rays))
    r4 = np.ascontiguousarray(r4, np.float64)
    n, K = r4.shape[0], problem.beam.nv
    Iv = np.empty((n, K))
    ray2 = np.zeros((n, 4))
    err = np.zeros(n, np.int32)
    st = cabi.RtStats()
    rc = hl.lib.rt_hip_calc_rays(device, m.N, problem.beam.dz, m.gain, m.seed_ref, K,
                                 problem.method if method is None else method, cabi._dp(r4), n, cabi._dp(Iv),
                                 cabi._dp(ray2), err.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st))
    hl.check(rc, "rt_hip_calc_rays")
    return dict(Iv=Iv, ray2=cabi.rays_from_array(ray2), err=err,
                stats={k: getattr(st, k) for k, _ in cabi.RtStats._fields_})


def calc_rays_lengths(problem: Problem, rays, exact: bool = False, device: int = 0) -> dict:
    """RayTrace::calc_ray for every ray at EVERY plasma length n = 2 .. N, from one march: one call over a plan in length
    spectra mode (Plan.enable_length_spectra).  The problem's method decides the sub-problems: prefix_lengths(n) with the
    forward method, suffix_lengths(n) with the backward one.  `rays`: RAY_DTYPE records or an [n][4] float64 array of
    (x, y, a, b), rounded to float as calc_ray rounds its arguments; `exact`: Plan.set_exact_emission.  Device memory is
    (N - 1) n K 8 bytes: there is no chunking as in calc_rays.

    Returns dict(lengths=[dict(n, Iv [n_rays][K], ray2 (RAY_DTYPE), err [n_rays] int32)], failure_code, failed_rays, stats)."""
    if problem.N < 3 or problem.N - 1 > cabi.RT_N_SCAN_MAX:
        raise ValueError(f"calc_rays_lengths: N = {problem.N}; length spectra take 3 <= N <= RT_N_SCAN_MAX + 1 = {cabi.RT_N_SCAN_MAX + 1}")
    rays = np.asarray(rays)
    if rays.dtype != cabi.RAY_DTYPE:
        rays = cabi.rays_from_array(np.asarray(rays, np.float64).reshape(-1, 4))
    with Plan(problem, device=device) as plan:
        plan.set_rays(rays)
        if exact:
            plan.set_exact_emission(True)
        plan.enable_length_spectra(True).run()
        out = plan.fetch(want_image=False)
        return dict(lengths=plan.fetch_length_spectra(), failure_code=out["failure_code"], failed_rays=out["failed_rays"], stats=out["stats"])


def _rays_arg(rays):
    rays = np.asarray(rays)
    if rays.dtype != cabi.RAY_DTYPE:
        rays = cabi.rays_from_array(np.asarray(rays, np.float64).reshape(-1, 4))
    return rays


def calc_rays_seeds(problem: Problem, seeds, rays, device: int = 0) -> dict:
    """RayTrace::calc_ray for every ray under every seed beam of `seeds` (1 .. RT_N_SEED_MAX Seed records), from one march:
    one call over a plan in spectra mode with spectra seeds (Plan.set_spectra_seeds).  `problem` must carry a seed (it makes
    the plan gain-only; it is not among the seeds unless passed again); `rays` as calc_rays_lengths takes them.  Device
    memory is n_seed n K 8 bytes: there is no chunking as in calc_rays.

    Returns dict(seeds=[dict(Iv [n_rays][K], ray2 (RAY_DTYPE), err [n_rays] int32)], failure_code, failed_rays, stats)."""
    seeds = _taken_seeds("calc_rays_seeds", seeds)   # (the refusals of the Python face, before a plan exists)
    rays = _rays_arg(rays)
    with Plan(problem, device=device) as plan:
        plan.set_rays(rays)
        plan.enable_spectra(True).set_spectra_seeds(seeds).run()
        out = plan.fetch(want_image=False)
        return dict(seeds=plan.fetch_seed_spectra(), failure_code=out["failure_code"], failed_rays=out["failed_rays"], stats=out["stats"])


def calc_rays_ase_seeds(problem: Problem, seeds, rays, exact: bool = False, device: int = 0) -> dict:
    """RayTrace::calc_ray for every ray of an EMISSION problem and of the same problem under every seed beam of `seeds`
    (1 .. RT_N_SEED_MAX Seed records), from one march: one call over a plan in spectra mode with ASE seeds
    (Plan.set_spectra_ase_seeds).  `problem` must carry no seed and tables with E0; `rays` as calc_rays_lengths takes them;
    `exact`: rt_hip_plan_set_exact_emission.  Device memory is (1 + n_seed) n K 8 bytes: there is no chunking as in calc_rays.

    Returns dict(ase=dict(Iv [n_rays][K], ray2 (RAY_DTYPE), err [n_rays] int32), seeds=[dict ...], failure_code, failed_rays,
    stats)."""
    seeds = _taken_seeds("calc_rays_ase_seeds", seeds)   # (the refusals of the Python face, before a plan exists)
    rays = _rays_arg(rays)
    with Plan(problem, device=device) as plan:
        plan.set_rays(rays)
        if exact:
            plan.set_exact_emission(True)
        plan.enable_spectra(True).set_spectra_ase_seeds(seeds).run()
        out = plan.fetch(want_image=False)
        full = plan.fetch_full_spectra()
        return dict(ase=full["ase"], seeds=full["seeds"], failure_code=out["failure_code"], failed_rays=out["failed_rays"], stats=out["stats"])


def calc_rays_seeds_lengths(problem: Problem, seeds, rays, device: int = 0) -> dict:
    """calc_rays_seeds at EVERY plasma length n = 2 .. N, from one march: one call over a plan in length spectra mode with
    spectra seeds.  The problem's method decides the sub-problems as in calc_rays_lengths.  Device memory is
    n_seed (N - 1) n K 8 bytes.

    Returns dict(seeds=[[dict(n, Iv, ray2, err)] for n = 2 .. N] per seed, failure_code, failed_rays, stats)."""
    if problem.N < 3 or problem.N - 1 > cabi.RT_N_SCAN_MAX:
        raise ValueError(f"calc_rays_seeds_lengths: N = {problem.N}; length spectra take 3 <= N <= RT_N_SCAN_MAX + 1 = {cabi.RT_N_SCAN_MAX + 1}")
    seeds = _taken_seeds("calc_rays_seeds_lengths", seeds)
    rays = _rays_arg(rays)
    with Plan(problem, device=device) as plan:
        plan.set_rays(rays)
        plan.enable_length_spectra(True).set_spectra_seeds(seeds).run()
        out = plan.fetch(want_image=False)
        return dict(seeds=plan.fetch_seed_length_spectra(), failure_code=out["failure_code"], failed_rays=out["failed_rays"], stats=out["stats"])


def calc_rays_ase_seeds_lengths(problem: Problem, seeds, rays, exact: bool = False, device: int = 0) -> dict:
    """calc_rays_ase_seeds at EVERY plasma length n = 2 .. N, from one march: one call over a plan in length spectra mode with
    ASE seeds (Plan.set_length_spectra_ase_seeds).  `problem` must carry no seed and tables with E0; its method decides the
    sub-problems as in calc_rays_lengths; `exact`: rt_hip_plan_set_exact_emission.  Device memory is
    (1 + n_seed) (N - 1) n K 8 bytes.

    Returns dict(ase=[dict(n, Iv, ray2, err)] for n = 2 .. N, seeds=[the same per seed], failure_code, failed_rays, stats)."""
    if problem.N < 3 or problem.N - 1 > cabi.RT_N_SCAN_MAX:
        raise ValueError(f"calc_rays_ase_seeds_lengths: N = {problem.N}; length spectra take 3 <= N <= RT_N_SCAN_MAX + 1 = {cabi.RT_N_SCAN_MAX + 1}")
    seeds = _taken_seeds("calc_rays_ase_seeds_lengths", seeds)   # (the refusals of the Python face, before a plan exists)
    rays = _rays_arg(rays)
    with Plan(problem, device=device) as plan:
        plan.set_rays(rays)
        if exact:
            plan.set_exact_emission(True)
        plan.enable_length_spectra(True).set_length_spectra_ase_seeds(seeds).run()
        out = plan.fetch(want_image=False)
        full = plan.fetch_full_length_spectra()
        return dict(ase=full["ase"], seeds=full["seeds"], failure_code=out["failure_code"], failed_rays=out["failed_rays"], stats=out["stats"])


def calc_ray(problem: Problem, ray, method: int | None = None, device: int = 0):
    """Mirror of RayTrace::calc_ray for one ray (x, y, a, b): returns (err, Iv [K], ray2 (x, y, a, b))."""
    ray = np.asarray(ray)
    one = ray.reshape(1) if ray.dtype == cabi.RAY_DTYPE else np.asarray(ray, np.float64).reshape(1, 4)
    out = calc_rays(problem, one, method, device)
    return int(out["err"][0]), out["Iv"][0], tuple(float(out["ray2"][0][k]) for k in ("x", "y", "a", "b"))


def calc_ray_path(problem: Problem, x, y, a, b, method: int | None = None, c: float = 0.5, device: int = 0):
    """Mirror of RayTrace::calc_ray_path (src/RayTraceImage.cpp:440-477): trace the rays of the
    tensor grid x * y * a * b through the problem's tables and return the path of each ray.

    Returns (xr, yr, Ir, n_errors): float32 arrays laid out as the reference lays them out,
    index = N2 * (i + j*Nx + k*Nx*Ny + m*Nx*Ny*Na) + step with N2 = 3 (N-1) + 1, i.e. shape
    [Nb][Na][Ny][Nx][N2] in C order."""
    grids = [np.ascontiguousarray(g, np.float64) for g in (x, y, a, b)]
    nx, ny, na, nb = (len(g) for g in grids)
    with Plan(problem, device, method=method) as plan:
        plan.set_step_factor(c).enable_path().set_ray_grid(0, 1, nx * ny * na * nb, grids=grids)
        out = plan.run().fetch_path()
    N2 = out["x"].shape[1]

    def lay(v):  # ray order is i, j, k, m with m fastest
        return np.ascontiguousarray(v.reshape(nx, ny, na, nb, N2).transpose(3, 2, 1, 0, 4))

    return lay(out["x"]), lay(out["y"]), lay(out["I"]), int((out["err"] != 0).sum())
