"""ctypes mirror of include/rt_hip.h (the C ABI of the HIP backend).

The same record types feed the product library (csrc/librt_hip.so) and, in
tests only, the CPU oracle -- so one marshalled problem is handed to both
sides.  Nothing here computes; it only lays numpy arrays out as the PODs the
header declares.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

RT_N_SUB = 3
RT_N_FAILED_MAX = 32
RT_N_SEED_MAX = 2
RT_N_SCAN_MAX = 32

RT_OK, RT_ERR_ARG, RT_ERR_NO_DEVICE, RT_ERR_HIP, RT_ERR_NOMEM = range(5)

c_double_p = C.POINTER(C.c_double)
c_float_p = C.POINTER(C.c_float)


class RtRay(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("a", C.c_float), ("b", C.c_float)]


#: numpy view of rt_ray[] (16-byte records, reference ray_struct layout)
RAY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("a", "<f4"), ("b", "<f4")])


class RtBeam(C.Structure):
    _fields_ = [
        ("nx", C.c_int32), ("ny", C.c_int32), ("na", C.c_int32), ("nb", C.c_int32),
        ("nv", C.c_int32),
        ("dx", C.c_double), ("dy", C.c_double), ("da", C.c_double), ("db", C.c_double),
        ("dz", C.c_double),
        ("x", c_double_p), ("y", c_double_p), ("a", c_double_p), ("b", c_double_p),
        ("dv", c_double_p),
    ]


class RtGain(C.Structure):
    _fields_ = [
        ("Nx", C.c_int32), ("Ny", C.c_int32), ("Nv", C.c_int32),
        ("x", c_double_p), ("y", c_double_p), ("n", c_double_p),
        ("g0", c_float_p), ("E0", c_float_p), ("gv", c_float_p),
    ]


class RtGainValues(C.Structure):
    """rt_gain_values: the values of one length of a table update, shapes as in the RtGain the plan was created with."""
    _fields_ = [("n", c_double_p), ("g0", c_float_p), ("E0", c_float_p), ("gv", c_float_p)]


class RtSeed(C.Structure):
    _fields_ = [
        ("dim", C.c_int32 * 5),
        ("x", c_double_p * 5),
        ("f", c_double_p * 5),
        ("f0", C.c_double),
    ]


class RtStats(C.Structure):
    _fields_ = [
        ("n_rays", C.c_uint64), ("cell_steps", C.c_uint64), ("n_escaped", C.c_uint64),
        ("n_skipped", C.c_uint64), ("kernel_ms", C.c_float), ("total_ms", C.c_float),
        ("march_ms", C.c_float), ("freq_ms", C.c_float),
    ]


def _fields(spec: str) -> list:
    """'uint: a b; ull: c' -> ctypes fields in that order (the diagnostic structs of rt_hip_debug_run_shape)."""
    types = {"uint": C.c_uint, "int": C.c_int, "ull": C.c_ulonglong, "float": C.c_float}
    return [(name, types[t.strip()]) for t, names in (g.split(":") for g in spec.split(";")) for name in names.split()]


class RtRunFacts(C.Structure):
    _fields_ = _fields(
        "uint: size; int: cu_count; ull: lds_limit n_rays blob_bytes n_iang; uint: n_tiles;"
        "int: K Kp L rays_per_pixel n_seed march_prune method; float: c_h3; uint: safe debug;"
        "int: use_emis own_cells exclusive path_on spectra_on step_on step_one_launch probe_on has_ray_list host_rays"
        " tables_bounded ntest_proven gv_has_nan; int: occupancy_per_cu scan_on")


class RtRunShape(C.Structure):
    _fields_ = _fields(
        "uint: size; int: kind lds_tab; uint: n_launch bthr; int: mode bounded opt last_march_inst; ull: mlds;"
        "uint: grid chunk park spin_limit no_skip late_first late_waves late_chunks; int: occupancy_asked; int: maxq nslot;"
        "uint: off_exp off_iang off_ctl off_rem off_nodes off_buf node_cap n_free per_wave split k_part n_consumers"
        " consumers_first; ull: flds tile_links; uint: fgrid; int: key_s6 key_emis key_excl;"
        "int: pass_kind pass_wg_waves pass_in_lds pass_nslot; ull: pass_lds; uint: pass_grid pass_fetch_shift")


class RtHistoryFacts(C.Structure):
    _fields_ = _fields("uint: size; int: nv nx ny na nb n_rec n_steps accumulate")


class RtHistoryLayout(C.Structure):
    _fields_ = _fields(
        "uint: size; uint: chunk wg_threads pix_wg aux_wg wg_per_rec grid; ull: bytes scratch_bytes;"
        "ull: off_E_v rec_E_v step_E_v off_nf rec_nf step_nf off_I_ang rec_I_ang step_I_ang;"
        "ull: off_E_sum rec_E_sum off_code rec_code off_flags rec_flags off_filled;"
        "ull: off_acc_E_v rec_acc_E_v off_acc_nf rec_acc_nf off_acc_I_ang rec_acc_I_ang off_acc_E_sum;"
        "ull: off_part off_pflag")


def _dp(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(c_double_p)


def _fp(a: np.ndarray | None):
    if a is None:
        return c_float_p()
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(c_float_p)


def seed_record(seed, keep: list) -> "RtSeed":
    """A Seed laid out as rt_seed; the arrays it points into are appended to `keep`."""
    s = RtSeed()
    for i in range(5):
        s.dim[i] = int(seed.x[i].shape[0])
        s.x[i] = _dp(seed.x[i])
        s.f[i] = _dp(seed.f[i])
        keep += [seed.x[i], seed.f[i]]
    s.f0 = seed.f0
    return s


class Marshalled:
    """A Problem laid out as C records.  Holds references to every numpy array
    it points into, so it must outlive the native call."""

    def __init__(self, problem):
        from .problem import Problem  # noqa: F401  (type only)

        p = problem
        self.problem = p
        self._keep = []
        b = p.beam
        self.beam = RtBeam(b.nx, b.ny, b.na, b.nb, b.nv, b.dx, b.dy, b.da, b.db, b.dz,
                           _dp(b.x), _dp(b.y), _dp(b.a), _dp(b.b), _dp(b.dv))
        self._keep += [b.x, b.y, b.a, b.b, b.dv]
        self.N = len(p.gain)
        self.gain = (RtGain * self.N)()
        for i, g in enumerate(p.gain):
            self.gain[i] = RtGain(g.Nx, g.Ny, g.Nv, _dp(g.x), _dp(g.y), _dp(g.n),
                                  _fp(g.g0), _fp(g.E0), _fp(g.gv))
            self._keep += [g.x, g.y, g.n, g.g0, g.E0, g.gv]
        self.seed = None
        if p.seed is not None:
            s = RtSeed()
            for i in range(5):
                s.dim[i] = int(p.seed.x[i].shape[0])
                s.x[i] = _dp(p.seed.x[i])
                s.f[i] = _dp(p.seed.f[i])
                self._keep += [p.seed.x[i], p.seed.f[i]]
            s.f0 = p.seed.f0
            self.seed = s

    @property
    def seed_ref(self):
        return C.byref(self.seed) if self.seed is not None else None


def _is_tensor(a) -> bool:
    return hasattr(a, "data_ptr") and hasattr(a, "is_cuda")   # a torch tensor, without importing torch


class GainValues:
    """The tables of a Plan.update_gain laid out as rt_gain_values[N]; holds a reference to every array it points into.

    `gain`: a Problem, or N entries (entry 0 is ignored and may be None) that are Gain records, dicts with the keys
    n, g0, E0 (optional), gv, or tuples (n, g0, E0, gv); E0 may be None.  `shapes` = [(Nx, Ny)] * N and K are the plan's.
    Either all arrays are numpy arrays (on_device False: rt_hip_plan_update_gain) or all are torch tensors on
    cuda:`device` (on_device True: rt_hip_plan_update_gain_dev).  Everything else is a ValueError, raised here, before any
    native call: wrong N, shapes, dtypes (float64 for n, float32 for the rest), non-contiguous arrays, a tensor on the
    CPU or on another device, host and device arrays mixed."""

    def __init__(self, gain, shapes, K: int, device: int = 0):
        entries = list(gain.gain) if hasattr(gain, "gain") and hasattr(gain, "beam") else list(gain)
        if len(entries) != len(shapes):
            raise ValueError(f"update_gain: {len(entries)} lengths given, the plan has N = {len(shapes)}")
        self.N = len(entries)
        self.vals = (RtGainValues * self.N)()
        self.tables = [None] * self.N      # per length (n, g0, E0, gv) as given
        self._keep = []
        kinds = set()
        for i in range(1, self.N):
            e = entries[i]
            if isinstance(e, dict):
                t = (e["n"], e["g0"], e.get("E0"), e["gv"])
            elif isinstance(e, (tuple, list)):
                if len(e) != 4:
                    raise ValueError(f"update_gain: length {i}: expected (n, g0, E0, gv)")
                t = tuple(e)
            elif e is not None and all(hasattr(e, k) for k in ("n", "g0", "E0", "gv")):
                t = (e.n, e.g0, e.E0, e.gv)
            else:
                raise ValueError(f"update_gain: length {i}: expected a Gain, a dict or a tuple (n, g0, E0, gv)")
            Nx, Ny = shapes[i]
            cells = Nx * Ny
            ptrs = []
            for name, a, dt, ok_shapes in (("n", t[0], "float64", ((cells,), (Ny, Nx))), ("g0", t[1], "float32", ((cells,), (Ny, Nx))),
                                           ("E0", t[2], "float32", ((cells,), (Ny, Nx))),
                                           ("gv", t[3], "float32", ((cells * K,), (cells, K), (Ny, Nx, K)))):
                if a is None:
                    if name != "E0":
                        raise ValueError(f"update_gain: length {i}: {name} is missing (only E0 may be None)")
                    ptrs.append(None)
                    continue
                if _is_tensor(a):
                    if not a.is_cuda:
                        raise ValueError(f"update_gain: length {i}: {name} is a torch tensor on the CPU (pass numpy arrays, or tensors on the plan's device)")
                    if a.device.index != device:
                        raise ValueError(f"update_gain: length {i}: {name} is on {a.device}, the plan on device {device}")
                    kinds.add("device")
                    dtype, shape, contiguous = str(a.dtype).replace("torch.", ""), tuple(a.shape), a.is_contiguous()
                    addr = a.data_ptr()
                elif isinstance(a, np.ndarray):
                    kinds.add("host")
                    dtype, shape, contiguous = str(a.dtype), a.shape, a.flags.c_contiguous
                    addr = a.ctypes.data
                else:
                    raise ValueError(f"update_gain: length {i}: {name} is neither a numpy array nor a torch tensor")
                if dtype != dt:
                    raise ValueError(f"update_gain: length {i}: {name} has dtype {dtype}, expected {dt}")
                if shape not in ok_shapes:
                    raise ValueError(f"update_gain: length {i}: {name} has shape {shape}, the plan's tables have {ok_shapes[-1]}")
                if not contiguous:
                    raise ValueError(f"update_gain: length {i}: {name} is not contiguous")
                self._keep.append(a)
                ptrs.append(addr)
            if len(kinds) > 1:
                raise ValueError("update_gain: host (numpy) and device (torch) arrays mixed in one update")
            self.tables[i] = t
            self.vals[i] = RtGainValues(C.cast(ptrs[0], c_double_p), C.cast(ptrs[1], c_float_p),
                                        C.cast(ptrs[2], c_float_p) if ptrs[2] is not None else c_float_p(),
                                        C.cast(ptrs[3], c_float_p))
        self.on_device = kinds == {"device"}


def rays_ptr(rays: np.ndarray):
    assert rays.dtype == RAY_DTYPE and rays.flags.c_contiguous
    return rays.ctypes.data_as(C.POINTER(RtRay))


def rays_from_array(a: np.ndarray) -> np.ndarray:
    """[n][4] float64 (x, y, a, b) -> rt_ray records, every coordinate rounded as the C cast (float) rounds it
    (what RayTrace::calc_ray does with its arguments and Problem.build_rays with the grids)."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("rays: expected an [n][4] array of (x, y, a, b)")
    out = np.empty(a.shape[0], dtype=RAY_DTYPE)
    for c, name in enumerate(("x", "y", "a", "b")):
        out[name] = a[:, c].astype(np.float32)
    return out


def rays_to_array(rays: np.ndarray) -> np.ndarray:
    """rt_ray records -> [n][4] float64 (x, y, a, b), exactly (every float is a double)."""
    rays = np.asarray(rays, dtype=RAY_DTYPE)
    return np.stack([rays[name].astype(np.float64) for name in ("x", "y", "a", "b")], axis=1) if len(rays) \
        else np.zeros((0, 4))


def declare_hip_api(lib: C.CDLL) -> None:
    """Attach argtypes/restype for every symbol include/rt_hip.h declares."""
    P = C.POINTER
    vp = C.c_void_p
    lib.rt_hip_device_count.argtypes = []
    lib.rt_hip_device_count.restype = C.c_int
    lib.rt_hip_last_error.argtypes = []
    lib.rt_hip_last_error.restype = C.c_char_p
    lib.rt_hip_selftest.argtypes = [C.c_int, P(C.c_ulonglong), P(C.c_ulonglong)]
    lib.rt_hip_selftest.restype = C.c_int
    lib.rt_hip_image_loop.argtypes = [
        C.c_int, C.c_int, P(RtBeam), P(RtGain), P(RtSeed), C.c_int, P(RtRay), C.c_size_t,
        C.c_double, c_double_p, c_double_p, P(C.c_uint), P(RtRay), C.c_int, P(C.c_int),
        P(RtStats)]
    lib.rt_hip_image_loop.restype = C.c_int
    lib.rt_hip_multi_image_loop.argtypes = list(lib.rt_hip_image_loop.argtypes)
    lib.rt_hip_multi_image_loop.restype = C.c_int
    lib.rt_hip_multi_last_mode.argtypes = []
    lib.rt_hip_multi_last_mode.restype = C.c_int
    lib.rt_hip_ray_list_grid_dims.argtypes = [P(RtRay), C.c_size_t, P(C.c_int * 4)]
    lib.rt_hip_ray_list_grid_dims.restype = C.c_int
    lib.rt_hip_host_libm_mode.argtypes = [C.c_int]
    lib.rt_hip_host_libm_mode.restype = C.c_int
    lib.rt_hip_pool_trim.argtypes = []
    lib.rt_hip_pool_trim.restype = None
    lib.rt_hip_plan_create.argtypes = [P(vp), C.c_int, C.c_int, P(RtBeam), P(RtGain), P(RtSeed),
                                       C.c_int, C.c_double]
    lib.rt_hip_plan_create.restype = C.c_int
    lib.rt_hip_plan_set_rays.argtypes = [vp, P(RtRay), C.c_size_t]
    lib.rt_hip_plan_set_rays.restype = C.c_int
    lib.rt_hip_plan_set_ray_grid.argtypes = [vp, c_double_p, C.c_int, c_double_p, C.c_int,
                                             c_double_p, C.c_int, c_double_p, C.c_int,
                                             C.c_int64, C.c_int64, C.c_int64]
    lib.rt_hip_plan_set_ray_grid.restype = C.c_int
    lib.rt_hip_plan_run.argtypes = [vp, vp, vp, vp]
    lib.rt_hip_plan_run.restype = C.c_int
    lib.rt_hip_plan_fetch.argtypes = [vp, c_double_p, c_double_p, P(C.c_uint), P(RtRay), C.c_int,
                                      P(C.c_int), P(RtStats)]
    lib.rt_hip_plan_fetch.restype = C.c_int
    lib.rt_hip_plan_kernel_ms.argtypes = [vp, P(C.c_float)]
    lib.rt_hip_plan_kernel_ms.restype = C.c_int
    lib.rt_hip_plan_kernel_times.argtypes = [vp, P(C.c_float), P(C.c_float)]
    lib.rt_hip_plan_kernel_times.restype = C.c_int
    lib.rt_hip_plan_last_fused.argtypes = [vp]
    lib.rt_hip_plan_last_fused.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_last_march_instance"):   # (a library built from an earlier commit, loaded for an A/B, has none)
        lib.rt_hip_plan_last_march_instance.argtypes = [vp]
        lib.rt_hip_plan_last_march_instance.restype = C.c_int
    lib.rt_hip_plan_set_timing_ring.argtypes = [vp, C.c_int]
    lib.rt_hip_plan_set_timing_ring.restype = C.c_int
    lib.rt_hip_plan_ring_times.argtypes = [vp, c_float_p, c_float_p, C.c_int, P(C.c_int)]
    lib.rt_hip_plan_ring_times.restype = C.c_int
    lib.rt_hip_plan_image_ptr.argtypes = [vp]
    lib.rt_hip_plan_image_ptr.restype = vp
    lib.rt_hip_plan_iang_ptr.argtypes = [vp]
    lib.rt_hip_plan_iang_ptr.restype = vp
    lib.rt_hip_plan_enable_probe.argtypes = [vp, C.c_int]
    lib.rt_hip_plan_enable_probe.restype = C.c_int
    lib.rt_hip_plan_fetch_probe.argtypes = [vp, c_float_p, c_float_p, P(C.c_int32), P(RtRay),
                                            P(C.c_uint32), P(C.c_uint32)]
    lib.rt_hip_plan_fetch_probe.restype = C.c_int
    lib.rt_hip_plan_set_exact_emission.argtypes = [vp, C.c_int]
    lib.rt_hip_plan_set_exact_emission.restype = C.c_int
    lib.rt_hip_plan_set_step_factor.argtypes = [vp, C.c_double]
    lib.rt_hip_plan_set_step_factor.restype = C.c_int
    lib.rt_hip_plan_enable_path.argtypes = [vp, C.c_int]
    lib.rt_hip_plan_enable_path.restype = C.c_int
    lib.rt_hip_plan_fetch_path.argtypes = [vp, c_float_p, P(C.c_int32)]
    lib.rt_hip_plan_fetch_path.restype = C.c_int
    lib.rt_hip_plan_enable_spectra.argtypes = [vp, C.c_int]
    lib.rt_hip_plan_enable_spectra.restype = C.c_int
    lib.rt_hip_plan_fetch_spectra.argtypes = [vp, c_double_p, P(RtRay), P(C.c_int32)]
    lib.rt_hip_plan_fetch_spectra.restype = C.c_int
    lib.rt_hip_plan_spectra_ptr.argtypes = [vp]
    lib.rt_hip_plan_spectra_ptr.restype = vp
    lib.rt_hip_calc_rays.argtypes = [C.c_int, C.c_int, C.c_double, P(RtGain), P(RtSeed), C.c_int, C.c_int, c_double_p,
                                     C.c_size_t, c_double_p, c_double_p, P(C.c_int32), P(RtStats)]
    lib.rt_hip_calc_rays.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_enable_step"):   # (a library built from an earlier commit, loaded for an A/B, has none)
        lib.rt_hip_plan_enable_step.argtypes = [vp, C.c_int]
        lib.rt_hip_plan_enable_step.restype = C.c_int
        lib.rt_hip_plan_fetch_step.argtypes = [vp, c_double_p, c_double_p, c_double_p]
        lib.rt_hip_plan_fetch_step.restype = C.c_int
        lib.rt_hip_plan_step_ptrs.argtypes = [vp, P(vp), P(vp)]
        lib.rt_hip_plan_step_ptrs.restype = C.c_int
        lib.rt_hip_step_loop.argtypes = [
            C.c_int, C.c_int, P(RtBeam), P(RtGain), P(RtSeed), C.c_int, P(RtRay), C.c_size_t,
            C.c_double, c_double_p, c_double_p, c_double_p, P(C.c_uint), P(RtRay), C.c_int, P(C.c_int),
            P(RtStats)]
        lib.rt_hip_step_loop.restype = C.c_int
    if hasattr(lib, "rt_hip_multi_step_loop"):   # (likewise)
        lib.rt_hip_plan_set_step_buffers.argtypes = [vp, vp, vp]
        lib.rt_hip_plan_set_step_buffers.restype = C.c_int
        lib.rt_hip_multi_step_loop.argtypes = list(lib.rt_hip_step_loop.argtypes)
        lib.rt_hip_multi_step_loop.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_update_gain"):   # (likewise)
        lib.rt_hip_plan_update_gain.argtypes = [vp, C.c_int, P(RtGainValues)]
        lib.rt_hip_plan_update_gain.restype = C.c_int
        lib.rt_hip_plan_update_gain_dev.argtypes = [vp, C.c_int, P(RtGainValues), vp]
        lib.rt_hip_plan_update_gain_dev.restype = C.c_int
        lib.rt_hip_plan_table_flags.argtypes = [vp, P(C.c_int), P(C.c_int), P(C.c_int), c_float_p]
        lib.rt_hip_plan_table_flags.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_set_seeds"):   # (likewise)
        lib.rt_hip_plan_set_seeds.argtypes = [vp, C.c_int, P(RtSeed)]
        lib.rt_hip_plan_set_seeds.restype = C.c_int
        lib.rt_hip_plan_fetch_seed_step.argtypes = [vp, C.c_int, c_double_p, c_double_p, c_double_p, P(C.c_uint)]
        lib.rt_hip_plan_fetch_seed_step.restype = C.c_int
        lib.rt_hip_plan_seed_step_ptrs.argtypes = [vp, C.c_int, P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_seed_step_ptrs.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_set_step_one_launch"):   # (likewise)
        lib.rt_hip_plan_set_step_one_launch.argtypes = [vp, C.c_int]
        lib.rt_hip_plan_set_step_one_launch.restype = C.c_int
    if hasattr(lib, "rt_hip_debug_run_shape"):   # (likewise)
        lib.rt_hip_debug_run_shape.argtypes = [P(RtRunFacts), P(RtRunShape)]
        lib.rt_hip_debug_run_shape.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_enable_length_scan"):   # (likewise)
        lib.rt_hip_plan_enable_length_scan.argtypes = [vp, C.c_int]
        lib.rt_hip_plan_enable_length_scan.restype = C.c_int
        lib.rt_hip_plan_fetch_length_step.argtypes = [vp, C.c_int, c_double_p, c_double_p, c_double_p, P(C.c_uint)]
        lib.rt_hip_plan_fetch_length_step.restype = C.c_int
        lib.rt_hip_plan_length_step_ptrs.argtypes = [vp, C.c_int, P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_length_step_ptrs.restype = C.c_int
        lib.rt_hip_length_scan_loop.argtypes = list(lib.rt_hip_step_loop.argtypes)   # (one row per length where step_loop has one array)
        lib.rt_hip_length_scan_loop.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_enable_suffix_scan"):   # (likewise)
        lib.rt_hip_plan_enable_suffix_scan.argtypes = [vp, C.c_int]
        lib.rt_hip_plan_enable_suffix_scan.restype = C.c_int
        lib.rt_hip_suffix_scan_loop.argtypes = list(lib.rt_hip_step_loop.argtypes)   # (row n - 2: the last n lengths)
        lib.rt_hip_suffix_scan_loop.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_set_scan_seeds"):   # (likewise)
        lib.rt_hip_plan_set_scan_seeds.argtypes = [vp, C.c_int, P(RtSeed)]
        lib.rt_hip_plan_set_scan_seeds.restype = C.c_int
        lib.rt_hip_plan_fetch_seed_length_step.argtypes = [vp, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, P(C.c_uint)]
        lib.rt_hip_plan_fetch_seed_length_step.restype = C.c_int
        lib.rt_hip_plan_seed_length_step_ptrs.argtypes = [vp, C.c_int, C.c_int, P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_seed_length_step_ptrs.restype = C.c_int
        a = list(lib.rt_hip_step_loop.argtypes)   # (n_seed, seeds behind scale; one row per seed and length where step_loop has one array)
        lib.rt_hip_seed_length_scan_loop.argtypes = a[:9] + [C.c_int, P(RtSeed)] + a[9:]
        lib.rt_hip_seed_length_scan_loop.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_set_ase_seeds"):   # (likewise)
        lib.rt_hip_plan_set_ase_seeds.argtypes = [vp, C.c_int, P(RtSeed), c_double_p]
        lib.rt_hip_plan_set_ase_seeds.restype = C.c_int
        lib.rt_hip_plan_fetch_full_step.argtypes = [vp, C.c_int, c_double_p, c_double_p, c_double_p, P(C.c_uint)]
        lib.rt_hip_plan_fetch_full_step.restype = C.c_int
        lib.rt_hip_plan_full_step_ptrs.argtypes = [vp, C.c_int, P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_full_step_ptrs.restype = C.c_int
        lib.rt_hip_full_step_loop.argtypes = [   # (no seed; n_seed, seeds, scales behind scale; one row per record)
            C.c_int, C.c_int, P(RtBeam), P(RtGain), C.c_int, P(RtRay), C.c_size_t, C.c_double, C.c_int, P(RtSeed), c_double_p,
            c_double_p, c_double_p, c_double_p, P(C.c_uint), P(RtRay), C.c_int, P(C.c_int), P(RtStats)]
        lib.rt_hip_full_step_loop.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_set_scan_ase_seeds"):   # (likewise)
        lib.rt_hip_plan_set_scan_ase_seeds.argtypes = [vp, C.c_int, P(RtSeed), c_double_p]
        lib.rt_hip_plan_set_scan_ase_seeds.restype = C.c_int
        lib.rt_hip_plan_fetch_full_length_step.argtypes = [vp, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, P(C.c_uint)]
        lib.rt_hip_plan_fetch_full_length_step.restype = C.c_int
        lib.rt_hip_plan_full_length_step_ptrs.argtypes = [vp, C.c_int, C.c_int, P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_full_length_step_ptrs.restype = C.c_int
        lib.rt_hip_full_length_scan_loop.argtypes = list(lib.rt_hip_full_step_loop.argtypes)   # (one row per record and length)
        lib.rt_hip_full_length_scan_loop.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_set_suffix_ase_seeds"):   # (likewise)
        lib.rt_hip_plan_set_suffix_ase_seeds.argtypes = [vp, C.c_int, P(RtSeed), c_double_p]
        lib.rt_hip_plan_set_suffix_ase_seeds.restype = C.c_int
        lib.rt_hip_full_suffix_scan_loop.argtypes = list(lib.rt_hip_full_length_scan_loop.argtypes)   # (row (r, n - 2): the last n lengths)
        lib.rt_hip_full_suffix_scan_loop.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_set_suffix_seeds"):   # (likewise)
        lib.rt_hip_plan_set_suffix_seeds.argtypes = list(lib.rt_hip_plan_set_scan_seeds.argtypes)
        lib.rt_hip_plan_set_suffix_seeds.restype = C.c_int
        lib.rt_hip_seed_suffix_scan_loop.argtypes = list(lib.rt_hip_seed_length_scan_loop.argtypes)   # (row (s, n - 2): the last n lengths)
        lib.rt_hip_seed_suffix_scan_loop.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_enable_length_spectra"):   # (likewise)
        lib.rt_hip_plan_enable_length_spectra.argtypes = [vp, C.c_int]
        lib.rt_hip_plan_enable_length_spectra.restype = C.c_int
        lib.rt_hip_plan_fetch_length_spectra.argtypes = [vp, C.c_int, c_double_p, P(RtRay), P(C.c_int32)]
        lib.rt_hip_plan_fetch_length_spectra.restype = C.c_int
        lib.rt_hip_plan_length_spectra_ptrs.argtypes = [vp, C.c_int, P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_length_spectra_ptrs.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_set_spectra_seeds"):   # (likewise)
        lib.rt_hip_plan_set_spectra_seeds.argtypes = [vp, C.c_int, P(RtSeed)]
        lib.rt_hip_plan_set_spectra_seeds.restype = C.c_int
        lib.rt_hip_plan_fetch_seed_spectra.argtypes = [vp, C.c_int, c_double_p, P(RtRay), P(C.c_int32)]
        lib.rt_hip_plan_fetch_seed_spectra.restype = C.c_int
        lib.rt_hip_plan_seed_spectra_ptrs.argtypes = [vp, C.c_int, P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_seed_spectra_ptrs.restype = C.c_int
        lib.rt_hip_plan_fetch_seed_length_spectra.argtypes = [vp, C.c_int, C.c_int, c_double_p, P(RtRay), P(C.c_int32)]
        lib.rt_hip_plan_fetch_seed_length_spectra.restype = C.c_int
        lib.rt_hip_plan_seed_length_spectra_ptrs.argtypes = [vp, C.c_int, C.c_int, P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_seed_length_spectra_ptrs.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_set_spectra_ase_seeds"):   # (likewise)
        lib.rt_hip_plan_set_spectra_ase_seeds.argtypes = [vp, C.c_int, P(RtSeed)]
        lib.rt_hip_plan_set_spectra_ase_seeds.restype = C.c_int
        lib.rt_hip_plan_fetch_full_spectra.argtypes = [vp, C.c_int, c_double_p, P(RtRay), P(C.c_int32)]
        lib.rt_hip_plan_fetch_full_spectra.restype = C.c_int
        lib.rt_hip_plan_full_spectra_ptrs.argtypes = [vp, C.c_int, P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_full_spectra_ptrs.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_set_length_spectra_ase_seeds"):   # (likewise)
        lib.rt_hip_plan_set_length_spectra_ase_seeds.argtypes = [vp, C.c_int, P(RtSeed)]
        lib.rt_hip_plan_set_length_spectra_ase_seeds.restype = C.c_int
        lib.rt_hip_plan_fetch_full_length_spectra.argtypes = [vp, C.c_int, C.c_int, c_double_p, P(RtRay), P(C.c_int32)]
        lib.rt_hip_plan_fetch_full_length_spectra.restype = C.c_int
        lib.rt_hip_plan_full_length_spectra_ptrs.argtypes = [vp, C.c_int, C.c_int, P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_full_length_spectra_ptrs.restype = C.c_int
    if hasattr(lib, "rt_hip_plan_history_create"):   # (likewise)
        up, bp = P(C.c_uint), P(C.c_ubyte)
        lib.rt_hip_plan_history_create.argtypes = [vp, C.c_int]
        lib.rt_hip_plan_history_create.restype = C.c_int
        lib.rt_hip_plan_history_append.argtypes = [vp, C.c_int, C.c_double, C.c_int, vp]
        lib.rt_hip_plan_history_append.restype = C.c_int
        lib.rt_hip_plan_history_ptrs.argtypes = [vp, C.c_int, P(vp), P(vp), P(vp), P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_history_ptrs.restype = C.c_int
        lib.rt_hip_plan_history_sum_ptrs.argtypes = [vp, C.c_int, P(vp), P(vp), P(vp), P(vp)]
        lib.rt_hip_plan_history_sum_ptrs.restype = C.c_int
        lib.rt_hip_plan_history_fetch.argtypes = [vp, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, up, up, bp]
        lib.rt_hip_plan_history_fetch.restype = C.c_int
        lib.rt_hip_plan_history_fetch_sum.argtypes = [vp, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]
        lib.rt_hip_plan_history_fetch_sum.restype = C.c_int
        lib.rt_hip_plan_history_info.argtypes = [vp, P(C.c_int), P(C.c_int), P(C.c_int)]
        lib.rt_hip_plan_history_info.restype = C.c_int
        lib.rt_hip_debug_history_layout.argtypes = [P(RtHistoryFacts), P(RtHistoryLayout)]
        lib.rt_hip_debug_history_layout.restype = C.c_int
    lib.rt_hip_plan_set_debug.argtypes = [vp, C.c_uint]
    lib.rt_hip_plan_set_debug.restype = C.c_int
    lib.rt_hip_plan_destroy.argtypes = [vp]
    lib.rt_hip_plan_destroy.restype = None


#: every symbol the header declares -- checked by tests/test_cabi_exports.py
HIP_API_SYMBOLS = [
    "rt_hip_device_count", "rt_hip_last_error", "rt_hip_selftest", "rt_hip_image_loop", "rt_hip_multi_image_loop",
    "rt_hip_multi_last_mode", "rt_hip_ray_list_grid_dims", "rt_hip_host_libm_mode", "rt_hip_pool_trim", "rt_hip_plan_create",
    "rt_hip_plan_set_rays", "rt_hip_plan_set_ray_grid", "rt_hip_plan_run", "rt_hip_plan_fetch",
    "rt_hip_plan_kernel_ms", "rt_hip_plan_kernel_times", "rt_hip_plan_last_fused", "rt_hip_plan_last_march_instance", "rt_hip_plan_set_timing_ring", "rt_hip_plan_ring_times", "rt_hip_plan_image_ptr", "rt_hip_plan_iang_ptr", "rt_hip_plan_enable_probe",
    "rt_hip_plan_fetch_probe", "rt_hip_plan_set_exact_emission", "rt_hip_plan_set_step_factor", "rt_hip_plan_enable_path",
    "rt_hip_plan_fetch_path", "rt_hip_plan_enable_spectra", "rt_hip_plan_fetch_spectra", "rt_hip_plan_spectra_ptr",
    "rt_hip_calc_rays", "rt_hip_plan_enable_step", "rt_hip_plan_fetch_step", "rt_hip_plan_step_ptrs", "rt_hip_step_loop",
    "rt_hip_plan_set_step_buffers", "rt_hip_multi_step_loop",
    "rt_hip_plan_update_gain", "rt_hip_plan_update_gain_dev", "rt_hip_plan_table_flags",
    "rt_hip_plan_set_seeds", "rt_hip_plan_fetch_seed_step", "rt_hip_plan_seed_step_ptrs",
    "rt_hip_plan_enable_length_scan", "rt_hip_plan_fetch_length_step", "rt_hip_plan_length_step_ptrs", "rt_hip_length_scan_loop",
    "rt_hip_plan_set_scan_seeds", "rt_hip_plan_fetch_seed_length_step", "rt_hip_plan_seed_length_step_ptrs",
    "rt_hip_seed_length_scan_loop",
    "rt_hip_plan_enable_suffix_scan", "rt_hip_suffix_scan_loop",
    "rt_hip_plan_set_ase_seeds", "rt_hip_plan_fetch_full_step", "rt_hip_plan_full_step_ptrs", "rt_hip_full_step_loop",
    "rt_hip_plan_set_scan_ase_seeds", "rt_hip_plan_fetch_full_length_step", "rt_hip_plan_full_length_step_ptrs",
    "rt_hip_full_length_scan_loop",
    "rt_hip_plan_set_suffix_ase_seeds", "rt_hip_full_suffix_scan_loop",
    "rt_hip_plan_set_suffix_seeds", "rt_hip_seed_suffix_scan_loop",
    "rt_hip_plan_enable_length_spectra", "rt_hip_plan_fetch_length_spectra", "rt_hip_plan_length_spectra_ptrs",
    "rt_hip_plan_set_spectra_seeds", "rt_hip_plan_fetch_seed_spectra", "rt_hip_plan_seed_spectra_ptrs",
    "rt_hip_plan_fetch_seed_length_spectra", "rt_hip_plan_seed_length_spectra_ptrs",
    "rt_hip_plan_set_spectra_ase_seeds", "rt_hip_plan_fetch_full_spectra", "rt_hip_plan_full_spectra_ptrs",
    "rt_hip_plan_set_length_spectra_ase_seeds", "rt_hip_plan_fetch_full_length_spectra", "rt_hip_plan_full_length_spectra_ptrs",
    "rt_hip_plan_set_step_one_launch", "rt_hip_debug_run_shape",
    "rt_hip_plan_history_create", "rt_hip_plan_history_append", "rt_hip_plan_history_ptrs", "rt_hip_plan_history_sum_ptrs",
    "rt_hip_plan_history_fetch", "rt_hip_plan_history_fetch_sum", "rt_hip_plan_history_info", "rt_hip_debug_history_layout",
    "rt_hip_plan_set_debug", "rt_hip_plan_destroy",
]
