"""Plumbing of the device-math tests (a plain helper module: `from devmath import ...`).

  Ref      tests/devmath_ref.c compiled with the host `cc -O2 -ffp-contract=off`: the restatement of exp_tab, exp_tab_vec,
           ase_step, ase_step_f32 and ase_update (tables handed in), and loops over the host libm's tanf / atanf
  Device   ctypes binding of csrc/librt_hip_devmath.so (rt_devmath.hip): the same functions on a device, and the seed-profile
           interpolation (pchip, seed_factor, seed_tab: tests/test_gpu_seed_profiles.py) and the two wave primitives of the
           step deposit (ev_sum, nf_scan), and the float32 blocks of the march (march_step, march_xsetup, f32, f64_div:
           tests/test_gpu_march_blocks.py; march_cell: tests/test_gpu_march_cell.py).  Load it only
           after the `hip` fixture of conftest.py has brought torch in -- one HIP runtime per process
  the high-precision reference: numpy.longdouble (>= 64 significand bits, asserted) exp / expm1, guarded by a cross-check
           of a 2 000-point subsample against mpmath (or the stdlib decimal module at 40 digits)

Errors are always measured against the high-precision reference, never against the restatement.
Measured figures go through note(): printed, and appended to $DEVMATH_PARITY_FILE when that is set (this is how
profiles/devmath_parity.txt was taken)."""
import ctypes
import math
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
DEVMATH_LIB = ROOT / "raytrace-miniapp_amd" / "csrc" / "librt_hip_devmath.so"
VEC = 4
EXP_TAB = 256
LD = np.longdouble
DBL_MAX = np.finfo(np.float64).max
EPS52 = 2.0 ** -52
EPS53 = 2.0 ** -53


def note(line):
    print(line)
    path = os.environ.get("DEVMATH_PARITY_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _ptr(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


_PD, _PF = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)


# ------------------------------------------------------------------------------------------------ the restatement
class Ref:
    _inst = None

    @classmethod
    def get(cls):
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst

    def __init__(self):
        self._dir = tempfile.TemporaryDirectory(prefix="devmath_ref_")
        so = Path(self._dir.name) / "libdevmath_ref.so"
        subprocess.run(["cc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so),
                        str(ROOT / "tests" / "devmath_ref.c"), "-lm"], check=True)
        L = self.lib = ctypes.CDLL(str(so))
        sz = ctypes.c_size_t
        L.dm_exp_tab.argtypes = L.dm_exp_tab_vec.argtypes = [_PD, _PD, _PD, sz]
        L.dm_ase_step.argtypes = L.dm_ase_step_f32.argtypes = [_PD, _PD, _PF, _PD, _PF, _PD, sz]
        L.dm_ase_update.argtypes = [_PD, _PD, _PF, _PF, _PF, _PD, ctypes.POINTER(ctypes.c_ubyte), sz]
        L.dm_host_tanf.argtypes = L.dm_host_atanf.argtypes = [_PF, _PF, sz]
        for f in (L.dm_exp_tab, L.dm_exp_tab_vec, L.dm_ase_step, L.dm_ase_step_f32, L.dm_ase_update, L.dm_host_tanf,
                  L.dm_host_atanf):
            f.restype = None

    def _exp(self, fn, tab, x):
        tab, x = _f64(tab), _f64(x)
        assert tab.size >= EXP_TAB
        out = np.empty_like(x)
        fn(_ptr(tab, ctypes.c_double), _ptr(x, ctypes.c_double), _ptr(out, ctypes.c_double), x.size)
        return out

    def exp_tab(self, tab, x):
        return self._exp(self.lib.dm_exp_tab, tab, x)

    def exp_tab_vec(self, tab, x):
        return self._exp(self.lib.dm_exp_tab_vec, tab, x)

    def _step(self, fn, tab, Iv, gs, rs, w):
        tab, Iv, gs, rs, w = _f64(tab), _f64(Iv), _f32(gs), _f64(rs), _f32(w)
        assert tab.size >= EXP_TAB and Iv.size == w.size == VEC * gs.size and rs.size == gs.size
        out = np.empty_like(Iv)
        fn(_ptr(tab, ctypes.c_double), _ptr(Iv, ctypes.c_double), _ptr(gs, ctypes.c_float), _ptr(rs, ctypes.c_double),
           _ptr(w, ctypes.c_float), _ptr(out, ctypes.c_double), gs.size)
        return out

    def ase_step(self, tab, Iv, gs, rs, w):
        return self._step(self.lib.dm_ase_step, tab, Iv, gs, rs, w)

    def ase_step_f32(self, tab2, Iv, gs, rs, w):
        return self._step(self.lib.dm_ase_step_f32, tab2, Iv, gs, rs, w)

    def ase_update(self, tab, Iv, gs, es, w):
        tab, Iv, gs, es, w = _f64(tab), _f64(Iv), _f32(gs), _f32(es), _f32(w)
        assert Iv.size == gs.size == es.size == w.size
        out, branch = np.empty_like(Iv), np.empty(Iv.size, np.uint8)
        self.lib.dm_ase_update(_ptr(tab, ctypes.c_double), _ptr(Iv, ctypes.c_double), _ptr(gs, ctypes.c_float),
                               _ptr(es, ctypes.c_float), _ptr(w, ctypes.c_float), _ptr(out, ctypes.c_double),
                               _ptr(branch, ctypes.c_ubyte), Iv.size)
        return out, branch.astype(bool)

    def _libm(self, fn, x):
        x = _f32(x)
        out = np.empty_like(x)
        fn(_ptr(x, ctypes.c_float), _ptr(out, ctypes.c_float), x.size)
        return out

    def host_tanf(self, x):
        return self._libm(self.lib.dm_host_tanf, x)

    def host_atanf(self, x):
        return self._libm(self.lib.dm_host_atanf, x)


# ------------------------------------------------------------------------------------------------ the device library
class DeviceMathError(RuntimeError):
    pass


class Device:
    """librt_hip_devmath.so.  A missing library is an error, not a skip: the default make target builds it."""
    EXP_TAB, EXP_TAB_VEC = 0, 1
    STEP_F64, STEP_F32 = 0, 1
    DEPOSIT_FAST, DEPOSIT_4 = 0, 1
    TAN, ATAN = 0, 1
    # the instances of the integrator step the product launches: (BOUNDED, OPT) of csrc/rt_march.hip
    MARCH_OPT_PRUNE, MARCH_OPT_NO_NTEST, MARCH_OPT_PRUNE_H24 = 1, 2, 4
    STEP_INSTANCES = {"ieee": (0, 0), "bounded": (1, 0), "prune": (1, 1 | 2), "prune_h24": (1, 1 | 2 | 4)}
    INV_NORM, DIV_BY_RECIP, DIV_BY_RECIP_SIGNED, FDIV_NR, FDIV_ONE_NR, FMIN_NAN_DROP = range(6)
    F64_DIV_BY_RECIP, F64_DIV_BY_RECIP_TINY_OK = 0, 1
    _inst = None

    @classmethod
    def get(cls):
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst

    def __init__(self):
        if not DEVMATH_LIB.exists():
            raise DeviceMathError(f"{DEVMATH_LIB} is not built (make -C {DEVMATH_LIB.parent})")
        L = self.lib = ctypes.CDLL(str(DEVMATH_LIB))
        sz, ci = ctypes.c_size_t, ctypes.c_int
        pi = ctypes.POINTER(ci)
        L.rt_devmath_error.restype = ctypes.c_char_p
        L.rt_devmath_error.argtypes = [ci]
        L.rt_devmath_vec.restype = ci
        L.rt_devmath_tables.argtypes = [_PD, ctypes.c_uint]
        L.rt_devmath_exp.argtypes = [ci, _PD, _PD, sz]
        L.rt_devmath_update.argtypes = [_PD, _PF, _PF, _PF, _PD, sz]
        L.rt_devmath_step.argtypes = [ci, _PD, _PF, _PD, _PF, _PD, sz]
        L.rt_devmath_div.argtypes = [_PD, _PD, _PD, sz]
        L.rt_devmath_deposit.argtypes = [ci, pi, ctypes.POINTER(_PD), _PD, _PD, pi, sz]
        L.rt_devmath_tan.argtypes = [ci, _PF, _PF, sz]
        ppd = ctypes.POINTER(_PD)
        L.rt_devmath_pchip.argtypes = [ci, _PD, _PD, _PD, _PD, sz]
        L.rt_devmath_seed_factor.argtypes = [pi, ppd, ppd, ctypes.c_double, _PD, _PD, sz]
        L.rt_devmath_seed_tab.argtypes = [pi, ppd, ppd, ctypes.c_double, pi, ppd, ctypes.c_uint, _PD, ctypes.POINTER(ctypes.c_ubyte)]
        L.rt_devmath_ev_sum.argtypes = [_PD, ctypes.POINTER(ctypes.c_ubyte), ctypes.c_double, ci, _PD]
        L.rt_devmath_nf_scan.argtypes = [pi, _PD, ctypes.c_double, ci, _PD]
        pu8 = ctypes.POINTER(ctypes.c_ubyte)
        L.rt_devmath_march_step.argtypes = [ci, ci, ctypes.c_float, _PF, _PF, pu8, ctypes.POINTER(ctypes.c_uint), sz]
        L.rt_devmath_march_xsetup.argtypes = [_PF, _PD, pu8, _PF, sz]
        L.rt_devmath_f32.argtypes = [ci, _PF, _PF, _PF, _PF, sz]
        L.rt_devmath_f64_div.argtypes = [ci, _PD, _PD, _PD, _PD, sz]
        for f in (L.rt_devmath_tables, L.rt_devmath_exp, L.rt_devmath_update, L.rt_devmath_step, L.rt_devmath_div,
                  L.rt_devmath_deposit, L.rt_devmath_tan, L.rt_devmath_pchip, L.rt_devmath_seed_factor, L.rt_devmath_seed_tab,
                  L.rt_devmath_ev_sum, L.rt_devmath_nf_scan, L.rt_devmath_march_step, L.rt_devmath_march_xsetup, L.rt_devmath_f32,
                  L.rt_devmath_f64_div):
            f.restype = ci
        assert L.rt_devmath_vec() == VEC

    def _check(self, status, what):
        if status != 0:
            raise DeviceMathError(f"{what}: HIP error {status}: {self.lib.rt_devmath_error(status).decode()}")

    def tables(self, n_blocks=1):
        """(first, last): the [2][256] doubles of LDS as the first and the last of n_blocks work-groups hold them."""
        out = np.empty(4 * EXP_TAB, np.float64)
        self._check(self.lib.rt_devmath_tables(_ptr(out, ctypes.c_double), n_blocks), "rt_devmath_tables")
        return out[:2 * EXP_TAB].copy(), out[2 * EXP_TAB:].copy()

    def exp(self, which, x):
        x = _f64(x)
        out = np.empty_like(x)
        self._check(self.lib.rt_devmath_exp(which, _ptr(x, ctypes.c_double), _ptr(out, ctypes.c_double), x.size), "rt_devmath_exp")
        return out

    def update(self, Iv, gs, es, w):
        Iv, gs, es, w = _f64(Iv), _f32(gs), _f32(es), _f32(w)
        assert Iv.size == gs.size == es.size == w.size
        out = np.empty_like(Iv)
        self._check(self.lib.rt_devmath_update(_ptr(Iv, ctypes.c_double), _ptr(gs, ctypes.c_float), _ptr(es, ctypes.c_float),
                                               _ptr(w, ctypes.c_float), _ptr(out, ctypes.c_double), Iv.size), "rt_devmath_update")
        return out

    def step(self, which, Iv, gs, rs, w):
        Iv, gs, rs, w = _f64(Iv), _f32(gs), _f64(rs), _f32(w)
        assert Iv.size == w.size == VEC * gs.size and rs.size == gs.size
        out = np.empty_like(Iv)
        self._check(self.lib.rt_devmath_step(which, _ptr(Iv, ctypes.c_double), _ptr(gs, ctypes.c_float), _ptr(rs, ctypes.c_double),
                                             _ptr(w, ctypes.c_float), _ptr(out, ctypes.c_double), gs.size), "rt_devmath_step")
        return out

    def div(self, a, b):
        a, b = _f64(a), _f64(b)
        assert a.size == b.size
        q = np.empty_like(a)
        self._check(self.lib.rt_devmath_div(_ptr(a, ctypes.c_double), _ptr(b, ctypes.c_double), _ptr(q, ctypes.c_double), a.size),
                    "rt_devmath_div")
        return q

    def deposit(self, which, grids, d, v):
        """grids: four 1-d arrays; d: four spacings; v: [n][4].  Returns idx [n][4]."""
        grids = [_f64(g) for g in grids]
        v = _f64(v)
        assert len(grids) == 4 and v.ndim == 2 and v.shape[1] == 4
        n_grid = (ctypes.c_int * 4)(*[g.size for g in grids])
        gp = (_PD * 4)(*[_ptr(g, ctypes.c_double) for g in grids])
        dd = (ctypes.c_double * 4)(*[float(x) for x in d])
        idx = np.empty(v.shape, np.int32)
        self._check(self.lib.rt_devmath_deposit(which, n_grid, gp, dd, _ptr(v, ctypes.c_double), _ptr(idx, ctypes.c_int),
                                                v.shape[0]), "rt_devmath_deposit")
        return idx

    def tan(self, which, x):
        x = _f32(x)
        out = np.empty_like(x)
        self._check(self.lib.rt_devmath_tan(which, _ptr(x, ctypes.c_float), _ptr(out, ctypes.c_float), x.size), "rt_devmath_tan")
        return out

    def ev_sum(self, Iv, deposits, scale):
        """The E_v wave sum (csrc/rt_step_evsum.inc) on one work-group of four waves: Iv [4][64][Kp] (wave, lane, frequency),
        deposits [4][64] bool -> the work-group's accumulator [Kp] = scale * sum of Iv over the depositing lanes."""
        Iv = _f64(Iv)
        deposits = np.ascontiguousarray(deposits, dtype=np.uint8)
        assert Iv.ndim == 3 and Iv.shape[:2] == (4, 64) and deposits.shape == (4, 64)
        out = np.empty(Iv.shape[2], np.float64)
        self._check(self.lib.rt_devmath_ev_sum(_ptr(Iv, ctypes.c_double), _ptr(deposits, ctypes.c_ubyte), float(scale), Iv.shape[2],
                                               _ptr(out, ctypes.c_double)), "rt_devmath_ev_sum")
        return out

    def nf_scan(self, pix, val, scale, n_pix):
        """The segmented scan of the nf deposit (csrc/rt_wave_runs.inc, rt_wave_runscan.inc) on one work-group of four waves:
        pix [4][64] (wave, lane; -1: the lane deposits nothing), val [4][64] -> nf [n_pix], nf[p] = scale * sum of val over the
        lanes of pixel p."""
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        val = _f64(val)
        assert pix.shape == val.shape == (4, 64)
        nf = np.empty(n_pix, np.float64)
        self._check(self.lib.rt_devmath_nf_scan(_ptr(pix, ctypes.c_int), _ptr(val, ctypes.c_double), float(scale), n_pix,
                                                _ptr(nf, ctypes.c_double)), "rt_devmath_nf_scan")
        return nf

    def march_step(self, instance, state, c=0.5):
        """One integrator step of the march per case (csrc/rt_march_step.inc) in one of STEP_INSTANCES.  state [n][14] float32 =
        n0, gxn, gyn, rx, ry, rz, sx, sy, sz, hsum, w_x, w_y, lim2, dzcap; c the step factor -> (out [n][8] = n, rx, ry, rz, sx, sy,
        sz, hsum; run [n] bool; counters: waves of the launch that took prune(0 .. 3) and the tiny-dividend block, and all
        waves).  The kernel runs whole waves: the last one is padded with copies of the last case."""
        bounded, opt = self.STEP_INSTANCES[instance]
        state = _f32(state)
        assert state.ndim == 2 and state.shape[1] == 14 and state.shape[0] >= 1
        n = state.shape[0]
        out, run, cnt = np.empty((n, 8), np.float32), np.empty(n, np.uint8), np.zeros(6, np.uint32)
        self._check(self.lib.rt_devmath_march_step(bounded, opt, float(c), _ptr(state, ctypes.c_float), _ptr(out, ctypes.c_float),
                                                   _ptr(run, ctypes.c_ubyte), _ptr(cnt, ctypes.c_uint), n), "rt_devmath_march_step")
        return out, run.astype(bool), dict(prune=[int(v) for v in cnt[:4]], tiny=int(cnt[4]), waves=int(cnt[5]))

    def march_xsetup(self, pos, lo, w, rw, nc, mirror):
        """The cross-cell set-up of the march per case (csrc/rt_march_xsetup.inc).  pos [n][2] float32 = px, py; lo [n][2] the
        lower corner of the cell, w [n][2] float32 its widths, rw [n][2] = 1 / (double) w (the interval records of
        rt_plan.hip); nc [n][4] = the corner indices n00, n10, n01, n11; mirror [n] -> [n][3] = n0, gxn, gyn."""
        pos, w = _f32(pos), _f32(w)
        lo, rw, nc = _f64(lo), _f64(rw), _f64(nc)
        mirror = np.ascontiguousarray(mirror, dtype=np.uint8)
        n = pos.shape[0]
        assert n >= 1 and pos.shape == w.shape == lo.shape == rw.shape == (n, 2) and nc.shape == (n, 4) and mirror.shape == (n,)
        fin = np.ascontiguousarray(np.concatenate([pos, w], axis=1))
        din = np.ascontiguousarray(np.stack([lo[:, 0], rw[:, 0], lo[:, 1], rw[:, 1], nc[:, 0], nc[:, 1], nc[:, 2], nc[:, 3]], axis=1))
        out = np.empty((n, 3), np.float32)
        self._check(self.lib.rt_devmath_march_xsetup(_ptr(fin, ctypes.c_float), _ptr(din, ctypes.c_double), _ptr(mirror, ctypes.c_ubyte),
                                                     _ptr(out, ctypes.c_float), n), "rt_devmath_march_xsetup")
        return out

    def march_cell(self, lds_tab, gain, use_emis, pos, ii):
        """The escape test and the cell set-up of the march per case (csrc/rt_march_cell.inc) on the march blob of the tables
        gain = (RtGain * N), packed by the product's own function; lds_tab: the instance that gathers from LDS with the
        product's ds_read_b128 sequence, otherwise from global memory.  pos [n][5] float32 = px, py, sz, z, z_stop; ii [n] int32 ->
        (iout [n][8] int32, fout [n][21] float32, dout [n][8] float64) as dm_march_cell_kernel lays them out
        (tests/march_cell_inputs.py names the columns)."""
        import importlib
        cabi = importlib.import_module("raytrace-miniapp_amd").cabi
        pos, ii = _f32(pos), np.ascontiguousarray(ii, dtype=np.int32)
        n = len(ii)
        assert n >= 1 and pos.shape == (n, 5)
        fn = self.lib.rt_devmath_march_cell
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(cabi.RtGain), ctypes.c_int, _PF, ctypes.POINTER(ctypes.c_int),
                       ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), _PF, _PD]
        io, fo, do = np.full((n, 8), -7, np.int32), np.full((n, 21), np.nan, np.float32), np.full((n, 8), np.nan, np.float64)
        self._check(fn(1 if lds_tab else 0, len(gain), gain, 1 if use_emis else 0, _ptr(pos, ctypes.c_float), _ptr(ii, ctypes.c_int), n,
                       _ptr(io, ctypes.c_int), _ptr(fo, ctypes.c_float), _ptr(do, ctypes.c_double)), "rt_devmath_march_cell")
        return io, fo, do

    def f32(self, which, a, b=None, y=None):
        """A float primitive of csrc/rt_math.h elementwise: INV_NORM inv_norm(a), DIV_BY_RECIP div_by_recip(a, b, y),
        DIV_BY_RECIP_SIGNED, FDIV_NR fdiv_nr(a, b), FDIV_ONE_NR fdiv_one_nr(b), FMIN_NAN_DROP fmin_nan_drop(a, b)."""
        ref = a if a is not None else b
        a, b, y = (_f32(v if v is not None else np.zeros_like(ref)) for v in (a, b, y))
        assert a.ndim == 1 and a.shape == b.shape == y.shape and a.size >= 1
        out = np.empty_like(a)
        self._check(self.lib.rt_devmath_f32(which, _ptr(a, ctypes.c_float), _ptr(b, ctypes.c_float), _ptr(y, ctypes.c_float),
                                            _ptr(out, ctypes.c_float), a.size), "rt_devmath_f32")
        return out

    def f64_div(self, which, a, b, y):
        """The double div_by_recip(a, b, y) of csrc/rt_math.h elementwise: F64_DIV_BY_RECIP the guarded form,
        F64_DIV_BY_RECIP_TINY_OK the form of the cross-cell set-up."""
        a, b, y = _f64(a), _f64(b), _f64(y)
        assert a.ndim == 1 and a.shape == b.shape == y.shape
        out = np.empty_like(a)
        self._check(self.lib.rt_devmath_f64_div(which, _ptr(a, ctypes.c_double), _ptr(b, ctypes.c_double), _ptr(y, ctypes.c_double),
                                                _ptr(out, ctypes.c_double), a.size), "rt_devmath_f64_div")
        return out

    def pchip(self, xs, ys, x):
        """pchip_eval (csrc/rt_math.h) of one axis xs, ys [n >= 2] at x [m]."""
        xs, ys, x = _f64(xs), _f64(ys), _f64(x)
        assert xs.ndim == 1 and xs.size == ys.size >= 2
        y = np.empty_like(x)
        self._check(self.lib.rt_devmath_pchip(xs.size, _ptr(xs, ctypes.c_double), _ptr(ys, ctypes.c_double), _ptr(x, ctypes.c_double),
                                              _ptr(y, ctypes.c_double), x.size), "rt_devmath_pchip")
        return y

    @staticmethod
    def _seed_args(seed):
        xs, fs = [_f64(seed.x[d]) for d in range(4)], [_f64(seed.f[d]) for d in range(4)]
        assert all(a.ndim == 1 and a.size == b.size >= 2 for a, b in zip(xs, fs))
        dim = (ctypes.c_int * 4)(*[a.size for a in xs])
        return dim, (_PD * 4)(*[_ptr(a, ctypes.c_double) for a in xs]), (_PD * 4)(*[_ptr(a, ctypes.c_double) for a in fs]), (xs, fs)

    def seed_factor(self, seed, pts):
        """seed_factor (csrc/rt_math.h) of a Seed (its four spatial axes and f0) at pts [m][4] = (x, y, a, b) -> f [m]."""
        dim, px, pf, keep = self._seed_args(seed)
        pts = _f64(pts)
        assert pts.ndim == 2 and pts.shape[1] == 4
        f = np.empty(pts.shape[0], np.float64)
        self._check(self.lib.rt_devmath_seed_factor(dim, px, pf, float(seed.f0), _ptr(pts, ctypes.c_double), _ptr(f, ctypes.c_double),
                                                    pts.shape[0]), "rt_devmath_seed_factor")
        return f

    def seed_tab(self, seed, grids, n_blocks=0):
        """rt_seed_tab_kernel (csrc/rt_march.hip) on the four ray grids -> (sf, sin), each [n0 + n1 + n2 + n3]: the per-axis
        factor at every grid value rounded to float, and whether it lies inside the profile.  n_blocks = 0: the product's
        launch, one thread per entry; otherwise that many work-groups of 256 (fewer: the kernel's grid-stride loop)."""
        dim, px, pf, keep = self._seed_args(seed)
        grids = [_f64(g) for g in grids]
        assert len(grids) == 4 and all(g.ndim == 1 and g.size >= 1 for g in grids)
        n_grid = (ctypes.c_int * 4)(*[g.size for g in grids])
        gp = (_PD * 4)(*[_ptr(g, ctypes.c_double) for g in grids])
        nn = sum(g.size for g in grids)
        sf, sin = np.empty(nn, np.float64), np.empty(nn, np.uint8)
        self._check(self.lib.rt_devmath_seed_tab(dim, px, pf, float(seed.f0), n_grid, gp, n_blocks, _ptr(sf, ctypes.c_double),
                                                 _ptr(sin, ctypes.c_ubyte)), "rt_devmath_seed_tab")
        return sf, sin


# ------------------------------------------------------------------------------------------------ tables
def _mp():
    try:
        import mpmath
        return mpmath
    except ImportError:
        return None


def exact_strings(fn, xs):
    """fn in {"exp", "expm1", "exp2"} of the doubles xs, as 40-digit decimal strings -- mpmath, else the stdlib decimal."""
    mp = _mp()
    out = []
    if mp is not None:
        with mp.workprec(200):
            for x in xs:
                x = mp.mpf(float(x))
                v = {"exp": mp.exp, "expm1": mp.expm1, "exp2": lambda t: mp.power(2, t)}[fn](x)
                out.append(mp.nstr(v, 40, strip_zeros=False, min_fixed=-10 ** 9, max_fixed=-10 ** 9 + 1))
        return out
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ctx.Emin, ctx.Emax = -10 ** 6, 10 ** 6
        ln2 = decimal.Decimal(2).ln()
        for x in xs:
            x = decimal.Decimal(float(x))
            if fn == "exp2":
                v = (x * ln2).exp()
            elif fn == "exp":
                v = x.exp()
            else:
                v = x.exp() - 1 if abs(x) > decimal.Decimal("1e-5") else sum(x ** k / math.factorial(k) for k in range(1, 12))
            out.append(format(+v, ".40e"))
    return out


def correct_tables():
    """(tab, tab2) with tab[j] the correctly rounded 2^(j/256) (float() of a 40-digit string rounds correctly) and
    tab2[j] = tab[j] with j << 12 taken from its high word."""
    tab = np.array([float(s) for s in exact_strings("exp2", np.arange(EXP_TAB) / 256.0)], dtype=np.float64)
    return tab, second_table(tab)


def second_table(tab):
    bits = np.asarray(tab, dtype=np.float64).view(np.uint64)
    j = np.arange(EXP_TAB, dtype=np.uint64)
    return (bits - (j << np.uint64(12 + 32))).view(np.float64)


# ------------------------------------------------------------------------------------------------ the reference
def require_long_double():
    assert np.finfo(LD).nmant >= 63, "numpy.longdouble has no 64-bit significand here: the reference needs mpmath throughout"


def ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def as_ld(got):
    """A double result as a long double, an overflow to +-inf read as +-2^1024 (the value IEEE rounding had in hand)."""
    g = ld(got)
    big = LD(2.0) ** 1024
    return np.where(np.isinf(g), np.sign(g) * big, g)


def spacing(ref_ld):
    """ulp of the double grid at |ref|: 2^(e - 52) for 2^e <= |ref| < 2^(e + 1), 2^-1074 in the subnormal range, that of
    DBL_MAX beyond it."""
    with np.errstate(over="ignore"):
        a = np.abs(ref_ld)
        r = np.minimum(a, LD(DBL_MAX)).astype(np.float64)
    r = np.where(ld(r) > a, np.nextafter(r, 0.0), r)         # rounded up into the next binade: step back
    _, e = np.frexp(r)                                        # r = m 2^e, 0.5 <= m < 1
    return np.ldexp(LD(1.0), np.where(r == 0.0, -1074, np.maximum(e - 53, -1074)))


def ulp_error(got, ref_ld):
    """|got - ref| in ulps of the double grid at ref; NaN where either is NaN.  A reference of 2^1024 or more stands for
    2^1024, as an overflowed result does: inf is then the exact answer."""
    big = LD(2.0) ** 1024
    with np.errstate(invalid="ignore", over="ignore"):
        ref_c = np.clip(ref_ld, -big, big)
        return (np.abs(as_ld(got) - ref_c) / spacing(ref_ld)).astype(np.float64)


def worst(err, x):
    """(largest finite error, the argument where it occurs) -- NaNs ignored."""
    e = np.where(np.isnan(err), -1.0, err)
    i = int(np.argmax(e))
    return float(e[i]), x[i]


def crosscheck_reference(fn, x, ref_ld, n=2000, seed=5):
    """Guards the reference itself: n of the points against mpmath (or decimal) at 40 digits; the long double value must
    agree to 2^-60 relative (its own rounding is 2^-64).  Returns the largest relative difference."""
    x = np.asarray(x, dtype=np.float64)
    ok = np.flatnonzero(np.isfinite(x) & np.isfinite(ref_ld) & (ref_ld != 0))
    pick = np.random.default_rng(seed).choice(ok, size=min(n, ok.size), replace=False)
    exact = np.array([LD(s) for s in exact_strings(fn, x[pick])], dtype=LD)
    rel = np.abs(ref_ld[pick] - exact) / np.abs(exact)
    # (LD(str) itself rounds a 40-digit string to 64 bits: 2^-64)
    worst_rel = float(np.max(rel)) if rel.size else 0.0
    assert worst_rel < 2.0 ** -60, (fn, worst_rel, x[pick][int(np.argmax(rel))])
    return worst_rel


def exp_ref(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(ld(x))


def expm1_ref(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.expm1(ld(x))


# ------------------------------------------------------------------------------------------------ the gates
# Both tiers call these; the device tier passes table_ulp = 1 for the device library's exp2 (documented to 1 ulp),
# the CPU tier 0 (its tables are correctly rounded).
EXP_TAB_ULP = 2.0            # rt_freq.hip, exp_tab: "<= 2 ulp"
EXP_TAB_VEC_ULP = 2.3        # rt_freq.hip, exp_tab_vec: measured 2.27 (tests/test_devmath_host.py), stated as 2.3
EM1_B_F64 = 1e-10            # rt_freq.hip, ase_step: e^x - 1 "to 1e-10" of S
EM1_B_F32 = 3e-10            # rt_freq.hip, ase_step_f32: "to 3e-10 of S"
TINY_REL_F32 = 2.0 ** -23    # the float rounding of rq
TINY_REL_F64 = 1.04e-10      # (ln2/512)^3 / 24 = 1.03e-10, the first term the quadratic leaves out; measured 1.04e-10
TINY_MAX = 1e-2              # "tiny" arguments: |x| <= 1e-2
UNDERFLOW = 2.0 ** -1073     # four roundings into the subnormal range, 2^-1075 each (the stated bounds are relative)


def gate_exp(name, got, x, bound_ulp, table_ulp=0.0):
    """An exponential against exp in long double, in ulp, on every argument; the documented edge behaviour exactly.
    Returns the worst figure."""
    x = np.asarray(x, dtype=np.float64)
    err = ulp_error(got, exp_ref(x))
    nan = np.isnan(x)
    w, at = worst(np.where(nan, 0.0, err), x)
    note(f"{name}: {x.size} arguments, worst {w:.3f} ulp at x = {at!r} ({float(at).hex()}), bound {bound_ulp + table_ulp:g} ulp")
    assert not np.isnan(err[~nan]).any(), f"{name}: NaN for a number"
    assert w <= bound_ulp + table_ulp, f"{name}: {w:.3f} ulp at x = {at!r}"
    got = np.asarray(got)
    for v, want in ((709.79, np.inf), (1100.0, np.inf), (1e308, np.inf), (np.inf, np.inf), (-745.14, 0.0), (-1100.0, 0.0),
                    (-1e308, 0.0), (-np.inf, 0.0), (0.0, 1.0)):
        assert (got[x == v] == want).all() and (x == v).any(), f"{name}: exp({v}) = {got[x == v][:1]}, expected {want}"
    assert (got[x == -745.13] == 2.0 ** -1074).all(), f"{name}: gradual underflow lost at -745.13"
    sub = got[x == -708.4]
    assert ((sub > 0) & (sub < 2.0 ** -1022)).all(), f"{name}: gradual underflow lost at -708.4"
    return w


def em1_bound(x, B, table_ulp=0.0):
    """|err| <= B e^x + 2^-52 max(1, e^x) (+ table_ulp 2^-52 e^x on a device), as a long double array."""
    ex = exp_ref(x)
    return LD(B) * ex + LD(EPS52) * np.maximum(LD(1.0), ex) + LD(table_ulp * EPS52) * ex


def gate_em1(name, got, x, B, tiny_rel, table_ulp=0.0):
    """e^x - 1 of a step form (the step's result for Iv = 0, rs = 1) against expm1 in long double."""
    x = np.asarray(x, dtype=np.float64)
    ref = expm1_ref(x)
    err = np.abs(ld(got) - ref)
    bound = em1_bound(x, B, table_ulp)
    ratio = (err / bound).astype(np.float64)
    w, at = worst(ratio, x)
    rel_S = (err / np.maximum(LD(1.0), exp_ref(x))).astype(np.float64)
    ws, ats = worst(rel_S, x)
    note(f"{name}: {x.size} arguments, worst |err| / max(1, e^x) = {ws:.3e} at x = {ats!r}; worst |err| / bound = {w:.3f} at x = {at!r} "
         f"(bound {B:g} e^x + 2^-52 max(1, e^x){' + 2^-52 e^x' if table_ulp else ''})")
    assert not np.isnan(ratio).any(), name
    assert w <= 1.0, f"{name}: |err| = {float(err[x == at][0]):.3e} at x = {at!r}, bound {float(bound[x == at][0]):.3e}"
    tiny = (np.abs(x) <= TINY_MAX) & (x != 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = (err[tiny] / np.abs(ref[tiny])).astype(np.float64)
    wt, att = worst(rel, x[tiny])
    # a device's table entry for j != 0 may be 1 ulp off: 2^-52 S against e^x - 1 >= ln2/512 where j != 0
    tiny_bound = tiny_rel + table_ulp * EPS52 / (math.log(2.0) / 512.0)
    note(f"{name}: {int(tiny.sum())} tiny arguments (|x| <= {TINY_MAX:g}), worst |err| / |e^x - 1| = {wt:.4e} at x = {att!r}, "
         f"bound {tiny_bound:.4e}")
    assert wt <= tiny_bound, f"{name}: tiny x = {att!r}: relative error {wt:.4e}"
    zero = np.asarray(got)[x == 0]
    assert (zero == 0).all(), f"{name}: e^0 - 1 != 0"
    return ws, wt


def gate_step_general(name, got, Iv, gs, rs, w, B, table_ulp=0.0):
    """A step form with general (Iv, rs): |err| <= delta |Iv + rs| + 2^-53 (|em1 (Iv + rs)| + |Iv'|) (+ underflow), delta
    the e^x - 1 bound; the reference is Iv + expm1(x) (Iv + rs) in long double with x = (double)(gs * w), the float
    product.  A reference beyond the double range must come out as the infinity of its sign."""
    gsv = np.repeat(np.asarray(gs, dtype=np.float32), VEC)
    rsv = ld(np.repeat(np.asarray(rs, dtype=np.float64), VEC))
    x = (gsv * np.asarray(w, dtype=np.float32)).astype(np.float64)
    Ivl = ld(Iv)
    em1 = expm1_ref(x)
    ref = Ivl + em1 * (Ivl + rsv)
    bound = em1_bound(x, B, table_ulp) * np.abs(Ivl + rsv) + LD(EPS53) * (np.abs(em1 * (Ivl + rsv)) + np.abs(ref)) + LD(UNDERFLOW)
    got = np.asarray(got, dtype=np.float64)
    over = np.abs(ref) > LD(DBL_MAX) * (1 + LD(2.0) ** -40)
    edge = ~over & (np.abs(ref) > LD(DBL_MAX) * (1 - LD(2.0) ** -40))
    assert (got[over] == np.sign(ref[over]).astype(np.float64) * np.inf).all(), f"{name}: overflow must give the signed infinity"
    m = ~over & ~edge
    ratio = (np.abs(ld(got[m]) - ref[m]) / bound[m]).astype(np.float64)
    wr, i = worst(ratio, np.flatnonzero(m))
    note(f"{name}: {int(m.sum())} finite cases (+ {int(over.sum())} overflows), worst |err| / bound = {wr:.3f} at Iv = {Iv[i]!r}, "
         f"gs = {gsv[i]!r}, rs = {float(rsv[i])!r}, w = {np.asarray(w)[i]!r}")
    assert not np.isnan(ratio).any(), name
    assert wr <= 1.0, f"{name}: case {i}: got {got[i]!r}, reference {float(ref[i])!r}"
    return wr


def update_reference(Iv, gs, es, w):
    """(ref, bound terms) of ase_update: the CPU formula (Helper.h:549-557 as oracle/rt_oracle.c restates it) in long double
    on the float-rounded gl = gs * w, el = es * w.  Returns (ref, small, other, bound, peak) -- `other` is what the branch the
    CPU does NOT take would give, `bound` the per-branch bound (+ underflow), `peak` the largest intermediate."""
    gl = ld((np.asarray(gs, dtype=np.float32) * np.asarray(w, dtype=np.float32)).astype(np.float64))
    el = ld((np.asarray(es, dtype=np.float32) * np.asarray(w, dtype=np.float32)).astype(np.float64))
    Ivl = ld(Iv)
    small = (np.abs(gl) < LD(1e-3))            # (1e-3 the double literal; gl is a widened float: exact in long double)
    P1 = 1 + LD(0.5) * gl * (1 + LD(0.3333333333) * gl)
    P2 = 1 + gl * (1 + LD(0.5) * gl)
    cubic = el * P1 + Ivl * P2
    with np.errstate(all="ignore"):
        eg, em1 = np.exp(gl), np.expm1(gl)
        ratio = np.where(gl != 0, el / np.where(gl != 0, gl, 1), 0)
        expo = ratio * em1 + Ivl * eg
        b_small = 8 * LD(EPS53) * (np.abs(el * P1) + np.abs(Ivl * P2))
        b_exp = 3 * spacing(eg) * (np.abs(ratio) + np.abs(Ivl)) + 4 * LD(EPS53) * (np.abs(ratio * em1) + np.abs(Ivl * eg))
        peak = np.where(small, np.abs(cubic), np.maximum(np.maximum(eg, np.abs(expo)), np.maximum(np.abs(ratio * em1), np.abs(Ivl * eg))))
    ref = np.where(small, cubic, expo)
    other = np.where(small, expo, cubic)
    return ref, small, other, np.where(small, b_small, b_exp) + LD(UNDERFLOW), peak


def gate_update(name, got, Iv, gs, es, w, near):
    """ase_update against the CPU formula: the per-branch bounds, overflow to the signed infinity, and -- on the floats
    around |gl| = 1e-3 (`near`) -- the CPU's branch: there the two branches differ by gl^3/24 (4e-11 of el, 2e-10 of Iv gl),
    five orders above the bound, so a result inside the bound of the CPU's branch was computed by that branch."""
    ref, small, other, bound, peak = update_reference(Iv, gs, es, w)
    got = np.asarray(got, dtype=np.float64)
    # Beyond the double range the CPU formula itself has no finite value: an intermediate (e^gl, a product, the sum) that
    # exceeds DBL_MAX is an infinity in double arithmetic, and what follows is +-inf or (0 inf, inf - inf) NaN.  `peak` is
    # the largest of them in long double; within 2^-40 of DBL_MAX either outcome is right.
    over = ~(peak <= LD(DBL_MAX) * (1 + LD(2.0) ** -40))
    edge = ~over & (peak > LD(DBL_MAX) * (1 - LD(2.0) ** -40))
    assert not np.isfinite(got[over]).any(), f"{name}: a finite result where the CPU formula overflows"
    inf = over & np.isinf(got) & np.isfinite(ref)
    assert (np.sign(got[inf]) == np.sign(ref[inf]).astype(np.float64)).all(), f"{name}: an infinity of the wrong sign"
    m = ~over & ~edge
    ratio = (np.abs(ld(got[m]) - ref[m]) / bound[m]).astype(np.float64)
    idx = np.flatnonzero(m)
    out = {}
    for label, sel in (("small branch", small[m]), ("exponential branch", ~small[m])):
        wr, i = worst(np.where(sel, ratio, -1.0), idx)
        note(f"{name}, {label}: {int(sel.sum())} cases, worst |err| / bound = {wr:.3f} at Iv = {Iv[i]!r}, gs = {gs[i]!r}, "
             f"es = {es[i]!r}, w = {w[i]!r}")
        out[label] = wr
    assert not np.isnan(ratio).any(), name
    assert max(out.values()) <= 1.0, (name, out)
    # the branch: around 1e-3 the other branch's value lies outside the bound (so the bound tells the branches apart)
    nm = near[m]
    apart = (np.abs(other[m][nm] - ref[m][nm]) / bound[m][nm]).astype(np.float64)
    note(f"{name}: {int(nm.sum())} cases within 300 float ulp of |gl| = 1e-3 ({int((small[m] & nm).sum())} below, "
         f"{int((~small[m] & nm).sum())} at or above): the other branch lies {apart.min():.0f} .. {apart.max():.0f} bounds away")
    assert nm.sum() > 0 and (small[m] & nm).any() and (~small[m] & nm).any()
    assert apart.min() > 4.0, f"{name}: the bound does not tell the two branches apart ({apart.min():.2f})"
    return out
