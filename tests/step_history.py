"""Inputs and the host restatement of the step-history tests (a plain helper module: `from step_history import ...`).
Nothing here touches a device; tests/test_step_history_host.py checks the restatement and the layout on the CPU,
tests/test_gpu_step_history.py runs the inputs.

The restatement is a plain numpy transcription of what the application does with a step's records on the host:
    file_step(history, i, records, codes, weight=None)
        intensity_struct::copy_step (src/RayTraceStructures.cpp:1835-1867): E_v, image (nf) and E_ang (I_ang) of every record
        into slab i, E_sum[i] = sum_j image[j] in the reference's sequential order (np.cumsum(...)[-1]);
        intensity_step_struct::valid() (:1647-1682) split into its two facts: flags bit 0 = some value < 0, bit 1 = some NaN;
        intensity_step_struct::add (:1579-1602) when a weight is given: acc = acc + weight * x, element by element, and
        E_sum_acc likewise from E_sum[i].
    new_history(n_steps, n_rec, nv, npix, nab)   the zeroed arrays file_step writes into
    gamma(m)        m u / (1 - m u), u = 2^-53: |sum in any order - exact sum| <= gamma(n - 1) * exact sum for n non-negative
                    doubles (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2)

Inputs of the GPU tier (WEIGHTS, N_STEPS and `cases`): see tests/test_gpu_step_history.py."""
import ctypes
import importlib
import math

import numpy as np

rt = importlib.import_module("raytrace-miniapp_amd")
cabi = rt.cabi

U = 2.0 ** -53
WEIGHTS = [1.0, 0.5, 3.0, 1e-3]
KEYS = ("E_v", "nf", "I_ang")


def gamma(m):
    return m * U / (1.0 - m * U)


def new_history(n_steps, n_rec, nv, npix, nab):
    def rec():
        return dict(E_v=np.zeros((n_steps, nv)), nf=np.zeros((n_steps, npix)), I_ang=np.zeros((n_steps, nab)), E_sum=np.zeros(n_steps),
                    failure_code=np.zeros(n_steps, np.uint32), flags=np.zeros(n_steps, np.uint32),
                    acc=dict(E_v=np.zeros(nv), nf=np.zeros(npix), I_ang=np.zeros(nab), E_sum=0.0))
    return dict(records=[rec() for _ in range(n_rec)], filled=np.zeros(n_steps, np.uint8))


def flags_of(rec):
    f = 0
    for k in KEYS:
        x = np.asarray(rec[k], dtype=np.float64)
        f |= (1 if (x < 0).any() else 0) | (2 if np.isnan(x).any() else 0)
    return f


def file_step(history, i, records, codes, weight=None):
    """File `records` (one dict(E_v, nf, I_ang) per block) with their failure `codes` as step i; weight: add to the running sum."""
    assert len(records) == len(history["records"]) == len(codes)
    for h, rec, code in zip(history["records"], records, codes):
        for k in KEYS:
            h[k][i] = np.asarray(rec[k], dtype=np.float64).ravel()
        h["E_sum"][i] = np.cumsum(h["nf"][i])[-1]
        h["flags"][i] = flags_of(rec)
        h["failure_code"][i] = code
        if weight is not None:
            w = np.float64(weight)
            for k in KEYS:
                h["acc"][k] = h["acc"][k] + w * h[k][i]
            h["acc"]["E_sum"] = float(np.float64(h["acc"]["E_sum"]) + w * h["E_sum"][i])
    history["filled"][i] = 1
    return history


def layout(hl, nv, nx, ny, na, nb, n_rec, n_steps, accumulate=1):
    """rt_hip_debug_history_layout as a dict; needs the library, no device."""
    f, out = cabi.RtHistoryFacts(), cabi.RtHistoryLayout()
    f.size, out.size = ctypes.sizeof(f), ctypes.sizeof(out)
    f.nv, f.nx, f.ny, f.na, f.nb, f.n_rec, f.n_steps, f.accumulate = nv, nx, ny, na, nb, n_rec, n_steps, accumulate
    hl.check(hl.lib.rt_hip_debug_history_layout(ctypes.byref(f), ctypes.byref(out)), "rt_hip_debug_history_layout")
    return {k: getattr(out, k) for k, _ in cabi.RtHistoryLayout._fields_}


def esum_ratio(e_sum, nf):
    """(|E_sum - fsum(nf)| / fsum(nf), the bound gamma(n - 1)) for one slab of non-negative values."""
    exact = math.fsum(float(x) for x in nf)
    return (abs(float(e_sum) - exact) / exact if exact > 0 else abs(float(e_sum))), gamma(len(nf) - 1)
