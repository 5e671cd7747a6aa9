"""Gain tables for the tests of Plan.update_gain (a plain helper module: `from table_variants import ...`).

A time loop has new n, g0, E0 and gv on the same grids at every step.  `tables_b` derives such a second snapshot "B" from
a problem's tables "A"; the `crafted_*` functions build tables on which one of the four facts rt_hip_plan_create derives
from the tables (tables_bounded, ntest_proven, gv_has_nan, gs_cap) differs from A's; `expected_flags` restates those
facts in numpy (raytrace-miniapp_amd/csrc/rt_plan.hip, "Ranges for the short division sequences of the integrator" and
the lineshape scan behind it), so that the helpers can be checked without a device.  Nothing here touches a device."""
import copy
import dataclasses

import numpy as np


def with_gain(p, gains, label=""):
    """p with other tables on the same grids (gain[0] included: it only decides use_emis)."""
    q = copy.copy(p)
    q.gain = list(gains)
    q.golden_image = q.golden_I_ang = None
    q.label = f"{p.label}{label}"
    return q


def tables_b(p):
    """Snapshot B: g0 x 0.5, E0 x 2, n -> 1 + 1.1 (n - 1), gv x 0.75 on every length -- all still finite and non-negative."""
    def b_of(g):
        return dataclasses.replace(g, n=1.0 + 1.1 * (g.n - 1.0), g0=g.g0 * np.float32(0.5),
                                   E0=None if g.E0 is None else g.E0 * np.float32(2.0), gv=g.gv * np.float32(0.75))
    return with_gain(p, [p.gain[0]] + [b_of(g) for g in p.gain[1:]], " tables B")


def _one_length(p, i, label, **changes):
    gains = list(p.gain)
    gains[i] = dataclasses.replace(p.gain[i], **changes)
    return with_gain(p, gains, label)


def crafted_row_wrap(p, i=1):
    """n[ix, iy] = 1 - 0.001 ix: neighbouring nodes differ by 0.001 (horizontally) or 0 (vertically), while the last node
    of a row and the first of the next differ by 0.001 (Nx - 1) -- a scan that compares across the row wrap sees that."""
    g = p.gain[i]
    assert g.Nx >= 40
    n = np.tile(1.0 - 0.001 * np.arange(g.Nx, dtype=np.float64), g.Ny)
    return _one_length(p, i, " row-wrap n", n=n)


def crafted_unbounded(p, i=1):
    """One node with n = 4.5: outside the range of the short division sequences (n + dn <= 4)."""
    g = p.gain[i]
    n = g.n.copy()
    n[(g.Ny // 2) * g.Nx + g.Nx // 2] = 4.5
    return _one_length(p, i, " one node n = 4.5", n=n)


def crafted_huge_lineshape(p, i=2):
    """One lineshape value of 1e30: gs_cap = 708 / max |gv| follows it."""
    gv = p.gain[i].gv.copy()
    gv[len(gv) // 3] = np.float32(1e30)
    return _one_length(p, i, " one gv = 1e30", gv=gv)


def crafted_no_e0(p, i=2):
    """E0 = None for one length (it packs as zeros); gain[0] keeps its E0, so the mode stays."""
    return _one_length(p, i, " no E0", E0=None)


def crafted_nan_lineshape(p, i=1, value=np.nan):
    """One non-finite lineshape value, in row 0 of one length: the NaN-table case of tests/test_gpu_edges.py."""
    gv = p.gain[i].gv.copy()
    gv[3] = value
    return _one_length(p, i, " one non-finite gv", gv=gv)


def crafted_nan_index(p, i=2):
    """One NaN in n: the integrator would never advance on it -- creation and update both refuse such a table."""
    n = p.gain[i].n.copy()
    n[len(n) // 2] = np.nan
    return _one_length(p, i, " one NaN in n", n=n)


# the smallest double that rounds to an infinite float (the midpoint of FLT_MAX and 2^128: the tie goes to even, which is
# 2^128), and the double below it, which rounds to FLT_MAX
FLOAT_INF_AS_FLOAT = 2.0 ** 128 - 2.0 ** 103
LARGEST_FINITE_AS_FLOAT = float(np.nextafter(FLOAT_INF_AS_FLOAT, 0.0))


def crafted_large_index(p, value, i=2):
    """One node of n set to `value`, a finite double: with FLOAT_INF_AS_FLOAT the march would round it to an infinite float
    (creation and update refuse the table like a NaN), with LARGEST_FINITE_AS_FLOAT to FLT_MAX (accepted, outside every
    verified range)."""
    n = p.gain[i].n.copy()
    n[len(n) // 2] = value
    return _one_length(p, i, f" one index of {value!r}", n=n)


def four_lengths(p):
    """N = 4 from the lengths of a three-length problem; the second is sub-sampled to every second grid column, so that
    Nx Ny differs from length to length and is no multiple of 64."""
    g1, g2 = p.gain[1], p.gain[2]
    K = g2.Nv

    def cols(a, k=1):
        return np.ascontiguousarray(a.reshape(g2.Ny, g2.Nx, k)[:, ::2, :]).reshape(-1)

    sub = dataclasses.replace(g2, x=g2.x[::2].copy(), n=cols(g2.n), g0=cols(g2.g0), E0=None if g2.E0 is None else cols(g2.E0),
                              gv=cols(g2.gv, K))
    q = with_gain(p, [p.gain[0], g1, sub, g2], " N = 4")
    assert len({g.Nx * g.Ny for g in q.gain[1:]}) > 1 and all((g.Nx * g.Ny) % 64 for g in q.gain[1:])
    return q


def neighbour_dn(g):
    """The largest |difference| of n between horizontal and vertical neighbours (never across the row wrap)."""
    n = g.n.reshape(g.Ny, g.Nx)
    dn = 0.0
    if g.Nx > 1:
        dn = max(dn, float(np.abs(np.diff(n, axis=1)).max()))
    if g.Ny > 1:
        dn = max(dn, float(np.abs(np.diff(n, axis=0)).max()))
    return dn


def expected_flags(p):
    """dict(bounded, ntest_proven, gv_nonfinite, gs_cap) as rt_hip_plan_create derives them from the tables of p."""
    bounded = ntest = True
    for g in p.gain[1:]:
        n_lo, n_hi, dn = float(g.n.min()), float(g.n.max()), neighbour_dn(g)
        w_min = min(float(np.diff(g.x).min()), float(np.diff(g.y).min()))
        if not (n_lo - dn >= 0.25 and n_hi + dn <= 4.0 and dn / w_min <= 1e12 and w_min >= 1e-12):
            bounded = False
        fy = max(1.2, 1.0 + 2.0 * g.y[0] / (g.y[1] - g.y[0])) if g.y[0] >= 0.0 else 1.2
        if not (8.0 * 0.1 * (1.2 + fy) * dn <= 0.05 - 1e-5):
            ntest = False
    if not (1e-12 <= p.beam.dz <= 1e6):
        bounded = False
    nonfinite, cap = 0, np.float32(np.finfo(np.float32).max)
    if p.use_emis:
        mags = np.concatenate([np.abs(g.gv) for g in p.gain[1:]])
        nonfinite = int(not np.isfinite(mags).all())
        wmax = np.float32(mags[np.isfinite(mags)].max(initial=0.0))
        if wmax > 0:
            cap = min(np.float32(708.0) / wmax, cap)
    return dict(bounded=int(bounded), ntest_proven=int(bounded and ntest), gv_nonfinite=nonfinite, gs_cap=np.float32(cap))


def as_tables(p, to=None):
    """The tables of p as the list Plan.update_gain takes: per length a tuple (n, g0, E0, gv), entry 0 None; `to` maps
    every array (e.g. to a torch tensor on the device)."""
    to = to or (lambda a: a)
    return [None] + [(to(g.n), to(g.g0), None if g.E0 is None else to(g.E0), to(g.gv)) for g in p.gain[1:]]
