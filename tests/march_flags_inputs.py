"""Inputs of tests/test_gpu_march_flags.py: small problems on ASE_small's and seed_small's tables whose rays leave the plasma
box part-way, complete, or escape in their first cell -- the populations in which the lane state of the march (escaped or
not, mirrored y axis or not) decides what a lane does next.

A ray grid of 2 x 2 pixels x 8 x 8 angles: 256 rays, four tiles of the frequency pass.  The tables span x in [0, 69.5 um],
y in [0, 24.5 um] (mirrored: the box is [-24.5, 24.5] um) and two lengths of 0.05 cm: a ray from the middle of the box
leaves it sideways beyond ~35 mrad in x or ~25 mrad in y, so angle grids of +-70 and +-45 mrad send about half of the rays
out part-way.  One pixel column lies 5 nm inside the upper x edge: its rays with a positive x angle leave in their first cell.
The pixel rows lie on both sides of y = 0."""
import copy
import importlib

import numpy as np

rt = importlib.import_module("raytrace-miniapp_amd")

GRID_X = np.array([0.0030, 0.0069450])           # cm; box edge at 0.00695
GRID_Y = np.array([-0.0011, 0.0011])
GRID_A = -70.0 + 20.0 * np.arange(8)             # mrad: -70 .. 70
GRID_B = -45.5 + 13.0 * np.arange(8)             # mrad: -45.5 .. 45.5


def two_sided(p):
    """p with every table mirrored into y < 0 explicitly: a y grid that starts below 0 takes the unmirrored branch
    (Helper.h:449-453), as tests/test_gpu_edges.py builds it"""
    q = copy.copy(p)
    gains = [p.gain[0]]
    for g in p.gain[1:]:
        Nx, Ny, K = g.Nx, g.Ny, g.Nv
        y2 = np.concatenate([-g.y[::-1] - 1e-6, g.y])

        def mir(a, w=1):
            a = a.reshape(Ny, Nx * w)
            return np.concatenate([a[::-1], a], axis=0).reshape(-1)
        gains.append(rt.Gain(g.x, y2, mir(g.n), mir(g.g0), mir(g.E0), mir(g.gv, K), K))
    q.gain = gains
    return q


def flag_problem(p, mirrored, N):
    """p on the ray grid above (its beam for an emission problem, its seed beam for a seeded one: the ray grid of
    create_image), with N - 1 lengths of tables"""
    q = copy.copy(p) if mirrored else two_sided(p)
    q.gain = list(q.gain[:N])
    which = "seed_beam" if p.seed_beam is not None else "beam"
    b = copy.copy(getattr(p, which))
    b.x, b.y, b.a, b.b = GRID_X.copy(), GRID_Y.copy(), GRID_A.copy(), GRID_B.copy()
    b.dx, b.dy, b.da, b.db = GRID_X[1] - GRID_X[0], GRID_Y[1] - GRID_Y[0], 20.0, 13.0
    setattr(q, which, b)
    q.golden_image = q.golden_I_ang = None
    q.label = f"{p.label} / march flags, {'mirrored' if mirrored else 'two-sided'} y, N = {N}"
    return q


def populations(ora, S):
    """(escaped part-way, complete, escaped in the first cell) as boolean masks over the rays of an oracle probe.
    Part-way: escaped with 0 < n_done < S.  The probe has no n_done; a slot that holds anything was entered, so with k
    such slots n_done is k or k + 1 (the slot the ray escaped in may be empty): 1 <= k < S - 1 implies 0 < n_done < S."""
    esc = (ora["flags"] & 1) != 0
    k = ((ora["ivl"] != 0) | (ora["gvl"] != 0) | (ora["evl"] != 0)).sum(axis=1)
    return esc & (k >= 1) & (k < S - 1), ~esc & ((ora["flags"] & 2) == 0), esc & (ora["steps"] <= 1)
