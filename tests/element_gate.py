"""Element-by-element gate of image and I_ang (a plain helper module: `from element_gate import ...`).

Why: image and I_ang span 8 to 13 decades, so a whole-array rel-L2 sees only the bright part -- a ray lost from a dim
pixel, a ray deposited next door or a last frequency that is off pass the 2e-7 gate by three orders of magnitude
(tests/test_element_gate.py shows it).  Here every element is compared on its own.

The bound ("Element gate"): on clean inputs every deposited term is non-negative (lineshape, g0, E0 >= 0;
Iv < 0 is error -2; scale and 2 dv are positive), and a sum of non-negative terms has condition number 1.  So the
relative error of an element is at most the largest relative error of a contributing Iv_r[k], plus reordering noise of
at most (n_e + K) 2^-52 (n_e = rays deposited into the element), plus n_e 2^-1022 absolute for gradual underflow.
That lets the project's existing gates be applied per element:

    DEFAULT_TIER  1e-5   default emission mode: the parity gate of BASELINE.json, what test_gpu_spectra.py applies per ray
    TIGHT_TIER    1e-11  seeded (gain-only) mode and set_exact_emission(True): the whole-array gate of those tests
    reordering    (n_e + K) 2^-52   one device run against another of the same rays (list / grid, slices, parts, modes)

Rule for an element (d = got - ref, ref >= 0 asserted): it passes iff |d| <= tol ref + n_e 2^-1022; where n_e == 0, got
must be exactly 0; non-finite entries must be equal; no element is left out (the helper asserts that it compared `size`
elements).  Inputs that are not non-negative (sign-flipped tables, gain beyond the range of exp) are out of scope and keep
their whole-array gates.

The measured figures of every comparison are printed before the assertion; with ELEMENT_PARITY_FILE set in the
environment they are appended to that file as well (this is how profiles/element_parity.txt was taken).
"""
import os

import numpy as np

DEFAULT_TIER = 1e-5
TIGHT_TIER = 1e-11
EPS = 2.0 ** -52
TINY = 2.0 ** -1022


def note(line):
    print(line)
    path = os.environ.get("ELEMENT_PARITY_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ---------------------------------------------------------------------------------------------- where a ray lands
def deposit_index(g, d, v):
    """getIndex of the reference (RayTraceImageCPU.cpp:11-16; deposit_index of oracle/rt_oracle.c): -1 outside
    [g[0] - d/2, g[n-1] + d/2], else the first grid point not below v - d/2.  The reference's bisection never looks
    at g[0] again once v - d/2 >= g[0], so the one value v - d/2 == g[0] lands in cell 1, not 0 (n >= 2); a NaN fails
    both range tests and every comparison of the bisection, which leaves it in the last cell."""
    g = np.asarray(g, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    n = len(g)
    t = v - 0.5 * d
    idx = np.searchsorted(g, t, side="left").astype(np.int64)
    if n >= 2:
        idx[t == g[0]] = 1
    idx[(v < g[0] - 0.5 * d) | (v > g[n - 1] + 0.5 * d)] = -1
    idx[np.isnan(v)] = n - 1
    return idx


def deposit_cells(p, rays, ray2=None):
    """(ix, iy, ia, ib) of every ray, -1 where it falls off the axis, by the prologue of the reference's deposit
    (RayTraceImageCPU.cpp:39-54, run_loop of oracle/rt_oracle.c): method 1 deposits at the launch ray, otherwise at
    the exit ray with a, b negated and y mirrored into the half plane of a one-sided image (beam.y[0] >= 0)."""
    b = p.beam
    if p.method == 1:
        out = {k: np.asarray(rays[k], dtype=np.float32) for k in "xyab"}
    else:
        assert ray2 is not None, "methods other than 1 deposit at the exit ray"
        out = {k: np.asarray(ray2[k], dtype=np.float32).copy() for k in "xyab"}
        out["a"] = -out["a"]
        out["b"] = -out["b"]
        if b.y[0] >= 0.0:
            out["y"] = np.where(out["y"] < 0, -out["y"], out["y"])
    return (deposit_index(b.x, b.dx, out["x"]), deposit_index(b.y, b.dy, out["y"]),
            deposit_index(b.a, b.da, out["a"]), deposit_index(b.b, b.db, out["b"]))


def _own_cells(g, d):
    v = np.asarray(g, dtype=np.float64).astype(np.float32)
    return np.array_equal(deposit_index(g, d, v), np.arange(len(g)))


def _count(cells, ok, p, n_img, n_ang):
    b = p.beam
    ix, iy, ia, ib = cells
    m = ok & (ix >= 0) & (iy >= 0)
    n_img += np.bincount(ix[m] + iy[m] * b.nx, minlength=b.nx * b.ny)
    m = ok & (ia >= 0) & (ib >= 0)
    n_ang += np.bincount(ia[m] + ib[m] * b.na, minlength=b.na * b.nb)


def contribution_counts(p, rays=None, ray2=None, err=None):
    """(n_e of the image per pixel [ny * nx] -- the same for every k of the pixel --, n_e of I_ang [nb * na]): how many
    rays the reference deposits into each element.  rays=None is the problem's own ray list; for a whole emission-mode
    grid whose points sit in their own cells the answer is the closed form na nb per pixel, nx ny per angle cell."""
    b = p.beam
    if rays is None and p.method == 1 and p.N_start == 0 and p.N_parallel == 1 and err is None and \
            _own_cells(b.x, b.dx) and _own_cells(b.y, b.dy) and _own_cells(b.a, b.da) and _own_cells(b.b, b.db):
        return np.full(b.nx * b.ny, b.na * b.nb, np.int64), np.full(b.na * b.nb, b.nx * b.ny, np.int64)
    if rays is None:
        rays = p.build_rays()
    ok = np.ones(len(rays), bool) if err is None else np.asarray(err) == 0
    n_img, n_ang = np.zeros(b.nx * b.ny, np.int64), np.zeros(b.na * b.nb, np.int64)
    _count(deposit_cells(p, rays, ray2), ok, p, n_img, n_ang)
    return n_img, n_ang


_whole_grid_counts = {}      # id(problem) -> (problem, counts): the session's fixtures are asked for again and again


def counts_from_oracle(oracle, p, rays=None, n_threads=8, chunk=1 << 22):
    """contribution_counts with the exit rays and return codes taken from the oracle's probe where the deposit needs
    them (seeded mode; any list that may hold failing rays), in chunks so that a 10^8-ray grid needs no second list."""
    if rays is None:
        if id(p) not in _whole_grid_counts:
            _whole_grid_counts[id(p)] = (p, _counts_from_oracle(oracle, p, None, n_threads, chunk))
        return _whole_grid_counts[id(p)][1]
    return _counts_from_oracle(oracle, p, rays, n_threads, chunk)


def _counts_from_oracle(oracle, p, rays, n_threads, chunk):
    if rays is None and p.method == 1:
        b = p.beam
        if p.N_start == 0 and p.N_parallel == 1 and all(_own_cells(g, d) for g, d in ((b.x, b.dx), (b.y, b.dy), (b.a, b.da), (b.b, b.db))):
            return contribution_counts(p)
    b = p.beam
    n_img, n_ang = np.zeros(b.nx * b.ny, np.int64), np.zeros(b.na * b.nb, np.int64)
    ids = p.ray_ids() if rays is None else None
    n = len(ids) if rays is None else len(rays)
    for lo in range(0, n, chunk):
        part = p.build_rays(ids[lo:lo + chunk]) if rays is None else np.ascontiguousarray(rays[lo:lo + chunk])
        ray2, err = oracle.exit_rays(p, part, n_threads=n_threads)
        _count(deposit_cells(p, part, ray2), err == 0, p, n_img, n_ang)
    return n_img, n_ang


def numpy_deposit(p, rays, probe):
    """image [ny * nx * K] and I_ang [nb * na] from the per-ray Iv, ray2 and err of oracle.probe, ray after ray in list
    order as RayTraceImageCPULoop deposits them (failing rays deposit nothing)."""
    b = p.beam
    K = b.nv
    ix, iy, ia, ib = deposit_cells(p, rays, probe["ray2"])
    ok = np.asarray(probe["err"]) == 0
    Iv = np.asarray(probe["Iv"], dtype=np.float64)
    image = np.zeros((b.nx * b.ny, K))
    m = ok & (ix >= 0) & (iy >= 0)
    np.add.at(image, ix[m] + iy[m] * b.nx, Iv[m] * p.scale)
    iang = np.zeros(b.na * b.nb)
    m = ok & (ia >= 0) & (ib >= 0)
    np.add.at(iang, ia[m] + ib[m] * b.na, (Iv[m] * (2.0 * b.dv)[None, :]).sum(axis=1))
    return image.reshape(-1), iang


# ---------------------------------------------------------------------------------------------- the gate
def _spread(n_e, size):
    n_e = np.asarray(n_e).reshape(-1)
    assert size % len(n_e) == 0, (size, len(n_e))
    return np.repeat(n_e, size // len(n_e)) if len(n_e) != size else n_e


def reordering_tol(n_e, K):
    """Two sums of the same n_e non-negative rows of K frequencies in different orders: (n_e + K) 2^-52 relative."""
    return (np.asarray(n_e, dtype=np.float64) + K) * EPS


def element_figures(got, ref, n_e):
    """dict(worst = largest |got - ref| / ref over the finite elements (inf if a zero of ref is not a zero of got),
    index = its flat index, n_e = its count, rel_l2 = the whole-array figure, count = elements looked at)."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    n_e = _spread(n_e, ref.size)
    fin = np.isfinite(got) & np.isfinite(ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - ref)
        rel = np.where(d <= n_e * TINY, 0.0, d / np.abs(ref))   # (the underflow allowance is no difference); x / 0 -> inf
    rel = np.where(fin, rel, 0.0)
    i = int(np.argmax(rel)) if rel.size else 0
    nb = np.linalg.norm(ref[fin])
    l2 = float(np.linalg.norm(got[fin] - ref[fin]) / nb) if nb > 0 else float(np.linalg.norm(got[fin]))
    return dict(worst=float(rel[i]) if rel.size else 0.0, index=i, n_e=int(n_e[i]) if rel.size else 0, rel_l2=l2,
                count=int(rel.size))


def _name(i, dims):
    if dims is None:
        return f"[{i}]"
    if len(dims) == 3:                                   # image [iy][ix][k]
        ny, nx, K = dims
        return f"(iy {i // (nx * K)}, ix {(i // K) % nx}, k {i % K})"
    nb, na = dims                                         # I_ang [ib][ia]
    return f"(ia {i % na}, ib {i // na})"


def assert_elements(got, ref, n_e, tol, label, dims=None):
    """The rule of the module's docstring on every element; tol is a number (a tier) or an array (reordering_tol).
    dims = (ny, nx, K) or (nb, na) names a failing element.  Returns element_figures."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    n = _spread(n_e, ref.size)
    tol_e = _spread(tol, ref.size) if np.ndim(tol) else np.full(ref.size, float(tol))
    fig = element_figures(got, ref, n)
    tier = f"{float(np.max(tol_e)) if tol_e.size else 0.0:.3g}"
    note(f"{label}: elements {fig['count']} of {ref.size} (excluded 0), worst per-element rel diff {fig['worst']:.3e} at "
         f"{_name(fig['index'], dims)} with n_e {fig['n_e']}, whole-array rel-L2 {fig['rel_l2']:.3e}, gate {tier}")
    fg, fr = np.isfinite(got), np.isfinite(ref)
    # non-finite entries must be equal (as same_outputs_in_a_failing_run has it)
    bad = (fg != fr) | (np.isnan(got) != np.isnan(ref))
    inf = ~fg & ~fr & ~np.isnan(got) & ~np.isnan(ref)
    bad |= inf & (got != ref)
    fin = fg & fr
    assert not (ref[fin] < 0).any(), f"{label}: the reference holds negative elements -- not an input of this gate"
    with np.errstate(invalid="ignore"):
        bad |= fin & (np.abs(got - ref) > tol_e * ref + n * TINY)
        bad |= (n == 0) & ~((got == 0) & (ref == 0))
    compared = int(fin.sum() + (~fin).sum())
    assert compared == ref.size == fig["count"], (label, compared, ref.size)
    if bad.any():
        idx = np.flatnonzero(bad)
        with np.errstate(invalid="ignore", divide="ignore"):
            sev = np.where(fin[idx] & (ref[idx] > 0), np.abs(got[idx] - ref[idx]) / ref[idx], np.inf)
        i = int(idx[int(np.argmax(sev))])
        raise AssertionError(
            f"{label}: {len(idx)} of {ref.size} elements fail the element gate; worst {_name(i, dims)}: got {got[i]!r}, "
            f"ref {ref[i]!r}, rel diff {abs(got[i] - ref[i]) / ref[i] if ref[i] > 0 else float('inf'):.3e}, "
            f"tol {tol_e[i]:.3e}, n_e {int(n[i])}")
    return fig


def gate_outputs(out, ref, p, counts, tol, label):
    """assert_elements on image and I_ang of two result dicts; counts = (n_img, n_ang) of contribution_counts;
    tol = a tier, or "reordering" for (n_e + K) 2^-52."""
    b = p.beam
    n_img, n_ang = counts
    figs = {}
    for key, n_e, dims in (("image", n_img, (b.ny, b.nx, b.nv)), ("I_ang", n_ang, (b.nb, b.na))):
        t = reordering_tol(n_e, b.nv) if isinstance(tol, str) else tol
        figs[key] = assert_elements(out[key], ref[key], n_e, t, f"{label} / {key}", dims)
    return figs
