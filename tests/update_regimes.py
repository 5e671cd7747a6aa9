"""Inputs that reach every arithmetic of the emission update, and the tile mixes that make the lanes of a tile disagree
(a plain helper module: `from update_regimes import ...`).  Nothing here touches a device:
tests/test_update_regimes_host.py asserts the census of every input on the CPU oracle, tests/test_gpu_update_regimes.py
runs them.

The frequency pass picks the arithmetic of a sub-segment from its float gain sum gs alone
(raytrace-miniapp_amd/csrc/rt_tile_rec.inc, rt_tile_batch.inc and the per-slot copies of the four scan kernels):

    small      RT_RS_MIN <= |gs| <= gs_cap (80 / 708)      ase_step_f32, when every slot of every lane of the tile is small
    regular    RT_RS_MIN <= |gs| <= gs_cap                  ase_step
    irregular  anything else but gs = es = 0                ase_update, e read again from the record
    identity   gs = es = 0

with gs_cap = 708 / max |gv|.  On every shipped table max |gv| = 1 and |gs| < 1.3: every tile of every other test is
all-small.  The lever here is ONE finite lineshape value w* in a row of the length-1 table that no ray of the test reads
(oracle.probe()["ivl"] lists the rows that are read; row 0 is what lanes without a live ray read): it moves gs_cap to
fl(708 / w*) and changes nothing the CPU computes.

Regimes (every one at N = 3, the tile-wide choice, and N = 5, the per-slot choice, under both methods):
    cap_split    w* = 1416: gs_cap = 0.5, about a quarter of the rays all-small, half regular, a quarter irregular
    cap_exact    three spikes whose gs_cap is the |gs| of one chosen slot, one ulp above it and one ulp below it
    tiny         g0 2^-97 (exact): half the slots below RT_RS_MIN = 1e-30
    zero_bands   g0 = +0 in one band of columns, -0 in another: gs == 0 with es != 0 (the sums start from +0, so every
                 such gs is +0: the census says so)
    zero_all     g0 = 0 everywhere: every lit slot is irregular
    absorbing    g0 negated in a band, under the spike: negative sums and sums that cancel, in every class
    big          g0 2^10: |gs| beyond 708, Iv overflows, rays fail with -3
    nan_g0       g0 = NaN in one cell that rays read
    nan_e0       E0 = NaN in one cell whose sub-segments are regular.  The CPU's cell set-up clamps E0 with
                 `E0 >= 0 ? E0 : 0` (oracle/rt_oracle.c, cell_setup), which sends a NaN to 0: no emission sum is ever NaN,
                 the outputs stay finite, and what the regime pins is that the device's set-up clamps alike
    seeded_need  (gain only) seed_small with g0 boosted so that the per-frequency gl falls below 700, into (700, 709.78],
                 beyond it and on NaN, beside rays whose seed factor is 0

The population of a regime is every 97th ray of the grid (4 114 rays) and 600 random rays that reach beyond the tables
(the escaped rays: n_done < S).  `classify` restates the per-slot rule in float32 on the oracle's march sums and sorts the
rays into small, regular, irregular and holed (regular but for a gs = 0 slot, which steers the tile like an irregular
one); `tile_branches` restates the tile-wide decision of rt_tile_rec.inc, `idle && big` included, on the sums of 64
consecutive rays -- the march records of the device are bit-equal to the oracle's (tests/test_gpu_parity.py, same_record),
so it is the device's decision; `compose` builds a ray LIST whose tiles (64 consecutive rays of the launch) hold stated
lane mixes, and the census asserts the branch every tile takes."""
import copy
import dataclasses
import importlib

import numpy as np

import method_pairs as mp
import table_variants as tv

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")

F = np.float32
RS_MIN = F(1e-30)                    # RT_RS_MIN, rt_device.h
W_SPLIT = F(1416.0)                  # gs_cap = 0.5
IDENTITY, SMALL, REGULAR, IRREGULAR, HOLED = 0, 1, 2, 3, 4
NAMES = {IDENTITY: "identity", SMALL: "small", REGULAR: "regular", IRREGULAR: "irregular", HOLED: "holed"}
TILE = 64
RAGGED = 17
STRIDE = 97

FINITE = ("cap_split", "cap_exact", "tiny", "zero_bands", "zero_all", "absorbing")
NONFINITE = ("big", "nan_g0", "nan_e0")
REGIMES = FINITE + NONFINITE
# the ray classes a regime must hold 64 rays of (the non-finite tables: only non-empty)
REACH = dict(cap_split=(SMALL, REGULAR, IRREGULAR), cap_exact=(SMALL, REGULAR, IRREGULAR), tiny=(SMALL, IRREGULAR),
             zero_bands=(SMALL, IRREGULAR), zero_all=(IRREGULAR,), absorbing=(SMALL, REGULAR, IRREGULAR),
             big=(SMALL, REGULAR, IRREGULAR), nan_g0=(SMALL, IRREGULAR), nan_e0=(SMALL,))


# ---------------------------------------------------------------------------------------------- problems and populations
_base = {}


def base(ase_small, N, method):
    """ASE_small (N = 3), or its tables repeated to N lengths as test_other_numbers_of_lengths repeats them, with `method`."""
    if (N, method) not in _base:
        p = ase_small
        if N != 3:
            p = copy.copy(ase_small)
            g = ase_small.gain
            p.gain = [g[0]] + [g[1 + (i % 2)] for i in range(N - 1)]
            p.golden_image = p.golden_I_ang = None
            p.label = f"{ase_small.label} / {N} lengths"
        _base[(N, method)] = mp.with_method(p, method)
    return _base[(N, method)]


def population(p):
    """Every 97th ray of the grid, then 600 random rays of which many leave the tables (tests/test_gpu_spectra.py,
    test_escaped_rays)."""
    rays = p.build_rays(np.arange(0, p.n_rays_total, STRIDE, dtype=np.int64))
    rng = np.random.default_rng(4242)
    gx, gy = p.gain[1].x, p.gain[1].y
    n = 600
    more = np.zeros(n, rt.cabi.RAY_DTYPE)
    more["x"] = rng.uniform(gx[0] - 0.1 * (gx[-1] - gx[0]), gx[-1] + 0.1 * (gx[-1] - gx[0]), n)
    more["y"] = rng.uniform(-1.1 * gy[-1], 1.1 * gy[-1], n)
    more["a"] = rng.uniform(-60, 60, n)
    more["b"] = rng.uniform(-60, 60, n)
    return np.concatenate([rays, more])


def gs_cap(p):
    return F(tv.expected_flags(p)["gs_cap"])


def classify(probe, cap):
    """(slot classes [n][S], ray classes [n]) of the rule above from the oracle's march sums.  A ray is IRREGULAR if any
    slot is, else REGULAR if any slot is beyond the float32 bound, else SMALL; IDENTITY if every slot is the identity
    (a dark or invalid ray).  Slots a ray never wrote (it escaped) are zeros in the probe, as on the device.
    A ray that would be REGULAR but holds a slot with gs = 0 is HOLED: rt_tile_rec.inc sends the tile of such a lane
    (`idle && big`) to the per-slot branch like an irregular one, because the straight-line block would run the identity
    slot as an update (0 * inf once Iv has overflowed).  REGULAR rays hold no such slot."""
    g, e = np.abs(probe["gvl"].astype(F)), probe["evl"].astype(F)
    cap = F(cap)
    with np.errstate(invalid="ignore"):
        regular = (g >= RS_MIN) & (g <= cap)                    # NaN fails both
        small = g <= F(cap * (F(80.0) / F(708.0)))
        lit = (probe["gvl"] != 0) | (e != 0)                    # NaN != 0
    slot = np.where(regular, np.where(small, SMALL, REGULAR), np.where(lit, IRREGULAR, IDENTITY)).astype(np.int8)
    ray = slot.max(axis=1)
    # a tile is small only when no slot of it is beyond the bound: a slot with gs = 0 and es != 0 is irregular already
    ray = np.where((ray == REGULAR) & (probe["gvl"] == 0).any(axis=1), HOLED, ray)
    return slot, ray.astype(np.int8)


def tile_branches(probe, cap):
    """The branch of rt_tile_batch.inc that each tile of 64 consecutive rays of the probe takes for SF = 6 in the default
    mode -- "small" (ase_step_f32 straight through), "regular" (ase_step straight through) or "mixed" (per slot) --,
    restated from rt_tile_rec.inc on the sums themselves, not through classify: per lane irregular, big and idle, then
    all_regular = no lane with irregular || (idle && big), all_small = all_regular && no big lane."""
    gv, e = probe["gvl"].astype(F), probe["evl"].astype(F)
    g, cap = np.abs(gv), F(cap)
    with np.errstate(invalid="ignore"):
        regular = (g >= RS_MIN) & (g <= cap)
        irregular = (~regular & ((gv != 0) | (e != 0))).any(axis=1)
        big = (~(g <= F(cap * (F(80.0) / F(708.0))))).any(axis=1)
        idle = (gv == 0).any(axis=1)
    mixes = irregular | (idle & big)
    out = []
    for lo in range(0, len(g), TILE):
        out.append("mixed" if mixes[lo:lo + TILE].any() else "regular" if big[lo:lo + TILE].any() else "small")
    return out


def stated_branch(lanes):
    """The branch a tile with these lane classes is composed to take."""
    return "mixed" if (IRREGULAR in lanes or HOLED in lanes) else "regular" if REGULAR in lanes else "small"


def free_row(p, probe, length=1):
    """A lineshape row of table `length` that no ray of the probe reads as the last cell of a sub-segment, not row 0: the
    free row nearest the middle of the table."""
    S3 = rt.cabi.RT_N_SUB
    used = np.zeros(p.gain[length].g0.size, bool)
    for L in range(1, p.N):
        if p.gain[L] is p.gain[length]:
            used[np.unique(probe["ivl"][:, (L - 1) * S3:L * S3])] = True
    free = np.flatnonzero(~used)
    free = free[free != 0]
    assert len(free), "no free lineshape row"
    return int(free[np.argmin(np.abs(free - used.size // 2))])


def _replace(p, i, label, **changes):
    """p with table i changed (every length that shares the table object follows it)."""
    old = p.gain[i]
    new = dataclasses.replace(old, **changes)
    q = tv.with_gain(p, [new if g is old and j > 0 else g for j, g in enumerate(p.gain)], label)
    return mp.with_method(q, p.method)


def _all_tables(p, label, fn):
    """p with fn(table) on every distinct table of lengths 1 .. N - 1."""
    done = {}
    gains = [p.gain[0]]
    for g in p.gain[1:]:
        if id(g) not in done:
            done[id(g)] = fn(g)
        gains.append(done[id(g)])
    return mp.with_method(tv.with_gain(p, gains, label), p.method)


def spiked(p, row, w, col=None):
    """One lineshape value w in `row` of the length-1 table."""
    g = p.gain[1]
    gv = g.gv.copy()
    gv[row * g.Nv + (g.Nv // 2 if col is None else col)] = F(w)
    return _replace(p, 1, f" / gv[{row}] = {float(w)!r}", gv=gv)


def _columns(g, lo, hi):
    """[Ny*Nx] mask of the columns int(lo Nx) <= ix < int(hi Nx)."""
    ix = np.tile(np.arange(g.Nx), g.Ny)
    return (ix >= int(lo * g.Nx)) & (ix < int(hi * g.Nx))


def exact_cap_spikes(probe, ray_cls_at, lo=0.05):
    """(ray, slot, (w_above, w_equal, w_below)): a slot whose |gs| is the largest of its ray (the nearest to 0.5 of them),
    whose ray is REGULAR under gs_cap = |gs| (so it holds no gs = 0 slot), and for which floats w exist with fl(708 / w) equal to |gs|, one ulp above
    and one ulp below it."""
    g = np.abs(probe["gvl"].astype(F))
    top = g.max(axis=1)
    order = np.argsort(np.abs(top - F(0.5)), kind="stable")       # near the cap of cap_split: every class stays populated
    for r in order:
        t = F(top[r])
        if not (t > lo) or not np.isfinite(t):
            continue
        w = F(F(708.0) / t)
        for c in (np.nextafter(w, F(0)), w, np.nextafter(w, F(np.inf))):
            if F(F(708.0) / c) != t:
                continue
            a, b = np.nextafter(c, F(0)), np.nextafter(c, F(np.inf))
            # walk to the nearest floats whose cap differs from t (several w may share a cap)
            while F(F(708.0) / a) == t:
                a = np.nextafter(a, F(0))
            while F(F(708.0) / b) == t:
                b = np.nextafter(b, F(np.inf))
            if F(F(708.0) / a) == np.nextafter(t, F(np.inf)) and F(F(708.0) / b) == np.nextafter(t, F(0)) \
                    and ray_cls_at(t)[r] == REGULAR:
                return int(r), int(np.argmax(g[r])), (F(a), F(c), F(b))
    raise AssertionError("no slot whose |gs| is an exact gs_cap")


# ---------------------------------------------------------------------------------------------- tile mixes
def _take(pool, n, used):
    """n rays of the pool, unused ones first; a pool smaller than n is gone through again (a ray may appear twice in a
    list: each appearance is traced and deposited on its own, here and on the CPU)."""
    assert len(pool), "empty pool"
    fresh = [i for i in pool if i not in used]
    out = (fresh + [i for i in pool if i in used])
    while len(out) < n:
        out = out + list(pool)
    out = out[:n]
    used.update(out)
    return out


def layouts(reach):
    """The tile mixes of a regime that reaches the classes `reach` (ascending): (name, lanes) with lanes a list of classes.
    For (SMALL, REGULAR, IRREGULAR) these are: all-small, all-regular, all-irregular; all-small except a regular ray in
    lane 0, and in lane 63; all-regular except an irregular ray in lane 0, and in lane 63; small and irregular
    interleaved; all-regular except a holed ray in lane 0, and in lane 63; and the ragged last tile of 17 rays that ends
    in an irregular ray is added by compose().  REGULAR lanes hold no gs = 0 slot, so the all-regular tile and the two
    small-with-one-regular tiles run the straight-line ase_step block on the device (tile_branches says which branch)."""
    out = [(f"all {NAMES[c]}", [c] * TILE) for c in reach]
    for lo, hi in zip(reach, reach[1:]):
        out.append((f"{NAMES[lo]}, {NAMES[hi]} in lane 0", [hi] + [lo] * (TILE - 1)))
        out.append((f"{NAMES[lo]}, {NAMES[hi]} in lane 63", [lo] * (TILE - 1) + [hi]))
    if len(reach) > 1:
        out.append((f"{NAMES[reach[0]]} and {NAMES[reach[-1]]} interleaved", [reach[0], reach[-1]] * (TILE // 2)))
    if REGULAR in reach:        # what the fix of rt_tile_rec.inc is about: one big lane with a gs = 0 slot among regular rays
        out.append(("regular, holed in lane 0", [HOLED] + [REGULAR] * (TILE - 1)))
        out.append(("regular, holed in lane 63", [REGULAR] * (TILE - 1) + [HOLED]))
    return out


def compose(ray_cls, reach, escaped_pool=(), pinned=None, extra=None):
    """(indices into the population, [(name, first, lanes)]) of the list: the tiles of layouts(reach), a tile of escaped
    rays with a written slot that is not small (if the population has 64), and the ragged tile.  pinned = (layout name,
    lane, ray, allowed): that ray sits in that lane, and the other lanes of the tile come from `allowed` only.
    extra = (name, pool): one more tile of 64 rays of that pool (a pool of fewer is gone through again)."""
    rng = np.random.default_rng(7)          # (drawn from the whole population, not from its first pixels)
    pools = {c: [int(i) for i in rng.permutation(np.flatnonzero(ray_cls == c))] for c in tuple(reach) + (HOLED,)}
    used, idx, tiles = set(), [], []
    if pinned is not None:
        used.add(pinned[2])
    for name, lanes in layouts(reach):
        picks = {}
        for c in set(lanes):
            pool = pools[c]
            if pinned is not None and pinned[0] == name:
                pool = [i for i in pool if i in pinned[3]]
            picks[c] = _take(pool, lanes.count(c), used)
        tile = [picks[c].pop(0) for c in lanes]
        if pinned is not None and pinned[0] == name:
            tile[pinned[1]] = pinned[2]
        tiles.append((name, len(idx), list(lanes)))
        idx += tile
    if len(escaped_pool) >= TILE:
        tile = _take([int(i) for i in escaped_pool], TILE, used)
        tiles.append(("escaped, a written slot not small", len(idx), [int(ray_cls[i]) for i in tile]))
        idx += tile
    if extra is not None and len(extra[1]):
        tile = _take([int(i) for i in extra[1]], TILE, used)
        tiles.append((extra[0], len(idx), [int(ray_cls[i]) for i in tile]))
        idx += tile
    last = reach[-1]
    tile = _take(pools[reach[0]], RAGGED - 1, used) + _take(pools[last], 1, used)
    tiles.append((f"ragged, {RAGGED} rays ending in {NAMES[last]}", len(idx), [reach[0]] * (RAGGED - 1) + [last]))
    idx += tile
    return np.asarray(idx, dtype=np.int64), tiles


# ---------------------------------------------------------------------------------------------- the cases
@dataclasses.dataclass
class Case:
    regime: str
    N: int
    method: int
    p: object                    # the problem the device gets (the first of `tables` for cap_exact)
    plain: object                # the same without the spike (None if the regime has none)
    tables: list                 # cap_exact: the three problems, gs_cap one ulp above |gs|, equal, one ulp below; else [p]
    rays: np.ndarray             # the composed list
    idx: np.ndarray              # ... as indices into the population
    tiles: list                  # [(name, first, lanes)]
    cls: np.ndarray              # ray classes of the list under p
    slot: np.ndarray             # slot classes of the list under p
    probe: dict                  # the oracle's probe of the list (Iv included)
    pop_cls: np.ndarray
    pop_probe: dict
    row: int                     # the spike row, -1 without a spike
    chosen: tuple = None         # cap_exact: (position in the list, slot, |gs|)
    n_escaped_pool: int = 0
    slices: list = None          # [(first, count)]: contiguous parts of the ray grid for the one-launch runs (grid_slices)

    @property
    def label(self):
        return f"{self.regime} / N = {self.N} / method {self.method}"

    @property
    def sorted_order(self):
        """The list sorted by class: every tile but the boundary ones is homogeneous."""
        return np.argsort(self.cls, kind="stable")


_cases = {}


def _rows(probe, idx):
    return {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in probe.items()}


def _most_read_row(probe, L=1, where=None):
    S3 = rt.cabi.RT_N_SUB
    iv = probe["ivl"][:, (L - 1) * S3:L * S3]
    lit = (probe["gvl"][:, (L - 1) * S3:L * S3] != 0) if where is None else where[:, (L - 1) * S3:L * S3]
    rows, n = np.unique(iv[lit], return_counts=True)
    return int(rows[np.argmax(n)])


def tables_of(regime, b, pop, oracle):
    """(problems, plain problem or None, spike row or -1) of a regime on the base problem b."""
    def scaled(k):
        return _all_tables(b, f" / g0 2^{k}", lambda g: dataclasses.replace(g, g0=g.g0 * F(2.0 ** k)))

    def readers(q):        # the list's population and the grid slices of the one-launch runs: the spike row is free of both
        return oracle.probe(q, np.concatenate([pop, grid_rays(q, grid_slices(oracle, q, F(708.0) / W_SPLIT))]), want_Iv=False)

    if regime in ("cap_split", "cap_exact"):
        row = free_row(b, readers(b))
        return [spiked(b, row, W_SPLIT)], b, row
    if regime == "tiny":
        return [scaled(-97)], None, -1
    if regime == "zero_bands":
        def f(g):
            g0 = g.g0.copy()
            g0[_columns(g, 0.15, 0.45)] = F(0.0)
            g0[_columns(g, 0.55, 0.85)] = F(-0.0)
            return dataclasses.replace(g, g0=g0)
        return [_all_tables(b, " / g0 = +0 and -0 in bands", f)], None, -1
    if regime == "zero_all":
        return [_all_tables(b, " / g0 = 0", lambda g: dataclasses.replace(g, g0=np.zeros_like(g.g0)))], None, -1
    if regime == "absorbing":
        q = _all_tables(b, " / g0 negated in a band", lambda g: dataclasses.replace(g, g0=np.where(_columns(g, 0.3, 0.6), -g.g0, g.g0)))
        row = free_row(q, readers(q))
        return [spiked(q, row, W_SPLIT)], q, row
    if regime == "big":
        return [scaled(10)], None, -1
    pr = oracle.probe(b, pop, want_Iv=False)
    if regime == "nan_g0":
        g = b.gain[1]
        g0 = g.g0.copy()
        g0[_most_read_row(pr)] = np.nan
        return [_replace(b, 1, " / one g0 = NaN", g0=g0)], None, -1
    if regime == "nan_e0":
        g = b.gain[1]
        slot, _ = classify(pr, gs_cap(b))
        E0 = g.E0.copy()
        E0[_most_read_row(pr, where=(slot == SMALL) | (slot == REGULAR))] = np.nan
        return [_replace(b, 1, " / one E0 = NaN", E0=E0)], None, -1
    raise KeyError(regime)


def case(oracle, ase_small, regime, N, method):
    """The Case of (regime, N, method), built once per session."""
    key = (regime, N, method)
    if key in _cases:
        return _cases[key]
    b = base(ase_small, N, method)
    pop = population(b)
    tables, plain, row = tables_of(regime, b, pop, oracle)
    p = tables[0]
    pr = oracle.probe(p, pop)
    cap = gs_cap(p)
    slot, cls = classify(pr, cap)
    reach = REACH[regime]
    S = slot.shape[1]
    # escaped rays (flag bit 0) that left slots unwritten (zeros in the probe), with a written slot that is not small
    esc = np.flatnonzero(((pr["flags"] & 1) != 0) & (slot == IDENTITY).any(axis=1) & (cls >= REGULAR))
    pinned = chosen = None
    if regime == "cap_exact":
        def cls_at(t):
            return classify(pr, t)[1]
        r, s, ws = exact_cap_spikes(pr, cls_at)
        t = np.abs(pr["gvl"][r, s]).astype(F)
        tables = [spiked(plain, row, w) for w in ws]
        p = tables[0]
        cap = gs_cap(tables[1])
        assert cap == t
        slot, cls = classify(pr, cap)
        top = np.abs(pr["gvl"]).max(axis=1)
        allowed = set(int(i) for i in np.flatnonzero(top < t * F(0.999)))
        pinned = ("all regular", 0, r, allowed)
        esc = np.flatnonzero(((pr["flags"] & 1) != 0) & (slot == IDENTITY).any(axis=1) & (cls >= REGULAR))
    extra = None
    if regime == "big":
        extra = ("rays that fail with -3", np.flatnonzero(pr["err"] == -3))
    elif regime == "nan_g0":
        extra = ("a gain sum is NaN", np.flatnonzero(np.isnan(pr["gvl"]).any(axis=1)))
    elif regime == "nan_e0":
        extra = ("read the NaN of E0", np.flatnonzero((pr["evl"] != oracle.probe(b, pop, want_Iv=False)["evl"]).any(axis=1)))
    idx, tiles = compose(cls, reach, esc, pinned, extra)
    if pinned is not None:
        first = [f for name, f, _ in tiles if name == "all regular"][0]
        chosen = (first, s, float(t))
    slices = grid_slices(oracle, plain if plain is not None else p, F(708.0) / W_SPLIT if plain is not None else gs_cap(p))
    c = Case(regime, N, method, p, plain, tables, pop[idx], idx, tiles, cls[idx], slot[idx], _rows(pr, idx), cls, pr, row,
             chosen, len(esc), slices)
    _cases[key] = c
    return c


_slices = {}


def grid_slices(oracle, q, cap, tiles=4):
    """[(first, count)] with stride 1: up to three runs of 4 tiles inside one pixel each (consecutive rays of the grid
    share a pixel and differ in their angles), the first pixel -- of every 7th -- that holds a tile of the "small" branch,
    of the "regular" branch and of the "mixed" branch under gs_cap = cap (tile_branches).  The one-launch runs need a ray
    grid (a list keeps the two kernels); a strided slice puts rays of different pixels side by side and nearly every
    tile comes out mixed."""
    key = (id(q), float(cap))
    if key not in _slices:
        gx, gy, ga, gb = q.ray_grid
        per_pixel, n_pix, count = len(ga) * len(gb), len(gx) * len(gy), tiles * TILE
        assert count <= per_pixel
        found = {}
        for pix in range(0, n_pix, 7):
            first = pix * per_pixel
            pr = oracle.probe(q, q.build_rays(first + np.arange(count, dtype=np.int64)), want_Iv=False)
            for b in tile_branches(pr, cap):
                found.setdefault(b, (first, count))
            if len(found) == 3:
                break
        _slices[key] = (q, sorted(set(found.values())))
    return _slices[key][1]


def grid_rays(p, slices):
    return np.concatenate([p.build_rays(first + np.arange(count, dtype=np.int64)) for first, count in slices])


# ---------------------------------------------------------------------------------------------- gain only: the wave-wide `need`
LOW, MID, HIGH, GLNAN = 0, 1, 2, 3            # the largest gl of a ray: <= 700, (700, 709.78], beyond (exp overflows), NaN
GL_NAMES = {LOW: "gl <= 700", MID: "700 < gl <= 709.78", HIGH: "gl > 709.78", GLNAN: "gl NaN"}
EXP_MAX = 709.782712893384               # log(DBL_MAX)


@dataclasses.dataclass
class SeededCase:
    method: int
    p: object
    rays: np.ndarray
    tiles: list                  # [(name, first, count)]
    lit: np.ndarray              # per ray of the list: the seed factor is not 0
    gl: np.ndarray               # per ray of the list: LOW .. GLNAN
    probe: dict
    pop_lit: np.ndarray
    pop_gl: np.ndarray
    empty: list = None           # the (f0, gl) classes the population does not hold: no tile of them

    @property
    def label(self):
        return f"seeded_need / method {self.method}"


def gl_of(p, probe):
    """[n][K] gl = sum over the slots of (double) gs (double) w, in slot order (Helper.h:569-580)."""
    K = p.beam.nv
    gl = np.zeros((len(probe["gvl"]), K))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(probe["gvl"].shape[1]):
            w = p.gain[s // rt.cabi.RT_N_SUB + 1].gv.reshape(-1, K)[probe["ivl"][:, s]]
            gl += probe["gvl"][:, s:s + 1].astype(np.float64) * w.astype(np.float64)
    return gl


_seeded = {}


def seeded_case(oracle, seed_small, method):
    """seed_small with g0 2^10 and one NaN in a cell that rays read, every 977th ray of the grid: tiles of rays whose seed
    factor is 0 and whose gl stays below 700 (the wave skips the exponential) with ONE lane that needs it -- a seed factor,
    a gl in (700, 709.78], an overflowing gl (0 inf = NaN on the CPU), a NaN gl -- in lane 0 and in lane 63."""
    if method in _seeded:
        return _seeded[method]
    b = mp.with_method(seed_small, method)
    pop = b.build_rays(np.arange(0, b.n_rays_total, 977, dtype=np.int64))
    plain = oracle.probe(b, pop)
    lit = plain["Iv"].any(axis=1)            # Iv = f0 f[4][k] exp(gl) with a finite gl: zero rows are the rays with f0 = 0
    q = _all_tables(b, " / g0 2^10", lambda g: dataclasses.replace(g, g0=g.g0 * F(1024.0)))
    g0 = q.gain[1].g0.copy()
    g0[_most_read_row(plain)] = np.nan
    p = _replace(q, 1, ", one g0 = NaN", g0=g0)
    pr = oracle.probe(p, pop)
    gl = gl_of(p, pr)
    with np.errstate(invalid="ignore"):
        top = np.where(np.isnan(gl).any(axis=1), np.nan, gl.max(axis=1))
        cls = np.where(np.isnan(top), GLNAN, np.where(top > EXP_MAX, HIGH, np.where(top > 700.0, MID, LOW))).astype(np.int8)
    quiet = [int(i) for i in np.flatnonzero(~lit & (cls == LOW))]
    used, idx, tiles, empty = set(), [], [], []

    def add(name, tile):
        tiles.append((name, len(idx), len(tile)))
        idx.extend(tile)

    add("quiet: f0 = 0, gl <= 700", _take(quiet, TILE, used))
    for name, pool in [("f0 != 0, " + GL_NAMES[LOW], lit & (cls == LOW)), ("f0 = 0, " + GL_NAMES[MID], ~lit & (cls == MID)),
                       ("f0 = 0, " + GL_NAMES[HIGH], ~lit & (cls == HIGH)), ("f0 = 0, " + GL_NAMES[GLNAN], ~lit & (cls == GLNAN)),
                       ("f0 != 0, " + GL_NAMES[MID], lit & (cls == MID)), ("f0 != 0, " + GL_NAMES[HIGH], lit & (cls == HIGH)),
                       ("f0 != 0, " + GL_NAMES[GLNAN], lit & (cls == GLNAN))]:
        pool = [int(i) for i in np.flatnonzero(pool)]
        if not pool:
            empty.append(name)
            continue
        add(f"quiet, {name} in lane 0", _take(pool, 1, used) + _take(quiet, TILE - 1, used))
        add(f"quiet, {name} in lane 63", _take(quiet, TILE - 1, used) + _take(pool, 1, used))
    a, c = _take(quiet, TILE // 2, used), _take([int(i) for i in np.flatnonzero(lit)], TILE // 2, used)
    add("f0 = 0 and f0 != 0 interleaved", [v for pair in zip(a, c) for v in pair])
    add(f"ragged, {RAGGED} rays", _take(quiet, RAGGED - 1, used) + _take([int(i) for i in np.flatnonzero(cls != LOW)], 1, used))
    idx = np.asarray(idx, dtype=np.int64)
    _seeded[method] = SeededCase(method, p, pop[idx], tiles, lit[idx], cls[idx], _rows(pr, idx), lit, cls, empty)
    return _seeded[method]
