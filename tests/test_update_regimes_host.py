"""Census of the inputs of tests/test_gpu_update_regimes.py on the CPU oracle (tests/update_regimes.py): every regime
reaches the arithmetics it is meant to reach, every composed tile holds the stated lane mix, the lineshape spike sits in a
row nobody reads and changes nothing the CPU computes.  Conditions on the inputs: no device, nothing skipped."""
import numpy as np
import pytest

import update_regimes as ur

CASES = [(r, N, m) for r in ur.REGIMES for N in (3, 5) for m in (1, 2)]


def shared_lengths(p):
    return [L for L in range(1, p.N) if p.gain[L] is p.gain[1]]


@pytest.mark.parametrize("regime,N,method", CASES)
def test_census(oracle, ase_small, regime, N, method):
    c = ur.case(oracle, ase_small, regime, N, method)
    p = c.p
    assert p.method == method and p.N == N and p.use_emis and c.slot.shape[1] == (N - 1) * 3
    pop = {ur.NAMES[k]: int((c.pop_cls == k).sum()) for k in range(4)}
    slots = ur.classify(c.pop_probe, ur.gs_cap(p))[0]
    share = {ur.NAMES[k]: round(float((slots == k).mean()), 3) for k in range(4)}
    err = {int(k): int(v) for k, v in zip(*np.unique(c.pop_probe["err"], return_counts=True))}
    print(f"census / {c.label}: gs_cap {float(ur.gs_cap(p))!r}, rays by class {pop}, slots by class {share}, return codes {err}, "
          f"list of {len(c.rays)} rays in {len(c.tiles)} tiles, escaped rays with a written slot that is not small: {c.n_escaped_pool}")
    # every class the regime is meant to reach
    floor = ur.TILE if regime in ur.FINITE or regime == "big" else 1
    for k in ur.REACH[regime]:
        assert pop[ur.NAMES[k]] >= floor, (c.label, ur.NAMES[k], pop)
    # every tile with exactly the stated lane mix
    assert len(c.rays) < 1500 and len(c.rays) == c.tiles[-1][1] + ur.RAGGED
    names = [t[0] for t in c.tiles]
    for name, _ in ur.layouts(ur.REACH[regime]):
        assert name in names, (c.label, name)
    for name, first, lanes in c.tiles:
        assert first % ur.TILE == 0
        assert list(c.cls[first:first + len(lanes)]) == list(lanes), (c.label, name)
    if regime in ("cap_split", "absorbing"):
        assert names[:8] == ["all small", "all regular", "all irregular", "small, regular in lane 0", "small, regular in lane 63",
                             "regular, irregular in lane 0", "regular, irregular in lane 63", "small and irregular interleaved"]
        assert c.cls[3 * 64] == ur.REGULAR and (c.cls[3 * 64 + 1:4 * 64] == ur.SMALL).all()
        assert c.cls[7 * 64 - 1] == ur.IRREGULAR and (c.cls[6 * 64:7 * 64 - 1] == ur.REGULAR).all()
        assert (c.cls[7 * 64:8 * 64:2] == ur.SMALL).all() and (c.cls[7 * 64 + 1:8 * 64:2] == ur.IRREGULAR).all()
    assert c.cls[-1] == ur.REACH[regime][-1] and len(c.rays) % ur.TILE == ur.RAGGED
    # the branch every tile takes on the device (SF = 6: N = 3), restated from rt_tile_rec.inc on the sums of its 64 rays
    cap = ur.gs_cap(p)
    got = ur.tile_branches(c.probe, cap)
    assert len(got) == len(c.tiles)
    for (name, first, lanes), b in zip(c.tiles, got):
        assert b == ur.stated_branch(lanes), (c.label, name, b)
    want = {"all small": "small", "all regular": "regular", "all irregular": "mixed", "small, regular in lane 0": "regular",
            "small, regular in lane 63": "regular", "regular, irregular in lane 0": "mixed", "regular, irregular in lane 63": "mixed",
            "small and irregular interleaved": "mixed", "small, irregular in lane 0": "mixed", "small, irregular in lane 63": "mixed",
            "regular, holed in lane 0": "mixed", "regular, holed in lane 63": "mixed", "escaped, a written slot not small": "mixed"}
    for (name, first, lanes), b in zip(c.tiles, got):
        assert want.get(name, b) == b, (c.label, name, b)
    order = c.sorted_order
    by_class = ur.tile_branches({k: c.probe[k][order] for k in ("gvl", "evl")}, cap)
    on_grid = [b for first, count in c.slices for b in ur.tile_branches(oracle.probe(p, p.build_rays(first + np.arange(count, dtype=np.int64)), want_Iv=False), cap)]
    count = lambda v: {b: v.count(b) for b in ("small", "regular", "mixed")}
    print(f"census / {c.label}: tiles by branch, composed list {count(got)}, list sorted by class {count(by_class)}, "
          f"grid slices {c.slices} of the one-launch runs {count(on_grid)}; holed rays in the population {int((c.pop_cls == ur.HOLED).sum())}")
    if len(ur.REACH[regime]) == 3:
        assert (c.pop_cls == ur.HOLED).sum() >= ur.TILE
        for v in (got, by_class, on_grid):
            assert all(count(v)[b] >= 1 for b in ("small", "regular", "mixed")), (c.label, count(v))
        assert count(got)["regular"] == 3 and count(got)["small"] == 1
    # escaped rays (n_done < S) with a written slot that is not small: every regime but the NaN tables has a tile of them
    if regime not in ("nan_g0", "nan_e0"):
        assert "escaped, a written slot not small" in names, c.label
        first = c.tiles[names.index("escaped, a written slot not small")][1]
        esc = slice(first, first + ur.TILE)
        assert ((c.probe["flags"][esc] & 1) != 0).all() and (c.slot[esc] >= ur.REGULAR).any(axis=1).all()
        assert (c.slot[esc] == ur.IDENTITY).any(axis=1).all()             # slots they never wrote
    else:
        print(f"census / {c.label}: {c.n_escaped_pool} escaped rays with a written slot that is not small -- no tile of them")
    # the regime's own point
    g, e = c.probe["gvl"], c.probe["evl"]
    if regime == "tiny":
        below = (np.abs(g) < ur.RS_MIN) & (g != 0)
        assert below.sum() >= 64 and (np.abs(g) >= ur.RS_MIN).sum() >= 64 and np.isfinite(c.probe["Iv"]).all() and not c.probe["err"].any()
    if regime in ("zero_bands", "zero_all"):
        zero_lit = (g == 0) & (e != 0)
        assert zero_lit.sum() >= 64
        if regime == "zero_bands":          # (a sum that starts from +0 stays +0 over the -0 band: no gs is -0)
            assert not np.signbit(g[zero_lit]).any() and ((g != 0) & (c.slot == ur.SMALL)).sum() >= 64
            assert any(np.signbit(t.g0[t.g0 == 0]).any() and not np.signbit(t.g0[t.g0 == 0]).all() for t in c.p.gain[1:])
    if regime == "absorbing":
        for k in (ur.SMALL, ur.REGULAR, ur.IRREGULAR):
            assert ((g < 0) & (c.slot == k)).sum() >= 64, ur.NAMES[k]
        assert (c.probe["Iv"] >= 0).all() and (np.abs(g.sum(axis=1)) < 0.1 * np.abs(g).sum(axis=1))[np.abs(g).sum(axis=1) > 0].any()
    if regime in ur.FINITE:
        assert np.isfinite(c.probe["Iv"]).all() and not c.probe["err"].any(), c.label
    if regime == "big":
        assert (np.abs(g) > 708).sum() >= 64 and (c.probe["err"] == -3).sum() >= 64 and np.isinf(c.probe["Iv"]).any()
    if regime == "nan_g0":
        assert np.isnan(g).any() and (c.probe["err"] == -3).any() and np.isnan(c.probe["Iv"]).any()
    if regime == "nan_e0":
        assert np.isnan(c.p.gain[1].E0).sum() == 1 and "read the NaN of E0" in names
        assert np.isfinite(e).all() and np.isfinite(c.probe["Iv"]).all() and not c.probe["err"].any()     # the CPU clamps it to 0


@pytest.mark.parametrize("regime,N,method", [k for k in CASES if k[0] in ("cap_split", "cap_exact", "absorbing")])
def test_the_spike_sits_in_a_row_nobody_reads_and_changes_nothing_on_the_cpu(oracle, ase_small, regime, N, method):
    c = ur.case(oracle, ase_small, regime, N, method)
    assert c.row > 0
    grid = ur.grid_rays(c.p, c.slices)
    assert len(grid) < 1500
    for q in c.tables:
        g, plain = q.gain[1], c.plain.gain[1]
        diff = np.flatnonzero(g.gv != plain.gv)
        assert len(diff) == 1 and diff[0] // g.Nv == c.row and np.isfinite(g.gv[diff[0]])
        assert np.array_equal(g.g0, plain.g0) and np.array_equal(g.E0, plain.E0) and np.array_equal(g.n, plain.n)
        assert ur.gs_cap(q) == np.float32(708.0) / g.gv[diff[0]] and ur.gs_cap(c.plain) == np.float32(708.0)
        for rays in (c.rays, grid):
            a, b = oracle.probe(q, rays), oracle.probe(c.plain, rays)
            for L in shared_lengths(q):
                assert c.row not in a["ivl"][:, (L - 1) * 3:L * 3]
            for key in ("gvl", "evl", "ivl", "flags", "steps", "err"):
                assert np.array_equal(a[key], b[key]), key
            assert np.array_equal(a["Iv"].view(np.uint64), b["Iv"].view(np.uint64))
            assert np.array_equal(a["ray2"].view(np.uint32), b["ray2"].view(np.uint32))
            ia, ib = oracle.image_loop(q, rays), oracle.image_loop(c.plain, rays)
            assert np.array_equal(ia["image"].view(np.uint64), ib["image"].view(np.uint64))
            assert np.array_equal(ia["I_ang"].view(np.uint64), ib["I_ang"].view(np.uint64)) and ia["failure_code"] == ib["failure_code"] == 0


@pytest.mark.parametrize("N,method", [(N, m) for N in (3, 5) for m in (1, 2)])
def test_cap_exact_reaches_equality_and_both_neighbours(oracle, ase_small, N, method):
    c = ur.case(oracle, ase_small, "cap_exact", N, method)
    pos, s, t = c.chosen
    t = np.float32(t)
    assert np.abs(c.probe["gvl"][pos, s]) == t == np.abs(c.probe["gvl"][pos]).max()
    caps = [ur.gs_cap(q) for q in c.tables]
    print(f"census / {c.label}: |gs| {float(t)!r} of slot {s} of ray {pos} of the list, gs_cap of the three tables {[float(v) for v in caps]!r}")
    assert caps[0] == np.nextafter(t, np.float32(np.inf)) and caps[1] == t and caps[2] == np.nextafter(t, np.float32(0))
    tile = slice(pos, pos + ur.TILE)
    cls = [ur.classify(c.probe, cap)[1] for cap in caps]
    assert cls[0][pos] == ur.REGULAR and cls[1][pos] == ur.REGULAR and cls[2][pos] == ur.IRREGULAR
    for k in cls:                       # the other 63 lanes of its tile stay regular (no gs = 0 slot among them) ...
        assert (k[tile][1:] == ur.REGULAR).all()
    # ... so the tile runs the straight-line ase_step block with the cap above |gs| and equal to it, and per slot below it
    rows = {k: c.probe[k][tile] for k in ("gvl", "evl")}
    assert [ur.tile_branches(rows, cap)[0] for cap in caps] == ["regular", "regular", "mixed"]
    assert pos % ur.TILE == 0 and np.array_equal(cls[1], c.cls)


@pytest.mark.parametrize("method", [1, 2])
def test_seeded_need_census(oracle, seed_small, method):
    c = ur.seeded_case(oracle, seed_small, method)
    assert c.p.seed is not None and not c.p.use_emis and c.p.method == method and c.p.N == 3
    pop = {(("f0 != 0" if l else "f0 = 0"), ur.GL_NAMES[g]): int(((c.pop_lit == l) & (c.pop_gl == g)).sum()) for l in (False, True) for g in range(4)}
    print(f"census / {c.label}: {pop}; list of {len(c.rays)} rays, return codes "
          f"{dict(zip(*[v.tolist() for v in np.unique(c.probe['err'], return_counts=True)]))}")
    for g in range(4):                                         # every class of gl, in the population and in the list
        assert (c.pop_gl == g).any() and (c.gl == g).any(), ur.GL_NAMES[g]
    assert len(c.rays) < 1500 and (~c.lit).sum() >= 64 and c.lit.sum() >= 32
    for name, first, n in c.tiles:
        lit, gl = c.lit[first:first + n], c.gl[first:first + n]
        quiet = ~lit & (gl == ur.LOW)
        if name.startswith("quiet:"):
            assert quiet.all()
        elif "in lane 0" in name:
            assert quiet[1:].all() and not quiet[0]
        elif "in lane 63" in name:
            assert quiet[:-1].all() and not quiet[-1] and n == ur.TILE
    names = " ".join(t[0] for t in c.tiles)
    # every (f0, gl) class has its two tiles, but the one the population does not hold: under the forward method the rays
    # without a seed factor are the escaped ones, whose gl is short, and none of them falls into the 1.4 % window
    print(f"census / {c.label}: classes without a ray, hence without a tile: {c.empty}")
    assert c.empty == ([] if method == 1 else ["f0 = 0, " + ur.GL_NAMES[ur.MID]])
    for lit in ("f0 = 0", "f0 != 0"):
        for g in range(4):
            name = f"{lit}, {ur.GL_NAMES[g]}"
            if name not in c.empty and not (lit == "f0 = 0" and g == ur.LOW):
                assert f"quiet, {name} in lane 0" in names and f"quiet, {name} in lane 63" in names, name
    # an all-zero-seed tile one lane of which overflows: 0 inf = NaN on the CPU, which a wave that skipped the exponential misses
    assert "quiet, f0 = 0, gl > 709.78 in lane 0" in names and "quiet, f0 = 0, gl NaN in lane 63" in names
    assert "quiet, f0 != 0, 700 < gl <= 709.78 in lane 0" in names
    assert (c.probe["err"] == -3).any() and np.isnan(c.probe["Iv"]).any() and np.isinf(c.probe["Iv"]).any()
