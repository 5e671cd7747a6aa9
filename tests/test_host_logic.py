"""Host-side logic around the back-end loop: ray list, scaling, sharding, checks."""
import copy
import importlib

import numpy as np
import pytest

rt = importlib.import_module("raytrace-miniapp_amd")
problem = importlib.import_module("raytrace-miniapp_amd.problem")


def test_ray_list_order_and_rounding(ase_small):
    p = ase_small
    rays = p.build_rays()
    b = p.beam
    assert len(rays) == b.nx * b.ny * b.na * b.nb
    # b fastest, then a, y, x  (RayTraceImage.cpp:305-309)
    assert rays["b"][1] == np.float32(b.b[1]) and rays["a"][1] == np.float32(b.a[0])
    assert rays["a"][b.nb] == np.float32(b.a[1])
    assert rays["y"][b.na * b.nb] == np.float32(b.y[1])
    assert rays["x"][b.ny * b.na * b.nb] == np.float32(b.x[1])
    assert rays["x"][-1] == np.float32(b.x[-1]) and rays["b"][-1] == np.float32(b.b[-1])


def test_strided_decomposition_partitions_the_rays(ase_small):
    p = ase_small
    ids = []
    for start in range(3):
        q = copy.copy(p)
        q.N_start, q.N_parallel = start, 3
        ids.append(q.ray_ids())
    allids = np.sort(np.concatenate(ids))
    assert np.array_equal(allids, np.arange(p.n_rays_total))
    q = copy.copy(p)
    q.N_parallel = 0
    with pytest.raises(ValueError):
        q.ray_ids()


def test_scale_problem_matches_the_reference_rule(ase_small, seed_small):
    q = rt.scale_problem(ase_small, 16.0)         # the ASE_medium stand-in
    b = q.beam
    assert (b.nx, b.ny, b.na, b.nb) == (120, 50, 38, 28) and q.n_rays_total == 6384000
    o = ase_small.beam
    # same physical extents, cell-centred (CreateImageHelpers.cpp:107-142)
    assert np.isclose(b.x[0] - 0.5 * b.dx, o.x[0] - 0.5 * o.dx) and np.isclose(b.x[-1] + 0.5 * b.dx, o.x[-1] + 0.5 * o.dx)
    q.validate()
    s = rt.scale_problem(seed_small, 16.0)
    assert (s.seed_beam.nx, s.seed_beam.ny, s.seed_beam.na, s.seed_beam.nb) == (240, 50, 102, 102)
    assert rt.scale_problem(ase_small, 0.1).n_rays_total == 33 * 14 * 10 * 7


def test_validate_rejects_what_create_image_rejects(ase_small, seed_small):
    q = copy.copy(ase_small)
    q.beam = copy.copy(ase_small.beam)
    q.beam.x = q.beam.x.copy()
    q.beam.x[3] += 1e-6
    with pytest.raises(ValueError, match="uniform"):
        q.validate()
    q = copy.copy(ase_small)
    q.gain = ase_small.gain * 7                     # N = 21 > N_MAX
    with pytest.raises(ValueError, match="length segments"):
        q.validate(enforce_reference_limits=True)
    q.validate()                                    # our limit is runtime
    big = problem.resample_frequency(ase_small, 128)
    with pytest.raises(ValueError, match="frequencies"):
        big.validate(enforce_reference_limits=True)
    big.validate()
    s = copy.copy(seed_small)
    s.seed_beam = copy.copy(seed_small.seed_beam)
    s.seed_beam.y = -s.seed_beam.y[::-1].copy()
    with pytest.raises(ValueError, match="Negitive y"):
        s.validate()


def test_resample_frequency_preserves_dv_sum(ase_small):
    q = problem.resample_frequency(ase_small, 512)
    assert q.beam.nv == 512 and q.gain[1].Nv == 512
    assert np.isclose(q.beam.dv.sum(), ase_small.beam.dv.sum())
    assert q.gain[1].gv.shape[0] == 106 * 26 * 512
    r0 = ase_small.gain[1].gv.reshape(-1, 52)
    r1 = q.gain[1].gv.reshape(-1, 512)
    assert np.array_equal(r1[:, 0], r0[:, 0]) and np.allclose(r1[:, -1], r0[:, -1])


def test_shard_columns_partitions_pixels(ase_small, seed_small):
    W = 4
    cols = []
    for r in range(W):
        s = problem.shard_columns(ase_small, r, W)
        assert s.beam.dx == ase_small.beam.dx and s.beam.ny == ase_small.beam.ny
        cols.append(s.beam.x)
    assert np.array_equal(np.sort(np.concatenate(cols)), ase_small.beam.x)
    s = problem.shard_columns(seed_small, 1, W)
    assert s.beam.nx == seed_small.beam.nx                       # deposit grid stays whole
    assert np.array_equal(s.seed_beam.x, seed_small.seed_beam.x[1::W])
    assert problem.shard_columns(ase_small, 0, 1) is ase_small


# ---- ray list -> tensor grid recognition (include/rt_hip.h, rt_hip_ray_list_grid_dims; host only) ----
def _grid_rays(nx, ny, na, nb, seed=0):
    import numpy as np
    cabi = importlib.import_module("raytrace-miniapp_amd.cabi")
    rng = np.random.default_rng(seed)
    g = [np.sort(rng.uniform(-1, 1, n)).astype(np.float32) for n in (nx, ny, na, nb)]
    ids = np.arange(nx * ny * na * nb)
    rays = np.empty(len(ids), dtype=cabi.RAY_DTYPE)
    rays["b"] = g[3][ids % nb]
    rays["a"] = g[2][(ids // nb) % na]
    rays["y"] = g[1][(ids // (nb * na)) % ny]
    rays["x"] = g[0][ids // (nb * na * ny)]
    return rays


@pytest.mark.parametrize("dims", [(5, 4, 3, 2), (7, 1, 1, 3), (1, 1, 1, 9), (3, 5, 1, 1), (1, 6, 2, 1), (64, 32, 7, 5)])
def test_ray_list_recognised_as_tensor_grid(dims):
    backend = importlib.import_module("raytrace-miniapp_amd.backend")
    rays = _grid_rays(*dims)
    got = backend.ray_list_grid_dims(rays)
    # axes of length 1 are indistinguishable from their neighbours: what counts is that the product and
    # the generated order agree, which the library checks ray by ray
    assert got is not None
    assert got[0] * got[1] * got[2] * got[3] == len(rays)
    nz = [d for d in dims if d > 1]
    assert [d for d in got if d > 1] == nz


def test_ray_list_that_is_not_a_grid_is_rejected():
    import numpy as np
    backend = importlib.import_module("raytrace-miniapp_amd.backend")
    rays = _grid_rays(6, 5, 4, 3)
    assert backend.ray_list_grid_dims(rays) == (6, 5, 4, 3)
    bad = rays.copy()
    bad["a"][len(bad) // 2] = np.nextafter(bad["a"][len(bad) // 2], np.float32(9))      # one ulp, one ray
    assert backend.ray_list_grid_dims(bad) is None
    assert backend.ray_list_grid_dims(rays[:-1]) is None                                 # ragged tail
    assert backend.ray_list_grid_dims(rays[::2].copy()) is None or len(rays[::2]) % 2 == 0   # strided subset
    sw = rays.copy()
    sw[[3, 4]] = sw[[4, 3]]                                                               # two rays swapped
    assert backend.ray_list_grid_dims(sw) is None
    neg = rays.copy()
    neg["x"][:] = 0.0
    neg["x"][7] = -0.0                                                                    # -0.0 is not +0.0 bit for bit
    assert backend.ray_list_grid_dims(neg) is None


def test_ray_list_check_sees_one_flipped_bit_anywhere():
    """The bit-wise check behind the recognition, in both of its forms (one thread up to 16 MB of list, host threads
    beyond) and on a list that is only 4-byte aligned, as a vector of four-float rays may be."""
    import numpy as np
    backend = importlib.import_module("raytrace-miniapp_amd.backend")
    cabi = importlib.import_module("raytrace-miniapp_amd.cabi")
    # 144 KB and 20.6 MB of list with many rays per pixel; few rays per pixel (compared a piece of a pixel column at a
    # time): small, 30.7 MB, one ray per pixel, and a column too long for a column table
    for dims in ((9, 7, 11, 13), (40, 30, 37, 29), (5, 40, 3, 2), (64, 5000, 3, 2), (300, 200, 1, 1), (2, 600000, 2, 1)):
        rays = _grid_rays(*dims, seed=3)
        n = len(rays)
        raw = np.zeros(n * 16 + 4, np.uint8)
        off = raw[4:].view(cabi.RAY_DTYPE)                                 # the same list, 4 bytes off 8-byte alignment
        off[:] = rays
        assert off.ctypes.data % 8 == 4 or off.ctypes.data % 8 == 0
        for lst in (rays, off):
            got = backend.ray_list_grid_dims(lst)
            assert got is not None and [d for d in got if d > 1] == [d for d in dims if d > 1]
            dims = got                                                     # (axes of length 1 may be named differently)
            rng = np.random.default_rng(n)
            spots = [0, 1, n - 1, n - 2, n // 2] + list(rng.integers(2, n - 2, 6))
            # ray 0 and the first ray of each period define the guess itself: a flip there changes the guessed grid,
            # and the rest of the list then disagrees with it
            for r in spots:
                for f in ("x", "y", "a", "b"):
                    keep = lst[f][r]
                    lst[f][r] = np.nextafter(keep, np.float32(9))
                    assert backend.ray_list_grid_dims(lst) != dims, (dims, int(r), f)
                    lst[f][r] = keep
            assert backend.ray_list_grid_dims(lst) == dims


def test_every_environment_switch_is_in_the_table_of_integration_md():
    """INTEGRATION.md holds ONE table of the RT_* environment variables the library, the adapter and the Python host
    read; a switch added to the code without a row there fails here."""
    import re
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    pkg = root / "raytrace-miniapp_amd"
    names = set()
    for f in list((pkg / "csrc").glob("*.hip")) + list((pkg / "csrc").glob("*.h")) + list((pkg / "host").glob("*.cpp")) + \
            list(pkg.glob("*.py")):
        names |= set(re.findall(r'"(RT_[A-Z][A-Z_0-9]+)"', f.read_text()))
    assert len(names) >= 20, names
    doc = (root / "INTEGRATION.md").read_text()
    missing = sorted(n for n in names if n not in doc)
    assert not missing, missing


def test_every_compile_time_switch_has_a_build_target():
    """Every RT_* name that a preprocessor conditional of csrc/ tests is defined (-DNAME) by some target of
    csrc/Makefile: an experiment whose build recipe is gone does not stay behind in the kernels."""
    import re
    from pathlib import Path
    csrc = Path(__file__).resolve().parents[1] / "raytrace-miniapp_amd" / "csrc"
    tested = {}
    for f in sorted(csrc.glob("*.hip")) + sorted(csrc.glob("*.h")) + sorted(csrc.glob("*.inc")):
        for line in f.read_text().splitlines():
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                for n in re.findall(r"\bRT_[A-Z][A-Z_0-9]*", line.split("//")[0]):
                    tested.setdefault(n, f.name)
    assert len(tested) >= 10, tested
    built = set(re.findall(r"-D(RT_[A-Z][A-Z_0-9]*)", (csrc / "Makefile").read_text()))
    orphans = {n: f for n, f in tested.items() if n not in built}
    assert not orphans, orphans


# ---- bench.py / multigpu plumbing that needs no GPU ---------------------------------------------------
def test_bench_module_does_not_touch_torch_before_it_spawns_its_ranks():
    """`python bench.py --gpus N` starts its ranks as a torch.distributed.run child; that is only safe if
    nothing before the spawn initialises HIP -- the module must not even import torch at import time."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    code = ("import sys, importlib.util\n"
            f"spec = importlib.util.spec_from_file_location('bench', {str(root / 'bench.py')!r})\n"
            "m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)\n"
            "assert 'torch' not in sys.modules, 'bench.py imported torch at module level'\n"
            "assert callable(m.self_launch) and callable(m.main)\n"
            "b = m.algorithmic_bytes(6384000, 75601675, 2, 52, False, 0, 6000, 1064)\n"
            "assert b['march'] == 7359904800 and b['freq'] == 7967232000 and b['path'] == 15327136800\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_assembler_single_rank_is_a_view_of_its_buffer(ase_small):
    import torch
    mg = importlib.import_module("raytrace-miniapp_amd.multigpu")
    p = rt.scale_problem(ase_small, 0.05)
    a = mg.Assembler(p, 0, 1)
    b = p.beam
    assert a.image.numel() == b.nx * b.ny * b.nv and a.iang.numel() == b.na * b.nb
    a.image.fill_(2.0)
    a.iang.fill_(3.0)
    img, ang = a.assemble()
    assert img.data_ptr() == a.buffer.data_ptr() and float(img.sum()) == 2.0 * a.image.numel()
    assert float(ang.sum()) == 3.0 * a.iang.numel()
    assert "gather" in a.describe()
    # tiles of an uneven split: widths differ by at most one column and cover the image
    cols = [mg.tile_columns(b.nx, r, 7) for r in range(7)]
    assert sum(cols) == b.nx and max(cols) - min(cols) <= 1


def test_magic_number_division_of_ray_numbers_is_exact():
    """DevRays::div_mul / div_sh (rt_raygrid.hip, magic_u31): x // d == (x * mul >> 32) >> sh for every x < 2^31, where
    mul = floor(2^(31+s) / d) + 1, s = ceil(log2 d), sh = s - 1 -- the rule the march uses to split a ray number
    into its grid indices (RayTraceImage.cpp:300-328) without an integer division.  The GPU parity tests cover the
    kernel itself; this pins the arithmetic, including the edge divisors."""
    import random
    rnd = random.Random(7)

    def magic(d):
        s = 0
        while (1 << s) < d:
            s += 1
        return (1 << (31 + s)) // d + 1, s - 1

    divisors = list(range(2, 600)) + [(1 << k) + e for k in range(1, 31) for e in (-1, 0, 1) if (1 << k) + e >= 2]
    divisors += [rnd.randrange(2, 1 << 31) for _ in range(500)]
    for d in divisors:
        mul, sh = magic(d)
        assert 0 < mul < (1 << 32) and sh >= 0
        xs = [0, 1, d - 1, d, d + 1, 2 * d - 1, (1 << 31) - 1, (1 << 31) - d, max(0, (1 << 31) - d - 1)]
        xs += [rnd.randrange(0, 1 << 31) for _ in range(40)]
        for x in xs:
            if 0 <= x < (1 << 31):
                assert ((x * mul) >> 32) >> sh == x // d, (d, x)


def test_cpu_baseline_uses_every_hardware_thread_of_the_affinity_mask(ase_small):
    """bench.py `cpu_baseline`: the reference's `threads` method takes std::thread::hardware_concurrency() threads
    (src/RayTraceImage.cpp:409-413); the baseline takes the affinity mask of this process, one pinned thread each,
    and times the unmodified reference loop (kind "reference") when oracle/_ref travelled, else the port."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, str(ROOT))
    bench = importlib.import_module("bench")
    info = bench.cpu_info()
    want = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    assert info["available"] == want == len(info["cpus"]) and 1 <= len(info["physical_cpus"]) <= want
    before = sorted(os.sched_getaffinity(0))
    rec = bench.cpu_baseline(ase_small, 4768067)
    assert sorted(os.sched_getaffinity(0)) == before, "the main thread's affinity is restored"
    assert rec["cores"] in (want, len(info["physical_cpus"])) and rec["all_hardware_threads"]["threads"] == want
    assert rec["kind"] in ("reference", "port") and rec["value"] > 0 and rec["one_core"]["value"] > 0
    assert rec["value"] >= 0.8 * rec["one_core"]["value"]          # more threads are not slower than one
    assert "round-robin" in rec["sample"] and "pinned" in rec["sample"]


def test_cpu_figure_for_config_5_is_a_sample_with_small_private_images():
    """bench.py `cpu_config5_sample` (the reference cannot run nv = 512, the restatement is timed on a
    sample and scaled by the ray count): every thread traces its own pixel columns into its own small image, the
    samples cover the whole grid, and the main thread's affinity is restored."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, str(ROOT))
    bench = importlib.import_module("bench")
    problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
    before = sorted(os.sched_getaffinity(0))
    rec = bench.cpu_config5_sample(rt, problem_mod, 4096 * 4096, 146242923)
    assert sorted(os.sched_getaffinity(0)) == before
    a, o = rec["all_threads"], rec["one_core"]
    assert rec["kind"] == "port" and a["rays"] == 512 * 512 and o["rays"] == 64 * 64 and o["threads"] == 1
    assert a["threads"] == min(len(before), 512) == rec["cores"]
    # both samples see the same mix of rays: ray-steps per ray agree to a few per cent, and with the full problem's
    assert abs(a["ray_steps"] / a["rays"] - o["ray_steps"] / o["rays"]) < 0.05 * a["ray_steps"] / a["rays"]
    assert abs(a["ray_steps"] / a["rays"] - 146242923 / 4096 ** 2) < 0.05 * a["ray_steps"] / a["rays"]
    assert a["value"] >= 0.8 * o["value"] and rec["ms_per_image_extrapolated"] == a["ms_per_image_extrapolated"] > 0


def test_bench_accounting_of_the_contract_formula():
    """B_read = 16 R + C_step S + 4 K 3 L R [+ (256 + 8 K) R_live]; the ASE_small figures of the
    survey (962 MB) must come out of bench.algorithmic_bytes."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, str(ROOT))
    bench = importlib.import_module("bench")
    a = bench.algorithmic_bytes(399000, 4768067, 2, 52, False, 0, 60 * 25, 19 * 14)
    assert a["march"] == 16 * 399000 + 96 * 4768067 and a["freq"] == 4 * 52 * 3 * 2 * 399000
    assert abs(a["path"] - 962e6) < 1e6 and a["write"] == 8 * (60 * 25 * 52 + 19 * 14)
    s = bench.algorithmic_bytes(7803000, 53573880, 2, 82, True, 6907454, 1500, 266)
    assert abs(s["path"] - 26.1e9) < 0.5e9


def _fracs(node, path=""):
    """Every (path, value) of a key named `frac` / ending in `_frac` in a nested record."""
    if isinstance(node, dict):
        for k, v in node.items():
            if (k == "frac" or k.endswith("_frac")) and not k.endswith("contract_frac") and k != "raw_frac":
                yield path + "/" + k, v
            yield from _fracs(v, path + "/" + k)
    elif isinstance(node, list):
        for i, v in enumerate(node):
            yield from _fracs(v, f"{path}[{i}]")


def test_bench_sub_records_never_show_a_fraction_above_one():
    """bench.py's `bounded_roof`: the contract formula's figure (algorithmic bytes over time over the HBM peak) exceeds 1
    where the caches serve the bytes; it is `contract_frac`.  `frac` is measured HBM traffic against the peak, the contract
    figure only while that is below 1, else null; `issue_frac` comes from the SQ pass.  """
    import importlib.util
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    spec = importlib.util.spec_from_file_location("bench_module", root / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    sys.modules["bench_module"] = bench
    spec.loader.exec_module(bench)
    hot = bench.bounded_roof(220.5e9, 26.2e-3)                      # config 5 by the formula: 1.05
    assert hot["contract_frac"] > 1.0 and hot["frac"] is None and hot["achieved"] is None
    meas = bench.bounded_roof(220.5e9, 26.2e-3, traffic=75.5e9)     # ... and by its measured traffic: 0.36
    assert meas["contract_frac"] > 1.0 and 0.3 < meas["frac"] < 0.4 and "measured" in meas["achieved_basis"]
    cool = bench.bounded_roof(15.33e9, 2.7e-3)
    assert cool["frac"] == cool["contract_frac"] and 0.69 < cool["frac"] < 0.72
    sq = {"avg": {"SQ_INSTS_VALU": 13.9e9, "SQ_INSTS_SALU": 0.8e9}}
    iss = bench.bounded_roof(206e9, 22e-3, None, sq, 2.28e9)
    assert 0.5 < iss["issue_frac"] < 0.7 and iss["issue"]["unit"] == "G wave-instr/s"
    for rec in (hot, meas, cool, iss):
        for path, v in _fracs(rec):
            assert v is None or v <= 1.0, (path, v)


def test_bench_dump_outputs_writes_float64_and_samples_large_images(tmp_path, monkeypatch):
    """bench.py --dump-outputs: image and I_ang as flat float64 .npy files; an image above DUMP_IMAGE_MAX_BYTES is
    written as a fixed, seeded sample whose element indices are written beside it."""
    import importlib.util
    import sys
    from pathlib import Path

    import torch
    root = Path(__file__).resolve().parents[1]
    spec = importlib.util.spec_from_file_location("bench_dump", root / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    sys.modules["bench_dump"] = bench
    spec.loader.exec_module(bench)
    image = torch.arange(1000, dtype=torch.float64) * 0.5
    iang = torch.arange(7, dtype=torch.float64)
    bench.dump_outputs(torch, str(tmp_path / "whole"), image, iang)
    img = np.load(tmp_path / "whole" / "image.npy")
    assert img.dtype == np.float64 and np.array_equal(img, image.numpy())
    assert np.array_equal(np.load(tmp_path / "whole" / "I_ang.npy"), iang.numpy())
    assert not (tmp_path / "whole" / "image_sample_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_IMAGE_MAX_BYTES", 8 * 100)
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), image, iang)
    idx = np.load(tmp_path / "a" / "image_sample_index.npy")
    sample = np.load(tmp_path / "a" / "image.npy")
    assert idx.dtype == np.float64 and len(idx) == 100 == len(np.unique(idx)) and sample.dtype == np.float64
    assert np.array_equal(sample, idx * 0.5)                                   # the values at those indices
    assert np.array_equal(idx, np.load(tmp_path / "b" / "image_sample_index.npy"))  # the same sample every run
