"""The launch rules of a run, without a device: rt_hip_debug_run_shape hands the decision a run makes (run_shape and
pass_shape, csrc/rt_run_shape.h) plain numbers and returns what the run would put on the queue.  The expected values
are worked out by hand from the rules; the boundaries are the measured ones the comments of rt_run_shape.h quote."""
import ctypes
import importlib

import pytest

cabi = importlib.import_module("raytrace-miniapp_amd").cabi

CU, LDS, BLOB = 256, 163840, 102400

#: every tuning knob of the launch; no test leaves one set
KNOBS = [
    "RT_HIP_MARCH", "RT_HIP_MARCH_IEEE", "RT_HIP_UPLOAD_SLICES", "RT_HIP_FUSED", "RT_HIP_FUSED_SEED", "RT_HIP_MARCH_THREADS",
    "RT_HIP_MARCH_MODE", "RT_HIP_MARCH_CHUNK", "RT_HIP_MARCH_PARK", "RT_HIP_MARCH_SPIN_LIMIT", "RT_HIP_LATE_X10",
    "RT_HIP_LATE2_X10", "RT_HIP_LATE_WAVES", "RT_HIP_LATE_CAP", "RT_HIP_FUSED_ROWS", "RT_HIP_FUSED_NODES", "RT_HIP_FUSED_SPLIT",
    "RT_HIP_FUSED_CONSUMERS", "RT_HIP_FUSED_CONSUMERS_FIRST", "RT_HIP_FREQ_WG_WAVES", "RT_HIP_FREQ_MIN_ROWS", "RT_HIP_FREQ_WGS",
]


@pytest.fixture(scope="module")
def hl(hip):
    return hip.HipLibrary.get()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    """No knob set unless the test sets it (through `monkeypatch`, which also deletes it again)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def shape(hl, knobs=None, monkeypatch=None, occupancy=1, **facts):
    f = cabi.RtRunFacts(size=ctypes.sizeof(cabi.RtRunFacts), cu_count=CU, lds_limit=LDS, blob_bytes=BLOB, tables_bounded=1,
                        c_h3=0.025, march_prune=1, ntest_proven=1, L=2, occupancy_per_cu=occupancy)
    for k, v in facts.items():
        assert hasattr(f, k), k
        setattr(f, k, v)
    for k, v in (knobs or {}).items():
        assert k in KNOBS
        monkeypatch.setenv(k, str(v))
    out = cabi.RtRunShape(size=ctypes.sizeof(cabi.RtRunShape))
    rc = hl.lib.rt_hip_debug_run_shape(ctypes.byref(f), ctypes.byref(out))
    assert rc == 0, hl.lib.rt_hip_last_error()
    return out


def has(out, **expected):
    got = {k: getattr(out, k) for k in expected}
    assert got == expected


TWO, IMAGE_ONE, STEP_ONE = 0, 1, 2

# A: the gain-only list of ASE_small's size on 256 CUs
A = dict(n_rays=399000, n_tiles=6235, use_emis=0, method=2, has_ray_list=1, K=84, Kp=84, n_iang=100)
# B: emission on the beam's own ray grid, 64 rays per pixel
B = dict(n_rays=1048576, n_tiles=16384, use_emis=1, method=1, own_cells=1, rays_per_pixel=64, K=64, Kp=64, n_iang=64)
B2 = dict(B, n_rays=589824, n_tiles=9216, n_iang=36, rays_per_pixel=36)


def test_case_a_two_kernels_gain_only_list(hl):
    out = shape(hl, **A)
    has(out, kind=TWO, lds_tab=1, n_launch=1, bthr=512, mode=3, opt=3, last_march_inst=7, bounded=1, grid=256, mlds=102400, chunk=64,
        late_first=0, late_waves=4, late_chunks=1246, occupancy_asked=0)
    has(out, pass_kind=0, pass_wg_waves=16, pass_nslot=9, pass_lds=161184, pass_grid=256, pass_fetch_shift=13)
    has(out, key_s6=1, key_emis=0, key_excl=0, park=12, spin_limit=1 << 24, no_skip=0)


def test_case_b_image_in_one_launch(hl):
    out = shape(hl, **B)
    has(out, kind=IMAGE_ONE, bthr=1024, mode=1, opt=3, chunk=64, maxq=2, nslot=0, per_wave=392,
        off_exp=102400, off_iang=106496, off_ctl=107008, off_rem=107024, off_nodes=109072, node_cap=162, off_buf=110368, n_free=16,
        flds=160544, split=1, k_part=16, n_consumers=4, consumers_first=0, tile_links=65536, fgrid=256,
        late_first=0, late_waves=4, late_chunks=3276, pass_fetch_shift=13, occupancy_asked=0)


def test_case_b2_36_rays_per_pixel(hl):
    out = shape(hl, **B2)
    has(out, kind=IMAGE_ONE, maxq=3, per_wave=456, off_ctl=106784, off_rem=106800, off_nodes=108848, node_cap=106, off_buf=109696,
        n_free=14, flds=160768, late_chunks=1843)


def test_case_c_step_in_one_launch(hl):
    out = shape(hl, **dict(B, step_on=1, step_one_launch=1))
    has(out, kind=STEP_ONE, per_wave=264, off_ctl=107520, off_rem=107536, off_nodes=109584, node_cap=162, off_buf=110880, n_free=16,
        flds=144672, k_part=16, n_consumers=4, late_chunks=3276)
    has(shape(hl, **dict(B, step_on=1, step_one_launch=0)), kind=TWO, pass_kind=2)


@pytest.mark.parametrize("per_cu, bthr", [(2559, 512), (2560, 768), (4095, 768), (4096, 1024)])
def test_threads_per_work_group(hl, per_cu, bthr):
    has(shape(hl, **dict(A, n_rays=CU * per_cu)), bthr=bthr)


def test_h2_h4_pruning(hl):
    has(shape(hl, **dict(A, n_rays=CU * 8191)), opt=3, bounded=1)
    has(shape(hl, **dict(A, n_rays=CU * 8192)), opt=7, bounded=1, last_march_inst=15)
    has(shape(hl, **dict(A, march_prune=2)), opt=7)
    has(shape(hl, **dict(A, march_prune=0)), opt=0, bounded=1)
    has(shape(hl, **dict(A, ntest_proven=0)), opt=0, bounded=1)
    has(shape(hl, **dict(A, tables_bounded=0)), opt=0, bounded=0, last_march_inst=0)


def test_upload_slices(hl):
    has(shape(hl, **dict(B, host_rays=1, n_rays=(1 << 21) - 1)), n_launch=1)
    has(shape(hl, **dict(B, host_rays=1, n_rays=1 << 21)), n_launch=3, kind=TWO)
    has(shape(hl, **dict(B, n_rays=1 << 21)), n_launch=1, kind=IMAGE_ONE)   # (only a list still on the host is sliced)


@pytest.mark.parametrize("change", [dict(rays_per_pixel=31), dict(exclusive=1), dict(probe_on=1), dict(debug=1), dict(safe=1)])
def test_what_keeps_the_image_run_two_kernels(hl, change):
    has(shape(hl, **dict(B, **change)), kind=TWO)


def test_i_ang_above_32_kb_keeps_two_kernels(hl):
    # tables of 64 KB, so that room in LDS is not what decides: a 32 KB I_ang goes along, a 33 KB one does not
    small_tables = dict(B, blob_bytes=65536)
    has(shape(hl, **dict(small_tables, n_iang=4096)), kind=IMAGE_ONE, off_ctl=65536 + 4096 + 32768)
    has(shape(hl, **dict(small_tables, n_iang=4224)), kind=TWO)


def test_fused_knob_keeps_two_kernels(hl, monkeypatch):
    has(shape(hl, {"RT_HIP_FUSED": 2}, monkeypatch, **B), kind=TWO)


def test_global_tables_ask_the_occupancy(hl):
    blob = LDS - 8192 + 16
    has(shape(hl, **dict(A, blob_bytes=LDS - 8192)), lds_tab=1, occupancy_asked=0)
    for occ, grid in ((1, 256), (3, 768), (0, 256)):   # (a query that reports nothing counts as one work-group)
        has(shape(hl, occupancy=occ, **dict(A, blob_bytes=blob)), lds_tab=0, bthr=256, mlds=0, occupancy_asked=1, grid=grid,
            late_chunks=0, late_waves=0)


def test_one_launch_that_does_not_fit_falls_through(hl):
    # 150 KB of tables: in LDS for the march (150 KB + 8 KB <= 160 KB), but none of the sixteen 3136-byte buffers of
    # the frequency pass fits beside them -- and at least half must
    blob = 150 * 1024
    out = shape(hl, **dict(B, blob_bytes=blob))
    # bthr 1024 (a candidate takes the full work-group), chunk and late zone by the two-kernel rule:
    # 1048576 / (256 * 16 * 8) = 32 -> 64; LATE2: 256 * 4 * 64 * 6 = 393216 rays, cap 20 % = 209715 -> 3276 chunks
    has(out, kind=TWO, lds_tab=1, bthr=1024, mlds=blob, chunk=64, late_first=0, late_waves=4, late_chunks=209715 // 64, pass_kind=0)
    # ... and with twice the rays, where the 20 % cap binds for neither zone and the two differ
    twice = dict(B, n_rays=CU * 8192, n_tiles=CU * 128)
    has(shape(hl, **twice), kind=IMAGE_ONE, late_chunks=(256 * 4 * 64 * 32 // 10) // 64)
    has(shape(hl, **dict(twice, blob_bytes=blob)), kind=TWO, late_chunks=(256 * 4 * 64 * 60 // 10) // 64)


def test_knobs_are_honoured_and_clamped(hl, monkeypatch):
    has(shape(hl, {"RT_HIP_MARCH_THREADS": 100}, monkeypatch, **A), bthr=64)       # (whole waves, not 100)
    has(shape(hl, {"RT_HIP_MARCH_THREADS": 5000}, monkeypatch, **A), bthr=1024)
    has(shape(hl, {"RT_HIP_MARCH_THREADS": 32}, monkeypatch, **A), bthr=64)
    monkeypatch.delenv("RT_HIP_MARCH_THREADS")
    has(shape(hl, {"RT_HIP_MARCH_CHUNK": 96}, monkeypatch, **A), chunk=96, late_chunks=79800 // 96)
    has(shape(hl, {"RT_HIP_MARCH_CHUNK": 100000}, monkeypatch, **A), chunk=4096)
    has(shape(hl, {"RT_HIP_MARCH_CHUNK": 100}, monkeypatch, **B), chunk=128)     # (one launch: whole tiles)
    monkeypatch.delenv("RT_HIP_MARCH_CHUNK")
    has(shape(hl, {"RT_HIP_FUSED_CONSUMERS": 99}, monkeypatch, **B), n_consumers=15, late_waves=1)
    has(shape(hl, {"RT_HIP_FUSED_CONSUMERS": 0}, monkeypatch, **B), n_consumers=0, late_waves=4)
    monkeypatch.delenv("RT_HIP_FUSED_CONSUMERS")
    has(shape(hl, {"RT_HIP_FUSED_SPLIT": 2}, monkeypatch, **B), split=0)
    has(shape(hl, {"RT_HIP_FUSED_SPLIT": 3}, monkeypatch, **B), split=2)
    has(shape(hl, {"RT_HIP_FUSED_SPLIT": 9}, monkeypatch, **B), split=2)
    monkeypatch.delenv("RT_HIP_FUSED_SPLIT")
    has(shape(hl, {"RT_HIP_MARCH": "global"}, monkeypatch, **A), lds_tab=0, bthr=256)
    has(shape(hl, {"RT_HIP_MARCH": "lds"}, monkeypatch, **A), lds_tab=1)
    monkeypatch.delenv("RT_HIP_MARCH")
    has(shape(hl, {"RT_HIP_MARCH_IEEE": 0}, monkeypatch, **A), bounded=0, opt=0)   # (set at all)
    monkeypatch.delenv("RT_HIP_MARCH_IEEE")
    has(shape(hl, {"RT_HIP_MARCH_PARK": "junk"}, monkeypatch, **A), park=12)
    has(shape(hl, {"RT_HIP_MARCH_PARK": 200}, monkeypatch, **A), park=64)
    # a knob changed between two calls of one process is seen
    monkeypatch.delenv("RT_HIP_MARCH_PARK")
    has(shape(hl, **A), park=12, bthr=512, chunk=64, lds_tab=1, bounded=1)


# ---- the two (method, seed) pairs Problem.method never produces (include/rt_hip.h takes any pair): emission with the
# ---- forward method, and gain-only with the backward method
FWD_EMIS = dict(B, method=2, own_cells=0)                  # (rt_hip_plan_set_ray_grid grants own_cells to method 1 only)
BWD_GAIN = dict(B, use_emis=0, method=1, own_cells=0)      # a seeded plan on the seed beam's grid
BWD_GAIN_OWN = dict(BWD_GAIN, own_cells=1)                 # ... and on the beam's own grid


def test_forward_emission_keeps_two_kernels_and_the_run_time_mode(hl):
    """The one-launch runs deposit at the launch ray by the few-runs rule: a deposit at the exit ray must not get there."""
    has(shape(hl, **FWD_EMIS), kind=TWO, mode=0, key_emis=1, pass_kind=0)
    has(shape(hl, **dict(FWD_EMIS, step_on=1, step_one_launch=1)), kind=TWO, mode=0, key_emis=1, pass_kind=2)
    # ... whatever own_cells says (the plan never sets it for method 2; the rule must not lean on that)
    has(shape(hl, **dict(FWD_EMIS, own_cells=1)), kind=TWO, mode=0)
    has(shape(hl, **dict(FWD_EMIS, own_cells=1, step_on=1, step_one_launch=1)), kind=TWO, mode=0)
    has(shape(hl, **dict(FWD_EMIS, has_ray_list=1)), kind=TWO, mode=0, key_emis=1)
    # the pair next to it is untouched
    has(shape(hl, **B), kind=IMAGE_ONE, mode=1, key_emis=1)
    has(shape(hl, **dict(B, has_ray_list=1, own_cells=0)), kind=TWO, mode=1)


@pytest.mark.parametrize("march_mode", [None, 0, 1, 2, 3, 4])
@pytest.mark.parametrize("facts", [BWD_GAIN, BWD_GAIN_OWN, dict(BWD_GAIN, has_ray_list=1)])
def test_backward_gain_only_takes_the_run_time_mode_under_every_march_mode(hl, monkeypatch, march_mode, facts):
    """RT_HIP_MARCH_MODE picks among the instances compiled for the gain-only FORWARD pair; none of them is backward."""
    knobs = {} if march_mode is None else {"RT_HIP_MARCH_MODE": march_mode}
    has(shape(hl, knobs, monkeypatch, **facts), kind=TWO, mode=0, key_emis=0, pass_kind=0)
    # (the forward pair does follow the knob: the case above is no accident of the harness)
    has(shape(hl, knobs, monkeypatch, **dict(facts, method=2, own_cells=0)), mode=3 if march_mode is None else march_mode)


@pytest.mark.parametrize("facts", [BWD_GAIN, BWD_GAIN_OWN])
def test_backward_gain_only_on_a_grid_may_take_the_one_launch(hl, monkeypatch, facts):
    """fused_gain does not ask for the method: RT_HIP_FUSED_SEED=1 takes a backward seeded grid into the one launch, with
    the run-time mode of the march and the gain-only deposit (row caches, consumer waves with a buffer of their own)."""
    out = shape(hl, {"RT_HIP_FUSED_SEED": 1}, monkeypatch, **facts)
    has(out, kind=IMAGE_ONE, mode=0, key_emis=0, key_excl=0, nslot=7, maxq=3, k_part=0, late_chunks=0, pass_kind=0)
    assert 3 <= out.n_free <= 16 and 1 <= out.n_consumers <= 4
    has(shape(hl, {"RT_HIP_FUSED_SEED": 1}, monkeypatch, **dict(facts, has_ray_list=1)), kind=TWO, mode=0)
    has(shape(hl, {"RT_HIP_FUSED_SEED": 1}, monkeypatch, **dict(facts, step_on=1)), kind=TWO, mode=0, pass_kind=2)
    monkeypatch.delenv("RT_HIP_FUSED_SEED")
    has(shape(hl, **facts), kind=TWO, mode=0)


def test_argument_errors(hl):
    lib = hl.lib

    def call(f, out):
        rc = lib.rt_hip_debug_run_shape(ctypes.byref(f) if f is not None else None, ctypes.byref(out) if out is not None else None)
        return rc, lib.rt_hip_last_error().decode()

    def facts(**kw):
        return cabi.RtRunFacts(**dict(dict(size=ctypes.sizeof(cabi.RtRunFacts), cu_count=CU, lds_limit=LDS, L=2), **kw))

    def out():
        return cabi.RtRunShape(size=ctypes.sizeof(cabi.RtRunShape))

    assert call(facts(), out())[0] == 0
    for f, o in ((None, out()), (facts(), None), (facts(size=8), out()), (facts(), cabi.RtRunShape(size=0)),
                 (facts(cu_count=0), out()), (facts(lds_limit=0), out())):
        rc, msg = call(f, o)
        assert rc != 0 and "rt_hip_debug_run_shape" in msg, (rc, msg)
