"""record_set (csrc/rt_run_shape.h, RecordSet of csrc/rt_records.h) through rt_hip_debug_run_shape: the LDS of the second
pass is where the number of records of a run shows -- one I_ang histogram and one E_v accumulator per record -- so it is
held against the hand-worked formula of tests/test_seed_scan_host.py for all four record families, with n_seed = 2 and
L = 3.  (The pass kinds themselves are pinned in tests/test_run_shape_host.py.)"""
import pytest

from test_seed_scan_host import LDS, lds_by_hand, no_knobs, shape  # noqa: F401  (no_knobs is a fixture)


@pytest.mark.parametrize("family, facts, kind, n_rec", [
    ("seed set", dict(scan_on=0, n_seed=2), 3, 2),
    ("ASE seeds", dict(scan_on=0, n_seed=2, use_emis=1), 7, 1 + 2),
    ("length scan", dict(scan_on=1, n_seed=0), 5, 3),
    ("scan with seeds", dict(scan_on=1, n_seed=2), 6, 2 * 3),
])
def test_lds_of_the_pass_counts_the_records_of_every_family(no_knobs, family, facts, kind, n_rec):
    out = shape(K=84, Kp=84, n_iang=266, L=3, **facts)
    assert out.pass_kind == kind, family
    assert out.pass_in_lds == 1 and out.pass_lds == lds_by_hand(True, 266, 84, n_rec) <= LDS, family
    # ... and with the histograms in global memory (more than 32 KB of I_ang): the accumulators alone
    out = shape(K=84, Kp=84, n_iang=4097, L=3, **facts)
    assert out.pass_kind == kind and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 4097, 84, n_rec), family
