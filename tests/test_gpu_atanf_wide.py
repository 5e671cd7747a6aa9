"""atan_wide of raytrace-miniapp_amd/csrc/rt_march.hip on the device itself: atanf_flt32_kernel through
librt_hip_devmath.so for arguments of every branch of libm's float routine beyond |x| = 7/16 -- [7/16, 11/16),
[11/16, 19/16), [19/16, 39/16), [39/16, 2^25), from 2^25 on -- against the host libm, bit for bit.  (The host-side check
of the restatement over every float: tests/test_atanf_wide.py.)"""
import numpy as np
import pytest

import devmath as dm

pytestmark = pytest.mark.gpu
EDGES = [0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 25, 2.0 ** 100]


@pytest.fixture(scope="module")
def dev(hip):
    return dm.Device.get()


def test_device_atanf_equals_the_host_libm_on_every_wide_branch(dev):
    ref = dm.Ref.get()
    rng = np.random.default_rng(11)
    xs = []
    for lo, hi in zip(EDGES[:-1], EDGES[1:]):
        x = np.exp(rng.uniform(np.log(lo), np.log(hi), 40000)).astype(np.float32)
        x = x[(x >= np.float32(lo)) & (x < np.float32(hi))]
        assert x.size > 30000                                   # (every branch really gets its sample)
        # ... and the floats at and next to the branch's lower edge
        e = np.float32(lo)
        xs += [x, np.array([e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(np.inf))], np.float32)]
    xs.append(np.array([np.inf, np.finfo(np.float32).max], np.float32))
    x = np.concatenate(xs)
    x = np.concatenate([x, -x])
    got, want = dev.tan(dm.Device.ATAN, x), ref.host_atanf(x)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print(f"device atanf, |x| >= 7/16: {x.size} arguments, {bad.size} differ from the host libm", flush=True)
    assert bad.size == 0, (x[bad[:4]], got[bad[:4]], want[bad[:4]])
    nan = dev.tan(dm.Device.ATAN, np.array([np.nan], np.float32))
    assert np.isnan(nan[0])
