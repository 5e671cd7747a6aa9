"""atan_wide of raytrace-miniapp_amd/csrc/rt_march.hip -- atanf for |x| >= 7/16, the branches of libm's float routine
(glibc 2.35 flt-32 s_atanf.c) that exit directions more than 23.6 degrees off the axis take -- against the host atanf:
every float of [7/16, 2^25), both signs, and every 4096th bit pattern from 2^25 to infinity, where the routine returns
+-pi/2.  (The |x| < 7/16 branch: tests/test_float_identities.py.)"""
import ctypes
import subprocess

C_SRC = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>
static uint32_t bf(float x){uint32_t u;memcpy(&u,&x,4);return u;}
static float fb(uint32_t u){float x;memcpy(&x,&u,4);return x;}
/* rt_march.hip, atan_wide */
static float ka(float x)
{
    const float hi[4] = { 4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f };
    const float lo[4] = { 5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f };
    const float A0 = 3.3333334327e-01f, A1 = -2.0000000298e-01f, A2 = 1.4285714924e-01f, A3 = -1.1111110449e-01f,
                A4 = 9.0908870101e-02f, A5 = -7.6918758452e-02f, A6 = 6.6610731184e-02f, A7 = -5.8335702866e-02f,
                A8 = 4.9768779427e-02f, A9 = -3.6531571299e-02f, A10 = 1.6285819933e-02f;
    const uint32_t hx = bf(x), ix = hx & 0x7fffffffu;
    if (ix >= 0x4c000000u) {
        if (ix > 0x7f800000u) return x + x;
        return (hx >> 31) ? -hi[3] - lo[3] : hi[3] + lo[3];
    }
    int id;
    x = fabsf(x);
    if (ix < 0x3f980000u) {
        if (ix < 0x3f300000u) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }
        else { id = 1; x = (x - 1.0f) / (x + 1.0f); }
    } else {
        if (ix < 0x401c0000u) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }
        else { id = 3; x = -1.0f / x; }
    }
    const float z = x * x, w = z * z;
    const float s1 = z * (A0 + w * (A2 + w * (A4 + w * (A6 + w * (A8 + w * A10)))));
    const float s2 = w * (A1 + w * (A3 + w * (A5 + w * (A7 + w * A9))));
    const float r = hi[id] - ((x * (s1 + s2) - lo[id]) - x);
    return (hx >> 31) ? -r : r;
}
unsigned long check(unsigned long *n_checked)
{
    unsigned long bad = 0, n = 0;
    for (uint32_t u = 0x3ee00000u; u < 0x4c000000u; u++) {
        const float x = fb(u);
        n += 2;
        bad += bf(atanf(x)) != bf(ka(x));
        bad += bf(atanf(-x)) != bf(ka(-x));
    }
    for (uint32_t u = 0x4c000000u; u <= 0x7f800000u; u += 4096u) { /* (ends on the infinity exactly) */
        const float x = fb(u);
        n += 2;
        bad += bf(atanf(x)) != bf(ka(x));
        bad += bf(atanf(-x)) != bf(ka(-x));
    }
    const float qnan = fb(0x7fc00000u);
    bad += ka(qnan) == ka(qnan);
    *n_checked = n;
    return bad;
}
"""


def test_wide_argument_atanf_restatement_equals_the_host_libm(tmp_path):
    # (-fno-builtin: the compiler must not fold atanf of a constant loop bound itself -- it rounds correctly, libm does not)
    src, so = tmp_path / "atanw.c", tmp_path / "atanw.so"
    src.write_text(C_SRC)
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-builtin", "-shared", "-fPIC", "-o", str(so), str(src), "-lm"], check=True)
    lib = ctypes.CDLL(str(so))
    lib.check.restype = ctypes.c_ulong
    n = ctypes.c_ulong(0)
    bad = lib.check(ctypes.byref(n))
    assert n.value > 440_000_000 and bad == 0, (n.value, bad)
