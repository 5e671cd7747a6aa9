/* Host restatement of the float64 building blocks of raytrace-miniapp_amd/csrc/rt_freq.hip: exp_tab, exp_tab_vec,
 * ase_step, ase_step_f32 and ase_update -- the same operations in the same order, the tables handed in.  Compiled by
 * tests/devmath.py with `cc -O2 -ffp-contract=off`; fma() / fmaf() are the C library's (exact).
 *
 * exp_tab, exp_tab_vec, ase_step and ase_step_f32 are fma / mul / add / ldexp sequences with no a*b+c left for a
 * compiler to contract: fed the tables a device dumped, this file gives what the device must give, bit for bit.
 * ase_update is not of that kind (its cubic is plain a*b+c, which the device build may contract, and its division is
 * the device's reciprocal sequence, a true division here): it is compared through bounds only.
 * dm_host_tanf / dm_host_atanf are loops over the host libm's own routines, nothing restated.
 *
 * Layout of the step forms: group g holds one (gs, rs) and VEC = 4 pairs (Iv, w), as a lane of the frequency loop. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define VEC 4
#define EXP_TAB 256

static inline uint64_t bits64(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static inline double from64(uint64_t u) { double v; memcpy(&v, &u, 8); return v; }
static inline uint32_t bits32(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static inline int32_t lo_word(double v) { return (int32_t) (uint32_t) bits64(v); }
static inline uint32_t hi_word(double v) { return (uint32_t) (bits64(v) >> 32); }
static inline double join(uint32_t hi, uint32_t lo) { return from64(((uint64_t) hi << 32) | lo); }
/* n >> 8 and n & 255 of a signed n, as the device has them (arithmetic shift, two's complement) */
static inline int32_t sar8(int32_t n) { return n >= 0 ? n >> 8 : -(int32_t) (((uint32_t) (-(n + 1)) >> 8) + 1); }

static double exp_tab1(double x, const double *tab)
{
    const double L2E  = 369.3299304675746;
    const double C_HI = 0x1.62e42fef00000p-9;
    const double C_LO = 0x1.473de6af278edp-42;
    const double xc   = fmin(fmax(x, -1100.0), 1100.0);
    const double t    = rint(xc * L2E);
    const int32_t n   = (int32_t) t;
    double r          = fma(-t, C_HI, xc);
    r                 = fma(-t, C_LO, r);
    double p          = fma(r, 1.0 / 120.0, 1.0 / 24.0);
    p                 = fma(r, p, 1.0 / 6.0);
    p                 = fma(r, p, 0.5);
    p                 = fma(r, p, 1.0);
    p                 = fma(r, p, 1.0);
    return ldexp(tab[n & (EXP_TAB - 1)] * p, sar8(n));
}

void dm_exp_tab(const double *tab, const double *x, double *out, size_t n)
{
    for (size_t i = 0; i < n; i++)
        out[i] = exp_tab1(x[i], tab);
}

void dm_exp_tab_vec(const double *tab, const double *x, double *out, size_t n)
{
    const double L2E   = 369.3299304675746;
    const double C_HI  = 0x1.62e42fef00000p-9;
    const double C_LO  = 0x1.473de6af278edp-42;
    const double MAGIC = 0x1.8p52;
    for (size_t i = 0; i < n; i++) {
        const double xc = fmin(fmax(x[i], -1100.0), 1100.0);
        double t        = fma(xc, L2E, MAGIC);
        const int32_t k = lo_word(t);
        t -= MAGIC;
        double r = fma(-t, C_HI, xc);
        r        = fma(-t, C_LO, r);
        double p = fma(r, 1.0 / 24.0, 1.0 / 6.0);
        p        = fma(r, p, 0.5);
        p        = fma(r, p, 1.0);
        p        = fma(r, p, 1.0);
        const double v = ldexp(tab[k & (EXP_TAB - 1)] * p, sar8(k));
        out[i]         = x[i] != x[i] ? x[i] : v;
    }
}

/* e^x - 1 of ase_step for x = (double)(gs * w) */
static double em1_f64(float gs, float w, const double *tab)
{
    const double L2E   = 369.3299304675746;
    const double LN2_N = 0.0027076061740622863;
    const double MAGIC = 0x1.8p52;
    const double x     = (double) (gs * w);
    double t           = fma(x, L2E, MAGIC);
    const int32_t n    = lo_word(t);
    t -= MAGIC;
    double rq      = fma(-t, LN2_N, x);
    const double T = tab[n & (EXP_TAB - 1)];
    const int32_t m = sar8(n);
    double q       = fma(rq, 1.0 / 6.0, 0.5);
    q              = fma(rq, q, 1.0);
    rq *= q;
    const uint32_t hi = ((uint32_t) m << 20) + hi_word(T); /* v_lshl_add_u32: modulo 2^32 */
    const double S    = join(hi, (uint32_t) lo_word(T));
    return fma(S, rq, S - 1.0);
}

/* e^x - 1 of ase_step_f32; tab2 is the second table (high words less j << 12) */
static double em1_f32(float gs, float w, const double *tab2)
{
    const float L2E   = 369.32993f;
    const float C_HI  = 2.7076062e-3f;
    const float C_LO  = (float) (0.0027076061740622863 - (double) 2.7076062e-3f);
    const float MAGIC = 12582912.0f;
    const float x     = gs * w;
    const float t     = fmaf(x, L2E, MAGIC);
    const uint32_t nb = bits32(t);
    const float n     = t - MAGIC;
    float r           = fmaf(-n, C_HI, x);
    r                 = fmaf(-n, C_LO, r);
    const double T    = tab2[nb & (EXP_TAB - 1)];
    float q           = fmaf(r, 1.0f / 6.0f, 0.5f);
    q                 = fmaf(r, q, 1.0f);
    const float rq    = r * q;
    const uint32_t hi = (nb << 12) + hi_word(T);
    const double S    = join(hi, (uint32_t) lo_word(T));
    return fma(S, (double) rq, S - 1.0);
}

void dm_ase_step(const double *tab, const double *Iv, const float *gs, const double *rs, const float *w, double *out, size_t groups)
{
    for (size_t g = 0; g < groups; g++)
        for (int j = 0; j < VEC; j++) {
            const double em1 = em1_f64(gs[g], w[g * VEC + j], tab);
            out[g * VEC + j] = fma(em1, Iv[g * VEC + j] + rs[g], Iv[g * VEC + j]);
        }
}

void dm_ase_step_f32(const double *tab2, const double *Iv, const float *gs, const double *rs, const float *w, double *out, size_t groups)
{
    for (size_t g = 0; g < groups; g++)
        for (int j = 0; j < VEC; j++) {
            const double em1 = em1_f32(gs[g], w[g * VEC + j], tab2);
            out[g * VEC + j] = fma(em1, Iv[g * VEC + j] + rs[g], Iv[g * VEC + j]);
        }
}

/* branch[i] (if not NULL): 1 where the cubic of the small-gain branch was taken */
void dm_ase_update(const double *tab, const double *Iv, const float *gs, const float *es, const float *w, double *out,
                   unsigned char *branch, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        const double gl = (double) (gs[i] * w[i]);
        const double el = (double) (es[i] * w[i]);
        const int small = fabs(gl) < 1e-3;
        if (branch)
            branch[i] = (unsigned char) small;
        if (small) {
            out[i] = el * (1.0 + 0.5 * gl * (1.0 + 0.3333333333 * gl)) + Iv[i] * (1.0 + gl * (1.0 + 0.5 * gl));
        } else {
            const double eg = exp_tab1(gl, tab);
            out[i]          = el / gl * (eg - 1.0) + Iv[i] * eg;
        }
    }
}

/* the host libm's tanf / atanf over an array (what rt_march.hip's float kernels restate) */
void dm_host_tanf(const float *x, float *out, size_t n)
{
    for (size_t i = 0; i < n; i++)
        out[i] = tanf(x[i]);
}

void dm_host_atanf(const float *x, float *out, size_t n)
{
    for (size_t i = 0; i < n; i++)
        out[i] = atanf(x[i]);
}
