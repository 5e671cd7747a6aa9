// rt_devmath.hip -- test-only unit: the float64 building blocks of the frequency pass (rt_freq.hip), the two float
// kernels of the march (rt_march.hip) and the seed-profile interpolation (pchip_eval / seed_factor of rt_math.h, and
// rt_seed_tab_kernel itself), each behind one elementwise kernel, and the two wave primitives of the step deposit (the E_v
// wave sum rt_step_evsum.inc, the segmented scan rt_wave_runs.inc / rt_wave_runscan.inc), each behind a kernel of one
// work-group, and the float32 blocks of the march -- one integrator step (rt_march_step.inc, in the four instances the product
// launches), the cross-cell set-up (rt_march_xsetup.inc), the escape test and cell set-up (rt_march_cell.inc, gathering from
// LDS and from global memory) and the float primitives of rt_math.h -- one case per lane in whole
// waves, so that tests/test_gpu_devmath.py, tests/test_gpu_march_blocks.py, tests/test_gpu_march_cell.py and
// tests/test_gpu_seed_profiles.py can run them on a device on inputs of their own choosing.  Builds to librt_hip_devmath.so with the product's flags; nothing
// of it is linked into librt_hip.so.
//
// The C face takes host arrays and gives host arrays: every call allocates, copies, launches, synchronises and
// frees, and returns 0 or the hipError_t of the first HIP call that failed, the frees included (rt_devmath_error names it).  Kernels: 256
// threads per work-group, a grid-stride loop, the two exponent tables filled in LDS by RT_FILL_EXP_TABLES -- the
// fill the product's kernels run -- and __syncthreads() before the first use.
#include "rt_freq.hip" // (includes rt_march.hip), as rt_launch.hip has it

#include "rt_blob_pack.h" // the host-side packing of the march blob, as rt_plan.hip has it

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <vector>

namespace {

using namespace rt;

constexpr int DM_BLOCK = 256;

enum : int { DM_EXP_TAB = 0, DM_EXP_TAB_VEC = 1 };
enum : int { DM_STEP_F64 = 0, DM_STEP_F32 = 1 };
enum : int { DM_DEPOSIT_FAST = 0, DM_DEPOSIT_4 = 1 };
enum : int { DM_TAN = 0, DM_ATAN = 1 };

// out[0..512): the tables as the first work-group sees them; out[512..1024): as the last one does
__global__ void __launch_bounds__(DM_BLOCK) dm_tables_kernel(double *out)
{
    __shared__ double exp2_tab[2 * EXP_TAB];
    RT_FILL_EXP_TABLES(exp2_tab)
    __syncthreads();
    // each thread copies entries that other threads wrote (thread t wrote entries t and 256 + t)
    for (int c = (int) threadIdx.x; c < 2 * EXP_TAB; c += (int) blockDim.x) {
        const int e = (c + 37) % (2 * EXP_TAB);
        if (blockIdx.x == 0)
            out[e] = exp2_tab[e];
        if (blockIdx.x == gridDim.x - 1) // (a launch of one work-group: it is both)
            out[2 * EXP_TAB + e] = exp2_tab[e];
    }
}

// exp_tab: one argument per thread and pass.  exp_tab_vec: VEC consecutive arguments per thread, the lock-step form;
// a ragged last group is padded with zeros and only its valid results are stored.
__global__ void __launch_bounds__(DM_BLOCK) dm_exp_kernel(int which, const double *x, double *out, size_t n)
{
    __shared__ double exp2_tab[2 * EXP_TAB];
    RT_FILL_EXP_TABLES(exp2_tab)
    __syncthreads();
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    const size_t first  = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (which == DM_EXP_TAB) {
        for (size_t i = first; i < n; i += stride)
            out[i] = exp_tab(x[i], exp2_tab);
    } else {
        const size_t groups = (n + VEC - 1) / VEC;
        for (size_t g = first; g < groups; g += stride) {
            double xv[VEC], ev[VEC];
#pragma unroll
            for (int j = 0; j < VEC; j++)
                xv[j] = g * VEC + j < n ? x[g * VEC + j] : 0.0;
            exp_tab_vec(xv, exp2_tab, ev);
#pragma unroll
            for (int j = 0; j < VEC; j++)
                if (g * VEC + j < n)
                    out[g * VEC + j] = ev[j];
        }
    }
}

__global__ void __launch_bounds__(DM_BLOCK) dm_update_kernel(const double *Iv, const float *gs, const float *es, const float *w,
                                                            double *out, size_t n)
{
    __shared__ double exp2_tab[2 * EXP_TAB];
    RT_FILL_EXP_TABLES(exp2_tab)
    __syncthreads();
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = ase_update(Iv[i], gs[i], es[i], w[i], exp2_tab);
}

// ase_step / ase_step_f32: group g holds one (gs, rs) and VEC (Iv, w) pairs, as a lane of the frequency loop does
__global__ void __launch_bounds__(DM_BLOCK) dm_step_kernel(int which, const double *Iv, const float *gs, const double *rs,
                                                          const float *w, double *out, size_t groups)
{
    __shared__ double exp2_tab[2 * EXP_TAB];
    RT_FILL_EXP_TABLES(exp2_tab)
    __syncthreads();
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for (size_t g = (size_t) blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        double iv[VEC];
        float wv[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            iv[j] = Iv[g * VEC + j];
            wv[j] = w[g * VEC + j];
        }
        if (which == DM_STEP_F64)
            ase_step(iv, gs[g], rs[g], wv, exp2_tab);
        else
            ase_step_f32(iv, gs[g], rs[g], wv, exp2_tab + EXP_TAB);
#pragma unroll
        for (int j = 0; j < VEC; j++)
            out[g * VEC + j] = iv[j];
    }
}

__global__ void __launch_bounds__(DM_BLOCK) dm_div_kernel(const double *a, const double *b, double *q, size_t n)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        q[i] = div_fast(a[i], b[i]);
}

// the four deposit cells of ray i: v[4 i + a] on axis a
struct DmAxes {
    int n[4];
    const double *g[4];
    double d[4], inv_d[4], g0[4], gl[4];
};
__global__ void __launch_bounds__(DM_BLOCK) dm_deposit_kernel(int which, const DmAxes X, const double *v, int *idx, size_t n)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        int ix[4];
        if (which == DM_DEPOSIT_4) {
            const AxisIn A[4] = { { X.n[0], X.g[0], X.d[0], X.inv_d[0], X.g0[0], X.gl[0], v[4 * i + 0] },
                                  { X.n[1], X.g[1], X.d[1], X.inv_d[1], X.g0[1], X.gl[1], v[4 * i + 1] },
                                  { X.n[2], X.g[2], X.d[2], X.inv_d[2], X.g0[2], X.gl[2], v[4 * i + 2] },
                                  { X.n[3], X.g[3], X.d[3], X.inv_d[3], X.g0[3], X.gl[3], v[4 * i + 3] } };
            deposit_index4(A, ix);
        } else {
#pragma unroll
            for (int a = 0; a < 4; a++)
                ix[a] = deposit_index_fast(X.n[a], X.g[a], X.d[a], X.inv_d[a], v[4 * i + a]);
        }
#pragma unroll
        for (int a = 0; a < 4; a++)
            idx[4 * i + a] = ix[a];
    }
}

__global__ void __launch_bounds__(DM_BLOCK) dm_tan_kernel(int which, const float *x, float *out, size_t n)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = which == DM_TAN ? tanf_flt32_kernel(x[i]) : atanf_flt32_kernel(x[i]);
}

// the seed profile (rt_math.h): one axis' interpolant; the whole factor at points [m][4] = (x, y, a, b)
__global__ void __launch_bounds__(DM_BLOCK) dm_pchip_kernel(int n, const double *xs, const double *ys, const double *x, double *y, size_t m)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride)
        y[i] = pchip_eval(n, xs, ys, x[i]);
}

__global__ void __launch_bounds__(DM_BLOCK) dm_seed_factor_kernel(const DevSeed sd, const double *pts, double *f, size_t m)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride)
        f[i] = seed_factor(sd, pts[4 * i + 0], pts[4 * i + 1], pts[4 * i + 2], pts[4 * i + 3]);
}

// ---- the two wave primitives of the step deposit, each on ONE work-group of DM_BLOCK threads: four waves, every wave with
// transposition rows and a pixel pattern of its own -----------------------------------------------------------------------
constexpr int DM_EV_KP_MAX = 64;

// rt_step_evsum.inc as a step tile includes it: Iv [256][Kp] (thread, frequency), deposits [256]; out [Kp] = the
// work-group's accumulator = scale * sum over the depositing threads
__global__ void __launch_bounds__(DM_BLOCK) dm_ev_sum_kernel(const double *Iv_in, const unsigned char *deposits, double scale, int Kp,
                                                            double *out)
{
    __shared__ double lds_ev[DM_EV_KP_MAX];
    __shared__ __align__(16) double rows[DM_BLOCK / WAVE][4 * XP_ROW];
    const struct {
        double scale;
    } H           = { scale };
    const int lane = lane_id();
    double *xpose  = rows[threadIdx.x >> 6];
    for (int c = (int) threadIdx.x; c < Kp; c += (int) blockDim.x)
        lds_ev[c] = 0.0;
    __syncthreads();
    const bool dep = deposits[threadIdx.x] != 0;
    for (int kb = 0; kb < Kp; kb += VEC) {
        double Iv[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            Iv[j] = Iv_in[(size_t) threadIdx.x * (size_t) Kp + kb + j];
#define EV_SUM_DEPOSITS dep
#define EV_SUM_INDEX kb
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
    }
    __syncthreads();
    for (int c = (int) threadIdx.x; c < Kp; c += (int) blockDim.x)
        out[c] = lds_ev[c];
}

// rt_wave_runs.inc and rt_wave_runscan.inc as the nf deposit of a step tile includes them: pix [256] (-1: no pixel),
// val [256]; nf [n_pix] += scale * val per pixel, one atomic per run of equal pixel and wave (the host face zeroes nf and
// has checked pix < n_pix)
__global__ void __launch_bounds__(DM_BLOCK) dm_nf_scan_kernel(const int *pix_in, const double *val, double scale, double *nf)
{
    const int lane = lane_id();
    const int pix  = pix_in[threadIdx.x];
    const bool dep = pix >= 0;
#define RUNS_PIX pix
#define RUNS_DEPOSITS dep
#include "rt_wave_runs.inc"
#undef RUNS_PIX
#undef RUNS_DEPOSITS
    double a = dep ? val[threadIdx.x] * scale : 0.0;
#include "rt_wave_runscan.inc"
    if (tail && a != 0.0)
        unsafeAtomicAdd(&nf[pix], a);
}

// ---- the float32 blocks of the march: one case per lane.  The fragments and inv_norm take wave-level decisions
// (__ballot), so these kernels run whole waves only: the index space is padded to a multiple of WAVE, a padding lane
// repeats the last case and stores nothing (no lane leaves early; the grid-stride loop ends for a whole wave at once: its
// stride is a multiple of DM_BLOCK) -------------------------------------------------------------------------------------
// rt_freq.hip, included above, ends with FMA contraction allowed (its float64 half); rt_launch.hip includes rt_march.hip in
// front of it.  The fragments below are float32 march code and must be compiled as march_wave compiles them:
#pragma clang fp contract(off)
enum : int { DM_STEP_IN = 14, DM_STEP_OUT = 8, DM_STEP_COUNTERS = 6 };
enum : int {
    DM_F32_INV_NORM = 0,
    DM_F32_DIV_BY_RECIP = 1,
    DM_F32_DIV_BY_RECIP_SIGNED = 2,
    DM_F32_FDIV_NR = 3,
    DM_F32_FDIV_ONE_NR = 4,
    DM_F32_FMIN_NAN_DROP = 5
};
enum : int { DM_F64_DIV_BY_RECIP = 0, DM_F64_DIV_BY_RECIP_TINY_OK = 1 };

__device__ __forceinline__ size_t dm_padded(size_t n) { return (n + WAVE - 1) / WAVE * WAVE; }

// the step factors as rt_hip_plan_set_step_factor derives them: what block [C] reads of DevParams
struct DmStepFactors {
    float c_cap, c_h1, c_h3;
};

// the stand-in for MarchDiag: which wave-uniform branches of block [C] this wave took in any of its passes
// (counters[k] += 1 per wave and launch: k = 0 .. 3 prune(k), 4 the tiny-dividend block, 5 every wave that held cases)
struct DmMarchDiag {
    unsigned took = 0;
    __device__ __forceinline__ void tick(int) {}
    __device__ __forceinline__ void tiny_dividend() { took |= 1u << 4; }
    __device__ __forceinline__ void prune(int i) { took |= 1u << i; }
    __device__ __forceinline__ void pass() { took |= 1u << 5; }
    __device__ __forceinline__ void wave_end(unsigned *counters)
    {
        if (lane_id() == 0)
            for (int k = 0; k < DM_STEP_COUNTERS; k++)
                if (took >> k & 1u)
                    atomicAdd(&counters[k], 1u);
    }
};

// rt_march_step.inc as march_wave includes it.  in [n][14] = n0, gxn, gyn, rx, ry, rz, sx, sy, sz, hsum, w_x, w_y, lim2,
// dzcap; out [n][8] = n, rx, ry, rz, sx, sy, sz, hsum; run [n]
template <bool BOUNDED, int OPT>
__global__ void __launch_bounds__(DM_BLOCK) dm_march_step_kernel(const DmStepFactors P, const float *in, float *out, unsigned char *run_out,
                                                                unsigned *counters, size_t n_cases)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    const size_t padded = dm_padded(n_cases);
    DmMarchDiag diag;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += stride) {
        const float *c = in + DM_STEP_IN * (i < n_cases ? i : n_cases - 1);
        diag.pass();
        const float n0 = c[0], gxn = c[1], gyn = c[2];
        float rx = c[3], ry = c[4], rz = c[5], sx = c[6], sy = c[7], sz = c[8], hsum = c[9], n = 0.0f;
        const float lim0 = 0.1f * c[10], lim1 = 0.1f * c[11]; // as block [C] has them from the interval records
        const float lim2 = c[12], dzcap = c[13];
        bool run;
        {
#include "rt_march_step.inc"
        }
        if (i < n_cases) {
            float *o = out + DM_STEP_OUT * i;
            o[0]     = n;
            o[1]     = rx;
            o[2]     = ry;
            o[3]     = rz;
            o[4]     = sx;
            o[5]     = sy;
            o[6]     = sz;
            o[7]     = hsum;
            run_out[i] = run ? 1 : 0;
        }
    }
    diag.wave_end(counters);
}

// rt_march_xsetup.inc as march_wave includes it.  fin [n][4] = px, py, w_x, w_y; din [n][8] = lo_x, rw_x, lo_y, rw_y and the
// corner indices n00, n10, n01, n11 (rounded and differenced here as block [A2] does it); mirror [n]; out [n][3] = n0, gxn, gyn.
// BOUNDED: the form of the instances that run under the ranges of the short forms (no sign copy on the quotients)
template <bool BOUNDED>
__global__ void __launch_bounds__(DM_BLOCK) dm_march_xsetup_kernel(const float *fin, const double *din, const unsigned char *mirror_in,
                                                                  float *out, size_t n_cases)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    const size_t padded = dm_padded(n_cases);
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += stride) {
        const size_t c  = i < n_cases ? i : n_cases - 1;
        const float px = fin[4 * c], py = fin[4 * c + 1];
        BlobGain G        = {}; // (the fragment reads one word of the lane's header: whether the y axis is mirrored)
        G.mirror_y        = mirror_in[c] != 0 ? 1 : 0;
        const double *d   = din + 8 * c;
        const f64x2 ix0 = { d[0], d[1] }, iy0 = { d[2], d[3] };
        const f32x4 ix1 = { fin[4 * c + 2], 0.0f, 0.0f, 0.0f }, iy1 = { fin[4 * c + 3], 0.0f, 0.0f, 0.0f };
        const double n00 = d[4], n10 = d[5], n01 = d[6], n11 = d[7];
        const float f00 = (float) n00, f10 = (float) n10, f01 = (float) n01, f11 = (float) n11;
        const double dnx0 = n10 - n00, dnx1 = n11 - n01, dny0 = n01 - n00, dny1 = n11 - n10;
        float n0, gxn, gyn;
        {
#include "rt_march_xsetup.inc"
        }
        if (i < n_cases) {
            out[3 * i]     = n0;
            out[3 * i + 1] = gxn;
            out[3 * i + 2] = gyn;
        }
    }
}

// rt_march_cell.inc as march_wave includes it: the escape test and the cell set-up, block [A2].  blob: the march blob as
// rt_hip_plan_create packs it (rt_blob_pack.h), blob_bytes a multiple of 16; LDS_TAB copies it to dynamic LDS, which starts at
// LDS address 0 (this kernel has no static LDS: the fragment's ds_read_b128 gather relies on it, as in rt_march_kernel), and the
// gather is the product's; otherwise the blob is read where it lies.  fin [n][5] = px, py, sz, z, z_stop; len [n] = the length
// ii of the case (checked by the host entry).  Every case starts from the same lane state -- the one below -- so that what
// a lane leaves untouched (an escaping lane: everything but `escaped`) is known.
// iout [n][DM_CELL_I] = escaped, st, c00, mirror, second gather taken, steps, cell_last, 0;
// fout [n][DM_CELL_F] = g0, E0, dzrem, ix1.xyzw, iy1.xyzw, f00, f10, f01, f11, z, gacc, eacc, pz, zc, path;
// dout [n][DM_CELL_D] = ix0.xy, iy0.xy, dnx0, dnx1, dny0, dny1.
// The second-gather flag is observed, not derived: bisect_interval is called on that arm of the fragment and nowhere else, and
// inside the include its name also raises the flag (a macro does not expand inside its own expansion).
enum : int { DM_CELL_IN = 5, DM_CELL_I = 8, DM_CELL_F = 21, DM_CELL_D = 8 };
template <bool LDS_TAB>
__global__ void __launch_bounds__(DM_BLOCK) dm_march_cell_kernel(const unsigned char *blob, unsigned blob_bytes, int use_emis_in,
                                                                const float *fin, const int *len, int *iout, float *fout, double *dout,
                                                                size_t n_cases)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    if (LDS_TAB) {
        const uint4 *src = reinterpret_cast<const uint4 *>(blob);
        uint4 *dst       = reinterpret_cast<uint4 *>(lds_raw);
        for (unsigned i = threadIdx.x; i < blob_bytes / 16; i += blockDim.x)
            dst[i] = src[i];
        __syncthreads();
    }
    const unsigned char *tab = LDS_TAB ? lds_raw : blob;
    const BlobGain *hdr      = reinterpret_cast<const BlobGain *>(tab);
    const unsigned lds_base  = LDS_TAB ? (unsigned) (size_t) (__attribute__((address_space(3))) unsigned char *) lds_raw : 0u;
    const bool use_emis      = use_emis_in != 0;
    DmMarchDiag diag;
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    const size_t padded = dm_padded(n_cases);
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += stride) {
        const size_t c = i < n_cases ? i : n_cases - 1;
        const float px = fin[DM_CELL_IN * c], py = fin[DM_CELL_IN * c + 1], sz = fin[DM_CELL_IN * c + 2];
        float z = fin[DM_CELL_IN * c + 3];
        const float z_stop = fin[DM_CELL_IN * c + 4];
        const BlobGain G   = march_blob_header(hdr, len[c], lds_base);
        // the lane state block [A2] writes, as march_wave declares it
        int st = ST_CELL, c00 = -1, cell_last = -1;
        unsigned steps = 0;
        bool regather  = false;
        float f00 = 1, f10 = 1, f01 = 1, f11 = 1;
        double dnx0 = 0, dnx1 = 0, dny0 = 0, dny1 = 0;
        f64x2 ix0 = { 0.0, 1.0 }, iy0 = { 0.0, 1.0 };
        f32x4 ix1 = { 1.0f, 0.0f, 0.0f, 0.0f }, iy1 = { 1.0f, 0.0f, 0.0f, 0.0f };
        float g0 = 0, E0 = 0, gacc = 0, eacc = 0;
        float dzrem = 0, zc = -1.0f, path = -1.0f, pz = -1.0f;
        {
#define bisect_interval(iv, n, v) (regather = true, bisect_interval(iv, n, v))
#include "rt_march_cell.inc"
#undef bisect_interval
        }
        if (i < n_cases) {
            int *io    = iout + DM_CELL_I * i;
            float *fo  = fout + DM_CELL_F * i;
            double *dd = dout + DM_CELL_D * i;
            // (whether the ray escaped is one of the lane's states, and the mirrored axis a word of its header: the columns
            // keep what they held when the two were flags beside `st` -- 1 = the lane waits for block [A], 2 = for [B])
            const bool escaped = st == ST_ESC;
            io[0]      = escaped ? 1 : 0;
            io[1]      = st == ST_XSETUP ? 2 : 1;
            io[2]      = c00;
            io[3]      = (!escaped && G.mirror_y != 0) ? 1 : 0;
            io[4]      = regather ? 1 : 0;
            io[5]      = (int) steps;
            io[6]      = cell_last;
            io[7]      = 0;
            fo[0]      = g0;
            fo[1]      = E0;
            fo[2]      = dzrem;
            fo[3]      = ix1.x;
            fo[4]      = ix1.y;
            fo[5]      = ix1.z;
            fo[6]      = ix1.w;
            fo[7]      = iy1.x;
            fo[8]      = iy1.y;
            fo[9]      = iy1.z;
            fo[10]     = iy1.w;
            fo[11]     = f00;
            fo[12]     = f10;
            fo[13]     = f01;
            fo[14]     = f11;
            fo[15]     = z;
            fo[16]     = gacc;
            fo[17]     = eacc;
            fo[18]     = pz;
            fo[19]     = zc;
            fo[20]     = path;
            dd[0]      = ix0.x;
            dd[1]      = ix0.y;
            dd[2]      = iy0.x;
            dd[3]      = iy0.y;
            dd[4]      = dnx0;
            dd[5]      = dnx1;
            dd[6]      = dny0;
            dd[7]      = dny1;
        }
    }
}

// the float primitives of rt_math.h, elementwise: out = f(a, b, y) (an argument a primitive does not take is not read)
__global__ void __launch_bounds__(DM_BLOCK) dm_f32_kernel(int which, const float *a, const float *b, const float *y, float *out,
                                                         size_t n_cases)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    const size_t padded = dm_padded(n_cases);
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += stride) {
        const size_t c = i < n_cases ? i : n_cases - 1;
        float r;
        switch (which) {
        case DM_F32_INV_NORM: r = inv_norm(a[c]); break;
        case DM_F32_DIV_BY_RECIP: r = div_by_recip<false>(a[c], b[c], y[c]); break;
        case DM_F32_DIV_BY_RECIP_SIGNED: r = div_by_recip_signed(a[c], b[c], y[c]); break;
        case DM_F32_FDIV_NR: r = fdiv_nr(a[c], b[c]); break;
        case DM_F32_FDIV_ONE_NR: r = fdiv_one_nr(b[c]); break;
        default: r = fmin_nan_drop(a[c], b[c]); break;
        }
        if (i < n_cases)
            out[i] = r;
    }
}

__global__ void __launch_bounds__(DM_BLOCK) dm_f64_div_kernel(int which, const double *a, const double *b, const double *y, double *out,
                                                             size_t n_cases)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n_cases; i += stride)
        out[i] = which == DM_F64_DIV_BY_RECIP ? div_by_recip<false>(a[i], b[i], y[i]) : div_by_recip<true>(a[i], b[i], y[i]);
}

// ---- host side -------------------------------------------------------------------------------------------------------
// device buffers of one call: freed when the call returns, whatever it returns
struct Bufs {
    void *p[8];
    int n = 0;
    ~Bufs() { (void) release(); } // (only on the early returns, where the call already reports an earlier error)
    // frees every buffer; the first error of the frees, or st if the call had failed before
    int release(int st)
    {
        const int fr = release();
        return st ? st : fr;
    }
    int release()
    {
        int first = 0;
        for (int i = 0; i < n; i++) {
            const hipError_t e = hipFree(p[i]);
            if (e != hipSuccess && !first)
                first = (int) e;
        }
        n = 0;
        return first;
    }
    hipError_t in(void **d, const void *h, size_t bytes)
    {
        hipError_t e = out(d, bytes);
        if (e == hipSuccess && bytes)
            e = hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
        return e;
    }
    hipError_t out(void **d, size_t bytes)
    {
        *d = nullptr;
        if (n >= 8)
            return hipErrorOutOfMemory;
        hipError_t e = hipMalloc(d, bytes ? bytes : 1);
        if (e == hipSuccess)
            p[n++] = *d;
        return e;
    }
};

#define DM_TRY(expr)                  \
    do {                              \
        const hipError_t e_ = (expr); \
        if (e_ != hipSuccess)         \
            return (int) e_;          \
    } while (0)

unsigned grid_for(size_t items)
{
    const size_t blocks = (items + DM_BLOCK - 1) / DM_BLOCK;
    return (unsigned) (blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks)); // beyond that the grid-stride loop takes over
}

int finish(void *host, const void *dev, size_t bytes)
{
    DM_TRY(hipGetLastError());
    DM_TRY(hipDeviceSynchronize());
    if (bytes)
        DM_TRY(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// the four axes of a seed profile in ONE device buffer [x0 | f0 | x1 | f1 | ...]; the frequency axis stays empty (neither
// seed_factor nor rt_seed_tab_kernel reads it)
int seed_tables(Bufs &B, DevSeed &sd, const int *dim, const double *const *xs, const double *const *fs, double f0)
{
    size_t total = 0;
    for (int d = 0; d < 4; d++) {
        if (dim[d] < 2 || !xs[d] || !fs[d])
            return (int) hipErrorInvalidValue;
        total += 2 * (size_t) dim[d];
    }
    double *tab;
    DM_TRY(B.out((void **) &tab, total * sizeof(double)));
    size_t at = 0;
    for (int d = 0; d < 4; d++) {
        const size_t bytes = (size_t) dim[d] * sizeof(double);
        DM_TRY(hipMemcpy(tab + at, xs[d], bytes, hipMemcpyHostToDevice));
        DM_TRY(hipMemcpy(tab + at + dim[d], fs[d], bytes, hipMemcpyHostToDevice));
        sd.x[d]   = tab + at;
        sd.f[d]   = tab + at + dim[d];
        sd.dim[d] = dim[d];
        at += 2 * (size_t) dim[d];
    }
    sd.x[4] = sd.f[4] = nullptr;
    sd.dim[4]         = 0;
    sd.pad            = 0;
    sd.f0             = f0;
    return 0;
}

} // namespace

#define DM_API extern "C" __attribute__((visibility("default")))

DM_API const char *rt_devmath_error(int status) { return hipGetErrorString((hipError_t) status); }

DM_API int rt_devmath_vec(void) { return rt::VEC; }

// out[1024]: [first work-group: tab[0..256), tab2[0..256)][last work-group: the same], n_blocks >= 1 work-groups launched
DM_API int rt_devmath_tables(double *out, unsigned n_blocks)
{
    Bufs B;
    double *d;
    if (n_blocks < 1)
        n_blocks = 1;
    DM_TRY(B.out((void **) &d, 4 * EXP_TAB * sizeof(double)));
    DM_TRY(hipMemset(d, 0xff, 4 * EXP_TAB * sizeof(double)));
    dm_tables_kernel<<<n_blocks, DM_BLOCK>>>(d);
    return B.release(finish(out, d, 4 * EXP_TAB * sizeof(double)));
}

DM_API int rt_devmath_exp(int which, const double *x, double *out, size_t n)
{
    Bufs B;
    double *dx, *dout;
    if (which != DM_EXP_TAB && which != DM_EXP_TAB_VEC)
        return (int) hipErrorInvalidValue;
    DM_TRY(B.in((void **) &dx, x, n * sizeof(double)));
    DM_TRY(B.out((void **) &dout, n * sizeof(double)));
    dm_exp_kernel<<<grid_for(which == DM_EXP_TAB ? n : (n + VEC - 1) / VEC), DM_BLOCK>>>(which, dx, dout, n);
    return B.release(finish(out, dout, n * sizeof(double)));
}

DM_API int rt_devmath_update(const double *Iv, const float *gs, const float *es, const float *w, double *out, size_t n)
{
    Bufs B;
    double *dIv, *dout;
    float *dgs, *des, *dw;
    DM_TRY(B.in((void **) &dIv, Iv, n * sizeof(double)));
    DM_TRY(B.in((void **) &dgs, gs, n * sizeof(float)));
    DM_TRY(B.in((void **) &des, es, n * sizeof(float)));
    DM_TRY(B.in((void **) &dw, w, n * sizeof(float)));
    DM_TRY(B.out((void **) &dout, n * sizeof(double)));
    dm_update_kernel<<<grid_for(n), DM_BLOCK>>>(dIv, dgs, des, dw, dout, n);
    return B.release(finish(out, dout, n * sizeof(double)));
}

// Iv, w, out: [groups][VEC]; gs, rs: [groups]
DM_API int rt_devmath_step(int which, const double *Iv, const float *gs, const double *rs, const float *w, double *out, size_t groups)
{
    Bufs B;
    double *dIv, *drs, *dout;
    float *dgs, *dw;
    if (which != DM_STEP_F64 && which != DM_STEP_F32)
        return (int) hipErrorInvalidValue;
    DM_TRY(B.in((void **) &dIv, Iv, groups * VEC * sizeof(double)));
    DM_TRY(B.in((void **) &dgs, gs, groups * sizeof(float)));
    DM_TRY(B.in((void **) &drs, rs, groups * sizeof(double)));
    DM_TRY(B.in((void **) &dw, w, groups * VEC * sizeof(float)));
    DM_TRY(B.out((void **) &dout, groups * VEC * sizeof(double)));
    dm_step_kernel<<<grid_for(groups), DM_BLOCK>>>(which, dIv, dgs, drs, dw, dout, groups);
    return B.release(finish(out, dout, groups * VEC * sizeof(double)));
}

DM_API int rt_devmath_div(const double *a, const double *b, double *q, size_t n)
{
    Bufs B;
    double *da, *db, *dq;
    DM_TRY(B.in((void **) &da, a, n * sizeof(double)));
    DM_TRY(B.in((void **) &db, b, n * sizeof(double)));
    DM_TRY(B.out((void **) &dq, n * sizeof(double)));
    dm_div_kernel<<<grid_for(n), DM_BLOCK>>>(da, db, dq, n);
    return B.release(finish(q, dq, n * sizeof(double)));
}

// four axes: grid g[a] of n_grid[a] >= 1 points with spacing d[a]; v, idx: [n][4]
DM_API int rt_devmath_deposit(int which, const int *n_grid, const double *const *g, const double *d, const double *v, int *idx, size_t n)
{
    Bufs B;
    DmAxes X;
    double *dv;
    int *didx;
    if (which != DM_DEPOSIT_FAST && which != DM_DEPOSIT_4)
        return (int) hipErrorInvalidValue;
    for (int a = 0; a < 4; a++) {
        if (n_grid[a] < 1)
            return (int) hipErrorInvalidValue;
        double *dg;
        DM_TRY(B.in((void **) &dg, g[a], (size_t) n_grid[a] * sizeof(double)));
        X.n[a]     = n_grid[a];
        X.g[a]     = dg;
        X.d[a]     = d[a];
        X.inv_d[a] = 1.0 / d[a]; // as rt_hip_plan_create has it
        X.g0[a]    = g[a][0];
        X.gl[a]    = g[a][n_grid[a] - 1];
    }
    DM_TRY(B.in((void **) &dv, v, n * 4 * sizeof(double)));
    DM_TRY(B.out((void **) &didx, n * 4 * sizeof(int)));
    dm_deposit_kernel<<<grid_for(n), DM_BLOCK>>>(which, X, dv, didx, n);
    return B.release(finish(idx, didx, n * 4 * sizeof(int)));
}

DM_API int rt_devmath_tan(int which, const float *x, float *out, size_t n)
{
    Bufs B;
    float *dx, *dout;
    if (which != DM_TAN && which != DM_ATAN)
        return (int) hipErrorInvalidValue;
    DM_TRY(B.in((void **) &dx, x, n * sizeof(float)));
    DM_TRY(B.out((void **) &dout, n * sizeof(float)));
    dm_tan_kernel<<<grid_for(n), DM_BLOCK>>>(which, dx, dout, n);
    return B.release(finish(out, dout, n * sizeof(float)));
}

// one axis of a seed profile: xs, ys [n], n >= 2; x, y [m]
DM_API int rt_devmath_pchip(int n, const double *xs, const double *ys, const double *x, double *y, size_t m)
{
    Bufs B;
    double *dxs, *dys, *dx, *dy;
    if (n < 2)
        return (int) hipErrorInvalidValue;
    DM_TRY(B.in((void **) &dxs, xs, (size_t) n * sizeof(double)));
    DM_TRY(B.in((void **) &dys, ys, (size_t) n * sizeof(double)));
    DM_TRY(B.in((void **) &dx, x, m * sizeof(double)));
    DM_TRY(B.out((void **) &dy, m * sizeof(double)));
    dm_pchip_kernel<<<grid_for(m), DM_BLOCK>>>(n, dxs, dys, dx, dy, m);
    return B.release(finish(y, dy, m * sizeof(double)));
}

// the four axes xs[d], fs[d] [dim[d]], dim[d] >= 2; pts [m][4]; f [m]
DM_API int rt_devmath_seed_factor(const int *dim, const double *const *xs, const double *const *fs, double f0, const double *pts,
                                  double *f, size_t m)
{
    Bufs B;
    DevSeed sd;
    double *dpts, *df;
    const int st = seed_tables(B, sd, dim, xs, fs, f0);
    if (st)
        return st;
    DM_TRY(B.in((void **) &dpts, pts, m * 4 * sizeof(double)));
    DM_TRY(B.out((void **) &df, m * sizeof(double)));
    dm_seed_factor_kernel<<<grid_for(m), DM_BLOCK>>>(sd, dpts, df, m);
    return B.release(finish(f, df, m * sizeof(double)));
}

// one work-group: Iv [256][Kp], deposits [256] (0 / not 0), Kp a multiple of VEC up to 64; out [Kp]
DM_API int rt_devmath_ev_sum(const double *Iv, const unsigned char *deposits, double scale, int Kp, double *out)
{
    Bufs B;
    double *dIv, *dout;
    unsigned char *ddep;
    if (Kp < VEC || Kp > DM_EV_KP_MAX || Kp % VEC != 0)
        return (int) hipErrorInvalidValue;
    DM_TRY(B.in((void **) &dIv, Iv, (size_t) DM_BLOCK * Kp * sizeof(double)));
    DM_TRY(B.in((void **) &ddep, deposits, DM_BLOCK));
    DM_TRY(B.out((void **) &dout, (size_t) Kp * sizeof(double)));
    dm_ev_sum_kernel<<<1, DM_BLOCK>>>(dIv, ddep, scale, Kp, dout);
    return B.release(finish(out, dout, (size_t) Kp * sizeof(double)));
}

// one work-group: pix [256] in -1 .. n_pix - 1, val [256]; nf [n_pix]
DM_API int rt_devmath_nf_scan(const int *pix, const double *val, double scale, int n_pix, double *nf)
{
    Bufs B;
    int *dpix;
    double *dval, *dnf;
    if (n_pix < 1)
        return (int) hipErrorInvalidValue;
    for (int i = 0; i < DM_BLOCK; i++)
        if (pix[i] < -1 || pix[i] >= n_pix)
            return (int) hipErrorInvalidValue;
    DM_TRY(B.in((void **) &dpix, pix, DM_BLOCK * sizeof(int)));
    DM_TRY(B.in((void **) &dval, val, DM_BLOCK * sizeof(double)));
    DM_TRY(B.out((void **) &dnf, (size_t) n_pix * sizeof(double)));
    DM_TRY(hipMemset(dnf, 0, (size_t) n_pix * sizeof(double)));
    dm_nf_scan_kernel<<<1, DM_BLOCK>>>(dpix, dval, scale, dnf);
    return B.release(finish(nf, dnf, (size_t) n_pix * sizeof(double)));
}

// rt_seed_tab_kernel of rt_march.hip, unchanged, on a DevRays made of the four grids g[a] [n_grid[a]], n_grid[a] >= 1:
// sf, sin [n_grid[0] + ... + n_grid[3]].  n_blocks = 0: as many work-groups as the product launches, one thread per
// entry; otherwise that many, so that fewer of them walk the entries in the kernel's grid-stride loop
DM_API int rt_devmath_seed_tab(const int *dim, const double *const *xs, const double *const *fs, double f0, const int *n_grid,
                               const double *const *g, unsigned n_blocks, double *sf, unsigned char *sin)
{
    Bufs B;
    DevSeed sd;
    const int st = seed_tables(B, sd, dim, xs, fs, f0);
    if (st)
        return st;
    size_t nn = 0;
    for (int a = 0; a < 4; a++) {
        if (n_grid[a] < 1 || !g[a])
            return (int) hipErrorInvalidValue;
        nn += (size_t) n_grid[a];
    }
    if (nn > (size_t) 1 << 24)
        return (int) hipErrorInvalidValue;
    double *dg, *dsf;
    unsigned char *dsin;
    DM_TRY(B.out((void **) &dg, nn * sizeof(double)));
    DevRays R = {};
    const double **slot[4] = { &R.gx, &R.gy, &R.ga, &R.gb };
    size_t at = 0;
    for (int a = 0; a < 4; a++) {
        DM_TRY(hipMemcpy(dg + at, g[a], (size_t) n_grid[a] * sizeof(double), hipMemcpyHostToDevice));
        *slot[a] = dg + at;
        at += (size_t) n_grid[a];
    }
    R.ngx = n_grid[0];
    R.ngy = n_grid[1];
    R.nga = n_grid[2];
    R.ngb = n_grid[3];
    DM_TRY(B.out((void **) &dsf, nn * sizeof(double)));
    DM_TRY(B.out((void **) &dsin, nn));
    DM_TRY(hipMemset(dsf, 0xff, nn * sizeof(double))); // (an entry the kernel leaves out reads as NaN / 255)
    DM_TRY(hipMemset(dsin, 0xff, nn));
    const unsigned blocks = n_blocks ? n_blocks : (unsigned) ((nn + 255) / 256);
    rt::rt_seed_tab_kernel<<<blocks, 256>>>(sd, R, dsf, dsin);
    const int rc = finish(sf, dsf, nn * sizeof(double));
    if (rc)
        return B.release(rc);
    DM_TRY(hipMemcpy(sin, dsin, nn, hipMemcpyDeviceToHost));
    return B.release(0);
}

// One integrator step of the march per case (rt_march_step.inc), in the instance (bounded, opt) -- one of the four the
// product launches: (0, 0), (1, 0), (1, PRUNE | NO_NTEST), (1, PRUNE | NO_NTEST | PRUNE_H24); anything else is refused.
// c: the step factor (rt_hip_plan_set_step_factor).  in [n][14], out [n][8], run [n] as dm_march_step_kernel says;
// counters [6]: waves of this launch that took prune(0 .. 3), the tiny-dividend block, and all waves
DM_API int rt_devmath_march_step(int bounded, int opt, float c, const float *in, float *out, unsigned char *run, unsigned *counters,
                                 size_t n)
{
    Bufs B;
    float *din, *dout;
    unsigned char *drun;
    unsigned *dcnt;
    constexpr int PN = MARCH_OPT_PRUNE | MARCH_OPT_NO_NTEST, PN24 = PN | MARCH_OPT_PRUNE_H24;
    if (!((opt == 0) || (bounded && (opt == PN || opt == PN24))) || n < 1)
        return (int) hipErrorInvalidValue;
    const DmStepFactors P = { c * 1.00001f, c * 0.1f, c * 0.05f };
    DM_TRY(B.in((void **) &din, in, n * DM_STEP_IN * sizeof(float)));
    DM_TRY(B.out((void **) &dout, n * DM_STEP_OUT * sizeof(float)));
    DM_TRY(B.out((void **) &drun, n));
    DM_TRY(B.out((void **) &dcnt, DM_STEP_COUNTERS * sizeof(unsigned)));
    DM_TRY(hipMemset(dcnt, 0, DM_STEP_COUNTERS * sizeof(unsigned)));
    const unsigned grid = grid_for(n);
    if (!bounded)
        dm_march_step_kernel<false, 0><<<grid, DM_BLOCK>>>(P, din, dout, drun, dcnt, n);
    else if (opt == 0)
        dm_march_step_kernel<true, 0><<<grid, DM_BLOCK>>>(P, din, dout, drun, dcnt, n);
    else if (opt == PN)
        dm_march_step_kernel<true, PN><<<grid, DM_BLOCK>>>(P, din, dout, drun, dcnt, n);
    else
        dm_march_step_kernel<true, PN24><<<grid, DM_BLOCK>>>(P, din, dout, drun, dcnt, n);
    const int rc = finish(out, dout, n * DM_STEP_OUT * sizeof(float));
    if (rc)
        return B.release(rc);
    DM_TRY(hipMemcpy(run, drun, n, hipMemcpyDeviceToHost));
    DM_TRY(hipMemcpy(counters, dcnt, DM_STEP_COUNTERS * sizeof(unsigned), hipMemcpyDeviceToHost));
    return B.release(0);
}

// The cross-cell set-up of the march per case (rt_march_xsetup.inc): fin [n][4], din [n][8], mirror [n], out [n][3] as
// dm_march_xsetup_kernel says
static int march_xsetup(bool bounded, const float *fin, const double *din, const unsigned char *mirror, float *out, size_t n)
{
    Bufs B;
    float *dfin, *dout;
    double *ddin;
    unsigned char *dmir;
    if (n < 1)
        return (int) hipErrorInvalidValue;
    DM_TRY(B.in((void **) &dfin, fin, n * 4 * sizeof(float)));
    DM_TRY(B.in((void **) &ddin, din, n * 8 * sizeof(double)));
    DM_TRY(B.in((void **) &dmir, mirror, n));
    DM_TRY(B.out((void **) &dout, n * 3 * sizeof(float)));
    if (bounded)
        dm_march_xsetup_kernel<true><<<grid_for(n), DM_BLOCK>>>(dfin, ddin, dmir, dout, n);
    else
        dm_march_xsetup_kernel<false><<<grid_for(n), DM_BLOCK>>>(dfin, ddin, dmir, dout, n);
    return B.release(finish(out, dout, n * 3 * sizeof(float)));
}
// ... in the generic instance, for any tables,
DM_API int rt_devmath_march_xsetup(const float *fin, const double *din, const unsigned char *mirror, float *out, size_t n)
{
    return march_xsetup(false, fin, din, mirror, out, n);
}
// ... and in the BOUNDED one: the cases must lie inside the ranges under which the plan selects it (rt_plan.hip)
DM_API int rt_devmath_march_xsetup_bounded(const float *fin, const double *din, const unsigned char *mirror, float *out, size_t n)
{
    return march_xsetup(true, fin, din, mirror, out, n);
}

// The march blob of the tables gain[1 .. N-1] (gain[0] is not read) as rt_hip_plan_create packs it: the same function,
// rt_blob_pack.h.  Host code only -- no device is touched.  Tables that rt_hip_plan_create refuses (a grid not strictly
// increasing or with a spacing below 1e-30, an index not finite as a float) are refused here.
static int pack_march_blob(int N, const rt_gain *gain, std::vector<unsigned char> &blob)
{
    if (N < 2 || !gain)
        return (int) hipErrorInvalidValue;
    for (int i = 1; i < N; i++)
        if (gain[i].Nx < 2 || gain[i].Ny < 2 || !gain[i].x || !gain[i].y || !gain[i].n || !gain[i].g0)
            return (int) hipErrorInvalidValue;
    blob.assign((sizeof(BlobGain) * (size_t) N + 15) / 16 * 16, 0);
    bool tiny_spacing = false, bad_index = false;
    for (int i = 1; i < N; i++)
        (void) blob_pack_length(blob, (size_t) i, gain[i].Nx, gain[i].Ny, gain[i].x, gain[i].y, gain[i].n, gain[i].g0, gain[i].E0,
                                tiny_spacing, bad_index);
    return tiny_spacing || bad_index ? (int) hipErrorInvalidValue : 0;
}

// every record a case of length i can reach lies inside the blob: the header's counts and offsets against its size
static bool blob_length_in_bounds(const std::vector<unsigned char> &blob, int i)
{
    BlobGain h;
    memcpy(&h, blob.data() + sizeof(BlobGain) * (size_t) i, sizeof(h));
    const size_t size = blob.size();
    auto inside       = [size](int off, size_t bytes) { return off >= 0 && off % 16 == 0 && (size_t) off <= size && bytes <= size - (size_t) off; };
    return h.Nx >= 2 && h.Ny >= 2 && inside(h.off_ix, sizeof(Interval) * (size_t) h.Nx) &&
           inside(h.off_iy, sizeof(Interval) * (size_t) h.Ny) && inside(h.off_node, sizeof(Node) * (size_t) h.Nx * (size_t) h.Ny);
}

// the blob itself, for the host-side tests of its records: *bytes = its size; copied to out when out != NULL and cap suffices
DM_API int rt_devmath_march_blob(int N, const rt_gain *gain, unsigned char *out, size_t cap, size_t *bytes)
{
    std::vector<unsigned char> blob;
    const int rc = pack_march_blob(N, gain, blob);
    if (rc || !bytes)
        return rc ? rc : (int) hipErrorInvalidValue;
    *bytes = blob.size();
    if (out) {
        if (cap < blob.size())
            return (int) hipErrorInvalidValue;
        memcpy(out, blob.data(), blob.size());
    }
    return 0;
}

// The escape test and the cell set-up of the march per case (rt_march_cell.inc), on the march blob of gain[1 .. N-1]; lds_tab:
// the instance that gathers from LDS.  fin [n][5], len [n], iout [n][8], fout [n][21], dout [n][8] as dm_march_cell_kernel says.
// Nothing is launched unless every len names a length of the blob, every offset of the headers lies inside it and (lds_tab)
// the blob fits the LDS a work-group may have.
DM_API int rt_devmath_march_cell(int lds_tab, int N, const rt_gain *gain, int use_emis, const float *fin, const int *len, size_t n,
                                 int *iout, float *fout, double *dout)
{
    std::vector<unsigned char> blob;
    int rc = pack_march_blob(N, gain, blob);
    if (rc)
        return rc;
    if (n < 1 || !fin || !len || !iout || !fout || !dout || blob.size() % 16 != 0 || blob.size() >= (1ull << 31))
        return (int) hipErrorInvalidValue;
    for (int i = 1; i < N; i++)
        if (!blob_length_in_bounds(blob, i) || (use_emis && !gain[i].E0))
            return (int) hipErrorInvalidValue;
    for (size_t c = 0; c < n; c++)
        if (len[c] < 1 || len[c] >= N)
            return (int) hipErrorInvalidValue;
    if (lds_tab) {
        int dev = 0, limit = 0;
        DM_TRY(hipGetDevice(&dev));
        DM_TRY(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
        if (limit < 1 || blob.size() > (size_t) limit)
            return (int) hipErrorInvalidValue;
        DM_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(dm_march_cell_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, limit));
    }
    Bufs B;
    unsigned char *dblob;
    float *dfin, *dfout;
    int *dlen, *diout;
    double *ddout;
    DM_TRY(B.in((void **) &dblob, blob.data(), blob.size()));
    DM_TRY(B.in((void **) &dfin, fin, n * DM_CELL_IN * sizeof(float)));
    DM_TRY(B.in((void **) &dlen, len, n * sizeof(int)));
    DM_TRY(B.out((void **) &diout, n * DM_CELL_I * sizeof(int)));
    DM_TRY(B.out((void **) &dfout, n * DM_CELL_F * sizeof(float)));
    DM_TRY(B.out((void **) &ddout, n * DM_CELL_D * sizeof(double)));
    if (lds_tab)
        dm_march_cell_kernel<true><<<grid_for(n), DM_BLOCK, blob.size()>>>(dblob, (unsigned) blob.size(), use_emis, dfin, dlen, diout, dfout, ddout, n);
    else
        dm_march_cell_kernel<false><<<grid_for(n), DM_BLOCK>>>(dblob, (unsigned) blob.size(), use_emis, dfin, dlen, diout, dfout, ddout, n);
    rc = finish(iout, diout, n * DM_CELL_I * sizeof(int));
    if (rc)
        return B.release(rc);
    DM_TRY(hipMemcpy(fout, dfout, n * DM_CELL_F * sizeof(float), hipMemcpyDeviceToHost));
    DM_TRY(hipMemcpy(dout, ddout, n * DM_CELL_D * sizeof(double), hipMemcpyDeviceToHost));
    return B.release(0);
}

// a float primitive of rt_math.h elementwise: which = 0 inv_norm(a), 1 div_by_recip(a, b, y), 2 div_by_recip_signed(a, b, y),
// 3 fdiv_nr(a, b), 4 fdiv_one_nr(b), 5 fmin_nan_drop(a, b); all three arrays hold n values whichever the primitive reads
DM_API int rt_devmath_f32(int which, const float *a, const float *b, const float *y, float *out, size_t n)
{
    Bufs B;
    float *da, *db, *dy, *dout;
    if (which < DM_F32_INV_NORM || which > DM_F32_FMIN_NAN_DROP || n < 1)
        return (int) hipErrorInvalidValue;
    DM_TRY(B.in((void **) &da, a, n * sizeof(float)));
    DM_TRY(B.in((void **) &db, b, n * sizeof(float)));
    DM_TRY(B.in((void **) &dy, y, n * sizeof(float)));
    DM_TRY(B.out((void **) &dout, n * sizeof(float)));
    dm_f32_kernel<<<grid_for(n), DM_BLOCK>>>(which, da, db, dy, dout, n);
    return B.release(finish(out, dout, n * sizeof(float)));
}

// the double div_by_recip(a, b, y) elementwise: which = 0 the guarded form, 1 TINY_OK
DM_API int rt_devmath_f64_div(int which, const double *a, const double *b, const double *y, double *out, size_t n)
{
    Bufs B;
    double *da, *db, *dy, *dout;
    if (which != DM_F64_DIV_BY_RECIP && which != DM_F64_DIV_BY_RECIP_TINY_OK)
        return (int) hipErrorInvalidValue;
    DM_TRY(B.in((void **) &da, a, n * sizeof(double)));
    DM_TRY(B.in((void **) &db, b, n * sizeof(double)));
    DM_TRY(B.in((void **) &dy, y, n * sizeof(double)));
    DM_TRY(B.out((void **) &dout, n * sizeof(double)));
    dm_f64_div_kernel<<<grid_for(n), DM_BLOCK>>>(which, da, db, dy, dout, n);
    return B.release(finish(out, dout, n * sizeof(double)));
}
