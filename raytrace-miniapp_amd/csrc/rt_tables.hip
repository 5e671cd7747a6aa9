// rt_tables.hip -- the gain tables of a resident plan rewritten in place, scanned and packed on the device
// (rt_hip_plan_update_gain, rt_hip_plan_update_gain_dev, rt_hip_plan_table_flags).
//
// rt_hip_plan_create packs the tables on the host (rt_plan.hip) and derives four facts from them that every run is
// chosen by: tables_bounded, ntest_proven, gv_has_nan and gs_cap.  A time loop has new n, g0, E0 and gv on the same
// grids at every step; this unit rewrites the two mutable parts of the arena -- Node[Nx * Ny] of every length inside
// the march blob and the lineshape rows -- and recomputes the four facts, in this order:
//   settle   the plan's last run is waited for and, where rays failed with -2 / -3, repeated, before a byte changes
//   scan     rt_table_scan_kernel reads the RAW tables: min n, max n, the largest neighbour difference dn, a flag for a
//            non-finite n, and (emission mode) the integer maximum of the magnitude bits of gv; the host waits for it
//   validate a non-finite index of refraction rejects the update: the integrator would never advance on it
//            (Helper.h:279-280), which on a GPU is a hung device.  No table has been touched at that point
//   pack     rt_table_pack_kernel writes the nodes and the rows; an event is recorded behind it, which the next
//            rt_hip_plan_run waits for on whatever queue it runs
// Every figure of the scan is a minimum or a maximum of values that are computed per element with one IEEE operation
// (or none): exact and independent of the order, so the summary has the bits of the host loops of rt_hip_plan_create
// (rt_plan.hip, "Ranges for the short division sequences" and the lineshape scan), and so have the four facts.
// A translation unit of its own: no kernel of rt_launch.hip is compiled differently for it.
#include "rt_runtime.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace rtr;

namespace rt {

// One length of an update, read by both kernels.  Work-groups [scan_n0, scan_gv0) of the scan launch take the nodes of
// the length, [scan_gv0, scan_end) its lineshape values; [pack_n0, pack_gv0) and [pack_gv0, pack_end) of the pack
// launch likewise.  The work-groups of a range stride over its items together.
struct TabDesc {
    const double *n;  // [cells]
    const float *g0;  // [cells]
    const float *E0;  // [cells] or NULL: packs as zeros
    const float *gv;  // [cells][K], tight
    Node *node_dst;   // [cells] inside the march blob
    float *gv_dst;    // [cells][Kp] in the arena
    unsigned cells, Nx, K, Kp;
    unsigned scan_n0, scan_gv0, scan_end;
    unsigned pack_n0, pack_gv0, pack_end;
    unsigned gv_vec;  // K == Kp and gv is aligned to 16 bytes: rows are copied 16 bytes per lane
    unsigned pad;
};

// What one work-group of the scan found (folded by the host: minima and maxima, no order enters)
struct TabPart {
    double n_lo, n_hi, dn;
    unsigned gv_finite, gv_all; // largest magnitude bits below infinity / of everything
    unsigned bad_n;             // some n is a NaN or an infinity as a float (a double beyond the largest float included)
    unsigned length;
};

constexpr int TAB_WG = 256;

__device__ inline double wave_min(double v)
{
    for (int m = WAVE / 2; m > 0; m >>= 1)
        v = fmin(v, __shfl_xor(v, m, WAVE));
    return v;
}
__device__ inline double wave_max(double v)
{
    for (int m = WAVE / 2; m > 0; m >>= 1)
        v = fmax(v, __shfl_xor(v, m, WAVE));
    return v;
}
__device__ inline unsigned wave_umax(unsigned v)
{
    for (int m = WAVE / 2; m > 0; m >>= 1) {
        const unsigned o = (unsigned) __shfl_xor((int) v, m, WAVE);
        v                = o > v ? o : v;
    }
    return v;
}

// the length whose range of work-groups holds wg (ranges are consecutive; at most 64 lengths)
__device__ inline int tab_length_of(const TabDesc *d, int N, unsigned wg, bool pack)
{
    int i = 1;
    while (i < N - 1 && wg >= (pack ? d[i].pack_end : d[i].scan_end))
        i++;
    return i;
}

extern "C" __global__ void __launch_bounds__(TAB_WG) rt_table_scan_kernel(const TabDesc *desc, int N, TabPart *part)
{
    __shared__ TabPart s_part[TAB_WG / WAVE];
    const unsigned wg = blockIdx.x, tid = threadIdx.x;
    const int i       = tab_length_of(desc, N, wg, false);
    const TabDesc d   = desc[i];
    // (fmin / fmax skip a NaN; a table with one is rejected whatever the ranges say)
    double n_lo = INFINITY, n_hi = -INFINITY, dn = 0.0;
    unsigned gfin = 0, gall = 0, bad = 0;
    if (wg < d.scan_gv0) {
        const unsigned stride = (d.scan_gv0 - d.scan_n0) * TAB_WG;
        for (unsigned c = (wg - d.scan_n0) * TAB_WG + tid; c < d.cells; c += stride) {
            const double v = d.n[c];
            // (not finite as the float the march rounds it to, rt_march_cell.inc: rt_hip_plan_create's test, rt_blob_pack.h --
            // inf, NaN, and a double beyond the largest float, which rounds to inf)
            bad |= (__float_as_uint((float) v) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
            n_lo = fmin(n_lo, v);
            n_hi = fmax(n_hi, v);
            // horizontal and vertical neighbours: column 0 has no horizontal one (c - 1 is the previous row's last node)
            if (c % d.Nx != 0)
                dn = fmax(dn, fabs(v - d.n[c - 1]));
            if (c >= d.Nx)
                dn = fmax(dn, fabs(v - d.n[c - d.Nx]));
        }
    } else {
        const unsigned long long count = (unsigned long long) d.cells * d.K;
        const unsigned long long stride = (unsigned long long) (d.scan_end - d.scan_gv0) * TAB_WG;
        const unsigned *u               = reinterpret_cast<const unsigned *>(d.gv);
        for (unsigned long long c = (unsigned long long) (wg - d.scan_gv0) * TAB_WG + tid; c < count; c += stride) {
            unsigned a = u[c] & 0x7fffffffu;
            gall       = a > gall ? a : gall;
            a          = a < 0x7f800000u ? a : 0u; // inf and NaN do not count
            gfin       = a > gfin ? a : gfin;
        }
    }
    n_lo = wave_min(n_lo);
    n_hi = wave_max(n_hi);
    dn   = wave_max(dn);
    gfin = wave_umax(gfin);
    gall = wave_umax(gall);
    bad  = wave_umax(bad);
    if ((tid & (WAVE - 1)) == 0)
        s_part[tid / WAVE] = TabPart{ n_lo, n_hi, dn, gfin, gall, bad, (unsigned) i };
    __syncthreads();
    if (tid == 0) {
        TabPart r = s_part[0];
        for (int w = 1; w < TAB_WG / WAVE; w++) {
            const TabPart o = s_part[w];
            r.n_lo          = fmin(r.n_lo, o.n_lo);
            r.n_hi          = fmax(r.n_hi, o.n_hi);
            r.dn            = fmax(r.dn, o.dn);
            r.gv_finite     = o.gv_finite > r.gv_finite ? o.gv_finite : r.gv_finite;
            r.gv_all        = o.gv_all > r.gv_all ? o.gv_all : r.gv_all;
            r.bad_n |= o.bad_n;
        }
        part[wg] = r;
    }
}

extern "C" __global__ void __launch_bounds__(TAB_WG) rt_table_pack_kernel(const TabDesc *desc, int N)
{
    const unsigned wg = blockIdx.x, tid = threadIdx.x;
    const int i       = tab_length_of(desc, N, wg, true);
    const TabDesc d   = desc[i];
    if (wg < d.pack_gv0) {
        // Node{n, g0, E0}: one node per lane, one 16-byte store
        const unsigned stride = (d.pack_gv0 - d.pack_n0) * TAB_WG;
        for (unsigned c = (wg - d.pack_n0) * TAB_WG + tid; c < d.cells; c += stride) {
            Node nd;
            nd.n          = d.n[c];
            nd.g0         = d.g0[c];
            nd.E0         = d.E0 ? d.E0[c] : 0.0f;
            d.node_dst[c] = nd;
        }
    } else {
        // rows of Kp floats from rows of K: four columns per lane (Kp is a multiple of four, so the four belong to one row)
        const unsigned q_row            = d.Kp / 4;
        const unsigned long long count  = (unsigned long long) d.cells * q_row;
        const unsigned long long stride = (unsigned long long) (d.pack_end - d.pack_gv0) * TAB_WG;
        float4 *dst                     = reinterpret_cast<float4 *>(d.gv_dst);
        for (unsigned long long q = (unsigned long long) (wg - d.pack_gv0) * TAB_WG + tid; q < count; q += stride) {
            float4 v;
            if (d.gv_vec) {
                v = reinterpret_cast<const float4 *>(d.gv)[q];
            } else {
                const unsigned long long row = q / q_row;
                const unsigned col           = (unsigned) (q - row * q_row) * 4;
                const float *src             = d.gv + row * d.K + col;
                v.x                          = src[0]; // (col < K always: Kp - K < 4)
                v.y                          = col + 1 < d.K ? src[1] : 0.0f;
                v.z                          = col + 2 < d.K ? src[2] : 0.0f;
                v.w                          = col + 3 < d.K ? src[3] : 0.0f;
            }
            dst[q] = v;
        }
    }
}

} // namespace rt

namespace {

unsigned groups_for(unsigned long long items)
{
    // enough work-groups to fill the device on a large table, one on a small one; the count bounds the partials
    const unsigned long long g = (items + (unsigned long long) rt::TAB_WG * 16 - 1) / ((unsigned long long) rt::TAB_WG * 16);
    return (unsigned) std::min<unsigned long long>(std::max<unsigned long long>(g, 1), 256);
}

// device memory of the plan's device that holds [ptr, ptr + bytes)
bool on_plan_device(const rt_hip_plan *p, const void *ptr, size_t bytes, size_t align)
{
    if (reinterpret_cast<uintptr_t>(ptr) % align)
        return false;
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
        (void) hipGetLastError(); // (a plain host pointer is an error to the runtime, not a type)
        return false;
    }
    if (at.type != hipMemoryTypeDevice || at.device != p->device)
        return false;
    hipDeviceptr_t base = nullptr;
    size_t size         = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(ptr)) != hipSuccess) {
        (void) hipGetLastError(); // (no range to compare with: the type and the device have been checked)
        return true;
    }
    const uintptr_t b = reinterpret_cast<uintptr_t>(base), q = reinterpret_cast<uintptr_t>(ptr);
    return q >= b && q - b <= size && bytes <= size - (q - b);
}

// scan -> validate -> pack on `stream`, from device pointers that have been checked (or are the call's own scratch)
int update_from_device(rt_hip_plan *p, const rt_gain_values *vals, hipStream_t stream)
{
    const int N   = p->P.N;
    const bool gv_scan = p->P.use_emis != 0; // (the lineshape scan of rt_hip_plan_create runs in emission mode only)
    // an earlier update may still be packing, on another queue
    if (p->tab_pending)
        HIP_TRY(hipStreamWaitEvent(stream, p->tab_ev, 0));
    // descriptors and the ranges of work-groups
    std::vector<rt::TabDesc> desc((size_t) N);
    memset(desc.data(), 0, sizeof(rt::TabDesc) * (size_t) N);
    unsigned scan_wg = 0, pack_wg = 0;
    for (int i = 1; i < N; i++) {
        const rt_hip_plan::TableShape &s = p->tab[(size_t) i];
        rt::TabDesc &d                   = desc[(size_t) i];
        d.n        = vals[i].n;
        d.g0       = vals[i].g0;
        d.E0       = vals[i].E0;
        d.gv       = vals[i].gv;
        d.node_dst = reinterpret_cast<rt::Node *>(const_cast<unsigned char *>(p->P.blob) + s.off_node);
        d.gv_dst   = const_cast<float *>(p->gv_dev[(size_t) i]);
        d.cells    = (unsigned) ((size_t) s.Nx * (size_t) s.Ny);
        d.Nx       = (unsigned) s.Nx;
        d.K        = (unsigned) p->P.K;
        d.Kp       = (unsigned) p->P.Kp;
        d.gv_vec   = (d.K == d.Kp && reinterpret_cast<uintptr_t>(d.gv) % 16 == 0) ? 1u : 0u;
        d.scan_n0  = scan_wg;
        scan_wg += groups_for(d.cells);
        d.scan_gv0 = scan_wg;
        if (gv_scan)
            scan_wg += groups_for((unsigned long long) d.cells * d.K);
        d.scan_end = scan_wg;
        d.pack_n0  = pack_wg;
        pack_wg += groups_for(d.cells);
        d.pack_gv0 = pack_wg;
        pack_wg += groups_for((unsigned long long) d.cells * (d.Kp / 4));
        d.pack_end = pack_wg;
    }
    // one page-locked block [descriptors | partials] and its device twin, kept with the plan
    const size_t desc_bytes = align_up(sizeof(rt::TabDesc) * (size_t) N, 256), part_bytes = sizeof(rt::TabPart) * (size_t) scan_wg;
    const size_t work_bytes = desc_bytes + part_bytes;
    if (p->tab_work_bytes < work_bytes) {
        if (p->tab_pending && hipEventSynchronize(p->tab_ev) != hipSuccess) // (the pack that reads the old block)
            (void) hipGetLastError();
        pool_free(p->device, p->tab_work);
        pinned_free(p->tab_pin);
        p->tab_work       = nullptr;
        p->tab_pin        = nullptr;
        p->tab_work_bytes = 0;
        HIP_TRY(pool_alloc(p->device, (void **) &p->tab_work, work_bytes));
        void *h = nullptr;
        HIP_TRY(pinned_alloc(&h, work_bytes));
        p->tab_pin        = static_cast<unsigned char *>(h);
        p->tab_work_bytes = work_bytes;
    }
    memcpy(p->tab_pin, desc.data(), sizeof(rt::TabDesc) * (size_t) N);
    const rt::TabDesc *desc_dev = reinterpret_cast<const rt::TabDesc *>(p->tab_work);
    rt::TabPart *part_dev       = reinterpret_cast<rt::TabPart *>(p->tab_work + desc_bytes);
    const rt::TabPart *part     = reinterpret_cast<const rt::TabPart *>(p->tab_pin + desc_bytes);
    if (!p->tab_ev)
        HIP_TRY(hipEventCreate(&p->tab_ev));
    // RT_HIP_TIMING=1: device time of the two kernels on stderr (diagnostic; waits for the pack)
    const bool timing = getenv("RT_HIP_TIMING") != nullptr;
    if (timing)
        for (hipEvent_t &e : p->tab_t)
            if (!e)
                HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipMemcpyAsync(p->tab_work, p->tab_pin, desc_bytes, hipMemcpyHostToDevice, stream));
    if (timing)
        HIP_TRY(hipEventRecord(p->tab_t[0], stream));
    hipLaunchKernelGGL(rt::rt_table_scan_kernel, dim3(scan_wg), dim3(rt::TAB_WG), 0, stream, desc_dev, N, part_dev);
    HIP_TRY(hipGetLastError());
    if (timing)
        HIP_TRY(hipEventRecord(p->tab_t[1], stream));
    HIP_TRY(hipMemcpyAsync(p->tab_pin + desc_bytes, part_dev, part_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream)); // the one wait of an update: the summary decides whether anything is written
    // ---- fold and validate: rt_hip_plan_create's tests on the same figures ----
    bool all_bounded = true, ntest_proven = true, gv_nan = false;
    uint32_t umax = 0;
    for (int i = 1; i < N; i++) {
        const rt_hip_plan::TableShape &s = p->tab[(size_t) i];
        const rt::TabDesc &d             = desc[(size_t) i];
        double n_lo = INFINITY, n_hi = -INFINITY, dn = 0.0;
        for (unsigned w = d.scan_n0; w < d.scan_gv0; w++) {
            if (part[w].bad_n)
                return fail_arg("rt_hip_plan_update_gain: non-finite index of refraction");
            n_lo = std::min(n_lo, part[w].n_lo);
            n_hi = std::max(n_hi, part[w].n_hi);
            dn   = std::max(dn, part[w].dn);
        }
        for (unsigned w = d.scan_gv0; w < d.scan_end; w++) {
            umax = std::max(umax, part[w].gv_finite);
            if (part[w].gv_all >= 0x7f800000u)
                gv_nan = true;
        }
        if (!(n_lo - dn >= 0.25 && n_hi + dn <= 4.0 && dn / s.w_min <= 1e12 && s.w_min >= 1e-12))
            all_bounded = false;
        if (!(8.0 * 0.1 * (1.2 + s.fy) * dn <= 0.05 - 1e-5))
            ntest_proven = false;
    }
    if (!p->dz_bounded)
        all_bounded = false;
    // ---- pack ----
    if (timing)
        HIP_TRY(hipEventRecord(p->tab_t[2], stream));
    hipLaunchKernelGGL(rt::rt_table_pack_kernel, dim3(pack_wg), dim3(rt::TAB_WG), 0, stream, desc_dev, N);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(p->tab_ev, stream));
    p->tab_pending = true; // rt_hip_plan_run waits for the event on its own queue
    if (timing) {
        float scan_ms = 0.0f, pack_ms = 0.0f;
        HIP_TRY(hipEventSynchronize(p->tab_ev));
        HIP_TRY(hipEventElapsedTime(&scan_ms, p->tab_t[0], p->tab_t[1]));
        HIP_TRY(hipEventElapsedTime(&pack_ms, p->tab_t[2], p->tab_ev));
        fprintf(stderr, "    plan_update scan %7.3f ms (%u work-groups)  pack %7.3f ms (%u work-groups)\n", scan_ms, scan_wg, pack_ms, pack_wg);
    }
    p->tables_bounded = all_bounded;
    p->ntest_proven   = all_bounded && ntest_proven;
    p->gv_has_nan     = gv_nan;
    float wmax        = 0.0f;
    memcpy(&wmax, &umax, sizeof(wmax));
    p->P.gs_cap = wmax > 0.0f ? 708.0f / wmax : FLT_MAX;
    if (!(p->P.gs_cap <= FLT_MAX))
        p->P.gs_cap = FLT_MAX;
    return RT_OK;
}

int check_args(rt_hip_plan *p, int N, const rt_gain_values *vals)
{
    if (!p || !vals)
        return fail_arg("rt_hip_plan_update_gain: NULL argument");
    if (N != p->P.N)
        return fail_arg("rt_hip_plan_update_gain: N differs from the plan's number of lengths");
    for (int i = 1; i < N; i++) {
        if (!vals[i].n || !vals[i].g0 || !vals[i].gv)
            return fail_arg("rt_hip_plan_update_gain: incomplete gain table");
        const size_t cells = (size_t) p->tab[(size_t) i].Nx * (size_t) p->tab[(size_t) i].Ny;
        if (cells * (size_t) p->P.Kp * sizeof(float) >= (1ull << 32))
            return fail_arg("rt_hip_plan_update_gain: a lineshape table of 4 GiB or more is not supported");
    }
    return RT_OK;
}

// the plan's last run becomes final before its tables change (what a fetch does first), uploads of the creation included
int settle_before_update(rt_hip_plan *p)
{
    HIP_TRY(hipSetDevice(p->device));
    if (p->staging && hipStreamSynchronize(p->upload_q) != hipSuccess)
        (void) hipGetLastError();
    plan_quiesce(p);
    return p->ran ? plan_settle_last_run(p) : (int) RT_OK;
}

} // namespace

extern "C" {

int rt_hip_plan_update_gain_dev(rt_hip_plan *p, int N, const rt_gain_values *vals, void *stream_v)
{
    int rc = check_args(p, N, vals);
    if (rc != RT_OK)
        return rc;
    HIP_TRY(hipSetDevice(p->device));
    for (int i = 1; i < N; i++) {
        const size_t cells = (size_t) p->tab[(size_t) i].Nx * (size_t) p->tab[(size_t) i].Ny;
        if (!on_plan_device(p, vals[i].n, cells * sizeof(double), sizeof(double)) ||
            !on_plan_device(p, vals[i].g0, cells * sizeof(float), sizeof(float)) ||
            (vals[i].E0 && !on_plan_device(p, vals[i].E0, cells * sizeof(float), sizeof(float))) ||
            !on_plan_device(p, vals[i].gv, cells * (size_t) p->P.K * sizeof(float), sizeof(float)))
            return fail_arg("rt_hip_plan_update_gain_dev: a table is not device memory of the plan's device (or misaligned, or too short)");
    }
    rc = settle_before_update(p);
    if (rc != RT_OK)
        return rc;
    return update_from_device(p, vals, reinterpret_cast<hipStream_t>(stream_v));
}

int rt_hip_plan_update_gain(rt_hip_plan *p, int N, const rt_gain_values *vals)
{
    int rc = check_args(p, N, vals);
    if (rc != RT_OK)
        return rc;
    rc = settle_before_update(p);
    if (rc != RT_OK)
        return rc;
    // the raw values travel into one scratch block; from there on this is the device call
    std::vector<rt_gain_values> dv((size_t) N);
    std::vector<size_t> off((size_t) N * 4, 0);
    size_t bytes = 0;
    for (int i = 1; i < N; i++) {
        const size_t cells = (size_t) p->tab[(size_t) i].Nx * (size_t) p->tab[(size_t) i].Ny;
        const size_t sz[4] = { cells * sizeof(double), cells * sizeof(float), vals[i].E0 ? cells * sizeof(float) : 0,
                               cells * (size_t) p->P.K * sizeof(float) };
        for (int t = 0; t < 4; t++) {
            off[(size_t) i * 4 + (size_t) t] = bytes;
            bytes += align_up(sz[t], 256);
        }
    }
    unsigned char *scratch = nullptr;
    HIP_TRY(pool_alloc(p->device, (void **) &scratch, bytes));
    hipStream_t q = lease_queue(p->device);
    rc            = [&]() {
        for (int i = 1; i < N; i++) {
            const size_t cells  = (size_t) p->tab[(size_t) i].Nx * (size_t) p->tab[(size_t) i].Ny;
            const size_t *o     = &off[(size_t) i * 4];
            const void *src[4]  = { vals[i].n, vals[i].g0, vals[i].E0, vals[i].gv };
            const size_t sz[4]  = { cells * sizeof(double), cells * sizeof(float), cells * sizeof(float), cells * (size_t) p->P.K * sizeof(float) };
            for (int t = 0; t < 4; t++)
                if (src[t])
                    HIP_TRY(hipMemcpyAsync(scratch + o[t], src[t], sz[t], hipMemcpyHostToDevice, q));
            dv[(size_t) i].n  = reinterpret_cast<const double *>(scratch + o[0]);
            dv[(size_t) i].g0 = reinterpret_cast<const float *>(scratch + o[1]);
            dv[(size_t) i].E0 = vals[i].E0 ? reinterpret_cast<const float *>(scratch + o[2]) : nullptr;
            dv[(size_t) i].gv = reinterpret_cast<const float *>(scratch + o[3]);
        }
        const int ru = update_from_device(p, dv.data(), q);
        if (ru != RT_OK)
            return ru;
        HIP_TRY(hipStreamSynchronize(q)); // the pack has read the scratch block
        return (int) RT_OK;
    }();
    if (rc != RT_OK && hipStreamSynchronize(q) != hipSuccess) // (whatever was queued still reads the scratch block)
        (void) hipGetLastError();
    pool_free(p->device, scratch);
    release_queue(p->device, q);
    return rc;
}

int rt_hip_plan_table_flags(rt_hip_plan *p, int *bounded, int *ntest_proven, int *gv_nonfinite, float *gs_cap)
{
    if (!p)
        return fail_arg("rt_hip_plan_table_flags: NULL plan");
    if (bounded)
        *bounded = p->tables_bounded ? 1 : 0;
    if (ntest_proven)
        *ntest_proven = p->ntest_proven ? 1 : 0;
    if (gv_nonfinite)
        *gv_nonfinite = p->gv_has_nan ? 1 : 0;
    if (gs_cap)
        *gs_cap = p->P.gs_cap;
    return RT_OK;
}

} // extern "C"
