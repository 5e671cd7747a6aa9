// rt_plan.hip -- the plan: one prepared problem on one device, and the host-pointer entry built on it.
//
// Replaces the host side of RayTraceImageCudaLoop (src/RayTraceImageCuda.cu:145-221) and of the
// copy_device helpers (src/RayTraceImageCuda.cu:224-329): where those issue ~30 cudaMalloc/cudaMemcpy
// calls per create_image, a plan packs every table into ONE arena, uploads it with ONE copy, zeroes
// outputs + control block and has rt_launch.hip put the march kernel and the frequency kernel back to back
// on one queue.  No data is cached across calls (Readme.txt:43); freed device allocations and the queues
// of a device are (rt_pool.hip).  Host code only.
#include "rt_runtime.h"
#include "rt_blob_pack.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>

using namespace rtr;

namespace {

// Bump allocator over the host image of a plan's arena: one buffer of a capacity computed up front (an upper bound, so nothing moves while the
// tables are copied in), page-locked when the upload is to run beside host work (rt_hip_image_loop), plain otherwise.
struct ArenaBuilder {
    unsigned char *base = nullptr;
    size_t cap = 0, used = 0;
    bool pinned = false, overflow = false;
    std::unique_ptr<unsigned char[]> own;
    ArenaBuilder() = default;
    ArenaBuilder(const ArenaBuilder &) = delete;
    ArenaBuilder &operator=(const ArenaBuilder &) = delete;
    ~ArenaBuilder()
    {
        if (pinned)
            rtr::pinned_free(base);
    }
    void start(size_t capacity, bool want_pinned)
    {
        cap = capacity;
        void *h = nullptr;
        if (want_pinned && rtr::pinned_alloc(&h, capacity) == hipSuccess) {
            base   = static_cast<unsigned char *>(h);
            pinned = true;
        } else {
            own.reset(new unsigned char[capacity]);
            base = own.get();
        }
    }
    // hands the page-locked buffer to the caller (who frees it with pinned_free once the upload has completed)
    void *release()
    {
        pinned = false;
        return base;
    }
    size_t reserve(size_t bytes) // zero-filled
    {
        const size_t off = rtr::align_up(used, 256);
        if (off + bytes > cap) {
            overflow = true;
            return 0;
        }
        memset(base + off, 0, bytes);
        used = off + bytes;
        return off;
    }
    size_t put(const void *src, size_t bytes)
    {
        const size_t off = rtr::align_up(used, 256);
        if (off + bytes > cap) {
            overflow = true;
            return 0;
        }
        if (bytes && src)
            memcpy(base + off, src, bytes);
        used = off + bytes;
        return off;
    }
};

// largest magnitude of n floats as bit patterns (non-negative floats order like their bit patterns): `finite` over the
// values below infinity, `all` over everything.  One pass that the compiler vectorises; the AVX2 instance is
// taken when the CPU has it (a plan of the shipped size scans 286 000 values on the critical path of every call).
template <int>
inline __attribute__((always_inline)) void magnitude_scan(const uint32_t *u, size_t n, uint32_t &finite, uint32_t &all)
{
    uint32_t m = 0, mall = 0;
    for (size_t c = 0; c < n; c++) {
        uint32_t a = u[c] & 0x7fffffffu;
        mall       = a > mall ? a : mall;
        a          = a < 0x7f800000u ? a : 0u; // inf and NaN do not count
        m          = a > m ? a : m;
    }
    finite = m;
    all    = mall;
}
// scan_on of a backward plan is the suffix scan (rt_runtime.h): the refusals name the scan that is on
bool suffix_scan(const rt_hip_plan *p) { return p->scan_on && p->P.method == 1; }

void magnitude_scan_plain(const uint32_t *u, size_t n, uint32_t &finite, uint32_t &all) { magnitude_scan<0>(u, n, finite, all); }
__attribute__((target("avx2"))) void magnitude_scan_avx2(const uint32_t *u, size_t n, uint32_t &finite, uint32_t &all)
{
    magnitude_scan<1>(u, n, finite, all);
}

} // namespace

// The kernels index rays with 32 bits; the march hands rays out in chunks of at most 4096 (the cap of
// RT_HIP_MARCH_CHUNK) and computes (rays of the launch + chunk - 1) / chunk in 32 bits.
const size_t rtr::MAX_LIST_RAYS = 0xffffffffull - 4096;

// Wait for the work of the plan's last run before any of its buffers is freed or parked in the pool:
// another plan may be handed a parked block at once (pool_alloc) and overwrite it.
void rtr::plan_quiesce(rt_hip_plan *p)
{
    history_wait(p); // an append of the step history, possibly on another queue, reads the records and the control block
    if (p && p->ran) {
        if (hipStreamSynchronize(p->last_stream) != hipSuccess)
            (void) hipGetLastError(); // a caller's stream that is gone: nothing is in flight on it
    }
    // a run that failed after its first enqueue (rt_hip_plan_run): zeroing kernel, memsets or march slices may still be
    // writing the plan's blocks on that queue
    if (p && p->queued && !(p->ran && p->queued_stream == p->last_stream)) {
        if (hipStreamSynchronize(p->queued_stream) != hipSuccess)
            (void) hipGetLastError();
    }
}

extern "C" {

int rt_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

const char *rt_hip_last_error(void) { return last_error().c_str(); }

int rt_hip_selftest(int device, unsigned long long *n_checked, unsigned long long *n_mismatch)
{
    if (!n_checked || !n_mismatch)
        return fail_arg("rt_hip_selftest: NULL argument");
    HIP_TRY(hipSetDevice(device));
    unsigned long long *d = nullptr, h[2] = { 0, 0 };
    HIP_TRY(hipMalloc((void **) &d, sizeof(h)));
    hipError_t e = hipMemset(d, 0, sizeof(h));
    if (e == hipSuccess && launch_selftest(d) != RT_OK)
        e = hipErrorLaunchFailure;
    if (e == hipSuccess)
        e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void) hipFree(d);
    HIP_TRY(e);
    *n_checked  = h[0];
    *n_mismatch = h[1];
    return RT_OK;
}

void rt_hip_plan_destroy(rt_hip_plan *p)
{
    if (!p)
        return;
    (void) hipSetDevice(p->device);
    plan_quiesce(p); // kernels of an unfetched (or failed) run may still use the buffers parked below
    if (p->staging) {
        if (hipStreamSynchronize(p->upload_q) != hipSuccess)
            (void) hipGetLastError();
        pinned_free(p->staging);
        p->staging = nullptr;
    }
    pinned_free(p->out_staging);
    p->out_staging = nullptr;
    if (p->ring.empty()) {
        if (p->ev0)
            (void) hipEventDestroy(p->ev0);
        if (p->ev1)
            (void) hipEventDestroy(p->ev1);
        if (p->evm)
            (void) hipEventDestroy(p->evm);
    }
    for (hipEvent_t e : p->ring) // (with a ring, ev0 / evm / ev1 alias one of its slots)
        (void) hipEventDestroy(e);
    if (p->tab_ev) { // the pack of a table update no run has waited for reads tab_work (rt_tables.hip)
        if (hipEventSynchronize(p->tab_ev) != hipSuccess)
            (void) hipGetLastError();
        (void) hipEventDestroy(p->tab_ev);
    }
    for (hipEvent_t e : p->tab_t)
        if (e)
            (void) hipEventDestroy(e);
    pool_free(p->device, p->tab_work);
    pinned_free(p->tab_pin);
    history_release(p);

    pool_free(p->device, p->tan_dev);
    pool_free(p->device, p->rec);
    (void) hipFree(p->path_dev);
    (void) hipFree(p->path_err);
    (void) hipFree(p->spec[0].Iv); // (ray2 and err of a set live in the same allocation)
    (void) hipFree(p->spec[1].Iv);
    pool_free(p->device, p->step_dev);
    pool_free(p->device, p->recs_dev);
    pool_free(p->device, p->scan_bnd);
    pool_free(p->device, p->lspec_dev);
    (void) hipFree(p->seedset_arena);
    (void) hipFree(p->seedset_tab);
    pool_free(p->device, p->arena);
    pool_free(p->device, p->rays_dev);
    pool_free(p->device, p->grid_dev);
    (void) hipFree(p->seedtab_dev);
    pool_free(p->device, p->image_own);
    pool_free(p->device, p->iang_own);
    pool_free(p->device, p->ctl);
    pool_free(p->device, p->tile_next);
    (void) hipFree(p->probe);
    (void) hipFree(p->bad_dev);
    delete p;
}

int rt_hip_plan_create(rt_hip_plan **out, int device, int N, const rt_beam *beam, const rt_gain *gain,
                       const rt_seed *seed, int method, double scale)
{
    return rtr::plan_create_on(out, nullptr, device, N, beam, gain, seed, method, scale);
}

} // extern "C"

int rtr::plan_create_on(rt_hip_plan **out, hipStream_t upload_q, int device, int N, const rt_beam *beam, const rt_gain *gain,
                        const rt_seed *seed, int method, double scale)
{
    if (!out || !beam || !gain)
        return fail_arg("rt_hip_plan_create: NULL argument");
    *out = nullptr;
    if (N < 2)
        return fail_arg("rt_hip_plan_create: need at least 2 lengths");
    if (method != 1 && method != 2)
        return fail_arg("rt_hip_plan_create: method must be 1 (backward) or 2 (forward)");
    if (beam->nx < 1 || beam->ny < 1 || beam->na < 1 || beam->nb < 1 || beam->nv < 1)
        return fail_arg("rt_hip_plan_create: empty beam grid");
    const int L = N - 1;
    if (L > 64)
        return fail_arg("rt_hip_plan_create: more than 65 lengths are not supported");
    const int K = beam->nv;
    for (int i = 1; i < N; i++) {
        if (gain[i].Nx < 2 || gain[i].Ny < 2 || !gain[i].x || !gain[i].y || !gain[i].n || !gain[i].g0 ||
            !gain[i].gv)
            return fail_arg("rt_hip_plan_create: incomplete gain table");
        if (gain[i].Nv != K)
            return fail_arg("rt_hip_plan_create: gain.Nv != beam.nv");
        // The cell set-up of the march forms its gather offsets as 24-bit multiply-adds (rt_march_cell.inc: interval number
        // x 48, node number x 16): interval and node numbers stay below 2^24.  (Checked before a device is asked for: the
        // refusal needs none.)
        if ((unsigned long long) gain[i].Nx * (unsigned long long) gain[i].Ny > rt::RT_MARCH_MAX_NODES)
            return fail_arg("rt_hip_plan_create: a gain table of more than 2^24 - 1 grid points is not supported");
    }
    int ndev = rt_hip_device_count();
    if (ndev <= 0) {
        last_error() = "no HIP device";
        return RT_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev)
        return fail_arg("rt_hip_plan_create: bad device index");
    HIP_TRY(hipSetDevice(device));

    rt_hip_plan *p = new rt_hip_plan();
    p->t_created   = std::chrono::steady_clock::now();
    p->device      = device;
    {
        // the CU count and the LDS a work-group may ask for do not change: asked once per device
        // (hipGetDeviceProperties costs ~0.3 ms a call)
        static std::mutex mu;
        static std::vector<std::pair<int, int>> known; // per device: {CUs, LDS bytes per work-group}
        std::lock_guard<std::mutex> lock(mu);
        if ((size_t) device >= known.size())
            known.resize((size_t) device + 1, { 0, 0 });
        if (known[(size_t) device].first == 0) {
            int n = 0, lds = 0;
            hipError_t e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device);
            if (e == hipSuccess)
                e = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
            if (e != hipSuccess || n < 1 || lds < 1) {
                delete p;
                return fail_hip(e, "hipDeviceGetAttribute(multiprocessor count, LDS per work-group)", __FILE__, __LINE__);
            }
            known[(size_t) device] = { n, lds };
        }
        p->cu_count  = known[(size_t) device].first;
        p->lds_limit = (size_t) known[(size_t) device].second;
    }

    static const bool timing = getenv("RT_HIP_TIMING") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto lap    = [&](const char *what) {
        if (timing) {
            const auto now = std::chrono::steady_clock::now();
            fprintf(stderr, "    plan_create %-18s %7.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
            t_prev = now;
        }
    };
    lap("device");
    // ---- pack the arena -------------------------------------------------
    ArenaBuilder ab;
    {
        // capacity: every piece below, each rounded up to the 256-byte alignment of its offset
        auto piece      = [](size_t bytes) { return align_up(bytes, 256) + 256; };
        const size_t kp = (size_t) ((K + 3) & ~3);
        size_t capacity = piece(sizeof(rt::DevGain) * (size_t) N), blob_bytes = align_up(sizeof(rt::BlobGain) * (size_t) N, 16);
        for (int i = 1; i < N; i++) {
            const size_t cells = (size_t) gain[i].Nx * (size_t) gain[i].Ny;
            capacity += piece(cells * kp * sizeof(float));
            blob_bytes += sizeof(rt::Interval) * ((size_t) gain[i].Nx + (size_t) gain[i].Ny) + sizeof(rt::Node) * cells;
        }
        if (blob_bytes >= rt::RT_MARCH_MAX_BLOB) { // (BlobGain::off_* are ints, and the march adds to them in 32 bits)
            delete p;
            return fail_arg("rt_hip_plan_create: march tables of 2 GiB or more are not supported");
        }
        capacity += piece(blob_bytes);
        capacity += piece(sizeof(double) * (size_t) beam->nx) + piece(sizeof(double) * (size_t) beam->ny) +
                    piece(sizeof(double) * (size_t) beam->na) + piece(sizeof(double) * (size_t) beam->nb) + 2 * piece(sizeof(double) * kp);
        if (seed)
            for (int i = 0; i < 5; i++)
                capacity += 2 * piece(sizeof(double) * ((size_t) (seed->dim[i] > 0 ? seed->dim[i] : 0) + kp));
        ab.start(capacity, upload_q != nullptr);
    }
    std::vector<rt::DevGain> dg((size_t) N);
    std::vector<size_t> off_gv((size_t) N, 0);
    const bool use_emis = gain[0].E0 != nullptr && seed == nullptr; // Helper.h:402
    const int Kp = (K + 3) & ~3; // rows padded to four frequencies (DevParams::Kp)
    for (int i = 1; i < N; i++) {
        const size_t cells = (size_t) gain[i].Nx * (size_t) gain[i].Ny;
        if (cells * (size_t) Kp * sizeof(float) >= (1ull << 32)) { // the frequency kernel addresses rows with 32 bits
            delete p;
            return fail_arg("rt_hip_plan_create: a lineshape table of 4 GiB or more is not supported");
        }
        if (Kp == K) {
            off_gv[(size_t) i] = ab.put(gain[i].gv, sizeof(float) * cells * (size_t) K);
        } else {
            off_gv[(size_t) i] = ab.reserve(sizeof(float) * cells * (size_t) Kp); // zero-filled
            float *dst         = reinterpret_cast<float *>(ab.base + off_gv[(size_t) i]);
            for (size_t c = 0; c < cells; c++)
                memcpy(dst + c * (size_t) Kp, gain[i].gv + c * (size_t) K, sizeof(float) * (size_t) K);
        }
    }
    const size_t off_bx  = ab.put(beam->x, sizeof(double) * (size_t) beam->nx);
    const size_t off_by  = ab.put(beam->y, sizeof(double) * (size_t) beam->ny);
    const size_t off_ba  = ab.put(beam->a, sizeof(double) * (size_t) beam->na);
    const size_t off_bb  = ab.put(beam->b, sizeof(double) * (size_t) beam->nb);
    const size_t off_bdv = ab.reserve(sizeof(double) * (size_t) Kp);
    memcpy(ab.base + off_bdv, beam->dv, sizeof(double) * (size_t) beam->nv);
    const size_t off_bdv2 = ab.reserve(sizeof(double) * (size_t) Kp); // 2 * dv (exact), RayTraceImageCPU.cpp:66
    for (int k = 0; k < beam->nv; k++) {
        const double d2 = 2.0 * beam->dv[k];
        memcpy(ab.base + off_bdv2 + sizeof(double) * (size_t) k, &d2, sizeof(double));
    }
    size_t off_sx[5] = { 0 }, off_sf[5] = { 0 };
    if (seed) {
        for (int i = 0; i < 5; i++) {
            // (axes 0 .. 3 are interpolated: two points at least; the fifth is a table of nv values, and nv = 1 is a problem like any other)
            if (seed->dim[i] < (i < 4 ? 2 : 1) || !seed->x[i] || !seed->f[i]) {
                delete p;
                return fail_arg("rt_hip_plan_create: incomplete seed table");
            }
            if (i == 4 && seed->dim[4] != K) {
                delete p;
                return fail_arg("rt_hip_plan_create: seed.dim[4] != beam.nv");
            }
            off_sx[i] = ab.put(seed->x[i], sizeof(double) * (size_t) seed->dim[i]);
            if (i == 4) { // the frequency profile, padded like the lineshape rows
                off_sf[i] = ab.reserve(sizeof(double) * (size_t) Kp);
                memcpy(ab.base + off_sf[i], seed->f[i], sizeof(double) * (size_t) seed->dim[i]);
            } else {
                off_sf[i] = ab.put(seed->f[i], sizeof(double) * (size_t) seed->dim[i]);
            }
        }
    }
    const size_t off_gain = ab.reserve(sizeof(rt::DevGain) * (size_t) N);
    // march blob: headers + grids + fused corner nodes of every length, copied to LDS
    // verbatim by rt_march_kernel<true>
    std::vector<unsigned char> blob(align_up(sizeof(rt::BlobGain) * (size_t) N, 16));
    bool tiny_spacing = false, bad_index = false, all_bounded = true, ntest_proven = true;
    p->tab.assign((size_t) N, rt_hip_plan::TableShape());
    for (int i = 1; i < N; i++) {
        const rt_gain &g  = gain[i];
        // (the header, the interval records of both axes and the fused nodes of this length: rt_blob_pack.h)
        const rt::BlobGain h = rt::blob_pack_length(blob, (size_t) i, g.Nx, g.Ny, g.x, g.y, g.n, g.g0, g.E0, tiny_spacing, bad_index);
        // Ranges for the short division sequences of the integrator (rt_math.h, fdiv_nr): with dn = the largest
        // difference of the index between neighbouring nodes, a step sees n within [min n - dn, max n + dn]
        // (bilinear value on the cell box with its 10 % margin, plus |r| < 0.1 w times a gradient of at most
        // 1.3 dn / w per axis) and index gradients of at most 1.3 dn / min(w).
        {
            double n_lo = g.n[0], n_hi = g.n[0], dn = 0.0, w_min = g.x[1] - g.x[0];
            for (int k = 1; k < g.Nx; k++)
                w_min = std::min(w_min, g.x[k] - g.x[k - 1]);
            for (int k = 1; k < g.Ny; k++)
                w_min = std::min(w_min, g.y[k] - g.y[k - 1]);
            for (int iy = 0; iy < g.Ny; iy++) {
                const double *row = g.n + (size_t) iy * (size_t) g.Nx;
                for (int ix = 0; ix < g.Nx; ix++) {
                    n_lo = std::min(n_lo, row[ix]);
                    n_hi = std::max(n_hi, row[ix]);
                    if (ix > 0)
                        dn = std::max(dn, fabs(row[ix] - row[ix - 1]));
                    if (iy > 0)
                        dn = std::max(dn, fabs(row[ix] - row[ix - g.Nx]));
                }
            }
            if (!(n_lo - dn >= 0.25 && n_hi + dn <= 4.0 && dn / w_min <= 1e12 && w_min >= 1e-12))
                all_bounded = false;
            // No quotient of the cross-cell set-up underflows (rt_march_xsetup.inc goes without the sign copy of a zero
            // quotient on that ground).  The node indices are doubles in [0.25, 4]: two that differ differ by at least
            // 2^-54, the spacing of the doubles at 0.25.  The other factor of a gradient dividend is a float v or 1 - v:
            // not zero, it is at least 2^-149 in magnitude.  A width is the difference of two grid values a float
            // position lies between, below 2^129.  So a non-zero gradient quotient is at least 2^-54 2^-149 2^-129 =
            // 2^-332, far inside the double range: a gradient quotient that is a zero has a dividend that is a zero.
            // (u and v themselves may underflow -- a position 2^-149 off a corner -- but a non-zero dividend gives the
            // same double with and without the copy, rt_math.h: only a -0 dividend tells the forms apart.)
            // The largest index change a step can see.  The loop condition of the integrator tests the n of the step just
            // taken, n0 + rx gxn + ry gyn with the r that passed |rx| < 0.1 wx, |ry| < 0.1 wy one step earlier (no
            // overshoot enters), and |gxn| wx <= 1.2 dn (the two edge differences of the cell weighted with v, 1 - v for
            // v in the cell box with its 10 % margin: |v| + |1 - v| <= 1.2), likewise gyn: |n - n0| <= 0.24 dn plus a few
            // roundings of floats below 4 (< 2e-6).  On the mirrored half plane (y[0] >= 0) the box of the first y
            // interval reaches down to |y| = 0, where u = -y[0] / wy: |u| + |1 - u| = 1 + 2 y[0] / wy there, which is what
            // weights the edge differences of gyn (a grid that starts at y = 0, as every shipped one does, adds nothing).
            // With a safety factor of 8 -- tables anywhere near the limit keep the test -- the march goes without it
            // (rt_march.hip, MARCH_OPT_NO_NTEST) when 8 x 0.1 (1.2 + fy) dn <= 0.05 - 1e-5.
            // (The ranges above assume the same 10 % margin; a mirrored grid that starts far from y = 0 extrapolates n
            // further than dn.  Such tables are not known; the generic instance can be forced with RT_HIP_MARCH_IEEE=1.)
            const double fy = g.y[0] >= 0.0 ? std::max(1.2, 1.0 + 2.0 * g.y[0] / (g.y[1] - g.y[0])) : 1.2;
            if (!(8.0 * 0.1 * (1.2 + fy) * dn <= 0.05 - 1e-5))
                ntest_proven = false;
            // (the grids stay; rt_hip_plan_update_gain scans new values against these)
            p->tab[(size_t) i].Nx    = g.Nx;
            p->tab[(size_t) i].Ny    = g.Ny;
            p->tab[(size_t) i].w_min = w_min;
            p->tab[(size_t) i].fy    = fy;
            p->tab[(size_t) i].off_node = (size_t) h.off_node;
        }
    }
    // (dz: a straight ray in a medium without refraction advances by up to 1250 cm per integrator step, Helper.h:288-297;
    // 1e6 cm keeps a sub-segment within a few hundred steps -- beyond it the instance with the watchdog marches)
    p->dz_bounded = beam->dz >= 1e-12 && beam->dz <= 1e6;
    if (!p->dz_bounded)
        all_bounded = false;
    p->tables_bounded = all_bounded;
    p->ntest_proven   = all_bounded && ntest_proven;
    p->march_prune    = (int) env_unsigned("RT_HIP_MARCH_PRUNE", 1, 0, 2);
    p->step_one_launch = env_unsigned("RT_HIP_STEP_ONE_LAUNCH", 0, 0, 1) == 1;
    if (tiny_spacing) {
        delete p;
        return fail_arg("rt_hip_plan_create: gain grid not strictly increasing, or spacing below 1e-30");
    }
    if (bad_index) {
        delete p;
        return fail_arg("rt_hip_plan_create: non-finite index of refraction");
    }
    const size_t off_blob = ab.put(blob.data(), blob.size());
    lap("pack");

#define PLAN_TRY(expr)                                   \
    do {                                                 \
        hipError_t e_ = (expr);                          \
        if (e_ != hipSuccess) {                          \
            rt_hip_plan_destroy(p);                      \
            return fail_hip(e_, #expr, __FILE__, __LINE__);        \
        }                                                \
    } while (0)

    if (ab.overflow) {
        delete p;
        return fail_arg("rt_hip_plan_create: internal error, the arena outgrew its computed capacity");
    }
    p->arena_bytes = align_up(ab.used, 256);
    PLAN_TRY(pool_alloc(device, (void **) &p->arena, p->arena_bytes));
    unsigned char *A = p->arena;
    p->gv_dev.assign((size_t) N, nullptr);
    for (int i = 1; i < N; i++) {
        dg[(size_t) i].gv    = reinterpret_cast<const float *>(A + off_gv[(size_t) i]);
        p->gv_dev[(size_t) i] = dg[(size_t) i].gv;
    }
    p->dv2_dev = reinterpret_cast<const double *>(A + off_bdv2);
    memcpy(ab.base + off_gain, dg.data(), sizeof(rt::DevGain) * (size_t) N);
    if (upload_q && ab.pinned) {
        // queued, not waited for: the staging buffer stays with the plan until the queue has been waited for
        // (rt_hip_plan_destroy), and every reader of the tables runs on this queue (rt_hip_image_loop)
        const size_t bytes = ab.used;
        p->staging         = ab.release();
        p->upload_q        = upload_q;
        PLAN_TRY(hipMemcpyAsync(p->arena, p->staging, bytes, hipMemcpyHostToDevice, upload_q));
    } else {
        PLAN_TRY(hipMemcpy(p->arena, ab.base, ab.used, hipMemcpyHostToDevice));
    }
    lap("alloc + upload");

    rt::DevParams &P = p->P;
    P.N        = N;
    P.L        = L;
    P.K        = K;
    P.Kp       = Kp;
    P.method   = method;
    P.use_emis = use_emis ? 1 : 0;
    P.has_seed = seed ? 1 : 0;
    P.dz0      = (float) beam->dz; // RayTraceImageCPU.cpp:31: double -> float at the call
    P.scale    = scale;
    P.beam.x   = reinterpret_cast<const double *>(A + off_bx);
    P.beam.y   = reinterpret_cast<const double *>(A + off_by);
    P.beam.a   = reinterpret_cast<const double *>(A + off_ba);
    P.beam.b   = reinterpret_cast<const double *>(A + off_bb);
    P.beam.dv  = reinterpret_cast<const double *>(A + off_bdv);
    P.beam.nx  = beam->nx;
    P.beam.ny  = beam->ny;
    P.beam.na  = beam->na;
    P.beam.nb  = beam->nb;
    P.beam.nv  = beam->nv;
    P.beam.dx  = beam->dx;
    P.beam.dy  = beam->dy;
    P.beam.da  = beam->da;
    P.beam.db  = beam->db;
    P.beam.inv_dx = 1.0 / beam->dx;
    P.beam.inv_dy = 1.0 / beam->dy;
    P.beam.inv_da = 1.0 / beam->da;
    P.beam.inv_db = 1.0 / beam->db;
    P.beam.g_first[0] = beam->x[0];
    P.beam.g_first[1] = beam->y[0];
    P.beam.g_first[2] = beam->a[0];
    P.beam.g_first[3] = beam->b[0];
    P.beam.g_last[0]  = beam->x[beam->nx - 1];
    P.beam.g_last[1]  = beam->y[beam->ny - 1];
    P.beam.g_last[2]  = beam->a[beam->na - 1];
    P.beam.g_last[3]  = beam->b[beam->nb - 1];
    if (seed) {
        for (int i = 0; i < 5; i++) {
            P.seed.x[i]   = reinterpret_cast<const double *>(A + off_sx[i]);
            P.seed.f[i]   = reinterpret_cast<const double *>(A + off_sf[i]);
            P.seed.dim[i] = seed->dim[i];
        }
        P.seed.f0 = seed->f0;
    }
    P.gain = reinterpret_cast<const rt::DevGain *>(A + off_gain);
    P.blob       = A + off_blob;
    P.blob_bytes = (unsigned) blob.size();
    if (const char *dbg = getenv("RT_HIP_DEBUG"))
        P.debug = (unsigned) strtoul(dbg, nullptr, 0);
    if (const char *ex = getenv("RT_HIP_EXACT_EMISSION")) // the loop signature has no parameter for it
        P.exact_emis = atoi(ex) ? 1 : 0;

    p->beam_x.assign(beam->x, beam->x + beam->nx);
    p->beam_y.assign(beam->y, beam->y + beam->ny);
    p->beam_a.assign(beam->a, beam->a + beam->na);
    p->beam_b.assign(beam->b, beam->b + beam->nb);
    p->n_image = (size_t) beam->nx * (size_t) beam->ny * (size_t) beam->nv;
    p->n_iang  = (size_t) beam->na * (size_t) beam->nb;
    PLAN_TRY(pool_alloc(device, (void **) &p->ctl, sizeof(rt::DevCtl)));
    PLAN_TRY(hipEventCreate(&p->ev0));
    PLAN_TRY(hipEventCreate(&p->ev1));
    PLAN_TRY(hipEventCreate(&p->evm));
    P.rec_stride = (unsigned) align_up((size_t) L * RT_N_SUB * 12 + sizeof(rt::RecMeta), 16);
    P.c_cap      = 0.5f * 1.00001f; // step safety factor c = 0.5 (Helper.h:381), see rt_hip_plan_set_step_factor
    P.c_h1       = 0.5f * 0.1f;
    P.c_h3       = 0.5f * 0.05f;
    {
        // largest finite |lineshape value| of the planes the emission-mode frequency pass reads (integer
        // maximum of the magnitude bits: non-negative floats order like their bit patterns, and the loop
        // vectorises)
        float wmax = 0.0f;
        if (use_emis) {
            uint32_t umax          = 0;
            static const bool avx2 = __builtin_cpu_supports("avx2");
            for (int i = 1; i < N; i++) {
                const size_t n = (size_t) gain[i].Nx * (size_t) gain[i].Ny * (size_t) K;
                uint32_t m = 0, mall = 0;
                (avx2 ? magnitude_scan_avx2 : magnitude_scan_plain)(reinterpret_cast<const uint32_t *>(gain[i].gv), n, m, mall);
                umax = m > umax ? m : umax;
                if (mall >= 0x7f800000u) // a NaN or an infinity: the frequency kernel then tests every value it reads
                    p->gv_has_nan = true;
            }
            memcpy(&wmax, &umax, sizeof(wmax));
        }
        P.gs_cap = wmax > 0.0f ? 708.0f / wmax : FLT_MAX;
        if (!(P.gs_cap <= FLT_MAX))
            P.gs_cap = FLT_MAX;
    }
    P.ctl = p->ctl;
    *out  = p;
    lap("rest");
    return RT_OK;
}

// What rt_hip_plan_set_ray_grid does for the creation seed, for every seed of the set: on a forward ray grid the seed
// profile is a product of one factor per grid axis, tabulated per grid point by rt_seed_tab_kernel (DevRays::sf / sin).
// Called when the grid or the set has changed, with the plan quiet.
int rtr::plan_build_seedset_tabs(rt_hip_plan *p)
{
    (void) hipFree(p->seedset_tab);
    p->seedset_tab = nullptr;
    for (int s = 0; s < RT_N_SEED_MAX; s++) {
        p->seedset_sf[s]  = nullptr;
        p->seedset_sin[s] = nullptr;
    }
    const rt::DevRays &R = p->P.rays;
    const int n_set = p->n_seed > 0 ? p->n_seed : p->n_scan_seed > 0 ? p->n_scan_seed : p->n_spec_seed; // (a seed set, the seeds of a scan or those of the spectra modes: never two of them)
    // (R.sf: a ray grid, a seeded plan, the forward method; ASE seeds on an emission plan, which has no creation seed and
    // hence no R.sf: the same grid and method)
    // (... and the ASE seeds of a scan, which is forward by construction)
    const bool ase_grid = p->P.use_emis && n_set > 0 && !R.list && R.gx && p->P.method != 1;
    if (n_set < 1 || (!R.sf && !ase_grid))
        return RT_OK;
    const size_t nn = (size_t) R.ngx + (size_t) R.ngy + (size_t) R.nga + (size_t) R.ngb;
    const size_t per_seed = align_up(nn * sizeof(double) + nn, 256);
    HIP_TRY(dev_malloc((void **) &p->seedset_tab, per_seed * (size_t) n_set));
    for (int s = 0; s < n_set; s++) {
        double *sf           = reinterpret_cast<double *>(p->seedset_tab + per_seed * (size_t) s);
        unsigned char *flags = reinterpret_cast<unsigned char *>(sf + nn);
        const int rc         = launch_seed_tab(p->seed_set[s], R, nn, sf, flags);
        if (rc != RT_OK)
            return rc;
        p->seedset_sf[s]  = sf;
        p->seedset_sin[s] = flags;
    }
    HIP_TRY(hipDeviceSynchronize());
    return RT_OK;
}

// rt_hip_image_loop only: the outputs of a run that are a few megabytes at most follow its kernels down the queue into
// page-locked staging -- one wait in rt_hip_plan_fetch instead of a wait and three blocking copies (larger images are
// fetched directly: copying them once more on the host would cost what the queueing saves).
void rtr::plan_stage_outputs(rt_hip_plan *p)
{
    constexpr size_t ctl_tail = offsetof(rt::DevCtl, failure_code), ctl_bytes = sizeof(rt::DevCtl) - ctl_tail;
    if (!p || !p->ran || !p->last_stream)
        return;
    if (p->last_step && (p->last_step_lent || p->last_records.n_rec() > 0)) // E_v and nf are the caller's, or one record of several: fetched the ordinary way
        return;
    // (a step run: E_v and nf travel where the image does)
    const double *big    = p->last_step ? p->step_dev : p->last_image;
    const size_t n_big   = p->last_step ? p->step_doubles : p->n_image;
    const size_t off_ang = align_up(ctl_bytes, 256), off_img = off_ang + align_up(p->n_iang * sizeof(double), 256);
    const size_t total   = off_img + n_big * sizeof(double);
    if (total > ((size_t) 4 << 20))
        return;
    if (p->out_staging && p->out_staging_bytes < total) {
        pinned_free(p->out_staging);
        p->out_staging = nullptr;
    }
    if (!p->out_staging) {
        void *h = nullptr;
        if (pinned_alloc(&h, total) != hipSuccess)
            return;
        p->out_staging       = static_cast<unsigned char *>(h);
        p->out_staging_bytes = total;
    }
    hipError_t e = hipMemcpyAsync(p->out_staging, reinterpret_cast<const unsigned char *>(p->ctl) + ctl_tail, ctl_bytes,
                                  hipMemcpyDeviceToHost, p->last_stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(p->out_staging + off_ang, p->last_iang, p->n_iang * sizeof(double), hipMemcpyDeviceToHost, p->last_stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(p->out_staging + off_img, big, n_big * sizeof(double), hipMemcpyDeviceToHost, p->last_stream);
    if (e != hipSuccess) {
        (void) hipGetLastError(); // fetched the ordinary way
        return;
    }
    p->out_staged = true;
}

// rt_hip_image_loop only: the list stays on the host until the run, which uploads it in slices
// beside the march (the caller's buffer outlives the call, the plan does not)
int rtr::plan_set_rays_deferred(rt_hip_plan *p, const rt_ray *rays, size_t n_rays)
{
    if (n_rays > MAX_LIST_RAYS)
        return fail_arg("ray list of 2^32 - 4096 rays or more: split the call");
    HIP_TRY(hipSetDevice(p->device));
    plan_quiesce(p);
    pool_free(p->device, p->rays_dev);
    pool_free(p->device, p->tan_dev);
    p->rays_dev = nullptr;
    p->tan_dev  = nullptr;
    if (n_rays) {
        HIP_TRY(pool_alloc(p->device, (void **) &p->rays_dev, n_rays * sizeof(rt_ray)));
        HIP_TRY(pool_alloc(p->device, (void **) &p->tan_dev, n_rays * 2 * sizeof(float)));
    }
    p->P.exclusive  = 0;
    p->P.own_cells  = 0;
    p->P.rays       = {};
    p->P.rays.list  = p->rays_dev;
    p->P.rays.sxy   = p->tan_dev;
    p->P.rays.count = n_rays;
    p->n_rays       = n_rays;
    p->host_rays    = n_rays ? rays : nullptr;
    return RT_OK;
}

extern "C" {

int rt_hip_plan_set_rays(rt_hip_plan *p, const rt_ray *rays, size_t n_rays)
{
    if (!p || (n_rays && !rays))
        return fail_arg("rt_hip_plan_set_rays: NULL argument");
    if (n_rays > MAX_LIST_RAYS)
        return fail_arg("rt_hip_plan_set_rays: 2^32 - 4096 rays or more: split the call");
    HIP_TRY(hipSetDevice(p->device));
    plan_quiesce(p);
    pool_free(p->device, p->rays_dev);
    p->rays_dev = nullptr;
    if (n_rays) {
        HIP_TRY(pool_alloc(p->device, (void **) &p->rays_dev, n_rays * sizeof(rt_ray)));
        HIP_TRY(hipMemcpy(p->rays_dev, rays, n_rays * sizeof(rt_ray), hipMemcpyHostToDevice));
    }
    pool_free(p->device, p->tan_dev);
    p->tan_dev = nullptr;
    if (n_rays) {
        // Helper.h:409-410 for every ray, at full lane occupancy, before the march
        HIP_TRY(pool_alloc(p->device, (void **) &p->tan_dev, n_rays * 2 * sizeof(float)));
        if (tan_mode(p->device) == 2) {
            std::vector<float> h(n_rays * 2);
            host_tangents(rays, n_rays, h.data());
            HIP_TRY(hipMemcpy(p->tan_dev, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        } else {
            const int rc = launch_tan(p->rays_dev, (unsigned long long) n_rays, p->tan_dev, nullptr);
            if (rc != RT_OK)
                return rc;
            HIP_TRY(hipDeviceSynchronize());
        }
    }
    p->P.exclusive  = 0;
    p->P.own_cells  = 0;
    p->P.rays       = {};
    p->P.rays.list  = p->rays_dev;
    p->P.rays.sxy   = p->tan_dev;
    p->P.rays.count = n_rays;
    p->n_rays       = n_rays;
    p->host_rays    = nullptr;
    return RT_OK;
}

int rt_hip_plan_set_ray_grid(rt_hip_plan *p, const double *gx, int ngx, const double *gy, int ngy,
                             const double *ga, int nga, const double *gb, int ngb, int64_t first,
                             int64_t stride, int64_t count)
{
    if (!p || !gx || !gy || !ga || !gb || ngx < 1 || ngy < 1 || nga < 1 || ngb < 1)
        return fail_arg("rt_hip_plan_set_ray_grid: bad grid");
    const int64_t total = (int64_t) ngx * ngy * nga * ngb;
    if (total > 0x7fffffffLL) // the reference indexes rays with int (RayTraceImage.cpp:302)
        return fail_arg("rt_hip_plan_set_ray_grid: more than 2^31 rays");
    if (first < 0 || stride < 1 || count < 0 || (count > 0 && first + (count - 1) * stride >= total))
        return fail_arg("rt_hip_plan_set_ray_grid: ray range outside the grid");
    HIP_TRY(hipSetDevice(p->device));
    plan_quiesce(p);
    pool_free(p->device, p->grid_dev);
    p->grid_dev     = nullptr;
    (void) hipFree(p->seedtab_dev);
    p->seedtab_dev  = nullptr;
    const size_t nn = (size_t) ngx + (size_t) ngy + (size_t) nga + (size_t) ngb;
    // one upload: the four grids, then the launch tangents of the a and b values -- Helper.h:409-410,
    // tanf(1e-3f * ray.a) depends only on the grid value: nga + ngb evaluations on the host, with the same libm
    // the CPU loop uses
    const size_t nt = (size_t) nga + (size_t) ngb;
    std::vector<double> h(nn + (nt + 1) / 2);
    memcpy(h.data(), gx, sizeof(double) * (size_t) ngx);
    memcpy(h.data() + ngx, gy, sizeof(double) * (size_t) ngy);
    memcpy(h.data() + ngx + ngy, ga, sizeof(double) * (size_t) nga);
    memcpy(h.data() + ngx + ngy + nga, gb, sizeof(double) * (size_t) ngb);
    {
        std::vector<float> ht(nt);
        for (int k = 0; k < nga; k++)
            ht[(size_t) k] = tanf(1e-3f * (float) ga[k]);
        for (int m = 0; m < ngb; m++)
            ht[(size_t) nga + (size_t) m] = tanf(1e-3f * (float) gb[m]);
        memcpy(h.data() + nn, ht.data(), nt * sizeof(float));
    }
    HIP_TRY(pool_alloc(p->device, (void **) &p->grid_dev, h.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(p->grid_dev, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    pool_free(p->device, p->tan_dev); // (the per-ray tangents of a list this plan may have held before)
    p->tan_dev            = nullptr;
    const float *tan_grid = reinterpret_cast<const float *>(p->grid_dev + nn);
    p->host_rays   = nullptr;
    rt::DevRays &R = p->P.rays;
    R              = {};
    R.list         = nullptr;
    R.tan_a        = tan_grid;
    R.tan_b        = tan_grid + nga;
    R.gx           = p->grid_dev;
    R.gy           = p->grid_dev + ngx;
    R.ga           = p->grid_dev + ngx + ngy;
    R.gb           = p->grid_dev + ngx + ngy + nga;
    R.ngx          = ngx;
    R.ngy          = ngy;
    R.nga          = nga;
    R.ngb          = ngb;
    R.first        = first;
    R.stride       = stride;
    R.count        = (unsigned long long) count;
    p->n_rays      = (unsigned long long) count;
    {
        const int divisors[3] = { ngb, nga, ngy };
        for (int t = 0; t < 3; t++)
            magic_u31((unsigned) divisors[t], R.div_mul[t], R.div_sh[t]);
    }
    if (p->P.has_seed && p->P.method != 1) {
        HIP_TRY(dev_malloc((void **) &p->seedtab_dev, nn * sizeof(double) + nn));
        unsigned char *flags = reinterpret_cast<unsigned char *>(p->seedtab_dev + nn);
        const int rc = launch_seed_tab(p->P.seed, R, nn, p->seedtab_dev, flags);
        if (rc != RT_OK)
            return rc;
        HIP_TRY(hipDeviceSynchronize());
        R.sf  = p->seedtab_dev;
        R.sin = flags;
    }
    // One ray per pixel, every pixel covered: in ASE mode ray ijkm lands in pixel (i, j)
    // (SURVEY.md 8(c) i) -- the deposit index of the ray is verified per ray by the kernel,
    // which falls back to atomics for any ray that does not land in its own pixel.
    // (as the floats a ray carries: a list recognised as a grid, rt_hip_image_loop, arrives as floats)
    auto same = [](const std::vector<double> &v, const double *g, int n) {
        if ((int) v.size() != n)
            return false;
        for (int i = 0; i < n; i++) {
            const float a = (float) v[(size_t) i], b = (float) g[i];
            if (memcmp(&a, &b, sizeof(float)) != 0)
                return false;
        }
        return true;
    };
    auto own_cell = [](const std::vector<double> &g, double d) { return grid_points_in_own_cells(g.data(), (int) g.size(), d); };
    p->P.own_cells = (p->P.method == 1 && same(p->beam_x, gx, ngx) && same(p->beam_y, gy, ngy) && same(p->beam_a, ga, nga) &&
                      same(p->beam_b, gb, ngb) && own_cell(p->beam_x, p->P.beam.dx) && own_cell(p->beam_y, p->P.beam.dy) &&
                      own_cell(p->beam_a, p->P.beam.da) && own_cell(p->beam_b, p->P.beam.db) &&
                      !getenv("RT_HIP_NO_OWN_CELLS"))
                         ? 1u
                         : 0u;
    // (with emission only: the gain-only instance of the frequency kernel carries no exclusive deposit)
    p->P.exclusive = (p->P.own_cells && p->P.use_emis && nga == 1 && ngb == 1 && first == 0 && stride == 1 && count == total) ? 1u : 0u;
    return plan_build_seedset_tabs(p); // (a seed set installed before the grid)
}

int rt_hip_plan_set_exact_emission(rt_hip_plan *p, int on)
{
    if (!p)
        return fail_arg("rt_hip_plan_set_exact_emission: NULL plan");
    p->P.exact_emis = on ? 1 : 0;
    return RT_OK;
}

int rt_hip_plan_set_step_factor(rt_hip_plan *p, double c)
{
    if (!p || !(c > 0.0) || !(c < 1.0))
        return fail_arg("rt_hip_plan_set_step_factor: c must be in (0, 1)");
    const float cf = (float) c; // RayTraceImage.cpp:462: (float) c at the call
    p->P.c_cap     = cf * 1.00001f;
    p->P.c_h1      = cf * 0.1f;
    p->P.c_h3      = cf * 0.05f;
    return RT_OK;
}

int rt_hip_plan_set_debug(rt_hip_plan *p, unsigned bits)
{
    if (!p)
        return fail_arg("rt_hip_plan_set_debug: NULL plan");
    p->P.debug = bits;
    return RT_OK;
}

} // extern "C"
// (below, with the installers: the seeds of a set, of a scan or of the spectra modes into the plan; n_seed = 0 removes them)
enum SeedsOwner { SEEDS_OF_SET = 0, SEEDS_OF_SCAN = 1, SEEDS_OF_SPECTRA = 2 };
static int seeds_install(rt_hip_plan *p, int n_seed, const rt_seed *seeds, SeedsOwner owner);
extern "C" {

int rt_hip_plan_enable_path(rt_hip_plan *p, int on)
{
    if (!p)
        return fail_arg("rt_hip_plan_enable_path: NULL plan");
    if (on && p->spectra_on)
        return fail_arg("rt_hip_plan_enable_path: the plan is in spectra mode (one per-ray output at a time)");
    if (on && p->step_on)
        return fail_arg("rt_hip_plan_enable_path: the plan is in step mode (one output mode at a time)");
    if (on && p->n_seed > 0)
        return fail_arg("rt_hip_plan_enable_path: the plan holds a seed set (step mode only)");
    if (on && p->scan_on)
        return fail_arg(suffix_scan(p) ? "rt_hip_plan_enable_path: the suffix scan is on (step mode only)"
                                       : "rt_hip_plan_enable_path: the length scan is on (step mode only)");
    if (on && p->lspec_on)
        return fail_arg("rt_hip_plan_enable_path: length spectra are on (one per-ray output at a time)");
    p->path_on = on != 0;
    return RT_OK;
}

int rt_hip_plan_fetch_path(rt_hip_plan *p, float *path, int32_t *err)
{
    if (!p || !p->ran || !p->path_on || !p->path_dev)
        return fail_arg("rt_hip_plan_fetch_path: the path tracer was not enabled for the last run");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->last_stream));
    const size_t n2 = (size_t) p->P.L * RT_N_SUB + 1;
    if (path)
        HIP_TRY(hipMemcpy(path, p->path_dev, (size_t) p->n_rays * n2 * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (err)
        HIP_TRY(hipMemcpy(err, p->path_err, (size_t) p->n_rays * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_hip_plan_enable_spectra(rt_hip_plan *p, int on)
{
    if (!p)
        return fail_arg("rt_hip_plan_enable_spectra: NULL plan");
    if (on && p->path_on)
        return fail_arg("rt_hip_plan_enable_spectra: the path tracer is enabled (one per-ray output at a time)");
    if (on && p->step_on)
        return fail_arg("rt_hip_plan_enable_spectra: the plan is in step mode (one output mode at a time)");
    if (on && p->n_seed > 0)
        return fail_arg("rt_hip_plan_enable_spectra: the plan holds a seed set (step mode only)");
    if (on && p->scan_on)
        return fail_arg(suffix_scan(p) ? "rt_hip_plan_enable_spectra: the suffix scan is on (step mode only)"
                                       : "rt_hip_plan_enable_spectra: the length scan is on (step mode only)");
    if (on && p->lspec_on)
        return fail_arg("rt_hip_plan_enable_spectra: length spectra are on (a mode of their own: rt_hip_plan_enable_length_spectra switches them off)");
    if (!on && p->spectra_on && p->n_spec_seed > 0) { // the seeds of rt_hip_plan_set_spectra_seeds exist only while the mode is on
        const int rc = seeds_install(p, 0, nullptr, SEEDS_OF_SPECTRA);
        if (rc != RT_OK)
            return rc;
    }
    p->spectra_on = on != 0;
    return RT_OK;
}

// (the accessors of the rows of a spectra run, of either mode: below, with the one table and the one path they share)

// Length spectra (include/rt_hip.h): a mode of its own beside spectra mode and the scans.  The switch owns the boundary
// states of the march while it is on, as scan_switch does for a scan; the method of the plan says prefix or suffix.
int rt_hip_plan_enable_length_spectra(rt_hip_plan *p, int on)
{
    auto fail = [&](const char *what) { return fail_arg((std::string("rt_hip_plan_enable_length_spectra") + what).c_str()); };
    if (!p)
        return fail(": NULL plan");
    if (on) {
        if (p->P.N < 3)
            return fail(": N < 3 (one length: spectra mode is the whole curve)");
        if (p->P.N - 1 > RT_N_SCAN_MAX)
            return fail(": more than RT_N_SCAN_MAX lengths");
        if (p->step_on)
            return fail(": the plan is in step mode (one output mode at a time)");
        if (p->spectra_on)
            return fail(": the plan is in spectra mode (length spectra are a mode of their own)");
        if (p->path_on)
            return fail(": the path tracer is enabled (one per-ray output at a time)");
        if (p->scan_on)
            return fail(suffix_scan(p) ? ": the suffix scan is on (it leaves step records, not spectra)" : ": the length scan is on (it leaves step records, not spectra)");
        if (p->n_seed > 0)
            return fail(p->P.use_emis ? ": the plan holds ASE seeds (length spectra take the creation seed alone)"
                                      : ": the plan holds a seed set (length spectra take the creation seed alone)");
    }
    if ((on != 0) == p->lspec_on)
        return RT_OK;
    HIP_TRY(hipSetDevice(p->device));
    if (p->ran) { // the last run keeps its buffers until it is final
        const int rs = plan_settle_last_run(p);
        if (rs != RT_OK)
            return rs;
    }
    plan_quiesce(p);
    p->lspec_on = on != 0;
    if (!p->lspec_on) { // the boundary states and the rows exist only while the mode is on
        pool_free(p->device, p->scan_bnd);
        p->scan_bnd       = nullptr;
        p->scan_bnd_bytes = 0;
        pool_free(p->device, p->lspec_dev);
        p->lspec_dev   = nullptr;
        p->lspec_bytes = 0;
        p->lspec       = {};
        // (the rows of a last length-spectra run are gone: the accessors say so by the buffer, rt_hip_plan_fetch keeps the
        // report and the counters)
        if (p->n_spec_seed > 0) // ... and so do the seeds of rt_hip_plan_set_spectra_seeds or rt_hip_plan_set_length_spectra_ase_seeds
            return seeds_install(p, 0, nullptr, SEEDS_OF_SPECTRA);
    }
    return RT_OK;
}

} // extern "C"

// ---- the rows of the last per-ray spectra run (rt_records.h: RowSet says which blocks there are) ---------------------------
// An accessor pair of the C ABI: the kinds of last run it serves (bits by RowKind), what it says after a run of another
// kind, and what of an index the run has not -- the length first, then "no seeds" where the pair asks for a seed and the run
// carried none, then the first index (nullptr: the pair has no such index, or no such refusal).
struct RowsAccessor {
    unsigned kinds;
    const char *not_kind, *bad_n, *no_seeds, *bad_first;
};
constexpr unsigned rows_bit(RowKind k) { return 1u << k; }
static const char NOT_LSPEC[] = ": the last run was not a length-spectra run (or length spectra have been switched off since)";
// (the plain pair serves block 0 of all three spectra-mode kinds: seed 0, or the ASE rows)
static const RowsAccessor ACC_SPEC      = { rows_bit(ROWS_SPEC) | rows_bit(ROWS_SPEC_SEEDS) | rows_bit(ROWS_SPEC_ASE_SEEDS), ": the last run was not a spectra run", nullptr,
                                            nullptr, nullptr };
static const RowsAccessor ACC_SEED_SPEC = { rows_bit(ROWS_SPEC_SEEDS), ": the last run was not a spectra run with spectra seeds", nullptr, nullptr,
                                            ": s must be 0 .. n_seed - 1 of the last run" };
static const RowsAccessor ACC_FULL_SPEC = { rows_bit(ROWS_SPEC_ASE_SEEDS), ": the last run was not a spectra run with ASE seeds", nullptr, nullptr,
                                            ": r must be 0 .. n_seed of the last run" };
// (a length alone means seed 0 of a run with seeds)
// (... or the ASE curve of a run with ASE seeds)
static const RowsAccessor ACC_LSPEC      = { rows_bit(ROWS_LSPEC) | rows_bit(ROWS_LSPEC_SEEDS) | rows_bit(ROWS_LSPEC_ASE_SEEDS), NOT_LSPEC, ": n must be 2 .. N of the last run", nullptr, nullptr };
static const RowsAccessor ACC_SEED_LSPEC = { rows_bit(ROWS_LSPEC) | rows_bit(ROWS_LSPEC_SEEDS), NOT_LSPEC, ": n must be 2 .. N of the last run",
                                             ": the last run carried no spectra seeds", ": s must be 0 .. n_seed - 1 of the last run" };

static const RowsAccessor ACC_FULL_LSPEC = { rows_bit(ROWS_LSPEC_ASE_SEEDS),
                                             ": the last run was not a length-spectra run with ASE seeds (or length spectra have been switched off since)",
                                             ": n must be 2 .. N of the last run", nullptr, ": r must be 0 .. n_seed of the last run" };

// what the last run wrote: the set of spectra mode it took, or the one block of length spectra (all NULL once length spectra
// have been switched off: the rows are gone, a fact of the buffer and not of the descriptor)
static const rt::SpecOut &rows_out(const rt_hip_plan *p) { return p->last_rows.lengths() ? p->lspec : p->spec[p->spec_last]; }

// The block of Iv and err of the last run that (s, n) means to the accessor `who`, or -1 behind its refusal (who == nullptr:
// behind no text at all, for the one accessor that answers NULL).
static int rows_block(const rt_hip_plan *p, const char *who, const RowsAccessor &a, int s, int n)
{
    auto fail = [&](const char *what) { return (void) (who ? fail_arg((std::string(who) + what).c_str()) : 0), -1; };
    if (!p || !p->ran || !(a.kinds & rows_bit(p->last_rows.kind)) || !rows_out(p).Iv)
        return fail(a.not_kind);
    const RowSet &R = p->last_rows;
    if (a.bad_n && R.ray2_block(n) < 0)
        return fail(a.bad_n);
    if (a.no_seeds && !R.row().seeds)
        return fail(a.no_seeds);
    if (R.block(s, n) < 0)
        return fail(a.bad_first);
    return R.block(s, n);
}
// ... the addresses of its rows (ray2 has the block of the length alone), and the rows through host pointers: as many as the
// RUN had rays, whatever ray set the plan has been given since
static int rows_ptrs(rt_hip_plan *p, const char *who, const RowsAccessor &a, int s, int n, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev)
{
    const int b = rows_block(p, who, a, s, n);
    if (b < 0)
        return RT_ERR_ARG;
    const size_t nr = p->last_rows.n_rays;
    const rt::SpecOut &o = rows_out(p);
    if (Iv_dev)
        *Iv_dev = o.Iv + (size_t) b * nr * (size_t) p->P.K;
    if (ray2_dev)
        *ray2_dev = o.ray2 + (size_t) p->last_rows.ray2_block(n) * nr;
    if (err_dev)
        *err_dev = o.err + (size_t) b * nr;
    return RT_OK;
}
static int rows_fetch(rt_hip_plan *p, const char *who, const RowsAccessor &a, int s, int n, double *Iv, rt_ray *ray2, int32_t *err)
{
    double *Iv_dev   = nullptr;
    rt_ray *ray2_dev = nullptr;
    int32_t *err_dev = nullptr;
    if (rows_ptrs(p, who, a, s, n, &Iv_dev, &ray2_dev, &err_dev) != RT_OK)
        return RT_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->last_stream));
    const size_t nr = p->last_rows.n_rays;
    if (nr == 0)
        return RT_OK;
    if (Iv)
        HIP_TRY(hipMemcpy(Iv, Iv_dev, nr * (size_t) p->P.K * sizeof(double), hipMemcpyDeviceToHost));
    if (ray2)
        HIP_TRY(hipMemcpy(ray2, ray2_dev, nr * sizeof(rt_ray), hipMemcpyDeviceToHost));
    if (err)
        HIP_TRY(hipMemcpy(err, err_dev, nr * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" {

int rt_hip_plan_fetch_spectra(rt_hip_plan *p, double *Iv, rt_ray *ray2, int32_t *err) { return rows_fetch(p, "rt_hip_plan_fetch_spectra", ACC_SPEC, 0, 0, Iv, ray2, err); }
double *rt_hip_plan_spectra_ptr(rt_hip_plan *p) { return rows_block(p, nullptr, ACC_SPEC, 0, 0) < 0 ? nullptr : rows_out(p).Iv; }
int rt_hip_plan_fetch_seed_spectra(rt_hip_plan *p, int s, double *Iv, rt_ray *ray2, int32_t *err)
{
    return rows_fetch(p, "rt_hip_plan_fetch_seed_spectra", ACC_SEED_SPEC, s, 0, Iv, ray2, err);
}
int rt_hip_plan_seed_spectra_ptrs(rt_hip_plan *p, int s, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev)
{
    return rows_ptrs(p, "rt_hip_plan_seed_spectra_ptrs", ACC_SEED_SPEC, s, 0, Iv_dev, ray2_dev, err_dev);
}
int rt_hip_plan_fetch_full_spectra(rt_hip_plan *p, int r, double *Iv, rt_ray *ray2, int32_t *err)
{
    return rows_fetch(p, "rt_hip_plan_fetch_full_spectra", ACC_FULL_SPEC, r, 0, Iv, ray2, err);
}
int rt_hip_plan_full_spectra_ptrs(rt_hip_plan *p, int r, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev)
{
    return rows_ptrs(p, "rt_hip_plan_full_spectra_ptrs", ACC_FULL_SPEC, r, 0, Iv_dev, ray2_dev, err_dev);
}
int rt_hip_plan_fetch_length_spectra(rt_hip_plan *p, int n, double *Iv, rt_ray *ray2, int32_t *err)
{
    return rows_fetch(p, "rt_hip_plan_fetch_length_spectra", ACC_LSPEC, 0, n, Iv, ray2, err);
}
int rt_hip_plan_length_spectra_ptrs(rt_hip_plan *p, int n, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev)
{
    return rows_ptrs(p, "rt_hip_plan_length_spectra_ptrs", ACC_LSPEC, 0, n, Iv_dev, ray2_dev, err_dev);
}
int rt_hip_plan_fetch_seed_length_spectra(rt_hip_plan *p, int s, int n, double *Iv, rt_ray *ray2, int32_t *err)
{
    return rows_fetch(p, "rt_hip_plan_fetch_seed_length_spectra", ACC_SEED_LSPEC, s, n, Iv, ray2, err);
}
int rt_hip_plan_seed_length_spectra_ptrs(rt_hip_plan *p, int s, int n, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev)
{
    return rows_ptrs(p, "rt_hip_plan_seed_length_spectra_ptrs", ACC_SEED_LSPEC, s, n, Iv_dev, ray2_dev, err_dev);
}

int rt_hip_plan_fetch_full_length_spectra(rt_hip_plan *p, int r, int n, double *Iv, rt_ray *ray2, int32_t *err)
{
    return rows_fetch(p, "rt_hip_plan_fetch_full_length_spectra", ACC_FULL_LSPEC, r, n, Iv, ray2, err);
}
int rt_hip_plan_full_length_spectra_ptrs(rt_hip_plan *p, int r, int n, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev)
{
    return rows_ptrs(p, "rt_hip_plan_full_length_spectra_ptrs", ACC_FULL_LSPEC, r, n, Iv_dev, ray2_dev, err_dev);
}

int rt_hip_plan_enable_step(rt_hip_plan *p, int on)
{
    if (!p)
        return fail_arg("rt_hip_plan_enable_step: NULL plan");
    if (on && (p->path_on || p->spectra_on))
        return fail_arg("rt_hip_plan_enable_step: the path tracer or spectra mode is enabled (one output mode at a time)");
    if (on && p->lspec_on)
        return fail_arg("rt_hip_plan_enable_step: length spectra are on (one output mode at a time)");
    p->step_on = on != 0;
    return RT_OK;
}

int rt_hip_plan_set_step_one_launch(rt_hip_plan *p, int on)
{
    if (!p)
        return fail_arg("rt_hip_plan_set_step_one_launch: NULL plan");
    if (on != 0 && on != 1)
        return fail_arg("rt_hip_plan_set_step_one_launch: on is 0 or 1");
    p->step_one_launch = on == 1; // (any mode: the next step run reads it, plan_launch_run)
    return RT_OK;
}

int rt_hip_plan_set_step_buffers(rt_hip_plan *p, double *E_v_dev, double *nf_dev)
{
    if (!p)
        return fail_arg("rt_hip_plan_set_step_buffers: NULL plan");
    if ((E_v_dev == nullptr) != (nf_dev == nullptr))
        return fail_arg("rt_hip_plan_set_step_buffers: E_v and nf are lent together or not at all");
    // (what the kernels need: 8-byte atomics and stores, the zeroing launch writes 8-byte words)
    if (reinterpret_cast<uintptr_t>(E_v_dev) % sizeof(double) || reinterpret_cast<uintptr_t>(nf_dev) % sizeof(double))
        return fail_arg("rt_hip_plan_set_step_buffers: a pointer is not aligned to 8 bytes");
    p->step_ev_lent = E_v_dev; // taken by the next step run; the last run's buffers stay those of rt_hip_plan_fetch_step
    p->step_nf_lent = nf_dev;
    return RT_OK;
}

int rt_hip_plan_step_ptrs(rt_hip_plan *p, double **E_v_dev, double **nf_dev)
{
    if (!p || !p->ran || !p->last_step)
        return fail_arg("rt_hip_plan_step_ptrs: the last run was not a step run");
    if (E_v_dev)
        *E_v_dev = p->step.E_v;
    if (nf_dev)
        *nf_dev = p->step.nf;
    return RT_OK;
}

int rt_hip_plan_enable_probe(rt_hip_plan *p, int on)
{
    if (!p)
        return fail_arg("rt_hip_plan_enable_probe: NULL plan");
    p->probe_on = on != 0;
    return RT_OK;
}

} // extern "C"

static int plan_prepare_probe(rt_hip_plan *p)
{
    const size_t n = (size_t) p->n_rays;
    if (!p->probe_on) {
        p->P.probe_on = 0;
        return RT_OK;
    }
    if (p->probe_rays != n || !p->probe) {
        (void) hipFree(p->probe);
        p->probe = nullptr;
        size_t bytes = n * (sizeof(rt_ray) + 8) + 1024;
        HIP_TRY(dev_malloc((void **) &p->probe, bytes));
        p->probe_rays = n;
    }
    unsigned char *b = p->probe;
    p->P.probe.ray2  = reinterpret_cast<rt_ray *>(b);
    b += n * sizeof(rt_ray);
    p->P.probe.flags = reinterpret_cast<uint32_t *>(b);
    b += n * 4;
    p->P.probe.steps = reinterpret_cast<uint32_t *>(b);
    p->P.probe_on    = 1;
    return RT_OK;
}

extern "C" {

int rt_hip_plan_run(rt_hip_plan *p, void *stream_v, double *image_dev, double *iang_dev)
{
    if (!p)
        return fail_arg("rt_hip_plan_run: NULL plan");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_v);
    const bool lspec   = p->lspec_on; // length spectra: a spectra run at every length (rt_spec_scan.hip)
    if (lspec && (image_dev || iang_dev))
        return fail_arg("rt_hip_plan_run: a length-spectra run takes no image buffers");
    if (lspec && (p->spectra_on || p->step_on || p->path_on || p->scan_on || p->n_seed > 0)) // (no call leads here: every switch refuses the other)
        return fail_arg("rt_hip_plan_run: length spectra together with another output mode");
    const bool spectra = p->spectra_on || lspec; // no image, no I_ang: neither allocated nor zeroed
    if (spectra && (image_dev || iang_dev))
        return fail_arg("rt_hip_plan_run: a spectra run takes no image buffers");
    if (spectra && p->path_on)
        return fail_arg("rt_hip_plan_run: spectra mode and the path tracer are both enabled");
    const bool step = p->step_on; // E_v, nf and I_ang: the image cube is neither allocated nor written
    if (step && (spectra || p->path_on))
        return fail_arg("rt_hip_plan_run: step mode together with spectra mode or the path tracer");
    if (step && image_dev)
        return fail_arg("rt_hip_plan_run: a step run takes no image buffer");
    const bool lent = step && p->step_ev_lent; // E_v and nf in the caller's memory (rt_hip_plan_set_step_buffers)
    const size_t nf_off = align_up((size_t) p->P.K * sizeof(double), 256) / sizeof(double);
    if (suffix_scan(p)) {
        if (!step || p->path_on)
            return fail_arg("rt_hip_plan_run: the suffix scan is on, which runs in step mode only");
        if (lent)
            return fail_arg("rt_hip_plan_run: a suffix scan writes the plan's own records, not lent step buffers");
        if (image_dev || iang_dev)
            return fail_arg("rt_hip_plan_run: a run with the suffix scan on takes no image and no I_ang buffer");
    } else if (p->scan_on) {
        if (!step || p->path_on)
            return fail_arg("rt_hip_plan_run: the length scan is on, which runs in step mode only");
        if (lent)
            return fail_arg("rt_hip_plan_run: a length scan writes the plan's own records, not lent step buffers");
        if (image_dev || iang_dev)
            return fail_arg("rt_hip_plan_run: a run with the length scan on takes no image and no I_ang buffer");
    }
    if (p->n_seed > 0) {
        if (!step || p->path_on)
            return fail_arg("rt_hip_plan_run: the plan holds a seed set, which runs in step mode only");
        if (lent)
            return fail_arg("rt_hip_plan_run: a seed set writes the plan's own records, not lent step buffers");
        if (image_dev || iang_dev)
            return fail_arg("rt_hip_plan_run: a run with a seed set takes no image and no I_ang buffer");
    }
    // the records this run leaves (a seed set, ASE seeds, a length scan, a scan with its seeds): all in one allocation of the plan
    const RecordSet recs = plan_record_set(p);
    const RowSet rows    = plan_row_set(p); // ... and the rows, of a per-ray spectra run (ROWS_NONE: of no other)
    const int n_rec      = recs.n_rec();
    double *primary      = nullptr; // the record rt_hip_plan_fetch and fetch_step serve: seed 0's or the ASE record, of all N lengths
    if (n_rec > 0) {
        const rt::DevBeam &B = p->P.beam;
        // (the spare cells of the one-point-axis case: rt_multi.hip, multi_step's buffer)
        const size_t ang_off = nf_off + (size_t) B.nx * (size_t) B.ny + ((B.nx < 2 || B.ny < 2) ? (size_t) B.nx + 2 : 0);
        const size_t stride  = align_up((ang_off + p->n_iang + ((B.na < 2 || B.nb < 2) ? (size_t) B.na + 2 : 0)) * sizeof(double), 256) / sizeof(double);
        if (!p->recs_dev || p->recs_doubles != stride * (size_t) n_rec) {
            plan_quiesce(p);
            pool_free(p->device, p->recs_dev);
            p->recs_dev     = nullptr;
            p->recs_doubles = 0;
            HIP_TRY(pool_alloc(p->device, (void **) &p->recs_dev, stride * (size_t) n_rec * sizeof(double)));
            p->recs_doubles = stride * (size_t) n_rec;
        }
        p->recs_stride  = stride;
        p->recs_nf_off  = nf_off;
        p->recs_ang_off = ang_off;
        primary         = p->recs_dev + (size_t) recs.primary() * stride;
        iang_dev        = primary + ang_off;
    }
    if (step && !lent && !n_rec && !p->step_dev) {
        // (one row and a cell to spare: on an axis of one grid point the reference's getIndex answers 1 for the coordinate
        // g[0] + d/2 exactly, deposit_index4 of rt_freq.hip likewise)
        p->step_doubles     = nf_off + (size_t) p->P.beam.nx * (size_t) p->P.beam.ny + (size_t) p->P.beam.nx + 2;
        HIP_TRY(pool_alloc(p->device, (void **) &p->step_dev, p->step_doubles * sizeof(double)));
    }
    rt::StepOut step_out = {};
    if (step)
        step_out = lent ? rt::StepOut{ p->step_ev_lent, p->step_nf_lent } : primary ? rt::StepOut{ primary, primary + nf_off } : rt::StepOut{ p->step_dev, p->step_dev + nf_off };
    if (!spectra && !step && !image_dev) {
        if (!p->image_own)
            HIP_TRY(pool_alloc(p->device, (void **) &p->image_own, p->n_image * sizeof(double)));
        image_dev = p->image_own;
    }
    if (!spectra && !iang_dev) {
        if (!p->iang_own)
            HIP_TRY(pool_alloc(p->device, (void **) &p->iang_own, p->n_iang * sizeof(double)));
        iang_dev = p->iang_own;
    }
    int rc = plan_prepare_probe(p);
    if (rc != RT_OK)
        return rc;
    // from here on work is queued: whatever happens below, destroy / quiesce must wait for this queue
    p->queued_stream = stream;
    p->queued        = true;
    if (p->tab_pending) { // tables rewritten by rt_hip_plan_update_gain, possibly on another queue: not read before the pack is done
        if (hipEventQuery(p->tab_ev) == hipSuccess) {
            p->tab_pending = false;
        } else {
            (void) hipGetLastError(); // (hipErrorNotReady)
            HIP_TRY(hipStreamWaitEvent(stream, p->tab_ev, 0));
        }
    }
    // an append of the step history still reads the records and the control block this run zeroes: behind it on the same
    // queue anyway, on another queue after its event
    if (p->hist.pending) {
        if (hipEventQuery(p->hist.ev) == hipSuccess) {
            p->hist.pending = false;
        } else {
            (void) hipGetLastError(); // (hipErrorNotReady)
            if (p->hist.stream != stream)
                HIP_TRY(hipStreamWaitEvent(stream, p->hist.ev, 0));
        }
    }
    if (p->probe_on && p->n_rays)
        HIP_TRY(hipMemsetAsync(p->probe, 0, (size_t) p->n_rays * (sizeof(rt_ray) + 8), stream));
    static_assert(sizeof(rt::DevCtl) % 8 == 0 && alignof(rt::DevCtl) >= 8, "zeroed in 8-byte words");
    // (exclusive mode writes every image row exactly once: its image is not zeroed)
    // (step mode: E_v and nf take the image's place in the zeroing launch, exclusive or not)
    rc = lent ? launch_zero4(stream, step_out.E_v, (size_t) p->P.K * sizeof(double), step_out.nf,
                             (size_t) p->P.beam.nx * (size_t) p->P.beam.ny * sizeof(double), iang_dev, p->n_iang * sizeof(double), p->ctl, sizeof(rt::DevCtl))
         : n_rec ? launch_zero3(stream, p->recs_dev, p->recs_doubles * sizeof(double), nullptr, 0, p->ctl, sizeof(rt::DevCtl))
         : step ? launch_zero3(stream, p->step_dev, p->step_doubles * sizeof(double), iang_dev, p->n_iang * sizeof(double), p->ctl, sizeof(rt::DevCtl))
              : launch_zero3(stream, (p->P.exclusive || spectra) ? nullptr : image_dev, p->n_image * sizeof(double), iang_dev,
                             p->n_iang * sizeof(double), p->ctl, sizeof(rt::DevCtl));
    if (rc != RT_OK)
        return rc;
    p->P.image   = image_dev;
    p->P.iang    = iang_dev;
    if (step)
        p->step = step_out;
    p->P.n_tiles = (unsigned) ((p->n_rays + rt::WAVE - 1) / rt::WAVE);
    if (!p->ring.empty()) {
        const size_t slot = (size_t) (p->runs % (p->ring.size() / 3)) * 3;
        p->ev0            = p->ring[slot];
        p->evm            = p->ring[slot + 1];
        p->ev1            = p->ring[slot + 2];
    }
    p->runs++;

    rc = plan_launch_run(p, stream);
    if (rc != RT_OK)
        return rc;
    p->last_stream = stream;
    p->last_image  = image_dev;
    p->last_iang   = iang_dev;
    p->last_rows   = rows;
    p->lspec_first_done = false;
    p->last_step   = step;
    p->last_step_lent = lent;
    p->last_records = recs;
    p->spec_last   = p->spec_sel;
    p->ran         = true;
    p->queued      = false; // (`ran` + last_stream cover it from here)
    p->repeated    = false;
    p->out_staged  = false;
    return RT_OK;
}

} // extern "C"

// A run with more failing rays than the report holds (RT_N_FAILED_MAX): which of them the kernels let into the report
// is decided by the order in which waves reach the counter of the control block -- two runs of the same rays, let alone
// two partitions of them, report different rays.  After the checking repeat the marks say which rays fail with error
// -2 / -3: the report becomes the first RT_N_FAILED_MAX of them in list order, the rays RayTraceImageCPULoop pushes first
// (RayTraceImageCPU.cpp:32-33).  Fewer marked rays than that (the rest of the count are invalid rays, which carry no
// mark): the report stays as the kernels left it.
static int report_first_marked(rt_hip_plan *p, const std::vector<unsigned char> &bad); // (below: the marks, one byte per ray, to the report)
static int plan_report_first_failed(rt_hip_plan *p)
{
    const size_t n = (size_t) p->n_rays, word = p->bad_word; // (a length scan: a 32-bit word per ray, marked under anything = any byte set)
    if (!p->bad_dev || p->bad_rays < n * word)
        return RT_OK;
    std::vector<unsigned char> bad(n * word);
    HIP_TRY(hipMemcpy(bad.data(), p->bad_dev, n * word, hipMemcpyDeviceToHost));
    if (word > 1) {
        for (size_t t = 0; t < n; t++) {
            unsigned char any = 0;
            for (size_t b = 0; b < word; b++)
                any |= bad[t * word + b];
            bad[t] = any;
        }
    }
    return report_first_marked(p, bad);
}

// ... after a length-spectra run the codes err [L][n] say which rays fail, under any n and with any code (error -1
// included: the rows are the report, nothing was deposited)
// (with the seeds of rt_hip_plan_set_spectra_seeds: err [n_seed][L][n], and after a spectra-mode run with them err [n_seed][n])
static int lspec_report_first_failed(rt_hip_plan *p)
{
    // (... and after one with the seeds of rt_hip_plan_set_spectra_ase_seeds err [1 + n_seed][n]: the ASE block first)
    const size_t n = p->last_rows.n_rays, nb = (size_t) p->last_rows.n_blocks();
    const int32_t *err_dev = rows_out(p).err;
    std::vector<int32_t> err(n * nb);
    if (n * nb && err_dev)
        HIP_TRY(hipMemcpy(err.data(), err_dev, n * nb * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<unsigned char> bad(n, 0);
    for (size_t j = 0; j < nb; j++)
        for (size_t t = 0; t < n; t++)
            bad[t] |= err[j * n + t] != 0;
    return report_first_marked(p, bad);
}

static int report_first_marked(rt_hip_plan *p, const std::vector<unsigned char> &bad)
{
    const size_t n       = bad.size();
    const rt::DevRays &R = p->P.rays;
    std::vector<double> g;
    if (!R.list) {
        g.resize((size_t) R.ngx + (size_t) R.ngy + (size_t) R.nga + (size_t) R.ngb);
        HIP_TRY(hipMemcpy(g.data(), p->grid_dev, g.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    rt_ray first[RT_N_FAILED_MAX];
    int k = 0;
    for (size_t t = 0; t < n && k < RT_N_FAILED_MAX; t++) {
        if (!bad[t])
            continue;
        if (R.list) {
            HIP_TRY(hipMemcpy(&first[k], R.list + t, sizeof(rt_ray), hipMemcpyDeviceToHost));
        } else { // ray t of the grid: ijkm = first + t stride, b fastest (rt_hip_plan_set_ray_grid)
            const long long ijkm = R.first + (long long) t * R.stride;
            const long long m = ijkm % R.ngb, a = (ijkm / R.ngb) % R.nga, j = (ijkm / ((long long) R.ngb * R.nga)) % R.ngy,
                            i = ijkm / ((long long) R.ngb * R.nga * R.ngy);
            first[k].x = (float) g[(size_t) i];
            first[k].y = (float) g[(size_t) R.ngx + (size_t) j];
            first[k].a = (float) g[(size_t) R.ngx + (size_t) R.ngy + (size_t) a];
            first[k].b = (float) g[(size_t) R.ngx + (size_t) R.ngy + (size_t) R.nga + (size_t) m];
        }
        k++;
    }
    if (k == RT_N_FAILED_MAX)
        HIP_TRY(hipMemcpy(p->ctl->failed, first, sizeof(first), hipMemcpyHostToDevice));
    return RT_OK;
}

// Wait for the last run and read the control block behind the chunk counters (failure code, failed rays, statistics);
// a run whose frequency pass reported failing rays is repeated without them first.  `staged`: the outputs that
// travelled behind the kernels (plan_stage_outputs) are still this run's.
static int plan_settle(rt_hip_plan *p, rt::DevCtl &c, bool &staged)
{
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->last_stream));
    history_wait(p); // (an append on another queue: the checking repeat below rewrites what it reads)
    constexpr size_t ctl_tail = offsetof(rt::DevCtl, failure_code), ctl_bytes = sizeof(rt::DevCtl) - ctl_tail;
    auto read_ctl = [&]() {
        return hipMemcpy(reinterpret_cast<unsigned char *>(&c) + ctl_tail, reinterpret_cast<const unsigned char *>(p->ctl) + ctl_tail,
                         ctl_bytes, hipMemcpyDeviceToHost);
    };
    // (outputs that travelled behind the kernels already: plan_stage_outputs)
    staged = p->out_staged && p->out_staging;
    if (staged)
        memcpy(reinterpret_cast<unsigned char *>(&c) + ctl_tail, p->out_staging, ctl_bytes);
    else
        HIP_TRY(read_ctl());
    // rays that failed in the frequency pass have been deposited: repeat the pass without them
    // (not after a spectra run: nothing was deposited, and the per-ray codes say which rays failed)
    if ((c.failure_code & ((1u << 2) | (1u << 3))) && !p->path_on && !p->last_rows.any() && !(p->P.debug & 1u) && !p->repeated) {
        const int rc = plan_repeat_checked(p);
        if (rc != RT_OK)
            return rc;
        p->repeated   = true; // this run's outputs are final; a second fetch must not repeat again
        p->out_staged = staged = false;
        HIP_TRY(read_ctl());
        if (c.n_failed > RT_N_FAILED_MAX) { // more failing rays than the report holds: the first of them in list order
            const int rf = plan_report_first_failed(p);
            if (rf != RT_OK)
                return rf;
            HIP_TRY(read_ctl());
        }
    }
    // length spectra: no repeat (nothing was deposited); more failing rays than the report holds: the first in list order
    // (a spectra-mode run with spectra seeds takes the same rule: a ray that fails under either seed is reported once)
    if (p->last_rows.any() && p->last_rows.kind != ROWS_SPEC && c.n_failed > RT_N_FAILED_MAX && !p->lspec_first_done) {
        const int rf = lspec_report_first_failed(p);
        if (rf != RT_OK)
            return rf;
        p->lspec_first_done = true;
        p->out_staged = staged = false;
        HIP_TRY(read_ctl());
    }
    return RT_OK;
}

int rtr::plan_settle_last_run(rt_hip_plan *p)
{
    rt::DevCtl c;
    bool staged = false;
    return plan_settle(p, c, staged);
}

// ---- the records of the last run (rt_records.h: RecordSet says which blocks there are) ---------------------------------
// Every rt_hip_plan_fetch_*_step / rt_hip_plan_*_step_ptrs pair below is a test of the kind, a test of the index and one
// of these two on the block the index means.
static int record_ptrs(rt_hip_plan *p, int block, double **E_v_dev, double **nf_dev, double **iang_dev)
{
    double *blk = p->recs_dev + (size_t) block * p->recs_stride;
    if (E_v_dev)
        *E_v_dev = blk;
    if (nf_dev)
        *nf_dev = blk + p->recs_nf_off;
    if (iang_dev)
        *iang_dev = blk + p->recs_ang_off;
    return RT_OK;
}
// the code of a block, by the one table that knows which array of the control block a kind's kernel writes (rt_runtime.h)
static unsigned record_code(const rt::DevCtl &c, const RecordSet &R, int block)
{
    // (REC_NONE has the one code of the run, whatever the block: record_code_slot's default at block 0)
    unsigned code = 0;
    memcpy(&code, reinterpret_cast<const unsigned char *>(&c) + sizeof(unsigned) * record_code_slot(R).word(R.kind == REC_NONE ? 0 : block), sizeof(code));
    return code;
}
static int record_fetch(rt_hip_plan *p, int block, double *E_v, double *nf, double *I_ang, unsigned int *code)
{
    rt::DevCtl c;
    bool staged  = false;
    const int rs = plan_settle(p, c, staged); // (a failing run is repeated here as rt_hip_plan_fetch repeats it)
    if (rs != RT_OK)
        return rs;
    const double *blk = p->recs_dev + (size_t) block * p->recs_stride;
    if (E_v)
        HIP_TRY(hipMemcpy(E_v, blk, (size_t) p->P.K * sizeof(double), hipMemcpyDeviceToHost));
    if (nf)
        HIP_TRY(hipMemcpy(nf, blk + p->recs_nf_off, (size_t) p->P.beam.nx * (size_t) p->P.beam.ny * sizeof(double), hipMemcpyDeviceToHost));
    if (I_ang)
        HIP_TRY(hipMemcpy(I_ang, blk + p->recs_ang_off, p->n_iang * sizeof(double), hipMemcpyDeviceToHost));
    if (code)
        *code = record_code(c, p->last_records, block);
    return RT_OK;
}
// every record of the last run through host pointers: row r of each output is block r
static int record_fetch_rows(rt_hip_plan *p, double *E_v, double *nf, double *I_ang, unsigned int *codes)
{
    int rc = RT_OK;
    for (int r = 0; rc == RT_OK && r < p->last_records.n_rec(); r++)
        rc = record_fetch(p, r, E_v ? E_v + (size_t) r * (size_t) p->P.K : nullptr, nf ? nf + (size_t) r * (size_t) p->P.beam.nx * (size_t) p->P.beam.ny : nullptr,
                          I_ang ? I_ang + (size_t) r * p->n_iang : nullptr, codes ? codes + r : nullptr);
    return rc;
}

extern "C" {

int rt_hip_plan_fetch(rt_hip_plan *p, double *image, double *I_ang, unsigned int *failure_code,
                      rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats)
{
    if (!p || !p->ran)
        return fail_arg("rt_hip_plan_fetch: plan has not run");
    if (p->last_rows.lengths() && (image || I_ang))
        return fail_arg("rt_hip_plan_fetch: the last run was a length-spectra run, it has no image (rt_hip_plan_fetch_length_spectra)");
    if (p->last_rows.any() && (image || I_ang))
        return fail_arg("rt_hip_plan_fetch: the last run was a spectra run, it has no image (rt_hip_plan_fetch_spectra)");
    if (p->last_step && image)
        return fail_arg("rt_hip_plan_fetch: the last run was a step run, it has no image (rt_hip_plan_fetch_step)");
    rt::DevCtl c;
    bool staged  = false;
    const int rs = plan_settle(p, c, staged);
    if (rs != RT_OK)
        return rs;
    constexpr size_t ctl_tail = offsetof(rt::DevCtl, failure_code), ctl_bytes = sizeof(rt::DevCtl) - ctl_tail;
    if (staged) {
        const size_t off_ang = align_up(ctl_bytes, 256), off_img = off_ang + align_up(p->n_iang * sizeof(double), 256);
        if (image)
            memcpy(image, p->out_staging + off_img, p->n_image * sizeof(double));
        if (I_ang)
            memcpy(I_ang, p->out_staging + off_ang, p->n_iang * sizeof(double));
    } else {
        if (image)
            HIP_TRY(hipMemcpy(image, p->last_image, p->n_image * sizeof(double), hipMemcpyDeviceToHost));
        if (I_ang)
            HIP_TRY(hipMemcpy(I_ang, p->last_iang, p->n_iang * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (failure_code)
        *failure_code = c.failure_code;
    int nf = (int) (c.n_failed < RT_N_FAILED_MAX ? c.n_failed : RT_N_FAILED_MAX);
    if (nf > max_failed)
        nf = max_failed;
    if (failed_rays)
        for (int i = 0; i < nf; i++)
            failed_rays[i] = c.failed[i];
    if (n_failed)
        *n_failed = failed_rays ? nf : 0;
    if (stats) {
        stats->n_rays     = c.n_rays;
        stats->cell_steps = c.cell_steps;
        stats->n_escaped  = c.n_escaped;
        stats->n_skipped  = c.n_skipped;
        float ms          = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
        stats->kernel_ms = ms;
        HIP_TRY(hipEventElapsedTime(&stats->march_ms, p->ev0, p->evm));
        HIP_TRY(hipEventElapsedTime(&stats->freq_ms, p->evm, p->ev1));
        stats->total_ms  = (float) std::chrono::duration<double, std::milli>(
                              std::chrono::steady_clock::now() - p->t_created).count();
    }
    return RT_OK;
}

int rt_hip_plan_fetch_step(rt_hip_plan *p, double *E_v, double *nf, double *I_ang)
{
    if (!p || !p->ran || !p->last_step)
        return fail_arg("rt_hip_plan_fetch_step: the last run was not a step run");
    rt::DevCtl c;
    bool staged  = false;
    const int rs = plan_settle(p, c, staged); // (a failing run is repeated here as rt_hip_plan_fetch repeats it)
    if (rs != RT_OK)
        return rs;
    const size_t n_pix = (size_t) p->P.beam.nx * (size_t) p->P.beam.ny, n_k = (size_t) p->P.K;
    if (staged) {
        constexpr size_t ctl_bytes = sizeof(rt::DevCtl) - offsetof(rt::DevCtl, failure_code);
        const size_t off_ang = align_up(ctl_bytes, 256), off_img = off_ang + align_up(p->n_iang * sizeof(double), 256);
        const double *s      = reinterpret_cast<const double *>(p->out_staging + off_img);
        if (E_v)
            memcpy(E_v, s, n_k * sizeof(double));
        if (nf)
            memcpy(nf, s + (p->step.nf - p->step.E_v), n_pix * sizeof(double));
        if (I_ang)
            memcpy(I_ang, p->out_staging + off_ang, p->n_iang * sizeof(double));
    } else {
        if (E_v)
            HIP_TRY(hipMemcpy(E_v, p->step.E_v, n_k * sizeof(double), hipMemcpyDeviceToHost));
        if (nf)
            HIP_TRY(hipMemcpy(nf, p->step.nf, n_pix * sizeof(double), hipMemcpyDeviceToHost));
        if (I_ang)
            HIP_TRY(hipMemcpy(I_ang, p->last_iang, p->n_iang * sizeof(double), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

} // extern "C"

// An accessor pair of the C ABI: the kinds of last run it serves (bits by RecordKind), what it says after a run of another
// kind, and what of a first index (seed or record) that the run has not.
struct Accessor {
    unsigned kinds;
    const char *not_kind, *bad_first;
};
constexpr unsigned kind_bit(RecordKind k) { return 1u << k; }
static const Accessor ACC_SEED        = { kind_bit(REC_SEEDS), ": the last run was not a step run with a seed set", ": no such seed in the set of the last run" };
// (on a scan with scan seeds a length alone means seed 0's curve, on a scan with ASE seeds the ASE curve; on a suffix scan n
// is the number of lengths of the run of the LAST n)
static const Accessor ACC_LENGTH      = { kind_bit(REC_SCAN) | kind_bit(REC_SCAN_SEEDS) | kind_bit(REC_SCAN_ASE_SEEDS) | kind_bit(REC_RSCAN) | kind_bit(REC_RSCAN_ASE_SEEDS) |
                                              kind_bit(REC_RSCAN_SEEDS),
                                          ": the last run was not a step run with the length scan on", "" };
static const Accessor ACC_FULL        = { kind_bit(REC_ASE_SEEDS), ": the last run was not a step run of an emission plan with ASE seeds",
                                          ": r must be 0 (ASE) .. n_seed of the last run" };
// (of a length scan or of a suffix scan, as rt_hip_plan_fetch_length_step serves both scans)
static const Accessor ACC_FULL_LENGTH = { kind_bit(REC_SCAN_ASE_SEEDS) | kind_bit(REC_RSCAN_ASE_SEEDS), ": the last run was not a step run of a length scan with ASE seeds",
                                          ": r must be 0 (ASE) .. n_seed of the last run" };
// (of a length scan or of a suffix scan, likewise)
static const Accessor ACC_SEED_LENGTH = { kind_bit(REC_SCAN_SEEDS) | kind_bit(REC_RSCAN_SEEDS), ": the last run was not a step run of a length scan with scan seeds",
                                          ": no such seed among the scan seeds of the last run" };

// The block of the last run that (s, n) means to the accessor `who`, or -1 behind its refusal: the kind, the first index,
// the length.
static int record_block(const rt_hip_plan *p, const char *who, const Accessor &a, int s, int n)
{
    auto fail = [&](const char *what) { return (void) fail_arg((std::string(who) + what).c_str()), -1; };
    if (!p || !(a.kinds & kind_bit(p->last_records.kind)))
        return fail(a.not_kind);
    const RecordSet &R = p->last_records;
    if (R.block(s, 2) < 0) // (every scan has length 2, a kind without lengths takes no notice of it)
        return fail(a.bad_first);
    if (R.block(s, n) < 0)
        return fail(": n must be 2 .. N of the last run");
    return R.block(s, n);
}
static int fetch_at(rt_hip_plan *p, const char *who, const Accessor &a, int s, int n, double *E_v, double *nf, double *I_ang, unsigned int *code)
{
    const int block = record_block(p, who, a, s, n);
    return block < 0 ? RT_ERR_ARG : record_fetch(p, block, E_v, nf, I_ang, code);
}
static int ptrs_at(rt_hip_plan *p, const char *who, const Accessor &a, int s, int n, double **E_v_dev, double **nf_dev, double **iang_dev)
{
    const int block = record_block(p, who, a, s, n);
    return block < 0 ? RT_ERR_ARG : record_ptrs(p, block, E_v_dev, nf_dev, iang_dev);
}

// rt_hip_plan_enable_length_scan and rt_hip_plan_enable_suffix_scan (include/rt_hip.h).  Both are the plan's scan_on: the
// boundary buffer, the records and their accessors are one scan's, run_shape and record_set tell the two apart by the method
// (1: the suffix scan of a backward plan, which never has the length scan on).
static int scan_switch(rt_hip_plan *p, const char *who, bool suffix, int on)
{
    auto fail = [&](const char *what) { return fail_arg((std::string(who) + what).c_str()); };
    if (!p)
        return fail(": NULL plan");
    if (suffix && p->P.method != 1)
        return fail(": the plan's method is not 1 (only the backward march of N lengths begins with the marches of the last n)");
    if (!suffix && !on && suffix_scan(p)) // (on: the method test below refuses it)
        return fail(": the suffix scan is on (rt_hip_plan_enable_suffix_scan switches it off)");
    if (on && p->lspec_on)
        return fail(": length spectra are on (they and a scan of step records exclude each other)");
    if (on) {
        if (!suffix && p->P.method != 2)
            return fail(": the plan's method is not 2 (only the forward march of N lengths holds the marches of fewer)");
        if (p->P.N < 3)
            return fail(": N < 3 (one length: the step record is the scan)");
        if (p->P.N - 1 > RT_N_SCAN_MAX)
            return fail(": more than RT_N_SCAN_MAX lengths");
        if (p->n_seed > 0)
            return fail(!suffix          ? ": the plan holds a seed set (a seed set and a length scan exclude each other)"
                        : p->P.use_emis ? ": the plan holds ASE seeds (ASE seeds and a suffix scan exclude each other)"
                                        : ": the plan holds a seed set (a seed set and a suffix scan exclude each other)");
        if (p->path_on || p->spectra_on)
            return fail(": the path tracer or spectra mode is enabled (the scan runs in step mode only)");
    }
    if ((on != 0) == p->scan_on)
        return RT_OK;
    HIP_TRY(hipSetDevice(p->device));
    if (p->ran) { // the last run keeps its records until it is final (wait, control block, the checking repeat)
        const int rs = plan_settle_last_run(p);
        if (rs != RT_OK)
            return rs;
    }
    plan_quiesce(p);
    p->scan_on = on != 0;
    if (!p->scan_on) { // the boundary states exist only while the scan is on
        pool_free(p->device, p->scan_bnd);
        p->scan_bnd       = nullptr;
        p->scan_bnd_bytes = 0;
        if (p->n_scan_seed > 0) { // ... and so do the seeds of the scan
            p->n_scan_seed = 0;
            (void) hipFree(p->seedset_arena);
            p->seedset_arena = nullptr;
            for (int s = 0; s < RT_N_SEED_MAX; s++)
                p->seed_set[s] = rt::DevSeed{};
            return plan_build_seedset_tabs(p); // (frees the factor tables; a backward plan has none)
        }
    }
    return RT_OK;
}

extern "C" {

int rt_hip_plan_fetch_seed_step(rt_hip_plan *p, int s, double *E_v, double *nf, double *I_ang, unsigned int *failure_code)
{
    return fetch_at(p, "rt_hip_plan_fetch_seed_step", ACC_SEED, s, 0, E_v, nf, I_ang, failure_code);
}
int rt_hip_plan_seed_step_ptrs(rt_hip_plan *p, int s, double **E_v_dev, double **nf_dev, double **iang_dev)
{
    return ptrs_at(p, "rt_hip_plan_seed_step_ptrs", ACC_SEED, s, 0, E_v_dev, nf_dev, iang_dev);
}
int rt_hip_plan_fetch_length_step(rt_hip_plan *p, int n, double *E_v, double *nf, double *I_ang, unsigned int *failure_code)
{
    return fetch_at(p, "rt_hip_plan_fetch_length_step", ACC_LENGTH, 0, n, E_v, nf, I_ang, failure_code);
}
int rt_hip_plan_length_step_ptrs(rt_hip_plan *p, int n, double **E_v_dev, double **nf_dev, double **iang_dev)
{
    return ptrs_at(p, "rt_hip_plan_length_step_ptrs", ACC_LENGTH, 0, n, E_v_dev, nf_dev, iang_dev);
}
int rt_hip_plan_fetch_full_step(rt_hip_plan *p, int r, double *E_v, double *nf, double *I_ang, unsigned int *failure_code)
{
    return fetch_at(p, "rt_hip_plan_fetch_full_step", ACC_FULL, r, 0, E_v, nf, I_ang, failure_code);
}
int rt_hip_plan_full_step_ptrs(rt_hip_plan *p, int r, double **E_v_dev, double **nf_dev, double **iang_dev)
{
    return ptrs_at(p, "rt_hip_plan_full_step_ptrs", ACC_FULL, r, 0, E_v_dev, nf_dev, iang_dev);
}
int rt_hip_plan_fetch_full_length_step(rt_hip_plan *p, int r, int n, double *E_v, double *nf, double *I_ang, unsigned int *failure_code)
{
    return fetch_at(p, "rt_hip_plan_fetch_full_length_step", ACC_FULL_LENGTH, r, n, E_v, nf, I_ang, failure_code);
}
int rt_hip_plan_full_length_step_ptrs(rt_hip_plan *p, int r, int n, double **E_v_dev, double **nf_dev, double **iang_dev)
{
    return ptrs_at(p, "rt_hip_plan_full_length_step_ptrs", ACC_FULL_LENGTH, r, n, E_v_dev, nf_dev, iang_dev);
}
int rt_hip_plan_fetch_seed_length_step(rt_hip_plan *p, int s, int n, double *E_v, double *nf, double *I_ang, unsigned int *failure_code)
{
    return fetch_at(p, "rt_hip_plan_fetch_seed_length_step", ACC_SEED_LENGTH, s, n, E_v, nf, I_ang, failure_code);
}
int rt_hip_plan_seed_length_step_ptrs(rt_hip_plan *p, int s, int n, double **E_v_dev, double **nf_dev, double **iang_dev)
{
    return ptrs_at(p, "rt_hip_plan_seed_length_step_ptrs", ACC_SEED_LENGTH, s, n, E_v_dev, nf_dev, iang_dev);
}

int rt_hip_plan_enable_length_scan(rt_hip_plan *p, int on) { return scan_switch(p, "rt_hip_plan_enable_length_scan", false, on); }
int rt_hip_plan_enable_suffix_scan(rt_hip_plan *p, int on) { return scan_switch(p, "rt_hip_plan_enable_suffix_scan", true, on); }

} // extern "C"

// The seeds every rt_hip_plan_set_*seeds takes, validated: `who` names the entry point in the messages.
static int seeds_validate(const rt_hip_plan *p, const char *who, int n_seed, const rt_seed *seeds)
{
    auto fail = [&](const char *what) { return fail_arg((std::string(who) + what).c_str()); };
    if (n_seed < 0 || n_seed > RT_N_SEED_MAX)
        return fail(": n_seed must be 0 .. RT_N_SEED_MAX");
    if (n_seed > 0 && !seeds)
        return fail(": NULL seeds");
    const int K = p->P.K;
    for (int s = 0; s < n_seed; s++) // (as rt_hip_plan_create validates its seed)
        for (int i = 0; i < 5; i++) {
            if (seeds[s].dim[i] < (i < 4 ? 2 : 1) || !seeds[s].x[i] || !seeds[s].f[i])
                return fail(": incomplete seed table");
            if (i == 4 && seeds[s].dim[4] != K)
                return fail(": seed.dim[4] != beam.nv");
        }
    return RT_OK;
}

// Settles the last run, packs the tables of the seeds into one device block and makes them the plan's seed set
// (owner: a set, the seeds of its scan, or those of its spectra modes); n_seed = 0 removes them.
static int seeds_install(rt_hip_plan *p, int n_seed, const rt_seed *seeds, SeedsOwner owner)
{
    const int Kp = p->P.Kp;
    HIP_TRY(hipSetDevice(p->device));
    if (p->ran) { // the last run keeps its set until it is final (wait, control block, the checking repeat)
        const int rs = plan_settle_last_run(p);
        if (rs != RT_OK)
            return rs;
    }
    plan_quiesce(p);
    // the tables of the set, packed as the arena packs the creation seed's: x[i], f[i], the frequency profile padded to Kp
    std::vector<unsigned char> h;
    size_t off_x[RT_N_SEED_MAX][5], off_f[RT_N_SEED_MAX][5];
    auto put = [&](const double *src, size_t n, size_t n_padded) {
        const size_t off = align_up(h.size(), 256);
        h.resize(off + n_padded * sizeof(double), 0);
        memcpy(h.data() + off, src, n * sizeof(double));
        return off;
    };
    for (int s = 0; s < n_seed; s++)
        for (int i = 0; i < 5; i++) {
            const size_t n = (size_t) seeds[s].dim[i];
            off_x[s][i]    = put(seeds[s].x[i], n, n);
            off_f[s][i]    = put(seeds[s].f[i], n, i == 4 ? (size_t) Kp : n);
        }
    unsigned char *arena = nullptr;
    if (n_seed > 0) {
        HIP_TRY(dev_malloc((void **) &arena, h.size() + 16));
        const hipError_t e = hipMemcpy(arena, h.data(), h.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void) hipFree(arena);
            HIP_TRY(e);
        }
    }
    (void) hipFree(p->seedset_arena);
    p->seedset_arena = arena;
    p->n_seed        = owner == SEEDS_OF_SET ? n_seed : 0;
    p->n_scan_seed   = owner == SEEDS_OF_SCAN ? n_seed : 0;
    p->n_spec_seed   = owner == SEEDS_OF_SPECTRA ? n_seed : 0;
    for (int s = 0; s < RT_N_SEED_MAX; s++) {
        p->seed_set[s] = rt::DevSeed{};
        if (s < n_seed) {
            for (int i = 0; i < 5; i++) {
                p->seed_set[s].x[i]   = reinterpret_cast<const double *>(arena + off_x[s][i]);
                p->seed_set[s].f[i]   = reinterpret_cast<const double *>(arena + off_f[s][i]);
                p->seed_set[s].dim[i] = seeds[s].dim[i];
            }
            p->seed_set[s].f0 = seeds[s].f0;
        }
    }
    return plan_build_seedset_tabs(p);
}

// What an installer of seeds requires of the plan: its flavour -- an emission plan (the seeds are ASE seeds and bring their
// scales) or a seeded one -- and its scans; and the words of its refusals that are its own.
enum ScanNeed { SCANS_OFF, LENGTH_SCAN_ON, SUFFIX_SCAN_ON, SPECTRA_ON, LSPEC_ON };
struct SeedsEntry {
    const char *who;
    bool emission;
    ScanNeed scan;
    const char *with_seed, *no_E0; // the wrong flavour: a seed where none may be (or none where one must be), tables without E0
    const char *noun, *runs;       // the seeds, as the refusals by the plan's scans and output modes name them
    const char *forward = nullptr; // (the seeds of a suffix scan) the installer a forward plan takes in this one's place
};
static const SeedsEntry SET_SEEDS = { "rt_hip_plan_set_seeds", false, SCANS_OFF, ": the plan was created without a seed (a set needs the gain-only mode)", nullptr,
                                      "a seed set", "a set runs" };
static const SeedsEntry SET_SCAN_SEEDS = { "rt_hip_plan_set_scan_seeds", false, LENGTH_SCAN_ON,
                                           ": the plan was created without a seed (scan seeds need the gain-only mode)", nullptr, "scan seeds", nullptr };
// ASE seeds: up to RT_N_SEED_MAX seed beams on an EMISSION plan (include/rt_hip.h).  The seeds travel as a set's do; what
// makes them ASE seeds is the plan: use_emis with n_seed > 0.
static const SeedsEntry SET_ASE_SEEDS = { "rt_hip_plan_set_ase_seeds", true, SCANS_OFF, ": not an emission plan (created without a seed, tables with E0)",
                                          ": not an emission plan (created without a seed, tables with E0)", "ASE seeds", "ASE seeds run" };
// ... of a length scan: they travel as the seeds of a scan do (n_scan_seed); use_emis with n_scan_seed > 0
static const SeedsEntry SET_SCAN_ASE_SEEDS = { "rt_hip_plan_set_scan_ase_seeds", true, LENGTH_SCAN_ON, ": not an emission plan (created without a seed, tables with E0)",
                                               ": not an emission plan (created without a seed, tables with E0)", "ASE seeds", nullptr };
// ... of a suffix scan, on a BACKWARD emission plan: the plan's method says which scan the seeds of a scan belong to
static const SeedsEntry SET_SUFFIX_ASE_SEEDS = { "rt_hip_plan_set_suffix_ase_seeds", true, SUFFIX_SCAN_ON,
                                                 ": the plan was created with a seed (the ASE record needs an emission plan)",
                                                 ": not an emission plan (tables without E0)", nullptr, nullptr, "rt_hip_plan_set_scan_ase_seeds" };
// The seeds of a suffix scan on a SEEDED backward plan: what rt_hip_plan_set_scan_seeds is to the length scan (gain-only, the
// creation seed not among them, the plan's scale); REC_RSCAN_SEEDS, rt_step_rscan_seeds.hip
static const SeedsEntry SET_SUFFIX_SEEDS = { "rt_hip_plan_set_suffix_seeds", false, SUFFIX_SCAN_ON,
                                             ": the plan was created without a seed (an emission plan takes rt_hip_plan_set_suffix_ase_seeds)", nullptr,
                                             nullptr, nullptr, "rt_hip_plan_set_scan_seeds" };

// The seeds of the two spectra modes on a SEEDED plan (rt_hip_plan_set_spectra_seeds): spectra mode or length spectra must be
// on; gain-only, the creation seed not among them, either method; rt_spec_seeds.hip and rt_spec_scan_seeds.hip
static const SeedsEntry SET_SPECTRA_SEEDS = { "rt_hip_plan_set_spectra_seeds", false, SPECTRA_ON,
                                              ": the plan was created without a seed (an emission plan: per-ray spectra with ASE seeds are not built)",
                                              nullptr, "spectra seeds", nullptr };

// ASE seeds of spectra mode on an EMISSION plan (rt_hip_plan_set_spectra_ase_seeds): spectra mode must be on, length spectra off;
// no scales (calc_ray has none); they travel as the spectra seeds do (n_spec_seed) -- what makes them ASE seeds is the plan:
// use_emis with n_spec_seed > 0; rt_spec_ase_seeds.hip
static const SeedsEntry SET_SPECTRA_ASE_SEEDS = { "rt_hip_plan_set_spectra_ase_seeds", true, SPECTRA_ON,
                                                  ": the plan was created with a seed (a seeded plan takes rt_hip_plan_set_spectra_seeds)",
                                                  ": not an emission plan (tables without E0)", "ASE seeds", nullptr };

// ASE seeds of length spectra on an EMISSION plan (rt_hip_plan_set_length_spectra_ase_seeds): length spectra must be on (and so
// spectra mode off); no scales; they travel as the spectra seeds do (n_spec_seed) -- use_emis with n_spec_seed > 0 and length
// spectra on; rt_spec_scan_ase_seeds.hip
static const SeedsEntry SET_LSPEC_ASE_SEEDS = { "rt_hip_plan_set_length_spectra_ase_seeds", true, LSPEC_ON,
                                                ": the plan was created with a seed (a seeded plan takes rt_hip_plan_set_spectra_seeds)",
                                                ": not an emission plan (tables without E0)", "ASE seeds", nullptr };

// The nine rt_hip_plan_set_*seeds: the plan's flavour, its scans, the seeds' tables (before the scans where the scans must be
// off, as each entry point has always ordered them), the install, the scales.
static int seeds_set(rt_hip_plan *p, const SeedsEntry &e, int n_seed, const rt_seed *seeds, const double *scales)
{
    auto fail = [&](const std::string &what) { return fail_arg((e.who + what).c_str()); };
    if (!p)
        return fail(": NULL plan");
    if (e.scan == SPECTRA_ON || e.scan == LSPEC_ON) { // the seeds of the per-ray modes: their own requirements, then the path of every installer
        if (e.emission == (p->P.has_seed != 0))
            return fail(e.with_seed);
        if (e.emission && !p->P.use_emis)
            return fail(e.no_E0);
        if (e.scan == LSPEC_ON && p->spectra_on)
            return fail(": spectra mode is on (a plan in spectra mode takes rt_hip_plan_set_spectra_ase_seeds)");
        if (e.scan == LSPEC_ON && !p->lspec_on)
            return fail(": length spectra are off (rt_hip_plan_enable_length_spectra first)");
        if (e.scan == SPECTRA_ON && e.emission && p->lspec_on) // (the text is older than rt_hip_plan_set_length_spectra_ase_seeds, which takes such a plan)
            return fail(": length spectra are on (per-ray ASE seeds at every length are not built)");
        if (e.scan == SPECTRA_ON && e.emission && !p->spectra_on)
            return fail(": spectra mode is off (rt_hip_plan_enable_spectra first)");
        if (!p->spectra_on && !p->lspec_on)
            return fail(": neither spectra mode nor length spectra are on (rt_hip_plan_enable_spectra or rt_hip_plan_enable_length_spectra first)");
        if (n_seed > RT_N_SEED_MAX)
            return fail(": more than RT_N_SEED_MAX seeds");
        const int rv = seeds_validate(p, e.who, n_seed, seeds);
        if (rv != RT_OK)
            return rv;
        if (n_seed == 0 && p->n_spec_seed == 0) // (nothing to remove: the plan stays as it is)
            return RT_OK;
        return seeds_install(p, n_seed, seeds, SEEDS_OF_SPECTRA);
    }
    if (p->lspec_on)
        return fail(": length spectra are on (they take the creation seed alone)");
    if (e.scan == SUFFIX_SCAN_ON && p->P.method != 1)
        return fail(std::string(": the plan's method is not 1 (a forward plan takes ") + e.forward + ")");
    if (e.emission == (p->P.has_seed != 0))
        return fail(e.with_seed);
    if (e.emission && !p->P.use_emis)
        return fail(e.no_E0);
    if (e.scan == SCANS_OFF) {
        const int rv = seeds_validate(p, e.who, n_seed, seeds);
        if (rv != RT_OK)
            return rv;
        const std::string scan = suffix_scan(p) ? "suffix" : "length";
        if ((e.emission || n_seed > 0) && p->scan_on)
            return fail(": the " + scan + " scan is on (" + e.noun + " and a " + scan + " scan exclude each other)");
        if (n_seed > 0 && (p->path_on || p->spectra_on))
            return fail(std::string(": the path tracer or spectra mode is enabled (") + e.runs + " in step mode only)");
        if (!e.emission && n_seed == 0 && (p->n_scan_seed > 0 || p->n_spec_seed > 0)) // (the seeds of a scan are rt_hip_plan_set_scan_seeds', those of spectra mode rt_hip_plan_set_spectra_seeds': there is no set to remove)
            return RT_OK;
        if (e.emission && n_seed == 0 && p->n_spec_seed > 0) // (likewise the ASE seeds of spectra mode, rt_hip_plan_set_spectra_ase_seeds': no ASE seeds of step mode to remove)
            return RT_OK;
    } else {
        if (e.scan == LENGTH_SCAN_ON && suffix_scan(p))
            return fail(std::string(": the suffix scan is on (it takes no ") + e.noun + ")");
        if (!p->scan_on)
            return fail(e.scan == LENGTH_SCAN_ON ? ": the length scan is off (rt_hip_plan_enable_length_scan first)"
                                                 : ": the suffix scan is off (rt_hip_plan_enable_suffix_scan first)");
        if (e.scan == SUFFIX_SCAN_ON && e.emission && n_seed > RT_N_SEED_MAX)
            return fail(": more than RT_N_SEED_MAX seeds");
        if (e.scan == SUFFIX_SCAN_ON && p->n_seed > 0) // (no call leads here: every installer of a set or of ASE seeds refuses a plan whose suffix scan is on)
            return fail(": the plan holds ASE seeds or a seed set (they and a suffix scan exclude each other)");
        const int rv = seeds_validate(p, e.who, n_seed, seeds);
        if (rv != RT_OK)
            return rv;
    }
    const int rc = seeds_install(p, n_seed, seeds, e.scan != SCANS_OFF ? SEEDS_OF_SCAN : SEEDS_OF_SET);
    if (rc != RT_OK || !e.emission)
        return rc;
    for (int s = 0; s < RT_N_SEED_MAX; s++)
        p->ase_scale[s] = (s < n_seed && scales) ? scales[s] : p->P.scale;
    return RT_OK;
}

extern "C" {

int rt_hip_plan_set_seeds(rt_hip_plan *p, int n_seed, const rt_seed *seeds) { return seeds_set(p, SET_SEEDS, n_seed, seeds, nullptr); }
int rt_hip_plan_set_scan_seeds(rt_hip_plan *p, int n_seed, const rt_seed *seeds) { return seeds_set(p, SET_SCAN_SEEDS, n_seed, seeds, nullptr); }
int rt_hip_plan_set_ase_seeds(rt_hip_plan *p, int n_seed, const rt_seed *seeds, const double *scales)
{
    return seeds_set(p, SET_ASE_SEEDS, n_seed, seeds, scales);
}
int rt_hip_plan_set_scan_ase_seeds(rt_hip_plan *p, int n_seed, const rt_seed *seeds, const double *scales)
{
    return seeds_set(p, SET_SCAN_ASE_SEEDS, n_seed, seeds, scales);
}
int rt_hip_plan_set_suffix_ase_seeds(rt_hip_plan *p, int n_seed, const rt_seed *seeds, const double *scales)
{
    return seeds_set(p, SET_SUFFIX_ASE_SEEDS, n_seed, seeds, scales);
}

int rt_hip_plan_set_suffix_seeds(rt_hip_plan *p, int n_seed, const rt_seed *seeds) { return seeds_set(p, SET_SUFFIX_SEEDS, n_seed, seeds, nullptr); }
int rt_hip_plan_set_spectra_seeds(rt_hip_plan *p, int n_seed, const rt_seed *seeds) { return seeds_set(p, SET_SPECTRA_SEEDS, n_seed, seeds, nullptr); }
int rt_hip_plan_set_spectra_ase_seeds(rt_hip_plan *p, int n_seed, const rt_seed *seeds)
{
    return seeds_set(p, SET_SPECTRA_ASE_SEEDS, n_seed, seeds, nullptr);
}

int rt_hip_plan_set_length_spectra_ase_seeds(rt_hip_plan *p, int n_seed, const rt_seed *seeds)
{
    return seeds_set(p, SET_LSPEC_ASE_SEEDS, n_seed, seeds, nullptr);
}

int rt_hip_plan_kernel_ms(rt_hip_plan *p, float *ms)
{
    if (!p || !p->ran || !ms)
        return fail_arg("rt_hip_plan_kernel_ms: plan has not run");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipEventSynchronize(p->ev1));
    HIP_TRY(hipEventElapsedTime(ms, p->ev0, p->ev1));
    return RT_OK;
}

int rt_hip_plan_set_timing_ring(rt_hip_plan *p, int n_runs)
{
    if (!p || n_runs < 1 || n_runs > 4096)
        return fail_arg("rt_hip_plan_set_timing_ring: 1 .. 4096 runs");
    HIP_TRY(hipSetDevice(p->device));
    plan_quiesce(p);
    if (p->ring.empty()) { // the plan's own triple becomes slot 0
        p->ring = { p->ev0, p->evm, p->ev1 };
    }
    while (p->ring.size() < (size_t) n_runs * 3) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreate(&e));
        p->ring.push_back(e);
    }
    while (p->ring.size() > (size_t) n_runs * 3) {
        (void) hipEventDestroy(p->ring.back());
        p->ring.pop_back();
    }
    p->ev0  = p->ring[0];
    p->evm  = p->ring[1];
    p->ev1  = p->ring[2];
    p->runs = 0;
    p->ran  = false;
    return RT_OK;
}

int rt_hip_plan_ring_times(rt_hip_plan *p, float *march_ms, float *freq_ms, int max_runs, int *n_runs)
{
    if (!p || !march_ms || !freq_ms || !n_runs || max_runs < 0)
        return fail_arg("rt_hip_plan_ring_times: bad argument");
    *n_runs = 0;
    if (!p->ran || p->ring.empty())
        return RT_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->last_stream));
    const unsigned long long slots = p->ring.size() / 3;
    const unsigned long long have  = p->runs < slots ? p->runs : slots;
    const unsigned long long take  = have < (unsigned long long) max_runs ? have : (unsigned long long) max_runs;
    for (unsigned long long i = 0; i < take; i++) { // oldest first
        const size_t slot = (size_t) ((p->runs - take + i) % slots) * 3;
        HIP_TRY(hipEventElapsedTime(&march_ms[i], p->ring[slot], p->ring[slot + 1]));
        HIP_TRY(hipEventElapsedTime(&freq_ms[i], p->ring[slot + 1], p->ring[slot + 2]));
    }
    *n_runs = (int) take;
    return RT_OK;
}

int rt_hip_plan_kernel_times(rt_hip_plan *p, float *march_ms, float *freq_ms)
{
    if (!p || !p->ran || !march_ms || !freq_ms)
        return fail_arg("rt_hip_plan_kernel_times: plan has not run");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipEventSynchronize(p->ev1));
    HIP_TRY(hipEventElapsedTime(march_ms, p->ev0, p->evm));
    HIP_TRY(hipEventElapsedTime(freq_ms, p->evm, p->ev1));
    // (a step run in one launch is (launch, 0) as include/rt_hip.h states it: what lies between its two last events is
    // the distance of two event records on a queue, ~5 us -- 5 % of a launch of one ray)
    if (p->last_fused && p->last_step)
        *freq_ms = 0.0f;
    return RT_OK;
}

int rt_hip_plan_last_fused(rt_hip_plan *p) { return p && p->ran && p->last_fused ? 1 : 0; }
int rt_hip_plan_last_march_instance(rt_hip_plan *p) { return p && p->ran ? p->last_march_inst : 0; }

double *rt_hip_plan_image_ptr(rt_hip_plan *p) { return p ? p->image_own : nullptr; }
double *rt_hip_plan_iang_ptr(rt_hip_plan *p) { return p ? p->iang_own : nullptr; }

int rt_hip_plan_fetch_probe(rt_hip_plan *p, float *gvl, float *evl, int32_t *ivl, rt_ray *ray2,
                            uint32_t *flags, uint32_t *steps)
{
    if (!p || !p->ran || !p->probe_on || !p->probe)
        return fail_arg("rt_hip_plan_fetch_probe: probe was not enabled for the last run");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->last_stream));
    const size_t n = (size_t) p->n_rays, S = (size_t) p->P.L * RT_N_SUB;
    {
        // the march records themselves are the probe: de-interleave them
        std::vector<unsigned char> h(rt::rec_bytes(n, p->P.rec_stride));
        if (n)
            HIP_TRY(hipMemcpy(h.data(), p->rec, h.size(), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < n; r++) {
            const unsigned char *rec = h.data();
            const rt::RecMeta *mt = reinterpret_cast<const rt::RecMeta *>(rec + rt::rec_meta_off((unsigned) r, (int) S, p->P.rec_stride));
            for (size_t q = 0; q < S; q++) {
                const rt::RecSlot sl = rt::rec_slot(rec, (unsigned) r, p->P.rec_stride, (int) q, (int) S, mt->flags_steps, p->P.method == 1);
                if (gvl)
                    gvl[r * S + q] = sl.g;
                if (evl)
                    evl[r * S + q] = sl.e;
                if (ivl)
                    ivl[r * S + q] = sl.c;
            }
        }
    }
    if (ray2)
        HIP_TRY(hipMemcpy(ray2, p->P.probe.ray2, n * sizeof(rt_ray), hipMemcpyDeviceToHost));
    if (flags)
        HIP_TRY(hipMemcpy(flags, p->P.probe.flags, n * 4, hipMemcpyDeviceToHost));
    if (steps)
        HIP_TRY(hipMemcpy(steps, p->P.probe.steps, n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

} // extern "C"

// What a host-pointer loop asks of its plan beyond one image or one step record: which scan, which seeds, installed how.
struct LoopRecords {
    ScanNeed scan        = SCANS_OFF;
    int n_seed           = 0;       // > 0: seeds[0 .. n_seed) are the seeds of the scan, or
    const rt_seed *seeds = nullptr;
    bool ase             = false;   // ... ASE seeds with `scales` (of the scan, where one is on): an emission plan of its own, no creation seed
    const double *scales = nullptr;
    // E_v, nf and I_ang hold one row per record of the run (rt_records.h: block r is row r), failure_code one code per row
    bool rows() const { return scan != SCANS_OFF || ase; }
};
// step mode, the scan and the seeds of such a loop, on its fresh plan (the plan's entry points refuse what they do not take:
// method, N, the creation seed, the tables of the seeds)
static int loop_records(rt_hip_plan *p, const LoopRecords &o)
{
    int rc = rt_hip_plan_enable_step(p, 1);
    if (rc == RT_OK && o.scan != SCANS_OFF)
        rc = scan_switch(p, o.scan == SUFFIX_SCAN_ON ? "rt_hip_plan_enable_suffix_scan" : "rt_hip_plan_enable_length_scan", o.scan == SUFFIX_SCAN_ON, 1);
    if (rc == RT_OK && o.n_seed > 0)
        rc = seeds_set(p, !o.ase ? (o.scan == SUFFIX_SCAN_ON ? SET_SUFFIX_SEEDS : SET_SCAN_SEEDS) : o.scan == SUFFIX_SCAN_ON ? SET_SUFFIX_ASE_SEEDS : o.scan == LENGTH_SCAN_ON ? SET_SCAN_ASE_SEEDS : SET_ASE_SEEDS,
                       o.n_seed, o.seeds, o.scales);
    return rc;
}
// the argument checks the host-pointer entry points share, in the order every one of them makes its own in
static int loop_check(const char *who, bool beam_ok, bool out_ok, const rt_ray *rays, size_t n_rays, bool seeds_ok = true)
{
    auto fail = [&](const char *what) { return fail_arg((std::string(who) + what).c_str()); };
    if (!beam_ok)
        return fail(": NULL beam");
    if (!out_ok)
        return fail(": NULL output");
    if (!rays && n_rays)
        return fail(": NULL ray list");
    if (n_rays > MAX_LIST_RAYS)
        return fail(": 2^32 - 4096 rays or more: split the call");
    if (!seeds_ok)
        return fail(": n_seed must be 1 .. RT_N_SEED_MAX, with seeds");
    return RT_OK;
}

// Every rt_hip_*_loop of one device: a plan of its own on a queue of its own, one run, the outputs through host pointers.
// image != NULL: the image cube and I_ang; else step mode with E_v, nf and I_ang -- one record, or the rows `o` asks for.
static int host_pointer_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed,
                             int method, const rt_ray *rays, size_t n_rays, double scale, double *image, double *E_v, double *nf,
                             double *I_ang, unsigned int *failure_code, rt_ray *failed_rays, int max_failed,
                             int *n_failed, rt_stats *stats, const LoopRecords &o = LoopRecords())
{
    const bool step = image == nullptr;
    // RT_HIP_TIMING=1: wall-clock split of this call on stderr (diagnostic)
    static const bool timing = getenv("RT_HIP_TIMING") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto lap    = [&](const char *what) {
        if (timing) {
            const auto now = std::chrono::steady_clock::now();
            fprintf(stderr, "  rt_hip_image_loop %-22s %7.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
            t_prev = now;
        }
    };
    // The call's own queue first: the tables travel on it from page-locked staging while the host goes on (grid
    // recognition, the small uploads, the launch), and everything that reads them is launched on it.
    hipStream_t q  = lease_queue(device);
    rt_hip_plan *p = nullptr;
    int rc         = plan_create_on(&p, q, device, N, beam, gain, seed, method, scale);
    if (rc != RT_OK) {
        release_queue(device, q);
        return rc;
    }
    if (step && (rc = loop_records(p, o)) != RT_OK) {
        rt_hip_plan_destroy(p);
        release_queue(device, q);
        return rc;
    }
    // (the seed-factor tables of a seeded plan are filled by a kernel outside this queue: rt_hip_plan_set_ray_grid)
    if (seed && q && hipStreamSynchronize(q) != hipSuccess)
        (void) hipGetLastError();
    lap("plan_create");
    // A list that is a whole tensor grid (what create_image builds) is not uploaded: the device
    // generates the rays while host threads check the list against the grid, ray by ray.  (Not with ASE seeds: their loops
    // upload the list, and their outputs are not staged.)
    GridGuess G;
    bool as_grid = !o.ase && n_rays >= (1u << 16) && !getenv("RT_HIP_NO_GRID_DETECT") && guess_ray_grid(rays, n_rays, G);
    lap("guess grid");
    if (as_grid) {
        rc = plan_set_guessed_grid(p, G, 0, (int64_t) n_rays);
        lap("set_ray_grid");
        if (rc == RT_OK)
            rc = rt_hip_plan_run(p, q, nullptr, nullptr); // asynchronous
        if (rc == RT_OK)
            plan_stage_outputs(p);
        lap(p->last_fused ? "run (one launch)" : "run (two launches)");
        if (rc == RT_OK && !verify_ray_grid(rays, n_rays, G, host_threads(16))) {
            as_grid = false; // not that grid after all: the speculative result is discarded below
            plan_quiesce(p);
        }
        lap("verify list");
    }
    if (rc == RT_OK && !as_grid) {
        rc = plan_set_rays_deferred(p, rays, n_rays);
        if (rc == RT_OK)
            rc = rt_hip_plan_run(p, q, nullptr, nullptr);
        if (rc == RT_OK && !o.ase)
            plan_stage_outputs(p);
    }
    if (rc == RT_OK)
        rc = rt_hip_plan_fetch(p, image, step ? nullptr : I_ang, o.rows() ? nullptr : failure_code, failed_rays, max_failed, n_failed, stats);
    if (rc == RT_OK && step)
        rc = o.rows() ? record_fetch_rows(p, E_v, nf, I_ang, failure_code) : rt_hip_plan_fetch_step(p, E_v, nf, I_ang);
    lap("fetch (wait + D2H)");
    rt_hip_plan_destroy(p); // waits for whatever is still in flight
    release_queue(device, q);
    lap("destroy");
    return rc;
}

extern "C" {

int rt_hip_image_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed,
                      int method, const rt_ray *rays, size_t n_rays, double scale, double *image,
                      double *I_ang, unsigned int *failure_code, rt_ray *failed_rays, int max_failed,
                      int *n_failed, rt_stats *stats)
{
    const int rc = loop_check("rt_hip_image_loop", true, image && I_ang, rays, n_rays);
    return rc != RT_OK ? rc : host_pointer_loop(device, N, beam, gain, seed, method, rays, n_rays, scale, image, nullptr, nullptr, I_ang, failure_code,
                                                failed_rays, max_failed, n_failed, stats);
}

int rt_hip_step_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                     const rt_ray *rays, size_t n_rays, double scale, double *E_v, double *nf, double *I_ang,
                     unsigned int *failure_code, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats)
{
    const int rc = loop_check("rt_hip_step_loop", true, E_v && nf && I_ang, rays, n_rays);
    return rc != RT_OK ? rc : host_pointer_loop(device, N, beam, gain, seed, method, rays, n_rays, scale, nullptr, E_v, nf, I_ang, failure_code,
                                                failed_rays, max_failed, n_failed, stats);
}

// The loops that return rows.  Of a scan: one row per length n = 2 .. N, with its seeds once per seed, [n_seed][N - 1][...].
// With ASE seeds (seed == NULL): row 0 of every output is the ASE record, row 1 + s seed s; of a scan the rows
// [1 + n_seed][N - 1][...], the ASE curve first.  with_seeds: the entry point takes seeds, 1 .. RT_N_SEED_MAX of them.
static int rows_loop(const char *who, const LoopRecords &o, bool with_seeds, int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed,
                     int method, const rt_ray *rays, size_t n_rays, double scale, double *E_v, double *nf, double *I_ang, unsigned int *failure_codes,
                     rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats)
{
    const int rc = loop_check(who, beam != nullptr, !o.ase || (E_v && nf && I_ang), rays, n_rays,
                              !with_seeds || (o.n_seed >= 1 && o.n_seed <= RT_N_SEED_MAX && o.seeds));
    return rc != RT_OK ? rc : host_pointer_loop(device, N, beam, gain, seed, method, rays, n_rays, scale, nullptr, E_v, nf, I_ang, failure_codes,
                                                failed_rays, max_failed, n_failed, stats, o);
}

int rt_hip_length_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                            const rt_ray *rays, size_t n_rays, double scale, double *E_v, double *nf, double *I_ang,
                            unsigned int *failure_codes, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats)
{
    return rows_loop("rt_hip_length_scan_loop", LoopRecords{ LENGTH_SCAN_ON }, false, device, N, beam, gain, seed, method, rays, n_rays, scale, E_v, nf, I_ang,
                     failure_codes, failed_rays, max_failed, n_failed, stats);
}

int rt_hip_suffix_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                            const rt_ray *rays, size_t n_rays, double scale, double *E_v, double *nf, double *I_ang,
                            unsigned int *failure_codes, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats)
{
    return rows_loop("rt_hip_suffix_scan_loop", LoopRecords{ SUFFIX_SCAN_ON }, false, device, N, beam, gain, seed, method, rays, n_rays, scale, E_v, nf, I_ang,
                     failure_codes, failed_rays, max_failed, n_failed, stats);
}

int rt_hip_seed_length_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                                 const rt_ray *rays, size_t n_rays, double scale, int n_seed, const rt_seed *seeds, double *E_v, double *nf,
                                 double *I_ang, unsigned int *failure_codes, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats)
{
    return rows_loop("rt_hip_seed_length_scan_loop", LoopRecords{ LENGTH_SCAN_ON, n_seed, seeds }, true, device, N, beam, gain, seed, method, rays, n_rays,
                     scale, E_v, nf, I_ang, failure_codes, failed_rays, max_failed, n_failed, stats);
}

int rt_hip_seed_suffix_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                                 const rt_ray *rays, size_t n_rays, double scale, int n_seed, const rt_seed *seeds, double *E_v, double *nf,
                                 double *I_ang, unsigned int *failure_codes, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats)
{
    return rows_loop("rt_hip_seed_suffix_scan_loop", LoopRecords{ SUFFIX_SCAN_ON, n_seed, seeds }, true, device, N, beam, gain, seed, method, rays, n_rays,
                     scale, E_v, nf, I_ang, failure_codes, failed_rays, max_failed, n_failed, stats);
}

int rt_hip_full_step_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, int method, const rt_ray *rays, size_t n_rays,
                          double scale, int n_seed, const rt_seed *seeds, const double *scales, double *E_v, double *nf, double *I_ang,
                          unsigned int *failure_codes, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats)
{
    return rows_loop("rt_hip_full_step_loop", LoopRecords{ SCANS_OFF, n_seed, seeds, true, scales }, true, device, N, beam, gain, nullptr, method, rays,
                     n_rays, scale, E_v, nf, I_ang, failure_codes, failed_rays, max_failed, n_failed, stats);
}

int rt_hip_full_length_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, int method, const rt_ray *rays, size_t n_rays,
                                 double scale, int n_seed, const rt_seed *seeds, const double *scales, double *E_v, double *nf, double *I_ang,
                                 unsigned int *failure_codes, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats)
{
    return rows_loop("rt_hip_full_length_scan_loop", LoopRecords{ LENGTH_SCAN_ON, n_seed, seeds, true, scales }, true, device, N, beam, gain, nullptr, method,
                     rays, n_rays, scale, E_v, nf, I_ang, failure_codes, failed_rays, max_failed, n_failed, stats);
}

int rt_hip_full_suffix_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, int method, const rt_ray *rays, size_t n_rays,
                                 double scale, int n_seed, const rt_seed *seeds, const double *scales, double *E_v, double *nf, double *I_ang,
                                 unsigned int *failure_codes, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats)
{
    return rows_loop("rt_hip_full_suffix_scan_loop", LoopRecords{ SUFFIX_SCAN_ON, n_seed, seeds, true, scales }, true, device, N, beam, gain, nullptr, method,
                     rays, n_rays, scale, E_v, nf, I_ang, failure_codes, failed_rays, max_failed, n_failed, stats);
}

int rt_hip_calc_rays(int device, int N, double dz, const rt_gain *gain, const rt_seed *seed, int K, int method, const double *rays,
                     size_t n, double *Iv, double *ray2, int32_t *err, rt_stats *stats)
{
    if (!gain || K < 1)
        return fail_arg("rt_hip_calc_rays: NULL gain tables or K < 1");
    if (!rays && n)
        return fail_arg("rt_hip_calc_rays: NULL ray list");
    if (n > MAX_LIST_RAYS)
        return fail_arg("rt_hip_calc_rays: 2^32 - 4096 rays or more: split the call");
    if (stats)
        memset(stats, 0, sizeof(*stats));
    if (n == 0)
        return RT_OK;
    const auto t_start = std::chrono::steady_clock::now();
    // calc_ray has no beam: a one-cell stand-in carries dz and K (the spectra kernel reads neither grids nor dv)
    const double zero = 0.0;
    std::vector<double> dv((size_t) K, 0.0);
    rt_beam beam;
    memset(&beam, 0, sizeof(beam));
    beam.nx = beam.ny = beam.na = beam.nb = 1;
    beam.nv = K;
    beam.dx = beam.dy = beam.da = beam.db = 1.0;
    beam.dz = dz;
    beam.x = beam.y = beam.a = beam.b = &zero;
    beam.dv = dv.data();
    // rays per chunk: the spectra of a chunk take at most 1 GiB of device memory, whole 64-ray tiles
    // (RT_HIP_CALC_RAYS_CHUNK: rays per chunk, for tests of the chunked path)
    size_t chunk = ((size_t) 1 << 30) / ((size_t) K * sizeof(double)) / 64 * 64;
    chunk        = chunk < 64 ? 64 : chunk;
    chunk        = (size_t) env_unsigned("RT_HIP_CALC_RAYS_CHUNK", (unsigned) (chunk > 0xffffff00ull ? 0xffffff00ull : chunk), 1, 0xffffff00u);
    const bool overlap = env_unsigned("RT_HIP_CALC_RAYS_OVERLAP", 1, 0, 1) == 1; // 0: download a chunk before the next one starts (A/B)
    hipStream_t q  = lease_queue(device);
    rt_hip_plan *p = nullptr;
    int rc         = plan_create_on(&p, nullptr, device, N, &beam, gain, seed, method, 1.0);
    if (rc != RT_OK) {
        release_queue(device, q);
        return rc;
    }
    rc = rt_hip_plan_enable_spectra(p, 1);
    std::vector<rt_ray> list, exit_rays[2];
    std::thread download;
    int rc_down[2] = { RT_OK, RT_OK };
    std::string err_down[2];
    // chunk c of the outputs, device -> caller, on a thread of its own: blocking copies do not wait for the run's queue
    auto fetch_chunk = [&](unsigned set, size_t begin, size_t count) {
        const rt::SpecOut o = p->spec[set];
        rc_down[set]        = [&]() {
            HIP_TRY(hipSetDevice(device));
            if (Iv)
                HIP_TRY(hipMemcpy(Iv + begin * (size_t) K, o.Iv, count * (size_t) K * sizeof(double), hipMemcpyDeviceToHost));
            if (err)
                HIP_TRY(hipMemcpy(err + begin, o.err, count * sizeof(int32_t), hipMemcpyDeviceToHost));
            if (ray2) {
                exit_rays[set].resize(count);
                HIP_TRY(hipMemcpy(exit_rays[set].data(), o.ray2, count * sizeof(rt_ray), hipMemcpyDeviceToHost));
                for (size_t r = 0; r < count; r++) {
                    const rt_ray &e = exit_rays[set][r];
                    double *d       = ray2 + 4 * (begin + r);
                    d[0] = e.x, d[1] = e.y, d[2] = e.a, d[3] = e.b;
                }
            }
            return (int) RT_OK;
        }();
        if (rc_down[set] != RT_OK)
            err_down[set] = last_error(); // (the error text is per thread)
    };
    unsigned set = 0;
    for (size_t begin = 0; begin < n && rc == RT_OK; begin += chunk, set ^= 1u) {
        const size_t count = n - begin < chunk ? n - begin : chunk;
        list.resize(count);
        for (size_t r = 0; r < count; r++) { // RayTraceImage.cpp:195-199: the coordinates are rounded to float
            const double *s = rays + 4 * (begin + r);
            list[r]         = rt_ray{ (float) s[0], (float) s[1], (float) s[2], (float) s[3] };
        }
        rc = rt_hip_plan_set_rays(p, list.data(), count);
        p->spec_sel = set;
        if (rc == RT_OK)
            rc = rt_hip_plan_run(p, q, nullptr, nullptr); // asynchronous: the previous chunk is still on its way down
        if (download.joinable())
            download.join();
        rt_stats st;
        unsigned int code = 0;
        if (rc == RT_OK)
            rc = rt_hip_plan_fetch(p, nullptr, nullptr, &code, nullptr, 0, nullptr, &st); // waits for the run
        if (rc == RT_OK && stats) {
            stats->n_rays += st.n_rays;
            stats->cell_steps += st.cell_steps;
            stats->n_escaped += st.n_escaped;
            stats->n_skipped += st.n_skipped;
            stats->kernel_ms += st.kernel_ms;
            stats->march_ms += st.march_ms;
            stats->freq_ms += st.freq_ms;
        }
        if (rc == RT_OK) {
            download = std::thread(fetch_chunk, set, begin, count);
            if (!overlap)
                download.join();
        }
    }
    if (download.joinable())
        download.join();
    for (unsigned d = 0; d < 2 && rc == RT_OK; d++) {
        if (rc_down[d] != RT_OK) {
            rc           = rc_down[d];
            last_error() = err_down[d];
        }
    }
    rt_hip_plan_destroy(p);
    release_queue(device, q);
    if (stats)
        stats->total_ms = (float) std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return rc;
}

void rt_hip_pool_trim(void) { pool_trim_all(); }

} // extern "C"
