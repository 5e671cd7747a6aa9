// rt_history.hip -- the step history of a time loop: the records of the last step run filed on the device.
//
// What the application does on the host behind every step (intensity_struct::copy_step, RayTraceStructures.cpp:1835-1867;
// intensity_step_struct::valid(), :1647-1682; intensity_step_struct::add, :1579-1602) as two launches on the run's queue:
//   rt_history_append_kernel  every block r of the run's record set at once: E_v, nf and I_ang copied into slab i of the
//                             history (and added to the running sum), the partial sum of nf and the partial flags of every
//                             work-group written to a scratch of the plan;
//   rt_history_finish_kernel  one work-group: the partials of a block added IN INDEX ORDER -> E_sum[r][i], the flags OR-ed,
//                             the block's failure code read from the run's control block, filled[i] = 1.
// Two launches and not one: the sum of a block's partials needs every partial, and the launch boundary is the one hand-off
// that costs no work-group a wait (no flags, no last arriver, no spinning); the second launch is ~2 us on a queue that
// never drains in a time loop.
// Determinism of E_sum: work-group w of a block owns pixels [w CHUNK, (w + 1) CHUNK), thread t of it the pairs t and
// t + 256 of that chunk (pixels 2t, 2t + 1, 512 + 2t, 512 + 2t + 1), added in that order; a wave adds its 64 lanes as a
// fixed tree, thread 0 the four wave sums in wave order, the finish kernel the work-groups' partials in index order.
// Nothing of that depends on the slot, the block, the number of blocks or an address (whether a pair is loaded as one
// 16-byte word or as two doubles is decided by alignment, and changes no operand of any addition).
// A unit of its own (like rt_tables.hip), so that no instance of rt_launch.hip is compiled differently for these kernels.
#include "rt_runtime.h"

#include <cstring>

using namespace rtr;

namespace rt {

constexpr unsigned HIST_WG      = 256;  // threads of a work-group
constexpr unsigned HIST_CHUNK   = 1024; // pixels of nf per work-group: two pairs per thread
constexpr unsigned HIST_AUX_MAX = 16;   // most work-groups per block for E_v and I_ang

struct HistAppend {
    // block r of the run: E_v at ev + r stride, nf and I_ang likewise (a plain step run: one block, stride 0)
    const double *ev, *nf, *ang;
    size_t stride;
    // slab i of block r of the history: h_* + r rec_* (doubles); the running sum: a_* + r arec_* (NULL: not asked for)
    double *h_ev, *h_nf, *h_ang;
    size_t rec_ev, rec_nf, rec_ang;
    double *a_ev, *a_nf, *a_ang;
    size_t arec_ev, arec_nf, arec_ang;
    double *part;    // [n_rec][wg_rec]
    unsigned *pflag; // [n_rec][wg_rec]
    unsigned nv, npix, nab, pix_wg, aux_wg;
    double weight;
};

struct HistFinish {
    const double *part;
    const unsigned *pflag;
    const unsigned *ctl; // the control block of the run as 32-bit words
    unsigned code_base, code_div, code_row; // rtr::CodeSlot
    double *esum;        // + r rec_esum (doubles): E_sum[r][i]
    unsigned *code, *flags; // + r rec_code / rec_flags (words)
    size_t rec_esum, rec_code, rec_flags;
    unsigned char *filled; // filled[i]
    double *acc_esum;      // [n_rec], NULL: not asked for
    unsigned n_rec, wg_rec, pix_wg;
    double weight;
};

// bit 0: negative, bit 1: NaN (intensity_step_struct::valid() asks for either)
__device__ __forceinline__ unsigned hist_flag(double x) { return (x < 0.0 ? 1u : 0u) | (x != x ? 2u : 0u); }

// Elements 2j and 2j + 1 of a span of n doubles: copied from s to d, added to the running sum a (if there is one), flagged;
// x0 / x1 are the values (0 where the span has ended).  vec: s and d are 16-byte aligned, so a whole pair is one 16-byte load
// and one 16-byte store (a is 256-byte aligned always).
__device__ __forceinline__ unsigned hist_pair(const double *__restrict__ s, double *__restrict__ d, double *__restrict__ a, size_t j, size_t n, bool vec,
                                              double w, double &x0, double &x1)
{
    const size_t e = 2 * j;
    x0 = x1 = 0.0;
    if (e >= n)
        return 0u;
    const bool whole = e + 1 < n;
    if (whole && vec) {
        const double2 v = *reinterpret_cast<const double2 *>(s + e);
        x0 = v.x;
        x1 = v.y;
        *reinterpret_cast<double2 *>(d + e) = v;
    } else {
        x0   = s[e];
        d[e] = x0;
        if (whole) {
            x1       = s[e + 1];
            d[e + 1] = x1;
        }
    }
    if (a) { // acc + weight * x, the product rounded first
        if (whole) {
            double2 v = *reinterpret_cast<double2 *>(a + e);
            v.x       = __dadd_rn(v.x, __dmul_rn(w, x0));
            v.y       = __dadd_rn(v.y, __dmul_rn(w, x1));
            *reinterpret_cast<double2 *>(a + e) = v;
        } else
            a[e] = __dadd_rn(a[e], __dmul_rn(w, x0));
    }
    return hist_flag(x0) | (whole ? hist_flag(x1) : 0u);
}

__device__ __forceinline__ bool hist_vec(const void *s, const void *d)
{
    return ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15u) == 0;
}

extern "C" __global__ void __launch_bounds__(HIST_WG) rt_history_append_kernel(const HistAppend A)
{
    __shared__ double wave_sum[HIST_WG / WAVE];
    __shared__ unsigned wg_flag;
    const unsigned wg_rec = A.pix_wg + A.aux_wg;
    const unsigned r = blockIdx.x / wg_rec, w = blockIdx.x % wg_rec, t = threadIdx.x;
    if (t == 0)
        wg_flag = 0u;
    __syncthreads();
    unsigned f = 0u;
    double sum = 0.0;
    if (w < A.pix_wg) { // one chunk of nf
        const size_t base = (size_t) w * HIST_CHUNK; // (a whole number of pairs)
        const size_t n    = (size_t) A.npix - base < HIST_CHUNK ? (size_t) A.npix - base : HIST_CHUNK;
        const double *s   = A.nf + (size_t) r * A.stride + base;
        double *d         = A.h_nf + (size_t) r * A.rec_nf + base;
        double *a         = A.a_nf ? A.a_nf + (size_t) r * A.arec_nf + base : nullptr;
        const bool vec    = hist_vec(s, d);
        double x0, x1, x2, x3;
        f |= hist_pair(s, d, a, t, n, vec, A.weight, x0, x1);
        f |= hist_pair(s, d, a, t + HIST_WG, n, vec, A.weight, x2, x3);
        sum = __dadd_rn(__dadd_rn(__dadd_rn(x0, x1), x2), x3);
    } else { // E_v, then I_ang: pairs handed round the aux work-groups of the block
        const size_t first = (size_t) (w - A.pix_wg) * HIST_WG + t, step = (size_t) A.aux_wg * HIST_WG;
        double x0, x1;
        {
            const double *s = A.ev + (size_t) r * A.stride;
            double *d       = A.h_ev + (size_t) r * A.rec_ev;
            double *a       = A.a_ev ? A.a_ev + (size_t) r * A.arec_ev : nullptr;
            const bool vec  = hist_vec(s, d);
            for (size_t j = first; 2 * j < A.nv; j += step)
                f |= hist_pair(s, d, a, j, A.nv, vec, A.weight, x0, x1);
        }
        {
            const double *s = A.ang + (size_t) r * A.stride;
            double *d       = A.h_ang + (size_t) r * A.rec_ang;
            double *a       = A.a_ang ? A.a_ang + (size_t) r * A.arec_ang : nullptr;
            const bool vec  = hist_vec(s, d);
            for (size_t j = first; 2 * j < A.nab; j += step)
                f |= hist_pair(s, d, a, j, A.nab, vec, A.weight, x0, x1);
        }
    }
    // the wave's 64 sums as a fixed tree (every lane ends with the same double), the four waves in wave order
    for (int o = WAVE / 2; o > 0; o >>= 1)
        sum = __dadd_rn(sum, __shfl_xor(sum, o, WAVE));
    if ((t & (WAVE - 1)) == 0)
        wave_sum[t / WAVE] = sum;
    if (f)
        atomicOr(&wg_flag, f); // (LDS; an integer OR has no order)
    __syncthreads();
    if (t == 0) {
        double s = wave_sum[0];
        for (unsigned k = 1; k < HIST_WG / WAVE; k++)
            s = __dadd_rn(s, wave_sum[k]);
        A.part[(size_t) r * wg_rec + w]  = s;
        A.pflag[(size_t) r * wg_rec + w] = wg_flag;
    }
}

extern "C" __global__ void __launch_bounds__(HIST_WG) rt_history_finish_kernel(const HistFinish F)
{
    for (unsigned r = threadIdx.x; r < F.n_rec; r += HIST_WG) {
        const double *p   = F.part + (size_t) r * F.wg_rec;
        const unsigned *q = F.pflag + (size_t) r * F.wg_rec;
        double s   = p[0]; // (pix_wg >= 1)
        unsigned f = q[0];
        for (unsigned w = 1; w < F.pix_wg; w++)
            s = __dadd_rn(s, p[w]);
        for (unsigned w = 1; w < F.wg_rec; w++)
            f |= q[w];
        F.esum[(size_t) r * F.rec_esum]   = s;
        F.flags[(size_t) r * F.rec_flags] = f;
        F.code[(size_t) r * F.rec_code]   = F.ctl[F.code_base + (r / F.code_div) * F.code_row + r % F.code_div];
        if (F.acc_esum)
            F.acc_esum[r] = __dadd_rn(F.acc_esum[r], __dmul_rn(F.weight, s));
    }
    if (threadIdx.x == 0)
        *F.filled = 1;
}

} // namespace rt

namespace {

constexpr unsigned long long up(unsigned long long v, unsigned long long a) { return (v + a - 1) / a * a; }

// The layout of a history and the shape of its two launches; `facts` validated by the caller.
void history_layout(const rt_hip_history_facts &f, rt_hip_history_layout &L)
{
    const unsigned size = L.size;
    memset(&L, 0, sizeof(L));
    L.size = size;
    const unsigned long long nv = (unsigned long long) f.nv, npix = (unsigned long long) f.nx * (unsigned long long) f.ny,
                             nab = (unsigned long long) f.na * (unsigned long long) f.nb, R = (unsigned long long) f.n_rec,
                             T = (unsigned long long) f.n_steps;
    L.chunk      = rt::HIST_CHUNK;
    L.wg_threads = rt::HIST_WG;
    L.pix_wg     = (unsigned) ((npix + rt::HIST_CHUNK - 1) / rt::HIST_CHUNK);
    const unsigned long long aux = (nv + nab + rt::HIST_CHUNK - 1) / rt::HIST_CHUNK;
    L.aux_wg     = (unsigned) (aux < 1 ? 1 : aux > rt::HIST_AUX_MAX ? rt::HIST_AUX_MAX : aux);
    L.wg_per_rec = L.pix_wg + L.aux_wg;
    L.grid       = (unsigned) R * L.wg_per_rec;
    unsigned long long o = 0;
    auto block = [&](unsigned long long &off, unsigned long long &rec, unsigned long long bytes_per_rec, unsigned long long align) {
        off = o;
        rec = up(bytes_per_rec, align);
        o += rec * R;
    };
    // the record-shaped arrays: every block of every array at a 256-byte boundary, the slabs of a block back to back
    L.step_E_v   = nv * 8;
    L.step_nf    = npix * 8;
    L.step_I_ang = nab * 8;
    block(L.off_E_v, L.rec_E_v, T * L.step_E_v, 256);
    block(L.off_nf, L.rec_nf, T * L.step_nf, 256);
    block(L.off_I_ang, L.rec_I_ang, T * L.step_I_ang, 256);
    if (f.accumulate) {
        block(L.off_acc_E_v, L.rec_acc_E_v, L.step_E_v, 256);
        block(L.off_acc_nf, L.rec_acc_nf, L.step_nf, 256);
        block(L.off_acc_I_ang, L.rec_acc_I_ang, L.step_I_ang, 256);
        L.off_acc_E_sum = o;
        o += up(R * 8, 256);
    }
    block(L.off_E_sum, L.rec_E_sum, T * 8, 8);
    block(L.off_code, L.rec_code, T * 4, 8);
    block(L.off_flags, L.rec_flags, T * 4, 8);
    L.off_filled = o;
    o += up(T, 256);
    // scratch of the partials
    L.off_part  = o;
    o += up(R * L.wg_per_rec * 8, 8);
    L.off_pflag = o;
    o += up(R * L.wg_per_rec * 4, 256);
    L.scratch_bytes = o - L.off_part;
    L.bytes         = o;
}

const char *facts_error(const rt_hip_history_facts &f)
{
    if (f.nv < 1 || f.nx < 1 || f.ny < 1 || f.na < 1 || f.nb < 1)
        return "a beam size below 1";
    if (f.n_rec < 1 || f.n_steps < 1)
        return "n_rec or n_steps below 1";
    // (the launch: n_rec wg_per_rec work-groups in 32 bits, far below the grid limit)
    const unsigned long long wg = ((unsigned long long) f.nx * (unsigned long long) f.ny + rt::HIST_CHUNK - 1) / rt::HIST_CHUNK + rt::HIST_AUX_MAX;
    if (wg * (unsigned long long) f.n_rec > 0x7fffffffull)
        return "more work-groups than a launch takes";
    return nullptr;
}

// what the history is bound to against the last run of the plan
bool same_binding(const History &h, const rt_hip_plan *p)
{
    const RecordSet &a = h.recs, &b = p->last_records;
    const rt::DevBeam &B = p->P.beam;
    return a.kind == b.kind && a.n_seed == b.n_seed && a.L == b.L && h.nv == p->P.K && h.nx == B.nx && h.ny == B.ny && h.na == B.na && h.nb == B.nb;
}

template <class T> T *at(const History &h, unsigned long long off) { return reinterpret_cast<T *>(h.dev + off); }

int fetch_rows(const void *src, void *dst, size_t bytes)
{
    if (dst && bytes)
        HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

} // namespace

void rtr::history_wait(rt_hip_plan *p)
{
    if (!p || !p->hist.pending)
        return;
    if (hipEventSynchronize(p->hist.ev) != hipSuccess)
        (void) hipGetLastError();
    p->hist.pending = false;
}

void rtr::history_release(rt_hip_plan *p)
{
    if (!p)
        return;
    history_wait(p);
    History &h = p->hist;
    if (h.ev)
        (void) hipEventDestroy(h.ev);
    pool_free(p->device, h.dev);
    h = History{};
}

extern "C" {

int rt_hip_debug_history_layout(const rt_hip_history_facts *facts, rt_hip_history_layout *out)
{
    if (!facts || !out || facts->size != sizeof(rt_hip_history_facts) || out->size != sizeof(rt_hip_history_layout))
        return fail_arg("rt_hip_debug_history_layout: NULL argument or a size field that is not this library's sizeof");
    if (const char *e = facts_error(*facts))
        return fail_arg((std::string("rt_hip_debug_history_layout: ") + e).c_str());
    history_layout(*facts, *out);
    return RT_OK;
}

int rt_hip_plan_history_create(rt_hip_plan *p, int n_steps)
{
    if (!p)
        return fail_arg("rt_hip_plan_history_create: NULL plan");
    if (n_steps < 0)
        return fail_arg("rt_hip_plan_history_create: n_steps < 0");
    HIP_TRY(hipSetDevice(p->device));
    history_release(p);
    p->hist.n_steps = n_steps;
    p->hist.filled.assign((size_t) n_steps, 0);
    return RT_OK;
}

int rt_hip_plan_history_append(rt_hip_plan *p, int step, double weight, int accumulate, void *stream_v)
{
    if (!p)
        return fail_arg("rt_hip_plan_history_append: NULL plan");
    History &h = p->hist;
    if (h.n_steps < 1)
        return fail_arg("rt_hip_plan_history_append: the plan has no history (rt_hip_plan_history_create)");
    if (!p->ran || !p->last_step)
        return fail_arg("rt_hip_plan_history_append: the last run was not a step run");
    if (step < 0 || step >= h.n_steps)
        return fail_arg("rt_hip_plan_history_append: step must be 0 .. n_steps - 1");
    if (h.bound && !same_binding(h, p))
        return fail_arg("rt_hip_plan_history_append: the record set or the beam sizes of the last run are not the ones the history is bound to");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t stream = stream_v ? reinterpret_cast<hipStream_t>(stream_v) : p->last_stream;
    const rt::DevBeam &B = p->P.beam;
    if (!h.bound) { // the first append: size, allocate and zero the history, bind it to this run
        rt_hip_history_facts f = {};
        f.size       = sizeof(f);
        f.nv         = p->P.K;
        f.nx         = B.nx;
        f.ny         = B.ny;
        f.na         = B.na;
        f.nb         = B.nb;
        f.n_rec      = p->last_records.n_rec() > 0 ? p->last_records.n_rec() : 1;
        f.n_steps    = h.n_steps;
        f.accumulate = 1; // (reserved always: one record per block beside n_steps of them)
        if (const char *e = facts_error(f))
            return fail_arg((std::string("rt_hip_plan_history_append: ") + e).c_str());
        rt_hip_history_layout lay = {};
        lay.size = sizeof(lay);
        history_layout(f, lay);
        unsigned char *dev = nullptr;
        HIP_TRY(pool_alloc(p->device, (void **) &dev, (size_t) lay.bytes));
        hipError_t e = hipSuccess;
        if (!h.ev)
            e = hipEventCreate(&h.ev);
        if (e == hipSuccess)
            e = hipMemsetAsync(dev, 0, (size_t) lay.bytes, stream);
        if (e != hipSuccess) {
            if (hipStreamSynchronize(stream) != hipSuccess)
                (void) hipGetLastError();
            pool_free(p->device, dev);
            HIP_TRY(e);
        }
        h.dev   = dev;
        h.lay   = lay;
        h.recs  = p->last_records;
        h.n_rec = f.n_rec;
        h.nv = f.nv, h.nx = f.nx, h.ny = f.ny, h.na = f.na, h.nb = f.nb;
        h.bound = true;
    }
    const rt_hip_history_layout &L = h.lay;
    // the run on another queue: not read before its end; an earlier append on another queue: the scratch is shared
    if (stream != p->last_stream)
        HIP_TRY(hipStreamWaitEvent(stream, p->ev1, 0));
    if (h.pending && h.stream != stream)
        HIP_TRY(hipStreamWaitEvent(stream, h.ev, 0));

    rt::HistAppend A = {};
    if (p->last_records.n_rec() > 0) {
        A.ev     = p->recs_dev;
        A.nf     = p->recs_dev + p->recs_nf_off;
        A.ang    = p->recs_dev + p->recs_ang_off;
        A.stride = p->recs_stride;
    } else { // a plain step run: the plan's step buffers or the lent ones, and the I_ang the run wrote
        A.ev     = p->step.E_v;
        A.nf     = p->step.nf;
        A.ang    = p->last_iang;
        A.stride = 0;
    }
    const size_t i = (size_t) step;
    A.h_ev    = at<double>(h, L.off_E_v) + i * (size_t) h.nv;
    A.h_nf    = at<double>(h, L.off_nf) + i * (size_t) h.nx * (size_t) h.ny;
    A.h_ang   = at<double>(h, L.off_I_ang) + i * (size_t) h.na * (size_t) h.nb;
    A.rec_ev  = (size_t) L.rec_E_v / 8;
    A.rec_nf  = (size_t) L.rec_nf / 8;
    A.rec_ang = (size_t) L.rec_I_ang / 8;
    if (accumulate) {
        A.a_ev     = at<double>(h, L.off_acc_E_v);
        A.a_nf     = at<double>(h, L.off_acc_nf);
        A.a_ang    = at<double>(h, L.off_acc_I_ang);
        A.arec_ev  = (size_t) L.rec_acc_E_v / 8;
        A.arec_nf  = (size_t) L.rec_acc_nf / 8;
        A.arec_ang = (size_t) L.rec_acc_I_ang / 8;
    }
    A.part   = at<double>(h, L.off_part);
    A.pflag  = at<unsigned>(h, L.off_pflag);
    A.nv     = (unsigned) h.nv;
    A.npix   = (unsigned) h.nx * (unsigned) h.ny;
    A.nab    = (unsigned) h.na * (unsigned) h.nb;
    A.pix_wg = L.pix_wg;
    A.aux_wg = L.aux_wg;
    A.weight = weight;

    const CodeSlot slot = record_code_slot(p->last_records);
    rt::HistFinish F = {};
    F.part      = A.part;
    F.pflag     = A.pflag;
    F.ctl       = reinterpret_cast<const unsigned *>(p->ctl);
    F.code_base = slot.base;
    F.code_div  = slot.div;
    F.code_row  = slot.row;
    F.esum      = at<double>(h, L.off_E_sum) + i;
    F.code      = at<unsigned>(h, L.off_code) + i;
    F.flags     = at<unsigned>(h, L.off_flags) + i;
    F.rec_esum  = (size_t) L.rec_E_sum / 8;
    F.rec_code  = (size_t) L.rec_code / 4;
    F.rec_flags = (size_t) L.rec_flags / 4;
    F.filled    = at<unsigned char>(h, L.off_filled) + i;
    F.acc_esum  = accumulate ? at<double>(h, L.off_acc_E_sum) : nullptr;
    F.n_rec     = (unsigned) h.n_rec;
    F.wg_rec    = L.wg_per_rec;
    F.pix_wg    = L.pix_wg;
    F.weight    = weight;

    hipLaunchKernelGGL(rt::rt_history_append_kernel, dim3(L.grid), dim3(rt::HIST_WG), 0, stream, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rt::rt_history_finish_kernel, dim3(1), dim3(rt::HIST_WG), 0, stream, F);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h.ev, stream));
    h.pending      = true;
    h.stream       = stream;
    h.filled[i]    = 1;
    return RT_OK;
}

int rt_hip_plan_history_info(rt_hip_plan *p, int *n_steps, int *n_rec, int *n_filled)
{
    if (!p)
        return fail_arg("rt_hip_plan_history_info: NULL plan");
    const History &h = p->hist;
    if (n_steps)
        *n_steps = h.n_steps;
    if (n_rec)
        *n_rec = h.bound ? h.n_rec : 0;
    if (n_filled) {
        int n = 0;
        for (unsigned char c : h.filled)
            n += c;
        *n_filled = n;
    }
    return RT_OK;
}

int rt_hip_plan_history_ptrs(rt_hip_plan *p, int r, double **E_v, double **nf, double **I_ang, double **E_sum, unsigned int **code,
                             unsigned int **flags)
{
    if (!p || !p->hist.bound)
        return fail_arg("rt_hip_plan_history_ptrs: the plan has no history yet (it is made by the first rt_hip_plan_history_append)");
    const History &h = p->hist;
    if (r < 0 || r >= h.n_rec)
        return fail_arg("rt_hip_plan_history_ptrs: r must be 0 .. n_rec - 1 of the history");
    const rt_hip_history_layout &L = h.lay;
    const unsigned long long R = (unsigned long long) r;
    if (E_v)
        *E_v = at<double>(h, L.off_E_v + R * L.rec_E_v);
    if (nf)
        *nf = at<double>(h, L.off_nf + R * L.rec_nf);
    if (I_ang)
        *I_ang = at<double>(h, L.off_I_ang + R * L.rec_I_ang);
    if (E_sum)
        *E_sum = at<double>(h, L.off_E_sum + R * L.rec_E_sum);
    if (code)
        *code = at<unsigned>(h, L.off_code + R * L.rec_code);
    if (flags)
        *flags = at<unsigned>(h, L.off_flags + R * L.rec_flags);
    return RT_OK;
}

int rt_hip_plan_history_sum_ptrs(rt_hip_plan *p, int r, double **E_v, double **nf, double **I_ang, double **E_sum)
{
    if (!p || !p->hist.bound)
        return fail_arg("rt_hip_plan_history_sum_ptrs: the plan has no history yet (it is made by the first rt_hip_plan_history_append)");
    const History &h = p->hist;
    if (r < 0 || r >= h.n_rec)
        return fail_arg("rt_hip_plan_history_sum_ptrs: r must be 0 .. n_rec - 1 of the history");
    const rt_hip_history_layout &L = h.lay;
    const unsigned long long R = (unsigned long long) r;
    if (E_v)
        *E_v = at<double>(h, L.off_acc_E_v + R * L.rec_acc_E_v);
    if (nf)
        *nf = at<double>(h, L.off_acc_nf + R * L.rec_acc_nf);
    if (I_ang)
        *I_ang = at<double>(h, L.off_acc_I_ang + R * L.rec_acc_I_ang);
    if (E_sum)
        *E_sum = at<double>(h, L.off_acc_E_sum + R * 8);
    return RT_OK;
}

int rt_hip_plan_history_fetch(rt_hip_plan *p, int r, double *E_v, double *nf, double *I_ang, double *E_sum, unsigned int *code,
                              unsigned int *flags, unsigned char *filled)
{
    if (!p || p->hist.n_steps < 1)
        return fail_arg("rt_hip_plan_history_fetch: the plan has no history (rt_hip_plan_history_create)");
    const History &h = p->hist;
    const size_t T   = (size_t) h.n_steps;
    if (!h.bound) { // nothing appended yet: every slot reads zero
        if (r != 0)
            return fail_arg("rt_hip_plan_history_fetch: r must be 0 before the first append");
        const rt::DevBeam &B = p->P.beam;
        if (E_v)
            memset(E_v, 0, T * (size_t) p->P.K * sizeof(double));
        if (nf)
            memset(nf, 0, T * (size_t) B.nx * (size_t) B.ny * sizeof(double));
        if (I_ang)
            memset(I_ang, 0, T * (size_t) B.na * (size_t) B.nb * sizeof(double));
        if (E_sum)
            memset(E_sum, 0, T * sizeof(double));
        if (code)
            memset(code, 0, T * sizeof(unsigned));
        if (flags)
            memset(flags, 0, T * sizeof(unsigned));
        if (filled)
            memset(filled, 0, T);
        return RT_OK;
    }
    if (r < 0 || r >= h.n_rec)
        return fail_arg("rt_hip_plan_history_fetch: r must be 0 .. n_rec - 1 of the history");
    HIP_TRY(hipSetDevice(p->device));
    history_wait(p);
    const rt_hip_history_layout &L = h.lay;
    const unsigned long long R = (unsigned long long) r;
    int rc = fetch_rows(h.dev + L.off_E_v + R * L.rec_E_v, E_v, T * (size_t) L.step_E_v);
    if (rc == RT_OK)
        rc = fetch_rows(h.dev + L.off_nf + R * L.rec_nf, nf, T * (size_t) L.step_nf);
    if (rc == RT_OK)
        rc = fetch_rows(h.dev + L.off_I_ang + R * L.rec_I_ang, I_ang, T * (size_t) L.step_I_ang);
    if (rc == RT_OK)
        rc = fetch_rows(h.dev + L.off_E_sum + R * L.rec_E_sum, E_sum, T * sizeof(double));
    if (rc == RT_OK)
        rc = fetch_rows(h.dev + L.off_code + R * L.rec_code, code, T * sizeof(unsigned));
    if (rc == RT_OK)
        rc = fetch_rows(h.dev + L.off_flags + R * L.rec_flags, flags, T * sizeof(unsigned));
    if (rc == RT_OK)
        rc = fetch_rows(h.dev + L.off_filled, filled, T);
    return rc;
}

int rt_hip_plan_history_fetch_sum(rt_hip_plan *p, int r, double *E_v, double *nf, double *I_ang, double *E_sum)
{
    if (!p || p->hist.n_steps < 1)
        return fail_arg("rt_hip_plan_history_fetch_sum: the plan has no history (rt_hip_plan_history_create)");
    const History &h = p->hist;
    if (!h.bound) {
        if (r != 0)
            return fail_arg("rt_hip_plan_history_fetch_sum: r must be 0 before the first append");
        const rt::DevBeam &B = p->P.beam;
        if (E_v)
            memset(E_v, 0, (size_t) p->P.K * sizeof(double));
        if (nf)
            memset(nf, 0, (size_t) B.nx * (size_t) B.ny * sizeof(double));
        if (I_ang)
            memset(I_ang, 0, (size_t) B.na * (size_t) B.nb * sizeof(double));
        if (E_sum)
            *E_sum = 0.0;
        return RT_OK;
    }
    if (r < 0 || r >= h.n_rec)
        return fail_arg("rt_hip_plan_history_fetch_sum: r must be 0 .. n_rec - 1 of the history");
    HIP_TRY(hipSetDevice(p->device));
    history_wait(p);
    const rt_hip_history_layout &L = h.lay;
    const unsigned long long R = (unsigned long long) r;
    int rc = fetch_rows(h.dev + L.off_acc_E_v + R * L.rec_acc_E_v, E_v, (size_t) L.step_E_v);
    if (rc == RT_OK)
        rc = fetch_rows(h.dev + L.off_acc_nf + R * L.rec_acc_nf, nf, (size_t) L.step_nf);
    if (rc == RT_OK)
        rc = fetch_rows(h.dev + L.off_acc_I_ang + R * L.rec_acc_I_ang, I_ang, (size_t) L.step_I_ang);
    if (rc == RT_OK)
        rc = fetch_rows(h.dev + L.off_acc_E_sum + R * 8, E_sum, sizeof(double));
    return rc;
}

} // extern "C"
