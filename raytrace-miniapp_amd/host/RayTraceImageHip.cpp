// RayTraceImageHip.cpp -- the C++ adapter a reference maintainer adds next to
// RayTraceImageCPU.cpp / RayTraceImageCuda.cu.  It implements the back-end loop
// signature that RayTrace::create_image dispatches to (declared `extern` at
// src/RayTraceImage.cpp:47-75) by flattening the reference structs into the
// POD records of include/rt_hip.h and calling the C ABI of librt_hip.so.
//
// Compiled against the reference's own headers (-I<reference>/src
// -I<reference>/src/include) -- nothing of the reference is restated here.
// See INTEGRATION.md for the dispatcher / harness / CMake lines that go with it.
//
//   RayTraceImageHipLoop          one device ("hip" arm)
//   RayTraceImageHipMultiGPULoop  all devices of the node ("hip-multigpu" arm) through
//        rt_hip_multi_image_loop: stands where the reference runs RayTraceImageThreadLoop
//        (src/RayTraceImage.cpp:89-134) with setGPU called in the spawning thread (:116).
//   RayTraceImageStepHipLoop      the one-device loop with the per-step record (intensity_step_struct,
//        src/RayTraceStructures.h:361-369) in place of the image cube: E_v[nv], the frequency-integrated image[nx*ny],
//        I_ang -- through rt_hip_step_loop
//   RayTraceImageStepHipMultiGPULoop  the same record from all devices of the node through rt_hip_multi_step_loop: device d
//        traces rays d, d + ndev, ... of the grid on the full beam, one RCCL sum-reduce of (E_v | nf | I_ang) assembles
//        them -- the application's multi-rank step (src/RayTraceImage.cpp:300-313, intensity_step_struct::sum_reduce)
//   RayTraceImageLengthScanHipLoop  the per-step record at EVERY plasma length n = 2 .. N -- what N - 1 create_image calls with
//        info->N = n and the first n tables leave -- from one forward march, through rt_hip_length_scan_loop
//   RayTraceCalcRaysHip           n calls of RayTrace::calc_ray (src/RayTraceImage.cpp:189-204) in one, through
//        rt_hip_calc_rays: per-ray spectrum, exit ray and return code
#include "RayTrace.h"
#include "common/RayTraceImageHelper.h"
#include "utilities/RayUtilityMacros.h"

#include "rt_hip.h"

#include <cstring>
#include <string>
#include <vector>

static_assert(sizeof(ray_struct) == sizeof(rt_ray), "ray_struct and rt_ray must share a layout");

namespace {

struct Flat {
    rt_beam beam;
    std::vector<rt_gain> gain;
    rt_seed seed;
    bool has_seed;
};

// gain and seed tables alone (what calc_ray takes: it has no beam)
Flat flatten_tables(int N, const RayTrace::ray_gain_struct *g, const RayTrace::ray_seed_struct *s)
{
    Flat f;
    memset(&f.beam, 0, sizeof(f.beam));
    f.gain.resize((size_t) N);
    for (int i = 0; i < N; i++) {
        rt_gain &o = f.gain[(size_t) i];
        o.Nx = g[i].Nx; o.Ny = g[i].Ny; o.Nv = g[i].Nv;
        o.x = g[i].x; o.y = g[i].y; o.n = g[i].n;
        o.g0 = g[i].g0; o.E0 = g[i].E0; o.gv = g[i].gv;
    }
    f.has_seed = s != NULL;
    memset(&f.seed, 0, sizeof(f.seed));
    if (s) {
        for (int i = 0; i < 5; i++) {
            f.seed.dim[i] = s->dim[i];
            f.seed.x[i]   = s->x[i];
            f.seed.f[i]   = s->f[i];
        }
        f.seed.f0 = s->f0;
    }
    return f;
}

Flat flatten(int N, const RayTrace::EUV_beam_struct &b, const RayTrace::ray_gain_struct *g,
             const RayTrace::ray_seed_struct *s)
{
    Flat f    = flatten_tables(N, g, s);
    f.beam.nx = b.nx; f.beam.ny = b.ny; f.beam.na = b.na; f.beam.nb = b.nb; f.beam.nv = b.nv;
    f.beam.dx = b.dx; f.beam.dy = b.dy; f.beam.da = b.da; f.beam.db = b.db; f.beam.dz = b.dz;
    f.beam.x = b.x; f.beam.y = b.y; f.beam.a = b.a; f.beam.b = b.b; f.beam.dv = b.dv;
    return f;
}

// counters and device times of the last loop call of this thread (the loop signature has no slot for
// them): read by harnesses that print ray-steps/s next to the reference's timing table
thread_local rt_stats g_last_stats = {};

void run_on_device(int device, int N, const Flat &f, int method, const ray_struct *rays, size_t n_rays,
                   double scale, double *image, double *I_ang, unsigned int &failure_code,
                   std::vector<ray_struct> &failed_rays, std::string &error)
{
    rt_ray failed[RT_N_FAILED_MAX];
    int n_failed      = 0;
    unsigned int code = 0;
    int rc = rt_hip_image_loop(device, N, &f.beam, f.gain.data(), f.has_seed ? &f.seed : NULL, method,
                               reinterpret_cast<const rt_ray *>(rays), n_rays, scale, image, I_ang, &code,
                               failed, RT_N_FAILED_MAX, &n_failed, &g_last_stats);
    if (rc != RT_OK) {
        error = std::string("HIP backend error: ") + rt_hip_last_error();
        return;
    }
    failure_code |= code;
    for (int i = 0; i < n_failed; i++) {
        ray_struct r;
        memcpy(&r, &failed[i], sizeof(r));
        failed_rays.push_back(r);
    }
}

} // namespace

int RayTraceImageHipDeviceCount() { return rt_hip_device_count(); }

// rt_stats of the last RayTraceImageHip*Loop call made by the calling thread
const rt_stats *RayTraceImageHipLastStats() { return &g_last_stats; }

void RayTraceImageHipLoop(int N, const RayTrace::EUV_beam_struct &beam, const RayTrace::ray_gain_struct *gain,
    const RayTrace::ray_seed_struct *seed, int method, const std::vector<ray_struct> &rays, double scale,
    double *image, double *I_ang, unsigned int &failure_code, std::vector<ray_struct> &failed_rays)
{
    failure_code = 0;
    Flat f       = flatten(N, beam, gain, seed);
    std::string error;
    run_on_device(0, N, f, method, rays.empty() ? NULL : &rays[0], rays.size(), scale, image, I_ang,
                  failure_code, failed_rays, error);
    if (!error.empty())
        RAY_ERROR(error); // device/runtime errors end the process, as CUDA_CHECK does (RayTraceImageCuda.cu:8-18)
}

// The Loop signature with `double *E_v, double *nf` in place of `image`: E_v[k] = sum over pixels of image[k + nv p],
// nf[p] = sum over k of 2 dv[k] image[k + nv p] -- the reductions of what RayTraceImageHipLoop would leave in image,
// which is never built.  The physical normalisation constants of intensity_step_struct are the caller's to apply.
void RayTraceImageStepHipLoop(int N, const RayTrace::EUV_beam_struct &beam, const RayTrace::ray_gain_struct *gain,
    const RayTrace::ray_seed_struct *seed, int method, const std::vector<ray_struct> &rays, double scale,
    double *E_v, double *nf, double *I_ang, unsigned int &failure_code, std::vector<ray_struct> &failed_rays)
{
    failure_code = 0;
    Flat f       = flatten(N, beam, gain, seed);
    rt_ray failed[RT_N_FAILED_MAX];
    int n_failed      = 0;
    unsigned int code = 0;
    int rc = rt_hip_step_loop(0, N, &f.beam, f.gain.data(), f.has_seed ? &f.seed : NULL, method,
                              rays.empty() ? NULL : reinterpret_cast<const rt_ray *>(&rays[0]), rays.size(), scale, E_v, nf,
                              I_ang, &code, failed, RT_N_FAILED_MAX, &n_failed, &g_last_stats);
    if (rc != RT_OK)
        RAY_ERROR(std::string("HIP backend error: ") + rt_hip_last_error());
    failure_code |= code;
    for (int i = 0; i < n_failed; i++) {
        ray_struct r;
        memcpy(&r, &failed[i], sizeof(r));
        failed_rays.push_back(r);
    }
}

// RayTraceImageStepHipLoop for every plasma length at once (forward method, 3 <= N <= RT_N_SCAN_MAX + 1): row n - 2 of
// E_v [N-1][nv], nf [N-1][nx*ny], I_ang [N-1][na*nb] and failure_codes [N-1] is what RayTraceImageStepHipLoop leaves for
// the first n of the tables (create_image_struct::pack is "for a single length": the caller packs N - 1 times, or once and
// calls this).  failure_code is the OR of the codes; failed_rays the rays that fail at any length, each once.
void RayTraceImageLengthScanHipLoop(int N, const RayTrace::EUV_beam_struct &beam, const RayTrace::ray_gain_struct *gain,
    const RayTrace::ray_seed_struct *seed, int method, const std::vector<ray_struct> &rays, double scale,
    double *E_v, double *nf, double *I_ang, unsigned int *failure_codes, unsigned int &failure_code,
    std::vector<ray_struct> &failed_rays)
{
    failure_code = 0;
    Flat f       = flatten(N, beam, gain, seed);
    rt_ray failed[RT_N_FAILED_MAX];
    int n_failed = 0;
    std::vector<unsigned int> codes((size_t) (N > 1 ? N - 1 : 1), 0u);
    int rc = rt_hip_length_scan_loop(0, N, &f.beam, f.gain.data(), f.has_seed ? &f.seed : NULL, method,
                                     rays.empty() ? NULL : reinterpret_cast<const rt_ray *>(&rays[0]), rays.size(), scale, E_v, nf,
                                     I_ang, codes.data(), failed, RT_N_FAILED_MAX, &n_failed, &g_last_stats);
    if (rc != RT_OK)
        RAY_ERROR(std::string("HIP backend error: ") + rt_hip_last_error());
    for (int n = 2; n <= N; n++) {
        failure_code |= codes[(size_t) (n - 2)];
        if (failure_codes)
            failure_codes[n - 2] = codes[(size_t) (n - 2)];
    }
    for (int i = 0; i < n_failed; i++) {
        ray_struct r;
        memcpy(&r, &failed[i], sizeof(r));
        failed_rays.push_back(r);
    }
}

void RayTraceImageHipMultiGPULoop(int N, const RayTrace::EUV_beam_struct &beam,
    const RayTrace::ray_gain_struct *gain, const RayTrace::ray_seed_struct *seed, int method,
    const std::vector<ray_struct> &rays, double scale, double *image, double *I_ang,
    unsigned int &failure_code, std::vector<ray_struct> &failed_rays)
{
    failure_code = 0;
    if (rt_hip_device_count() < 1)
        RAY_ERROR("Hip-MultiGPU is not availible");
    Flat f = flatten(N, beam, gain, seed);
    rt_ray failed[RT_N_FAILED_MAX];
    int n_failed      = 0;
    unsigned int code = 0;
    // all devices of the node behind one call: pixel-column tiles + one RCCL gather (ASE), ray chunks +
    // one RCCL sum-reduce otherwise; device binding, communicator and assembly live behind the C ABI
    int rc = rt_hip_multi_image_loop(0, N, &f.beam, f.gain.data(), f.has_seed ? &f.seed : NULL, method,
                                     rays.empty() ? NULL : reinterpret_cast<const rt_ray *>(&rays[0]), rays.size(), scale,
                                     image, I_ang, &code, failed, RT_N_FAILED_MAX, &n_failed, &g_last_stats);
    if (rc != RT_OK)
        RAY_ERROR(std::string("HIP backend error: ") + rt_hip_last_error());
    failure_code |= code;
    for (int i = 0; i < n_failed; i++) {
        ray_struct r;
        memcpy(&r, &failed[i], sizeof(r));
        failed_rays.push_back(r);
    }
}

// RayTraceImageStepHipLoop on all devices of the node: same signature, same outputs up to summation order.  The cube
// exists on no device; what crosses the links is one sum-reduce of nv + nx*ny + na*nb doubles.
void RayTraceImageStepHipMultiGPULoop(int N, const RayTrace::EUV_beam_struct &beam, const RayTrace::ray_gain_struct *gain,
    const RayTrace::ray_seed_struct *seed, int method, const std::vector<ray_struct> &rays, double scale,
    double *E_v, double *nf, double *I_ang, unsigned int &failure_code, std::vector<ray_struct> &failed_rays)
{
    failure_code = 0;
    if (rt_hip_device_count() < 1)
        RAY_ERROR("Hip-MultiGPU is not availible");
    Flat f = flatten(N, beam, gain, seed);
    rt_ray failed[RT_N_FAILED_MAX];
    int n_failed      = 0;
    unsigned int code = 0;
    int rc = rt_hip_multi_step_loop(0, N, &f.beam, f.gain.data(), f.has_seed ? &f.seed : NULL, method,
                                    rays.empty() ? NULL : reinterpret_cast<const rt_ray *>(&rays[0]), rays.size(), scale,
                                    E_v, nf, I_ang, &code, failed, RT_N_FAILED_MAX, &n_failed, &g_last_stats);
    if (rc != RT_OK)
        RAY_ERROR(std::string("HIP backend error: ") + rt_hip_last_error());
    failure_code |= code;
    for (int i = 0; i < n_failed; i++) {
        ray_struct r;
        memcpy(&r, &failed[i], sizeof(r));
        failed_rays.push_back(r);
    }
}

// n independent RayTrace::calc_ray calls (src/RayTraceImage.cpp:189-204: trace a ray, return its spectrum Iv[K], its
// exit ray and its return code) on device 0.  rays / ray2: [n][4] doubles (x, y, a, b) as calc_ray takes and returns
// them; Iv: [n][K]; err: [n] (0, -1, -2, -3).  Returns RT_OK or the status of the C ABI (rt_hip_last_error has the text).
int RayTraceCalcRaysHip(size_t n, const double *rays, int N, double dz, const RayTrace::ray_gain_struct *gain,
    const RayTrace::ray_seed_struct *seed, int K, int method, double *Iv, double *ray2, int *err)
{
    static_assert(sizeof(int) == sizeof(int32_t), "err is handed over as int32_t");
    Flat f = flatten_tables(N, gain, seed);
    return rt_hip_calc_rays(0, N, dz, f.gain.data(), f.has_seed ? &f.seed : NULL, K, method, rays, n, Iv, ray2,
                            reinterpret_cast<int32_t *>(err), &g_last_stats);
}
