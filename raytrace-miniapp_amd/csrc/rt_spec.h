// rt_spec.h -- spectra mode (rt_spec.hip): the per-ray outputs of RayTrace::calc_ray and the argument block of
// rt_spec_kernel (the frequency kernel's block, rt_device.h, with the outputs in place of image and I_ang, which it
// never touches).
#pragma once

#include "rt_device.h"

namespace rt {

struct SpecOut {
    double *Iv;   // [n_rays][K], row stride K
    rt_ray *ray2; // [n_rays] exit ray (zeros for a ray with error -1)
    int32_t *err; // [n_rays] 0, -1, -2, -3 (Helper.h:47-56)
};
struct SpecKArg {
    FreqHot hot;
    FreqCold cold;
    SpecOut out;
};

} // namespace rt
