// rt_step.h -- step mode (rt_step.hip): the outputs of the application's per-step record (intensity_step_struct,
// src/RayTraceStructures.h:361-369) and the argument block of rt_step_kernel (the frequency kernel's block,
// rt_device.h, whose image pointer stays NULL, plus the two reduced outputs).
#pragma once

#include "rt_device.h"

namespace rt {

struct StepOut {
    double *E_v; // [K]       sum over all pixels of image[k + K p]
    double *nf;  // [nx * ny] sum over k of 2 dv[k] image[k + K p], p = ix + iy nx
};
struct StepKArg {
    FreqHot hot;
    FreqCold cold;
    StepOut out;
};

} // namespace rt
