// rt_march_guard.h -- which optical-depth marches along caller-supplied rays may start (rt_medium.hip: rt_medium_device), and how long any may get.
// A frame's rays start at the camera or on a surface, so plan_march (rt_frame_plan.h) can bound every ray parameter by the scene and refuse a step
// that would not advance there.  A ray a caller hands over in device memory can lie anywhere: DensityRegion::Tau (core/volume.cpp:137-153) runs
// `while (t0 < t1) t0 += step`, and at t = 3e8 a step of 10 is below half an ulp -- t + step == t, the loop never ends.  So
//   host, before any launch   march_caps: the limits of plan_march -- a positive finite step, at most 2^20 Tau samples and 65536 march steps over the
//                             volume's diagonal -- computed the same way; the kernel carries both as loop caps
//   per lane, after clipping  march_advances: t + step > t at the larger in magnitude of the clipped t0, t1 (the ulp grows with |t|: a step that
//                             advances there advances at every t the loop reaches), for the smallest step the query uses; a clipped interval
//                             that is not finite cannot be marched either.  Such a query gets zeros and RT_MEDIUM_NO_ADVANCE in its status.
// The tests are on values and bit patterns only.  No HIP header: tests/medium_guard_host.cpp runs both with a host compiler.
#pragma once
#include <math.h>
#include "rt_ray_guard.h"

#define RT_MARCH_MAX_TAUS (1 << 20)      // Tau samples of one optical-depth march (plan_march's limit)
#define RT_MARCH_MAX_STEPS 65536         // steps of one emission march (plan_march's limit)

#define RT_MEDIUM_NO_ADVANCE 1           // status bit 0: unusable ray, non-finite clipped interval, or t + step == t inside it
#define RT_MEDIUM_TOO_LONG 2             // status bit 1: the emission march along this ray would take more than RT_MARCH_MAX_STEPS steps

namespace rt {

RT_RAY_HD bool march_step_ok(float step) { return ray_finite(step) && step > 0.f; }

// may `while (t < t1) t += step`, started in [t0, t1], run?
RT_RAY_HD bool march_advances(float t0, float t1, float step) {
    if (!ray_finite(t0) || !ray_finite(t1) || !march_step_ok(step)) return false;
    const float a = fabsf(t0), b = fabsf(t1), t = a > b ? a : b;
    const float next = t + step;                                                 // float32 addition, as the loop performs it
    return next > t;
}

// The caps of a query with this step over a medium of volume-space diagonal `diag` and, for a density region, world diagonal `wdiag`:
// plan_march's expressions.  MARCH_OK, or which limit refuses the step.
enum { MARCH_OK = 0, MARCH_BAD_STEP = 1, MARCH_TOO_MANY_TAUS = 2, MARCH_TOO_MANY_STEPS = 3 };
struct MarchCaps { int steps = 0, taus = 0; };
inline int march_caps(float step_size, double diag, double wdiag, bool density, MarchCaps &c) {
    c = MarchCaps{};
    if (!march_step_ok(step_size)) return MARCH_BAD_STEP;
    const double nsteps = ceil(diag / step_size) + 2;
    if (nsteps > RT_MARCH_MAX_STEPS) return MARCH_TOO_MANY_STEPS;
    c.steps = int(nsteps);
    if (density) {
        const float half = .5f * step_size;                                      // the smallest step a Tau march is called with (emission.cpp:84)
        if (!march_step_ok(half)) return MARCH_BAD_STEP;
        const double taus = ceil(wdiag / double(half)) + 2;
        if (taus > double(RT_MARCH_MAX_TAUS)) return MARCH_TOO_MANY_TAUS;
        const double wsteps = ceil(wdiag / step_size) + 2;
        if (wsteps > RT_MARCH_MAX_STEPS) return MARCH_TOO_MANY_STEPS;
        c.taus = int(taus);
        if (int(wsteps) > c.steps) c.steps = int(wsteps);
    }
    return MARCH_OK;
}

}  // namespace rt
