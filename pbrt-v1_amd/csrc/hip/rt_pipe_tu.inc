// rt_pipe_tu.inc -- one integrator's instantiations of rt::pipe_shade_kernel, in the order of flavour::Shade (rt_flavour.h)
#include "rt_pipeline.h"
#include "rt_flavour.h"
namespace rt {
RT_FLAVOUR_TABLE(RT_TU_TABLE, PipeShadeFn, Shade, Shade::flavour(K), pipe_shade_kernel<f.count, RT_TU_INTEG, f.vol, f.ext>)
}  // namespace rt
