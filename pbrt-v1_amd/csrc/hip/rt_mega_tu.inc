// rt_mega_tu.inc -- one integrator's instantiations of rt::render_kernel, in the order of flavour::Mega (rt_flavour.h)
#include "rt_render_kernel.h"
#include "rt_flavour.h"
namespace rt {
RT_FLAVOUR_TABLE(RT_TU_TABLE, RenderKernelFn, Mega, Mega::flavour(K, RT_TU_INTEG), render_kernel<f.count, RT_TU_INTEG, f.accel, f.vol, f.waves, f.ext>)
}  // namespace rt
