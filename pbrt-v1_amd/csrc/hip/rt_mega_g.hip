// rt_mega_g.hip -- rt::render_kernel for the debug integrator (RT_INTEGRATOR_DEBUG: u, v, normals, hit mask of the camera ray; rt_integrate.h), in the
// order of flavour::Debug (rt_flavour.h)
#include "rt_render_kernel.h"
#include "rt_flavour.h"
namespace rt {
RT_FLAVOUR_TABLE(g_render_kernels_debug, RenderKernelFn, Debug, Debug::flavour(K), render_kernel<f.count, RT_INTEGRATOR_DEBUG, f.accel, f.vol, f.waves, f.ext>)
}  // namespace rt
