// rt_mega_rays_tu.inc -- one integrator's radiance-query kernels (rt_radiance_device): rt::render_kernel_fixed over the traits fixed::Rays, in the
// order of flavour::Rays (rt_flavour.h)
#include "rt_render_kernel.h"
#include "rt_fixed_frame.h"
namespace rt {
RT_FLAVOUR_TABLE(RT_TU_TABLE, RenderKernelFn, Rays, Rays::flavour(K, RT_TU_INTEG), render_kernel_fixed<f.count, RT_TU_INTEG, f.accel, f.vol, f.waves, f.ext, fixed::Rays>)
}  // namespace rt
