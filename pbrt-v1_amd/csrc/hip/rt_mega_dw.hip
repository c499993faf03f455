// rt_mega_dw.hip -- rt::render_kernel for DirectLighting "weighted" (RT_INTEG_DIRECT_WEIGHTED; three passes per frame, rt_weighted.h), in the order of
// flavour::Weighted (rt_flavour.h)
#include "rt_render_kernel.h"
#include "rt_flavour.h"
namespace rt {
RT_FLAVOUR_TABLE(g_render_kernels_weighted, RenderKernelFn, Weighted, Weighted::flavour(K), render_kernel<f.count, RT_INTEG_DIRECT_WEIGHTED, f.accel, f.vol, f.waves, f.ext>)
}  // namespace rt
