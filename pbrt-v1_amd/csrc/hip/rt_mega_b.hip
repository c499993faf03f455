// rt_mega_b.hip -- rt::bidir_kernel (rt_bidir.h) for the bidirectional integrator: 4 instantiations, k = ACCEL*2 + COUNT, all with the glossy / quadric / infinite-light
// code (the EXT shading set) at natural register allocation -- one flavour per accelerator covers every material, quadric and light
#include "rt_bidir.h"
namespace rt {
extern const RenderKernelFn g_render_kernels_bidir[4];
const RenderKernelFn g_render_kernels_bidir[4] = {bidir_kernel<false, 0>, bidir_kernel<true, 0>, bidir_kernel<false, 1>, bidir_kernel<true, 1>};
}  // namespace rt
