// rt_mega_b.hip -- rt::bidir_kernel (rt_bidir.h) for the bidirectional integrator, in the order of flavour::Bidir (rt_flavour.h)
#include "rt_bidir.h"
#include "rt_flavour.h"
namespace rt {
RT_FLAVOUR_TABLE(g_render_kernels_bidir, RenderKernelFn, Bidir, Bidir::flavour(K), bidir_kernel<f.count, f.accel>)
}  // namespace rt
