// rt_mega_f.hip -- rt::render_kernel_fixed for the fixed frame (rt_fixed_frame.h): the twins of the high-occupancy, timed kernels without EXT and without a
// medium of whitted, directlighting and path, each for kd-tree and grid, in the order of flavour::Fixed
#include "rt_render_kernel.h"
#include "rt_fixed_frame.h"
namespace rt {
RT_FLAVOUR_TABLE(g_render_kernels_fixed, RenderKernelFn, Fixed, Fixed::flavour(K), render_kernel_fixed<f.count, flavour::Fixed::integrator(K), f.accel, f.vol, f.waves, f.ext, fixed::Frame>)
}  // namespace rt
