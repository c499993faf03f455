// rt_mega_rp.hip -- the radiance-query kernels for integrator 2 (0 whitted, 1 directlighting, 2 path)
#define RT_TU_INTEG 2
#define RT_TU_TABLE g_radiance_kernels_path
#include "rt_mega_rays_tu.inc"
