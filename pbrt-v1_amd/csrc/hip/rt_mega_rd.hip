// rt_mega_rd.hip -- the radiance-query kernels for integrator 1 (0 whitted, 1 directlighting, 2 path)
#define RT_TU_INTEG 1
#define RT_TU_TABLE g_radiance_kernels_direct
#include "rt_mega_rays_tu.inc"
