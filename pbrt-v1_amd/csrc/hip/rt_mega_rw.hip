// rt_mega_rw.hip -- the radiance-query kernels for integrator 0 (0 whitted, 1 directlighting, 2 path)
#define RT_TU_INTEG 0
#define RT_TU_TABLE g_radiance_kernels_whitted
#include "rt_mega_rays_tu.inc"
