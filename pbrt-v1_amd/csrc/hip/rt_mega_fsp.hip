// rt_mega_fsp.hip -- the scene twins of the fixed-frame kernels (rt_fixed_frame.h, flavour::FixedScene) for integrator 2 (1 directlighting, 2 path)
#define RT_TU_INTEG 2
#define RT_TU_TABLE g_render_kernels_fixed_scene_path
#include "rt_mega_fs_tu.inc"
