// rt_mega_fs_tu.inc -- one integrator's scene twins of the fixed-frame kernels: rt::render_kernel_scene over fixed::Frame and fixed::Scene<...>, in the
// order of flavour::FixedScene.  The including unit defines RT_TU_INTEG (the integrator) and RT_TU_TABLE (the table's name) first.
#include "rt_render_kernel.h"
#include "rt_fixed_frame.h"
namespace rt {
RT_FLAVOUR_TABLE(RT_TU_TABLE, RenderKernelFn, FixedScene, FixedScene::flavour(K), render_kernel_scene<f.count, RT_TU_INTEG, f.accel, f.vol, f.waves, f.ext, fixed::Frame,
                 fixed::Scene<(flavour::FixedScene::axes(K) & fixed::SCENE_ONE_LIGHT) != 0, (flavour::FixedScene::axes(K) & fixed::SCENE_NO_SPECULAR) != 0>>)
}  // namespace rt
