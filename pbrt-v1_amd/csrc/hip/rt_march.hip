// rt_march.hip -- rt::pipe_march_kernel (rt_pipe_march.h), in the order of flavour::March (rt_flavour.h)
#include "rt_pipe_march.h"
#include "rt_flavour.h"
namespace rt {
RT_FLAVOUR_TABLE(g_pipe_march, PipeMarchFn, March, March::flavour(K), pipe_march_kernel<f.count, f.accel, f.ext>)
}  // namespace rt
