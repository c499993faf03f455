// rt_trace.hip -- rt::pipe_trace_kernel (the dominant kernel of the queue pipeline), in the order of flavour::Trace (rt_flavour.h)
#include "rt_pipeline.h"
#include "rt_flavour.h"
namespace rt {
RT_FLAVOUR_TABLE(g_pipe_trace, PipeTraceFn, Trace, Trace::flavour(K), pipe_trace_kernel<f.count, f.accel, f.ext>)
}  // namespace rt
