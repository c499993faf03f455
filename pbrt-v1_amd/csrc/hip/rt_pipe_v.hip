// rt_pipe_v.hip -- rt::pipe_vertex_kernel (rt_pipe_vertex.h), in the order of flavour::Vertex (rt_flavour.h)
#include "rt_pipe_vertex.h"
#include "rt_flavour.h"
namespace rt {
RT_FLAVOUR_TABLE(g_pipe_vertex, PipeShadeFn, Vertex, Vertex::flavour(K), pipe_vertex_kernel<f.count, f.ext>)
}  // namespace rt
