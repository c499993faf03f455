// rt_libm.h -- the libm functions of the device code, in one place: rt_sinf, rt_cosf, rt_acosf, rt_atan2f, rt_powf, rt_expf.  The product
// build forwards each to the device's libm.  A test build with -DRT_PORTABLE_LIBM (tools/build_variant.py, libpbrt_hip_plm.so) routes them to
// rt_libm_portable.h, the implementation the compiled reference and the CPU oracle can be made to share bit for bit: frames whose geometry
// goes through libm are then comparable pixel by pixel.
#pragma once
#include "rt_math.h"

#ifdef RT_PORTABLE_LIBM
#define PLM_FN __host__ __device__ inline
#include "rt_libm_portable.h"
RT_DEV float rt_sinf(float x) { return plm_sinf(x); }
RT_DEV float rt_cosf(float x) { return plm_cosf(x); }
RT_DEV float rt_acosf(float x) { return plm_acosf(x); }
RT_DEV float rt_atan2f(float y, float x) { return plm_atan2f(y, x); }
RT_DEV float rt_powf(float x, float y) { return plm_powf(x, y); }
RT_DEV float rt_expf(float x) { return plm_expf(x); }
#else
RT_DEV float rt_sinf(float x) { return sinf(x); }
RT_DEV float rt_cosf(float x) { return cosf(x); }
RT_DEV float rt_acosf(float x) { return acosf(x); }
RT_DEV float rt_atan2f(float y, float x) { return atan2f(y, x); }
RT_DEV float rt_powf(float x, float y) { return powf(x, y); }
RT_DEV float rt_expf(float x) { return expf(x); }
#endif
