// la3d_instance_f16.hip - the instance engine of la3d_instance.hip compiled for IEEE float16 depth planes (la3d_fit_instances_depth16,
// LA3D_DTYPE_F16): instance_fit_f16 and the fit_instances_f16_kernel instantiations.  A translation unit of its own, so that it
// compiles side by side with the float32 one.
#define LA3D_INSTANCE_DT 1
#include "la3d_instance.hip"
