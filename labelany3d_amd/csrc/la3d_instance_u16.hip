// la3d_instance_u16.hip - the instance engine of la3d_instance.hip compiled for uint16 x scale depth planes
// (la3d_fit_instances_depth16, LA3D_DTYPE_U16): instance_fit_u16 and the fit_instances_u16_kernel instantiations.  A translation unit
// of its own, so that it compiles side by side with the float32 one.
#define LA3D_INSTANCE_DT 2
#include "la3d_instance.hip"
