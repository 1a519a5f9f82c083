// nz_fractal_shaped.hip -- the billow and ridged instantiations of nz_fractal.hip's kernels (nz_launch_fractal_shaped).
//
// Same source, own translation unit: with the shaped kernels in the same module the compiler schedules one of the
// fBm kernels differently (fractal_tab3_kernel<DomainRotatedPerlin> came out one VGPR smaller), and the fBm code is
// tuned as it stands.  Kept apart, nz_fractal.o is the fBm module it always was.
#define NZ_FRACTAL_SHAPED_TU 1
#include "nz_fractal.hip"
