// leveled_lut_tables_ab.hip -- the finish of the several-table leveled LUT (mosfhet_amd/csrc/leveled_lut_kernels.h: lut_tables_finish_kernel) compiled alone for
// tools/check_lds_barriers.py: the exchanges of its transforms and the updates of the grouped accumulators stand in front of workgroup barriers of two-wavefront
// teams at N = 2048.
//   -DAB_N=1024 | -DAB_N=2048
#include "../../mosfhet_amd/csrc/leveled_lut_kernels.h"

using namespace mosfhet;

#ifndef AB_N
#define AB_N 2048
#endif
#if AB_N == 1024
using AbF = Fft1024;
#else
using AbF = Fft2048;
#endif

template __global__ void mosfhet::lut_tables_finish_kernel<AbF>(LutParams);
