// leveled_lut_ab.hip -- the leveled-LUT kernels (mosfhet_amd/csrc/leveled_lut_kernels.h) compiled alone for tools/check_lds_barriers.py: at N = 2048 their transforms'
// exchanges and the accumulator updates of the finishing kernel stand in front of workgroup barriers of two-wavefront teams.  lut_cmux_kernel carries the two
// modes of the per-input memories (capi_ram.inc) as well: the update of e in LDS between the products of a write stands in front of such a barrier too.  And the
// step of an automaton (capi_automaton.inc, mode 4): its rotated difference is written to LDS in front of the product's first barrier as mode 2 writes its own.
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

template __global__ void mosfhet::lut_prepare_kernel<AbF>(LutParams);
template __global__ void mosfhet::lut_level0_kernel<AbF>(LutParams);
template __global__ void mosfhet::lut_cmux_kernel<AbF>(LutParams);
