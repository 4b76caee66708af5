// bycomp_ab.hip -- the one-CU by-component bootstrap kernels (pbs_split_kernel / pbs_ga_split_kernel with SOLO: mosfhet_amd/csrc/bootstrap_kernels.h) compiled alone,
// one instantiation per build, for tools/check_lds_barriers.py: two-wavefront teams whose exchanges and hand-over buffers stand in front of workgroup barriers.
//   -DAB_L=4 -DAB_BG=9 [-DAB_GA | -DAB_TP]      (AB_BG = 0: the run-time gadget of length AB_L; AB_TP: pbs_kernel<.., BYC = true>, the by-component form of the throughput kernel)
#include "../../mosfhet_amd/csrc/bootstrap_kernels.h"

using namespace mosfhet;

#ifndef AB_L
#define AB_L 4
#endif
#ifndef AB_BG
#define AB_BG 9
#endif

#if defined(AB_TP)
template __global__ void mosfhet::pbs_kernel<Fft2048, AB_L, AB_BG, true>(PbsParams, ParkArg<true>);
#elif defined(AB_GA)
template __global__ void mosfhet::pbs_ga_split_kernel<Fft2048L, AB_L, AB_BG, true>(GaParams, SplitParams);
#else
template __global__ void mosfhet::pbs_split_kernel<Fft2048L, AB_L, AB_BG, true>(PbsParams, SplitParams);
#endif
