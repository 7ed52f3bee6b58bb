// p3d_resident_dct.hpp -- interface of the single-kernel DCT loop of the windowed jobs (p3d_patch_dct.hip)
#pragma once
#include <hip/hip_runtime.h>

#include "p3d_fft.hpp"
#include "p3d_resident.hpp"

namespace p3d {

struct ResidentDctArgs {
    ResidentArgs r;    // as the FFT loop takes them, one packed mask per job (mask_period > 0); x, out and the mask words in natural sample order
    const c32* fac;    // the factors of the job's norm (p3d_dct_tables.hpp): [fwd nil | inv nil | fwd nxl | inv nxl]
};

// the shapes of resident_patch_launch
hipError_t resident_dct_patch_launch(int nil, int nxl, const ResidentDctArgs& a, hipStream_t st);

}  // namespace p3d
