// p3d_dct.hpp -- interface of the DCT passes (p3d_dct.hip) towards the API layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "p3d_fft.hpp"

namespace p3d {

// device tables of one norm (p3d_dct_tables.hpp): forward / inverse coefficients of axis 1 (length n1) and axis 2 (length n2)
struct DctTab {
    const c32 *f1, *i1, *f2, *i2;
};

// what one pass over the groups of four does with the spectrum in the row-major buffer w [nslices][n1][n2]
enum DctGroupMode {
    DCT_FUSED = 0,         // V -> combine -> threshold -> split -> V'   (one iteration's spectrum pass)
    DCT_COMBINE = 1,       // V -> X                                     (statistics, percentile ranking, forward test hook)
    DCT_SPLIT = 2,         // X -> V                                     (inverse test hook)
    DCT_SHRINK_SPLIT = 3,  // X -> threshold -> split -> V'              (second half after a percentile ranking)
};
hipError_t dct_launch_group(int mode, c32* w, const DctTab& tab, const c32* tau, int niter, int iter, int op, int nslices, int n1, int n2,
                            const int* done, hipStream_t st);

// gen_launch_update (p3d_generic.hpp) with the even/odd reordering of both axes folded into the addressing of w: sample (i1, i2) of x, mask
// and out lives at w[perm(n1, i1)][perm(n2, i2)].  mode 0 / 1 as there; mode 2: out = w through the reordering, nothing else (complex64)
hipError_t dct_launch_update(c32* w, const void* x, int dtype, const float* mask, size_t mask_stride, void* out, double* sums, int mode, int adaptive, int write_out,
                             float alpha, int nslices, int n1, int n2, const int* done, int zero_fill, hipStream_t st);

}  // namespace p3d
