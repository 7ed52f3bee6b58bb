// p3d_patch.hpp -- windowed POCS (p3d_patch.hip): overlapping (w_il x w_xl) windows of every slice are gathered into a patch cube, run as independent
// jobs and blended back by a tapered overlap-add.  Window p = a * n_xl + b of slice s is job s * npatch + p; it starts at (starts_il[a], starts_xl[b]).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p3d {

struct PatchGeom {
    int nil, nxl;            // the slice
    int w_il, w_xl;          // the window
    int n_il, n_xl;          // windows per axis; npatch = n_il * n_xl
    const int* starts_il;    // device [n_il], strictly increasing, starts_il[a] + w_il <= nil
    const int* starts_xl;    // device [n_xl]
};

// patches[job][r][c] = src[(job / npatch) % src_slices][starts_il[a] + r][starts_xl[b] + c] for njobs jobs; elem_bytes 8 (complex64) or 4 (float32: real
// cubes and mask windows).  nonbinary (float32 only, may be NULL): raised when a gathered value is neither 0 nor 1.
hipError_t patch_launch_gather(const PatchGeom& g, const void* src, int src_slices, void* patches, size_t njobs, int elem_bytes, int* nonbinary, hipStream_t st);

// the windows of `nmasks` masks (job index as above) in the packed form of the single-kernel loop (ResidentArgs::bits): per mask [w_il][w_xl / 16] words,
// bit q of word (r, tl) = (mask window[r][tl + (w_xl / 16) q] == 1).  w_xl must be a multiple of 16.  nonbinary as above.
hipError_t patch_launch_pack(const PatchGeom& g, const float* mask, int mask_slices, uint16_t* bits, size_t nmasks, int* nonbinary, hipStream_t st);

// out[s][i][j] = sum_k W_k y_k / sum_k W_k over the windows k covering (i, j) whose job state is >= 0, in ascending window order, W_k = taper_il[i - start_il]
// taper_xl[j - start_xl]; 0 where no such window.  first_* / last_* (device, [nil] / [nxl]): the first and last window of the axis that covers a position.
struct PatchBlend {
    const float* taper_il;   // device [w_il]
    const float* taper_xl;   // device [w_xl]
    const int* first_il;
    const int* last_il;
    const int* first_xl;
    const int* last_xl;
    const int* state;        // device [nslices * npatch]: < 0 = the job is inactive and contributes nothing
};
hipError_t patch_launch_blend(const PatchGeom& g, const PatchBlend& b, const void* patches, void* out, int nslices, int dtype, hipStream_t st);

}  // namespace p3d
