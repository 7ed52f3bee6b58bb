/*
 * p3d.h -- C ABI of libp3d_hip.so: the MI355X (gfx950) implementation of the POCS hot path of
 * fwrnke/pseudo-3D-interpolation.
 *
 * The reference has no FFI layer; its boundary for this path is the Python callable
 *     POCS_algorithm(x, mask, auxiliary_data, transform, itransform, transform_kind, niter, thresh_op,
 *                    thresh_model, eps, alpha, p_max, p_min, sqrt_decay, decay_kind, verbose, version,
 *                    results_dict, path_results)         pseudo_3D_interpolation/functions/POCS.py:371-391
 * called once per (iline, xline) slice by xr.apply_ufunc(..., vectorize=True)
 *                                                        pseudo_3D_interpolation/cube_POCS_interpolation_3D.py:314-340
 * The entry points below are what a ctypes binding of that callable needs (INTEGRATION.md shows
 * the stub): plain pointers and sizes, no Python / torch types.
 *
 * Conventions
 *   - every function returns P3D_OK (0) or a negative error code; p3d_last_error() gives the text
 *     (thread-local);
 *   - a "slice" is one (nil x nxl) array, C-contiguous, xline fastest; a cube is [nslices][nil][nxl]
 *     (the slice-major layout written by cube_binning_3D.py:1313-1351);
 *   - *_dev functions take DEVICE pointers (hipMalloc / p3d_malloc / torch data_ptr), the
 *     un-suffixed ones take HOST pointers and stage through buffers owned by the plan;
 *   - a plan is bound to one device and one internal stream and is not re-entrant; different plans
 *     may be used from different host threads / processes;
 *   - all calls are synchronous: when they return, outputs are complete.
 */
#ifndef P3D_H
#define P3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_ABI_VERSION 1

#define P3D_OK 0
#define P3D_ERR_INVALID (-1)     /* bad argument */
#define P3D_ERR_UNSUPPORTED (-2) /* shape / option not covered by the HIP kernels */
#define P3D_ERR_HIP (-3)         /* a HIP runtime call failed (no GPU, out of memory, ...) */

/* element type of the observed cube `x` and of the result (np.iscomplexobj(x), POCS.py:511, 653-656) */
#define P3D_C64 0 /* complex64: frequency-domain cube (dim 'freq_twt') */
#define P3D_F32 1 /* float32 : time-domain cube (dim 'twt'); result is np.real() of the iterate */
#define P3D_C128 2 /* complex128 and */
#define P3D_F64 3  /* float64 cubes: the double-precision entry points only (p3d_pocs64_*) */

/* thresh_op (POCS.py:91-102 -> threshold_operator.py:9-112) */
#define P3D_OP_HARD 0
#define P3D_OP_SOFT 1
#define P3D_OP_GARROTE 2
/* '-percentile' variants (POCS.py:43-58, 95-102): Re(tau) of every iteration is a PERCENTAGE; the threshold applied to a
 * slice is np.percentile(abs(X), tau) of that slice's spectrum at that iteration (linear interpolation).  These run on the
 * unfused pipeline (the spectrum has to exist in memory to be ranked). */
#define P3D_OP_PERCENTILE 16 /* OR-ed with P3D_OP_HARD / _SOFT / _GARROTE */

/* version (POCS.py:564-575).  FAST is accepted and runs REGULAR: in the reference the momentum
 * term of 'fast' is identically zero (POCS.py:549-550, 566-571, 629). */
#define P3D_VER_REGULAR 0
#define P3D_VER_FAST 1
#define P3D_VER_ADAPTIVE 2

/* p3d_pocs_params.flags */
#define P3D_FLAG_PROFILE 1 /* bracket every kernel launch with HIP events; read with p3d_last_profile() */
#define P3D_FLAG_PRIMED 2  /* p3d_pocs_prime_dev has just run on exactly this cube and mask: p3d_pocs_run_dev may skip its first pass */
/* `mask` holds one mask PER SLICE, [nslices][nil][nxl] (float32 for the float32 loops, double for the *64 loops; host or device exactly as the entry point
 * takes its shared mask): slice s is interpolated with mask[s], as POCS_algorithm(x[s], mask[s], ...) would.  Honoured by every run entry point that takes
 * p3d_pocs_params; p3d_multi_run hands each device's block its own part of the mask.  The float32 FFT loop then runs its unfused passes (fft2 | threshold |
 * ifft2 | update) for every shape -- the fused paths rest on packed forms of one mask.  P3D_FLAG_PRIMED is ignored together with this flag: the primed
 * first pass packs one mask.  Plans grow their mask buffers to max_slices slices when the flag is first seen. */
#define P3D_FLAG_MASK_PER_SLICE 4

typedef struct p3d_plan p3d_plan;

typedef struct p3d_pocs_params {
    int32_t niter;     /* number of iterations (POCS.py:560) */
    int32_t thresh_op; /* P3D_OP_* */
    int32_t version;   /* P3D_VER_* */
    int32_t flags;     /* P3D_FLAG_* */
    double eps;        /* early exit: iiter > 2 and cost < eps (POCS.py:631); 0 disables */
    double alpha;      /* re-insertion weight (POCS.py:616-619) */
} p3d_pocs_params;

/* number of doubles per slice written by p3d_pocs_stats*: everything get_threshold_decay
 * (POCS.py:169-368) needs from X0 = fft2(x):
 *   [0] Re, [1] Im of the lexicographic max of X0 (numpy's complex .max(), POCS.py:288)
 *   [2] max |X0|, [3] min |X0|   (POCS.py:261-262)
 *   [4] sum |X0|^2               (POCS.py:299)
 *   [5] reserved (0)                                                                       */
#define P3D_STATS_PER_SLICE 6

int p3d_abi_version(void);
const char* p3d_last_error(void);
/* HIP_VERSION this library was compiled against and the version of the HIP runtime the process bound (they differ when another copy of
 * libamdhip64 was mapped first; the Python binding warns when major.minor disagree) */
int p3d_runtime_info(int* compiled_hip_version, int* runtime_hip_version);
int p3d_device_count(int* n);
/* compute units of a device: the persistent passes run one or two workgroups on each (tests size their jobs by it) */
int p3d_device_cus(int device, int* n);

/* 1 when the HIP kernels cover an (nil, nxl) slice shape, else 0 */
int p3d_shape_supported(int nil, int nxl);

int p3d_plan_create(p3d_plan** out, int device, int nil, int nxl, int max_slices);
int p3d_plan_destroy(p3d_plan* plan);

/* device-memory helpers so that a pure-ctypes caller needs no other GPU runtime */
int p3d_malloc(p3d_plan* plan, void** dptr, size_t bytes);
int p3d_free(p3d_plan* plan, void* dptr);   /* `plan` may be NULL (the buffer outlived its plan) */
int p3d_memcpy_h2d(p3d_plan* plan, void* dst_dev, const void* src_host, size_t bytes);
int p3d_memcpy_d2h(p3d_plan* plan, void* dst_host, const void* src_dev, size_t bytes);
/* The same without a plan, for callers that keep whole cubes resident in HBM across several plans (bench.py, a pipeline that chains
 * steps 12 -> 13 -> 14 on device buffers) and use no other GPU runtime: blocking calls on the device's null stream.
 * kind: 0 host -> device, 1 device -> host, 2 device -> device. */
int p3d_dev_malloc(int device, void** dptr, size_t bytes);
int p3d_dev_free(void* dptr);
int p3d_dev_memcpy(int device, void* dst, const void* src, size_t bytes, int kind);
int p3d_dev_memset(int device, void* dptr, int value, size_t bytes);
int p3d_dev_synchronize(int device);
int p3d_dev_mem_info(int device, size_t* free_bytes, size_t* total_bytes);
/* page-locked host memory: copies to / from it run at the PCIe rate (pageable NumPy memory is staged by the runtime at a
 * quarter of it); the chunk pipeline of pocs_cube keeps its staging buffers here */
int p3d_host_alloc(void** hptr, size_t bytes);
int p3d_host_free(void* hptr);
/* page-lock a caller's array IN PLACE for the duration of a job (the host-buffer entry point of the Python mirror,
 * functions/POCS.py pocs_cube, does this with the cube it is handed and the result it returns -- the stand-in for the dask workers'
 * netCDF chunks of cube_POCS_interpolation_3D.py:314-340): transfers to / from it are DMA both ways at once.
 * P3D_ERR_UNSUPPORTED when the runtime refuses the range (the caller then simply goes on with pageable memory). */
int p3d_host_register(void* hptr, size_t bytes);
int p3d_host_unregister(void* hptr);

/* Batched 2-D FFT of complex64 slices, numpy.fft.fft2 / ifft2 conventions (unnormalised forward,
 * 1/(nil*nxl) inverse).  Replaces the callables injected at cube_POCS_interpolation_3D.py:255-257;
 * exported as a test hook.  in == out is allowed. */
int p3d_fft2_c64_dev(p3d_plan* plan, const void* in_dev, void* out_dev, int nslices, int inverse);
int p3d_fft2_c64(p3d_plan* plan, const void* in_host, void* out_host, int nslices, int inverse);

/* Thresholded spectrum of every slice: threshold(fft2(x), tau_s, kind) as the first half of one POCS
 * iteration computes it (POCS.py:592-599 -> threshold_operator.py:9-112).  tau: HOST [nslices][2]
 * doubles (Re, Im).  Test hook: lets a checker see the keep/zero decision of every coefficient. */
int p3d_fft2_shrink_c64(p3d_plan* plan, const void* in_host, const double* tau, int thresh_op, void* out_host,
                        int nslices);

/* Per-slice statistics of X0 = fft2(x) for the threshold schedule (replaces the device-independent
 * part of get_threshold_decay, POCS.py:535-546).  stats_host: [nslices][P3D_STATS_PER_SLICE]. */
int p3d_pocs_stats_dev(p3d_plan* plan, const void* x_dev, int dtype, int nslices, double* stats_host);
/* p3d_pocs_stats_dev for a caller that is about to run the job on the same cube: with the mask at hand the statistics pass IS the
 * first pass of the job (forward row transform into the work buffer, compact copy of the observed samples, sum |x_obs|), so a
 * following p3d_pocs_run_dev(..., flags | P3D_FLAG_PRIMED) on the same plan, pointers, dtype and batch skips it (one full pass over
 * the cube per job).  The flag is a promise about the CONTENTS of x_dev and mask_dev (unchanged in between); the plan checks the
 * rest and runs the ordinary first pass when anything else used it meanwhile, for APOCS and for float32 cubes that take the
 * half-spectrum path.  Same statistics, same results, bit for bit. */
int p3d_pocs_prime_dev(p3d_plan* plan, const void* x_dev, int dtype, const float* mask_dev, int nslices, double* stats_host);
int p3d_pocs_stats(p3d_plan* plan, const void* x_host, int dtype, int nslices, double* stats_host);

/* thresh_model = 'data-driven' (get_threshold_decay, functions/POCS.py:356-362): the schedule is read off the sorted forward
 * transform of the slice, complex numbers in NumPy's lexicographic order.  Two steps, so that the bounds are formed by the caller
 * in the reference's own arithmetic (tau = p * x_fwd.max(), complex64):
 *   p3d_pocs_sorted_spectrum   x (HOST or device, complex64 [nslices][nil][nxl]) -> fft2 -> sorted per slice, descending, kept
 *                              in the plan's staging buffers; peaks_host [nslices][2] = x_fwd.max() (POCS.py:288)
 *   p3d_pocs_data_driven_pick  bounds_host [nslices][4] = tau_min (re, im), tau_max (re, im) ->
 *                              count_host [nslices] = Nv = #{tau_min < X < tau_max} (0: the reference raises IndexError),
 *                              tau_host [nslices][niter][2] = v[0], v[ceil(i (Nv - 1) / (niter - 1))] (float32 pairs)
 * The pick must follow the sort directly (any other call on the plan in between invalidates the sorted keys: P3D_ERR_INVALID). */
int p3d_pocs_sorted_spectrum(p3d_plan* plan, const void* x, int nslices, float* peaks_host);
int p3d_pocs_data_driven_pick(p3d_plan* plan, int nslices, int niter, const float* bounds_host, float* tau_host, int64_t* count_host);

/* The POCS loop (POCS.py:549-632) for a batch of slices sharing one trace mask, or bringing one mask each (P3D_FLAG_MASK_PER_SLICE).
 *   x        [nslices][nil][nxl] observed data, zeros at missing traces, dtype as given
 *   mask     [nil][nxl] float32, 1 = observed trace, 0 = missing (cube_POCS_interpolation_3D.py:242-244), shared by the batch; with
 *            P3D_FLAG_MASK_PER_SLICE in params->flags [nslices][nil][nxl], one mask per slice (the same holds for the `mask` of every
 *            other *_run entry point below, float32 or double as documented there)
 *   tau      HOST, [nslices][niter][2] doubles: Re, Im of the threshold used at each iteration
 *            (decay[k], or sqrt(decay[k]) for sqrt_decay; POCS.py:595)
 *   active   HOST, [nslices] uint8 or NULL: 0 marks an all-zero slice, which the reference returns
 *            untouched with niterations = 0 (POCS.py:515-521)
 *   out      [nslices][nil][nxl], same dtype as x
 *   niter_done  HOST [nslices] int32: iterations executed per slice (POCS.py:634)
 *   sums     HOST [(niter+1)][nslices] doubles or NULL: sums[0][s] = sum|x_s|, sums[k+1][s] =
 *            sum|x_k| after iteration k (0 where not executed); cost_k = ((S_k+1 - S_k)/S_k+1)^2
 *            (POCS.py:622)
 *   elapsed_ms  device time of the whole call measured with HIP events on the plan's stream, or NULL */
int p3d_pocs_run_dev(p3d_plan* plan, const void* x_dev, int dtype, const float* mask_dev, const double* tau,
                     const uint8_t* active, const p3d_pocs_params* params, void* out_dev, int nslices,
                     int32_t* niter_done, double* sums, double* elapsed_ms);
int p3d_pocs_run(p3d_plan* plan, const void* x_host, int dtype, const float* mask_host, const double* tau,
                 const uint8_t* active, const p3d_pocs_params* params, void* out_host, int nslices,
                 int32_t* niter_done, double* sums, double* elapsed_ms);

/* The same two calls for a cube in HOST memory spread over several devices from ONE process: contiguous blocks of the slice axis
 * (the split of sharding.slice_block) go to devices[0 .. ndev-1], one host thread and one plan per entry (a device may be listed
 * more than once), chunks of ~256 MiB; every device copies its own block back, there is no collective.  The reference's
 * counterpart is the dask worker farm over slices (cube_POCS_interpolation_3D.py:291-340).  Arguments as p3d_pocs_stats /
 * p3d_pocs_run; tau is required. */
int p3d_multi_stats(int ndev, const int* devices, int nil, int nxl, const void* x_host, int dtype, int nslices, double* stats_host);
int p3d_multi_run(int ndev, const int* devices, int nil, int nxl, const void* x_host, int dtype, const float* mask_host,
                  const double* tau, const uint8_t* active, const p3d_pocs_params* params, void* out_host, int nslices,
                  int32_t* niter_done, double* sums);

/* ---- transform_kind = 'DCT': the loop with scipy.fft.dctn / idctn (type 2) as the sparsifying transform -------------------------
 * norm: the `norm` keyword of both callables.  The DCT is computed from the plan's own batched 2-D FFT of the even/odd-reordered slice
 * plus one pass over groups of four coefficients (csrc/p3d_dct.hip), float32 arithmetic; every shape of p3d_shape_supported is covered.
 * Real cubes run as complex with zero imaginary part.  The same loop in double precision: p3d_pocs64_dct_run on a plan64, below. */
#define P3D_DCT_BACKWARD 0 /* norm=None / 'backward': unnormalised forward, 1/(2 nil * 2 nxl) inverse */
#define P3D_DCT_ORTHO 1    /* norm='ortho' */
/* Batched 2-D DCT-II (inverse = 0) / its inverse (inverse = 1) of complex64 slices; test hook like p3d_fft2_c64.  in == out is allowed. */
int p3d_dct2_c64_dev(p3d_plan* plan, const void* in_dev, void* out_dev, int nslices, int inverse, int norm);
int p3d_dct2_c64(p3d_plan* plan, const void* in_host, void* out_host, int nslices, int inverse, int norm);
/* threshold(dctn(x), tau_s, kind) of every slice, arguments as p3d_fft2_shrink_c64: the keep/zero decision of every coefficient */
int p3d_dct_shrink_c64(p3d_plan* plan, const void* in_host, const double* tau, int thresh_op, void* out_host, int nslices, int norm);
/* the statistics of p3d_pocs_stats* taken from X0 = dctn(x) */
int p3d_pocs_dct_stats_dev(p3d_plan* plan, const void* x_dev, int dtype, int nslices, double* stats_host, int norm);
int p3d_pocs_dct_stats(p3d_plan* plan, const void* x_host, int dtype, int nslices, double* stats_host, int norm);
/* p3d_pocs_run* with the DCT pair in place of fft2 / ifft2; every operator, version and option of p3d_pocs_params, P3D_OP_PERCENTILE
 * included (P3D_FLAG_PRIMED and P3D_FLAG_PROFILE are ignored) */
int p3d_pocs_dct_run_dev(p3d_plan* plan, const void* x_dev, int dtype, const float* mask_dev, const double* tau, const uint8_t* active,
                         const p3d_pocs_params* params, void* out_dev, int nslices, int32_t* niter_done, double* sums,
                         double* elapsed_ms, int norm);
int p3d_pocs_dct_run(p3d_plan* plan, const void* x_host, int dtype, const float* mask_host, const double* tau, const uint8_t* active,
                     const p3d_pocs_params* params, void* out_host, int nslices, int32_t* niter_done, double* sums,
                     double* elapsed_ms, int norm);

/* ---- windowed POCS: overlapping windows of every slice as independent jobs, blended by a tapered overlap-add (csrc/p3d_patch.hip) ------------
 * A slice of nil x nxl points is cut into n_il x n_xl windows of the slice shape of `plan` (w_il x w_xl); window p = a * n_xl + b starts at
 * (starts_il[a], starts_xl[b]) and window p of slice s is job s * npatch + p, npatch = n_il * n_xl.  Every job is one POCS job of its own
 * (statistics, schedule, early exit, iteration count); the result is out[s][i][j] = sum_k W_k y_k / sum_k W_k over the active windows k covering
 * (i, j) in ascending window order, W_k = taper_il[i - start_il] * taper_xl[j - start_xl], 0 where there is none.  float32 kernels: complex64 /
 * float32 cubes.  A patch plan borrows `plan` (not owned; it must outlive the patch plan and hold max_slices * npatch slices), runs on its stream
 * and is as little re-entrant.
 *   create   starts_* HOST int32, strictly increasing with start + w <= extent; taper_* HOST float32 [w_il] / [w_xl], positive and finite;
 *            anything else is P3D_ERR_INVALID
 *   info     windows per slice, jobs the plan holds, and whether the single-kernel loop covers the window shape (extents of 32, 64, 128 with at
 *            most 8192 points)
 *   gather   cube_dev [nslices][nil][nxl] -> patches_dev [nslices * npatch][w_il][w_xl], dtype as given
 *   mask     the windows of mask_dev -- [nil][nxl] with mask_slices = 1, [nslices][nil][nxl] with mask_slices = nslices -- packed for the
 *            single-kernel loop (kept in the patch plan: npatch resp. nslices * npatch masks) and, where windows_dev is not NULL, as float32
 *            [nslices * npatch][w_il][w_xl], one per job, the mask the plan's own loops take with P3D_FLAG_MASK_PER_SLICE; *nonbinary (may be
 *            NULL) = 1 when a weight is neither 0 nor 1
 *   route    *single_kernel = 1 when p3d_patch_run_dev takes the job: window shape covered, binary masks in the last p3d_patch_mask_dev, P3D_OP_HARD /
 *            _SOFT / _GARROTE, P3D_VER_REGULAR / _FAST, and the environment variable P3D_NO_PATCH_RESIDENT unset (read at every call).  Every other job
 *            runs p3d_pocs_run_dev / p3d_pocs_dct_run_dev of `plan` on the patch cube with windows_dev and P3D_FLAG_MASK_PER_SLICE.
 *   run      the whole loop of every job in ONE kernel, a workgroup per job, with the masks of the last p3d_patch_mask_dev; arguments as
 *            p3d_pocs_run_dev with nslices * npatch jobs in place of slices (tau [jobs][niter][2], active / niter_done [jobs], sums
 *            [niter + 1][jobs]); results are bit for bit those of p3d_pocs_run_dev on window p's jobs with window p's mask.  P3D_ERR_UNSUPPORTED for
 *            a job p3d_patch_route does not give it
 *   dct_route / dct_run   the same two with scipy.fft.dctn / idctn (type 2, norm P3D_DCT_BACKWARD / P3D_DCT_ORTHO) as the transform of every window: the
 *            single-kernel DCT loop (csrc/p3d_resident_dct_job.hpp) takes the jobs p3d_patch_route gives the FFT loop, for a norm it knows; tau is the
 *            schedule of the windows' DCT spectra (p3d_pocs_dct_stats_dev on the patch cube).  Results agree with p3d_pocs_dct_run_dev on the patch cube
 *            to float32 rounding, not bit for bit (another FFT, another summation order).  P3D_ERR_UNSUPPORTED for a job dct_route does not give it
 *   blend    patches_dev (results) -> out_dev [nslices][nil][nxl]; active HOST [nslices * npatch] uint8 or NULL: 0 = the window contributes nothing */
typedef struct p3d_patch_plan p3d_patch_plan;
int p3d_patch_plan_create(p3d_patch_plan** out, p3d_plan* plan, int nil, int nxl, const int32_t* starts_il, int n_il, const int32_t* starts_xl,
                          int n_xl, const float* taper_il, const float* taper_xl, int max_slices);
int p3d_patch_plan_destroy(p3d_patch_plan* pplan);
int p3d_patch_plan_info(p3d_patch_plan* pplan, int* npatch, int* max_jobs, int* resident_shape);
int p3d_patch_gather_dev(p3d_patch_plan* pplan, const void* cube_dev, int dtype, int nslices, void* patches_dev);
int p3d_patch_mask_dev(p3d_patch_plan* pplan, const float* mask_dev, int mask_slices, int nslices, float* windows_dev, int* nonbinary);
int p3d_patch_route(p3d_patch_plan* pplan, const p3d_pocs_params* params, int* single_kernel);
int p3d_patch_run_dev(p3d_patch_plan* pplan, const void* patches_dev, int dtype, const double* tau, const uint8_t* active,
                      const p3d_pocs_params* params, void* out_dev, int nslices, int32_t* niter_done, double* sums, double* elapsed_ms);
int p3d_patch_dct_route(p3d_patch_plan* pplan, const p3d_pocs_params* params, int norm, int* single_kernel);
int p3d_patch_dct_run_dev(p3d_patch_plan* pplan, const void* patches_dev, int dtype, const double* tau, const uint8_t* active,
                          const p3d_pocs_params* params, int norm, void* out_dev, int nslices, int32_t* niter_done, double* sums, double* elapsed_ms);
int p3d_patch_blend_dev(p3d_patch_plan* pplan, const void* patches_dev, int dtype, const uint8_t* active, void* out_dev, int nslices);

/* The same loop in the REFERENCE's precision.  POCS_algorithm computes in complex128 / float64 whenever its input is, under NumPy < 2 for every
 * input, and under NumPy >= 2 for the soft / garrote operators, FPOCS and APOCS on complex64 / float32 input as well (threshold_operator.py:37-39,
 * 76-78; POCS.py:566-575, 616: tau, the momentum scalar and the weights 1 - alpha * mask are float64 / complex128).  A plan64 runs
 * fft2 -> threshold -> ifft2 -> re-insertion -> cost in double precision for any slice extents up to 5120: two fused kernels per iteration on tiles
 * of lines in LDS (extents beyond 5088, whose tiles do not fit: six plain passes over the cube).  A precision path, bound by its double-precision
 * butterflies: about a tenth of the float32 rate.  dtype of x and out: P3D_C128, P3D_F64, or P3D_C64 / P3D_F32 (converted on load / store: what the reference's final
 * cast to the input dtype does, cube_POCS_interpolation_3D.py:324); x, out, mask may be host or device pointers; mask is DOUBLE [nil][nxl];
 * tau [nslices][niter][2], stats, sums and the error behaviour as p3d_pocs_stats / p3d_pocs_run; thresh_op: hard, soft, garrote, each also OR-ed
 * with P3D_OP_PERCENTILE (p3d_pocs64_run only: tau then holds the percentages, as in p3d_pocs_run; the threshold of a slice and iteration is
 * np.percentile(|X|, perc) by an exact radix select on the 64-bit moduli with a double interpolation weight, csrc/p3d_select64.hip). */
typedef struct p3d_plan64 p3d_plan64;
int p3d_plan64_create(p3d_plan64** out, int device, int nil, int nxl, int max_slices);
int p3d_plan64_destroy(p3d_plan64* plan);
int p3d_pocs64_stats(p3d_plan64* plan, const void* x, int dtype, int nslices, double* stats_host);
/* test hook: batched fft2 / ifft2 (numpy.fft conventions) of HOST complex128 slices [nslices][nil][nxl] through the loop's own passes (p3d_f64.hip) */
int p3d_fft2_c128(p3d_plan64* plan, const void* in_host, void* out_host, int nslices, int inverse);
int p3d_pocs64_run(p3d_plan64* plan, const void* x, int dtype, const double* mask, const double* tau, const uint8_t* active,
                   const p3d_pocs_params* params, void* out, int nslices, int32_t* niter_done, double* sums, double* elapsed_ms);
/* test hook: thr_host[s] = np.percentile(|spectrum[s]|, perc_host[s]) of HOST complex128 slices [nslices][nil][nxl] through the loop's own select kernels */
int p3d_pocs64_percentile(p3d_plan64* plan, const void* spectrum_host_c128, int nslices, const double* perc_host, double* thr_host);
/* thresh_model = 'data-driven' in double precision: p3d_pocs_sorted_spectrum / p3d_pocs_data_driven_pick above in doubles.  x (host or device, dtype as
 * p3d_pocs64_run) -> fft2 -> 128-bit lexicographic keys sorted per slice, descending, kept in the plan's work buffer; peaks_host [nslices][2] =
 * x_fwd.max(); bounds_host [nslices][4] = tau_min (re, im), tau_max (re, im); tau_host [nslices][niter][2] the picks (double pairs), count_host
 * [nslices] = Nv.  The pick must follow the sort directly (any other call on the plan in between: P3D_ERR_INVALID). */
int p3d_pocs64_sorted_spectrum(p3d_plan64* plan, const void* x, int dtype, int nslices, double* peaks_host);
int p3d_pocs64_data_driven_pick(p3d_plan64* plan, int nslices, int niter, const double* bounds_host, double* tau_host, int64_t* count_host);
/* ... and with scipy.fft.dctn / idctn (type 2, norm: P3D_DCT_BACKWARD / P3D_DCT_ORTHO) in place of fft2 / ifft2: the passes of the float32 DCT loop in
 * double on the same plan64 (csrc/p3d_dct64.hip) -- the plan's line-pass fft2 of the even/odd-reordered iterate, one pass over groups of four coefficients
 * (combine, threshold, split; the factors are doubles), ifft2, and the re-insertion with the reordering folded into its addresses; cost sums without
 * atomics, so results are bitwise repeatable.  Arguments, host-or-device pointers, dtypes, P3D_FLAG_MASK_PER_SLICE, versions, early exit and error
 * behaviour are those of p3d_pocs64_stats / p3d_pocs64_run (thresh_op: hard, soft, garrote -- no percentile variants); real cubes run as complex with
 * zero imaginary part. */
/* test hook: batched dctn (inverse = 0) / idctn (inverse = 1) of HOST complex128 slices through those passes */
int p3d_dct2_c128(p3d_plan64* plan, const void* in_host, void* out_host, int nslices, int inverse, int norm);
int p3d_pocs64_dct_stats(p3d_plan64* plan, const void* x, int dtype, int nslices, double* stats_host, int norm);
int p3d_pocs64_dct_run(p3d_plan64* plan, const void* x, int dtype, const double* mask, const double* tau, const uint8_t* active,
                       const p3d_pocs_params* params, void* out, int nslices, int32_t* niter_done, double* sums, double* elapsed_ms, int norm);

/* Steps 12 / 14 of the workflow: transform every trace of a (nt, ntraces) time-domain cube (ntraces = nil*nxl, the
 * slice-major layout: sample index slowest) to the frequency domain and back, with the conventions of
 *     xrft.fft(da, dim='twt', shift=False, true_phase=True, true_amplitude=True, shape={dim: nfft})
 *                                                                                  cube_apply_FFT.py:240-254
 *     xrft.ifft(da, dim='freq_twt', true_phase=True, true_amplitude=True)          cube_apply_IFFT.py:83-94
 * i.e. F[k] = dt * exp(-2*pi*i*f_k*t0) * sum_n x[n] exp(-2*pi*i*k*n/nfft) = dt * sum_n x[n] exp(-2*pi*i*f_k*(t0 + n*dt)),
 * f_k = fftfreq(nfft, dt)[k], and its exact inverse.  (The xrft fork the reference pins is not available; this is upstream
 * xrft's documented convention.)  For nfft == nt this is what xrft computes whichever way it gets there: its true_phase path
 * rotates the trace by nt/2 samples (ifftshift) and refers the phase to the centre sample t[nt/2], and the two shifts cancel
 * exactly.  For nfft > nt (--upsampling-factor; `shape=` exists only in the fork) the trace is zero-padded at its END here and
 * every sample keeps its physical time t0 + n*dt; an implementation that rotates BEFORE padding would instead place the first
 * half of the trace one record length later (phase exp(-2*pi*i*f_k*nt*dt) on those samples) and report direct_lag = t[nt/2].
 * Which of the two the fork does cannot be established here (parity unpinned); step 14 inverts THIS
 * convention exactly, so 12 -> 13 -> 14 round trips are unaffected, but spectra of an upsampled step 12 should not be mixed
 * with spectra written by the reference's step 12.
 *   p3d_time2freq: x HOST float32 [nt][ntraces] -> out HOST complex64 [nfreq][ntraces]; the trace is zero-padded to
 *       nfft >= nt (--upsampling-factor); real_only != 0 keeps k = 0..nfft/2 (--compute_real, nfreq = nfft/2+1) else
 *       nfreq = nfft; window (HOST float32 [nfreq] or NULL) multiplies every frequency sample (cube_apply_FFT.py:273-278).
 *   p3d_freq2time: X HOST complex64 [nfreq][ntraces] -> out HOST float32 [nfft][ntraces] (real part).  kidx (HOST int32
 *       [nfreq]) gives the FFT bin k of every stored frequency sample (0..nfft-1), so spectra whose filtered samples were
 *       dropped (--drop-filtered-freq) are zero-filled; real_only != 0 completes the Hermitian half.
 * Any nfft up to 10240 (any-length line FFT).  Both allocate their own device buffers on `device`. */
int p3d_time2freq(int device, const float* x, int nt, size_t ntraces, double dt, double t0, int nfft, int real_only,
                  const float* window, void* out);
int p3d_freq2time(int device, const void* X, int nfreq, const int32_t* kidx, size_t ntraces, double dt, double t0, int nfft,
                  int real_only, float* out);
/* the same transforms on DEVICE buffers (x / out of p3d_time2freq, X / out of p3d_freq2time), for callers that keep the cube in HBM
 * across steps 12 -> 13 -> 14; window and kidx stay HOST arrays */
int p3d_time2freq_dev(int device, const float* x_dev, int nt, size_t ntraces, double dt, double t0, int nfft, int real_only,
                      const float* window, void* out_dev);
int p3d_freq2time_dev(int device, const void* X_dev, int nfreq, const int32_t* kidx, size_t ntraces, double dt, double t0, int nfft,
                      int real_only, float* out_dev);

/* Sparse-spectrum statistics of the last p3d_pocs_run[_dev] on this plan: fraction of 8-column blocks of the thresholded spectra
 * that kept at least one coefficient, averaged over slices and iterations (blocks the threshold empties are neither transformed
 * back, stored nor re-read -- exact, since they are zeros); -1 when the dense path ran (shape not eligible, P3D_NO_SPARSE=1,
 * generic lengths). */
int p3d_last_sparsity(p3d_plan* plan, double* nonzero_fraction);

/* After a run with P3D_FLAG_PROFILE: average duration (ms) and launch count of the spectrum
 * (column) pass and of the space (row) pass kernels of the iteration loop. */
int p3d_last_profile(p3d_plan* plan, double* colpass_ms, int* colpass_launches, double* rowpass_ms,
                     int* rowpass_launches);

/* ---- WAVELET variant (transform_kind = 'WAVELET') ---------------------------------------------------------------------------
 * Replaces the pywt.wavedec2 / pywt.waverec2(wavelet, mode='smooth') pair the reference passes to POCS_algorithm
 * (cube_POCS_interpolation_3D.py:260-264; POCS.py:524-525, 585-588, 608-609) and the per-level, per-detail thresholding of
 * threshold_wavelet (POCS.py:105-166).  The caller passes the four filters of the orthogonal / biorthogonal bank (doubles,
 * PyWavelets' dec_lo, dec_hi, rec_lo, rec_hi; 2..64 taps); `level` < 0 selects pywt.dwt_max_level(min(nil, nxl), flen).
 * Coefficients of one slice are a flat complex64 vector: cA, then (cH, cV, cD) of every level, coarsest first (PyWavelets'
 * list order); p3d_wavelet_info reports nlev, the vector length and the (rows, cols) of cA and of each level's details.
 * In p3d_wavelet_stats / p3d_wavelet_run (and p3d_shearlet_stats / p3d_shearlet_run below) the cube pointers `x`, `mask` and `out`
 * may be host OR device pointers (the copy into the plan's staging area is a hipMemcpyDefault): a caller that keeps the cube in
 * HBM pays a device-to-device copy instead of the PCIe transfer.  `elapsed_ms` is the device time of the loop alone. */
typedef struct p3d_wplan p3d_wplan;
int p3d_wavelet_plan_create(p3d_wplan** out, int device, int nil, int nxl, int max_slices, const double* dec_lo,
                            const double* dec_hi, const double* rec_lo, const double* rec_hi, int flen, int level);
int p3d_wavelet_plan_destroy(p3d_wplan* plan);
int p3d_wavelet_info(p3d_wplan* plan, int* nlev, int64_t* ncoef, int32_t* shapes);
/* test hooks: x HOST complex64 [nslices][nil][nxl] <-> coef HOST complex64 [nslices][ncoef] (waverec2 crops to nil x nxl) */
int p3d_wavedec2_c64(p3d_wplan* plan, const void* x, void* coef, int nslices);
int p3d_waverec2_c64(p3d_wplan* plan, const void* coef, void* x, int nslices);
/* statistics for the threshold schedule (POCS.py:253-254, 281): stats HOST double [nslices][nlev][3][4] =
 * (Re, Im of the lexicographic max; max |d|; min |d|) of each detail array, levels coarsest first. dtype as p3d_pocs_run. */
int p3d_wavelet_stats(p3d_wplan* plan, const void* x, int dtype, int nslices, double* stats);
/* the loop (POCS.py:549-632, WAVELET branches).  x/out HOST [nslices][nil][nxl] (dtype), mask HOST float32 [nil][nxl],
 * tau HOST double [nslices][niter][nlev][3][2] (Re, Im), active HOST uint8 [nslices] or NULL, niter_done HOST int32
 * [nslices] or NULL, sums HOST double [niter + 1][nslices] or NULL (sum |x| per iteration; row 0 = the input). */
int p3d_wavelet_run(p3d_wplan* plan, const void* x, int dtype, const float* mask, const double* tau, const uint8_t* active,
                    const p3d_pocs_params* prm, void* out, int nslices, int32_t* niter_done, double* sums,
                    double* elapsed_ms);

/* The WAVELET loop in the REFERENCE's double precision (p3d_wavelet64.hip): pywt.wavedec2 / waverec2 keep float64 for float64 input and
 * POCS_algorithm never narrows (functions/POCS.py:585-588, 596-597, 608-609; threshold_wavelet POCS.py:105-166); the driver casts to the input
 * dtype only at the end (cube_POCS_interpolation_3D.py:324).  Same decomposition, thresholds, schedule layout (tau [nslices][niter][nlev][3][2],
 * stats [nslices][nlev][3][4]) and error behaviour as p3d_wavelet_*; every sample, tap, weight and statistic in double.  dtype of x / out:
 * P3D_C128, P3D_F64, or P3D_C64 / P3D_F32 (converted on load / store); x, out, mask may be host or device pointers; mask is DOUBLE [nil][nxl].
 * A precision path (one thread per output sample and axis, no LDS tiles). */
typedef struct p3d_wplan64 p3d_wplan64;
int p3d_wavelet64_plan_create(p3d_wplan64** out, int device, int nil, int nxl, int max_slices, const double* dec_lo,
                              const double* dec_hi, const double* rec_lo, const double* rec_hi, int filter_len, int level);
int p3d_wavelet64_plan_destroy(p3d_wplan64* plan);
int p3d_wavelet64_info(p3d_wplan64* plan, int* nlev, int64_t* ncoef);
int p3d_wavelet64_stats(p3d_wplan64* plan, const void* x, int dtype, int nslices, double* stats);
int p3d_wavelet64_run(p3d_wplan64* plan, const void* x, int dtype, const double* mask, const double* tau, const uint8_t* active,
                      const p3d_pocs_params* params, void* out, int nslices, int32_t* niter_done, double* sums, double* elapsed_ms);

/* ---- SHEARLET variant (transform_kind = 'SHEARLET') --------------------------------------------------------------------------
 * Replaces FFST.shearletTransformSpect / inverseShearletTransformSpect (cube_POCS_interpolation_3D.py:269-274; POCS.py:526-527,
 * 589-590, 610-611) for spectra Psi supplied by the caller (the reference's `auxiliary_data`): ST_s = ifft2(Psi_s * fft2(x)),
 * x = ifft2(sum_s fft2(ST_s) * Psi_s); per-shearlet thresholds (POCS.py:598 with a (nsh,) tau).  psi: HOST float32
 * [nsh][nil][nxl], FFT order (what fftshift_spectra=True yields), real.  float32 cubes keep real coefficients. */
typedef struct p3d_splan p3d_splan;
int p3d_shearlet_plan_create(p3d_splan** out, int device, int nil, int nxl, int nsh, const float* psi, int max_slices);
int p3d_shearlet_plan_destroy(p3d_splan* plan);
/* How much of the frame the loop has to touch: a shearlet's spectrum vanishes on most rows of the frequency plane (a Parseval frame
 * covers every frequency about twice), and the fused passes skip the 8-row groups on which it does -- exact, those rows carry only
 * zeros through the iteration.  row_group_fraction: share of the (shearlet, 8-row group) pairs that are NOT skipped (1.0: dense
 * path, e.g. P3D_SHEARLET_NO_SUPPORT=1 or the unfused passes).  paired (may be NULL): 1 when float32 cubes take the Hermitian form of
 * the loop -- symmetric spectra (Psi_s(-k) = Psi_s(k), FFST's realCoefficients=True) give real coefficients, the work slices are
 * Hermitian along the rows, so only rows 0 ... nil/2 are computed / stored / read and the column pass sends two columns through
 * one complex transform (results agree with the general form to float32 rounding; P3D_SHEARLET_NO_PAIR=1 switches it off). */
int p3d_shearlet_info(p3d_splan* plan, double* row_group_fraction, int* paired);
/* test hooks: x HOST complex64 [nslices][nil][nxl] <-> st HOST complex64 [nslices][nsh][nil][nxl] */
int p3d_shearlet_transform_c64(p3d_splan* plan, const void* x, void* st, int nslices);
int p3d_shearlet_inverse_c64(p3d_splan* plan, const void* st, void* x, int nslices);
/* statistics for the schedule (POCS.py:257-258, 285, 318): stats HOST double [nslices][nsh][5] = (Re, Im of the lexicographic
 * maximum -- signed maximum for float32 cubes; max |c|; min |c|; sum |c|^2) of each shearlet's coefficients */
int p3d_shearlet_stats(p3d_splan* plan, const void* x, int dtype, int nslices, double* stats);
/* the loop (POCS.py:549-632, SHEARLET branches); arguments as p3d_wavelet_run with tau HOST double [nslices][niter][nsh][2] */
int p3d_shearlet_run(p3d_splan* plan, const void* x, int dtype, const float* mask, const double* tau, const uint8_t* active,
                     const p3d_pocs_params* prm, void* out, int nslices, int32_t* niter_done, double* sums,
                     double* elapsed_ms);
/* The SHEARLET loop in the REFERENCE's double precision (p3d_shearlet64.hip): np.fft.fft2 / ifft2 inside FFST compute in double and hand back
 * complex128 / float64 coefficients, so POCS_algorithm's loop runs in double whatever the cube's dtype; the driver narrows at the end
 * (cube_POCS_interpolation_3D.py:324).  Same frame, thresholds, schedule layout (tau [nslices][niter][nsh][2], stats [nslices][nsh][5]) and error
 * behaviour as p3d_shearlet_*; every sample, spectrum, weight and statistic in double.  psi: HOST DOUBLE [nsh][nil][nxl].  dtype of x / out:
 * P3D_C128, P3D_F64, or P3D_C64 / P3D_F32 (converted on load / store); x, out, mask may be host or device pointers; mask is DOUBLE [nil][nxl].
 * Three fused passes per iteration over the coefficients where both extents have a plan on the double-precision register engine (p3d_mix64.hip), unfused
 * passes on the line transforms of p3d_plan64 otherwise. */
typedef struct p3d_splan64 p3d_splan64;
int p3d_shearlet64_plan_create(p3d_splan64** out, int device, int nil, int nxl, int nsh, const double* psi, int max_slices);
int p3d_shearlet64_plan_destroy(p3d_splan64* plan);
/* fused: 1 when the loop runs its three fused passes on the double-precision register engine (both extents have a plan there; P3D_SHEARLET64_UNFUSED=1 at
 * plan creation switches them off; bit 1 set as well -- 3 -- when REAL cubes take the Hermitian form of those passes: symmetric spectra, even extents, rows
 * 0 ... nil/2 only and two columns per transform, P3D_SHEARLET64_NO_PAIR=1 switches it off), 0 for the unfused passes; row_group_fraction (may be NULL): share of the (shearlet, row group) pairs the fused passes
 * touch -- rows on which a shearlet's spectrum vanishes are skipped, exactly (1.0: none skipped; P3D_SHEARLET64_NO_SUPPORT=1) */
int p3d_shearlet64_info(p3d_splan64* plan, int* fused, double* row_group_fraction);
/* 1 when a plan for (nil, nxl) slices would run the fused passes */
int p3d_shearlet64_fused_shape(int nil, int nxl);
int p3d_shearlet64_stats(p3d_splan64* plan, const void* x, int dtype, int nslices, double* stats);
int p3d_shearlet64_run(p3d_splan64* plan, const void* x, int dtype, const double* mask, const double* tau, const uint8_t* active,
                       const p3d_pocs_params* params, void* out, int nslices, int32_t* niter_done, double* sums, double* elapsed_ms);

/* ---- step-15 slice smoothing (cube_postprocessing_3D.py:88-124 wraps scipy.ndimage.gaussian_filter / median_filter) ----------
 * x/out HOST float32 [nslices][ny][nx]; boundary mode 'reflect'.  gaussian: separable, radius int(truncate * sigma + 0.5);
 * median: size x size window, size in {3, 5, 7}. */
int p3d_smooth_gaussian(int device, const float* x, size_t nslices, int ny, int nx, double sigma, double truncate, float* out);
int p3d_smooth_median(int device, const float* x, size_t nslices, int ny, int nx, int size, float* out);

/* ---- step-15 automatic gain control (functions/signal.py:325-409, zero padding) along the time axis ----------------------------
 * x/out HOST float32 [nt][ntraces] (time-slow: the slice-major (twt, iline, xline) cube); win: samples (an even win is made odd);
 * kind 0 = rms, 1 = mean, 2 = median; squared: sign(y) * y^2 of the gained trace; gain (may be NULL): HOST float32 [nt][ntraces],
 * the gain function g (0 replaced by 1).  Cubes larger than the free device memory go through in chunks of traces. */
int p3d_agc(int device, const float* x, size_t nt, size_t ntraces, int win, int kind, int squared, float* out, float* gain);

/* the same on DEVICE buffers [nt][ntraces] (x_dev != out_dev; gain_dev may be NULL), one pass over the whole cube (no chunking) */
int p3d_agc_dev(int device, const float* x_dev, size_t nt, size_t ntraces, int win, int kind, int squared, float* out_dev, float* gain_dev);

/* ---- step-11 pre-processing (cube_preprocessing_3D.py), csrc/p3d_preproc.hip ------------------------------------------------------
 * Every cube argument is a DEVICE float32 matrix [nt][ntraces] (time-slow); every table argument is a HOST array designed in NumPy.
 * Callers split cubes larger than the device memory into chunks of traces (every operation is per trace).
 *   p3d_pre_reduce_dev:  res[ntraces] = rms (kind 0, sqrt(sum x^2 / nt)) or max |x| (kind 1) of every trace, 0 replaced by 1;
 *       kind 2: the rms without that replacement.
 *   p3d_pre_balance_dev: the same into ref[ntraces], then out = x / ref (trace balancing).
 *   p3d_pre_gain_dev:    the reference's gain() along twt.  prm: doubles indexed by P3D_GAIN_* (flags: OR of the P3D_GAIN_* bits);
 *       curves: HOST [4][nt] doubles (tpow, epow, linear, pgc factors; pgc is applied in float32), NULL when no curve is used; work:
 *       DEVICE [nt][ntraces] floats, needed with AGC, qclip or norm_rms splitting the pass (may be NULL otherwise).
 *   p3d_pre_sosfiltfilt_dev: scipy.signal.sosfiltfilt(sos, x, padtype='odd', padlen) along twt, sos / zi HOST [nsec][6] / [nsec][2]
 *       (sosfilt_zi), double-precision recursion; work: DEVICE [nt + 2 padlen][ntraces] floats for nsec <= 8, DOUBLES (8-byte
 *       aligned) for longer cascades, which run in groups of 8 sections with the signal between the groups held in double; or NULL
 *       (allocated).  A misaligned work buffer is refused (P3D_ERR_INVALID), and so is one too short where the runtime can tell: the
 *       room is counted to the end of the allocation that holds the pointer (best effort: not for another allocator's memory).
 *   p3d_pre_upfirdn_dev: out[i] = sum_q h[(pre_remove + i) down - up q] x[q], i < nout (scipy's resample_poly after its padding).
 *   p3d_pre_spectral_dev: forward FFT of x at length nt; Z[k] = op(fac[k] X[src[k] >> 2]) for k < num (op = src & 3: 0 plain, 1
 *       conjugate, 2 real part; src < 0: 0); inverse FFT at length num (unnormalised); out = |Z| * s1 (modulus) or Re Z * s1 * s2.
 *       FFT lengths up to 10240 (P3D_ERR_UNSUPPORTED beyond); work: DEVICE (nt + num) * ntraces complex64 or NULL (allocated). */
enum {
    P3D_GAIN_FLAGS = 0, P3D_GAIN_BIAS = 1, P3D_GAIN_GPOW = 2, P3D_GAIN_AGC_WIN = 3, P3D_GAIN_AGC_KIND = 4, P3D_GAIN_AGC_SQRT = 5,
    P3D_GAIN_CLIP = 6, P3D_GAIN_PCLIP = 7, P3D_GAIN_NCLIP = 8, P3D_GAIN_QCLIP = 9, P3D_GAIN_SCALE = 10, P3D_GAIN_NPRM = 11
};
/* flag bits (prm[P3D_GAIN_FLAGS]); the bit of an entry with a parameter has the entry's name with an F_ prefix */
#define P3D_GAIN_F_BIAS 1u
#define P3D_GAIN_F_TPOW 2u
#define P3D_GAIN_F_EPOW 4u
#define P3D_GAIN_F_GPOW 8u
#define P3D_GAIN_F_AGC 16u
#define P3D_GAIN_F_CLIP 32u
#define P3D_GAIN_F_PCLIP 64u
#define P3D_GAIN_F_NCLIP 128u
#define P3D_GAIN_F_QCLIP 256u
#define P3D_GAIN_F_LINEAR 512u
#define P3D_GAIN_F_PGC 1024u
#define P3D_GAIN_F_NORM_RMS 2048u
#define P3D_GAIN_F_SCALE 4096u
#define P3D_GAIN_F_NORM 8192u
#define P3D_GAIN_NBITS 14
int p3d_pre_reduce_dev(int device, const float* x_dev, size_t nt, size_t ntraces, int kind, float* res_dev);
int p3d_pre_balance_dev(int device, const float* x_dev, size_t nt, size_t ntraces, int kind, float* out_dev, float* ref_dev);
int p3d_pre_gain_dev(int device, const float* x_dev, size_t nt, size_t ntraces, const double* prm, const double* curves, float* out_dev,
                     float* work_dev);
int p3d_pre_sosfiltfilt_dev(int device, const float* x_dev, size_t nt, size_t ntraces, int nsec, const double* sos, const double* zi, int padlen,
                            float* out_dev, void* work_dev);
int p3d_pre_upfirdn_dev(int device, const float* x_dev, size_t nt, size_t ntraces, const double* h, int nh, int up, int down, long long pre_remove,
                        size_t nout, float* out_dev);
int p3d_pre_spectral_dev(int device, const float* x_dev, size_t nt, size_t ntraces, int num, const int* src, const float* fac, int modulus,
                         double s1, double s2, float* out_dev, void* work_dev);

/* ---- step-15 iline / xline upsampling (cube_postprocessing_3D.py:350-488) ---------------------------------------------------------
 * x HOST [nslices][ny][nx], out HOST [nslices][my][mx], dtype P3D_F32 or P3D_C64.  Output line o of the iline axis reads source line
 * iy[o] and, when wy[o] != 0, line iy[o] + 1 with weight wy[o] in [0, 1) (the same for the xline axis with ix / wx); float32 arithmetic. */
int p3d_upsample(int device, const void* x, int dtype, size_t nslices, int ny, int nx, const int* iy, const float* wy, int my, const int* ix,
                 const float* wx, int mx, void* out);

/* ---- step-10 trace stacking into the binned cube (cube_binning_3D.py:922-1240), csrc/p3d_binning.hip -----------------------------------
 * CSR input built by the host: traces sorted into bin order, bin b = il * nxl + xl owns traces bin_start[b] .. bin_start[b + 1] - 1
 * (bin_start: nil * nxl + 1 entries over ALL bins, from 0 to ntraces).  Trace t: samples[trace_off[t] .. + trace_len[t]) (float32);
 * its sample i lands on output sample j = i + shift[t], zero outside 0 <= i < trace_len[t] (the padding counts).  weight: normalised
 * float64 weights (IDW only, may be NULL otherwise).  out: [nt][nil][nxl] float32 (slice-major), empty bins 0.
 * method 0 = average (double sum / k), 1 = median (exact, np.median of the float32 stack), 2 = nearest (the first trace of the bin),
 * 3 = IDW (double sum of w * x).  No atomics: bitwise repeatable.
 *   p3d_bin_stack: HOST buffers; runs in chunks of whole inlines so that the chunk's cube slab, its span of samples and its tables fit in
 *       half of the free device memory, or in max_bytes when that is smaller (0: no cap); a single inline beyond it is P3D_ERR_UNSUPPORTED.
 *   p3d_bin_stack_dev: DEVICE buffers, one launch over the whole cube. */
int p3d_bin_stack(int device, const float* samples, const long long* trace_off, const int* trace_len, const int* shift, const double* weight,
                  size_t ntraces, const long long* bin_start, int nil, int nxl, int nt, int method, size_t max_bytes, float* out);
int p3d_bin_stack_dev(int device, const float* samples_dev, const long long* trace_off_dev, const int* trace_len_dev, const int* shift_dev,
                      const double* weight_dev, const long long* bin_start_dev, int nil, int nxl, int nt, int method, float* out_dev);

/* ---- step 8: despiking of a 2-D section (p3d_despike.hip; the reference's despike_2D) -------------------------------------------------------
 * The section is trace-major [ntr][ns] float32, the layout of the SEG-Y file.  w: odd number of adjacent traces, 3 ... P3D_DESPIKE_MAX_TRACES
 * (larger: P3D_ERR_UNSUPPORTED); mode 0 = mean, 1 = median, 2 = rms of |a| over the w traces of a window, per sample row.
 *   detect: sample (t, x) is a candidate if |a[t][x]| > threshold * (the smallest window value among the windows that contain trace x), in
 *       float32 with NumPy's order of summation.  Rows t < main_end (main view) or t >= add_start (additional view; pass INT_MAX for none) are
 *       examined.  splits: nsplits + 1 ascending trace boundaries from 0 to ntr on the HOST (NULL / 0: one split); windows never cross one.
 *       mask [ntr][(ns + 63) / 64]: bit t % 64 of word t / 64 of trace x; counts [2][ntr]: candidates per trace in the main / additional view.
 *   replace: spike records of 8 ints (trace, lo, hi, first, last, c0, c1, 0) on the HOST, sorted by level; level l owns records
 *       level_start[l] .. level_start[l + 1] and is one launch.  Rows lo .. hi of the trace are rewritten from columns c0 .. c1 (at most
 *       P3D_DESPIKE_MAX_TRACES): out 0 = scaled (a / (max(a) / f(|win|)) * blackman, taper in double), 1 = mode (f(win)), 2 = threshold
 *       (f(win) * threshold), 3 = zeros, 4 = median (np.median of win).
 * The plain entry points take HOST sections / masks / counts, the _dev ones DEVICE buffers (the section never leaves the device between the two). */
#define P3D_DESPIKE_MAX_TRACES 31
int p3d_despike_detect(int device, const float* section, int ntr, int ns, int w, int mode, float threshold, int main_end, int add_start, const int* splits,
                       int nsplits, unsigned long long* mask, int* counts);
int p3d_despike_detect_dev(int device, const float* section_dev, int ntr, int ns, int w, int mode, float threshold, int main_end, int add_start,
                           const int* splits, int nsplits, unsigned long long* mask_dev, int* counts_dev);
int p3d_despike_replace(int device, float* section, int ntr, int ns, const int* spikes, size_t nspikes, const int* level_start, int nlevels, int mode, int out,
                        float threshold);
int p3d_despike_replace_dev(int device, float* section_dev, int ntr, int ns, const int* spikes, size_t nspikes, const int* level_start, int nlevels, int mode,
                            int out, float threshold);

/* ---- step 5: static correction of a 2-D section (p3d_static.hip; the reference's detect_seafloor_reflection / compensate_static) --------------
 * The section is trace-major [ntr][ns] float32.  The valid slice of trace x is [0, ns) (padded = 0) or [max(first[x], 0), + nvalid) cut at the end
 * of the trace (padded = 1: a zero-padded file); row numbers below count from the start of the slice.
 *   scan:   first[x] = index of the first non-zero sample, -1 for a trace of zeros (such traces are left out of everything that follows:
 *           peak 0, cross 0, peak_idx -1).
 *   stalta: c = running sum of a^2 (double), sta = (c[i] - c[i - nsta]) / nsta (c[i] / nsta for i < nsta), lta alike, sta = 0 for i < nlta - 1,
 *           ratio = sta / lta (0 where lta == 0); 1 <= nsta <= nlta <= P3D_STATIC_MAX_NLTA (larger: P3D_ERR_UNSUPPORTED).
 *           max:   peak[x] = the largest ratio of rows nlta ... 2 nlta - 1 (0 when the slice has no such row);
 *           cross: cross[x] = the first row whose ratio exceeds threshold (0 when none does).  The ratio is never stored.
 *   peak:   window base[x] - win ... base[x] + win, clipped to the slice; the n largest (signed) amplitudes, equal ones by ascending position;
 *           their positions ascending p[0] < p[1] < ..., the group p[:i] with i the first index where p[i + 1] - p[i] > 1 (p[:1] for i = 0, all
 *           when there is no gap); peak_idx[x] = the position (row of the slice) of the largest amplitude of the group.  1 <= win <=
 *           P3D_STATIC_MAX_WIN, 1 <= n <= 2 win + 1 (beyond: P3D_ERR_UNSUPPORTED); 0 <= base[x] < rows of the slice is the caller's duty
 *           (a window that misses the slice altogether yields -1).
 *   shift:  out[x][t] = in[x][t - shift[x]] where 0 <= t - shift[x] < ns, else 0; in and out must not overlap.
 * The _dev entry points take DEVICE buffers and return after the kernels have finished; detect / peak / shift take HOST arrays.  detect = scan, then
 * (when *threshold is NaN) max and *threshold = the largest peak of the live traces, then cross. */
#define P3D_STATIC_MAX_WIN 255
#define P3D_STATIC_MAX_NLTA 7680
int p3d_static_scan_dev(int device, const float* section_dev, int ntr, int ns, int* first_dev);
int p3d_static_stalta_max_dev(int device, const float* section_dev, int ntr, int ns, const int* first_dev, int padded, int nvalid, int nsta, int nlta,
                              double* peak_dev);
int p3d_static_stalta_cross_dev(int device, const float* section_dev, int ntr, int ns, const int* first_dev, int padded, int nvalid, int nsta, int nlta,
                                double threshold, int* cross_dev);
int p3d_static_peak_dev(int device, const float* section_dev, int ntr, int ns, const int* first_dev, int padded, int nvalid, const int* base_dev, int win,
                        int n, int* peak_idx_dev);
int p3d_static_shift_dev(int device, const float* in_dev, int ntr, int ns, const int* shift_dev, float* out_dev);
int p3d_static_detect(int device, const float* section, int ntr, int ns, int padded, int nvalid, int nsta, int nlta, double* threshold, int* first,
                      int* cross);
int p3d_static_peak(int device, const float* section, int ntr, int ns, const int* first, int padded, int nvalid, const int* base, int win, int n,
                    int* peak_idx);
int p3d_static_shift(int device, const float* section, int ntr, int ns, const int* shift, float* out);

/* ---- step 7: mistie correction of crossing 2-D lines (p3d_mistie.hip; the reference's mistie_correction_segy.py) -----------------------------------
 * Lines: all vertices (shot points) as doubles xy [nv][2] (x, y), line L owns vertices line_off[L] ... line_off[L + 1] - 1 (line_off: HOST, nlines + 1
 * entries from 0 to nv, also in the _dev entry points: a small table); segment s of a line joins its vertices s and s + 1.
 *   cross:   every point at which a segment of line i meets a segment of line j, for the line pairs (i, j), 0 <= i < j < nlines, of pairs [npairs][2]
 *            (HOST; the caller keeps the pairs whose bounding boxes overlap).  A segment pair is a hit when it crosses properly, touches at an end
 *            point or shares a vertex (the point is then that vertex, exactly); otherwise the point is A0 + t (A1 - A0) on line i's segment.  Collinear
 *            overlapping segments give the two ends of the overlap (part 0 and 1; one point when they coincide).  Segments are taken in tiles of 64 and
 *            tile pairs with disjoint bounding boxes are skipped.  Hits are appended IN NO DEFINED ORDER to hits[capacity]; *needed is the number of hits
 *            found, which may exceed capacity (then the first `capacity` appended ones were stored: call again with a buffer of *needed).  One crossing
 *            through a shared vertex of consecutive segments is found once per segment: callers sort by (pair, seg_i, seg_j, part) and drop repeated
 *            points.
 *   nearest: for crossing c at points[c] and side s in {0, 1}, the vertex of line lines[c][s] nearest to the point: index[c][s] (first minimum of
 *            sqrt(dx^2 + dy^2) in double, the whole line is searched; -1 for a line without vertices or a line number out of range) and dist[c][s].
 *   xcorr:   a, b float32 [ncross][ns]; ranges [ncross][4] = (first sample, length) of the window of a and of b.  Per crossing: the samples at which
 *            either trace is exactly 0 are dropped, n remain; cc = scipy.signal.correlate(a, b, mode='same') by direct sums in double (lags
 *            -(n / 2) ... n - 1 - n / 2); k = the first arg max of cc if |max| >= |min| else the first arg min; shift = n / 2 - k; coeff = Pearson's r
 *            of the n samples (double; NaN when a trace is constant, n = 1 included).  status: 0 fine, P3D_MISTIE_EMPTY no sample left,
 *            P3D_MISTIE_LENGTHS the two windows differ in length, P3D_MISTIE_RANGE a window outside the trace (or longer than max_len); shift, coeff
 *            and n are 0 then.  path: AUTO keeps the compacted traces in LDS when the longest window has at most P3D_MISTIE_LDS_SAMPLES samples, else in
 *            global memory (work: DEVICE [ncross][2][ns] floats, or NULL: allocated); LDS / GLOBAL force one form (LDS beyond the limit:
 *            P3D_ERR_UNSUPPORTED).  Both forms give identical results.  max_len (_dev only): the longest window of the batch.
 * Applying a line's offset needs no entry of its own: p3d_static_shift with one shift for all traces. */
#define P3D_MISTIE_LDS_SAMPLES 8064
#define P3D_MISTIE_PATH_AUTO 0
#define P3D_MISTIE_PATH_LDS 1
#define P3D_MISTIE_PATH_GLOBAL 2
#define P3D_MISTIE_EMPTY 1
#define P3D_MISTIE_LENGTHS 2
#define P3D_MISTIE_RANGE 3
typedef struct p3d_mistie_hit {
    int32_t pair, seg_i, seg_j, part;
    double x, y;
} p3d_mistie_hit;
int p3d_mistie_cross_dev(int device, const double* xy_dev, const long long* line_off, int nlines, const int* pairs, int npairs, p3d_mistie_hit* hits_dev,
                         size_t capacity, size_t* needed);
int p3d_mistie_nearest_dev(int device, const double* xy_dev, const long long* line_off, int nlines, const double* points_dev, const int* lines_dev,
                           size_t ncross, int* index_dev, double* dist_dev);
int p3d_mistie_xcorr_dev(int device, const float* a_dev, const float* b_dev, size_t ncross, int ns, const int* ranges_dev, int max_len, int path,
                         float* work_dev, int* shift_dev, double* coeff_dev, int* n_dev, int* status_dev);
int p3d_mistie_cross(int device, const double* xy, const long long* line_off, int nlines, const int* pairs, int npairs, p3d_mistie_hit* hits, size_t capacity,
                     size_t* needed);
int p3d_mistie_nearest(int device, const double* xy, const long long* line_off, int nlines, const double* points, const int* lines, size_t ncross, int* index,
                       double* dist);
int p3d_mistie_xcorr(int device, const float* a, const float* b, size_t ncross, int ns, const int* ranges, int path, int* shift, double* coeff, int* n,
                     int* status);

/* ---- steps 3 and 4: DelayRecordingTime correction and padding (p3d_delrt.hip; the reference's delrt_correction_segy.py / delrt_padding_segy.py) ----
 * Sections are trace-major float32 and start at 16-byte boundaries (any hipMalloc'ed buffer does).  Both operations only copy and compare, so the
 * results are bit-identical to NumPy's; NaN samples are outside the contract (a comparison with NaN never holds: NaNs are skipped).
 *   pad:     out[x][t] = in[x][t - top[x]] for top[x] <= t < top[x] + ns_in, else 0; in [ntr][ns_in], out [ntr][ns_out], ns_out >= ns_in, top one int
 *            per trace; in and out must not overlap.  top[x] < 0 or top[x] + ns_in > ns_out: P3D_ERR_INVALID before anything is launched (the _dev
 *            entry copies its DEVICE table back for this check).
 *   windows: for delay change c with reference trace ref[c] (n_traces <= ref[c] <= ntr - 1 - n_traces, else P3D_ERR_INVALID before the launch):
 *            peak_val[c] = the maximum of trace ref[c] and peak_idx[c] = the FIRST row that holds it (np.argmax);
 *            maxima[c][j], j = 0 ... 2 n_traces = the maximum of trace ref[c] - n_traces + j over rows [max(peak_idx - n_samples / 2, 0),
 *            min(peak_idx + n_samples / 2 + 1, ns)) -- the plain maximum: the reference's clipping to peak_val is left to the caller.
 *            All changes of a file go in one launch (m = 0: nothing is done).  n_traces >= 1, n_samples >= 1.
 * p3d_delrt_pad_dev: all pointers DEVICE.  p3d_delrt_windows_dev: the section and the three results DEVICE, ref HOST (m entries, a small table).
 * p3d_delrt_pad / p3d_delrt_windows take HOST arrays; windows takes the packed subsets [m][2 n_traces + 1][ns] (only the traces that are needed
 * cross the bus), which are a section of their own with ref[c] = c (2 n_traces + 1) + n_traces: the same kernel serves both forms. */
int p3d_delrt_pad_dev(int device, const float* in_dev, int ntr, int ns_in, int ns_out, const int* top_dev, float* out_dev);
int p3d_delrt_pad(int device, const float* section, int ntr, int ns_in, int ns_out, const int* top, float* out);
int p3d_delrt_windows_dev(int device, const float* section_dev, int ntr, int ns, const int* ref, int m, int n_traces, int n_samples, int* peak_idx_dev,
                          float* peak_val_dev, float* maxima_dev);
int p3d_delrt_windows(int device, const float* subsets, int m, int ns, int n_traces, int n_samples, int* peak_idx, float* peak_val, float* maxima);

/* ---- step 2: reprojection of header coordinates (p3d_proj.hip; the reference's reproject_segy.py, which takes the projection from pyproj) ----
 * Transverse Mercator between geographic degrees and projected metres on one ellipsoid, all arithmetic in double: the Krueger series in the
 * third flattening to n^6 (Karney 2011), accurate to nanometres within a few degrees of the central meridian and to well under a micrometre
 * over a UTM zone with its neighbours.  prm = {a, f, lon0_deg, lat0_deg, k0, x0, y0} (HOST, 7 doubles): semi-major axis, flattening,
 * central meridian, latitude of origin, scale on the central meridian, false easting, false northing.  The series constants are computed
 * on the host per call and passed to the kernel by value.
 *   inverse == 0: (x, y) = (longitude, latitude) in degrees -> (ox, oy) = (easting, northing);
 *   inverse != 0: (x, y) = (easting, northing) -> (ox, oy) = (longitude, latitude) in degrees (Newton's iteration for the latitude: 5 steps, fixed).
 * One thread per point; ox may be x and oy may be y (in place), no other overlap.  Non-finite inputs give non-finite outputs (no error).
 * p3d_proj_tmerc_dev: the four arrays DEVICE.  p3d_proj_tmerc: the four arrays HOST.  n = 0: nothing is done.
 *   smooth: out[i] = sum_k padded[i + k] * w[wlen - 1 - k], k = 0 ... wlen - 1 in this order, i = 0 ... n - 1 (np.convolve(padded, w, 'valid')):
 *   padded DEVICE with n + wlen - 1 samples, out DEVICE with n samples (another buffer), w HOST with wlen >= 1 weights. */
int p3d_proj_tmerc_dev(int device, const double* x_dev, const double* y_dev, size_t n, const double* prm, int inverse, double* ox_dev, double* oy_dev);
int p3d_proj_tmerc(int device, const double* x, const double* y, size_t n, const double* prm, int inverse, double* ox, double* oy);
int p3d_proj_smooth_dev(int device, const double* padded_dev, size_t n, const double* w, int wlen, double* out_dev);

/* ---- step 6: tide compensation (p3d_tide.hip; the reference's tide_compensation_segy.py, which takes the prediction from tpxo-tide-prediction) ----
 * Harmonic tide prediction along a track, all arithmetic in double, one thread per point.  Point i has lon[i], lat[i] in degrees and t[i] in seconds
 * since 1992-01-01T00:00:00 (may be negative).  The tables are a SUBSET of a tidal atlas on a uniform grid: node (i, j) lies at (lon0 + i dlon,
 * lat0 + j dlat), grid = {lon0, dlon, lat0, dlat} (HOST, 4 doubles, both spacings positive); hre / him int32 [nc][nxs][nys] hold the real and imaginary
 * part of the elevation constants in millimetres, wet uint8 [nxs][nys] is non-zero on water; nxs, nys >= 2.  The longitudes are already unwrapped
 * onto the subset's axis.  ids (HOST, nc ints, 1 <= nc <= P3D_TIDE_CONSTITUENTS) name the constituent of each table plane: m2, s2, n2, k2, k1, o1, p1,
 * q1, m4, mf, 2n2, mm, mn4, ms4 = 0 ... 13, with the frequencies and phases of OTPS constit.h.
 *   per point: the bilinear weights of the enclosing cell (a point on the last row or column uses the last cell with weights 0 / 1); the weights of
 *   dry nodes are dropped and the rest divided by their sum; the result is NaN when the four nodes are dry or the remaining weights sum to 0, and
 *   also for a non-finite point or one more than 1e-9 of a cell outside the subset (no table is read then).  z_c = (sum w hre + i sum w him) / 1000.
 *   T = t / 86400 + 48622 - 51544.4993 days, N = (125.0445 - 0.05295377 T) mod 360 degrees; the nodal factor f_c and phase u_c of OTPS `nodal` from
 *   sin / cos of N, 2 N, 3 N;  tide = sum_c f_c (Re z_c cos theta_c - Im z_c sin theta_c),  theta_c = omega_c t + phi0_c + u_c, in metres.
 * Entry with the _dev suffix: lon, lat, t, hre, him, wet and tide DEVICE (tide a buffer of its own).  Entry without it: all of them HOST.  n = 0: nothing is done. */
#define P3D_TIDE_CONSTITUENTS 14
int p3d_tide_predict_dev(int device, const double* lon_dev, const double* lat_dev, const double* t_dev, size_t n, const int* hre_dev, const int* him_dev,
                         const unsigned char* wet_dev, int nc, int nxs, int nys, const double* grid, const int* ids, double* tide_dev);
int p3d_tide_predict(int device, const double* lon, const double* lat, const double* t, size_t n, const int* hre, const int* him, const unsigned char* wet,
                     int nc, int nxs, int nys, const double* grid, const int* ids, double* tide);

/* ---- steps 9 and 16: SEG-Y <-> float32 sections (p3d_segy.hip; the reference's cnv_segy2netcdf.py / cube_cnv_netcdf2segy_3D.py, which use segysak) ----
 * A record is a 240-byte trace header followed by ns samples, all big-endian; ns = 1 ... 65535.  The sample conversions are bit-identical to
 * functions/segy.py (ieee2ibm: mantissa to nearest, ties to even; +-0 and NaN -> 0, +-Inf -> 0x7FFFFFFF / 0xFFFFFFFF; ibm2ieee: NumPy's cast of the
 * exact double, so subnormals are rounded to nearest-even, larger magnitudes become +-inf and a zero mantissa keeps its sign).
 *   encode: section float32, trace-major [ntr][ns] or slice-major [ns][ntr] (the ('twt', 'iline', 'xline') cube, ntr = nil nxl) -> ntr records of
 *           240 + 4 ns bytes in format 1 (IBM) or 5 (IEEE).  Every header is the 240-byte template overlaid with the columns: column c puts
 *           values[c][x] (int32) as a big-endian word of columns[c][1] = 2 or 4 bytes (the low 16 bits for 2) at byte offset columns[c][0] of
 *           trace x's header.  columns: HOST, [ncol][2], ncol <= P3D_SEGY_MAX_COLUMNS; values: [ncol][ntr].
 *   decode: records of 240 + ns bytes(fmt) bytes, fmt 1, 2 (int32), 3 (int16), 5, 8 (int8) -> samples float32 [ntr][ns] (integers converted as NumPy's
 *           astype(float32) converts them) and words[k][x] = the header word of fields[k] = {byte offset, width 2 | 4, signed != 0} of trace x, as
 *           int32 (an unsigned 4-byte word keeps its bit pattern).  fields: HOST, [nf][3], nf <= P3D_SEGY_MAX_COLUMNS; words: [nf][ntr].
 * P3D_ERR_INVALID before anything is launched: ns outside 1 ... 65535, another format or layout, more than 16 columns / fields, a width other than
 * 2 or 4, a column / field that leaves the 240 bytes or overlaps another.  ntr = 0: nothing is done.
 * Entries with the _dev suffix: the section, the records, the template, values and words DEVICE; section and records start at 16-byte boundaries
 * and do not overlap.  Entries without it: all of them HOST. */
#define P3D_SEGY_MAX_COLUMNS 16
#define P3D_SEGY_TRACE_MAJOR 0
#define P3D_SEGY_SLICE_MAJOR 1
int p3d_segy_encode_dev(int device, const float* section_dev, int ntr, int ns, int layout, int fmt, const unsigned char* template_dev, const int* columns,
                        int ncol, const int* values_dev, unsigned char* records_dev);
int p3d_segy_encode(int device, const float* section, int ntr, int ns, int layout, int fmt, const unsigned char* tmpl, const int* columns, int ncol,
                    const int* values, unsigned char* records);
int p3d_segy_decode_dev(int device, const unsigned char* records_dev, int ntr, int ns, int fmt, const int* fields, int nf, float* samples_dev, int* words_dev);
int p3d_segy_decode(int device, const unsigned char* records, int ntr, int ns, int fmt, const int* fields, int nf, float* samples, int* words);

/* ---- step 1: merging short SEG-Y files with their neighbours (p3d_merge.hip; the reference's merge_segys.py, which uses pandas and segyio) ----
 * A record is a 240-byte trace header followed by the samples, reclen = 240 ... 240 + 4 * 65535 bytes in all, of any sample format: samples are
 * moved as bytes.  The records of a group of files lie back to back.
 *   keys:    per record TRACE_SEQUENCE_LINE (bytes 1-4, int32) and two 64-bit fingerprints of its header: of all 240 bytes (fp_full) and of all
 *            but bytes 5-8, TRACE_SEQUENCE_FILE (fp_sub).  Equal headers give equal fingerprints; the converse is the caller's to confirm.
 *            Dword l = 0 ... 59 of the header, read as a little-endian d, contributes splitmix64((l + 1) << 32 | d); the terms are XORed.
 *   records: nout output records from a plan of three int tables [nout].  src[r] >= 0: record src[r], verbatim but for bytes 5-8 = r + 1
 *            (big-endian).  src[r] = -1: a gap between the rows lo_row[r] < r < hi_row[r], which hold records: each of the 91 header words (SEG-Y
 *            rev 1, 2 or 4 bytes, signed) is  (int32)(slope * (r - lo) + v_lo), slope = (v_hi - v_lo) / (hi - lo)  in IEEE double without fused
 *            multiply-add (pandas' linear interpolation cast to int32), stored with its width; bytes 5-8 = r + 1; the samples are zero bytes.
 *            lo_row / hi_row are read for gap rows only.
 * P3D_ERR_INVALID before anything is launched and before any memory is touched: reclen out of range, nsrc < 1 or nout < 1, src[r] outside
 * -1 ... nsrc - 1, a gap in the first or the last row, a gap whose lo_row / hi_row do not enclose it inside 0 ... nout - 1 or are gaps themselves,
 * output records that overlap the input.  keys with n = 0: nothing is done.
 * Entries with the _dev suffix: the records and the results DEVICE (any alignment of the records; 16-byte stores when reclen and both record
 * buffers are multiples of 16, 4-byte stores for multiples of 4, single bytes otherwise); the plan is a HOST table in both forms.  Entries
 * without the suffix: everything HOST. */
int p3d_merge_keys_dev(int device, const unsigned char* records_dev, int n, int reclen, int* tracl_dev, uint64_t* fp_full_dev, uint64_t* fp_sub_dev);
int p3d_merge_keys(int device, const unsigned char* records, int n, int reclen, int* tracl, uint64_t* fp_full, uint64_t* fp_sub);
int p3d_merge_records_dev(int device, const unsigned char* records_dev, int nsrc, int reclen, int nout, const int* src, const int* lo_row, const int* hi_row,
                          unsigned char* out_dev);
int p3d_merge_records(int device, const unsigned char* records, int nsrc, int reclen, int nout, const int* src, const int* lo_row, const int* hi_row,
                      unsigned char* out);

/* ---- 3-D FFT POCS: a whole volume as ONE job (csrc/p3d_vol.hip) ------------------------------------------------------------------------------
 * POCS_algorithm(x, mask, transform=np.fft.fftn, itransform=np.fft.ifftn, transform_kind='FFT', ...) on a volume x of (n0, n1, n2) points,
 * C-contiguous, n2 fastest: the spectrum couples all three axes, there is one schedule, one cost, one iteration count and one early exit for
 * the volume.  Per iteration: the fft2 passes of a p3d_plan for (n1, n2) slices, one kernel that transforms a tile of plane positions along
 * axis 0, thresholds and transforms back (the 3-D spectrum never goes to memory), the ifft2 passes, and the re-insertion with cost sums
 * folded in a fixed order (results are bitwise repeatable).  float32 kernels: complex64 volumes, or float32 ones, which run as complex
 * with a zero imaginary part and return the real part.
 *   shape_supported  1 when n0 is a 7-smooth length from 1 to 1024 (n0 = 1: the axis-0 pass thresholds only) and p3d_shape_supported(n1, n2)
 *   create   `plan`: a p3d_plan for (n1, n2) slices on `device` to borrow (not owned: it must outlive the volume plan, which runs on its stream
 *            and is as little re-entrant), or NULL: the volume plan creates and owns one.  Allocates the complex64 work volume.
 *            P3D_ERR_UNSUPPORTED for any other n0 or slice shape
 *   fft3     np.fft.fftn (inverse = 0) / ifftn (inverse = 1) of one complex64 volume through the loop's own passes; test hook like p3d_fft2_c64;
 *            in == out is allowed
 *   shrink   threshold(fftn(x), tau, thresh_op), tau HOST [2] doubles (Re, Im): the keep / zero decision of every coefficient (test hook)
 *   stats    stats_host [P3D_STATS_PER_SLICE] of X0 = fftn(x), the layout of p3d_pocs_stats for ONE volume
 *   run      the loop.  x, out [n0][n1][n2] of `dtype` (P3D_C64 / P3D_F32); mask float32 [n1][n2], or [n0][n1][n2] with P3D_FLAG_MASK_PER_SLICE
 *            in params->flags; tau HOST [niter][2] doubles; niter_done HOST, one int32; sums HOST [niter + 1] doubles or NULL (sum |x_k|, 0 where
 *            not executed); elapsed_ms device time of the call or NULL.  hard / soft / garrote, every version, eps and alpha of p3d_pocs_params
 *            (P3D_FLAG_PRIMED is ignored; P3D_FLAG_PROFILE brackets every axis-0 pass with HIP events, read with p3d_vol_last_profile: mean device
 *            milliseconds of that kernel in the last run and its launches).  An all-zero volume comes back untouched with niter_done = 0.  A device `out` that
 *            overlaps `x` is written through a staging volume (every iteration reads x).
 * The *_dev entries take DEVICE pointers for x, mask and out, the others HOST pointers (staged through volumes the plan allocates on first use). */
typedef struct p3d_vol_plan p3d_vol_plan;
int p3d_vol_shape_supported(int n0, int n1, int n2);
int p3d_vol_plan_create(p3d_vol_plan** out, int device, int n0, int n1, int n2, p3d_plan* plan);
int p3d_vol_plan_destroy(p3d_vol_plan* vplan);
int p3d_vol_fft3_c64_dev(p3d_vol_plan* vplan, const void* in_dev, void* out_dev, int inverse);
int p3d_vol_fft3_c64(p3d_vol_plan* vplan, const void* in_host, void* out_host, int inverse);
int p3d_vol_shrink_c64(p3d_vol_plan* vplan, const void* in_host, const double* tau, int thresh_op, void* out_host);
int p3d_vol_last_profile(p3d_vol_plan* vplan, double* zpass_ms, int* zpass_launches);
int p3d_vol_stats_dev(p3d_vol_plan* vplan, const void* x_dev, int dtype, double* stats_host);
int p3d_vol_stats(p3d_vol_plan* vplan, const void* x_host, int dtype, double* stats_host);
int p3d_vol_run_dev(p3d_vol_plan* vplan, const void* x_dev, int dtype, const float* mask_dev, const double* tau, const p3d_pocs_params* params, void* out_dev,
                    int32_t* niter_done, double* sums, double* elapsed_ms);
int p3d_vol_run(p3d_vol_plan* vplan, const void* x_host, int dtype, const float* mask_host, const double* tau, const p3d_pocs_params* params, void* out_host,
                int32_t* niter_done, double* sums, double* elapsed_ms);

/* ---- 3-D FFT POCS in double precision (csrc/p3d_vol64.hip) -----------------------------------------------------------------------------------
 * The volume loop above in the reference's own precision (POCS.py:566-575, 616: complex128 / float64 throughout): a complex128 work volume, the line
 * passes of a p3d_plan64 for (n1, n2) slices, one axis-0 kernel on complex128 with NumPy's threshold semantics in double, a double mask, cost sums
 * folded in a fixed order (no atomics: results are bitwise repeatable).  Within 1e-10 of the float64 oracle on every seeded case, none set aside.
 *   shape_supported  1 when n0 is a 7-smooth length from 1 to 1024 and (n1, n2) is a slice shape p3d_plan64_create takes (extents up to 5120)
 *   create   `plan`: a p3d_plan64 for (n1, n2) slices on `device` to borrow (not owned: it must outlive the volume plan, which runs on its stream
 *            and is as little re-entrant), or NULL: the volume plan creates and owns one.  Allocates the complex128 work volume.
 *            P3D_ERR_UNSUPPORTED for any other n0 or slice shape
 *   fft3     np.fft.fftn (inverse = 0) / ifftn (inverse = 1) of one complex128 volume through the loop's own passes (test hook); in == out is allowed
 *   shrink   threshold(fftn(x), tau, thresh_op) of a complex128 volume, tau HOST [2] doubles (Re, Im) (test hook)
 *   stats    stats_host [P3D_STATS_PER_SLICE] of X0 = fftn(x), every reduction in double
 *   run      the loop.  x, out [n0][n1][n2] of `dtype`: P3D_C128, P3D_F64, or P3D_C64 / P3D_F32 (converted on load / store; real volumes run as complex
 *            with a zero imaginary part); mask DOUBLE [n1][n2], or [n0][n1][n2] with P3D_FLAG_MASK_PER_SLICE; tau, niter_done, sums, elapsed_ms, the
 *            operators (hard / soft / garrote), versions, eps, alpha, P3D_FLAG_PROFILE (read with last_profile), the all-zero volume and an `out` that
 *            overlaps `x` as in the float32 entries above.
 * The *_dev entries take DEVICE pointers for x, mask and out, the others HOST pointers (staged through volumes the plan allocates on first use). */
typedef struct p3d_vol64_plan p3d_vol64_plan;
int p3d_vol64_shape_supported(int n0, int n1, int n2);
int p3d_vol64_plan_create(p3d_vol64_plan** out, int device, int n0, int n1, int n2, p3d_plan64* plan);
int p3d_vol64_plan_destroy(p3d_vol64_plan* vplan);
int p3d_vol64_fft3_c128_dev(p3d_vol64_plan* vplan, const void* in_dev, void* out_dev, int inverse);
int p3d_vol64_fft3_c128(p3d_vol64_plan* vplan, const void* in_host, void* out_host, int inverse);
int p3d_vol64_shrink_c128(p3d_vol64_plan* vplan, const void* in_host, const double* tau, int thresh_op, void* out_host);
int p3d_vol64_last_profile(p3d_vol64_plan* vplan, double* zpass_ms, int* zpass_launches);
int p3d_vol64_stats_dev(p3d_vol64_plan* vplan, const void* x_dev, int dtype, double* stats_host);
int p3d_vol64_stats(p3d_vol64_plan* vplan, const void* x_host, int dtype, double* stats_host);
int p3d_vol64_run_dev(p3d_vol64_plan* vplan, const void* x_dev, int dtype, const double* mask_dev, const double* tau, const p3d_pocs_params* params, void* out_dev,
                      int32_t* niter_done, double* sums, double* elapsed_ms);
int p3d_vol64_run(p3d_vol64_plan* vplan, const void* x_host, int dtype, const double* mask_host, const double* tau, const p3d_pocs_params* params, void* out_host,
                  int32_t* niter_done, double* sums, double* elapsed_ms);

/* ---- 3-D DCT POCS: a whole volume as ONE job with the cosine transform (csrc/p3d_vol_dct.hip) ---------------------------------------------------
 * POCS_algorithm(x, mask, transform=partial(scipy.fft.dctn, norm=...), itransform=partial(scipy.fft.idctn, norm=...), transform_kind='DCT', ...) on a
 * volume x of (n0, n1, n2) points, C-contiguous, n2 fastest: the type-2 DCT over all three axes, one schedule, one cost, one iteration count and one
 * early exit for the volume.  norm: P3D_DCT_BACKWARD / P3D_DCT_ORTHO, the `norm` keyword of both callables.  Per iteration on a complex64 work volume in
 * the reordered sample order of the DCT along axes 1 and 2: the fft2 passes of a p3d_plan for (n1, n2) slices, the group pass of the 2-D DCT loop
 * (combine), one kernel that transforms a tile of plane positions along axis 0 -- the reordering of axis 0 folded into its loads and stores --, combines,
 * thresholds, splits and transforms back (the 3-D cosine spectrum never goes to memory), the group pass again (split), the ifft2 passes, and the
 * re-insertion with cost sums folded in a fixed order (results are bitwise repeatable).  float32 kernels: complex64 volumes, or float32 ones, which run as
 * complex with a zero imaginary part and return the real part.
 *   shape_supported  1 when n0 is a 7-smooth length from 1 to 1024 (n0 = 1: the axis-0 pass is its group step alone) and p3d_shape_supported(n1, n2)
 *   create   `plan`: a p3d_plan for (n1, n2) slices on `device` to borrow (not owned: it must outlive the volume plan, which runs on its stream
 *            and is as little re-entrant), or NULL: the volume plan creates and owns one.  Allocates the complex64 work volume and the DCT tables of all
 *            three axes for both norms.  P3D_ERR_UNSUPPORTED for any other n0 or slice shape
 *   dct3     scipy.fft.dctn (inverse = 0) / idctn (inverse = 1) of one complex64 volume through the loop's own passes (test hook); in == out is allowed
 *   shrink   threshold(dctn(x), tau, thresh_op), tau HOST [2] doubles (Re, Im): the keep / zero decision of every coefficient (test hook)
 *   stats    stats_host [P3D_STATS_PER_SLICE] of X0 = dctn(x), the layout of p3d_pocs_stats for ONE volume
 *   run      the loop, every argument as p3d_vol_run takes it (dtypes, the mask and P3D_FLAG_MASK_PER_SLICE, tau, niter_done, sums, elapsed_ms, hard / soft /
 *            garrote, versions, eps, alpha, P3D_FLAG_PROFILE read with p3d_voldct_last_profile, the all-zero volume, an `out` that overlaps `x`).
 * The *_dev entries take DEVICE pointers for x, mask and out, the others HOST pointers (staged through volumes the plan allocates on first use). */
typedef struct p3d_voldct_plan p3d_voldct_plan;
int p3d_voldct_shape_supported(int n0, int n1, int n2);
int p3d_voldct_plan_create(p3d_voldct_plan** out, int device, int n0, int n1, int n2, p3d_plan* plan);
int p3d_voldct_plan_destroy(p3d_voldct_plan* vplan);
int p3d_voldct_dct3_c64_dev(p3d_voldct_plan* vplan, const void* in_dev, void* out_dev, int norm, int inverse);
int p3d_voldct_dct3_c64(p3d_voldct_plan* vplan, const void* in_host, void* out_host, int norm, int inverse);
int p3d_voldct_shrink_c64(p3d_voldct_plan* vplan, const void* in_host, const double* tau, int thresh_op, int norm, void* out_host);
int p3d_voldct_last_profile(p3d_voldct_plan* vplan, double* zpass_ms, int* zpass_launches);
int p3d_voldct_stats_dev(p3d_voldct_plan* vplan, const void* x_dev, int dtype, int norm, double* stats_host);
int p3d_voldct_stats(p3d_voldct_plan* vplan, const void* x_host, int dtype, int norm, double* stats_host);
int p3d_voldct_run_dev(p3d_voldct_plan* vplan, const void* x_dev, int dtype, const float* mask_dev, const double* tau, const p3d_pocs_params* params, int norm,
                       void* out_dev, int32_t* niter_done, double* sums, double* elapsed_ms);
int p3d_voldct_run(p3d_voldct_plan* vplan, const void* x_host, int dtype, const float* mask_host, const double* tau, const p3d_pocs_params* params, int norm,
                   void* out_host, int32_t* niter_done, double* sums, double* elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* P3D_H */
