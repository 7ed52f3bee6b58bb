// p3d_proj.hip -- step 2 of the workflow (the reference's reproject_segy.py): the transverse Mercator projection between geographic and projected
// coordinates in double precision, and the convolution half of the reference's coordinate smoothing (functions/filter.py:smooth).
//
// The projection is the Krueger series in the third flattening n = f / (2 - f) to n^6 (Karney, "Transverse Mercator with an accuracy of a few
// nanometers", J. Geodesy 85, 2011, eqs. 7-11, 35, 36): rectifying radius A, forward coefficients alpha_1..6, inverse coefficients beta_1..6.  They
// are computed once per call on the host and reach the kernel by value in its arguments (TmArgs, scalar registers): no table in global memory.
//
//   tmerc_fwd_kernel   one thread per point (lon, lat in degrees) -> (E, N).  tau = tan(lat), tau' = the tangent of the conformal latitude,
//                      xi' = atan2(tau', cos lam), eta' = asinh(sin lam / hypot(tau', cos lam)).  The six-term sums are ONE complex Clenshaw
//                      recurrence in sin / cos 2 xi', sinh / cosh 2 eta', and these four come from tau', cos lam and sin lam by the double-angle
//                      formulas: no transcendental call for them.  Per point: tan, sincos(lam), atanh, sinh, atan2, asinh.
//                      lam = 0 gives E = x0 exactly and lat = 0 gives N = y0 - k0 A xi0 + k0 A xi0 exactly (every term of the sums is a product with
//                      an exact zero; the unit is compiled without contraction into fused multiply-adds).
//   tmerc_inv_kernel   (E, N) -> (lon, lat) in degrees: sincos(2 xi), sinh(2 eta) (cosh from it), the same recurrence with beta, sincos(xi'),
//                      sinh(eta'), atan2, then tau from tau' by Newton's iteration with a FIXED count of 5 steps (no data-dependent exit; three reach
//                      double precision), each with one atanh and one sinh, and atan.
//   proj_smooth_kernel out[i] = sum_k padded[i + k] * w[wlen - 1 - k], k ascending, a multiply and an add per term (np.convolve(..., 'valid')).
//
// Both projection kernels read index i and then write index i only, so the outputs may be the inputs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "p3d.h"
#include "p3d_host.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

constexpr int PROJ_BS = 256;
constexpr double DEG = 0.017453292519943295769;            // pi / 180
constexpr double RAD = 57.295779513082320877;              // 180 / pi

// what a kernel needs of one projection, passed by value: A, alpha_1..6, beta_1..6, e (the 14 series constants) and the five placements
struct TmArgs {
    double A;                // rectifying radius a / (1 + n) (1 + n^2 / 4 + n^4 / 64 + n^6 / 256)
    double alpha[6];
    double beta[6];
    double e;                // first eccentricity
    double lon0;             // degrees
    double kA;               // k0 * A
    double x0, y0;
    double xi0;              // xi at (lat0, lam = 0)
};

// sum_j c[j - 1] sin(2 j (x + i y)) by Clenshaw's recurrence, from s2 = sin 2x, c2 = cos 2x, sh2 = sinh 2y, ch2 = cosh 2y
__host__ __device__ inline void clenshaw_sin(const double (&c)[6], double s2, double c2, double sh2, double ch2, double& re, double& im)
{
    const double r = 2.0 * c2 * ch2, i = -2.0 * s2 * sh2;   // 2 cos(2 z)
    double hr1 = 0.0, hi1 = 0.0, hr2 = 0.0, hi2 = 0.0;
#pragma unroll
    for (int j = 5; j >= 0; --j) {
        const double hr = c[j] + (r * hr1 - i * hi1) - hr2;
        const double hi = (r * hi1 + i * hr1) - hi2;
        hr2 = hr1;
        hi2 = hi1;
        hr1 = hr;
        hi1 = hi;
    }
    const double sr = s2 * ch2, si = c2 * sh2;              // sin(2 z)
    re = sr * hr1 - si * hi1;
    im = sr * hi1 + si * hr1;
}

// tau' (tangent of the conformal latitude) of tau (tangent of the geographic latitude)
__host__ __device__ inline double taup_of(double tau, double e)
{
    const double t1 = sqrt(1.0 + tau * tau);
    const double sigma = sinh(e * atanh(e * tau / t1));
    return tau * sqrt(1.0 + sigma * sigma) - sigma * t1;
}

__global__ void __launch_bounds__(PROJ_BS) tmerc_fwd_kernel(const double* __restrict__ lon, const double* __restrict__ lat, size_t n, TmArgs p,
                                                            double* ox, double* oy)
{
    const size_t i = (size_t)blockIdx.x * PROJ_BS + threadIdx.x;
    if (i >= n) return;
    const double lam = (lon[i] - p.lon0) * DEG;
    const double tau = tan(lat[i] * DEG);
    const double taup = taup_of(tau, p.e);
    double sl, cl;
    sincos(lam, &sl, &cl);
    const double h2 = taup * taup + cl * cl, h = sqrt(h2);
    const double xip = atan2(taup, cl);
    const double shp = sl / h;                               // sinh eta'
    const double etap = asinh(shp);
    const double chp = sqrt(1.0 + shp * shp);
    double dxi, deta;
    clenshaw_sin(p.alpha, 2.0 * taup * cl / h2, (cl * cl - taup * taup) / h2, 2.0 * shp * chp, 1.0 + 2.0 * shp * shp, dxi, deta);
    ox[i] = p.x0 + p.kA * (etap + deta);
    oy[i] = p.y0 + p.kA * ((xip + dxi) - p.xi0);
}

__global__ void __launch_bounds__(PROJ_BS) tmerc_inv_kernel(const double* __restrict__ x, const double* __restrict__ y, size_t n, TmArgs p,
                                                            double* olon, double* olat)
{
    const size_t i = (size_t)blockIdx.x * PROJ_BS + threadIdx.x;
    if (i >= n) return;
    const double xi = (y[i] - p.y0) / p.kA + p.xi0;
    const double eta = (x[i] - p.x0) / p.kA;
    double s2, c2;
    sincos(2.0 * xi, &s2, &c2);
    const double sh2 = sinh(2.0 * eta), ch2 = sqrt(1.0 + sh2 * sh2);
    double dxi, deta;
    clenshaw_sin(p.beta, s2, c2, sh2, ch2, dxi, deta);
    const double xip = xi - dxi, etap = eta - deta;
    double sx, cx;
    sincos(xip, &sx, &cx);
    const double shp = sinh(etap);
    const double taup = sx / sqrt(shp * shp + cx * cx);
    const double lam = atan2(shp, cx);
    const double e2m = 1.0 - p.e * p.e;
    double tau = taup / e2m;
#pragma unroll 1
    for (int it = 0; it < 5; ++it) {
        const double ti = taup_of(tau, p.e);
        tau += (taup - ti) / sqrt(1.0 + ti * ti) * (1.0 + e2m * tau * tau) / (e2m * sqrt(1.0 + tau * tau));
    }
    olon[i] = p.lon0 + lam * RAD;
    olat[i] = atan(tau) * RAD;
}

__global__ void __launch_bounds__(PROJ_BS) proj_smooth_kernel(const double* __restrict__ padded, size_t n, const double* __restrict__ w, int wlen,
                                                              double* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * PROJ_BS + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int k = 0; k < wlen; ++k) acc += padded[i + k] * w[wlen - 1 - k];
    out[i] = acc;
}

// prm = {a, f, lon0_deg, lat0_deg, k0, x0, y0} -> the kernel arguments
int tm_args(const double* prm, TmArgs& t)
{
    if (!prm) return fail(P3D_ERR_INVALID, "NULL projection parameters");
    const double a = prm[0], f = prm[1], lon0 = prm[2], lat0 = prm[3], k0 = prm[4], x0 = prm[5], y0 = prm[6];
    for (int k = 0; k < 7; ++k)
        if (!std::isfinite(prm[k])) return fail(P3D_ERR_INVALID, "projection parameter %d is not finite", k);
    if (!(a > 0.0) || !(f >= 0.0 && f < 1.0) || !(k0 > 0.0)) return fail(P3D_ERR_INVALID, "bad ellipsoid or scale (a = %g, f = %g, k0 = %g)", a, f, k0);
    if (std::fabs(lat0) > 90.0 || std::fabs(lon0) > 360.0) return fail(P3D_ERR_INVALID, "bad origin (lon0 = %g, lat0 = %g degrees)", lon0, lat0);
    const double n = f / (2.0 - f), n2 = n * n, n3 = n2 * n, n4 = n2 * n2, n5 = n4 * n, n6 = n3 * n3;
    t.A = a / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0 + n6 / 256.0);
    t.alpha[0] = n / 2.0 - 2.0 * n2 / 3.0 + 5.0 * n3 / 16.0 + 41.0 * n4 / 180.0 - 127.0 * n5 / 288.0 + 7891.0 * n6 / 37800.0;
    t.alpha[1] = 13.0 * n2 / 48.0 - 3.0 * n3 / 5.0 + 557.0 * n4 / 1440.0 + 281.0 * n5 / 630.0 - 1983433.0 * n6 / 1935360.0;
    t.alpha[2] = 61.0 * n3 / 240.0 - 103.0 * n4 / 140.0 + 15061.0 * n5 / 26880.0 + 167603.0 * n6 / 181440.0;
    t.alpha[3] = 49561.0 * n4 / 161280.0 - 179.0 * n5 / 168.0 + 6601661.0 * n6 / 7257600.0;
    t.alpha[4] = 34729.0 * n5 / 80640.0 - 3418889.0 * n6 / 1995840.0;
    t.alpha[5] = 212378941.0 * n6 / 319334400.0;
    t.beta[0] = n / 2.0 - 2.0 * n2 / 3.0 + 37.0 * n3 / 96.0 - n4 / 360.0 - 81.0 * n5 / 512.0 + 96199.0 * n6 / 604800.0;
    t.beta[1] = n2 / 48.0 + n3 / 15.0 - 437.0 * n4 / 1440.0 + 46.0 * n5 / 105.0 - 1118711.0 * n6 / 3870720.0;
    t.beta[2] = 17.0 * n3 / 480.0 - 37.0 * n4 / 840.0 - 209.0 * n5 / 4480.0 + 5569.0 * n6 / 90720.0;
    t.beta[3] = 4397.0 * n4 / 161280.0 - 11.0 * n5 / 504.0 - 830251.0 * n6 / 7257600.0;
    t.beta[4] = 4583.0 * n5 / 161280.0 - 108847.0 * n6 / 3991680.0;
    t.beta[5] = 20648693.0 * n6 / 638668800.0;
    t.e = std::sqrt(f * (2.0 - f));
    t.lon0 = lon0;
    t.kA = k0 * t.A;
    t.x0 = x0;
    t.y0 = y0;
    t.xi0 = 0.0;
    if (lat0 != 0.0) {                                         // xi at (lat0, lam = 0): eta' = 0, so the sums are plain sine series
        const double xip = std::atan(taup_of(std::tan(lat0 * DEG), t.e));
        double dxi, deta;
        clenshaw_sin(t.alpha, std::sin(2.0 * xip), std::cos(2.0 * xip), 0.0, 1.0, dxi, deta);
        t.xi0 = xip + dxi;
    }
    return P3D_OK;
}

int launch_tmerc(const double* x, const double* y, size_t n, const TmArgs& t, int inverse, double* ox, double* oy)
{
    const size_t blocks = (n + PROJ_BS - 1) / PROJ_BS;
    if (blocks > 0x7fffffffull) return fail(P3D_ERR_UNSUPPORTED, "%zu points are too many for one launch", n);
    if (inverse) {
        tmerc_inv_kernel<<<(unsigned)blocks, PROJ_BS, 0, 0>>>(x, y, n, t, ox, oy);
    } else {
        tmerc_fwd_kernel<<<(unsigned)blocks, PROJ_BS, 0, 0>>>(x, y, n, t, ox, oy);
    }
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_proj_tmerc_dev(int device, const double* x_dev, const double* y_dev, size_t n, const double* prm, int inverse, double* ox_dev, double* oy_dev)
{
    TmArgs t;
    if (int rc = tm_args(prm, t)) return rc;
    if (n == 0) return P3D_OK;
    if (!x_dev || !y_dev || !ox_dev || !oy_dev) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (ox_dev == oy_dev || ox_dev == y_dev || oy_dev == x_dev) return fail(P3D_ERR_INVALID, "an output may only be the input of the same coordinate");
    if (int rc = use_device(device)) return rc;
    if (int rc = launch_tmerc(x_dev, y_dev, n, t, inverse, ox_dev, oy_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_proj_tmerc(int device, const double* x, const double* y, size_t n, const double* prm, int inverse, double* ox, double* oy)
{
    TmArgs t;
    if (int rc = tm_args(prm, t)) return rc;
    if (n == 0) return P3D_OK;
    if (!x || !y || !ox || !oy) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (n > SIZE_MAX / sizeof(double)) return fail(P3D_ERR_INVALID, "%zu points", n);
    if (int rc = use_device(device)) return rc;
    const size_t bytes = n * sizeof(double);
    DevBuf dx, dy;
    P3D_TRY(hipMalloc(&dx.p, bytes));
    P3D_TRY(hipMalloc(&dy.p, bytes));
    P3D_TRY(hipMemcpy(dx.p, x, bytes, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dy.p, y, bytes, hipMemcpyHostToDevice));
    if (int rc = launch_tmerc((const double*)dx.p, (const double*)dy.p, n, t, inverse, (double*)dx.p, (double*)dy.p)) return rc;   // in place
    P3D_TRY(hipMemcpy(ox, dx.p, bytes, hipMemcpyDeviceToHost));
    P3D_TRY(hipMemcpy(oy, dy.p, bytes, hipMemcpyDeviceToHost));
    return P3D_OK;
}

int p3d_proj_smooth_dev(int device, const double* padded_dev, size_t n, const double* w, int wlen, double* out_dev)
{
    if (wlen < 1) return fail(P3D_ERR_INVALID, "a window of %d samples", wlen);
    if (n == 0) return P3D_OK;
    if (!padded_dev || !w || !out_dev) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (padded_dev == out_dev) return fail(P3D_ERR_INVALID, "the smoothing needs separate input and output buffers");
    const size_t blocks = (n + PROJ_BS - 1) / PROJ_BS;
    if (blocks > 0x7fffffffull) return fail(P3D_ERR_UNSUPPORTED, "%zu samples are too many for one launch", n);
    if (int rc = use_device(device)) return rc;
    DevBuf dw;
    P3D_TRY(hipMalloc(&dw.p, (size_t)wlen * sizeof(double)));
    P3D_TRY(hipMemcpy(dw.p, w, (size_t)wlen * sizeof(double), hipMemcpyHostToDevice));
    proj_smooth_kernel<<<(unsigned)blocks, PROJ_BS, 0, 0>>>(padded_dev, n, (const double*)dw.p, wlen, out_dev);
    P3D_TRY(hipGetLastError());
    P3D_TRY(hipDeviceSynchronize());                               // dw is freed on return
    return P3D_OK;
}

}  // extern "C"
