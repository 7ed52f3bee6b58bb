// p3d_tide.hip -- step 6 of the workflow (the reference's tide_compensation_segy.py, which takes the prediction from tpxo-tide-prediction): the
// harmonic tide prediction along a track, in double precision.
//
//   tide_predict_kernel   one thread per point (lon, lat in degrees, t in seconds since 1992-01-01T00:00:00).
//                         1. the four bilinear weights of the enclosing cell of the subset grid; the weights of dry nodes are dropped and the rest
//                            renormalised, four dry corners give NaN;
//                         2. the lunar node N at t, sin / cos of N, 2 N and 3 N (one sincos, the multiples by the angle-sum formulas);
//                         3. the nodal factor f and phase u of the seven families the 14 constituents fall into (OTPS `nodal`), computed ONCE per point:
//                            mm, mf, q1, o1, k1, m2 (with n2, 2n2, ms4), k2; m4 and mn4 take f_m2^2 and 2 u_m2; p1 and s2 have f = 1, u = 0;
//                         4. the loop over the nc constituents of the call: the interpolated complex constant z_c (eight int32 loads), theta_c =
//                            omega_c t + phi0_c + u_c, one sincos, tide += f_c (Re z_c cos theta_c - Im z_c sin theta_c).
//
// The constituent ids of the call reach the kernel as 4-bit fields of one 64-bit argument, and the per-id constants (omega, phi0, family) are a
// __constant__ table: the id is the same for every lane, the table read is a scalar load, and the family selects among values already in
// registers by compares -- no array in private memory, so no scratch.  Every table index is clamped into the subset before it is used.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "p3d.h"
#include "p3d_host.hpp"

using p3d::DevBuf;
using p3d::fail;
using p3d::use_device;

namespace {

constexpr int TIDE_BS = 256;
constexpr int NCON = P3D_TIDE_CONSTITUENTS;
constexpr double DEG = 0.017453292519943295769;            // pi / 180
constexpr double EDGE = 1e-9;                              // cells: how far beyond the first / last node a point still counts as on it

enum Family { F_UNITY = 0, F_MM, F_MF, F_Q1, F_O1, F_K1, F_M2, F_K2, F_M2SQ };

// ids in the order m2, s2, n2, k2, k1, o1, p1, q1, m4, mf, 2n2, mm, mn4, ms4; angular frequency (rad / s) and phase at 1992-01-01 (rad): OTPS constit.h
__constant__ double OMEGA[NCON] = {1.405189e-4, 1.454441e-4, 1.378797e-4, 1.458423e-4, 7.292117e-5, 6.759774e-5, 7.252295e-5,
                                   6.495854e-5, 2.810377e-4, 0.053234e-4, 1.352405e-4, 0.026392e-4, 2.783984e-4, 2.859630e-4};
__constant__ double PHASE[NCON] = {1.731557546, 0.0,         6.050721243, 3.487600001, 0.173003674, 1.558553872, 6.110181633,
                                   5.877717569, 3.463115091, 1.756042456, 4.086699633, 1.964021610, 1.499093481, 1.731557546};
__constant__ int FAMILY[NCON] = {F_M2, F_UNITY, F_M2, F_K2, F_K1, F_O1, F_UNITY, F_Q1, F_M2SQ, F_MF, F_M2, F_MM, F_M2SQ, F_M2};

struct TideArgs {
    double lon0, dlon, lat0, dlat;       // the subset's axes: node (i, j) is at (lon0 + i dlon, lat0 + j dlat)
    int nxs, nys, nc;
    unsigned long long ids;              // constituent c of the call has id (ids >> 4 c) & 15
};

__global__ void __launch_bounds__(TIDE_BS) tide_predict_kernel(const double* __restrict__ lon, const double* __restrict__ lat, const double* __restrict__ t,
                                                               size_t n, const int* __restrict__ hre, const int* __restrict__ him,
                                                               const unsigned char* __restrict__ wet, TideArgs a, double* __restrict__ tide)
{
    const size_t i = (size_t)blockIdx.x * TIDE_BS + threadIdx.x;
    if (i >= n) return;
    const double nan = __builtin_nan("");
    const double ts = t[i];
    const double fx = (lon[i] - a.lon0) / a.dlon, fy = (lat[i] - a.lat0) / a.dlat;
    // a point outside the subset (or a non-finite one) has no cell: NaN, and no table is read
    if (!(fx >= -EDGE && fx <= (double)(a.nxs - 1) + EDGE && fy >= -EDGE && fy <= (double)(a.nys - 1) + EDGE) || !(fabs(ts) <= 1e300)) {
        tide[i] = nan;
        return;
    }
    // 1. the cell: the lower node clamped to 0 ... extent - 2, so a point on the last row / column has weights 0 / 1 in the last cell
    const int ix = min(max((int)floor(fx), 0), a.nxs - 2), iy = min(max((int)floor(fy), 0), a.nys - 2);
    const double wx = fmin(fmax(fx - (double)ix, 0.0), 1.0), wy = fmin(fmax(fy - (double)iy, 0.0), 1.0);
    const size_t c00 = (size_t)ix * (size_t)a.nys + (size_t)iy, c10 = c00 + (size_t)a.nys;      // (ix, iy), (ix + 1, iy); + 1: iy + 1
    double w00 = wet[c00] ? (1.0 - wx) * (1.0 - wy) : 0.0;
    double w01 = wet[c00 + 1] ? (1.0 - wx) * wy : 0.0;
    double w10 = wet[c10] ? wx * (1.0 - wy) : 0.0;
    double w11 = wet[c10 + 1] ? wx * wy : 0.0;
    const bool dry = !(wet[c00] | wet[c00 + 1] | wet[c10] | wet[c10 + 1]);
    const double wsum = ((w00 + w01) + w10) + w11;
    if (dry || !(wsum > 0.0)) {                                  // four dry corners, or every wet one has weight 0
        tide[i] = nan;
        return;
    }
    w00 /= wsum;
    w01 /= wsum;
    w10 /= wsum;
    w11 /= wsum;

    // 2. the lunar node
    const double T = ts / 86400.0 + 48622.0 - 51544.4993;
    const double N = fmod(125.0445 - 0.05295377 * T, 360.0) * DEG;
    double S1, C1;
    sincos(N, &S1, &C1);
    const double S2 = 2.0 * S1 * C1, C2 = C1 * C1 - S1 * S1;
    const double S3 = S2 * C1 + C2 * S1;

    // 3. f and u of the seven families
    const double f_mm = 1.0 - 0.130 * C1;
    const double f_mf = 1.043 + 0.414 * C1, u_mf = (-23.7 * S1 + 2.7 * S2 - 0.4 * S3) * DEG;
    const double q1r = 1.0 + 0.188 * C1, q1i = 0.188 * S1;
    const double f_q1 = sqrt(q1r * q1r + q1i * q1i), u_q1 = atan(0.189 * S1 / (1.0 + 0.189 * C1));
    const double o1r = 1.0 + 0.189 * C1 - 0.0058 * C2, o1i = 0.189 * S1 - 0.0058 * S2;
    const double f_o1 = sqrt(o1r * o1r + o1i * o1i), u_o1 = (10.8 * S1 - 1.3 * S2 + 0.2 * S3) * DEG;
    const double k1r = 1.0 + 0.1158 * C1 - 0.0029 * C2, k1i = 0.1554 * S1 - 0.0029 * S2;
    const double f_k1 = sqrt(k1r * k1r + k1i * k1i), u_k1 = atan(-k1i / k1r);
    const double m2r = 1.0 - 0.03731 * C1 + 0.00052 * C2, m2i = 0.03731 * S1 - 0.00052 * S2;
    const double f_m2 = sqrt(m2r * m2r + m2i * m2i), u_m2 = atan(-m2i / m2r);
    const double k2r = 1.0 + 0.2852 * C1 + 0.0324 * C2, k2i = 0.3108 * S1 + 0.0324 * S2;
    const double f_k2 = sqrt(k2r * k2r + k2i * k2i), u_k2 = atan(-k2i / k2r);

    // 4. the harmonic sum
    const size_t plane = (size_t)a.nxs * (size_t)a.nys;
    double sum = 0.0;
    for (int c = 0; c < a.nc; ++c) {
        const int id = (int)((a.ids >> (4 * c)) & 15ull);          // < NCON: checked on the host
        const int fam = FAMILY[id];
        double f = 1.0, u = 0.0;
        if (fam == F_MM) { f = f_mm; }
        else if (fam == F_MF) { f = f_mf; u = u_mf; }
        else if (fam == F_Q1) { f = f_q1; u = u_q1; }
        else if (fam == F_O1) { f = f_o1; u = u_o1; }
        else if (fam == F_K1) { f = f_k1; u = u_k1; }
        else if (fam == F_M2) { f = f_m2; u = u_m2; }
        else if (fam == F_K2) { f = f_k2; u = u_k2; }
        else if (fam == F_M2SQ) { f = f_m2 * f_m2; u = 2.0 * u_m2; }
        const int* re = hre + (size_t)c * plane;
        const int* im = him + (size_t)c * plane;
        const double zr = (((w00 * (double)re[c00] + w01 * (double)re[c00 + 1]) + w10 * (double)re[c10]) + w11 * (double)re[c10 + 1]) / 1000.0;
        const double zi = (((w00 * (double)im[c00] + w01 * (double)im[c00 + 1]) + w10 * (double)im[c10]) + w11 * (double)im[c10 + 1]) / 1000.0;
        double st, ct;
        sincos(OMEGA[id] * ts + PHASE[id] + u, &st, &ct);
        sum += f * (zr * ct - zi * st);
    }
    tide[i] = sum;
}

// grid = {lon0, dlon, lat0, dlat}, ids[nc] -> the kernel's arguments
int tide_args(const double* grid, const int* ids, int nc, int nxs, int nys, TideArgs& a)
{
    if (!grid || !ids) return fail(P3D_ERR_INVALID, "NULL grid numbers or constituent ids");
    if (nc < 1 || nc > NCON) return fail(P3D_ERR_INVALID, "%d constituents (1 ... %d)", nc, NCON);
    if (nxs < 2 || nys < 2) return fail(P3D_ERR_INVALID, "a subset of %d x %d nodes holds no cell", nxs, nys);
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(grid[k])) return fail(P3D_ERR_INVALID, "grid number %d is not finite", k);
    if (!(grid[1] > 0.0) || !(grid[3] > 0.0)) return fail(P3D_ERR_INVALID, "the grid spacing must be positive (dlon = %g, dlat = %g)", grid[1], grid[3]);
    a.lon0 = grid[0];
    a.dlon = grid[1];
    a.lat0 = grid[2];
    a.dlat = grid[3];
    a.nxs = nxs;
    a.nys = nys;
    a.nc = nc;
    a.ids = 0;
    for (int c = 0; c < nc; ++c) {
        if (ids[c] < 0 || ids[c] >= NCON) return fail(P3D_ERR_INVALID, "constituent id %d at position %d (0 ... %d)", ids[c], c, NCON - 1);
        a.ids |= (unsigned long long)ids[c] << (4 * c);
    }
    return P3D_OK;
}

int launch_tide(const double* lon, const double* lat, const double* t, size_t n, const int* hre, const int* him, const unsigned char* wet, const TideArgs& a,
                double* tide)
{
    const size_t blocks = (n + TIDE_BS - 1) / TIDE_BS;
    if (blocks > 0x7fffffffull) return fail(P3D_ERR_UNSUPPORTED, "%zu points are too many for one launch", n);
    tide_predict_kernel<<<(unsigned)blocks, TIDE_BS, 0, 0>>>(lon, lat, t, n, hre, him, wet, a, tide);
    P3D_TRY(hipGetLastError());
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_tide_predict_dev(int device, const double* lon_dev, const double* lat_dev, const double* t_dev, size_t n, const int* hre_dev, const int* him_dev,
                         const unsigned char* wet_dev, int nc, int nxs, int nys, const double* grid, const int* ids, double* tide_dev)
{
    TideArgs a;
    if (int rc = tide_args(grid, ids, nc, nxs, nys, a)) return rc;
    if (n == 0) return P3D_OK;
    if (!lon_dev || !lat_dev || !t_dev || !hre_dev || !him_dev || !wet_dev || !tide_dev) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (tide_dev == lon_dev || tide_dev == lat_dev || tide_dev == t_dev) return fail(P3D_ERR_INVALID, "the result needs a buffer of its own");
    if (int rc = use_device(device)) return rc;
    if (int rc = launch_tide(lon_dev, lat_dev, t_dev, n, hre_dev, him_dev, wet_dev, a, tide_dev)) return rc;
    P3D_TRY(hipDeviceSynchronize());
    return P3D_OK;
}

int p3d_tide_predict(int device, const double* lon, const double* lat, const double* t, size_t n, const int* hre, const int* him, const unsigned char* wet,
                     int nc, int nxs, int nys, const double* grid, const int* ids, double* tide)
{
    TideArgs a;
    if (int rc = tide_args(grid, ids, nc, nxs, nys, a)) return rc;
    if (n == 0) return P3D_OK;
    if (!lon || !lat || !t || !hre || !him || !wet || !tide) return fail(P3D_ERR_INVALID, "NULL buffer");
    if (n > SIZE_MAX / sizeof(double)) return fail(P3D_ERR_INVALID, "%zu points", n);
    if (int rc = use_device(device)) return rc;
    const size_t bytes = n * sizeof(double), nodes = (size_t)nxs * (size_t)nys, table = (size_t)nc * nodes * sizeof(int);
    DevBuf dlon, dlat, dt, dre, dim, dwet, dout;
    P3D_TRY(hipMalloc(&dlon.p, bytes));
    P3D_TRY(hipMalloc(&dlat.p, bytes));
    P3D_TRY(hipMalloc(&dt.p, bytes));
    P3D_TRY(hipMalloc(&dout.p, bytes));
    P3D_TRY(hipMalloc(&dre.p, table));
    P3D_TRY(hipMalloc(&dim.p, table));
    P3D_TRY(hipMalloc(&dwet.p, nodes));
    P3D_TRY(hipMemcpy(dlon.p, lon, bytes, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dlat.p, lat, bytes, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dt.p, t, bytes, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dre.p, hre, table, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dim.p, him, table, hipMemcpyHostToDevice));
    P3D_TRY(hipMemcpy(dwet.p, wet, nodes, hipMemcpyHostToDevice));
    if (int rc = launch_tide((const double*)dlon.p, (const double*)dlat.p, (const double*)dt.p, n, (const int*)dre.p, (const int*)dim.p,
                             (const unsigned char*)dwet.p, a, (double*)dout.p))
        return rc;
    P3D_TRY(hipMemcpy(tide, dout.p, bytes, hipMemcpyDeviceToHost));
    return P3D_OK;
}

}  // extern "C"
