"""Plain NumPy restatement of step 2's device code (csrc/p3d_proj.hip): the Krueger series of the transverse Mercator projection to n^6, forward
and inverse, with the six-term sums written out term by term (twelve transcendental calls, no recurrence), and the window convolution.
prm = (a, f, lon0_deg, lat0_deg, k0, x0, y0) as in include/p3d.h."""
import numpy as np


def constants(a, f):
    n = f / (2 - f)
    A = a / (1 + n) * (1 + n**2 / 4 + n**4 / 64 + n**6 / 256)
    alpha = [n / 2 - 2 * n**2 / 3 + 5 * n**3 / 16 + 41 * n**4 / 180 - 127 * n**5 / 288 + 7891 * n**6 / 37800,
             13 * n**2 / 48 - 3 * n**3 / 5 + 557 * n**4 / 1440 + 281 * n**5 / 630 - 1983433 * n**6 / 1935360,
             61 * n**3 / 240 - 103 * n**4 / 140 + 15061 * n**5 / 26880 + 167603 * n**6 / 181440,
             49561 * n**4 / 161280 - 179 * n**5 / 168 + 6601661 * n**6 / 7257600,
             34729 * n**5 / 80640 - 3418889 * n**6 / 1995840,
             212378941 * n**6 / 319334400]
    beta = [n / 2 - 2 * n**2 / 3 + 37 * n**3 / 96 - n**4 / 360 - 81 * n**5 / 512 + 96199 * n**6 / 604800,
            n**2 / 48 + n**3 / 15 - 437 * n**4 / 1440 + 46 * n**5 / 105 - 1118711 * n**6 / 3870720,
            17 * n**3 / 480 - 37 * n**4 / 840 - 209 * n**5 / 4480 + 5569 * n**6 / 90720,
            4397 * n**4 / 161280 - 11 * n**5 / 504 - 830251 * n**6 / 7257600,
            4583 * n**5 / 161280 - 108847 * n**6 / 3991680,
            20648693 * n**6 / 638668800]
    return A, alpha, beta, np.sqrt(f * (2 - f))


def _taup(tau, e):
    sigma = np.sinh(e * np.arctanh(e * tau / np.sqrt(1 + tau * tau)))
    return tau * np.sqrt(1 + sigma * sigma) - sigma * np.sqrt(1 + tau * tau)


def _xi_eta(lat_deg, lam, alpha, e):
    taup = _taup(np.tan(np.radians(lat_deg)), e)
    xip = np.arctan2(taup, np.cos(lam))
    etap = np.arcsinh(np.sin(lam) / np.hypot(taup, np.cos(lam)))
    xi, eta = xip.copy(), etap.copy()
    for j, c in enumerate(alpha, 1):
        xi = xi + c * np.sin(2 * j * xip) * np.cosh(2 * j * etap)
        eta = eta + c * np.cos(2 * j * xip) * np.sinh(2 * j * etap)
    return xi, eta


def tm_forward(lon, lat, prm):
    a, f, lon0, lat0, k0, x0, y0 = (float(v) for v in prm)
    A, alpha, _, e = constants(a, f)
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    xi, eta = _xi_eta(lat, np.radians(lon - lon0), alpha, e)
    xi0 = _xi_eta(np.array(lat0), np.array(0.0), alpha, e)[0]
    return x0 + k0 * A * eta, y0 + k0 * A * (xi - xi0)


def tm_inverse(x, y, prm):
    a, f, lon0, lat0, k0, x0, y0 = (float(v) for v in prm)
    A, alpha, beta, e = constants(a, f)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    xi = (y - y0) / (k0 * A) + _xi_eta(np.array(lat0), np.array(0.0), alpha, e)[0]
    eta = (x - x0) / (k0 * A)
    xip, etap = xi.copy(), eta.copy()
    for j, c in enumerate(beta, 1):
        xip = xip - c * np.sin(2 * j * xi) * np.cosh(2 * j * eta)
        etap = etap - c * np.cos(2 * j * xi) * np.sinh(2 * j * eta)
    taup = np.sin(xip) / np.hypot(np.sinh(etap), np.cos(xip))
    lam = np.arctan2(np.sinh(etap), np.cos(xip))
    e2m = 1 - e * e
    tau = taup / e2m
    for _ in range(5):
        ti = _taup(tau, e)
        tau = tau + (taup - ti) / np.sqrt(1 + ti * ti) * (1 + e2m * tau * tau) / (e2m * np.sqrt(1 + tau * tau))
    return lon0 + np.degrees(lam), np.degrees(np.arctan(tau))


def tmerc(x, y, prm, inverse=False, device=0):
    """`_ffi.proj_tmerc` on the CPU."""
    return (tm_inverse if inverse else tm_forward)(x, y, prm)


def tmerc_dev_unavailable(*args, **kwargs):
    raise AssertionError('a device entry point was called in a host test')


def convolve_valid(padded, w, device=0):
    """`_ffi.proj_smooth` on the CPU: out[i] = sum_k padded[i + k] * w[len(w) - 1 - k], k ascending."""
    padded, w = np.asarray(padded, dtype=np.float64), np.asarray(w, dtype=np.float64)
    out = np.zeros(padded.size - w.size + 1)
    for k in range(w.size):
        out = out + padded[k:k + out.size] * w[w.size - 1 - k]
    return out
