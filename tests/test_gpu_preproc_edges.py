"""Step-11 trace kernels (csrc/p3d_preproc.hip) at the edges tests/golden/preproc.npz does not reach: more than one workgroup and a
partial last one, the gridDim.y stride, every ``sos_*_kernel<NS>`` instantiation and group count, every route of the time-axis FFT,
the resampling ratios of -dt / -fs, ties and non-finite values in the quantile.  Every reference is float64 SciPy / NumPy computed
here from the float32 input (tests/helpers/preproc_reference.py).

Bounds.  rtol 1e-6 elementwise, with no absolute term, for the float32 elementwise stages (the one gain chain with an AGC in it
adds 1e-6 of the largest reference value, as tests/test_gpu_preproc.py does for such chains) and 1e-5 (rel-L2 per trace) as the cap
everywhere are the project's; below the cap, the filter and spectral bounds are measured from the references: the kernel may be at
most 4 x (filter) or 8 x (spectral) as far from float64 as a float64 model with the kernel's documented float32 storage, or
scipy.fft's own complex64 transforms, are (the worst trace of the one against the worst trace of the other).  upfirdn accumulates in double and rounds once: its bound is the float32 spacing."""
import numpy as np
import pytest

from helpers import preproc_reference as R
from pseudo_3d_interpolation_amd import _ffi
from pseudo_3d_interpolation_amd.functions import signal as S

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
FILTER_MARGIN, SPECTRAL_MARGIN = 4, 8


def run(x, op, **kw):
    y, refs = _ffi.trace_ops(x, [op], **kw)
    return (y, refs[0]) if refs else (y, None)


def gain_op(nt, flags, curves=None, **prm):
    """('gain', prm, curves) from the flag names and parameters of include/p3d.h (curves: {name: [nt]})."""
    p = np.zeros(_ffi.GAIN_NPRM)
    p[_ffi.GAIN_PRM['flags']] = sum(_ffi.GAIN_FLAG[f] for f in flags)
    for k, v in prm.items():
        p[_ffi.GAIN_PRM[k]] = v
    c = None
    if curves:
        c = np.ones((4, nt))
        for k, v in curves.items():
            c[('tpow', 'epow', 'linear', 'pgc').index(k)] = v
    return ('gain', p, c)


def assert_elementwise(got, want, what, after_agc=False):
    """The existing bound of the float32 elementwise stages (tests/test_gpu_preproc.py): rtol 1e-6 and no absolute term, NaN where
    the reference has NaN -- qclip, balance, reduce and a gain chain without AGC.  ``after_agc``: the existing bound of a gain
    chain with an AGC in it, which adds 1e-6 of the largest finite reference value as an absolute term (test_gain there)."""
    assert got.dtype == np.float32 and got.shape == want.shape, what
    atol = 0.0
    if after_agc:
        fin = want[np.isfinite(want)]
        atol = 1e-6 * float(np.max(np.abs(fin))) if fin.size else 0.0
    with np.errstate(invalid='ignore'):
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.maximum(np.abs(want.astype(np.float64)), 1e-30)
    err = err[np.isfinite(want) & (want != 0)]
    print(f'{what}: worst relative error {float(err.max()) if err.size else 0.0:.2e}')
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=atol, equal_nan=True, err_msg=str(what))


def assert_within(got, want, yardstick, margin, what):
    """The error is the rel-L2 per trace against float64; the WORST trace of the kernel is compared with margin x the WORST trace of
    the yardstick (and with 1e-5), not trace by trace: one trace's yardstick error is one draw of a rounding error, on a line of 2,
    3 or 64 samples it can be zero or far below its usual size while the kernel's draw for that trace is not, so the ratio of two
    single traces says nothing about the kernel; the worst over the traces is the stable figure of both."""
    assert got.dtype == np.float32 and got.shape == want.shape, what
    err, floor = float(R.rel_l2(got, want).max()), float(R.rel_l2(yardstick, want).max())
    print(f'{what}: kernel {err:.2e}, yardstick {floor:.2e}, bound {margin} x = {margin * floor:.2e}')
    assert err <= margin * floor, (what, err, floor)
    assert err <= 1e-5, (what, err)
    return err


# ---- trace counts: one lane per trace, TPB = 256 ------------------------------------------------------------------------------------
NT0 = 64
TWT0 = np.arange(NT0) * 0.001
TPOW0 = R.tpow_curve(TWT0, 1.5)
SOS2, ZI2, PAD2 = R.design((3, 0.3, 'lowpass'))
SOS9, ZI9, PAD9 = R.design((17, 0.3, 'lowpass'))      # 9 sections: the grouped kernels (8 + 1); padlen 54 < 64


def _ref_filter(sos, pad):
    return lambda x: (R.sosfiltfilt(sos, x), R.sosfiltfilt_f32_storage(sos, x, pad, group=sos.shape[0] + 1), FILTER_MARGIN)


# name -> (operation, reference(x) -> (float64 reference, yardstick or None, margin)); a yardstick of None: the elementwise bound
TRACE_OPS = {
    'balance_rms': (('balance', 0), lambda x: (R.balance(x, 0), None, 0)),
    'balance_max': (('balance', 1), lambda x: (R.balance(x, 1), None, 0)),
    'reduce_rms': (('reduce', 2), lambda x: ((x, R.reference_amplitude(x, 2)), None, 0)),
    'gain_all_barriers': (gain_op(NT0, ('tpow', 'agc', 'qclip', 'norm_rms', 'scale'), {'tpow': TPOW0}, agc_win=11, agc_kind=_ffi.AGC_KIND['rms'],
                                  qclip=0.9, scale=3.0),
                          lambda x: (R.gain_stages(x, tpow=TPOW0, agc_win=11, qclip_q=0.9, norm_rms=True, scale=3.0), None, 0)),
    'filter_2': (('filter', SOS2, ZI2, PAD2), _ref_filter(SOS2, PAD2)),
    'filter_9': (('filter', SOS9, ZI9, PAD9), _ref_filter(SOS9, PAD9)),
    'upfirdn_2_3': (S.resample_poly_op(NT0, 2, 3, 'hann'), lambda x: (R.resample_poly(x, 2, 3), None, -1)),
    'resample_64_48': (S.resample_op(NT0, 48, 'hann'), lambda x: (R.resample(x, 48, 'hann'), R.resample_c64(x, 48, 'hann'), SPECTRAL_MARGIN)),
    'envelope': (S.envelope_op(NT0), lambda x: (R.envelope(x), R.envelope_c64(x), SPECTRAL_MARGIN)),
}


def _check(name, got, ref, x, what):
    want, yardstick, margin = ref(x)
    y, r = got
    if name.startswith(('balance', 'reduce')):
        assert_elementwise(y, want[0], what)
        assert_elementwise(r, want[1], (what, 'amplitudes'))
    elif margin == 0:
        assert_elementwise(y, want, what, after_agc=name == 'gain_all_barriers')
    elif margin < 0:
        assert y.shape == want.shape, what
        err = float(R.rel_l2(y, want).max())
        print(f'{what}: kernel {err:.2e}, bound {EPS32:.2e}')
        assert err <= EPS32, (what, err)
    else:
        assert_within(y, want, yardstick, margin, what)


def _same_bits(a, b, what, keep=None):
    for u, v in zip(a, b):
        if u is None:
            continue
        if keep is not None:
            u, v = u[..., keep], v[..., keep]
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32), err_msg=str(what))


@pytest.mark.parametrize('name', list(TRACE_OPS))
@pytest.mark.parametrize('ntr', [1, 255, 256, 257, 513])
def test_trace_counts(ntr, name):
    """One trace, a partial block, a full block, a block and one lane, two blocks and one lane: against the reference per trace;
    every trace bit for bit what it is when run alone (chunks of one trace); bit for bit the same with a last chunk of one trace;
    untouched by NaN in the neighbouring lanes."""
    op, ref = TRACE_OPS[name]
    x = R.traces(NT0, ntr, seed=ntr)
    if ntr > 2:
        x[:, 2] = 0.0                                   # an all-zero trace among the others
    whole = run(x, op)
    _check(name, whole, ref, x, (name, ntr))
    _same_bits(whole, run(x, op, chunk_traces=1), (name, ntr, 'every trace alone'))
    if ntr > 1:
        _same_bits(whole, run(x, op, chunk_traces=256 if ntr == 513 else ntr - 1), (name, ntr, 'a last chunk of one trace'))
        bad = x.copy()
        poisoned = np.arange(ntr) % 3 == 1
        bad[:, poisoned] = np.nan
        _same_bits(whole, run(bad, op), (name, ntr, 'NaN neighbours'), keep=~poisoned)


# ---- the gridDim.y stride: more rows than the 65535 blocks of grid2() ------------------------------------------------------------
@pytest.mark.parametrize('nt', [65535, 65536, 70001])
def test_more_rows_than_grid_y(nt):
    x = R.traces(nt, 3, seed=nt)
    twt = np.arange(nt) * 0.0001
    tpow, linear = R.tpow_curve(twt, 0.5), np.linspace(0.5, 2.0, nt)
    pgc = R.pgc_curve(nt, {0: 1.0, nt // 3: 2.5, nt - 1: 0.5})
    op = gain_op(nt, ('tpow', 'pclip', 'linear', 'pgc'), {'tpow': tpow, 'linear': linear, 'pgc': pgc}, pclip=1.0)
    assert_elementwise(run(x, op)[0], R.gain_stages(x, tpow=tpow, pclip=1.0, linear=linear, pgc=pgc), ('gain', nt))
    for kind in (0, 1):
        y, r = run(x, ('balance', kind))
        want = R.balance(x, kind)
        assert_elementwise(y, want[0], ('balance', kind, nt))
        assert_elementwise(r, want[1], ('balance amplitudes', kind, nt))
    for up, down in ((1, 2), (3, 2)):
        y = run(x, S.resample_poly_op(nt, up, down, 'hann'))[0]
        want = R.resample_poly(x, up, down)
        assert y.shape == want.shape
        err = float(R.rel_l2(y, want).max())
        print(f'resample_poly {up}/{down} nt={nt}: kernel {err:.2e}, bound {EPS32:.2e}')
        assert err <= EPS32, (up, down, nt, err)
    y = run(x, ('filter', SOS2, ZI2, PAD2))[0]
    assert_within(y, R.sosfiltfilt(SOS2, x), R.sosfiltfilt_f32_storage(SOS2, x, PAD2), FILTER_MARGIN, ('filter, 2 sections', nt))


# ---- every cascade length --------------------------------------------------------------------------------------------------------
# sections -> kernels: 1 ... 8 sos_fused_kernel<1 ... 8>; 9 sos_fwd / sos_bwd_kernel<8> + <1> (two groups); 16 <8> + <8>;
# 17 <8> + <8> + <1> (three groups)
@pytest.mark.parametrize('name,args,nsec', R.FILTER_DESIGNS, ids=[d[0] for d in R.FILTER_DESIGNS])
def test_filter_cascade(name, args, nsec):
    """The kernel against float64 sosfiltfilt, within 4 x the float64 model with no group boundary (``group`` above the section
    count; test_preproc_reference_host.py: that model is within 1e-7 of sosfiltfilt).  The model rounds to float32 between the
    forward and the backward pass and in the result.  Up to 8 sections that is the kernel's own storage (sos_fused_kernel).  For
    9, 16 and 17 sections it is not: the grouped kernels keep double from the first forward group to the last backward one and
    round the result only, so their own floor is lower than the model's, and the bound is the fused path's -- valid, not tight."""
    sos, zi, padlen = R.design(args)
    assert sos.shape[0] == nsec
    for nt in (padlen + 1, 1500):
        x = R.traces(nt, 5, seed=nsec)
        y = run(x, ('filter', sos, zi, padlen))[0]
        model = R.sosfiltfilt_f32_storage(sos, x, padlen, group=nsec + 1)
        assert_within(y, R.sosfiltfilt(sos, x), model, FILTER_MARGIN, (name, nt))
    with pytest.raises(_ffi.P3DError, match='greater than padlen'):
        run(np.zeros((padlen, 2), np.float32), ('filter', sos, zi, padlen))


def test_filter_work_buffer_size():
    """A caller's work buffer: [nt + 2 padlen][ntraces] floats carry a cascade of up to 8 sections; a longer one keeps the signal
    between its groups in double, and a buffer of floats is refused, not overrun."""
    nt, ntr = NT0, 8
    x = R.traces(nt, ntr, seed=3)
    dx, dout = _ffi.DeviceArray((nt, ntr), np.float32).upload(x), _ffi.DeviceArray((nt, ntr), np.float32)
    floats = _ffi.DeviceArray((nt + 2 * PAD9, ntr), np.float32)
    doubles = _ffi.DeviceArray((nt + 2 * PAD9, ntr), np.float64)

    def call(sos, zi, pad, work):
        _ffi.check(_ffi.lib().p3d_pre_sosfiltfilt_dev(0, dx.ptr, nt, ntr, sos.shape[0], _ffi._ptr(np.ascontiguousarray(sos)),
                                                      _ffi._ptr(np.ascontiguousarray(zi)), pad, dout.ptr, work.ptr))
        return dout.download()

    try:
        np.testing.assert_array_equal(call(SOS2, ZI2, PAD2, floats), run(x, ('filter', SOS2, ZI2, PAD2))[0])
        with pytest.raises(_ffi.P3DError, match='work buffer too small'):
            call(SOS9, ZI9, PAD9, floats)
        np.testing.assert_array_equal(call(SOS9, ZI9, PAD9, doubles), run(x, ('filter', SOS9, ZI9, PAD9))[0])
    finally:
        for a in (dx, dout, floats, doubles):
            a.free()


# ---- upfirdn: the ratios of -dt / -fs resampling ---------------------------------------------------------------------------------
@pytest.mark.parametrize('up,down', [(2, 3), (3, 2), (5, 8), (8, 5), (4, 5), (7, 1), (1, 7), (1, 1)])
def test_upfirdn_ratios(up, down):
    for window in ('hann', 'blackman'):
        for nt in (1, 2, 21, 1000, 1001):
            x = R.traces(nt, 3, seed=nt + up)
            want = R.resample_poly(x, up, down, window)
            y = run(x, S.resample_poly_op(nt, up, down, window))[0]
            assert y.dtype == np.float32 and y.shape == want.shape, (up, down, window, nt, y.shape, want.shape)
            err = float(R.rel_l2(y, want).max())
            print(f'resample_poly {up}/{down} {window} nt={nt}: kernel {err:.2e}, bound {EPS32:.2e}')
            assert err <= EPS32, (up, down, window, nt, err)


# ---- the routes of the time-axis FFT (find_ops / flex_factors / pick_col_tile / axis0_fft_impl) --------------------------------------
ROUTES = [
    (256, 'tuned power of two'), (1024, 'tuned power of two'), (4096, 'tuned power of two'),
    (1000, 'register engine (2, 5)'), (1500, 'register engine (2, 3, 5)'), (2401, 'register engine (7^4)'),
    (3000, 'register engine (2, 3, 5)'), (1001, 'register engine (7 x 11 x 13)'), (1331, 'register engine (11^3)'),
    (100, 'LDS-image passes, 8 columns per workgroup'), (3125, 'LDS-image passes, 2 columns per workgroup'),
    (5000, 'LDS-image passes, 1 column per workgroup'), (5120, 'LDS-image passes, 1 column per workgroup'),
    (1700, 'LDS-image passes, direct prime 17'), (1150, 'LDS-image passes, direct prime 23'),
    (5100, 'LDS-image passes, direct prime 17, 1 column per workgroup'),
    (1009, 'chirp-z on 2048'), (2003, 'chirp-z on 4096'), (2001, 'chirp-z on 4096 (3 x 23 x 29)'),
    (4001, 'LDS-image passes, one direct pass of the prime 4001 (chirp-z would need 8192)'),
    (8192, 'workgroup-per-line fallback, 128 KiB of LDS'), (10240, 'workgroup-per-line fallback, 160 KiB of LDS'),
]


def route_class(route):
    for key in ('tuned', 'register engine', 'fallback', 'one direct pass', 'direct prime', 'chirp-z'):
        if key in route:
            return key
    return 'LDS-image'


@pytest.mark.parametrize('nt,route', ROUTES, ids=[f'{n}-{route_class(r).replace(" ", "_")}' for n, r in ROUTES])
def test_envelope_routes(nt, route):
    counts = (1, 7, 8, 9, 257) if nt <= 4096 else (3,)
    x = R.traces(nt, max(counts), seed=nt)
    want, yardstick = R.envelope(x), R.envelope_c64(x)
    worst = 0.0
    for ntr in counts:
        y = run(x[:, :ntr], S.envelope_op(nt))[0]
        worst = max(worst, assert_within(y, want[:, :ntr], yardstick[:, :ntr], SPECTRAL_MARGIN, ('envelope', nt, ntr, route)))
    print(f'ROUTE {route_class(route)} | envelope {nt}: worst {worst:.2e}')


@pytest.mark.parametrize('nt,num', [(2001, 1000), (1500, 4001), (4001, 4096), (1024, 1000), (1000, 1000), (10240, 5120), (3, 2), (2, 3)])
def test_resample_lengths(nt, num):
    x = R.traces(nt, 3 if nt > 3 else 64, seed=nt + num)       # the 2- and 3-point transforms: 64 traces for a yardstick that means something
    for window in (None, 'hann'):
        y = run(x, S.resample_op(nt, num, window))[0]
        want = R.resample(x, num, window)
        err = assert_within(y, want, R.resample_c64(x, num, window), SPECTRAL_MARGIN, ('resample', nt, num, window))
        print(f'ROUTE resample {nt} -> {num} {window}: worst {err:.2e}')


def test_fft_length_limit():
    """10240 runs (test_envelope_routes, test_resample_lengths); one more sample, in or out, is refused before any launch."""
    x = np.ones((10241, 2), np.float32)
    with pytest.raises(_ffi.UnsupportedError):
        run(x, S.envelope_op(10241))
    with pytest.raises(_ffi.UnsupportedError):
        run(x, S.resample_op(10241, 5000))
    with pytest.raises(_ffi.UnsupportedError):
        run(x[:10240], S.resample_op(10240, 10241))
    assert run(x[:10240], S.resample_op(10240, 10240))[0].shape == (10240, 2)


# ---- quantile clipping -------------------------------------------------------------------------------------------------------------
def _quantile_traces(nt):
    rng = np.random.default_rng(nt)
    cols = [rng.integers(-2, 3, nt).astype(np.float32),             # many ties, zeros among them
            np.zeros(nt, np.float32),                               # all zero
            np.full(nt, -1.5, np.float32),                          # constant
            rng.standard_normal(nt).astype(np.float32),             # ordinary
            rng.standard_normal(nt).astype(np.float32),             # ... with a NaN
            rng.standard_normal(nt).astype(np.float32),             # ordinary, between the two
            rng.standard_normal(nt).astype(np.float32),             # ... with +Inf
            np.round(rng.standard_normal(nt) * 2).astype(np.float32) / 2]
    x = np.stack(cols, axis=1)
    x[nt // 2, 4] = np.nan
    x[nt // 3, 6] = np.inf
    return np.ascontiguousarray(x)


@pytest.mark.parametrize('nt', [7, 200, 201])
def test_quantile_ties_and_non_finite(nt):
    x = _quantile_traces(nt)
    k = (nt - 1) // 2
    qs = [0.0, 0.25, 0.5, 0.75, 1.0, (k + 0.499) / (nt - 1), (k + 0.501) / (nt - 1)]     # q (n - 1) = k + 0.499 / k + 0.501
    finite = [0, 1, 2, 3, 5, 7]
    for q in qs:
        got = run(x, gain_op(nt, ('qclip',), qclip=q))[0]
        with np.errstate(invalid='ignore'):
            want = R.qclip(x, q)
        assert_elementwise(got, want, ('qclip', nt, q))
        # the trace with a NaN has a NaN quantile, and a comparison with NaN clips nothing (np.where in the reference): the
        # trace comes back as it went in, NaN included; the traces next to it are what they are without it
        np.testing.assert_array_equal(got[:, 4].view(np.uint32), x[:, 4].view(np.uint32))
        alone = run(np.ascontiguousarray(x[:, finite]), gain_op(nt, ('qclip',), qclip=q))[0]
        np.testing.assert_array_equal(got[:, finite], alone)
        assert np.isfinite(got[:, finite]).all()
    # with norm_rms after the qclip the NaN sample reaches the rms, and the whole trace is NaN, as in NumPy
    got = run(x, gain_op(nt, ('qclip', 'norm_rms'), qclip=0.5))[0]
    with np.errstate(invalid='ignore'):
        want = R.gain_stages(x, qclip_q=0.5, norm_rms=True)
    assert np.isnan(got[:, 4]).all() and np.isnan(want[:, 4]).all()
    assert_elementwise(got, want, ('qclip + norm_rms', nt))


# ---- reduce and balance on degenerate traces -------------------------------------------------------------------------------------
@pytest.mark.parametrize('nt', [1, 33])
def test_reduce_and_balance_like_numpy(nt):
    rng = np.random.default_rng(nt)
    x = rng.standard_normal((nt, 6)).astype(np.float32)
    x[:, 1] = 0.0
    x[nt // 2, 2] = np.nan
    x[nt // 2, 4] = np.inf
    x[0, 5] = -np.inf
    for kind in (0, 1):
        y, r = run(x, ('balance', kind))
        with np.errstate(invalid='ignore', over='ignore'):
            want_y, want_r = R.balance(x, kind)
        assert r[1] == 1.0 and np.array_equal(y[:, 1], x[:, 1])                # all zero: amplitude 1, the trace unchanged
        assert np.isnan(r[2]) and np.isnan(y[:, 2]).all()                      # NaN: NaN throughout
        assert np.isposinf(r[4]) and np.isposinf(r[5])                         # Inf: amplitude Inf, x / Inf = 0, Inf / Inf = NaN
        assert_elementwise(r, want_r, ('amplitudes', kind, nt))
        assert_elementwise(y, want_y, ('balance', kind, nt))
        _, r0 = run(x, ('reduce', kind))
        np.testing.assert_array_equal(r0.view(np.uint32), r.view(np.uint32))
    _, plain = run(x, ('reduce', 2))
    with np.errstate(invalid='ignore', over='ignore'):
        assert_elementwise(plain, R.reference_amplitude(x, 2), ('plain rms', nt))
    assert plain[1] == 0.0                                                     # kind 2: no 0 -> 1 guard
