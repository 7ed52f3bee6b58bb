#!/opt/conda/bin/python3.9
"""Golden vectors for step 11 (cube pre-processing), produced by the REFERENCE's own functions and scipy.signal.

Run in the build container only (the reference does not travel):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_preproc.py

Recorded in ``preproc.npz`` (data only, no source text):

  * filter designs: ``buttord`` N / Wn, ``butter(..., output='sos')``, ``sosfilt_zi`` and sosfiltfilt's pad length for the
    reference's bandpass (scipy's band-stop branch), lowpass and highpass specifications (``FILTER_CASES``), one of them of high
    order; the outputs of the reference's ``filter_frequency`` on (4, nt) traces for an even, an odd and a just-above-padlen nt;
  * error messages: unsorted / inverted corner frequencies and nt <= padlen;
  * ``gain(...)`` for every parameter alone and a combined set on (3, 4, nt) data (time on the last axis), with twt in seconds
    (starting at 0) and in samples; ``qclip`` and ``norm_rms`` on 1-D traces;
  * ``calc_reference_amplitude`` (rms, max) with an all-zero trace;
  * ``resample_poly`` for (up, down) in {(1,2), (2,1), (1,3), (3,1)} x {hann, hamming, blackman}; ``resample`` to shorter and longer
    lengths, odd and even, window hann;
  * ``envelope`` for an even and an odd nt;
  * ``get_resampled_twt`` and ``ffloat`` cases;
  * the step-11 chain of the command line ``--balance rms --gain tpow=2 agc=1 --filter bandpass --filter_freqs 50 100 800 1000
    -f 2 --envelope`` composed from the reference's functions in its order (cube_preprocessing_3D.py:170-360) on a (256, 5, 6)
    (twt, iline, xline) cube sampled at 0.2 ms, float32 between the steps (the float32 output of this package).
"""
import json
import os
import warnings

import numpy as np
import scipy.signal as ss

from pseudo_3D_interpolation.functions.filter import bandpass_filter, filter_frequency
from pseudo_3D_interpolation.functions.signal import calc_reference_amplitude, envelope, gain, get_resampled_twt
from pseudo_3D_interpolation.functions.utils import ffloat

warnings.filterwarnings('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
FILTER_CASES = [
    ('bandpass', [100, 200, 2000, 3000], 10000.0),
    ('bandpass', [5, 10, 60, 80], 500.0),
    ('lowpass', [1000, 2000], 10000.0),
    ('highpass', [2000, 1000], 10000.0),
    ('lowpass', [200, 215], 1000.0),       # order 19: 10 sections (two groups on the GPU)
]
GAIN_CASES = [
    dict(tpow=2.0), dict(tpow=-1.0), dict(epow=1.5), dict(epow=0.8, etpow=1.3), dict(epow=0.5, ebase=10.0), dict(gpow=0.5),
    dict(agc=True, agc_win=0.01), dict(agc=True, agc_win=0.02, agc_kind='mean'), dict(clip=1.2), dict(pclip=0.9), dict(nclip=-0.7),
    dict(linear=(1, 3)), dict(pgc={0.01: 1.0, 0.05: 3.0, 0.1: 0.5}), dict(bias=0.25), dict(scale=2.5), dict(scale=4.0, norm=True),
    dict(tpow=2.0, gpow=0.5, clip=1.5, linear=(1, 2), scale=3.0, bias=0.1),
]


def main():
    rng = np.random.default_rng(11)
    out, meta = {}, {}
    # ---- filters
    for i, (ft, freqs, fs) in enumerate(FILTER_CASES):
        wp, ws = ([freqs[0], freqs[-1]], [freqs[1], freqs[2]]) if ft == 'bandpass' else freqs
        N, Wn = ss.buttord(wp, ws, 1, 10, analog=False, fs=fs)
        sos = ss.butter(N, Wn, analog=False, btype=ft, output='sos', fs=fs)
        ntaps = 2 * sos.shape[0] + 1 - min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())
        padlen = 3 * int(ntaps)
        out[f'f{i}/N'] = np.array(N)
        out[f'f{i}/Wn'] = np.atleast_1d(Wn)
        out[f'f{i}/sos'] = sos
        out[f'f{i}/zi'] = ss.sosfilt_zi(sos)
        out[f'f{i}/padlen'] = np.array(padlen)
        for nt in (200, 201, padlen + 1):
            x = rng.standard_normal((4, nt)).astype(np.float32)
            out[f'f{i}/x{nt}'] = x
            out[f'f{i}/y{nt}'] = filter_frequency(x, freqs, fs, ft, axis=-1)
        out[f'f{i}/nts'] = np.array([200, 201, padlen + 1])
        try:
            filter_frequency(np.zeros((1, padlen), np.float32), freqs, fs, ft)
        except ValueError as e:
            meta[f'f{i}/short'] = str(e)
    meta['filter_cases'] = FILTER_CASES
    for ft, freqs in (('bandpass', [200, 100, 2000, 3000]), ('lowpass', [2000, 1000]), ('highpass', [1000, 2000])):
        try:
            filter_frequency(np.zeros((1, 300), np.float32), freqs, 10000.0, ft)
        except ValueError as e:
            meta[f'err/{ft}'] = [freqs, str(e)]
    # ---- gain
    nt = 200
    xg = rng.standard_normal((3, 4, nt)).astype(np.float32)
    xg[0, 1] = 0.0
    out['g/x'] = xg
    twt = np.arange(nt) * 0.0005
    out['g/twt'] = twt
    for i, kw in enumerate(GAIN_CASES):
        out[f'g/{i}/twt'] = gain(xg.copy(), twt, **kw)
        out[f'g/{i}/samples'] = gain(xg.copy(), np.arange(nt), **{k: v for k, v in kw.items() if not k.startswith('agc')})
    meta['gain_cases'] = [{k: (list(v.items()) if isinstance(v, dict) else v) for k, v in kw.items()} for kw in GAIN_CASES]
    x1 = rng.standard_normal((3, nt)).astype(np.float32)
    out['g/x1'] = x1
    for q in (0.5, 0.9, 0.99):
        out[f'g/qclip{q}'] = np.stack([gain(x1[k].copy(), twt, qclip=q) for k in range(3)])
    out['g/norm_rms'] = np.stack([gain(x1[k].copy(), twt, norm_rms=True) for k in range(3)])
    # ---- balance
    xb = rng.standard_normal((5, nt)).astype(np.float32)
    xb[2] = 0.0
    out['b/x'] = xb
    out['b/rms'] = calc_reference_amplitude(xb, axis=-1, scale='rms')
    out['b/max'] = calc_reference_amplitude(xb, axis=-1, scale='max')
    # ---- resampling
    for nt in (200, 201):
        x = rng.standard_normal((4, nt)).astype(np.float32)
        out[f'r/x{nt}'] = x
        for up, down in ((1, 2), (2, 1), (1, 3), (3, 1)):
            for w in ('hann', 'hamming', 'blackman'):
                out[f'r/poly{nt}_{up}_{down}_{w}'] = ss.resample_poly(x, up, down, axis=-1, window=w)
        for num in (100, 101, 400, 401):
            out[f'r/fft{nt}_{num}'] = ss.resample(x, num, window='hann', axis=-1)
    # ---- envelope
    for nt in (200, 201):
        x = rng.standard_normal((4, nt)).astype(np.float32)
        out[f'e/x{nt}'] = x
        out[f'e/y{nt}'] = envelope(x, axis=-1)
    # ---- coordinates
    tw = np.arange(0, 200) * 0.1 + 5.0
    for nres in (100, 67, 400):
        out[f'c/twt{nres}'] = get_resampled_twt(tw, nres, 200)
    meta['ffloat'] = [[v, ffloat(v)] for v in (0.2, 0.25, 1.0, 2.0, 0.1 * 3, 1 / 3, 12.5, 100.0)]
    # ---- the composed step-11 chain (its own random stream: the arrays above do not move)
    crng = np.random.default_rng(3)
    cube = crng.standard_normal((256, 5, 6)).astype(np.float32)
    cube[:, 1, 2] = 0.0
    ctwt = np.round(np.arange(256) * 0.2, 3)                   # ms
    y = np.moveaxis(cube, 0, -1)                               # (iline, xline, twt): the reference's core dims
    ref = calc_reference_amplitude(y, axis=-1, scale='rms')
    y = (y / ref[..., None]).astype(np.float32)
    y = gain(y, ctwt / 1000.0, tpow=2.0, agc=1.0).astype(np.float32)
    y = bandpass_filter(y, [50, 100, 800, 1000], fs=1 / (0.2 / 1000), axis=-1).astype(np.float32)
    y = ss.resample_poly(y, 1, 2, window='hann', axis=-1).astype(np.float32)
    y = envelope(y, axis=-1)
    out['chain/x'] = cube
    out['chain/twt'] = ctwt
    out['chain/ref'] = ref
    out['chain/env'] = np.moveaxis(y, -1, 0)
    out['chain/twt_out'] = np.around(get_resampled_twt(ctwt, 128, 256).astype('float64'), 3)
    out['__meta__'] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, 'preproc.npz'), **out)
    print('wrote preproc.npz with', len(out), 'arrays')


if __name__ == '__main__':
    main()
