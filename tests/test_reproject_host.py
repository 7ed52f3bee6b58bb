"""Step 2 without a GPU: the NumPy restatement of the projection and of the convolution (tests/helpers/reproject_numpy.py) against the mpmath
oracle and the reference's ``smooth`` recorded in tests/golden/reproject.npz (make_golden_reproject.py), which pins fixture and formulas on the
CPU; ``parse_crs`` on every accepted and refused form; the parser against the reference's flag list; output naming; and the command line end to
end with the device calls replaced by the restatement.

Tolerances (the issue's): forward 1e-6 m against the oracle (three orders below the finest header unit, 1e-3 m at scalar -1000; the float64 series
measured 3.7e-9 m when the fixture was made), inverse 1e-11 degrees (1e-6 m on the ground), smoothing 1e-6 m, header integers exact (the fixture
holds no value within 1e-6 m of a rounding tie)."""
import datetime
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import reproject_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd import _ffi  # noqa: E402
from pseudo_3d_interpolation_amd import reproject_segy as cli  # noqa: E402
from pseudo_3d_interpolation_amd.functions import crs as C  # noqa: E402
from pseudo_3d_interpolation_amd.functions import filter as F  # noqa: E402
from pseudo_3d_interpolation_amd.functions import segy as S  # noqa: E402
from pseudo_3d_interpolation_amd.functions.header import get_textual_header, unscale_coordinates  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'reproject.npz'))
SETTINGS = [str(s) for s in G['proj/settings']]
STRINGS = json.loads(str(G['proj/strings']))
TOL_M, TOL_DEG = 1e-6, 1e-11


def host_grid_to_grid(crs_src, crs_dst, x, y, device=0):
    return H.tm_forward(*H.tm_inverse(x, y, crs_src.prm), crs_dst.prm)


@pytest.fixture
def on_host(monkeypatch):
    """The three device calls of step 2 replaced by their NumPy restatement."""
    monkeypatch.setattr(_ffi, 'proj_tmerc', H.tmerc)
    monkeypatch.setattr(_ffi, 'proj_smooth', H.convolve_valid)
    monkeypatch.setattr(C, '_grid_to_grid', host_grid_to_grid)


# ---- fixture and formulas ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SETTINGS)
def test_series_against_the_oracle(name):
    prm, lon, lat, E, N = (G[f'proj/{name}/{k}'] for k in ('prm', 'lon', 'lat', 'E', 'N'))
    assert lon.size == 63 and np.abs(lat).max() == 84 and np.ptp(lon) == 10
    gE, gN = H.tm_forward(lon, lat, prm)
    print(name, 'forward', np.abs(gE - E).max(), np.abs(gN - N).max())
    assert np.abs(gE - E).max() <= TOL_M and np.abs(gN - N).max() <= TOL_M
    glon, glat = H.tm_inverse(E, N, prm)
    print(name, 'inverse', np.abs(glon - lon).max(), np.abs(glat - lat).max())
    assert np.abs(glon - lon).max() <= TOL_DEG and np.abs(glat - lat).max() <= TOL_DEG
    on_meridian, on_equator = lon == prm[2], lat == 0
    assert on_meridian.sum() == 9 and np.all(gE[on_meridian] == prm[5])
    if prm[3] == 0:
        assert on_equator.sum() == 7 and np.all(gN[on_equator] == prm[6])
    parsed = C.parse_crs(STRINGS[name])
    assert parsed.is_projected and parsed.prm.tobytes() == prm.tobytes()          # the parser gives the fixture's parameters bit for bit


def test_zone_to_zone_against_the_oracle():
    src, dst = G['z2z/prm_src'], G['z2z/prm_dst']
    gE, gN = H.tm_forward(*H.tm_inverse(G['z2z/E_src'], G['z2z/N_src'], src), dst)
    assert np.abs(gE - G['z2z/E_dst']).max() <= TOL_M and np.abs(gN - G['z2z/N_dst']).max() <= TOL_M
    assert C.parse_crs('EPSG:32632').prm.tobytes() == src.tobytes() and C.parse_crs('EPSG:32633').prm.tobytes() == dst.tobytes()


def test_header_fixture_is_consistent():
    lon, lat = G['hdr/lon_mas'] / 3600000, G['hdr/lat_mas'] / 3600000
    E, N = H.tm_forward(lon, lat, G['proj/utm60s_wgs84/prm'])
    assert lon.size == 300 and np.abs(E - G['hdr/E']).max() <= TOL_M and np.abs(N - G['hdr/N']).max() <= TOL_M
    for sc in G['hdr/scalars'].tolist():
        x, y = unscale_coordinates(E, N, sc)
        assert np.array_equal(x, G[f'hdr/{sc}/x']) and np.array_equal(y, G[f'hdr/{sc}/y']), sc
        assert np.abs(G[f'hdr/{sc}/y']).max() < 2**31


@pytest.mark.parametrize('length,wl', [tuple(c) for c in G['smooth/cases'].tolist()])
def test_smooth_against_the_reference(on_host, length, wl):
    data, want = G[f'smooth/in/{length}'], G[f'smooth/out/{length}/{wl}']
    got = F.smooth(data, wl)
    assert got.shape == want.shape == data.shape and np.abs(got - want).max() <= TOL_M
    assert 1e5 <= np.abs(data).max() <= 1.1e7


def test_smooth_windows_pass_through_and_errors(on_host):
    errors = json.loads(str(G['smooth/errors']))
    data = G['smooth/in/64']
    assert F.smooth(data, 2) is data and F.smooth(data, 0) is data
    for window in ('flat', 'hamming', 'bartlett', 'blackman'):
        assert np.abs(F.smooth(data, 7, window=window) - G[f'smooth/window/{window}']).max() <= TOL_M
    assert sorted(errors) == ['11/51', '12/51', 'ndim', 'window']
    for key in ('11/51', '12/51'):
        with pytest.raises(ValueError) as exc:
            F.smooth(G[f'smooth/in/{key.split("/")[0]}'], 51)
        assert str(exc.value) == errors[key]
    with pytest.raises(ValueError) as exc:
        F.smooth(np.zeros((4, 4)), 3)
    assert str(exc.value) == errors['ndim']
    with pytest.raises(ValueError) as exc:
        F.smooth(np.arange(20.0), 5, window='kaiser')
    assert str(exc.value) == errors['window']


# ---- parse_crs -----------------------------------------------------------------------------------------------------------------------
WGS84, GRS80 = (6378137.0, 1 / 298.257223563), (6378137.0, 1 / 298.257222101)


def test_parse_crs_epsg_codes():
    for text, ell in (('EPSG:4326', WGS84), ('epsg:4258', GRS80), (' Epsg:4326 ', WGS84), ('4326', WGS84), (4326, WGS84)):
        c = C.parse_crs(text)
        assert c.kind == 'geographic' and c.is_geographic and not c.is_projected and (c.a, c.f) == ell and c.epsg in (4326, 4258)
    for zone in (1, 32, 60):
        n, s = C.parse_crs(f'EPSG:{32600 + zone}'), C.parse_crs(f'epsg:{32700 + zone}')
        assert (n.kind, n.a, n.f, n.lon0, n.lat0, n.k0, n.x0, n.y0, n.epsg) == ('tmerc', *WGS84, 6 * zone - 183, 0, 0.9996, 500000, 0, 32600 + zone)
        assert (s.lon0, s.x0, s.y0, s.epsg) == (6 * zone - 183, 500000, 10000000, 32700 + zone) and s.is_projected and not s.is_geographic
    for zone in (28, 32, 38):
        e = C.parse_crs(f'EPSG:{25800 + zone}')
        assert (e.kind, e.a, e.f, e.lon0, e.k0, e.x0, e.y0, e.epsg) == ('tmerc', *GRS80, 6 * zone - 183, 0.9996, 500000, 0, 25800 + zone)
    assert C.parse_crs('EPSG:32760').lon0 == 177 and C.parse_crs(C.parse_crs('EPSG:32760')) == C.parse_crs('EPSG:32760')


def test_parse_crs_proj4_strings():
    assert C.parse_crs('+proj=longlat +datum=WGS84 +no_defs').kind == 'geographic' and C.parse_crs('+proj=longlat +datum=WGS84').epsg is None
    assert (C.parse_crs('+proj=longlat +ellps=GRS80').a, C.parse_crs('+proj=longlat +ellps=GRS80').f) == GRS80
    u = C.parse_crs('+proj=utm +zone=60 +south +datum=WGS84 +units=m +no_defs')
    assert u.epsg == 32760 and u.prm.tobytes() == C.parse_crs('EPSG:32760').prm.tobytes()
    assert C.parse_crs('+PROJ=UTM +ZONE=32 +ELLPS=WGS84').epsg == 32632 and C.parse_crs('+proj=utm +zone=32').epsg == 32632
    g = C.parse_crs('+proj=utm +zone=32 +ellps=GRS80')
    assert g.epsg is None and g.prm.tobytes() == C.parse_crs('EPSG:25832').prm.tobytes()
    t = C.parse_crs('+proj=tmerc +lat_0=-41.5 +lon_0=173 +k=0.9996 +x_0=1600000 +y_0=250000.5 +ellps=GRS80')
    assert (t.kind, t.a, t.f, t.lon0, t.lat0, t.k0, t.x0, t.y0, t.epsg) == ('tmerc', *GRS80, 173, -41.5, 0.9996, 1600000, 250000.5, None)
    assert C.parse_crs('+proj=tmerc +lon_0=9 +k_0=0.9999 +datum=WGS84').k0 == 0.9999 and C.parse_crs('+proj=tmerc +lon_0=9').k0 == 1.0
    assert C.parse_crs('+proj=tmerc +lon_0=9').to_epsg() is None and C.parse_crs('EPSG:25832').to_epsg() == 25832


@pytest.mark.parametrize('text', [
    'EPSG:2193', 'EPSG:3857', 'EPSG:32661', 'EPSG:32600', 'EPSG:25839', 'EPSG:25827', 'EPSG:4269', 'WGS84', '', 'urn:ogc:def:crs:EPSG::4326',
    '+proj=merc +datum=WGS84', '+proj=utm +zone=61', '+proj=utm +zone=0', '+proj=utm', '+proj=utm +zone=32.5', '+proj=longlat +datum=NAD83',
    '+proj=longlat +ellps=bessel', '+proj=tmerc +lon_0=9 +k=1 +k_0=1', '+proj=tmerc +lon_0=nine', '+proj=tmerc +lon_0=9 +towgs84=1,2,3 +nadgrids=x',
    '+proj=tmerc +lon_0=9 +units=ft', '+proj=tmerc +lat_0=95', '+proj=tmerc +k=0', '+proj=utm +zone=32 +datum=WGS84 +ellps=GRS80', 'proj=utm zone=32',
    None, 4.5])
def test_parse_crs_refuses_with_the_accepted_list(text):
    with pytest.raises(NotImplementedError, match=r'EPSG:32601-32660.*no datum shifts'):
        C.parse_crs(text)


def test_transform_host_rules(on_host, monkeypatch):
    lon, lat = G['proj/utm32n_wgs84/lon'], G['proj/utm32n_wgs84/lat']
    with pytest.raises(NotImplementedError, match='different ellipsoids.*no datum shifts'):
        C.transform('EPSG:4326', 'EPSG:25832', lon, lat)
    with pytest.raises(NotImplementedError, match='different ellipsoids'):
        C.transform('EPSG:32632', 'EPSG:25832', lon, lat)
    same = C.transform('EPSG:32632', '+proj=utm +zone=32 +datum=WGS84', lon, lat)
    assert same[0].tobytes() == lon.tobytes() and same[1].tobytes() == lat.tobytes() and same[0] is not lon
    E, N = C.transform('epsg:4326', 'epsg:32632', lon, lat)
    assert np.abs(E - G['proj/utm32n_wgs84/E']).max() <= TOL_M and np.abs(N - G['proj/utm32n_wgs84/N']).max() <= TOL_M
    blon, blat = C.transform('epsg:32632', 'epsg:4326', E, N)
    assert np.abs(blon - lon).max() <= TOL_DEG and np.abs(blat - lat).max() <= TOL_DEG
    with pytest.raises(ValueError, match='non-finite'):
        C.transform('epsg:4326', 'epsg:32632', np.array([9.0, np.nan]), np.array([50.0, 50.0]))
    with pytest.raises(ValueError, match='shape'):
        C.transform('epsg:4326', 'epsg:32632', np.zeros(3), np.zeros(4))
    monkeypatch.setattr(_ffi, 'proj_tmerc', H.tmerc_dev_unavailable)
    empty = C.transform('epsg:4326', 'epsg:32632', np.zeros(0), np.zeros(0))
    assert empty[0].shape == (0,)


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_flags_are_the_reference_list():
    want = json.loads(str(G['cli_flags']))
    got = [a for a in cli.define_input_args()._actions if a.dest != 'help']
    assert [a.dest for a in got] == [w['dest'] for w in want] and len(want) == 13
    assert [w['dest'] for w in want] == ['input_path', 'crs_src', 'crs_dst', 'output_dir', 'inplace', 'filename_suffix', 'suffix', 'txt_suffix',
                                         'scalar_coords', 'src_coords', 'dst_coords', 'smooth', 'verbose']
    for a, w in zip(got, want):
        assert list(a.option_strings) == w['flags'] and a.default == w['default'] and a.nargs == w['nargs'] and a.const == w['const'], w['dest']
        assert a.required == w['required'] and (None if a.choices is None else list(a.choices)) == w['choices'], w['dest']
        assert (None if a.type is None else a.type.__name__) == w['type'] and a.help == w['help'], w['dest']
    assert cli.define_input_args().description == str(G['cli_description'])
    args = cli.define_input_args().parse_args(['x.sgy', '--crs_src', 'a', '--crs_dst', 'b', '--smooth'])
    assert args.scalar_coords == -100 and args.smooth == 11 and args.src_coords == args.dst_coords == 'source'
    cfg = open(os.path.join(ROOT, 'setup.cfg')).read()
    assert '02_reproject_segy = pseudo_3d_interpolation_amd.reproject_segy:main' in cfg


def write_arcsec(path, ntr=300, units=2, **extra):
    rng = np.random.default_rng(5)
    data = rng.standard_normal((ntr, 16)).astype(np.float32)
    headers = {'SourceX': G['hdr/lon_mas'][:ntr], 'SourceY': G['hdr/lat_mas'][:ntr], 'CoordinateUnits': units, 'SourceGroupScalar': 1,
               'FieldRecord': np.arange(ntr) + 100, 'CDP_X': np.arange(ntr) * 3, 'GroupY': 7 - np.arange(ntr), **extra}
    return S.write_segy(str(path), data, 0.25, headers=headers, text='C 1 CLIENT'.ljust(80) + 'C 2 LINE'.ljust(80))


def check_other_bytes(src, dst, changed_fields):
    """Samples, binary header and every trace-header byte outside ``changed_fields`` are the input's."""
    a, b = open(src, 'rb').read(), open(dst, 'rb').read()
    assert len(a) == len(b) and a[3200:3600] == b[3200:3600]
    size = 240 + 16 * 4
    ta, tb = (np.frombuffer(v[3600:], np.uint8).reshape(-1, size).copy() for v in (a, b))
    for name in changed_fields:
        byte, dt = S.TRACE_FIELDS[name]
        ta[:, byte - 1:byte - 1 + np.dtype(dt).itemsize] = tb[:, byte - 1:byte - 1 + np.dtype(dt).itemsize] = 0
    assert np.array_equal(ta, tb)


def header_lines(path):
    return [line[3:].rstrip() for line in get_textual_header(path).split('\n')]


@pytest.mark.parametrize('scalar', G['hdr/scalars'].tolist())
def test_arc_seconds_to_utm60s(on_host, tmp_path, scalar):
    src = write_arcsec(tmp_path / 'line.sgy')
    before = open(src, 'rb').read()
    with pytest.raises(SystemExit):
        cli.main(['02_reproject_segy', src, '--crs_src', 'EPSG:4326', '--crs_dst', 'EPSG:32760', '-sc', str(scalar)])
    dst = str(tmp_path / 'line_reproj.sgy')
    assert sorted(os.listdir(tmp_path)) == ['line.sgy', 'line_reproj.sgy'] and open(src, 'rb').read() == before
    out = S.SegyFile(dst)
    assert np.array_equal(out.header('SourceX'), G[f'hdr/{scalar}/x']) and np.array_equal(out.header('SourceY'), G[f'hdr/{scalar}/y'])
    assert set(out.header('CoordinateUnits').tolist()) == {1} and set(out.header('SourceGroupScalar').tolist()) == {scalar}
    check_other_bytes(src, dst, ['SourceX', 'SourceY', 'CoordinateUnits', 'SourceGroupScalar'])
    lines = header_lines(dst)
    assert ' CRS (PROJECTED): EPSG:32760' in lines and f' {datetime.date.today().isoformat()}: REPROJECT (BYTES:73 77)' in lines
    assert lines[0] == ' CLIENT' and not any('REPROJECT' in line for line in header_lines(src))


def test_projected_source_with_arc_second_units_is_forced_geographic(on_host, tmp_path, capsys):
    src = write_arcsec(tmp_path / 'line.sgy')
    with pytest.raises(SystemExit):
        cli.main(['x', src, '--crs_src', 'EPSG:32632', '--crs_dst', 'EPSG:32760', '--dst_coords', 'CDP', '-V', '1'])
    assert 'Forced source CRS to be geographic (WGS84 - EPSG:4326)!' in capsys.readouterr().out
    out = S.SegyFile(str(tmp_path / 'line_reproj.sgy'))
    assert np.array_equal(out.header('CDP_X'), G['hdr/-100/x']) and np.array_equal(out.header('CDP_Y'), G['hdr/-100/y'])
    assert np.array_equal(out.header('SourceX'), G['hdr/lon_mas']) and ' ' + f'{datetime.date.today().isoformat()}: REPROJECT (BYTES:181 185)' in header_lines(out.path)
    check_other_bytes(src, out.path, ['CDP_X', 'CDP_Y', 'CoordinateUnits', 'SourceGroupScalar'])


def test_millimetre_northing_outside_32_bits_is_refused(on_host, tmp_path):
    src = write_arcsec(tmp_path / 'line.sgy', SourceY=G['hdr/lat_mas'] + int(35.7 * 3600000))      # latitude -36.8: northing 5.9e6 m
    with pytest.raises(OverflowError, match='32-bit'):
        cli.main(['x', src, '--crs_src', 'EPSG:4326', '--crs_dst', 'EPSG:32760', '-sc', '-1000'])


def test_utm32_to_utm33(on_host, tmp_path):
    n = G['z2z/E_src'].size
    x_in, y_in = np.around(G['z2z/E_src'] * 100).astype(np.int64), np.around(G['z2z/N_src'] * 100).astype(np.int64)
    src = write_arcsec(tmp_path / 'line.sgy', ntr=n, units=1, SourceX=x_in, SourceY=y_in, SourceGroupScalar=-100)
    with pytest.raises(SystemExit):
        cli.main(['x', src, '--crs_src', 'EPSG:32632', '--crs_dst', 'EPSG:32633', '-sc', '-10', '--txt_suffix', 'z33'])
    out = S.SegyFile(str(tmp_path / 'line_z33.sgy'))
    wx, wy = unscale_coordinates(*host_grid_to_grid(C.parse_crs(32632), C.parse_crs(32633), x_in / 100, y_in / 100), -10)
    assert np.array_equal(out.header('SourceX'), wx) and np.array_equal(out.header('SourceY'), wy)
    # the input was rounded to centimetres (0.005 m, stretched by at most a few 1e-4 between the grids), the output to decimetres (0.05 m)
    assert np.abs(out.header('SourceX') / 10 - G['z2z/E_dst']).max() <= 0.056 and np.abs(out.header('SourceY') / 10 - G['z2z/N_dst']).max() <= 0.056
    assert set(out.header('CoordinateUnits').tolist()) == {1} and set(out.header('SourceGroupScalar').tolist()) == {-10}
    assert ' CRS (PROJECTED): EPSG:32633' in header_lines(out.path)


def test_smooth_run(on_host, tmp_path):
    src = write_arcsec(tmp_path / 'line.sgy')
    with pytest.raises(SystemExit):
        cli.main(['x', src, '--crs_src', 'EPSG:4326', '--crs_dst', 'EPSG:32760', '--smooth', '--inplace'])
    out = S.SegyFile(src)
    assert os.listdir(tmp_path) == ['line.sgy']
    assert np.array_equal(out.header('SourceX'), G['hdr/smooth11/x']) and np.array_equal(out.header('SourceY'), G['hdr/smooth11/y'])
    assert not np.array_equal(G['hdr/smooth11/x'], G['hdr/-100/x'])
    assert f' {datetime.date.today().isoformat()}: REPROJECT (BYTES:73 77) SMOOTHED' in header_lines(src)


def test_refusals_leave_no_output(on_host, tmp_path):
    src = write_arcsec(tmp_path / 'dd.sgy', units=3)
    with pytest.raises(NotImplementedError, match='Functionality to convert DD data is not implemented.'):
        cli.main(['x', src, '--crs_src', 'EPSG:4326', '--crs_dst', 'EPSG:32760', '--inplace'])
    dms = write_arcsec(tmp_path / 'dms.sgy', units=4)
    with pytest.raises(NotImplementedError, match='Functionality to convert DMS data is not implemented.'):
        cli.main(['x', dms, '--crs_src', 'EPSG:4326', '--crs_dst', 'EPSG:32760', '--inplace'])
    ok = write_arcsec(tmp_path / 'ok.sgy')
    with pytest.raises(NotImplementedError, match='Functionality to convert to geographic output CRS is not yet implemented.'):
        cli.main(['x', ok, '--crs_src', 'EPSG:32760', '--crs_dst', 'EPSG:4326'])
    with pytest.raises(NotImplementedError, match='EPSG code 2193 is not known here'):
        cli.main(['x', ok, '--crs_src', 'EPSG:4326', '--crs_dst', 'EPSG:2193'])
    assert sorted(os.listdir(tmp_path)) == ['dd.sgy', 'dms.sgy', 'ok.sgy']
    with pytest.raises(FileNotFoundError):
        cli.main(['x', str(tmp_path / 'missing.sgy'), '--crs_src', 'EPSG:4326', '--crs_dst', 'EPSG:32760'])
    with pytest.raises(FileNotFoundError, match='does not exist'):
        cli.main(['x', ok, '--crs_src', 'EPSG:4326', '--crs_dst', 'EPSG:32760', '-o', str(tmp_path / 'nowhere')])


def test_directory_and_list_inputs_and_naming(on_host, tmp_path):
    d = tmp_path / 'lines'
    d.mkdir()
    one, two = write_arcsec(d / 'a_env.sgy'), write_arcsec(d / 'b_env.sgy')
    write_arcsec(d / 'c_raw.sgy')
    write_arcsec(d / 'd_env.segy')
    out = tmp_path / 'out'
    out.mkdir()
    (out / 'a_env_reproj.sgy').write_bytes(b'stale')                     # an existing output is removed first
    common = ['--crs_src', 'EPSG:4326', '--crs_dst', 'EPSG:32760']
    cli.main(['x', str(d), *common, '-fns', 'env', '-o', str(out), '-V', '1'])
    assert sorted(os.listdir(out)) == ['a_env_reproj.sgy', 'b_env_reproj.sgy']
    for name in os.listdir(out):
        assert np.array_equal(S.SegyFile(str(out / name)).header('SourceX'), G['hdr/-100/x'])
    logs = [n for n in os.listdir(d) if n.endswith('.log')]
    log = open(d / logs[0]).read()
    assert len(logs) == 1 and logs[0].endswith('_reproject_segy.log') and '\x1b' not in log
    assert 'Processing total of < 2 > files' in log and 'Processing file < a_env.sgy >' in log and 'Output file already exists and will be removed!' in log
    os.remove(d / logs[0])
    cli.main(['x', str(d), *common, '-s', 'segy', '--txt_suffix', 'utm'])
    assert sorted(n for n in os.listdir(d) if 'utm' in n) == ['d_env_utm.segy']
    os.remove(next(d / n for n in os.listdir(d) if n.endswith('.log')))

    (d / 'list.txt').write_text('a_env.sgy\nb_env.sgy\n')
    cli.main(['x', str(d / 'list.txt'), *common, '--inplace', '-sc', '0'])
    for path in (one, two):
        seg = S.SegyFile(path)
        assert np.array_equal(seg.header('SourceY'), G['hdr/0/y']) and set(seg.header('SourceGroupScalar').tolist()) == {0}
    assert len([n for n in os.listdir(d) if n.endswith('.log')]) == 1 and not any(n.endswith('_reproj.sgy') for n in os.listdir(d))
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(SystemExit, match='No input files to process'):
        cli.main(['x', str(empty), *common])
