"""Step 6 without a GPU: the netCDF classic reader against the helper's writer (and against scipy where installed), ``load_subset`` on the
synthetic model (seam, clamp, errors, a sparse file of the real atlas's size), the recording-time conversion, the parser against the reference's
flag list, what is refused, the float64 helper oracle against the mpmath fixture (tests/golden/tide.npz, make_golden_tide.py), the reference's
conversions and the ``.tid`` lines."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import tide_numpy as H  # noqa: E402

from pseudo_3d_interpolation_amd import tide_compensation_segy as cli  # noqa: E402
from pseudo_3d_interpolation_amd.functions import tide as T  # noqa: E402
from pseudo_3d_interpolation_amd.functions import tide_model as M  # noqa: E402
from pseudo_3d_interpolation_amd.functions import utils as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'tide.npz'))
TOL_M = 1e-8


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp('model'))
    return (folder, *H.make_model(folder))


# ---- reader ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('version', [1, 2])
def test_reader_against_the_writer(tmp_path, version):
    rng = np.random.default_rng(version)
    a, b, c = rng.integers(-2**31, 2**31, (5, 3)).astype(np.int32), rng.standard_normal(5), rng.standard_normal((3, 5)).astype(np.float32)
    d = rng.integers(-100, 100, 3).astype(np.int16)                        # 6 bytes: padded to 8 in the file
    path = H.write_classic(str(tmp_path / 'x.nc'), {'nx': 5, 'ny': 3}, [('a', ('nx', 'ny'), a), ('d', ('ny',), d), ('b', ('nx',), b), ('c', ('ny', 'nx'), c)],
                           version=version, attrs={'title': 'abcde', 'note': 'xy'})
    f = M.ClassicFile(path)
    assert open(path, 'rb').read(4) == b'CDF' + bytes([version])
    assert f.dims == {'nx': 5, 'ny': 3} and f.attrs == {'title': 'abcde', 'note': 'xy'} and list(f.variables) == ['a', 'd', 'b', 'c']
    for name, want in (('a', a), ('d', d), ('b', b), ('c', c)):
        got = f.var(name)
        assert isinstance(got, np.memmap) and got.dtype.byteorder == '>' and got.shape == want.shape and np.array_equal(got, want)
        assert f.variables[name]['dims'] == {'a': ('nx', 'ny'), 'd': ('ny',), 'b': ('nx',), 'c': ('ny', 'nx')}[name]
    with pytest.raises(ValueError, match='x.nc.*no variable'):
        f.var('hRe')


def test_reader_against_scipy(tmp_path):
    netcdf_file = pytest.importorskip('scipy.io').netcdf_file
    path = str(tmp_path / 's.nc')
    rng = np.random.default_rng(0)
    re, lon = rng.integers(-1500, 1500, (6, 4)).astype(np.int32), np.arange(1, 7) * 60.0
    with netcdf_file(path, 'w', version=2) as nc:
        nc.title = 'from scipy'
        nc.createDimension('nx', 6)
        nc.createDimension('ny', 4)
        v = nc.createVariable('lon_z', 'd', ('nx',))
        v[:] = lon
        v.units = 'degrees'
        w = nc.createVariable('hRe', 'i', ('nx', 'ny'))
        w[:] = re
    f = M.ClassicFile(path)
    assert f.dims == {'nx': 6, 'ny': 4} and f.attrs['title'] == 'from scipy' and f.variables['lon_z']['attrs']['units'] == 'degrees'
    assert np.array_equal(f.var('lon_z'), lon) and np.array_equal(f.var('hRe'), re)
    mine = H.write_classic(str(tmp_path / 'm.nc'), {'nx': 6, 'ny': 4}, [('lon_z', ('nx',), lon), ('hRe', ('nx', 'ny'), re)])
    with netcdf_file(mine, 'r', mmap=False) as nc:                          # and the helper's writer is read by scipy
        assert np.array_equal(nc.variables['hRe'][:], re) and np.array_equal(nc.variables['lon_z'][:], lon)


def test_reader_refuses_what_it_cannot_read(tmp_path):
    bad = tmp_path / 'bad.nc'
    bad.write_bytes(b'CDF\x05' + b'\x00' * 60)
    with pytest.raises(ValueError, match='bad.nc.*not a netCDF classic file'):
        M.open_model_file(str(bad))
    short = tmp_path / 'short.nc'
    short.write_bytes(b'CDF\x01\x00\x00')
    with pytest.raises(ValueError, match='short.nc.*ends early'):
        M.open_model_file(str(short))
    hdf = tmp_path / 'four.nc'
    hdf.write_bytes(M.HDF5_MAGIC + b'\x00' * 100)
    if not M.h5py_enabled:
        with pytest.raises(ImportError, match='reading netCDF needs xarray \\+ h5netcdf, or h5py'):
            M.open_model_file(str(hdf))
    # a record variable: dimension of length 0 first
    rec = H.write_classic(str(tmp_path / 'rec.nc'), {'time': 0, 'nx': 2}, [('lon_z', ('nx',), np.arange(2.0)), ('h', ('time', 'nx'), np.zeros((0, 2)))])
    f = M.ClassicFile(rec)
    assert f.variables['h']['record'] and not f.variables['lon_z']['record']
    with pytest.raises(ValueError, match='rec.nc.*record variable'):
        f.var('h')
    with pytest.raises(ValueError, match='axis.nc.*lat_z does not rise uniformly'):
        M.uniform_axis([0, 1, 2.000001], 'axis.nc', 'lat_z')
    with pytest.raises(ValueError, match='does not rise uniformly'):
        M.uniform_axis([3, 2, 1], 'axis.nc', 'lat_z')
    assert M.uniform_axis(-90 + 180 / 5400 * np.arange(5401), 'p', 'lat_z') == (-90.0, pytest.approx(1 / 30, rel=1e-12))


# ---- load_subset -----------------------------------------------------------------------------------------------------------------------
def whole(fields, names):
    return np.array([fields[c][0] for c in names]), np.array([fields[c][1] for c in names])


def test_subset_inside_the_grid(model):
    folder, lon_z, lat_z, fields, hz = model
    names = ('k1', 'm2')
    sub = M.load_subset(folder, names, [41.0, 52.5, 47.0], [-12.0, -3.0, -7.5])
    # cells 40 ... 45 to 50 ... 55 and -15 ... -10 to -5 ... 0, one node more on each side
    assert (sub.lon0, sub.dlon, sub.lat0, sub.dlat) == (35.0, 5.0, -20.0, 5.0) and sub.hre.shape == (2, 6, 6) and sub.wet.shape == (6, 6)
    assert sub.hre.dtype == sub.him.dtype == np.int32 and sub.wet.dtype == np.uint8 and sub.hre.flags.c_contiguous and sub.hre.dtype.isnative
    re, im = whole(fields, names)
    assert np.array_equal(sub.hre, re[:, 6:12, 14:20]) and np.array_equal(sub.him, im[:, 6:12, 14:20]) and sub.wet.all()
    assert np.array_equal(sub.lon, [41.0, 52.5, 47.0]) and sub.constituents == names and sub.ids.tolist() == [4, 0]
    assert np.array_equal(sub.grid, [35.0, 5.0, -20.0, 5.0])


@pytest.mark.parametrize('lons', [[358.0, 1.0, 3.0], [-2.0, 361.0, 363.0], [718.0, 1.0, -357.0]])
def test_subset_across_the_seam(model, lons):
    folder, lon_z, lat_z, fields, hz = model
    sub = M.load_subset(folder, ['m2'], lons, [61.0, 62.0, 66.0])
    # cells 355 ... 360 and 0 ... 5: nodes 350 ... 370 = indices 69, 70, 71, 0, 1; latitudes 55 ... 75
    assert (sub.lon0, sub.lat0) == (350.0, 55.0) and sub.hre.shape == (1, 5, 5)
    rows = [69, 70, 71, 0, 1]
    assert np.array_equal(sub.hre[0], fields['m2'][0][rows, 29:34]) and np.array_equal(sub.wet, (hz[rows, 29:34] > 0).astype(np.uint8))
    assert np.allclose(sub.lon, [358.0, 361.0, 363.0], rtol=0, atol=1e-12) and (np.diff(sub.lon0 + sub.dlon * np.arange(5)) > 0).all()
    assert sub.wet[4, 2:5].tolist() == [0, 0, 0] and sub.wet[:3].all()           # the dry block starts at 5 E (index 0), 65 N


def test_subset_clamps_the_latitude_and_keeps_a_cell(model):
    folder = model[0]
    top = M.load_subset(folder, ['m2'], [100.0], [90.0])
    assert top.lat0 + top.dlat * (top.hre.shape[2] - 1) == 90.0 and top.lat0 == 85.0 and top.hre.shape == (1, 4, 2)
    bottom = M.load_subset(folder, ['m2'], [100.0, 101.0], [-90.0, -89.0])
    assert bottom.lat0 == -90.0 and bottom.hre.shape[2] == 3
    one = M.load_subset(folder, ['s2'], [0.0], [0.0])                            # a single point on a node, on the seam
    assert one.hre.shape == (1, 4, 4) and one.lon0 == -5.0 and one.lon[0] == 0.0           # the axis starts below the first node: -5, 0, 5, 10
    assert np.array_equal(one.hre[0], model[3]['s2'][0][[70, 71, 0, 1], 17:21])


def test_subset_without_a_grid_file_is_all_wet(tmp_path):
    H.make_model(str(tmp_path), constituents=('m2',), grid=False)
    assert M.load_subset(str(tmp_path), ['m2'], [7.0], [70.0]).wet.all()


def test_subset_errors(model, tmp_path):
    folder = model[0]
    with pytest.raises(ValueError, match='span 190.000 degrees'):
        M.load_subset(folder, ['m2'], [0.0, 95.0, 190.0], [0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match='latitudes'):
        M.load_subset(folder, ['m2'], [0.0], [90.5])
    with pytest.raises(ValueError, match="'z9'"):
        M.load_subset(folder, ['z9'], [0.0], [0.0])
    with pytest.raises(ValueError, match='non-finite'):
        M.load_subset(folder, ['m2'], [np.nan], [0.0])
    H.make_model(str(tmp_path), constituents=('m2',))
    with pytest.raises(FileNotFoundError, match='h_k1_\\*.nc'):
        M.load_subset(str(tmp_path), ['m2', 'k1'], [0.0], [0.0])
    regional = tmp_path / 'regional'
    regional.mkdir()
    H.write_classic(str(regional / 'h_m2_r.nc'), {'nx': 4, 'ny': 3}, [('lon_z', ('nx',), np.arange(4.0)), ('lat_z', ('ny',), np.arange(3.0)),
                                                                      ('hRe', ('nx', 'ny'), np.zeros((4, 3), np.int32)),
                                                                      ('hIm', ('nx', 'ny'), np.zeros((4, 3), np.int32))])
    with pytest.raises(ValueError, match='h_m2_r.nc.*do not cover the circle'):
        M.load_subset(str(regional), ['m2'], [1.5], [1.5])


def test_subset_closes_every_file_it_opened(model, monkeypatch):
    """A netCDF-4 file is an open h5py handle: each file opened for a subset is closed once, whether the subset is returned or an error raised."""
    folder, log, real = model[0], [], M.open_model_file

    class Recorded:
        def __init__(self, path):
            self.inner, self.path = real(path), path

        def var(self, name):
            assert ('close', self.path) not in log
            return self.inner.var(name)

        def close(self):
            log.append(('close', self.path))
            self.inner.close()

    def opening(path):
        log.append(('open', path))
        return Recorded(path)

    monkeypatch.setattr(M, 'open_model_file', opening)
    want = real(os.path.join(folder, 'h_k1_synthetic.nc')).var('hRe')
    sub = M.load_subset(folder, ['m2', 'k1'], [20.0, 31.0], [-10.0, 4.0])
    opened = [p for what, p in log if what == 'open']
    assert len(opened) == 3 and sorted(opened) == sorted(p for what, p in log if what == 'close')
    assert np.array_equal(sub.hre[1], want[2:8, 15:21])                          # the subset outlives the files: copies
    del log[:]
    with pytest.raises(ValueError, match='latitudes'):
        M.load_subset(folder, ['m2'], [0.0], [90.5])
    assert [what for what, _ in log] == ['open', 'close']


def test_subset_of_a_sparse_file_of_atlas_size(tmp_path):
    """A file of the real atlas's extent (10800 x 5401 nodes, 233 MB per variable) whose tables are holes: the subset has the shape of the
    bounding box and the file is never read whole (it would be 467 MB; the subset's rows are 2 x 5 x 5 values)."""
    nx, ny = 10800, 5401
    lon_z, lat_z = np.arange(1, nx + 1) / 30.0, -90.0 + np.arange(ny) / 30.0
    path = H.write_classic(str(tmp_path / 'h_m2_big.nc'), {'nx': nx, 'ny': ny},
                           [('lon_z', ('nx',), lon_z), ('lat_z', ('ny',), lat_z), ('hRe', ('nx', 'ny'), None), ('hIm', ('nx', 'ny'), None)], version=2,
                           sparse=('hRe', 'hIm'))
    assert os.path.getsize(path) > 2 * nx * ny * 4 and os.stat(path).st_blocks * 512 < 2**22
    sub = M.load_subset(str(tmp_path), ['m2'], [359.99, 0.01, 0.03], [-41.31, -41.29, -41.30])
    assert sub.hre.shape == (1, 5, 5) and not sub.hre.any() and not isinstance(sub.hre, np.memmap) and sub.wet.all()
    assert abs(sub.lon0 - (360 - 2 / 30)) < 1e-9 and abs(sub.lat0 - (-90 + 1459 / 30)) < 1e-9 and sub.lon[1] > 360


# ---- times -----------------------------------------------------------------------------------------------------------------------------
def test_header_times_and_seconds_since_1992():
    times = T.header_times([1992, 2024, 1985, 2023], [1, 366, 32, 365], [0, 23, 6, 0], [0, 59, 30, 0], [0, 59, 15, 1])
    assert times.tolist() == np.array(['1992-01-01T00:00:00', '2024-12-31T23:59:59', '1985-02-01T06:30:15', '2023-12-31T00:00:01'], 'datetime64[s]').tolist()
    sec = T.seconds_since_1992(times)
    assert sec.dtype == np.float64 and sec[0] == 0.0 and sec[2] == -((365 * 7 + 1) * 86400 - (31 * 86400 + 6 * 3600 + 30 * 60 + 15))
    assert sec[1] == (33 * 365 + 9) * 86400 - 1                                  # 1992 ... 2024: 33 years, 9 of them leap
    assert T.seconds_since_1992(['1991-12-31T23:59:59.5', '1992-01-01'])[0] == -0.5
    assert np.isnan(T.seconds_since_1992(np.array(['NaT'], 'datetime64[s]'))[0])
    for bad, words in (((2023, 366, 0, 0, 0), 'day of year 366'), ((0, 1, 0, 0, 0), 'year 0'), ((2024, 0, 0, 0, 0), 'day of year 0'),
                       ((2024, 1, 24, 0, 0), '24:0:0'), ((2024, 1, 0, 60, 0), '0:60:0'), ((2024, 1, 0, 0, 60), '0:0:60'), ((98, 1, 0, 0, 0), 'year 98')):
        cols = [[g, v, g] for g, v in zip((2024, 5, 1, 2, 3), bad)]             # the second of three traces is the bad one
        with pytest.raises(ValueError, match=f'trace #1 .*{words}'):
            T.header_times(*cols)


# ---- command line and refusals ---------------------------------------------------------------------------------------------------------
def test_cli_flags_are_the_reference_list():
    want = json.loads(str(G['cli_flags']))
    got = [a for a in cli.define_input_args()._actions if a.dest != 'help']
    assert [a.dest for a in got] == [w['dest'] for w in want] and len(want) == 13
    assert [w['dest'] for w in want] == ['input_path', 'model_dir', 'output_dir', 'inplace', 'suffix', 'filename_suffix', 'txt_suffix', 'constituents',
                                         'correct_minor', 'src_coords', 'crs_src', 'write_aux', 'verbose']
    for a, w in zip(got, want):
        assert list(a.option_strings) == w['flags'] and a.default == w['default'] and a.nargs == w['nargs'] and a.const == w['const'], w['dest']
        assert a.required == w['required'] and (None if a.choices is None else list(a.choices)) == w['choices'], w['dest']
        assert (None if a.type is None else a.type.__name__) == w['type'] and a.help == w['help'], w['dest']
    assert cli.define_input_args().description == str(G['cli_description'])
    args = cli.define_input_args().parse_args(['x.sgy', 'model'])
    assert args.constituents == list(T.DEFAULT_CONSTITUENTS) == list(M.CONSTITUENTS[:8]) and args.crs_src == 'epsg:32760' and not args.write_aux
    assert tuple(json.loads(str(G['cli_flags']))[7]['choices']) == M.CONSTITUENTS == H.CONSTITUENTS
    cfg = open(os.path.join(ROOT, 'setup.cfg')).read()
    assert '06_compensate_tide = pseudo_3d_interpolation_amd.tide_compensation_segy:main' in cfg


def test_minor_constituents_and_full_mode_are_refused_before_any_file_is_touched(tmp_path):
    missing = str(tmp_path / 'nowhere')
    with pytest.raises(NotImplementedError, match='minor constituents'):
        T.tide_predict(missing, [0.0], [0.0], ['2020-01-01'], correct_minor=True)
    with pytest.raises(NotImplementedError, match="mode='full'"):
        T.tide_predict(missing, [0.0], [0.0], ['2020-01-01'], mode='full')
    with pytest.raises(ValueError, match='neither'):
        T.tide_predict(missing, [0.0], [0.0], ['2020-01-01'], mode='grid')
    with pytest.raises(ValueError, match='non-finite'):
        T.tide_predict(missing, [np.inf], [0.0], ['2020-01-01'])
    with pytest.raises(ValueError, match='non-finite'):
        T.tide_predict(missing, [0.0], [0.0], np.array(['NaT'], 'datetime64[s]'))
    with pytest.raises(ValueError, match='one time per position'):
        T.tide_predict(missing, [0.0, 1.0], [0.0, 1.0], ['2020-01-01'])
    with pytest.raises(FileNotFoundError):
        cli.main(['06_compensate_tide', str(tmp_path / 'no.sgy'), missing])


def test_minor_constituents_are_refused_before_the_copy(tmp_path):
    from pseudo_3d_interpolation_amd.functions import segy as S
    src = S.write_segy(str(tmp_path / 'line.sgy'), np.zeros((3, 8), np.float32), 0.05)
    with pytest.raises(NotImplementedError, match='minor constituents'):
        cli.main(['06_compensate_tide', src, str(tmp_path), '--correct_minor'])
    with pytest.raises(NotImplementedError, match='EPSG code 27200'):
        cli.main(['06_compensate_tide', src, str(tmp_path), '--crs_src', 'epsg:27200'])
    assert os.listdir(tmp_path) == ['line.sgy']


# ---- the oracle, the conversions, the auxiliary file ---------------------------------------------------------------------------------
def test_helper_oracle_against_mpmath():
    lon, lat, t, terms = (G[f'pred/{k}'] for k in ('lon', 'lat', 't', 'terms'))
    names = tuple(str(c) for c in G['pred/constituents'])
    assert names == H.CONSTITUENTS and terms.shape == (lon.size, 14) and lon.size >= 300
    assert sorted(set(G['pred/ndry'].tolist())) == [0, 1, 2, 3, 4] and t.min() == -220838400.0 and t.max() == 1356998400.0
    lon_z, lat_z, fields, hz = H.model_fields()
    re, im = whole(fields, names)
    got = H.predict(np.mod(lon, 360), lat, t, re, im, hz > 0, lon_z[0], 5.0, -90.0, 5.0, names, periodic=True, parts=True)
    assert np.array_equal(np.isnan(got), np.isnan(terms)) and np.isnan(terms[G['pred/ndry'] == 4]).all()
    worst = np.nanmax(np.abs(got.sum(axis=1) - terms.sum(axis=1)))
    print('helper against mpmath:', worst)
    assert worst <= TOL_M and np.nanmax(np.abs(got - terms)) <= TOL_M


def test_conversions_are_the_reference():
    depth = G['conv/depth']
    assert np.array_equal(U.depth2twt(depth), G['conv/depth2twt']) and np.array_equal(U.depth2twt(depth, v=1480), G['conv/depth2twt_v1480'])
    for units in ('s', 'ms', 'ns'):
        dt = float(G[f'conv/dt/{units}'])
        assert np.array_equal(U.depth2samples(depth, dt, units=units), G[f'conv/depth2samples/{units}'])
        assert np.array_equal(U.depth2samples(depth, dt, v=1480, units=units), G[f'conv/depth2samples_v1480/{units}'])
        assert np.array_equal(U.twt2samples(depth / 700, dt, units=units), G[f'conv/twt2samples/{units}'])


def test_tid_lines():
    times = np.array(['2024-03-01T10:20:30', '2024-03-01T10:20:31', '2024-03-01T10:20:32'], 'datetime64[s]')
    tides = np.array([0.75, -0.0123456789, -0.01])
    lines = cli.aux_lines([1, 2, 3], [11, 12, 13], [101, 102, 103], times, tides, 0.05)
    assert cli.AUX_HEADER == 'tracl,tracr,fldr,time,tide_m,tide_ms,tide_samples\n'
    assert lines == ['1,11,101,2024-03-01T10:20:30,0.750000,1.000,20\n', '2,12,102,2024-03-01T10:20:31,-0.012346,-0.016,-0\n',
                     '3,13,103,2024-03-01T10:20:32,-0.010000,-0.013,-0\n']
