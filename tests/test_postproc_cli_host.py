"""Step 15 (15_cube_postprocessing) on the CPU: the command line, the mutual-exclusion rule, the AGC window bookkeeping against the
reference's numbers (tests/golden/agc.npz, tests/golden/make_golden_agc.py), the upsampling grid / metadata / file name, and the
installed console script.  Nothing here touches a GPU."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

FLAGS = ["path_cube", "--path_out", "--upsample", "--spatial-dealiasing", "--remove-footprint", "--direction", "--footprint-sigma",
         "--buffer-center", "--buffer-filter", "--smooth", "--smooth-sigma", "--smooth-size", "--rescale", "--agc", "--agc-win", "--agc-kind",
         "--agc-sqrt", "--verbose"]


def test_help_lists_every_flag_of_the_reference():
    res = subprocess.run([sys.executable, "-m", "pseudo_3d_interpolation_amd.cube_postprocessing_3D", "--help"], cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    for flag in FLAGS:
        assert flag in res.stdout, flag
    for choice in ("linear", "nearest", "slinear", "cubic", "polynomial", "profile-iline", "profile-xline", "gaussian", "median", "rms", "mean"):
        assert choice in res.stdout, choice


def test_parser_defaults_match_the_reference():
    from pseudo_3d_interpolation_amd import cube_postprocessing_3D as pp
    a = pp.define_input_args().parse_args(["c.nc"])
    assert (a.path_out, a.upsample, a.spatial_dealiasing, a.remove_footprint, a.direction) == (None, None, False, None, None)
    assert (a.footprint_sigma, a.buffer_center, a.buffer_filter, a.smooth, a.smooth_sigma, a.smooth_size) == (7, 0.20, 3, None, 1, 3)
    assert (a.rescale, a.agc, a.agc_win, a.agc_kind, a.agc_sqrt, a.verbose) == (None, False, None, "rms", False, 0)
    b = pp.define_input_args().parse_args(["c.nc", "--upsample", "--remove-footprint", "--rescale", "--verbose"])
    assert (b.upsample, b.remove_footprint, b.rescale, b.verbose) == ("linear", "slice", [], 1)


@pytest.mark.parametrize("extra", [["--agc", "--upsample"], ["--agc", "--smooth", "gaussian"], ["--agc", "--remove-footprint", "slice"],
                                   ["--remove-footprint", "profile", "--smooth", "median"], ["--remove-footprint", "profile", "--upsample", "nearest"]])
def test_mutually_exclusive_options_write_nothing(tmp_path, capsys, extra):
    from pseudo_3d_interpolation_amd import cube_postprocessing_3D as pp
    path = tmp_path / "cube_twt.npz"
    path.write_bytes(b"")
    assert pp.main(["15_cube_postprocessing", str(path), "--agc-win", "0.01"] + extra) is None
    assert os.listdir(tmp_path) == ["cube_twt.npz"]
    assert "mutually exclusive" in capsys.readouterr().out


def test_agc_window_and_time_units_match_the_reference():
    from pseudo_3d_interpolation_amd.functions.signal import get_AGC_samples
    from pseudo_3d_interpolation_amd.functions.utils import convert_twt
    g = load_golden("agc.npz")
    for win, dt, units, dt_s, n in zip(g["samples/win"], g["samples/dt"], g["samples/units"], g["samples/dt_s"], g["samples/n"]):
        assert convert_twt(float(dt), str(units), "s") == dt_s
        assert get_AGC_samples(float(win), float(dt_s)) == n, (win, dt, units)
    assert get_AGC_samples(0.01, 1e-4) == 101


def test_agc_rejects_what_the_reference_rejects():
    from pseudo_3d_interpolation_amd.functions.signal import AGC
    x = np.ones((10, 4), np.float32)
    with pytest.raises(TypeError):
        AGC(x, 5.0)
    with pytest.raises(TypeError):
        AGC(x, np.int64(5))
    with pytest.raises(ValueError):
        AGC(x, 5, kind="max")
    with pytest.raises(NotImplementedError):
        AGC(x, 5, pad=False)
    with pytest.raises(NotImplementedError):
        AGC(x, 5, pad_mode="reflect")


def _map_cube(d_il, d_xl, bin_il=1.0, bin_xl=3.0):
    from pseudo_3d_interpolation_amd.cube_io import Cube
    il = 100 + d_il * np.arange(6)
    xl = 7 + d_xl * np.arange(5)
    fold = np.arange(30, dtype=np.float64).reshape(6, 5) ** 1.5
    return Cube({"fold": fold, "trace_t": np.zeros(4, np.float32)}, {"fold": ("iline", "xline"), "trace_t": ("twt",)},
                {"twt": np.arange(4.0), "iline": il, "xline": xl},
                {"bin_size_iline": bin_il, "bin_size_xline": bin_xl, "history": "h;", "text": "t"}, {},
                {"iline": {"bin_il": bin_il}, "xline": {"bin_xl": bin_xl}})


@pytest.mark.parametrize("d_il,d_xl", [(2, 1), (3, 1), (4, 1), (1, 2), (1, 3), (1, 4)])
def test_upsampled_grid_and_metadata(d_il, d_xl):
    from pseudo_3d_interpolation_amd import cube_postprocessing_3D as pp
    cube = _map_cube(d_il, d_xl, bin_il=1.0 * d_xl, bin_xl=1.0 * d_il)
    out, fac = pp.upsample_ilxl(cube, spatial_dealiasing=False, return_factor=True, verbose=0)
    assert fac == {"iline": d_il, "xline": d_xl}
    assert np.array_equal(out.coords["iline"], np.arange(100, 100 + 5 * d_il + 1))
    assert np.array_equal(out.coords["xline"], np.arange(7, 7 + 4 * d_xl + 1))
    assert out.coord_attrs["iline"]["bin_il"] == 1.0 and out.coord_attrs["xline"]["bin_xl"] == 1.0
    assert out.attrs["bin_size_iline"] == 1.0 and out.attrs["bin_size_xline"] == 1.0
    assert cube.coord_attrs["iline"]["bin_il"] == d_xl             # the input is left alone
    f = out.data_vars["fold"]
    assert f.shape == (out.coords["iline"].size, out.coords["xline"].size)
    src = cube.data_vars["fold"]
    assert np.array_equal(f[::d_il, ::d_xl], src)                 # source lines are copies
    if d_il > 1:                                                  # linear weights (j mod d) / d between neighbouring lines
        j = 1
        assert np.allclose(f[j, ::d_xl], (1 - j / d_il) * src[0] + j / d_il * src[1], rtol=1e-12)
    else:
        j = d_xl - 1
        assert np.allclose(f[::d_il, j], (1 - j / d_xl) * src[:, 0] + j / d_xl * src[:, 1], rtol=1e-12)
    near = pp.upsample_ilxl(cube, method="nearest", spatial_dealiasing=False, verbose=0)
    d = max(d_il, d_xl)
    lines = np.arange(near.data_vars["fold"].shape[0 if d_il > 1 else 1])
    pick = np.where(lines % d > d / 2, lines // d + 1, lines // d)  # ties (d = 2, 4) go to the lower line
    want = src[pick] if d_il > 1 else src[:, pick]
    assert np.array_equal(near.data_vars["fold"], want)


def test_upsampling_interp_tables():
    from pseudo_3d_interpolation_amd import cube_postprocessing_3D as pp
    i0, w = pp.interp_table([0, 4, 8], np.arange(9))
    assert list(i0) == [0, 0, 0, 0, 1, 1, 1, 1, 2] and np.allclose(w, [0, .25, .5, .75, 0, .25, .5, .75, 0])
    i0, w = pp.interp_table([0, 2, 4], np.arange(5), "nearest")
    assert list(i0) == [0, 0, 1, 1, 2] and not w.any()
    i0, w = pp.interp_table([0, 3], np.arange(4), "nearest")
    assert list(i0) == [0, 0, 1, 1]


def test_upsampling_errors_and_no_gap():
    from pseudo_3d_interpolation_amd import cube_postprocessing_3D as pp
    for method in ("cubic", "polynomial"):
        with pytest.raises(NotImplementedError, match=method):
            pp.upsample_ilxl(_map_cube(2, 1), method=method, verbose=0)
    cube = _map_cube(2, 1)
    cube.coord_attrs["xline"].pop("bin_xl")
    with pytest.raises(ValueError, match="bin_il"):
        pp.upsample_ilxl(cube, spatial_dealiasing=False, verbose=0)
    same = _map_cube(1, 1)
    out, fac = pp.upsample_ilxl(same, verbose=0)
    assert out is same and fac == {"iline": 1, "xline": 1}


@pytest.mark.parametrize("d_il,d_xl,name,want", [(1, 4, "survey_6x1+5m_twt", "survey_1+5x1+5m_twt_upsampled"),
                                                  (2, 1, "area_5x10m_env", "area_5x5m_env_upsampled"),
                                                  (3, 1, "area_5x7+5m_env", "area_5x2+5m_env_upsampled")])
def test_upsampled_file_name_history_and_text(tmp_path, d_il, d_xl, name, want):
    from pseudo_3d_interpolation_amd import cube_postprocessing_3D as pp
    from pseudo_3d_interpolation_amd.cube_io import open_cube, save_cube
    bil, bxl = [float(v.replace("+", ".")) for v in name.split("_")[1][:-1].split("x")]
    cube = _map_cube(d_il, d_xl, bin_il=bil, bin_xl=bxl)
    path = save_cube(cube, str(tmp_path / f"{name}.npz"))
    pp.main(["15_cube_postprocessing", path, "--upsample"])
    out = open_cube(str(tmp_path / f"{want}.npz"))
    assert out.attrs["history"] == "h;cube_postprocessing_3D: iline/xline bin size upsampling;"
    assert out.attrs["text"].startswith("t\n") and out.attrs["text"].endswith(": UPSAMPLING")
    assert out.data_vars["fold"].shape == (5 * d_il + 1, 4 * d_xl + 1)
    alt = tmp_path / "elsewhere.npz"
    pp.main(["15_cube_postprocessing", path, "--upsample", "nearest", "--path_out", str(alt)])
    assert alt.exists()


@pytest.fixture(scope="module")
def prefix(tmp_path_factory):
    if not os.path.isfile(os.path.join(ROOT, "pseudo-3d-interpolation_amd", "libp3d_hip.so")):
        pytest.skip("libp3d_hip.so not built")
    dest = tmp_path_factory.mktemp("prefix")
    made = [p for p in ("build", "pseudo_3d_interpolation_amd.egg-info") if not os.path.exists(os.path.join(ROOT, p))]
    res = subprocess.run([sys.executable, "-m", "pip", "install", "--no-deps", "--no-build-isolation", "--no-index", "--prefix", str(dest), "."],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    for p in made:
        shutil.rmtree(os.path.join(ROOT, p), ignore_errors=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    site = [os.path.dirname(p) for p in glob.glob(os.path.join(str(dest), "**", "pseudo_3d_interpolation_amd"), recursive=True) if os.path.isdir(p)]
    scripts = glob.glob(os.path.join(str(dest), "**", "15_cube_postprocessing"), recursive=True)
    assert len(site) == 1 and len(scripts) == 1, (site, scripts)
    return dest, site[0], scripts[0]


def test_installed_console_script(prefix):
    dest, site, script = prefix
    res = subprocess.run([script, "--help"], cwd=str(dest), env=dict(os.environ, PYTHONPATH=site), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    for flag in FLAGS:
        assert flag in res.stdout, flag
    assert os.path.isfile(os.path.join(site, "pseudo_3d_interpolation_amd", "functions", "signal.py"))
