"""``02_reproject_segy --help`` from an installed copy (``pip install .`` into a scratch prefix, the fixture of test_packaging.py) lists the
reference's flags."""
import os
import subprocess

from test_packaging import prefix  # noqa: F401  (module-scoped fixture: one installation for this file)

FLAGS = ['input_path', '--crs_src', '--crs_dst', '--output_dir', '-o', '--inplace', '-i', '--filename_suffix', '-fns', '--suffix', '-s', '--txt_suffix',
         '--scalar_coords', '-sc', '{-1000,-100,-10,0,10,100,1000}', '--src_coords', '--dst_coords', '{source,CDP,group}', '--smooth', '--verbose', '-V']


def test_console_script_shows_the_flags_of_the_reference(prefix):  # noqa: F811
    dest, site, bindir = prefix
    res = subprocess.run([os.path.join(bindir, '02_reproject_segy'), '--help'], cwd=str(dest), env=dict(os.environ, PYTHONPATH=site), capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    for flag in FLAGS:
        assert flag in res.stdout, (flag, res.stdout)
    assert os.path.isfile(os.path.join(site, 'pseudo_3d_interpolation_amd', 'functions', 'crs.py'))
