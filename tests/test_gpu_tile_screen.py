"""The column pass's empty-tile screen (col_kernel<1024, 8, COL_ITER*>: a tile that a bound taken after the first pass of its transform proves
empty ends there, p3d_tile_screen.hpp) against the same pass without it (P3D_NO_TILE_SCREEN=1), bit for bit: result cube, iteration counts,
cost sums and the share of kept column blocks.  nil = nxl = 1024, the smallest shape that runs these kernels (128 tiles per slice).

P3D_TILE_SCREEN_COUNT=1 makes the library print how many tiles of every iteration the screen ended; the tests read it to know that the
screen was at work where it should be (and idle where every tile is kept), so that "the same with and without" is not vacuous."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NIL = NXL = 1024
_data = {}


def _recipe(n):
    """(mask, complex64 cube) of the bench recipe: the plane-wave slices of oracle.synthetic_slice, 80 % of the traces missing.  Computed once."""
    if "mask" not in _data:
        from oracle import pocs_oracle as orc
        _data["mask"] = orc.synthetic_mask(NIL, NXL, 0.8)
        _data["slices"] = {}
    from oracle import pocs_oracle as orc
    for s in range(n):
        if s not in _data["slices"]:
            _data["slices"][s] = (orc.synthetic_slice(NIL, NXL, 900 + s) * _data["mask"]).astype(np.complex64)
    cube = np.stack([_data["slices"][s] for s in range(n)])
    cube.setflags(write=False)
    return _data["mask"], cube


def _run(cube, mask, max_slices, niter, op="hard", eps=0.0, model="exponential", p_min=1e-3, tau=None, active=None):
    from pseudo_3d_interpolation_amd import _ffi as ffi
    from pseudo_3d_interpolation_amd.functions.POCS import _schedule_from_stats
    n = cube.shape[0]
    dtype = ffi.P3D_F32 if cube.dtype == np.float32 else ffi.P3D_C64
    maskf = mask.astype(np.float32)
    with ffi.Plan(NIL, NXL, max_slices) as plan:
        x, o, m = plan.alloc(cube.nbytes).upload(cube), plan.alloc(cube.nbytes), plan.alloc(maskf.nbytes).upload(maskf)
        st = plan.prime_dev(x.ptr, dtype, m.ptr, n)
        if tau is None:
            tau = _schedule_from_stats(st, NIL * NXL, model, niter, 0.99, p_min, "values")
        done, sums, _ = plan.run_dev(x.ptr, dtype, m.ptr, tau, niter, o.ptr, n, thresh_op=op, eps=eps, primed=True, want_sums=True, active=active)
        got = o.download(cube.shape, cube.dtype)
        frac = plan.last_sparsity()
        for b in (x, o, m):
            b.free()
    return got, np.asarray(done).copy(), np.asarray(sums).copy(), frac, st


def _both(monkeypatch, capfd, cube, mask, max_slices, niter, **kw):
    """The job with the screen off and on; asserts that nothing differs.  Returns (the run with the screen on, tiles the screen ended per
    iteration, tiles per iteration)."""
    monkeypatch.setenv("P3D_TILE_SCREEN_COUNT", "1")
    monkeypatch.setenv("P3D_NO_TILE_SCREEN", "1")
    capfd.readouterr()
    ref = _run(cube, mask, max_slices, niter, **kw)
    assert "p3d tile screen" not in capfd.readouterr().err      # switched off: not even counted
    monkeypatch.delenv("P3D_NO_TILE_SCREEN")
    got = _run(cube, mask, max_slices, niter, **kw)
    lines = re.findall(r"p3d tile screen: iteration (\d+): (\d+) of (\d+) tiles", capfd.readouterr().err)
    screened = [int(c) for _, c, _ in lines]
    total = int(lines[0][2]) if lines else 0
    print("kept blocks", got[3], "screened per iteration", screened, "of", total, "done", got[1].tolist())
    assert np.array_equal(got[1], ref[1])                                        # done
    assert np.array_equal(got[2].view(np.uint8), ref[2].view(np.uint8))          # sums
    assert got[3] == ref[3]                                                      # last_sparsity(): a count of the tile flags
    assert np.array_equal(got[0].view(np.uint8), ref[0].view(np.uint8))          # out
    return got, screened, total


@pytest.mark.parametrize("nslices", [3, 9])
def test_bench_recipe_slices(nslices, monkeypatch, capfd):
    mask, cube = _recipe(nslices)
    got, screened, total = _both(monkeypatch, capfd, cube, mask, nslices + 2, 8)
    assert total == nslices * 128 and len(screened) == 8
    assert 0.0 < got[3] < 1.0                       # tiles that keep something and tiles that do not
    # the first threshold is 0.99 of the largest coefficient: six plane waves per slice, everything else far below it -- nearly every tile is
    # emptied and the bound settles it; the last thresholds lie under the noise floor, where no tile is emptied any more
    assert screened[0] > 0.5 * total
    # never more than the threshold empties: kept blocks (a block is a tile here) + screened tiles <= all tiles, summed over the 8 iterations
    assert sum(screened) <= round((1.0 - got[3]) * 8 * total)


def test_first_threshold_is_the_largest_modulus(monkeypatch, capfd):
    """The inverse-proportional model starts AT max |X|: that coefficient must be kept, so its tile must not be screened away."""
    mask, cube = _recipe(3)
    got, screened, total = _both(monkeypatch, capfd, cube, mask, 3, 8, model="inverse_proportional")
    assert got[3] > 0.0 and screened[0] > 0


def test_a_slice_of_noise_keeps_every_tile(monkeypatch, capfd):
    rng = np.random.default_rng(77)
    cube = (rng.standard_normal((1, NIL, NXL)) + 1j * rng.standard_normal((1, NIL, NXL))).astype(np.complex64)
    mask = np.ones((NIL, NXL))
    # |X| of white noise is Rayleigh around sqrt(2 * 1024 * 1024) ~ 1450: each tile of 8192 coefficients holds thousands above 1000
    tau = np.full((1, 4), 1000.0)
    got, screened, total = _both(monkeypatch, capfd, cube, mask, 1, 4, tau=tau)
    assert got[3] == 1.0 and screened == [0, 0, 0, 0] and total == 128


def test_an_all_zero_slice_switched_off(monkeypatch, capfd):
    mask, cube = _recipe(3)
    cube = cube.copy()
    cube[1] = 0
    got, screened, total = _both(monkeypatch, capfd, cube, mask, 3, 8, active=[1, 0, 1])
    assert not got[0][1].any() and screened[0] > 0
    assert max(screened) <= 2 * 128                 # the slice that is off is not looked at


def test_early_exit(monkeypatch, capfd):
    mask, cube = _recipe(3)
    # (the oracle's costs of these slices fall below 1e-2 at the fifth, sixth and fifth iteration)
    got, screened, total = _both(monkeypatch, capfd, cube, mask, 5, 10, eps=1e-2, p_min=1e-2)
    assert max(got[1]) < 10 and len(set(got[1].tolist())) > 1, got[1]     # the early exit switched the slices off mid-job, not all at once
    assert screened[0] > 0


@pytest.mark.parametrize("op", ["soft", "garrote"])
def test_soft_and_garrote(op, monkeypatch, capfd):
    mask, cube = _recipe(3)
    got, screened, total = _both(monkeypatch, capfd, cube, mask, 3, 8, op=op)
    assert 0.0 < got[3] < 1.0 and screened[0] > 0


def test_float32_cube(monkeypatch, capfd):
    """A float32 cube takes the row-pair passes and the half spectrum (513 columns: 65 tiles, the last one a single column wide)."""
    mask, cube = _recipe(3)
    real = np.ascontiguousarray(cube.real)
    got, screened, total = _both(monkeypatch, capfd, real, mask, 3, 8)
    assert got[0].dtype == np.float32 and 0.0 < got[3] < 1.0
    assert total == 3 * 65 and screened[0] > 0      # the half spectrum goes through the same column kernel: the screen is at work there too
