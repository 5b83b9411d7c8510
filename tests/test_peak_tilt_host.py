"""thz_host_arrival_plane_fit (csrc/tilt_fit_host.cpp): the plane through the arrival times from its ten moments.
No GPU: the moments are built in numpy from planted planes."""
import numpy as np
import pytest

import peak_tilt_model as model
import thz_image_explorer_amd as pkg


def _moments(u, v, t):
    return np.array([u.size, u.sum(), v.sum(), (u * u).sum(), (u * v).sum(), (v * v).sum(), t.sum(), (u * t).sum(),
                     (v * t).sum(), (t * t).sum()], np.float64)


def _grid(nx, ny, dx, dy):
    U, V = model.plane_coords(nx, ny, dx, dy)
    return U.ravel().copy(), V.ravel().copy()


@pytest.mark.parametrize("nx,ny,dx,dy,a,b,t0", [
    (24, 20, 1.0, 1.0, -0.0699, 0.0408, 6.4),       # 1.2 / -0.7 degrees
    (17, 19, 0.5, 0.5, -0.1164, -0.0582, 25.0),     # 2 / 1 degrees
    (33, 16, 0.25, 1.0, 0.1747, -0.0291, 25.6),
    (16, 16, 1.0, 1.0, 0.0, 0.0, 5.0),
    (2, 2, 1.0, 1.0, 0.3, -0.2, 1.0),               # the smallest grid that spans a plane
])
def test_planted_plane_comes_back(nx, ny, dx, dy, a, b, t0):
    u, v = _grid(nx, ny, dx, dy)
    t = t0 + a * u + b * v
    rc, fit = pkg.host_arrival_plane_fit(_moments(u, v, t))
    assert rc == 0 and fit.n_used == nx * ny
    scale = max(abs(a), abs(b), 1e-3)  # the plane of zero slope: against a thousandth of a ps per mm
    assert abs(fit.slope_x_ps_per_mm - a) <= 1e-12 * scale and abs(fit.slope_y_ps_per_mm - b) <= 1e-12 * scale
    assert abs(fit.t0_ps - t0) <= 1e-12 * t0
    assert fit.tilt_x_deg == pytest.approx(np.rad2deg(-fit.slope_x_ps_per_mm * model.C_MM_PER_PS), rel=1e-15, abs=0)
    assert fit.tilt_y_deg == pytest.approx(np.rad2deg(-fit.slope_y_ps_per_mm * model.C_MM_PER_PS), rel=1e-15, abs=0)
    assert fit.rms_ps <= 1e-6      # sqrt of what the cancellation leaves of a zero residual: ~1e-8 ps


def test_noisy_plane_matches_lstsq_on_a_masked_grid():
    rng = np.random.default_rng(5)
    u, v = _grid(17, 19, 0.5, 0.5)
    keep = rng.random(u.size) > 0.3
    u, v = u[keep], v[keep]
    t = 25.0 - 0.1164 * u - 0.0582 * v + 0.01 * rng.standard_normal(u.size)
    rc, fit = pkg.host_arrival_plane_fit(_moments(u, v, t))
    A = np.stack([np.ones_like(u), u, v], 1)
    sol = np.linalg.lstsq(A, t, rcond=None)[0]
    rms = np.sqrt(((t - A @ sol) ** 2).mean())
    assert rc == 0 and fit.n_used == u.size
    assert abs(fit.slope_x_ps_per_mm - sol[1]) <= 1e-12 * abs(sol[1])
    assert abs(fit.slope_y_ps_per_mm - sol[2]) <= 1e-12 * abs(sol[2])
    assert abs(fit.t0_ps - sol[0]) <= 1e-12 * abs(sol[0])
    assert abs(fit.rms_ps - rms) <= 1e-9 * rms


def _skipped(u, v, t):
    rc, fit = pkg.host_arrival_plane_fit(_moments(np.asarray(u, float), np.asarray(v, float), np.asarray(t, float)))
    assert rc == 1
    assert fit.as_tuple() == (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0)


def test_degenerate_inputs_are_skipped_with_zeros():
    _skipped([0.0, 1.0], [0.0, 1.0], [1.0, 2.0])                                # two pixels
    _skipped([], [], [])                                                         # none
    u, v = _grid(1, 19, 0.5, 0.5)
    _skipped(u, v, 3.0 + 0.1 * v)                                                # one row
    u, v = _grid(17, 1, 0.5, 0.5)
    _skipped(u, v, 3.0 + 0.1 * u)                                                # one column
    d = np.arange(12.0) - 5.5
    _skipped(0.5 * d, 0.25 * d, 3.0 + 0.1 * d)                                   # a diagonal line
    _skipped(0.3 * d + 1.0, 0.7 * d - 2.0, 3.0 + 0.1 * d)                        # a line off the centre
    _skipped([0.0, 1.0, 2.0], [np.nan, 0.0, 1.0], [1.0, 2.0, 3.0])               # a moment that is no number


def test_null_pointers_are_refused():
    lib = pkg.load_library()
    assert lib.thz_host_arrival_plane_fit(None, None) == -1
