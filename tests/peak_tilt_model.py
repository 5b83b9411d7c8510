"""numpy fp64 model of the arrival-time maps and the arrival-plane fit (include/thzgpu.h, "Pulse arrival times"),
and the planted cubes the tests of the feature share.  Not a test module."""
import numpy as np

C_MM_PER_PS = 0.299792458


def planted_cube(nx, ny, nt, dx, dy, tilt_x_deg, tilt_y_deg, dead=0.0, seed=1, noise=0.01, dt=0.05, tau=0.35):
    """derivative-of-Gaussian pulses (tau ps, step dt ps, `noise` of the unit amplitude) whose arrival plane the two
    angles flatten; a fraction `dead` of the pixels has amplitude 0 -> (time f32, cube f32, u mm, v mm, live mask)"""
    rng = np.random.default_rng(seed)
    t = (1000.0 + dt * np.arange(nt)).astype(np.float32)
    u = (np.arange(nx) - nx / 2) * dx
    v = (np.arange(ny) - ny / 2) * dy
    a, b = -np.deg2rad(tilt_x_deg) / C_MM_PER_PS, -np.deg2rad(tilt_y_deg) / C_MM_PER_PS
    tc = float(t[0]) + nt * dt * 0.5 + a * u[:, None] + b * v[None, :]
    amp = 1.0 + 0.5 * rng.random((nx, ny))
    live = rng.random((nx, ny)) >= dead if dead > 0 else np.ones((nx, ny), bool)
    amp = amp * live
    z = (t[None, None, :].astype(np.float64) - tc[:, :, None]) / tau
    s = amp[:, :, None] * (-z) * np.exp(-z * z) + noise * rng.standard_normal((nx, ny, nt))
    return t, s.astype(np.float32), u, v, live


def mean_step(time):
    t = np.asarray(time, np.float32)
    return (float(t[-1]) - float(t[0])) / (t.size - 1) if t.size > 1 else 0.0


def peak_model(x, mode):
    """x (..., nt) f32 -> index (int64), fp64 parabola offset, value (f32), and the rounding bar of the f32 offset.
    NaNs never win; a trace of NaNs gives index 0; ties go to the lowest index (np.argmax's rule)."""
    x = np.asarray(x, np.float32)
    nt = x.shape[-1]
    x64 = x.astype(np.float64)
    key = {0: np.abs(x64), 1: x64, 2: -x64}[mode]
    key = np.where(np.isnan(key), -np.inf, key)
    first_number = np.argmax(~np.isnan(x64), axis=-1)        # an all -Inf key row: the first number wins, not a NaN
    k = np.where(np.isneginf(key).all(-1), np.where(np.isnan(x64).all(-1), 0, first_number), key.argmax(-1))
    take = lambda idx: np.take_along_axis(x64, idx[..., None], -1)[..., 0]
    y0, ym, yp = take(k), take(np.clip(k - 1, 0, nt - 1)), take(np.clip(k + 1, 0, nt - 1))
    den = ym - 2 * y0 + yp
    ok = (k > 0) & (k < nt - 1) & (den != 0) & np.isfinite(ym) & np.isfinite(y0) & np.isfinite(yp)
    with np.errstate(all="ignore"):
        off = np.where(ok, 0.5 * (ym - yp) / np.where(ok, den, 1.0), 0.0)
        bar = np.where(ok, 8 * np.finfo(np.float32).eps * (np.abs(ym) + 2 * np.abs(y0) + np.abs(yp)) / np.abs(np.where(ok, den, 1.0)), 0.0)
    value = np.take_along_axis(x, k[..., None], -1)[..., 0]
    return k, np.clip(off, -0.5, 0.5), value, bar, ok


def plane_mask(value, rel_threshold):
    a = np.abs(np.asarray(value, np.float32))
    fin = np.isfinite(a)
    vmax = a[fin].max() if fin.any() else np.float32(0)
    return fin & (a >= np.float32(rel_threshold) * vmax)     # f32 product, f32 compare


def plane_coords(nx, ny, dx, dy):
    u = (np.arange(nx) - nx / 2) * float(np.float32(dx))
    v = (np.arange(ny) - ny / 2) * float(np.float32(dy))
    return np.broadcast_to(u[:, None], (nx, ny)), np.broadcast_to(v[None, :], (nx, ny))


def plane_moments(index, offset, value, dx, dy, dt_ps, rel_threshold):
    nx, ny = index.shape
    w = plane_mask(value, rel_threshold)
    U, V = plane_coords(nx, ny, dx, dy)
    u, v = U[w], V[w]
    t = (index[w].astype(np.float64) + offset[w].astype(np.float64)) * dt_ps
    return np.array([w.sum(), u.sum(), v.sum(), (u * u).sum(), (u * v).sum(), (v * v).sum(), t.sum(), (u * t).sum(),
                     (v * t).sum(), (t * t).sum()], np.float64)


def plane_lstsq(index, offset, value, dx, dy, dt_ps, rel_threshold):
    """least squares plane through the participating pixels -> dict like thz_tilt_fit"""
    nx, ny = index.shape
    w = plane_mask(value, rel_threshold)
    U, V = plane_coords(nx, ny, dx, dy)
    u, v = U[w], V[w]
    t = (index[w].astype(np.float64) + offset[w].astype(np.float64)) * dt_ps
    A = np.stack([np.ones_like(u), u, v], 1)
    sol = np.linalg.lstsq(A, t, rcond=None)[0]
    res = t - A @ sol
    return dict(t0_ps=sol[0], slope_x_ps_per_mm=sol[1], slope_y_ps_per_mm=sol[2], n_used=int(w.sum()),
                rms_ps=float(np.sqrt((res * res).mean())), tilt_x_deg=float(np.rad2deg(-sol[1] * C_MM_PER_PS)),
                tilt_y_deg=float(np.rad2deg(-sol[2] * C_MM_PER_PS)), half_width=max(np.abs(u).max(), np.abs(v).max()))


def edge_delay_samples(dtheta_x_deg, dtheta_y_deg, u, v, dt=0.05):
    """an angle error as delay at the grid's edge, in samples of dt"""
    return max(abs(np.deg2rad(dtheta_x_deg)) * np.abs(u).max(), abs(np.deg2rad(dtheta_y_deg)) * np.abs(v).max()) / C_MM_PER_PS / dt
