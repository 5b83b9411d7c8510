"""numpy model of the optical-property maps (csrc/optical.hip) and the inputs of their tests.

The anchor is fp64 throughout; the per-bin values are f32 numpy operations in the operation order of
oracle/thz_oracle.c:754-774 (numpy rounds every f32 array operation once, like the C code built without contraction);
only the logarithm is another one than libm's: numpy's fp64 log rounded to f32."""
import numpy as np

EPS = 2.0 ** -23
C_LIGHT = np.float32(2.99792458e8)
PI_F = np.float32(3.14159274101257324219)
TWO_PI = 2.0 * np.pi
MAX_BANDS = 8


def anchor(P, Pr, a0, a1):
    """per pixel of P (npix, nf) f32 against the reference phases Pr (nf) f32 over the bins [a0, a1):
    -> (m int32, w f32 = (float)(m 2 pi), s64: the line's slope in rad / bin, b64: the line at bin 0)"""
    npix = P.shape[0]
    if a0 == a1:
        return np.zeros(npix, np.int32), np.zeros(npix, np.float32), np.zeros(npix), np.zeros(npix)
    na = a1 - a0
    centre = a0 + 0.5 * (na - 1)
    kc = np.arange(a0, a1, dtype=np.float64) - centre
    delta = P[:, a0:a1].astype(np.float64) - Pr[a0:a1].astype(np.float64)
    with np.errstate(all="ignore"):
        s = (delta * kc).sum(axis=1) / (na * (na * na - 1.0) / 12.0)
        b = delta.sum(axis=1) / na - s * centre
        m = np.where(np.isfinite(b), np.rint(b / TWO_PI), 0.0) + 0.0      # (an integer: -0 is 0)
        w = (m * TWO_PI).astype(np.float32)
    return np.clip(m, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int32), w, s, b


def per_bin(A, P, w, Ar, Pr, f, d):
    """(npix, nf) f32 values of every bin: -> dict(n, alpha, kappa, arg: the logarithm's argument, f_hz).
    w: (npix) f32 from anchor(); d: f32 scalar or (npix) f32"""
    A, P, Ar, Pr, f = (np.asarray(x, np.float32) for x in (A, P, Ar, Pr, f))
    d = np.asarray(d, np.float32)
    d = d[:, None] if d.ndim else d
    one, two, four = np.float32(1.0), np.float32(2.0), np.float32(4.0)
    with np.errstate(all="ignore"):
        f_hz = f * np.float32(1.0e12)
        delta_phi = (P - np.asarray(w, np.float32)[:, None]) - Pr
        omega = (two * PI_F) * f_hz
        n = one + C_LIGHT * delta_phi / (omega * d)
        amp = np.fmax(A, np.float32(1e-12))
        amp_ref = np.fmax(Ar, np.float32(1e-12))
        n_safe = np.fmax(n, np.float32(1e-6))
        np1 = n_safe + one
        arg = (np1 * np1) / (four * n_safe) * amp / amp_ref
        # the correctly rounded f32 logarithm (numpy's own f32 log is up to 4 ulp off near 0.78)
        alpha = (np.float32(-2.0) / d) * np.log(arg.astype(np.float64)).astype(np.float32)
        kappa = kappa_of(alpha, f)
    assert all(x.dtype == np.float32 for x in (n, alpha, kappa, arg))
    return dict(n=n, alpha=alpha, kappa=kappa, arg=arg, f_hz=f_hz)


def kappa_of(alpha, f):
    """the extinction coefficient's own operations on given absorption values"""
    with np.errstate(all="ignore"):
        return np.asarray(alpha, np.float32) * C_LIGHT / ((np.float32(4.0) * PI_F) * (np.asarray(f, np.float32) * np.float32(1.0e12)))


def band_means(v, bands):
    """fp64 means of per-bin values (npix, nf) over the bands -> (n_bands, npix) f64"""
    with np.errstate(all="ignore"):
        return np.stack([v[:, k0:k1].astype(np.float64).mean(axis=1) for k0, k1 in bands])


def ulps(got, want):
    """distance in units of the last place of `want` (f32), inf where only one is finite"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.abs(want))
        dist = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp
    both_nan = np.isnan(got) & np.isnan(want)
    same = (got == want) | both_nan
    return np.where(same, 0.0, np.where(np.isfinite(got) & np.isfinite(want), dist, np.inf))


def make_inputs(npix, nf, anchor_range, seed=0, df_thz=0.01):
    """Spectra the way a scan has them: per pixel a phase lag that grows with the bin (slope 0.05 ... 0.3 rad / bin, a
    refractive index of 1.2 ... 2.4 at 1 mm and 0.01 THz per bin), its own multiple of 2 pi on top (-3 ... 3), 0.05 rad of
    noise; amplitudes in 0.05 ... 1.  -> dict(A, P (npix, nf), Ar, Pr, f (nf), m (npix) planted, d_img (npix), d).
    Guaranteed (asserted here on the model, so conditions of the GPU tests and not measurements): with the anchor
    `anchor_range` every pixel's line at bin 0 is finite and b / 2 pi lies at least 1e-3 from a half-integer, so the
    count m survives fp64 sums taken in another order — and equals the planted one."""
    rng = np.random.default_rng([seed, npix, nf])
    k = np.arange(nf, dtype=np.float64)
    f = (k * df_thz).astype(np.float32)
    Pr = (-0.3 * k + 0.2 * rng.standard_normal(nf)).astype(np.float32)
    Ar = (0.2 + rng.random(nf)).astype(np.float32)
    m = rng.integers(-3, 4, npix)
    slope = 0.05 + 0.25 * rng.random(npix)
    delta = TWO_PI * m[:, None] + slope[:, None] * k[None, :] + 0.05 * rng.standard_normal((npix, nf))
    P = (Pr.astype(np.float64)[None, :] + delta).astype(np.float32)
    A = (Ar[None, :] * (0.05 + 0.95 * rng.random((npix, nf)))).astype(np.float32)
    d_img = (1e-3 * (0.5 + rng.random(npix))).astype(np.float32)
    a0, a1 = anchor_range
    if a0 != a1:
        got_m, _, _, b = anchor(P, Pr, a0, a1)
        assert np.all(np.isfinite(b))
        frac = np.abs(b / TWO_PI - np.floor(b / TWO_PI) - 0.5)
        assert frac.min() >= 1e-3, frac.min()
        assert np.array_equal(got_m, m)
    return dict(A=A, P=P, Ar=Ar, Pr=Pr, f=f, m=m.astype(np.int32), d_img=d_img, d=np.float32(1e-3))


def delayed_pulse_cube(nx, ny, nt, seed=0):
    """A scan of one pulse through a sample of varying optical thickness: every trace is the noise-free reference pulse,
    delayed by a whole number of samples that varies over the grid (a plane from about -40 to +40 plus a few samples of
    scatter), scaled by 0.5 ... 1, plus 1 % noise.  -> (time, cube (nx, ny, nt) f32, pulse (nt) f32, delay (nx, ny) int)"""
    rng = np.random.default_rng([seed, nx, ny, nt])
    dt = 0.05
    time = (np.float32(1000.0) + np.float32(dt) * np.arange(nt, dtype=np.float32)).astype(np.float32)
    tau, centre = 0.35, 100   # early in the trace: the phase turns by 0.63 rad per bin, far from the unwrap's pi

    def pulse(shift):
        z = (np.arange(nt, dtype=np.float64)[None, :] - centre - np.asarray(shift, np.float64).reshape(-1, 1)) * dt / tau
        return -z * np.exp(-z * z)

    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    delay = np.rint(-40.0 + 80.0 * (i * ny + j) / (nx * ny - 1)).astype(np.int64) + rng.integers(-3, 4, (nx, ny))
    scale = 0.5 + 0.5 * rng.random((nx, ny))
    cube = scale[..., None] * pulse(delay.ravel()).reshape(nx, ny, nt) + 0.01 * rng.standard_normal((nx, ny, nt))
    return time, cube.astype(np.float32), pulse(0)[0].astype(np.float32), delay


def delay_samples(slope, nt):
    """the pixel's delay against the reference in samples, from the anchor's slope (rad / bin): bin k of an nt-point
    transform turns by -2 pi k D / nt for a delay of D samples"""
    return -np.asarray(slope, np.float64) * nt / TWO_PI
