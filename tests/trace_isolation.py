"""Per-trace error bars for the FFT kernels that pack two real traces into one complex transform (the P kernels,
fft_p.hpp, and the chirp-z kernels, fft_fb.hpp).  Each trace is held to its OWN scale: a bar relative to the largest
value of the whole cube lets a dark pixel be wrong by as much as its bright partner's rounding noise.

References are numpy float64 transforms of the same f32 inputs (not the f32 oracle).  Shared by
test_emu_kernels.py (the emulation) and test_gpu_trace_isolation.py (the device)."""
import numpy as np

import synth

TRACE_TOL = 1e-5   # max |dev - ref64| / max |ref64|, per trace

# per-trace factors on synthetic traces: (strong, weak) and (weak, strong) pairs, zero traces next to a live one and next
# to each other, a NaN and an Inf sample next to a clean trace, and an odd count (the last pair has one trace)
RATIOS = (1.0, 1e2, 1e3, 1e4, 1e6)
FACTORS = [f for r in RATIOS for f in ((1.0, 1.0 / r), (1.0 / r, 1.0))]
FACTORS = [x for pair in FACTORS for x in pair] + [1.0, 0.0, 0.0, 1.0, 0.0, 0.0, "nan", 1.0, 1.0, "inf", 1.0]
ZERO_LIVE = (21, 22)     # zero traces whose partner is live
ZERO_ZERO = (24, 25)     # a pair of zero traces
BAD = (26, 29)           # the NaN and the Inf trace
CLEAN_NEXT_TO_BAD = (27, 28)


def make_cube(nt, factors=FACTORS, first_id=41):
    """(len(factors), nt) f32: synthetic traces (bias subtracted, io.rs:578-586) times their factor; "nan" / "inf"
    put one non-finite sample into a unit-scale trace"""
    n = len(factors)
    x = synth.make_traces(np.arange(n) + first_id, max(nt, 320))[:, :nt].astype(np.float32)
    for i, f in enumerate(factors):
        if f == "nan":
            x[i, nt // 3] = np.nan
        elif f == "inf":
            x[i, nt // 2] = -np.inf
        else:
            x[i] *= np.float32(f)
    return np.ascontiguousarray(x, np.float32)


def status(factors=FACTORS):
    """per trace: 'live', 'zero' or 'bad'"""
    return ["bad" if f in ("nan", "inf") else ("zero" if f == 0.0 else "live") for f in factors]


def numpy_unwrap(raw):
    """the reference's numpy_unwrap (math_tools.rs:211-240) in float64, along the last axis"""
    d = np.diff(raw, axis=-1)
    d = np.where(d > np.pi, d - 2 * np.pi, np.where(d < -np.pi, d + 2 * np.pi, d))
    return np.concatenate([raw[..., :1], raw[..., :1] + np.cumsum(d, axis=-1)], axis=-1)


def forward_ref(x, pre, mask, cmask=None):
    """float64 spectra of f32 traces: X = rfft(x pre); stored spectrum Y = X mask (H), with a real DC / Nyquist bin when
    H is given; amplitudes |X mask (H)|; unwrapped phases of X"""
    nt = x.shape[-1]
    with np.errstate(invalid="ignore"):   # the NaN / Inf traces
        return _forward_ref(x, pre, mask, cmask, nt)


def _forward_ref(x, pre, mask, cmask, nt):
    X = np.fft.rfft(x.astype(np.float64) * (1.0 if pre is None else pre.astype(np.float64)), axis=-1)
    m = np.ones(X.shape[-1]) if mask is None else mask.astype(np.float64)
    Y = X * m
    if cmask is not None:
        Y = Y * (cmask[:, 0].astype(np.float64) + 1j * cmask[:, 1])
    amp = np.abs(Y)
    if cmask is not None:
        Y[:, 0] = Y[:, 0].real
        if nt % 2 == 0:
            Y[:, -1] = Y[:, -1].real
    return dict(X=X, fft=Y, amp=amp, ph=numpy_unwrap(np.angle(X)))


def inverse_ref(Y, nt, post):
    """float64 C2R of spectra (imaginary parts of DC / Nyquist ignored, as realfft does) times the post window, and
    the intensity sum y^2"""
    Y = np.array(Y, np.complex128)
    Y[:, 0] = Y[:, 0].real
    if nt % 2 == 0:
        Y[:, -1] = Y[:, -1].real
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.fft.irfft(Y, n=nt, axis=-1) * (1.0 if post is None else post.astype(np.float64))
        return y, (y ** 2).sum(-1)


def as_complex(f):
    f = np.asarray(f)
    return f[..., 0].astype(np.float64) + 1j * f[..., 1].astype(np.float64)


def trace_errors(dev, ref):
    """max |dev - ref| / max |ref| of every trace (last axis); inf where the reference is zero and dev is not"""
    dev = np.asarray(dev)
    dev = dev.astype(np.complex128) if np.iscomplexobj(dev) else dev.astype(np.float64)
    with np.errstate(invalid="ignore"):
        num = np.abs(dev - ref).max(axis=-1)
    den = np.abs(ref).max(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num == 0, 0.0, np.inf))


def check(name, got, ref, st, tol=TRACE_TOL):
    """live traces within tol of their own scale; zero traces exactly zero; returns a list of failure strings"""
    bad = []
    got = np.asarray(got)
    errs = trace_errors(got, ref)
    for i, s in enumerate(st):
        if s == "live":
            if not np.all(np.isfinite(got[i])):
                bad.append(f"{name}[{i}] not finite")
            elif not errs[i] < tol:
                bad.append(f"{name}[{i}] {errs[i]:.2e}")
        elif s == "zero" and not np.all(got[i] == 0):
            bad.append(f"{name}[{i}] not exactly zero (max {np.abs(got[i]).max():.2e})")
    return bad


def check_intensity(img, ref_img, st, tol=TRACE_TOL):
    bad = []
    for i, s in enumerate(st):
        if s == "live" and not abs(float(img[i]) - ref_img[i]) <= tol * ref_img[i]:
            bad.append(f"img[{i}] {abs(float(img[i]) - ref_img[i]) / ref_img[i]:.2e}")
        elif s == "zero" and img[i] != 0:
            bad.append(f"img[{i}] = {img[i]:.2e}, not zero")
        elif s == "bad" and np.isfinite(img[i]):
            bad.append(f"img[{i}] of a non-finite trace is finite")
    return bad


def check_phases(ph, ref, st, factors=FACTORS, tol=TRACE_TOL):
    """unwrapped phases of live traces with phase_parity at the per-trace spectrum bar (it scales by each trace's own
    max |X|); zero traces: bit-identical whether the partner is live or zero"""
    from test_gpu_parity import phase_parity
    bad = []
    live = [i for i, s in enumerate(st) if s == "live"]
    Xf = np.stack([ref["X"].real, ref["X"].imag], -1)
    ok, msg = phase_parity(np.asarray(ph)[live], ref["ph"][live], Xf[live], spectrum_tol=tol)
    if not ok:
        bad.append("phases: " + msg)
    if factors is FACTORS:
        bits = np.ascontiguousarray(np.asarray(ph, np.float32)).view(np.uint32)
        for i in ZERO_LIVE:
            if not np.array_equal(bits[i], bits[ZERO_ZERO[0]]):
                bad.append(f"phases of zero trace {i} depend on its partner")
    return bad
