"""Developer tool: unmixing on a resident recompute — thz_unmix on the amplitude bins 1 .. 500 at
K = 4 and K = 16 endmembers and 64 and 256 sweeps, alternating in one process with thz_pca_scores (K = 8) over the same
matrix: the yardstick of the two passes that read the cube, which move the same bytes.  The stage timer (hipEvent pairs)
stands around all the launches of a call, so the three launches are separated by what each call leaves out:
    projection   a call without a residual and with no sweep (its solve launch only copies zeros: it is in the figure)
    solve        the call with n sweeps and no residual, minus the one above
    residual     the whole call, minus the call without a residual
each the difference of medians of calls that alternate round by round.  Then the accuracy of the device's logf (the
absorbance mode with one column, one endmember 1 and the reference 1 returns -logf(X) itself), and, once, the host route
the call replaces: the download of the amplitudes and scipy.optimize.nnls over the rows.  Nothing here is a bar.

    python scripts/gpu_unmix_timing.py [--rounds 20] [--out profiles/unmix_timing.txt] [--no-host] [nx ny nt]
"""
import argparse
import os
import sys
import time as clock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import synth  # noqa: E402
import thz_image_explorer_amd as pkg  # noqa: E402


def logf_accuracy(eng, n=1 << 20):
    """-> (largest error in ulp of the result, the x it was found at) of the device's logf over n values"""
    rng = np.random.default_rng(1)
    x = np.exp(rng.uniform(np.log(1e-6), np.log(1e3), n)).astype(np.float32)
    x[:4096] = np.linspace(0.5, 2.0, 4096, dtype=np.float32)          # around 1, where log is small against its argument
    d_x, d_a, d_b = eng.to_device(x), eng.empty(n), eng.empty(n)
    one = np.ones((1, 1), np.float32)
    eng.unmix(n, 1, d_x, 1, 1, one, d_a, 0, ref=one.ravel(), proj=d_b)
    got = -d_b.download((n,), np.float32).astype(np.float64)
    want = np.log(x.astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want) / ulp
    return float(err.max()), float(x[int(err.argmax())])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="leave the scipy route out")
    ap.add_argument("shape", nargs="*", type=int, default=[512, 512, 1001])
    a = ap.parse_args()
    nx, ny, nt = a.shape[:3]
    npix = nx * ny
    tm = synth.make_time(nt)
    nf = nt // 2 + 1
    first, count = 1, min(nf - 1, 500, pkg.PCA_MAX_LEN)
    rng = np.random.default_rng(0)
    t = {}
    with pkg.Engine(0) as eng:
        eng.set_time_axis(tm)
        sess = pkg.Session(eng, nx, ny, tm)
        d_t = eng.to_device(tm)
        eng.synth_cube(eng.lib.thz_session_buffer(sess.h, pkg.BUF_RAW), npix, 0, d_t)
        sess.upload(None)
        sess.recompute(pkg.chain_cfg_default(tm))
        d_amp = eng.lib.thz_session_buffer(sess.h, pkg.BUF_AMPLITUDES) + 4 * first
        d_scores = eng.empty((8, npix))
        d_abund, d_proj, d_resid, d_kkt = eng.empty((16, npix)), eng.empty((16, npix)), eng.empty(npix), eng.empty(npix)
        comps = rng.standard_normal((8, count)).astype(np.float32)
        ends = {}
        eng.enable_timing(1)
        try:
            for k in (4, 16):
                pick = pkg.cluster_cfg(first, count, 1, 1, init=0)
                e = np.stack([sess.cluster_row(pkg.BUF_AMPLITUDES, pick, int(p)) for p in rng.integers(0, npix, k)])
                ends[k] = e
                for sweeps in (64, 256):
                    calls = {"projection": dict(n_sweeps=0, proj=d_proj), "no residual": dict(n_sweeps=sweeps, proj=d_proj, kkt=d_kkt),
                             "whole call": dict(n_sweeps=sweeps, proj=d_proj, kkt=d_kkt, resid=d_resid)}
                    names = [f"K={k} {sweeps} sweeps: {c}" for c in calls] + [f"K={k} {sweeps} sweeps: K=8 scores", f"K={k} {sweeps} sweeps: whole call (host)"]
                    for name in names:
                        t[name] = []
                    for r in range(3 + a.rounds):
                        row = []
                        for kw in calls.values():
                            t0 = clock.perf_counter()
                            eng.unmix(npix, count, d_amp, nf, 1, e, d_abund, **kw)
                            eng.sync()
                            host_us = (clock.perf_counter() - t0) * 1e6
                            row.append(eng.stage_time_ns(pkg.STAGE_PCA) * 1e-3)
                        eng.pca_scores(npix, count, d_amp, nf, 1, None, comps, d_scores)
                        eng.sync()
                        row += [eng.stage_time_ns(pkg.STAGE_PCA) * 1e-3, host_us]
                        if r >= 3:
                            for name, v in zip(names, row):
                                t[name].append(v)
        finally:
            eng.enable_timing(0)
        ulp, at = logf_accuracy(eng)
        host = ""
        if not a.no_host:
            from scipy.optimize import nnls
            eng.unmix(npix, count, d_amp, nf, 1, ends[4], d_abund, 256)
            dev = d_abund.download((16, npix), np.float32)[:4].T
            t0 = clock.perf_counter()
            amp = sess.download(pkg.BUF_AMPLITUDES).reshape(npix, -1)
            t_down = clock.perf_counter() - t0
            x = amp[:, first:first + count].astype(np.float64)
            basis = ends[4].astype(np.float64).T.copy()
            t0 = clock.perf_counter()
            ref = np.stack([nnls(basis, row)[0] for row in x])
            t_nnls = clock.perf_counter() - t0
            worst = float((np.abs(dev - ref).max(axis=1) / np.maximum(ref.max(axis=1), 1e-30)).max())
            host = (f"host route, once, K = 4: download of the amplitudes {t_down * 1e3:.0f} ms ({amp.nbytes / 1e6:.0f} MB) + scipy.optimize.nnls over "
                    f"{npix} rows {t_nnls:.1f} s; the device's abundances after 256 sweeps differ from it by at most {worst:.3g} of the pixel's largest "
                    f"(cond(G) = {np.linalg.cond(basis.T @ basis):.3g}: rows of one synthetic scan are nearly parallel)")
        sess.close()
    nbytes = 4.0 * npix * count
    med = {name: float(np.median(v)) for name, v in t.items()}
    lines = [f"unmixing of the resident amplitudes, {nx} x {ny} x {nt}, bins {first} .. {first + count - 1} ({count}): {nbytes / 1e6:.0f} MB per pass; "
             f"{a.rounds} rounds after 3 warm-up, the calls alternating round by round; us",
             f"{'what':>40s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    for name, v in t.items():
        v = np.array(v)
        lines.append(f"{name:>40s} {np.median(v):10.1f} {v.min():10.1f} {v.max():10.1f}")
    for k in (4, 16):
        for sweeps in (64, 256):
            tag = f"K={k} {sweeps} sweeps: "
            p, s, w, y = med[tag + "projection"], med[tag + "no residual"], med[tag + "whole call"], med[tag + "K=8 scores"]
            lines.append(f"K = {k}, {sweeps} sweeps: projection {p:.1f} ({nbytes / (p * 1e-6) / 1e12:.2f} TB/s, {p / y:.2f} x the K = 8 score launch), "
                         f"solve {s - p:.1f}, residual {w - s:.1f} ({nbytes / (max(w - s, 1e-3) * 1e-6) / 1e12:.2f} TB/s)")
    lines.append(f"logf on the device against f64 log over 2^20 values in 1e-6 .. 1e3 and 4096 in 0.5 .. 2: largest error {ulp:.2f} ulp (at x = {at:.6g})")
    if host:
        lines.append(host)
    lines.append("(host): host time around the whole C call and its synchronisation, with the upload of the endmembers' table")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
