"""Developer tool: k-means on a resident recompute — one thz_session_cluster_step (assign, per-cluster
sums, inertia and fold) on the amplitudes 0.2 .. 5 THz at K = 4 and K = 16, alternating in one process with
thz_pca_scores over the same matrix (the same traffic: every row once, K table rows per pixel; it takes at most 8
components, so K = 16 stands against 8).  Device time from the stage timer (hipEvent pairs around the launches), host
time around the whole C call.  Then a whole thz_session_cluster (farthest-first, a fixed number of steps) and, once, the
host route it replaces: the download of the amplitudes and the numpy model of tests/cluster_model.py with the same
number of steps.  Nothing here is a bar.

    python scripts/gpu_cluster_timing.py [--rounds 20] [--steps 5] [--out profiles/cluster_timing.txt] [nx ny nt]
"""
import argparse
import os
import sys
import time as clock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import cluster_model as model  # noqa: E402
import synth  # noqa: E402
import thz_image_explorer_amd as pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="leave the numpy route out")
    ap.add_argument("shape", nargs="*", type=int, default=[512, 512, 1001])
    a = ap.parse_args()
    nx, ny, nt = a.shape[:3]
    npix = nx * ny
    tm = synth.make_time(nt)
    first, count = model.band_bins(tm)
    count = min(count, pkg.PCA_MAX_LEN)
    nf = nt // 2 + 1
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
        eng.enable_timing(1)
        try:
            for k in (4, 16):
                ks = min(k, pkg.PCA_MAX_COMPONENTS)
                cfg = pkg.cluster_cfg(first, count, 1, k, init=0)
                cent = np.stack([sess.cluster_row(pkg.BUF_AMPLITUDES, cfg, int(p)) for p in rng.integers(0, npix, k)])
                comps = rng.standard_normal((ks, count)).astype(np.float32)
                names = (f"K={k} step (launches)", f"K={k} step (call)", f"K={ks} scores (launch)", f"K={ks} scores (call)")
                for name in names:
                    t[name] = []
                for r in range(3 + a.rounds):
                    t0 = clock.perf_counter()
                    sess.cluster_step(pkg.BUF_AMPLITUDES, cfg, cent)
                    row = [eng.stage_time_ns(pkg.STAGE_PCA) * 1e-3, (clock.perf_counter() - t0) * 1e6]
                    t0 = clock.perf_counter()
                    eng.pca_scores(npix, count, d_amp, nf, 1, None, comps, d_scores)
                    eng.sync()
                    row += [eng.stage_time_ns(pkg.STAGE_PCA) * 1e-3, (clock.perf_counter() - t0) * 1e6]
                    if r >= 3:
                        for name, v in zip(names, row):
                            t[name].append(v)
        finally:
            eng.enable_timing(0)
        whole = pkg.cluster_cfg(first, count, 1, 4, max_iter=a.steps)
        t["K=4 session_cluster"] = []
        for r in range(2 + max(a.rounds // 4, 3)):
            t0 = clock.perf_counter()
            out, label, _, cent = sess.cluster(pkg.BUF_AMPLITUDES, whole)
            if r >= 2:
                t["K=4 session_cluster"].append((clock.perf_counter() - t0) * 1e6)
        host = ""
        if not a.no_host:
            t0 = clock.perf_counter()
            amp = sess.download(pkg.BUF_AMPLITUDES).reshape(npix, -1)
            t_down = clock.perf_counter() - t0
            t0 = clock.perf_counter()
            want = model.kmeans(np.ascontiguousarray(amp[:, first:first + count]), 4, max_iter=a.steps)
            t_numpy = clock.perf_counter() - t0
            same = int((want["label"] == label).sum())
            host = (f"host route, once: download of the amplitudes {t_down * 1e3:.0f} ms ({amp.nbytes / 1e6:.0f} MB) + numpy farthest-first and "
                    f"{want['iterations']} steps {t_numpy * 1e3:.0f} ms; {same} of {npix} labels equal the device's")
        sess.close()
    nbytes = 4.0 * npix * count
    lines = [f"k-means of the resident amplitudes, {nx} x {ny} x {nt}, bins {first} .. {first + count - 1} ({count}); {a.rounds} rounds after 3 "
             f"warm-up, a step alternating with thz_pca_scores over the same {nbytes / 1e6:.0f} MB; us",
             f"{'what':>24s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    for name, v in t.items():
        v = np.array(v)
        lines.append(f"{name:>24s} {np.median(v):10.1f} {v.min():10.1f} {v.max():10.1f}")
    for k in (4, 16):
        s, p = np.median(t[f"K={k} step (launches)"]), np.median(t[f"K={min(k, 8)} scores (launch)"])
        lines.append(f"K = {k}: the step's launches take {s / p:.2f} x the score launch (K = {min(k, 8)}); the step reads the matrix twice "
                     f"(assign, then the sums over the labels): {2 * nbytes / (s * 1e-6) / 1e12:.2f} TB/s")
    lines.append(f"thz_session_cluster, K = 4, farthest-first (a mean and 4 seeding steps) and {out.iterations} steps (converged {out.converged}): "
                 f"median {np.median(t['K=4 session_cluster']) * 1e-3:.2f} ms")
    if host:
        lines.append(host)
    lines.append("(call): host time around the whole C call, with its upload of the centroids, its download and its synchronisation")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
