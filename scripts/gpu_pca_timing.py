"""Developer tool: the principal-component calls on a resident recompute — thz_session_pca_sums, _pca_gram
and _pca_project on the amplitudes 0.2 .. 5 THz, K = 4 — alternating in one process with thz_peak_map over a cube of the
bytes the Gram kernel reads.  Device time of the Gram and score launches from the stage timer (hipEvent pairs around the
launches); the sums call has no stage of its own and is timed on the host around the whole call, as is the Gram call a
second time, so that the launch can be told from its upload, download and synchronisation.  Once, the host route this
replaces: the download of the amplitudes and numpy's covariance and eigh.  Nothing here is a bar.

    python scripts/gpu_pca_timing.py [--rounds 20] [--out profiles/pca_timing.txt] [nx ny nt]
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

F32_MATRIX_TFLOPS, HBM_TBS = 157.3, 8.0   # the data sheet's f32 matrix rate and HBM3E bandwidth of one MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("shape", nargs="*", type=int, default=[512, 512, 1001])
    a = ap.parse_args()
    nx, ny, nt = a.shape[:3]
    npix, k = nx * ny, 4
    tm = synth.make_time(nt)
    f = np.arange(nt // 2 + 1) / (float(tm[-1]) - float(tm[0]))
    bins = np.flatnonzero((f >= 0.2) & (f <= 5.0))
    first, count = int(bins[0]), int(min(bins.size, pkg.PCA_MAX_LEN))
    cfg = pkg.pca_cfg(first, count, 1, k)
    t = {name: [] for name in ("peak_map", "sums (call)", "gram (launches)", "gram (call)", "scores (launch)", "scores (call)")}
    with pkg.Engine(0) as eng:
        eng.set_time_axis(tm)
        sess = pkg.Session(eng, nx, ny, tm)
        d_t = eng.to_device(tm)
        eng.synth_cube(eng.lib.thz_session_buffer(sess.h, pkg.BUF_RAW), npix, 0, d_t)
        sess.upload(None)
        sess.recompute(pkg.chain_cfg_default(tm))
        d_same = eng.empty((npix, count))          # a cube of the bytes the Gram kernel reads, for the streaming pass
        d_idx, d_off, d_val = eng.alloc(4 * npix), eng.empty((npix,)), eng.empty((npix,))
        eng.lib.thz_memcpy_d2d(eng.ctx, d_same.ptr, eng.lib.thz_session_buffer(sess.h, pkg.BUF_DATA), npix * count * 4)
        eng.enable_timing(1)
        try:
            for r in range(3 + a.rounds):
                eng.peak_map(npix, count, d_same, 1, d_idx, d_off, d_val)
                row = [eng.stage_time_ns(pkg.binding.STAGE_PEAK) * 1e-3]
                t0 = clock.perf_counter()
                total, n = sess.pca_sums(pkg.BUF_AMPLITUDES, cfg)
                row.append((clock.perf_counter() - t0) * 1e6)
                mu = (total / n).astype(np.float32)
                t0 = clock.perf_counter()
                gram = sess.pca_gram(pkg.BUF_AMPLITUDES, cfg, mu)
                wall = (clock.perf_counter() - t0) * 1e6
                row += [eng.stage_time_ns(pkg.STAGE_PCA) * 1e-3, wall]
                if r == 0:
                    t0 = clock.perf_counter()
                    rc, comp, ev, tot = pkg.host_pca_components(gram, n, k)
                    t_eig = (clock.perf_counter() - t0) * 1e6
                    assert rc == 0
                t0 = clock.perf_counter()
                eng._check(eng.lib.thz_session_pca_project(sess.h, pkg.BUF_AMPLITUDES, cfg, mu.ctypes.data, comp.ctypes.data))
                wall = (clock.perf_counter() - t0) * 1e6
                row += [eng.stage_time_ns(pkg.STAGE_PCA) * 1e-3, wall]
                if r >= 3:
                    for name, v in zip(t, row):
                        t[name].append(v)
        finally:
            eng.enable_timing(0)
        # the host route, once
        t0 = clock.perf_counter()
        amp = sess.download(pkg.BUF_AMPLITUDES).reshape(npix, -1)
        t_down = clock.perf_counter() - t0
        t0 = clock.perf_counter()
        x = amp[:, first:first + count].astype(np.float64)
        x -= x.mean(axis=0)
        w, v = np.linalg.eigh(x.T @ x / (npix - 1))
        t_numpy = clock.perf_counter() - t0
        sess.close()
    flop, nbytes = 2.0 * npix * count * count, 4.0 * npix * count
    n32 = (count + 31) // 32
    lines = [f"principal components of the resident amplitudes, {nx} x {ny} x {nt}, bins {first} .. {first + count - 1} ({count}), K = {k}; "
             f"{a.rounds} rounds after 3 warm-up, alternating with thz_peak_map over {nbytes / 1e6:.0f} MB; us",
             f"{'what':>18s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    for name, v in t.items():
        v = np.array(v)
        lines.append(f"{name:>18s} {np.median(v):10.1f} {v.min():10.1f} {v.max():10.1f}")
    g = np.median(t["gram (launches)"]) * 1e-6
    lines += [f"thz_host_pca_components ({count} x {count}, once): {t_eig:.0f} us; eigenvalues {np.array2string(ev, precision=5)} of total variance {tot:.5g}",
              f"Gram launches: {flop / 1e9:.1f} GFLOP as full products ({flop / g / 1e12:.2f} TF, {100 * flop / g / 1e12 / F32_MATRIX_TFLOPS:.1f} % of the "
              f"{F32_MATRIX_TFLOPS} TF f32 matrix rate; the kernel computes {n32 * (n32 + 1) // 2} of the {n32 * n32} "
              f"32 x 32 tiles) over {nbytes / 1e6:.0f} MB ({nbytes / g / 1e12:.2f} TB/s, {100 * nbytes / g / 1e12 / HBM_TBS:.1f} % of {HBM_TBS} TB/s)",
              f"streaming pass over the same bytes (thz_peak_map): {nbytes / (np.median(t['peak_map']) * 1e-6) / 1e12:.2f} TB/s",
              f"host route, once: download of the amplitudes {t_down * 1e3:.0f} ms ({amp.nbytes / 1e6:.0f} MB) + numpy mean, covariance and eigh {t_numpy * 1e3:.0f} ms",
              "(call): host time around the whole C call, with its uploads, its download and its synchronisation; no vector-FMA form of the Gram kernel was built"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
