"""Developer tool: thz_session_optical_maps on the resident spectra of one recompute, alternating with thz_peak_map — a
streaming pass of known speed — over a cube of as many bytes as the map reads of the two spectrum cubes
(8 |hull| npix); device time per call from the stage timers.  Then, once, the host route the map replaces: download
both spectrum cubes and loop thz_host_optical_properties over the pixels.

    python scripts/gpu_optical_timing.py [--rounds 30] [--out profiles/optical_map_timing.txt] [--no-host] [nx ny nt]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import synth  # noqa: E402
import thz_image_explorer_amd as pkg  # noqa: E402
from thz_image_explorer_amd.binding import STAGE_OPTICAL, STAGE_PEAK  # noqa: E402

BANDS_THZ = [(0.3, 1.0), (1.0, 2.0), (2.0, 4.0)]   # three bands inside the default 0.2 - 5 THz band pass
ANCHOR_THZ = (0.3, 1.5)


def bins(f, lo, hi):
    k = np.flatnonzero((f >= lo) & (f < hi))
    return int(k[0]), int(k[-1]) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("shape", nargs="*", type=int, default=[512, 512, 1001])
    a = ap.parse_args()
    nx, ny, nt = a.shape
    npix, nf, warmup = nx * ny, nt // 2 + 1, 5
    lines = []
    with pkg.Engine(0) as eng:
        tm = synth.make_time(nt)
        sess = pkg.Session(eng, nx, ny, tm)
        d_t = eng.to_device(tm)
        eng.synth_cube(eng.lib.thz_session_buffer(sess.h, pkg.BUF_RAW), npix, 0, d_t)
        sess.upload(None, subtract_bias=False)
        sess.recompute(pkg.chain_cfg_default(tm))
        f = pkg.host_frequency_axis(tm)
        _, ref_amp, ref_phase = eng.reference_spectrum(tm, tm, synth.make_traces([npix + 7], nt)[0])
        bands = [bins(f, lo, hi) for lo, hi in BANDS_THZ]
        anchor = bins(f, *ANCHOR_THZ)
        cfg = pkg.optical_cfg(1e-3, anchor, bands)
        hull = (min(anchor[0], min(b[0] for b in bands)), max(anchor[1], max(b[1] for b in bands)))
        nhull = hull[1] - hull[0]
        nbytes = 8 * nhull * npix
        # the streaming pass: a cube of the same bytes, rows as long as a pixel's two hull slices
        d_cube = eng.alloc(nbytes).zero()
        d_idx = eng.alloc(4 * npix)
        times = {"optical_maps": [], "peak_map, same bytes": []}
        eng.enable_timing(1)
        try:
            for r in range(warmup + a.rounds):
                eng._check(eng.lib.thz_session_optical_maps(sess.h, ref_amp.ctypes.data, ref_phase.ctypes.data, nf, C.byref(cfg), None))
                row = [eng.stage_time_ns(STAGE_OPTICAL)]
                eng.peak_map(npix, 2 * nhull, d_cube, 0, d_idx, None, None)
                row.append(eng.stage_time_ns(STAGE_PEAK))
                if r >= warmup:
                    for k, v in zip(times, row):
                        times[k].append(v * 1e-3)
        finally:
            eng.enable_timing(0)
        lines.append(f"thz_session_optical_maps on a resident {nx}x{ny}x{nt} recompute ({eng.kernel_variant()}), bands {bands} + anchor {anchor} of {nf} bins: "
                     f"hull {hull}, {nhull} bins, {nbytes / 1e6:.0f} MB of the two spectrum cubes")
        lines.append(f"alternating, {a.rounds} rounds after {warmup} warm-up; device time per call (us)")
        lines.append(f"{'kernel':>28s} {'median':>9s} {'min':>9s} {'max':>9s} {'spread':>8s} {'GB/s':>8s} {'vs peak_map':>12s}")
        base = np.median(times["peak_map, same bytes"])
        for k, v in times.items():
            v = np.array(v)
            med = np.median(v)
            spread = np.percentile(v, 90) - np.percentile(v, 10)
            lines.append(f"{k:>28s} {med:9.1f} {v.min():9.1f} {v.max():9.1f} {spread:8.1f} {nbytes / med / 1e3:8.0f} {med / base:12.3f}")
        lines.append("spread: 10th to 90th percentile of the rounds; GB/s: 8 |hull| npix bytes over the median")
        print("\n".join(lines), flush=True)
        if not a.no_host:
            # the route the map replaces: both cubes to the host, the host loop per pixel and band
            t0 = time.perf_counter()
            A, P = sess.download(pkg.BUF_AMPLITUDES), sess.download(pkg.BUF_PHASES)
            t_down = time.perf_counter() - t0
            t0 = time.perf_counter()
            out = np.empty((3, len(bands), npix), np.float32)
            for p in range(npix):
                vals = pkg.host_optical_properties(A[p], P[p], ref_amp, ref_phase, f, 1e-3)
                for b, (k0, k1) in enumerate(bands):
                    for q in range(3):
                        out[q, b, p] = vals[q][k0:k1].mean()
            t_loop = time.perf_counter() - t0
            lines.append(f"host route, once: download of both cubes ({2 * npix * nf * 4 / 1e6:.0f} MB) {t_down * 1e3:.0f} ms, "
                         f"thz_host_optical_properties over {npix} pixels from Python {t_loop:.1f} s (no anchor: the host loop has none)")
            print(lines[-1], flush=True)
        sess.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
