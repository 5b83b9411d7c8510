"""Developer tool: thz_peak_map against thz_intensity — the parent's kernel with the same bytes — on one resident cube
in one process, the two alternating.  Device time per call from the stage timers (hipEvent pairs around the launch).

    python scripts/gpu_peak_timing.py [--rounds 30] [--out profiles/peak_map_timing.txt] [nx ny nt ...]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import synth  # noqa: E402
import thz_image_explorer_amd as pkg  # noqa: E402
from thz_image_explorer_amd.binding import STAGE_INTENSITY, STAGE_PEAK  # noqa: E402


def measure(eng, nx, ny, nt, rounds, warmup=5):
    npix = nx * ny
    tm = synth.make_time(nt)
    eng.set_time_axis(tm)
    d_t, d_cube = eng.to_device(tm), eng.empty((npix, nt))
    eng.synth_cube(d_cube, npix, 0, d_t)
    d_img, d_idx, d_off, d_val = eng.empty((npix,)), eng.alloc(4 * npix), eng.empty((npix,)), eng.empty((npix,))
    times = {"intensity": [], "peak_map mode 0": [], "peak_map mode 1": []}
    eng.enable_timing(1)
    try:
        for r in range(warmup + rounds):
            eng.intensity(npix, d_cube, d_img)
            a = eng.stage_time_ns(STAGE_INTENSITY)
            eng.peak_map(npix, nt, d_cube, 0, d_idx, d_off, d_val)
            b = eng.stage_time_ns(STAGE_PEAK)
            eng.peak_map(npix, nt, d_cube, 1, d_idx, d_off, d_val)
            c = eng.stage_time_ns(STAGE_PEAK)
            if r >= warmup:
                for k, v in zip(times, (a, b, c)):
                    times[k].append(v * 1e-3)
    finally:
        eng.enable_timing(0)
        for b in (d_t, d_cube, d_img, d_idx, d_off, d_val):
            b.free()
    return {k: np.array(v) for k, v in times.items()}, npix * nt * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("shape", nargs="*", type=int, default=[512, 512, 1001, 1024, 1024, 4096])
    a = ap.parse_args()
    lines = [f"thz_peak_map vs thz_intensity, one resident cube, alternating, {a.rounds} rounds after 5 warm-up; device time per call (us)",
             f"{'cube':>16s} {'kernel':>16s} {'median':>9s} {'min':>9s} {'max':>9s} {'spread':>8s} {'GB/s':>8s} {'vs intensity':>13s}"]
    with pkg.Engine(0) as eng:
        for i in range(0, len(a.shape), 3):
            nx, ny, nt = a.shape[i:i + 3]
            t, nbytes = measure(eng, nx, ny, nt, a.rounds)
            base = np.median(t["intensity"])
            for k, v in t.items():
                med = np.median(v)
                spread = np.percentile(v, 90) - np.percentile(v, 10)
                lines.append(f"{f'{nx}x{ny}x{nt}':>16s} {k:>16s} {med:9.1f} {v.min():9.1f} {v.max():9.1f} {spread:8.1f} {nbytes / med / 1e3:8.0f} {med / base:13.3f}")
    lines.append("spread: 10th to 90th percentile of the rounds; GB/s: the cube's bytes over the median")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
