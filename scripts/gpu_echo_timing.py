"""Developer tool: thz_echo_map (K = 1, 2, 4; mode 1, guard 30, threshold 0.2) against thz_peak_map (mode 1) — one pass
over the same bytes — on one resident cube in one process, the four alternating.  Device time per call from the stage
timers (hipEvent pairs around the launch).  The bar of DESIGN.md §4.8: K = 2 stays within twice the peak map's median
plus that run's spread, or the rounds behind the first do not run from registers or cache.

    python scripts/gpu_echo_timing.py [--rounds 30] [--out profiles/echo_map_timing.txt] [nx ny nt ...]
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
from thz_image_explorer_amd.binding import STAGE_ECHO, STAGE_PEAK  # noqa: E402

KS = (1, 2, 4)


def measure(eng, nx, ny, nt, rounds, warmup=5):
    npix = nx * ny
    tm = synth.make_time(nt)
    eng.set_time_axis(tm)
    d_t, d_cube = eng.to_device(tm), eng.empty((npix, nt))
    eng.synth_cube(d_cube, npix, 0, d_t)
    kmax = max(KS)
    d_idx, d_off, d_val, d_cnt = eng.alloc(4 * kmax * npix), eng.empty((kmax * npix,)), eng.empty((kmax * npix,)), eng.alloc(4 * npix)
    times = {"peak_map": [], **{f"echo_map K={k}": [] for k in KS}}
    found = {}
    eng.enable_timing(1)
    try:
        for r in range(warmup + rounds):
            eng.peak_map(npix, nt, d_cube, 1, d_idx, d_off, d_val)
            row = [eng.stage_time_ns(STAGE_PEAK)]
            for k in KS:
                eng.echo_map(npix, nt, d_cube, pkg.echo_cfg(pkg.PEAK_MAX, k, 30, 0.2), d_idx, d_off, d_val, d_cnt)
                row.append(eng.stage_time_ns(STAGE_ECHO))
                if r == 0:
                    found[k] = float(d_cnt.download((npix,), np.int32).mean())
            if r >= warmup:
                for name, v in zip(times, row):
                    times[name].append(v * 1e-3)
    finally:
        eng.enable_timing(0)
        for b in (d_t, d_cube, d_idx, d_off, d_val, d_cnt):
            b.free()
    return {k: np.array(v) for k, v in times.items()}, npix * nt * 4, found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("shape", nargs="*", type=int, default=[512, 512, 1001, 1024, 1024, 4096])
    a = ap.parse_args()
    lines = [f"thz_echo_map (mode 1, guard 30, threshold 0.2) vs thz_peak_map (mode 1), one resident cube, alternating, {a.rounds} rounds "
             "after 5 warm-up; device time per call (us)",
             f"{'cube':>16s} {'kernel':>16s} {'median':>9s} {'min':>9s} {'max':>9s} {'spread':>8s} {'GB/s':>8s} {'vs peak_map':>12s} {'found':>6s}"]
    verdicts = []
    with pkg.Engine(0) as eng:
        for i in range(0, len(a.shape), 3):
            nx, ny, nt = a.shape[i:i + 3]
            t, nbytes, found = measure(eng, nx, ny, nt, a.rounds)
            base = np.median(t["peak_map"])
            spreads = {}
            for k, v in t.items():
                med = np.median(v)
                spreads[k] = np.percentile(v, 90) - np.percentile(v, 10)
                n_found = found.get(int(k.split("=")[1]), 1.0) if "=" in k else 1.0
                lines.append(f"{f'{nx}x{ny}x{nt}':>16s} {k:>16s} {med:9.1f} {v.min():9.1f} {v.max():9.1f} {spreads[k]:8.1f} {nbytes / med / 1e3:8.0f} "
                             f"{med / base:12.3f} {n_found:6.2f}")
            k2 = np.median(t["echo_map K=2"])
            bar = 2 * base + max(spreads["peak_map"], spreads["echo_map K=2"])
            verdicts.append(f"{nx}x{ny}x{nt}: K = 2 takes {k2:.1f} us, the bar (2 x peak_map + spread) is {bar:.1f} us: {'within' if k2 <= bar else 'OVER'}")
    lines.append("spread: 10th to 90th percentile of the rounds; GB/s: the cube's bytes over the median; found: mean number of ranks per trace")
    lines += verdicts
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
