"""Developer tool: thz_wavelet_denoise on one resident cube in one process — db2 and db4 at J = 3 and 5, hard shrinkage,
universal thresholds — the calls alternating round by round with a thz_memcpy_d2d of the same cube, the yardstick for one
read plus one write.  Each call is timed by the host clock around the call and a device synchronise; beside it the
kernel's device time from the stage timer (a hipEvent pair around the launch).  The rate is 4 J nt Lf npix / t: the
multiply-adds of the two analysis and the two synthesis chains, the operations the algorithm needs.

No bar is fixed: the table states medians, spread, the ratio to the copy and what the LDS traffic of the layout comes
to (3 Lf ds_read_b32 and 3 ds_write_b32 per output and level) against the guide's ds_read_b32 rate.

    python scripts/gpu_wavelet_timing.py [--rounds 7] [--out profiles/wavelet_timing.txt] [nx ny nt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import synth  # noqa: E402
import thz_image_explorer_amd as pkg  # noqa: E402
from thz_image_explorer_amd.binding import STAGE_ECHO  # noqa: E402

PEAK_F32_TF = 157.3
LDS_READ_B32_BYTES_PER_S = 75e12   # ds_read_b32, every CU streaming
CASES = [(order, J) for order in (2, 4) for J in (3, 5)]


def flops(nt, Lf, J, npix):
    return 2.0 * 4.0 * J * nt * Lf * npix


def measure(eng, nx, ny, nt, rounds, warmup=2):
    npix = nx * ny
    tm = synth.make_time(nt)
    eng.set_time_axis(tm)
    d_t, d_cube, d_out = eng.to_device(tm), eng.empty((npix, nt)), eng.empty((npix, nt))
    d_sigma, d_kept = eng.empty((npix,)), eng.alloc(4 * npix)
    eng.synth_cube(d_cube, npix, 0, d_t)
    wall = {c: [] for c in CASES + ["copy"]}
    dev = {c: [] for c in CASES}
    kept = {}
    eng.enable_timing(1)
    try:
        for r in range(warmup + rounds):
            for case in CASES + ["copy"]:
                eng.sync()
                t0 = time.perf_counter()
                if case == "copy":
                    eng._check(eng.lib.thz_memcpy_d2d(eng.ctx, d_out.ptr, d_cube.ptr, 4 * npix * nt))
                else:
                    order, J = case
                    _, hn, gn = pkg.host_wavelet_filter(order)
                    _, scale = pkg.host_wavelet_universal(nt, J)
                    eng.wavelet_denoise(npix, nt, d_cube, hn, gn, scale, pkg.wavelet_cfg(2 * order, J, 1, 0), d_out, d_sigma, d_kept)
                eng.sync()
                ms = (time.perf_counter() - t0) * 1e3
                if r >= warmup:
                    wall[case].append(ms)
                    if case != "copy":
                        dev[case].append(eng.stage_time_ns(STAGE_ECHO) * 1e-6)
                elif case != "copy":
                    kept[case] = float(d_kept.download((npix,), np.int32).mean())
    finally:
        eng.enable_timing(0)
        for b in (d_t, d_cube, d_out, d_sigma, d_kept):
            b.free()
    return {c: np.array(v) for c, v in wall.items()}, {c: np.array(v) for c, v in dev.items()}, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("shape", nargs="*", type=int, default=[512, 512, 1001])
    a = ap.parse_args()
    nx, ny, nt = a.shape[:3]
    npix = nx * ny
    with pkg.Engine(0) as eng:
        wall, dev, kept = measure(eng, nx, ny, nt, a.rounds)
    copy = float(np.median(wall["copy"]))
    cube_bytes = 2.0 * 4 * npix * nt
    lines = [f"thz_wavelet_denoise, {nx}x{ny}x{nt} resident cube (synthetic pulses, 1 % noise), hard shrinkage, universal thresholds; the calls "
             f"alternating with thz_memcpy_d2d of the cube, {a.rounds} rounds after 2 warm-ups; host clock around call + synchronise (ms)",
             f"{'case':>10s} {'median':>9s} {'min':>9s} {'max':>9s} {'spread':>8s} {'device':>9s} {'x copy':>7s} {'GF':>8s} {'TF':>7s} {'of 157.3':>9s} "
             f"{'LDS ms':>7s} {'kept':>7s}",
             f"{'copy':>10s} {copy:9.3f} {wall['copy'].min():9.3f} {wall['copy'].max():9.3f} {wall['copy'].max() - wall['copy'].min():8.3f} "
             f"{'':>9s} {1.0:7.2f}   ({cube_bytes / (copy * 1e-3) / 1e12:.2f} TB/s read + written)"]
    for order, J in CASES:
        v, Lf = wall[(order, J)], 2 * order
        med = float(np.median(v))
        tf = flops(nt, Lf, J, npix) / (med * 1e-3) / 1e12
        lds_bytes = 4.0 * (3 * Lf + 3) * J * nt * npix     # reads and writes of the level loops, the select's passes not counted
        lines.append(f"{'db%d J %d' % (order, J):>10s} {med:9.3f} {v.min():9.3f} {v.max():9.3f} {v.max() - v.min():8.3f} "
                     f"{float(np.median(dev[(order, J)])):9.3f} {med / copy:7.2f} {flops(nt, Lf, J, npix) / 1e9:8.1f} {tf:7.2f} {tf / PEAK_F32_TF:9.3f} "
                     f"{lds_bytes / LDS_READ_B32_BYTES_PER_S * 1e3:7.3f} {kept[(order, J)]:7.1f}")
    lines.append("spread: max - min of the rounds; device: median of the stage timer; x copy: median / the copy's median; GF: 2 * 4 J nt Lf npix "
                 "(a multiply-add is two operations); LDS ms: 4 (3 Lf + 3) J nt npix bytes of ds_read_b32 / ds_write_b32 at 75 TB/s; "
                 "kept: mean coefficients kept per trace")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
