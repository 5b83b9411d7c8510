"""Developer tool: thz_sparse_deconv on one resident cube in one process — P = 64 and 128 taps, 0, 100 and 200 iterations,
ISTA and FISTA, the calls alternating.  Device time per call from the stage timer (a hipEvent pair around the launch).
The rate is 4 nt P n_iter npix / t: two products of nt x P multiply-adds per trace and iteration, the operations the
algorithm needs whatever the kernel executes (its zero taps are not counted).  Beside it the f32 vector peak and the
guide's figure for an untuned v_pk_fma_f32 GEMM.

Two checks stand in for a fixed rate: t(200) - t(100) equals t(100) - t(0) within the run's spread (an iteration must not
touch HBM: the cube is read once and written once whatever n_iter), and the LDS bank conflicts predicted from the bank
rule (none in the tap loop) — no counter pass is taken here.

The host line: thz_host_sparse_trace on a sample of traces over the host's threads, scaled to the cube.

    python scripts/gpu_sparse_timing.py [--rounds 5] [--out profiles/sparse_timing.txt] [nx ny nt]
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import sparse_model  # noqa: E402
import synth  # noqa: E402
import thz_image_explorer_amd as pkg  # noqa: E402
from thz_image_explorer_amd.binding import STAGE_ECHO  # noqa: E402

PEAK_F32_TF, UNTUNED_PK_FMA_TF = 157.3, 52.0
HBM_BYTES_PER_S = 8.0e12
TAPS = (64, 128)
ITERS = (0, 100, 200)


def flops(nt, P, n_iter, npix):
    return 4.0 * nt * P * n_iter * npix


def measure(eng, nx, ny, nt, rounds, warmup=1):
    npix = nx * ny
    tm = synth.make_time(nt)
    eng.set_time_axis(tm)
    d_t, d_cube, d_out = eng.to_device(tm), eng.empty((npix, nt)), eng.empty((npix, nt))
    d_resid, d_nnz = eng.empty((npix,)), eng.alloc(4 * npix)
    eng.synth_cube(d_cube, npix, 0, d_t)
    cases = [(P, n, acc) for P in TAPS for acc in (0, 1) for n in ITERS]
    times = {c: [] for c in cases}
    nnz = {}
    eng.enable_timing(1)
    try:
        for r in range(warmup + rounds):
            for P, n, acc in cases:
                h, step = sparse_model.pulse_taps(P, P // 2)
                eng.sparse_deconv(npix, nt, d_cube, h, pkg.sparse_cfg(P, P // 2, n, acc, step, 0.05, 0.0), d_out, d_resid, d_nnz)
                if r >= warmup:
                    times[(P, n, acc)].append(eng.stage_time_ns(STAGE_ECHO) * 1e-6)
                else:
                    nnz[(P, n, acc)] = float(d_nnz.download((npix,), np.int32).mean())
    finally:
        eng.enable_timing(0)
        for b in (d_t, d_cube, d_out, d_resid, d_nnz):
            b.free()
    return {c: np.array(v) for c, v in times.items()}, nnz


def host_time(nt, P, n_iter, acc, traces, threads):
    """seconds thz_host_sparse_trace takes for `traces` traces on `threads` threads"""
    y = synth.make_traces(np.arange(traces), nt)
    h, step = sparse_model.pulse_taps(P, P // 2)
    cfg = pkg.sparse_cfg(P, P // 2, n_iter, acc, step, 0.05, 0.0)
    pkg.host_sparse_trace(y[0], h, cfg)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(lambda row: pkg.host_sparse_trace(row, h, cfg), y))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-traces", type=int, default=1024)
    ap.add_argument("shape", nargs="*", type=int, default=[512, 512, 1001])
    a = ap.parse_args()
    nx, ny, nt = a.shape[:3]
    npix = nx * ny
    lines = [f"thz_sparse_deconv, {nx}x{ny}x{nt} resident cube (synthetic pulses, 1 % noise), taps of the same pulse, rel_lambda 0.05, "
             f"step 1/(sum|h|)^2; the calls alternating, {a.rounds} rounds after 1 warm-up; device time per call (ms)",
             f"{'P':>4s} {'form':>6s} {'n_iter':>6s} {'median':>9s} {'min':>9s} {'max':>9s} {'spread':>8s} {'TF':>7s} {'of 157.3':>9s} {'of 52':>7s} {'spikes':>7s}"]
    verdicts = []
    with pkg.Engine(0) as eng:
        t, nnz = measure(eng, nx, ny, nt, a.rounds)
    for P in TAPS:
        for acc in (0, 1):
            med, spread = {}, {}
            for n in ITERS:
                v = t[(P, n, acc)]
                med[n], spread[n] = float(np.median(v)), float(v.max() - v.min())
                tf = flops(nt, P, n, npix) / (med[n] * 1e-3) / 1e12
                lines.append(f"{P:4d} {'FISTA' if acc else 'ISTA':>6s} {n:6d} {med[n]:9.2f} {v.min():9.2f} {v.max():9.2f} {spread[n]:8.2f} "
                             f"{tf:7.2f} {tf / PEAK_F32_TF:9.3f} {tf / UNTUNED_PK_FMA_TF:7.3f} {nnz[(P, n, acc)]:7.1f}")
            d1, d2 = med[100] - med[0], med[200] - med[100]
            tol = spread[0] + spread[100] + spread[200]
            verdicts.append(f"P {P} {'FISTA' if acc else 'ISTA'}: t(100) - t(0) = {d1:.2f} ms, t(200) - t(100) = {d2:.2f} ms, the run's spread {tol:.2f} ms: "
                            f"{'equal within it' if abs(d1 - d2) <= tol else f'apart by {abs(d1 - d2):.2f} ms, MORE than it'}; "
                            f"{(d2 / 100) * 1e3:.1f} us an iteration, {flops(nt, P, 100, npix) / (d2 * 1e-3) / 1e12:.2f} TF in the iterations alone")
    lines.append("spread: max - min of the rounds; TF: 4 nt P n_iter npix / median; spikes: mean non-zeros per trace")
    lines.append(f"for scale: reading and writing the cube once per iteration would add {100 * 2 * npix * nt * 4 / HBM_BYTES_PER_S * 1e3:.0f} ms "
                 "per 100 iterations at the HBM peak of 8 TB/s")
    lines += verdicts
    threads = min(16, os.cpu_count() or 1)
    for P in TAPS:
        sec = host_time(nt, P, 100, 1, a.host_traces, threads)
        whole = sec * npix / a.host_traces
        lines.append(f"host: thz_host_sparse_trace, P {P}, 100 FISTA iterations, {a.host_traces} traces on {threads} threads: {sec:.2f} s, "
                     f"scaled to the cube {whole:.0f} s ({flops(nt, P, 100, npix) / whole / 1e9:.1f} GF)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
