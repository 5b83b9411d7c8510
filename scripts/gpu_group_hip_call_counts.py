"""One fixed sequence of group calls, meant to be run under `rocprofv3 --hip-trace --stats -- python <this file>`.

A change of the group layer's host orchestration (csrc/group*.cpp) that moves no device work must leave the number of
calls per HIP API name unchanged: hipMalloc, hipFree, hipStreamSynchronize, hipEventRecord, hipStreamWaitEvent,
hipMemcpyAsync, hipMemcpy2DAsync and the kernel launches (hipSetDevice alone may differ).  Run it for the build before
and the build after, each from its own tree, and compare the two stats tables
(profiles/group_hip_api_stats_*.csv hold the pair taken when the layer was split into group_*.cpp).

The sequence: a same-device group of two members over a 36 x 32 x 256 cube; upload; three recomputes with pixel
means and one region of interest (gather level TIME); the Deconvolution stage; the 3-D voxel view with a threshold.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synth  # noqa: E402
import thz_image_explorer_amd as pkg  # noqa: E402


def main():
    nx, ny, nt = 36, 32, 256
    time, cube = synth.make_cube(nx, ny, nt)
    cfg = pkg.chain_cfg_default(time)
    cfg.want_means = 1
    psf = pkg.psf_from_npz(np.load(os.path.join(ROOT, "tests", "golden", "psf_sample.npz")))
    with pkg.Group(devices=[0, 0]) as g:
        gs = pkg.GroupSession(g, nx, ny, time, 0.5, 0.5)
        try:
            gs.upload(cube, subtract_bias=False)
            gs.set_rois([[(4, 4), (28, 6), (26, 30), (8, 27)]])
            for _ in range(3):
                gs.recompute(cfg, 1, pkg.GATHER_TIME)
            rc = gs.deconvolve(psf, pkg.DeconvCfg(20, 5, 0.4, 3.0, 0.5))
            inst, thr, dims, count = gs.voxels(pkg.voxel_cfg_default(), nx * ny * nt // 8, 1, (nx, ny, nt))
            roi = gs.roi(0)
            print(f"deconvolve rc={rc} voxels count={count} kept={len(inst)} threshold={thr:.6g} roi keys={sorted(roi)[:3]}")
            print("image checksum", float(np.abs(gs.download(pkg.BUF_IMG)).sum()))
        finally:
            gs.close()


if __name__ == "__main__":
    main()
