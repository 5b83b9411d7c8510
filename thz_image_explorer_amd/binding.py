"""ctypes binding of libthzgpu.so (include/thzgpu.h).

Test / bench harness glue only: the product is the C-ABI library.  There is no
CPU fallback — if the library is missing or no GPU is visible, loading or
`Engine()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libthzgpu.so")

THZ_OK = 0
STATUS = {0: "THZ_OK", -1: "THZ_ERR_INVALID", -2: "THZ_ERR_UNSUPPORTED", -3: "THZ_ERR_HIP",
          -4: "THZ_ERR_NOT_READY", -5: "THZ_ERR_ABORTED"}

WIN_ADAPTED_BLACKMAN, WIN_BLACKMAN, WIN_HANNING, WIN_HAMMING, WIN_FLAT_TOP = range(5)
STAGE_FFT, STAGE_FD_MASK, STAGE_IFFT, STAGE_PIPELINE, STAGE_TD_WINDOW, STAGE_INTENSITY, \
    STAGE_MEAN, STAGE_ROI, STAGE_VOXEL_OPACITY, STAGE_VOXEL_SELECT, STAGE_VOXEL_EMIT, STAGE_PROBE, STAGE_PEAK, \
    STAGE_OPTICAL, STAGE_ECHO, STAGE_PCA = range(16)
PEAK_ABS, PEAK_MAX, PEAK_MIN = range(3)  # thz_peak_map's mode: largest |x|, maximum, minimum


class WindowCfg(C.Structure):
    _fields_ = [("type", C.c_int32), ("lower", C.c_float), ("upper", C.c_float)]


class Spline(C.Structure):
    _fields_ = [("knots", C.c_void_p), ("values", C.c_void_p), ("coeff_a", C.c_void_p), ("coeff_b", C.c_void_p),
                ("coeff_c", C.c_void_p), ("coeff_d", C.c_void_p), ("n_knots", C.c_size_t)]


class HybridFit(C.Structure):
    _fields_ = [("base_a", C.c_float), ("base_b", C.c_float), ("correction", Spline)]


class Psf(C.Structure):
    _fields_ = [("wx_fit", HybridFit), ("wy_fit", HybridFit), ("x0_spline", Spline), ("y0_spline", Spline)]


class DeconvCfg(C.Structure):
    _fields_ = [("n_iterations", C.c_uint32), ("n_filters", C.c_uint32), ("start_freq", C.c_float),
                ("end_freq", C.c_float), ("win_width", C.c_float), ("band_begin", C.c_uint32),
                ("band_end", C.c_uint32)]


def psf_from_npz(z) -> "Psf":
    """Builds a thz_psf from the arrays of a psf.npz (keys of io.rs:146-166).
    The f32 copies are kept alive on the returned object."""
    keep = []

    def arr(key):
        a = np.ascontiguousarray(np.asarray(z[key], np.float64).astype(np.float32))
        keep.append(a)
        return a

    def spline(prefix, knots_key, values_key):
        k, v = arr(knots_key), arr(values_key)
        co = [arr(f"{prefix}coeff_{c}") for c in "abcd"]
        return Spline(k.ctypes.data, v.ctypes.data, co[0].ctypes.data, co[1].ctypes.data, co[2].ctypes.data,
                      co[3].ctypes.data, k.size)

    psf = Psf()
    psf.wx_fit = HybridFit(float(np.asarray(z["wx_base_a"]).ravel()[0]), float(np.asarray(z["wx_base_b"]).ravel()[0]),
                           spline("wx_corr_", "wx_corr_knots_thz", "wx_corr_values_mm"))
    psf.wy_fit = HybridFit(float(np.asarray(z["wy_base_a"]).ravel()[0]), float(np.asarray(z["wy_base_b"]).ravel()[0]),
                           spline("wy_corr_", "wy_corr_knots_thz", "wy_corr_values_mm"))
    psf.x0_spline = spline("x0_", "x0_knots_thz", "x0_values_mm")
    psf.y0_spline = spline("y0_", "y0_knots_thz", "y0_values_mm")
    psf._keep = keep
    return psf


class VoxelCfg(C.Structure):
    _fields_ = [("opacity_threshold", C.c_float), ("contrast", C.c_float), ("sigma", C.c_float),
                ("radius", C.c_int32)]


VOXEL_INSTANCE = np.dtype([("position", np.float32, 3), ("scale", np.float32), ("color", np.float32, 4)])
VOXEL_MAX_INSTANCES = 2_000_000


class ChainCfg(C.Structure):
    _fields_ = [("tilt_active", C.c_int32), ("tilt_x_deg", C.c_double), ("tilt_y_deg", C.c_double),
                ("td_before_active", C.c_int32), ("td_before_low", C.c_double), ("td_before_high", C.c_double),
                ("td_before_width", C.c_double), ("fft_window", WindowCfg),
                ("fd_active", C.c_int32), ("fd_low", C.c_double), ("fd_high", C.c_double), ("fd_width", C.c_double),
                ("td_after_active", C.c_int32), ("td_after_low", C.c_double), ("td_after_high", C.c_double),
                ("td_after_width", C.c_double), ("want_means", C.c_int32), ("scale_factor", C.c_int32),
                ("avg_in_fourier_space", C.c_int32)]


class PipelineIo(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("d_raw", "d_pre_win", "d_fd_mask", "d_fd_cmask", "d_post_win", "d_fft", "d_amp",
                                          "d_phase", "d_data_out", "d_img", "d_sums")] + [("band_lo", C.c_size_t), ("band_hi", C.c_size_t)]


class TiltSrc(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("nt_in", C.c_size_t), ("d_taper", C.c_void_p), ("d_insert_index", C.c_void_p),
                ("d_src_sum", C.c_void_p)]


class RoiOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("signal_fft", "phase_fft", "signal", "roi_data", "count")]


class PlotOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("signal", "signal_fft", "phase_fft", "filtered_signal", "filtered_signal_fft",
                                  "filtered_phase_fft", "avg_signal", "avg_signal_fft", "avg_phase_fft")]


BUF_RAW, BUF_FFT, BUF_AMPLITUDES, BUF_PHASES, BUF_DATA, BUF_IMG, BUF_AVG_FFT, BUF_AVG_AMPLITUDES, \
    BUF_AVG_PHASES, BUF_OPACITY, BUF_PEAK_INDEX, BUF_PEAK_OFFSET, BUF_PEAK_VALUE, \
    BUF_OPT_N, BUF_OPT_ALPHA, BUF_OPT_KAPPA, BUF_OPT_WRAPS, BUF_OPT_SLOPE, \
    BUF_ECHO_INDEX, BUF_ECHO_OFFSET, BUF_ECHO_VALUE, BUF_ECHO_COUNT, BUF_LAYER_THICKNESS, BUF_LAYER_DELAY, \
    BUF_PCA_SCORES, BUF_PCA_COMPONENTS, BUF_PCA_MEAN, \
    BUF_CLUSTER_LABELS, BUF_CLUSTER_DIST, BUF_CLUSTER_CENTROIDS, \
    BUF_SPARSE, BUF_SPARSE_RESID, BUF_SPARSE_NNZ, \
    BUF_UNMIX_ABUNDANCE, BUF_UNMIX_PROJ, BUF_UNMIX_RESID, BUF_UNMIX_KKT, \
    BUF_DENOISED, BUF_DENOISE_SIGMA, BUF_DENOISE_KEPT = range(40)
SPARSE_MAX_TAPS, SPARSE_MAX_NT, SPARSE_MAX_ITER = 256, 4608, 4096  # THZ_SPARSE_*: taps, samples and iterations of one call
# THZ_WAVELET_*: taps, levels and samples of one denoising call, and the most (levels + 2) * samples
WAVELET_MAX_TAPS, WAVELET_MAX_LEVELS, WAVELET_MAX_NT, WAVELET_MAX_WORDS = 16, 6, 4608, 36864
OPTICAL_MAX_BANDS = 8
ECHO_MAX = 4
PCA_MAX_LEN, PCA_MAX_COMPONENTS, PCA_CHAIN = 512, 8, 1024  # THZ_PCA_*: columns, components, products per f32 accumulator
CLUSTER_MAX = 16  # THZ_CLUSTER_MAX: clusters of one k-means call
CLUSTER_INIT_GIVEN, CLUSTER_INIT_FARTHEST = range(2)  # thz_cluster_cfg's init
UNMIX_MAX, UNMIX_MAX_SWEEPS = 16, 4096  # THZ_UNMIX_*: endmembers and sweeps of one unmixing call
LAYER_BETWEEN, LAYER_REFERENCE = range(2)  # thz_layer_map's mode: consecutive pulses, rank 0 against a fixed arrival


class TiltFit(C.Structure):
    """thz_tilt_fit: the arrival plane and the angles that flatten it"""
    _fields_ = [("tilt_x_deg", C.c_double), ("tilt_y_deg", C.c_double), ("slope_x_ps_per_mm", C.c_double),
                ("slope_y_ps_per_mm", C.c_double), ("t0_ps", C.c_double), ("rms_ps", C.c_double), ("n_used", C.c_uint64)]

    def as_tuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


class OpticalCfg(C.Structure):
    """thz_optical_cfg: thickness, anchor range and bands of thz_optical_maps"""
    _fields_ = [("thickness", C.c_float), ("anchor_k0", C.c_uint32), ("anchor_k1", C.c_uint32), ("n_bands", C.c_uint32),
                ("band_k0", C.c_uint32 * 8), ("band_k1", C.c_uint32 * 8)]


def optical_cfg(thickness, anchor, bands) -> OpticalCfg:
    """anchor: (a0, a1) bins or None for none; bands: list of (k0, k1) bin ranges.  More than OPTICAL_MAX_BANDS bands
    keep their count (the library refuses it) but only the first eight ranges"""
    cfg = OpticalCfg()
    cfg.thickness = float(thickness)
    cfg.anchor_k0, cfg.anchor_k1 = (0, 0) if anchor is None else (int(anchor[0]), int(anchor[1]))
    cfg.n_bands = len(bands)
    for i, (k0, k1) in enumerate(list(bands)[:OPTICAL_MAX_BANDS]):
        cfg.band_k0[i], cfg.band_k1[i] = int(k0), int(k1)
    return cfg


class EchoCfg(C.Structure):
    """thz_echo_cfg: key, number of ranks, guard distance and relative threshold of thz_echo_map"""
    _fields_ = [("mode", C.c_int32), ("n_echoes", C.c_int32), ("guard", C.c_int32), ("rel_threshold", C.c_float)]


class LayerCfg(C.Structure):
    """thz_layer_cfg: what thz_layer_map takes the delays between, and the mm per sample of every layer"""
    _fields_ = [("mode", C.c_int32), ("scale", C.c_float * 4), ("ref_index", C.c_int32), ("ref_offset", C.c_float)]


def echo_cfg(mode=PEAK_MAX, n_echoes=2, guard=30, rel_threshold=0.2) -> EchoCfg:
    return EchoCfg(int(mode), int(n_echoes), int(guard), float(rel_threshold))


def layer_cfg(mode=LAYER_BETWEEN, scale=(1.0,), ref_index=0, ref_offset=0.0) -> LayerCfg:
    """scale: mm per sample of delay for each layer; a shorter list is continued with its last value"""
    sc = [float(v) for v in np.atleast_1d(scale)][:4]
    cfg = LayerCfg(int(mode), (C.c_float * 4)(*(sc + [sc[-1]] * (4 - len(sc)))), int(ref_index), float(ref_offset))
    return cfg


class PcaCfg(C.Structure):
    """thz_pca_cfg: the columns of the matrix, the number of components, centring and an optional device mask"""
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("step", C.c_uint32), ("n_components", C.c_int32),
                ("center", C.c_int32), ("d_mask", C.c_void_p)]


class PcaOut(C.Structure):
    """thz_pca_out: eigenvalues (descending), trace of the covariance, unmasked pixels"""
    _fields_ = [("eigenvalues", C.c_double * 8), ("total_variance", C.c_double), ("count", C.c_uint64)]


def pca_cfg(first, count, step=1, n_components=3, center=True, mask=None) -> PcaCfg:
    """mask: device pointer / DevBuf of one uint8 per pixel, or None"""
    return PcaCfg(int(first), int(count), int(step), int(n_components), int(bool(center)), _dp(mask))


class ClusterCfg(C.Structure):
    """thz_cluster_cfg: the columns of the matrix, the number of clusters, the seeding, the step limit, an optional device
    mask and (init 0) the host centroids"""
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("step", C.c_uint32), ("n_clusters", C.c_int32),
                ("init", C.c_int32), ("max_iter", C.c_int32), ("d_mask", C.c_void_p), ("centroids", C.c_void_p)]


class ClusterOut(C.Structure):
    """thz_cluster_out: inertia, labelled unmasked pixels, pixels per cluster, steps run, whether the last changed nothing"""
    _fields_ = [("inertia", C.c_double), ("count", C.c_uint64), ("counts", C.c_uint64 * 16), ("iterations", C.c_int32),
                ("converged", C.c_int32)]


def cluster_cfg(first, count, step=1, n_clusters=3, init=CLUSTER_INIT_FARTHEST, max_iter=100, mask=None, centroids=None) -> ClusterCfg:
    """mask: device pointer / DevBuf of one uint8 per pixel, or None; centroids: (n_clusters, count) host floats for
    init 0 — the array is kept alive by the returned struct"""
    cfg = ClusterCfg(int(first), int(count), int(step), int(n_clusters), int(init), int(max_iter), _dp(mask), None)
    if centroids is not None:
        cfg._centroids = np.ascontiguousarray(centroids, np.float32)
        cfg.centroids = cfg._centroids.ctypes.data
    return cfg


class SparseCfg(C.Structure):
    """thz_sparse_cfg: taps and centre tap, iterations, ISTA (0) or FISTA (1), step and the threshold's two parts"""
    _fields_ = [("n_taps", C.c_int32), ("center", C.c_int32), ("n_iter", C.c_int32), ("accelerate", C.c_int32),
                ("step", C.c_float), ("rel_lambda", C.c_float), ("min_lambda", C.c_float)]


def sparse_cfg(n_taps, center, n_iter=100, accelerate=True, step=1.0, rel_lambda=0.05, min_lambda=0.0) -> SparseCfg:
    return SparseCfg(int(n_taps), int(center), int(n_iter), int(accelerate), float(step), float(rel_lambda), float(min_lambda))


class WaveletCfg(C.Structure):
    """thz_wavelet_cfg: taps and levels, soft (0) or hard (1) shrinkage, thresholds times the median (0) or as given (1)"""
    _fields_ = [("n_taps", C.c_int32), ("n_levels", C.c_int32), ("shrink", C.c_int32), ("noise_mode", C.c_int32)]


def wavelet_cfg(n_taps, n_levels, shrink=0, noise_mode=0) -> WaveletCfg:
    return WaveletCfg(int(n_taps), int(n_levels), int(shrink), int(noise_mode))


class UnmixCfg(C.Structure):
    """thz_unmix_cfg: endmembers, sweeps of the coordinate descent, raw values (0) or absorbance against a reference"""
    _fields_ = [("n_endmembers", C.c_int32), ("n_sweeps", C.c_int32), ("absorbance", C.c_int32)]


class UnmixSessionCfg(C.Structure):
    """thz_unmix_session_cfg: the columns of the matrix, thz_unmix_cfg's three, the host endmembers (NULL: the resident
    k-means centroids) and the host reference spectrum of the absorbance mode"""
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("step", C.c_uint32), ("n_endmembers", C.c_int32),
                ("n_sweeps", C.c_int32), ("absorbance", C.c_int32), ("endmembers", C.c_void_p), ("ref", C.c_void_p)]


def unmix_session_cfg(first, count, step=1, n_endmembers=3, n_sweeps=256, endmembers=None, ref=None, absorbance=None) -> UnmixSessionCfg:
    """endmembers: (n_endmembers, count) host floats, or None for the resident k-means centroids; ref: (count) host floats,
    which turn the absorbance mode on unless `absorbance` says otherwise — the arrays are kept alive by the returned struct"""
    on = ref is not None if absorbance is None else bool(absorbance)
    cfg = UnmixSessionCfg(int(first), int(count), int(step), int(n_endmembers), int(n_sweeps), int(on), None, None)
    if endmembers is not None:
        cfg._endmembers = np.ascontiguousarray(endmembers, np.float32)
        cfg.endmembers = cfg._endmembers.ctypes.data
    if ref is not None:
        cfg._ref = np.ascontiguousarray(ref, np.float32)
        cfg.ref = cfg._ref.ctypes.data
    return cfg


class ThzError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


# every symbol include/thzgpu.h declares: (name, restype, argtypes)
_P = C.c_void_p
_SZ = C.c_size_t
SYMBOLS = [
    ("thz_abi_version", C.c_int, []),
    ("thz_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("thz_destroy", None, [_P]),
    ("thz_release_scratch", C.c_int, [_P]),
    ("thz_last_error", C.c_char_p, [_P]),
    ("thz_stream", _P, [_P]),
    ("thz_sync", C.c_int, [_P]),
    ("thz_malloc", C.c_int, [_P, C.POINTER(_P), _SZ]),
    ("thz_free", C.c_int, [_P, _P]),
    ("thz_memcpy_h2d", C.c_int, [_P, _P, _P, _SZ]),
    ("thz_memcpy_d2h", C.c_int, [_P, _P, _P, _SZ]),
    ("thz_memcpy_d2d", C.c_int, [_P, _P, _P, _SZ]),
    ("thz_memset", C.c_int, [_P, _P, C.c_int, _SZ]),
    ("thz_set_time_axis", C.c_int, [_P, _P, _SZ]),
    ("thz_set_kernel_family", C.c_int, [_P, C.c_int]),
    ("thz_nt", _SZ, [_P]),
    ("thz_nf", _SZ, [_P]),
    ("thz_get_frequency", C.c_int, [_P, _P]),
    ("thz_host_frequency_axis", C.c_int, [_P, _SZ, _P]),
    ("thz_host_fft_window", C.c_int, [_P, _SZ, C.POINTER(WindowCfg), _P]),
    ("thz_host_adapted_blackman", C.c_int, [_P, _SZ, C.c_float, C.c_float, _P]),
    ("thz_host_td_bandpass", C.c_int, [_P, _SZ, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.c_double, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("thz_host_fd_bandpass", C.c_int, [_P, _SZ, C.c_double, C.c_double, C.c_double, _P,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("thz_host_water_line_mask", C.c_int, [_P, _SZ, _P, _SZ, C.c_float, _P]),
    ("thz_host_wiener_filter", C.c_int, [_P, _SZ, C.c_float, _P]),
    ("thz_host_tilt_plan", _SZ, [_P, _SZ, _SZ, _SZ, C.c_double, C.c_double, C.c_float, C.c_float, _P, _P]),
    ("thz_tilt_apply", C.c_int, [_P, _SZ, _P, _SZ, _P, _P, _SZ, _P]),
    ("thz_fft", C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("thz_apply_fd_mask", C.c_int, [_P, _SZ, _P, _P, _P]),
    ("thz_apply_fd_cmask", C.c_int, [_P, _SZ, _P, _P, _P]),
    ("thz_ifft", C.c_int, [_P, _SZ, _P, _P, _P, _P]),
    ("thz_pipeline", C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("thz_pipeline_ex", C.c_int, [_P, _SZ, _P]),
    ("thz_pipeline_tilted", C.c_int, [_P, _SZ, _P, _P]),
    ("thz_apply_td_window", C.c_int, [_P, _SZ, _P, _P, _P]),
    ("thz_intensity", C.c_int, [_P, _SZ, _P, _P]),
    ("thz_subtract_bias", C.c_int, [_P, _SZ, _P, _P]),
    ("thz_pixel_mean", C.c_int, [_P, _SZ, _SZ, _SZ, C.c_int, _P, _P]),
    ("thz_pixel_sum", C.c_int, [_P, _SZ, _SZ, C.c_int, _P, _P]),
    ("thz_roi_mask", C.c_int, [_P, _P, _SZ, C.c_uint64, _SZ, _SZ, _P]),
    ("thz_roi_mean", C.c_int, [_P, _P, _SZ, _SZ, _SZ, _P, _P, _P, C.c_int]),
    ("thz_scale3d", C.c_int, [_P, _P, _SZ, _SZ, _SZ, C.c_int, _SZ, _P]),
    ("thz_host_psf_eval", C.c_int, [C.POINTER(Psf), _P, _SZ, _P, _P, _P, _P]),
    ("thz_host_filter_bank", C.c_int, [_P, _SZ, C.POINTER(DeconvCfg), _P, _P]),
    ("thz_host_band_psf", C.c_int, [C.POINTER(Psf), C.c_float, C.c_float, C.c_float, _SZ, _SZ, _P,
                                    C.POINTER(_SZ), C.POINTER(_SZ)]),
    ("thz_polar_ifft", C.c_int, [_P, _P, _P, C.c_int, _P]),
    ("thz_deconvolve", C.c_int, [_P, C.POINTER(Psf), C.POINTER(DeconvCfg), _SZ, _SZ, C.c_float, C.c_float,
                                 _P, _P, _P, _P, _P, _P]),
    ("thz_synth_cube", C.c_int, [_P, _P, _SZ, C.c_uint64, _P, C.c_uint32, C.c_int]),
    ("thz_chain_cfg_default", C.c_int, [_P, _SZ, C.POINTER(ChainCfg)]),
    ("thz_session_create", C.c_int, [_P, _SZ, _SZ, _SZ, _P, C.c_float, C.c_float, C.POINTER(_P)]),
    ("thz_session_destroy", None, [_P]),
    ("thz_session_upload", C.c_int, [_P, _P, C.c_int]),
    ("thz_session_recompute", C.c_int, [_P, C.POINTER(ChainCfg)]),
    ("thz_session_recompute_from", C.c_int, [_P, C.POINTER(ChainCfg), C.c_int]),
    ("thz_session_set_fd_filters", C.c_int, [_P, _P, _P, _SZ]),
    ("thz_session_set_rois", C.c_int, [_P, _SZ, _P, _P]),
    ("thz_session_roi_count", _SZ, [_P]),
    ("thz_session_roi", C.c_int, [_P, _SZ, C.POINTER(RoiOut)]),
    ("thz_session_grid", C.c_int, [_P, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("thz_session_deconvolve", C.c_int, [_P, C.POINTER(Psf), C.POINTER(DeconvCfg), _P, _P]),
    ("thz_session_nt_out", _SZ, [_P]),
    ("thz_session_time_out", C.c_int, [_P, _P]),
    ("thz_session_buffer", _P, [_P, C.c_int]),
    ("thz_session_download", C.c_int, [_P, C.c_int, _SZ, _SZ, _P]),
    ("thz_host_slab", C.c_int, [_SZ, C.c_int, C.c_int, C.POINTER(_SZ), C.POINTER(_SZ)]),
    ("thz_group_create", C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(_P)]),
    ("thz_group_unique_id", C.c_int, [_P]),
    ("thz_group_create_rank", C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    ("thz_group_destroy", None, [_P]),
    ("thz_group_last_error", C.c_char_p, [_P]),
    ("thz_group_world", C.c_int, [_P]),
    ("thz_group_local_count", C.c_int, [_P]),
    ("thz_group_rank", C.c_int, [_P, C.c_int]),
    ("thz_group_ctx", _P, [_P, C.c_int]),
    ("thz_group_all_reduce_sum", C.c_int, [_P, C.POINTER(_P), _SZ]),
    ("thz_group_all_reduce_u64", C.c_int, [_P, C.POINTER(_P), _SZ]),
    ("thz_group_gather", C.c_int, [_P, C.POINTER(_P), C.POINTER(_SZ), _P]),
    ("thz_group_sync", C.c_int, [_P]),
    ("thz_group_session_create", C.c_int, [_P, _SZ, _SZ, _SZ, _P, C.c_float, C.c_float, C.POINTER(_P)]),
    ("thz_group_session_destroy", None, [_P]),
    ("thz_group_session_member", _P, [_P, C.c_int]),
    ("thz_group_session_upload", C.c_int, [_P, _P, C.c_int]),
    ("thz_group_session_recompute", C.c_int, [_P, C.POINTER(ChainCfg), C.c_int, C.c_int]),
    ("thz_group_session_deconvolve", C.c_int, [_P, C.POINTER(Psf), C.POINTER(DeconvCfg), _P, _P]),
    ("thz_group_session_result", _P, [_P, C.c_int]),
    ("thz_group_session_download", C.c_int, [_P, C.c_int, _SZ, _SZ, _P]),
    ("thz_group_session_grid", C.c_int, [_P, C.POINTER(_SZ), C.POINTER(_SZ)]),
    ("thz_group_session_set_rois", C.c_int, [_P, _SZ, _P, _P]),
    ("thz_group_session_roi", C.c_int, [_P, _SZ, C.POINTER(RoiOut)]),
    ("thz_session_plot", C.c_int, [_P, _SZ, _SZ, C.POINTER(PlotOut)]),
    ("thz_session_voxels", C.c_int, [_P, C.POINTER(VoxelCfg), C.c_uint64, C.c_int, _SZ, _SZ, _SZ, _P, C.c_uint64,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_float), _P]),
    ("thz_group_session_voxels", C.c_int, [_P, C.POINTER(VoxelCfg), C.c_uint64, C.c_int, _SZ, _SZ, _SZ, _P,
                                           C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_float), _P]),
    ("thz_peak_map", C.c_int, [_P, _SZ, _SZ, _P, C.c_int, _P, _P, _P]),
    ("thz_arrival_plane_moments", C.c_int, [_P, _SZ, _SZ, C.c_float, C.c_float, C.c_double, _P, _P, _P, C.c_float, _P]),
    ("thz_host_arrival_plane_fit", C.c_int, [_P, C.POINTER(TiltFit)]),
    ("thz_session_peak_map", C.c_int, [_P, C.c_int, C.c_int]),
    ("thz_session_estimate_tilt", C.c_int, [_P, C.c_int, C.c_int, C.c_float, C.POINTER(TiltFit)]),
    ("thz_group_session_estimate_tilt", C.c_int, [_P, C.c_int, C.c_int, C.c_float, C.POINTER(TiltFit)]),
    ("thz_group_session_peak_result", _P, [_P, C.c_int]),
    ("thz_optical_maps", C.c_int, [_P, _SZ, _SZ, _P, _P, _P, _P, _P, C.POINTER(OpticalCfg), _P, _P, _P, _P, _P, _P]),
    ("thz_session_optical_maps", C.c_int, [_P, _P, _P, _SZ, C.POINTER(OpticalCfg), _P]),
    ("thz_echo_map", C.c_int, [_P, _SZ, _SZ, _P, C.POINTER(EchoCfg), _P, _P, _P, _P]),
    ("thz_layer_map", C.c_int, [_P, _SZ, C.c_int, _P, _P, C.POINTER(LayerCfg), _P, _P]),
    ("thz_host_echo_trace", C.c_int, [_P, _SZ, C.POINTER(EchoCfg), _P, _P, _P, _P]),
    ("thz_session_echo_map", C.c_int, [_P, C.c_int, C.POINTER(EchoCfg)]),
    ("thz_session_layer_map", C.c_int, [_P, C.POINTER(LayerCfg)]),
    ("thz_pca_sums", C.c_int, [_P, _SZ, _SZ, _P, _SZ, _SZ, _P, _P, _P]),
    ("thz_pca_gram", C.c_int, [_P, _SZ, _SZ, _P, _SZ, _SZ, _P, _P, _P]),
    ("thz_host_pca_components", C.c_int, [_P, _SZ, C.c_uint64, C.c_int, _P, _P, _P]),
    ("thz_pca_scores", C.c_int, [_P, _SZ, _SZ, _P, _SZ, _SZ, _P, _P, C.c_int, _P]),
    ("thz_session_pca", C.c_int, [_P, C.c_int, C.POINTER(PcaCfg), C.POINTER(PcaOut)]),
    ("thz_session_pca_sums", C.c_int, [_P, C.c_int, C.POINTER(PcaCfg), _P, _P]),
    ("thz_session_pca_gram", C.c_int, [_P, C.c_int, C.POINTER(PcaCfg), _P, _P]),
    ("thz_session_pca_project", C.c_int, [_P, C.c_int, C.POINTER(PcaCfg), _P, _P]),
    ("thz_cluster_step", C.c_int, [_P, _SZ, _SZ, _P, _SZ, _SZ, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    ("thz_host_cluster_update", C.c_int, [_P, _P, C.c_int, _SZ, _P, _P]),
    ("thz_session_cluster", C.c_int, [_P, C.c_int, C.POINTER(ClusterCfg), C.POINTER(ClusterOut)]),
    ("thz_session_cluster_step", C.c_int, [_P, C.c_int, C.POINTER(ClusterCfg), _P, _P, _P, _P, _P, _P]),
    ("thz_session_cluster_row", C.c_int, [_P, C.c_int, C.POINTER(ClusterCfg), C.c_uint64, _P]),
    ("thz_sparse_deconv", C.c_int, [_P, _SZ, _SZ, _P, _P, C.POINTER(SparseCfg), _P, _P, _P]),
    ("thz_host_sparse_trace", C.c_int, [_P, _SZ, _P, C.POINTER(SparseCfg), _P, _P, _P]),
    ("thz_host_sparse_kernel", C.c_int, [_P, _SZ, C.c_int, C.c_int, _P, _P]),
    ("thz_session_sparse_deconv", C.c_int, [_P, C.c_int, _P, C.POINTER(SparseCfg)]),
    ("thz_wavelet_denoise", C.c_int, [_P, _SZ, _SZ, _P, _P, _P, _P, C.POINTER(WaveletCfg), _P, _P, _P]),
    ("thz_host_wavelet_trace", C.c_int, [_P, _SZ, _P, _P, _P, C.POINTER(WaveletCfg), _P, _P, _P]),
    ("thz_host_wavelet_filter", C.c_int, [C.c_int, _P, _P, C.POINTER(C.c_int)]),
    ("thz_host_wavelet_universal", C.c_int, [_SZ, C.c_int, _P]),
    ("thz_session_wavelet_denoise", C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(WaveletCfg)]),
    ("thz_unmix", C.c_int, [_P, _SZ, _SZ, _P, _SZ, _SZ, _P, _P, C.POINTER(UnmixCfg), _P, _P, _P, _P]),
    ("thz_host_unmix_prepare", C.c_int, [_P, C.c_int, _SZ, _P, _P]),
    ("thz_host_unmix_solve", C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P]),
    ("thz_session_unmix", C.c_int, [_P, C.c_int, C.POINTER(UnmixSessionCfg)]),
    ("thz_host_align_reference", C.c_int, [_P, _SZ, _P, _P, _SZ, _P]),
    ("thz_reference_spectrum", C.c_int, [_P, _P, _SZ, _P, _P, _SZ, C.POINTER(WindowCfg), _P, _P, _P]),
    ("thz_host_optical_properties", C.c_int, [_P, _P, _P, _P, _P, _SZ, C.c_float, _P, _P, _P]),
    ("thz_traffic_probe", C.c_int, [_P, _SZ, _SZ, _P, _P, _P, _P, _P]),
    ("thz_voxel_cfg_default", C.c_int, [C.POINTER(VoxelCfg)]),
    ("thz_host_gaussian_kernel1d", C.c_int, [C.c_float, C.c_int, _P]),
    ("thz_voxel_opacity", C.c_int, [_P, _SZ, _SZ, _P, C.POINTER(VoxelCfg), _P]),
    ("thz_select_histogram", C.c_int, [_P, _P, _SZ, C.c_int, C.c_uint32, _P]),
    ("thz_host_select_step", C.c_int, [_P, C.c_int, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    ("thz_host_select_value", C.c_float, [C.c_int, C.c_int, C.c_int]),
    ("thz_kth_largest", C.c_int, [_P, _P, _SZ, C.c_uint64, C.POINTER(C.c_float)]),
    ("thz_voxel_threshold", C.c_int, [_P, _P, _SZ, C.c_uint64, C.POINTER(C.c_float)]),
    ("thz_voxel_instances", C.c_int, [_P, _P, _SZ, _SZ, _SZ, _SZ, _SZ, C.c_float, C.c_float, C.c_int, _SZ, _SZ,
                                      _SZ, _P, C.c_uint64, C.POINTER(C.c_uint64), _P]),
    ("thz_enable_timing", C.c_int, [_P, C.c_int]),
    ("thz_stage_time_ns", C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    ("thz_timing_collect", C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("thz_kernel_variant", C.c_char_p, [_P]),
]

_lib = None


def load_library() -> C.CDLL:
    """Loads libthzgpu.so and declares every prototype.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _rc(rc: int, what: str):
    if rc != THZ_OK:
        raise ThzError(rc, what)


# -- host multipliers (no GPU, no context) ---------------------------------
def host_frequency_axis(time: np.ndarray) -> np.ndarray:
    t = np.ascontiguousarray(time, np.float32)
    out = np.empty(t.size // 2 + 1, np.float32)
    _rc(load_library().thz_host_frequency_axis(t.ctypes.data, t.size, out.ctypes.data), "frequency_axis")
    return out


def host_fft_window(time, wtype=WIN_ADAPTED_BLACKMAN, lower=1.0, upper=7.0) -> np.ndarray:
    t = np.ascontiguousarray(time, np.float32)
    cfg = WindowCfg(int(wtype), float(lower), float(upper))
    out = np.empty(t.size, np.float32)
    _rc(load_library().thz_host_fft_window(t.ctypes.data, t.size, C.byref(cfg), out.ctypes.data), "fft_window")
    return out


def host_adapted_blackman(axis, lower: float, upper: float) -> np.ndarray:
    a = np.ascontiguousarray(axis, np.float32)
    out = np.empty(a.size, np.float32)
    _rc(load_library().thz_host_adapted_blackman(a.ctypes.data, a.size, lower, upper, out.ctypes.data),
        "adapted_blackman")
    return out


def host_td_bandpass(time, low: float, high: float, width: float):
    """-> (multiplier, clamped_low, clamped_high, lower_idx, upper_idx)"""
    t = np.ascontiguousarray(time, np.float32)
    lo, hi = C.c_double(low), C.c_double(high)
    l, u = C.c_int64(), C.c_int64()
    out = np.empty(t.size, np.float32)
    _rc(load_library().thz_host_td_bandpass(t.ctypes.data, t.size, C.byref(lo), C.byref(hi), width,
                                            out.ctypes.data, C.byref(l), C.byref(u)), "td_bandpass")
    return out, lo.value, hi.value, l.value, u.value


def host_fd_bandpass(frequency, low: float, high: float, width: float):
    """-> (multiplier, lower_idx, upper_idx)"""
    f = np.ascontiguousarray(frequency, np.float32)
    l, u = C.c_int64(), C.c_int64()
    out = np.empty(f.size, np.float32)
    _rc(load_library().thz_host_fd_bandpass(f.ctypes.data, f.size, low, high, width, out.ctypes.data,
                                            C.byref(l), C.byref(u)), "fd_bandpass")
    return out, l.value, u.value


def host_water_line_mask(frequency, lines_thz, sigma_thz=0.01) -> np.ndarray:
    f = np.ascontiguousarray(frequency, np.float32)
    ln = np.ascontiguousarray(lines_thz, np.float32)
    out = np.empty(f.size, np.float32)
    _rc(load_library().thz_host_water_line_mask(f.ctypes.data, f.size, ln.ctypes.data, ln.size, sigma_thz,
                                                out.ctypes.data), "water_line_mask")
    return out


def host_wiener_filter(ref_fft, eps_rel=1e-3) -> np.ndarray:
    """ref_fft (nf, 2) f32 -> (nf, 2) complex multiplier"""
    r = np.ascontiguousarray(ref_fft, np.float32).reshape(-1, 2)
    out = np.empty_like(r)
    _rc(load_library().thz_host_wiener_filter(r.ctypes.data, r.shape[0], eps_rel, out.ctypes.data), "wiener_filter")
    return out


def host_tilt_plan(time, nx, ny, tilt_x_deg, tilt_y_deg, dx, dy):
    """-> (num_steps, new_time, insert_index (nx*ny int32))"""
    t = np.ascontiguousarray(time, np.float32)
    L = load_library()
    steps = int(L.thz_host_tilt_plan(t.ctypes.data, t.size, nx, ny, tilt_x_deg, tilt_y_deg, dx, dy, None, None))
    new_time = np.empty(t.size + 2 * steps, np.float32)
    ins = np.empty(nx * ny, np.int32)
    L.thz_host_tilt_plan(t.ctypes.data, t.size, nx, ny, tilt_x_deg, tilt_y_deg, dx, dy,
                         new_time.ctypes.data, ins.ctypes.data)
    return steps, new_time, ins


def host_psf_eval(psf: Psf, freqs):
    f = np.ascontiguousarray(freqs, np.float32)
    out = [np.empty(f.size, np.float32) for _ in range(4)]
    _rc(load_library().thz_host_psf_eval(C.byref(psf), f.ctypes.data, f.size, *[o.ctypes.data for o in out]), "psf_eval")
    return tuple(out)  # wx, wy, x0, y0


def host_filter_bank(time, cfg: DeconvCfg):
    t = np.ascontiguousarray(time, np.float32)
    filters = np.empty((cfg.n_filters, 499), np.float32)
    centers = np.empty(cfg.n_filters, np.float32)
    _rc(load_library().thz_host_filter_bank(t.ctypes.data, t.size, C.byref(cfg), filters.ctypes.data,
                                            centers.ctypes.data), "filter_bank")
    return filters, centers


def host_band_psf(psf: Psf, center_freq, dx, dy, img_rows, img_cols):
    r, c = C.c_size_t(), C.c_size_t()
    L = load_library()
    _rc(L.thz_host_band_psf(C.byref(psf), center_freq, dx, dy, img_rows, img_cols, None, C.byref(r), C.byref(c)), "band_psf")
    out = np.empty((r.value, c.value), np.float32)
    _rc(L.thz_host_band_psf(C.byref(psf), center_freq, dx, dy, img_rows, img_cols, out.ctypes.data,
                            C.byref(r), C.byref(c)), "band_psf")
    return out


def host_align_reference(scan_time, ref_time, ref_signal):
    """OpenRef alignment -> (aligned reference of the scan's length, mode 0/1/2)"""
    st, rt, rs = (np.ascontiguousarray(x, np.float32) for x in (scan_time, ref_time, ref_signal))
    out = np.empty(st.size, np.float32)
    mode = load_library().thz_host_align_reference(st.ctypes.data, st.size, rt.ctypes.data, rs.ctypes.data, rs.size,
                                                   out.ctypes.data)
    if mode < 0:
        raise ThzError(mode, "thz_host_align_reference")
    return out, mode


def host_optical_properties(sample_amp, sample_phase, ref_amp, ref_phase, freq, thickness):
    """-> (refractive index, absorption coefficient, extinction coefficient)"""
    arrs = [np.ascontiguousarray(x, np.float32) for x in (sample_amp, sample_phase, ref_amp, ref_phase, freq)]
    out = [np.empty(arrs[4].size, np.float32) for _ in range(3)]
    _rc(load_library().thz_host_optical_properties(*[a.ctypes.data for a in arrs], arrs[4].size, thickness,
                                                   *[o.ctypes.data for o in out]), "optical_properties")
    return tuple(out)


def host_arrival_plane_fit(moments):
    """ten moments of thz_arrival_plane_moments -> (status: 0 fitted, 1 skipped; TiltFit)"""
    m = np.ascontiguousarray(moments, np.float64)
    if m.size != 10:
        raise ValueError("ten moments expected")
    fit = TiltFit()
    rc = load_library().thz_host_arrival_plane_fit(m.ctypes.data, C.byref(fit))
    if rc < 0:
        raise ThzError(rc, "thz_host_arrival_plane_fit")
    return rc, fit


def host_echo_trace(x, cfg: EchoCfg):
    """thz_echo_map's selection for one host vector -> (index int32, offset f32, value f32: n_echoes each; count)"""
    a = np.ascontiguousarray(x, np.float32).ravel()
    k = max(int(cfg.n_echoes), 1)
    idx, off, val = np.full(k, -2, np.int32), np.zeros(k, np.float32), np.zeros(k, np.float32)
    n = C.c_int32()
    _rc(load_library().thz_host_echo_trace(a.ctypes.data, a.size, C.byref(cfg), idx.ctypes.data, off.ctypes.data,
                                           val.ctypes.data, C.byref(n)), "thz_host_echo_trace")
    return idx, off, val, n.value


def host_pca_components(gram, count, k):
    """thz_host_pca_components -> (rc, components f32 (k, L), eigenvalues f64 (k), total variance)"""
    g = np.ascontiguousarray(gram, np.float64)
    n = g.shape[0] if g.ndim == 2 else int(round(np.sqrt(g.size)))
    comp, ev, tot = np.zeros((max(int(k), 1), n), np.float32), np.zeros(max(int(k), 1), np.float64), C.c_double()
    rc = load_library().thz_host_pca_components(g.ctypes.data, n, int(count), int(k), comp.ctypes.data, ev.ctypes.data, C.byref(tot))
    return rc, comp, ev, tot.value


def host_cluster_update(sums, counts, previous):
    """thz_host_cluster_update -> (rc, centroids f32 (K, L)); sums f64 (K, L), counts (K), previous f32 (K, L)"""
    t = np.ascontiguousarray(sums, np.float64)
    n = np.ascontiguousarray(counts, np.uint64)
    prev = np.ascontiguousarray(previous, np.float32)
    k, width = (t.shape if t.ndim == 2 else (1, t.size))
    out = np.zeros((max(k, 1), max(width, 1)), np.float32)
    rc = load_library().thz_host_cluster_update(t.ctypes.data, n.ctypes.data, int(k), int(width), prev.ctypes.data, out.ctypes.data)
    return rc, out[:k, :width]


def host_sparse_trace(y, taps, cfg: SparseCfg):
    """thz_host_sparse_trace -> (rc, x f32 (nt), resid, nnz)"""
    a = np.ascontiguousarray(y, np.float32).ravel()
    h = np.ascontiguousarray(taps, np.float32).ravel()
    x = np.zeros(max(a.size, 1), np.float32)
    resid, nnz = C.c_float(), C.c_int32()
    rc = load_library().thz_host_sparse_trace(a.ctypes.data, a.size, h.ctypes.data, C.byref(cfg), x.ctypes.data, C.byref(resid),
                                              C.byref(nnz))
    return rc, x[:a.size], resid.value, nnz.value


def host_sparse_kernel(ref, n_taps, center):
    """thz_host_sparse_kernel -> (rc, taps f32 (n_taps), step)"""
    r = np.ascontiguousarray(ref, np.float32).ravel()
    taps, step = np.zeros(max(int(n_taps), 1), np.float32), C.c_float()
    rc = load_library().thz_host_sparse_kernel(r.ctypes.data, r.size, int(n_taps), int(center), taps.ctypes.data, C.byref(step))
    return rc, taps[:max(int(n_taps), 0)], step.value


def _wavelet_vectors(hn, gn, scale):
    """the three host vectors of a denoising call as contiguous f32; the two filters must have the same length"""
    h, g, s = (np.ascontiguousarray(v, np.float32).ravel() for v in (hn, gn, scale))
    if h.size != g.size:
        raise ValueError("hn and gn differ in length")
    return h, g, s


def host_wavelet_trace(y, hn, gn, scale, cfg: WaveletCfg):
    """thz_host_wavelet_trace -> (rc, x f32 (nt), sigma, kept)"""
    a = np.ascontiguousarray(y, np.float32).ravel()
    h, g, s = _wavelet_vectors(hn, gn, scale)
    x = np.zeros(max(a.size, 1), np.float32)
    sigma, kept = C.c_float(), C.c_int32()
    rc = load_library().thz_host_wavelet_trace(a.ctypes.data, a.size, h.ctypes.data, g.ctypes.data, s.ctypes.data, C.byref(cfg),
                                               x.ctypes.data, C.byref(sigma), C.byref(kept))
    return rc, x[:a.size], sigma.value, kept.value


def host_wavelet_filter(order):
    """thz_host_wavelet_filter -> (rc, hn f32 (Lf), gn f32 (Lf)): the Daubechies analysis pair of order 1 .. 4"""
    hn, gn, n = np.zeros(WAVELET_MAX_TAPS, np.float32), np.zeros(WAVELET_MAX_TAPS, np.float32), C.c_int(0)
    rc = load_library().thz_host_wavelet_filter(int(order), hn.ctypes.data, gn.ctypes.data, C.byref(n))
    return rc, hn[:n.value].copy(), gn[:n.value].copy()


def host_wavelet_universal(nt, n_levels):
    """thz_host_wavelet_universal -> (rc, scale f32 (n_levels)): the universal thresholds under the MAD noise estimate"""
    scale = np.zeros(max(int(n_levels), 1), np.float32)
    rc = load_library().thz_host_wavelet_universal(int(nt), int(n_levels), scale.ctypes.data)
    return rc, scale[:max(int(n_levels), 0)]


def host_unmix_prepare(endmembers):
    """thz_host_unmix_prepare -> (rc, G f32 (K, K), rd f32 (K)); endmembers f32 (K, L)"""
    e = np.ascontiguousarray(endmembers, np.float32)
    k, width = (e.shape if e.ndim == 2 else (1, e.size))
    g, rd = np.zeros((max(k, 1), max(k, 1)), np.float32), np.zeros(max(k, 1), np.float32)
    rc = load_library().thz_host_unmix_prepare(e.ctypes.data, int(k), int(width), g.ctypes.data, rd.ctypes.data)
    return rc, g, rd


def host_unmix_solve(b, g, rd, n_sweeps):
    """thz_host_unmix_solve of one pixel's projections b (K) -> (rc, a f32 (K), kkt)"""
    bb = np.ascontiguousarray(b, np.float32).ravel()
    gg, r = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(rd, np.float32)
    a, kkt = np.zeros(max(bb.size, 1), np.float32), C.c_float()
    rc = load_library().thz_host_unmix_solve(bb.ctypes.data, gg.ctypes.data, r.ctypes.data, int(bb.size), int(n_sweeps), a.ctypes.data,
                                             C.byref(kkt))
    return rc, a[:bb.size], kkt.value


def voxel_cfg_default() -> VoxelCfg:
    cfg = VoxelCfg()
    _rc(load_library().thz_voxel_cfg_default(C.byref(cfg)), "voxel_cfg_default")
    return cfg


def host_gaussian_kernel1d(sigma, radius):
    out = np.empty(2 * radius + 1, np.float32)
    _rc(load_library().thz_host_gaussian_kernel1d(sigma, radius, out.ctypes.data), "gaussian_kernel1d")
    return out


def host_select_step(hist, k):
    """one level of the radix select -> (bin, rank inside the bin)"""
    h = np.ascontiguousarray(hist, np.uint64)
    b, r = C.c_int(), C.c_uint64()
    _rc(load_library().thz_host_select_step(h.ctypes.data, h.size, int(k), C.byref(b), C.byref(r)), "select_step")
    return b.value, r.value


def host_select_value(bin0, bin1, bin2) -> float:
    return float(load_library().thz_host_select_value(bin0, bin1, bin2))


def chain_cfg_default(time) -> ChainCfg:
    t = np.ascontiguousarray(time, np.float32)
    cfg = ChainCfg()
    _rc(load_library().thz_chain_cfg_default(t.ctypes.data, t.size, C.byref(cfg)), "chain_cfg_default")
    return cfg


def _pack_rois(polys):
    """list of (n, 2) vertex arrays -> (n_rois, size_t counts, u64 vertices) for thz_*_set_rois"""
    polys = [np.ascontiguousarray(p, np.uint64).reshape(-1, 2) for p in polys]
    counts = (_SZ * max(len(polys), 1))(*[p.shape[0] for p in polys])
    flat = np.concatenate(polys).ravel() if polys else np.zeros(0, np.uint64)
    return len(polys), counts, np.ascontiguousarray(flat, np.uint64)


def _roi_out(nt_out, want):
    nf = nt_out // 2 + 1
    sizes = dict(signal_fft=nf, phase_fft=nf, signal=nt_out, roi_data=nt_out)
    want = list(sizes) if want is None else want
    res = {k: np.empty(sizes[k], np.float32) for k in want}
    cnt = C.c_uint32()
    ro = RoiOut(count=C.addressof(cnt), **{k: v.ctypes.data for k, v in res.items()})
    return res, cnt, ro


class Session:
    """thz_session: resident cube + whole-chain recompute"""

    def __init__(self, eng: "Engine", nx, ny, time, dx=1.0, dy=1.0):
        self.eng, self.nx, self.ny = eng, nx, ny
        t = np.ascontiguousarray(time, np.float32)
        self.nt = t.size
        self.h = _P()
        eng._check(eng.lib.thz_session_create(eng.ctx, nx, ny, t.size, t.ctypes.data, dx, dy, C.byref(self.h)))

    def close(self):
        if self.h:
            self.eng.lib.thz_session_destroy(self.h)
            self.h = None

    def upload(self, cube, subtract_bias=True):
        """cube: host (nx, ny, nt) array, or None when THZ_BUF_RAW was filled on the device"""
        c = None if cube is None else np.ascontiguousarray(cube, np.float32)
        if c is not None and c.size != self.nx * self.ny * self.nt:
            raise ValueError(f"cube has {c.size} samples, the session {self.nx * self.ny * self.nt}")
        self.eng._check(self.eng.lib.thz_session_upload(self.h, c.ctypes.data if c is not None else None, int(subtract_bias)))

    def recompute(self, cfg: ChainCfg, start_stage: int = 1):
        """UpdateType::Filter(start_stage): 1 = everything, 6 / 7 = from the resident spectrum"""
        self.eng._check(self.eng.lib.thz_session_recompute_from(self.h, C.byref(cfg), int(start_stage)))

    def set_fd_filters(self, real_mask=None, cmask=None):
        """further Frequency-domain plugins: K14 (real, nf) and K13 (complex, (nf, 2))"""
        r = None if real_mask is None else np.ascontiguousarray(real_mask, np.float32)
        c = None if cmask is None else np.ascontiguousarray(cmask, np.float32)
        nf = r.size if r is not None else (c.size // 2 if c is not None else 0)
        self.eng._check(self.eng.lib.thz_session_set_fd_filters(self.h, r.ctypes.data if r is not None else None,
                                                                c.ctypes.data if c is not None else None, nf))

    def set_rois(self, polys):
        """regions of interest: list of (n, 2) integer vertex arrays (x, y) in raw-grid pixels; [] removes them"""
        n, counts, flat = _pack_rois(polys)
        self.eng._check(self.eng.lib.thz_session_set_rois(self.h, n, counts, flat.ctypes.data if flat.size else None))

    def roi(self, index, want=None):
        """per-region vectors of the last recompute -> dict (+ 'count')"""
        res, cnt, ro = _roi_out(self.nt_out, want)
        self.eng._check(self.eng.lib.thz_session_roi(self.h, index, C.byref(ro)))
        res["count"] = cnt.value
        return res

    def deconvolve(self, psf, cfg, abort=None, progress=None):
        """the chain's Deconvolution stage on the last recompute's output -> status (0 applied, 1 skipped)"""
        rc = self.eng.lib.thz_session_deconvolve(self.h, C.byref(psf), C.byref(cfg),
                                                 C.byref(abort) if abort is not None else None,
                                                 C.byref(progress) if progress is not None else None)
        if rc < 0:
            self.eng._check(rc)
        return rc

    @property
    def nt_out(self):
        return int(self.eng.lib.thz_session_nt_out(self.h))

    def grid(self):
        """(nx, ny, dx, dy) of the outputs: the raw grid, or the block grid behind a scaling stage"""
        nx, ny, dx, dy = _SZ(), _SZ(), C.c_float(), C.c_float()
        self.eng._check(self.eng.lib.thz_session_grid(self.h, C.byref(nx), C.byref(ny), C.byref(dx), C.byref(dy)))
        return nx.value, ny.value, dx.value, dy.value

    def time_out(self):
        t = np.empty(self.nt_out, np.float32)
        self.eng._check(self.eng.lib.thz_session_time_out(self.h, t.ctypes.data))
        return t

    def voxels(self, cfg: "VoxelCfg", max_instances=VOXEL_MAX_INSTANCES, scaling=1, orig_dims=None, capacity=None):
        """update_intensity_image's 3-D part -> (instances, threshold, (cube_width, cube_height, cube_depth))"""
        orig = orig_dims or (self.nx, self.ny, self.nt_out)
        n, thr = C.c_uint64(), C.c_float()
        dims = np.zeros(3, np.float32)
        if capacity is None:   # count first
            self.eng._check(self.eng.lib.thz_session_voxels(self.h, C.byref(cfg), max_instances, scaling, orig[0],
                                                            orig[1], orig[2], None, 0, C.byref(n), C.byref(thr),
                                                            dims.ctypes.data))
            capacity = n.value
        out = np.zeros(capacity, VOXEL_INSTANCE)
        self.eng._check(self.eng.lib.thz_session_voxels(self.h, C.byref(cfg), max_instances, scaling, orig[0], orig[1],
                                                        orig[2], out.ctypes.data if capacity else None, capacity,
                                                        C.byref(n), C.byref(thr), dims.ctypes.data))
        return out[:min(n.value, capacity)], thr.value, tuple(float(x) for x in dims)

    def peak_map(self, which=0, mode=PEAK_ABS):
        """arrival-time maps of THZ_BUF_RAW / THZ_BUF_DATA -> (index int32, offset f32, value f32), each (gx, gy)"""
        self.eng._check(self.eng.lib.thz_session_peak_map(self.h, int(which), int(mode)))
        gx, gy = self._cube_pix(which)
        return tuple(self.download(b, npix=gx * gy).reshape(gx, gy) for b in (BUF_PEAK_INDEX, BUF_PEAK_OFFSET, BUF_PEAK_VALUE))

    def estimate_tilt(self, which=0, mode=PEAK_ABS, rel_threshold=0.25):
        """map + moments + fit -> (status: 0 fitted, 1 skipped; TiltFit)"""
        fit = TiltFit()
        rc = self.eng.lib.thz_session_estimate_tilt(self.h, int(which), int(mode), float(rel_threshold), C.byref(fit))
        if rc < 0:
            self.eng._check(rc)
        return rc, fit

    def optical_maps(self, ref_amp, ref_phase, cfg: "OpticalCfg", thickness=None):
        """thz_session_optical_maps on the last recompute's amplitudes and phases -> (n, alpha, kappa: (n_bands, gx, gy)
        f32; wraps (gx, gy) int32; slope (gx, gy) f32).  thickness: device pointer / DevBuf of one f32 per pixel, or None
        for cfg.thickness everywhere"""
        ra, rp = (np.ascontiguousarray(x, np.float32) for x in (ref_amp, ref_phase))
        if ra.size != rp.size:
            raise ValueError("reference amplitudes and phases differ in length")
        self.eng._check(self.eng.lib.thz_session_optical_maps(self.h, ra.ctypes.data, rp.ctypes.data, ra.size, C.byref(cfg),
                                                              _dp(thickness)))
        gx, gy = self.grid()[:2]
        nb = int(cfg.n_bands)
        bands = [self.download(b, npix=nb * gx * gy).reshape(nb, gx, gy) if nb else np.empty((0, gx, gy), np.float32)
                 for b in (BUF_OPT_N, BUF_OPT_ALPHA, BUF_OPT_KAPPA)]
        return (*bands, self.download(BUF_OPT_WRAPS, npix=gx * gy).reshape(gx, gy),
                self.download(BUF_OPT_SLOPE, npix=gx * gy).reshape(gx, gy))

    def echo_map(self, which, cfg: "EchoCfg"):
        """thz_session_echo_map of THZ_BUF_RAW / THZ_BUF_DATA -> (index int32, offset f32, value f32: (n_echoes, gx, gy);
        count int32 (gx, gy))"""
        self.eng._check(self.eng.lib.thz_session_echo_map(self.h, int(which), C.byref(cfg)))
        gx, gy = self._cube_pix(which)
        k = int(cfg.n_echoes)
        self._echo_grid = (k, gx, gy)
        return (*(self.download(b, npix=k * gx * gy).reshape(k, gx, gy) for b in (BUF_ECHO_INDEX, BUF_ECHO_OFFSET, BUF_ECHO_VALUE)),
                self.download(BUF_ECHO_COUNT, npix=gx * gy).reshape(gx, gy))

    def layer_map(self, cfg: "LayerCfg"):
        """thz_session_layer_map on the last echo_map -> (thickness, delay), each (rows, gx, gy) f32: rows = n_echoes - 1
        between consecutive pulses, 1 against a fixed arrival"""
        self.eng._check(self.eng.lib.thz_session_layer_map(self.h, C.byref(cfg)))
        k, gx, gy = self._echo_grid
        rows = k - 1 if cfg.mode == LAYER_BETWEEN else 1
        return tuple(self.download(b, npix=rows * gx * gy).reshape(rows, gx, gy) for b in (BUF_LAYER_THICKNESS, BUF_LAYER_DELAY))

    def _cube_pix(self, which):
        """(gx, gy) of the cube `which` names for the per-trace maps: the raw grid, the last recompute's, or the grid of
        the cube the spike trains were taken of"""
        if which == BUF_SPARSE:
            return self._sparse_grid[:2]
        if which == BUF_DENOISED:
            return self._denoise_grid[:2]
        return (self.nx, self.ny) if which == BUF_RAW else self.grid()[:2]

    def _trace_cube(self, which):
        """(gx, gy, nt) of the cube a per-trace stage reads: THZ_BUF_RAW, THZ_BUF_DATA or the denoised traces"""
        if which == BUF_DENOISED:
            return self._denoise_grid
        return (self.nx, self.ny, self.nt) if which == BUF_RAW else (*self.grid()[:2], self.nt_out)

    def sparse_deconv(self, which, taps, cfg: "SparseCfg"):
        """thz_session_sparse_deconv of THZ_BUF_RAW / THZ_BUF_DATA / THZ_BUF_DENOISED -> (x f32 (gx, gy, nt), resid f32
        (gx, gy), nnz int32 (gx, gy)); the spike trains stay resident as THZ_BUF_SPARSE"""
        h = np.ascontiguousarray(taps, np.float32).ravel()
        self.eng._check(self.eng.lib.thz_session_sparse_deconv(self.h, int(which), h.ctypes.data, C.byref(cfg)))
        gx, gy, nts = self._trace_cube(which)
        self._sparse_grid = (gx, gy, nts)
        return (self.download(BUF_SPARSE).reshape(gx, gy, -1), self.download(BUF_SPARSE_RESID).reshape(gx, gy),
                self.download(BUF_SPARSE_NNZ).reshape(gx, gy))

    def wavelet_denoise(self, which, hn, gn, scale, cfg: "WaveletCfg"):
        """thz_session_wavelet_denoise of THZ_BUF_RAW / THZ_BUF_DATA -> (x f32 (gx, gy, nt), sigma f32 (gx, gy), kept int32
        (gx, gy)); the denoised traces stay resident as THZ_BUF_DENOISED"""
        h, g, s = _wavelet_vectors(hn, gn, scale)
        self.eng._check(self.eng.lib.thz_session_wavelet_denoise(self.h, int(which), h.ctypes.data, g.ctypes.data, s.ctypes.data,
                                                                 C.byref(cfg)))
        gx, gy, nts = self._trace_cube(which)
        self._denoise_grid = (gx, gy, nts)
        return (self.download(BUF_DENOISED).reshape(gx, gy, -1), self.download(BUF_DENOISE_SIGMA).reshape(gx, gy),
                self.download(BUF_DENOISE_KEPT).reshape(gx, gy))

    def _pca_pix(self, which):
        gx, gy = (self.nx, self.ny) if which == BUF_RAW else self.grid()[:2]
        return gx, gy

    def pca(self, which, cfg: "PcaCfg"):
        """thz_session_pca -> (eigenvalues f64 (K), total variance, count, scores f32 (K, gx, gy), components f32 (K, L),
        mean f32 (L))"""
        out = PcaOut()
        self.eng._check(self.eng.lib.thz_session_pca(self.h, int(which), C.byref(cfg), C.byref(out)))
        gx, gy = self._pca_pix(which)
        k, n = int(cfg.n_components), int(cfg.count)
        return (np.array(out.eigenvalues[:k]), out.total_variance, out.count,
                self.download(BUF_PCA_SCORES, npix=k * gx * gy).reshape(k, gx, gy),
                self.download(BUF_PCA_COMPONENTS, npix=k * n).reshape(k, n), self.download(BUF_PCA_MEAN, npix=n))

    def pca_sums(self, which, cfg: "PcaCfg"):
        """thz_session_pca_sums -> (sum f64 (L), count)"""
        s, n = np.zeros(int(cfg.count), np.float64), C.c_uint64()
        self.eng._check(self.eng.lib.thz_session_pca_sums(self.h, int(which), C.byref(cfg), s.ctypes.data, C.byref(n)))
        return s, n.value

    def pca_gram(self, which, cfg: "PcaCfg", mu=None):
        """thz_session_pca_gram -> f64 (L, L)"""
        n = int(cfg.count)
        g = np.zeros((n, n), np.float64)
        m = None if mu is None else np.ascontiguousarray(mu, np.float32)
        self.eng._check(self.eng.lib.thz_session_pca_gram(self.h, int(which), C.byref(cfg), None if m is None else m.ctypes.data,
                                                          g.ctypes.data))
        return g

    def pca_project(self, which, cfg: "PcaCfg", mu, components):
        """thz_session_pca_project -> scores f32 (K, gx, gy); fills the three resident buffers"""
        m = None if mu is None else np.ascontiguousarray(mu, np.float32)
        v = np.ascontiguousarray(components, np.float32)
        self.eng._check(self.eng.lib.thz_session_pca_project(self.h, int(which), C.byref(cfg), None if m is None else m.ctypes.data,
                                                             v.ctypes.data))
        gx, gy = self._pca_pix(which)
        k = int(cfg.n_components)
        return self.download(BUF_PCA_SCORES, npix=k * gx * gy).reshape(k, gx, gy)

    def cluster(self, which, cfg: "ClusterCfg"):
        """thz_session_cluster -> (ClusterOut, labels int32 (npix), dist2 f32 (npix), centroids f32 (K, L)); npix: the
        pixels of the matrix, flattened"""
        out = ClusterOut()
        self.eng._check(self.eng.lib.thz_session_cluster(self.h, int(which), C.byref(cfg), C.byref(out)))
        return (out,) + self.cluster_buffers(which, cfg)

    def cluster_buffers(self, which, cfg: "ClusterCfg", npix=None):
        """the three resident buffers of the last call -> (labels, dist2, centroids)"""
        if npix is None:
            if which == BUF_PCA_SCORES:
                raise ValueError("npix is needed for BUF_PCA_SCORES")
            gx, gy = self._pca_pix(which)
            npix = gx * gy
        k, n = int(cfg.n_clusters), int(cfg.count)
        return (self.download(BUF_CLUSTER_LABELS, npix=npix), self.download(BUF_CLUSTER_DIST, npix=npix),
                self.download(BUF_CLUSTER_CENTROIDS, npix=k * n).reshape(k, n))

    def cluster_step(self, which, cfg: "ClusterCfg", centroids, want_sums=True):
        """thz_session_cluster_step with cfg.n_clusters rows of centroids -> (sums f64 (K, L) or None, counts (K),
        inertia, changed, farthest)"""
        m = np.ascontiguousarray(centroids, np.float32)
        k, n = int(cfg.n_clusters), int(cfg.count)
        assert m.size == k * n
        sums = np.zeros((k, n), np.float64) if want_sums else None
        counts, inertia, changed, far = np.zeros(k, np.uint64), C.c_double(), C.c_uint64(), C.c_uint64()
        self.eng._check(self.eng.lib.thz_session_cluster_step(self.h, int(which), C.byref(cfg), m.ctypes.data,
                                                              None if sums is None else sums.ctypes.data, counts.ctypes.data,
                                                              C.byref(inertia), C.byref(changed), C.byref(far)))
        return sums, counts, inertia.value, changed.value, far.value

    def cluster_row(self, which, cfg: "ClusterCfg", pixel):
        """thz_session_cluster_row -> f32 (count)"""
        row = np.zeros(int(cfg.count), np.float32)
        self.eng._check(self.eng.lib.thz_session_cluster_row(self.h, int(which), C.byref(cfg), int(pixel), row.ctypes.data))
        return row

    def unmix(self, which, cfg: "UnmixSessionCfg"):
        """thz_session_unmix -> (abundances f32 (K, gx, gy), projections f32 (K, gx, gy), resid f32 (gx, gy), kkt f32
        (gx, gy)); the four stay resident as THZ_BUF_UNMIX_*"""
        self.eng._check(self.eng.lib.thz_session_unmix(self.h, int(which), C.byref(cfg)))
        gx, gy = self._pca_pix(which)
        k = int(cfg.n_endmembers)
        return (self.download(BUF_UNMIX_ABUNDANCE, npix=k * gx * gy).reshape(k, gx, gy),
                self.download(BUF_UNMIX_PROJ, npix=k * gx * gy).reshape(k, gx, gy),
                self.download(BUF_UNMIX_RESID, npix=gx * gy).reshape(gx, gy), self.download(BUF_UNMIX_KKT, npix=gx * gy).reshape(gx, gy))

    def plot(self, px, py, want=None):
        """UpdateType::Plot copy-out for pixel (px, py) -> dict of host vectors"""
        nto = self.nt_out
        nf = nto // 2 + 1
        sizes = dict(signal=self.nt, signal_fft=nf, phase_fft=nf, filtered_signal=nto, filtered_signal_fft=nf,
                     filtered_phase_fft=nf, avg_signal=nto, avg_signal_fft=nf, avg_phase_fft=nf)
        want = list(sizes) if want is None else want
        res = {k: np.empty(sizes[k], np.float32) for k in want}
        po = PlotOut(**{k: v.ctypes.data for k, v in res.items()})
        self.eng._check(self.eng.lib.thz_session_plot(self.h, px, py, C.byref(po)))
        return res

    def download(self, which, pix0=0, npix=None):
        nto = self.nt_out
        nf = nto // 2 + 1
        per = {BUF_RAW: (self.nt,), BUF_FFT: (nf, 2), BUF_AMPLITUDES: (nf,), BUF_PHASES: (nf,), BUF_DATA: (nto,),
               BUF_IMG: (), BUF_OPACITY: (nto,)}
        if which in (BUF_PEAK_INDEX, BUF_PEAK_OFFSET, BUF_PEAK_VALUE):  # npix: the mapped grid's, from the caller
            out = np.empty(npix, np.int32 if which == BUF_PEAK_INDEX else np.float32)
        elif BUF_OPT_N <= which <= BUF_OPT_SLOPE:  # npix: entries of the last call's (band, pixel) array, from the caller
            out = np.empty(npix, np.int32 if which == BUF_OPT_WRAPS else np.float32)
        elif BUF_ECHO_INDEX <= which <= BUF_LAYER_DELAY:  # npix: entries of the last call's (row, pixel) array, likewise
            out = np.empty(npix, np.int32 if which in (BUF_ECHO_INDEX, BUF_ECHO_COUNT) else np.float32)
        elif BUF_PCA_SCORES <= which <= BUF_PCA_MEAN:  # npix: entries of the flattened array, likewise
            out = np.empty(npix, np.float32)
        elif BUF_CLUSTER_LABELS <= which <= BUF_CLUSTER_CENTROIDS:  # npix: entries of the flattened array, likewise
            out = np.empty(npix, np.int32 if which == BUF_CLUSTER_LABELS else np.float32)
        elif BUF_UNMIX_ABUNDANCE <= which <= BUF_UNMIX_KKT:  # npix: entries of the flattened array, likewise
            out = np.empty(npix, np.float32)
        elif BUF_SPARSE <= which <= BUF_SPARSE_NNZ:  # pix0 / npix: pixels of the grid the spike trains were taken of
            gx, gy, nts = getattr(self, "_sparse_grid", (0, 0, 0))
            npix = max(gx * gy - pix0, 0) if npix is None else npix
            out = np.empty((npix, nts) if which == BUF_SPARSE else npix, np.int32 if which == BUF_SPARSE_NNZ else np.float32)
        elif BUF_DENOISED <= which <= BUF_DENOISE_KEPT:  # likewise the grid the denoised traces were taken of
            gx, gy, nts = getattr(self, "_denoise_grid", (0, 0, 0))
            npix = max(gx * gy - pix0, 0) if npix is None else npix
            out = np.empty((npix, nts) if which == BUF_DENOISED else npix, np.int32 if which == BUF_DENOISE_KEPT else np.float32)
        elif which in per:
            gx, gy = (self.nx, self.ny) if which == BUF_RAW else self.grid()[:2]
            npix = gx * gy - pix0 if npix is None else npix
            out = np.empty((npix,) + per[which], np.float32)
        else:
            out = np.empty((nf, 2) if which == BUF_AVG_FFT else (nf,), np.float32)
            pix0, npix = 0, 1
        self.eng._check(self.eng.lib.thz_session_download(self.h, which, pix0, npix, out.ctypes.data))
        return out


GATHER_SMALL, GATHER_TIME, GATHER_ALL = range(3)
GROUP_ID_BYTES = 128


def host_slab(nx: int, world: int, rank: int):
    """(x0, n) rows of `rank`: the x-slab partition of include/thzgpu.h (thz_host_slab)"""
    x0, n = _SZ(), _SZ()
    _rc(load_library().thz_host_slab(nx, world, rank, C.byref(x0), C.byref(n)), "host_slab")
    return x0.value, n.value


def group_unique_id() -> bytes:
    buf = C.create_string_buffer(GROUP_ID_BYTES)
    _rc(load_library().thz_group_unique_id(buf), "group_unique_id")
    return buf.raw


class Group:
    """thz_group: the members of a multi-GPU tiling driven by this process.  Group(devices=[0, 1, ...]) is one
    process over n devices; Group(device=d, rank=r, world=w, uid=...) one member of a process-per-GPU launch."""

    def __init__(self, devices=None, device=None, rank=0, world=1, uid=None):
        self.lib = load_library()
        self.h = _P()
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            rc = self.lib.thz_group_create(arr, len(devices), C.byref(self.h))
        else:
            rc = self.lib.thz_group_create_rank(device, rank, world, uid, C.byref(self.h))
        if rc != THZ_OK:
            raise ThzError(rc, "thz_group_create failed (no HIP device, RCCL missing, or a bad device list)")
        self.world = self.lib.thz_group_world(self.h)
        self.ranks = [self.lib.thz_group_rank(self.h, i) for i in range(self.lib.thz_group_local_count(self.h))]

    def _check(self, rc):
        if rc != THZ_OK:
            raise ThzError(rc, self.lib.thz_group_last_error(self.h).decode())

    def engine(self, i: int) -> "Engine":
        """Engine view of local member i's context (owned by the group: do not close it)"""
        e = Engine.__new__(Engine)
        e.lib, e.ctx, e._bufs = self.lib, _P(self.lib.thz_group_ctx(self.h, i)), []
        return e

    def all_reduce_sum(self, bufs, count):
        arr = (_P * len(bufs))(*[_dp(b) for b in bufs])
        self._check(self.lib.thz_group_all_reduce_sum(self.h, arr, count))

    def all_reduce_u64(self, bufs, count):
        arr = (_P * len(bufs))(*[_dp(b) for b in bufs])
        self._check(self.lib.thz_group_all_reduce_u64(self.h, arr, count))

    def gather(self, send, counts, recv_root):
        arr = (_P * len(send))(*[_dp(b) for b in send])
        cnt = (_SZ * len(counts))(*counts)
        self._check(self.lib.thz_group_gather(self.h, arr, cnt, _dp(recv_root)))

    def sync(self):
        self._check(self.lib.thz_group_sync(self.h))

    def close(self):
        if self.h:
            self.lib.thz_group_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class GroupSession:
    """thz_group_session: one x-slab session per member, C2 / C1 inside the library"""

    def __init__(self, group: Group, nx, ny, time, dx=1.0, dy=1.0):
        self.g, self.nx, self.ny = group, nx, ny
        t = np.ascontiguousarray(time, np.float32)
        self.nt = t.size
        self.h = _P()
        group._check(group.lib.thz_group_session_create(group.h, nx, ny, t.size, t.ctypes.data, dx, dy, C.byref(self.h)))

    def member(self, i) -> "Session":
        """Session view of local member i's slab session (owned by the group session: do not close it)"""
        s = Session.__new__(Session)
        x0, n = host_slab(self.nx, self.g.world, self.g.ranks[i])
        s.eng, s.nx, s.ny, s.nt = self.g.engine(i), n, self.ny, self.nt
        s.h = _P(self.g.lib.thz_group_session_member(self.h, i))
        return s

    def member_buffer(self, i, which) -> int:
        """device pointer of a buffer of local member i's slab session"""
        return self.g.lib.thz_session_buffer(_P(self.g.lib.thz_group_session_member(self.h, i)), which) or 0

    def upload(self, cube=None, subtract_bias=True):
        c = None if cube is None else np.ascontiguousarray(cube, np.float32)
        self.g._check(self.g.lib.thz_group_session_upload(self.h, c.ctypes.data if c is not None else None, int(subtract_bias)))

    def recompute(self, cfg: ChainCfg, start_stage=1, gather=GATHER_SMALL):
        self.g._check(self.g.lib.thz_group_session_recompute(self.h, C.byref(cfg), int(start_stage), int(gather)))

    def set_rois(self, polys):
        """regions of interest over the whole grid (every rank sets the same ones)"""
        n, counts, flat = _pack_rois(polys)
        self.g._check(self.g.lib.thz_group_session_set_rois(self.h, n, counts, flat.ctypes.data if flat.size else None))

    def roi(self, index, want=None, nt_out=None):
        """per-region vectors of the last recompute -> dict (+ 'count'); sized like the chain's output traces (a
        tilt extends them) unless nt_out says otherwise"""
        res, cnt, ro = _roi_out(self.member(0).nt_out if nt_out is None else nt_out, want)
        self.g._check(self.g.lib.thz_group_session_roi(self.h, index, C.byref(ro)))
        res["count"] = cnt.value
        return res

    def deconvolve(self, psf, cfg, abort=None, progress=None):
        """band-parallel Deconvolution stage over the group -> status (0 applied, 1 skipped)"""
        rc = self.g.lib.thz_group_session_deconvolve(self.h, C.byref(psf), C.byref(cfg),
                                                     C.byref(abort) if abort is not None else None,
                                                     C.byref(progress) if progress is not None else None)
        if rc < 0:
            self.g._check(rc)
        return rc

    def grid(self):
        """(nx, ny) of the outputs' whole grid: the raw one, or the block grid behind a scaling stage"""
        nx, ny = _SZ(), _SZ()
        self.g._check(self.g.lib.thz_group_session_grid(self.h, C.byref(nx), C.byref(ny)))
        return nx.value, ny.value

    def download(self, which, nt_out=None):
        """gathered buffer of rank 0 (whole grid) or a pixel-mean vector; traces and spectra are sized like the
        chain's output traces (a tilt extends them) unless nt_out says otherwise"""
        nto = self.member(0).nt_out if nt_out is None else nt_out
        nf = nto // 2 + 1
        per = {BUF_FFT: (nf, 2), BUF_AMPLITUDES: (nf,), BUF_PHASES: (nf,), BUF_DATA: (nto,), BUF_IMG: ()}
        if which in per:
            gx, gy = self.grid()
            out = np.empty((gx * gy,) + per[which], np.float32)
            self.g._check(self.g.lib.thz_group_session_download(self.h, which, 0, gx * gy, out.ctypes.data))
        else:
            out = np.empty((nf, 2) if which == BUF_AVG_FFT else (nf,), np.float32)
            self.g._check(self.g.lib.thz_group_session_download(self.h, which, 0, 1, out.ctypes.data))
        return out

    def estimate_tilt(self, which=0, mode=PEAK_ABS, rel_threshold=0.25):
        """thz_session_estimate_tilt over the whole grid (collective) -> (status, TiltFit), the same on every rank"""
        fit = TiltFit()
        rc = self.g.lib.thz_group_session_estimate_tilt(self.h, int(which), int(mode), float(rel_threshold), C.byref(fit))
        if rc < 0:
            self.g._check(rc)
        return rc, fit

    def peak_maps(self, npix):
        """the gathered whole-grid maps of the last estimate_tilt on rank 0 -> (index, offset, value), npix each"""
        out = []
        for which, dt in ((BUF_PEAK_INDEX, np.int32), (BUF_PEAK_OFFSET, np.float32), (BUF_PEAK_VALUE, np.float32)):
            p = self.g.lib.thz_group_session_peak_result(self.h, which)
            if not p:
                raise ThzError(-4, "the arrival-time maps are not on this process")
            a = np.empty(npix, dt)
            eng = self.g.engine(self.g.ranks.index(0))
            eng._check(eng.lib.thz_memcpy_d2h(eng.ctx, a.ctypes.data, _P(p), a.nbytes))
            out.append(a)
        return tuple(out)

    def voxels(self, cfg: "VoxelCfg", max_instances=VOXEL_MAX_INSTANCES, scaling=1, orig_dims=None, capacity=None):
        """the 3-D tab's instances over the WHOLE grid (collective: every rank calls it) ->
        (instances, threshold, (cube_width, cube_height, cube_depth), count).  Only the process that drives rank 0
        receives instances; elsewhere the array is empty.  count is the whole grid's."""
        lib = self.g.lib
        orig = orig_dims or (self.nx, self.ny, self.member(0).nt_out)
        root = 0 in self.g.ranks
        n, thr = C.c_uint64(), C.c_float()
        dims = np.zeros(3, np.float32)
        if capacity is None:   # count first
            self.g._check(lib.thz_group_session_voxels(self.h, C.byref(cfg), max_instances, scaling, orig[0], orig[1],
                                                       orig[2], None, 0, C.byref(n), C.byref(thr), dims.ctypes.data))
            capacity = n.value
        out = np.zeros(capacity if root else 0, VOXEL_INSTANCE)
        self.g._check(lib.thz_group_session_voxels(self.h, C.byref(cfg), max_instances, scaling, orig[0], orig[1],
                                                   orig[2], out.ctypes.data if out.size else None, out.size,
                                                   C.byref(n), C.byref(thr), dims.ctypes.data))
        return out[:min(n.value, out.size)], thr.value, tuple(float(x) for x in dims), n.value

    def close(self):
        if self.h:
            self.g.lib.thz_group_session_destroy(self.h)
            self.h = None


class DevBuf:
    """A device allocation owned through thz_malloc/thz_free."""

    def __init__(self, eng: "Engine", nbytes: int):
        self.eng = eng
        self.nbytes = int(nbytes)
        p = _P()
        eng._check(eng.lib.thz_malloc(eng.ctx, C.byref(p), self.nbytes))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            self.eng.lib.thz_free(self.eng.ctx, self.ptr)
            self.ptr = None

    def upload(self, a: np.ndarray) -> "DevBuf":
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        self.eng._check(self.eng.lib.thz_memcpy_h2d(self.eng.ctx, self.ptr, a.ctypes.data, a.nbytes))
        return self

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        self.eng._check(self.eng.lib.thz_memcpy_d2h(self.eng.ctx, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def zero(self):
        self.eng._check(self.eng.lib.thz_memset(self.eng.ctx, self.ptr, 0, self.nbytes))
        return self


def _dp(x) -> Optional[int]:
    """device pointer of a DevBuf / int / None"""
    if x is None:
        return None
    if isinstance(x, DevBuf):
        return x.ptr
    return int(x)


class Engine:
    """One thz_ctx.  Methods are 1:1 with the C entry points."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.ctx = _P()
        rc = self.lib.thz_create(device, C.byref(self.ctx))
        if rc != THZ_OK:
            raise ThzError(rc, "thz_create failed (no HIP device?)")
        self._bufs = []

    # -- helpers
    def _check(self, rc: int):
        if rc != THZ_OK:
            raise ThzError(rc, self.lib.thz_last_error(self.ctx).decode())

    def release_scratch(self):
        """frees the device scratch the context keeps between calls (thz_release_scratch)"""
        self._check(self.lib.thz_release_scratch(self.ctx))

    def close(self):
        if self.ctx:
            for b in self._bufs:
                b.free()
            self._bufs = []
            self.lib.thz_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def alloc(self, nbytes: int) -> DevBuf:
        b = DevBuf(self, nbytes)
        self._bufs.append(b)
        return b

    def to_device(self, a: np.ndarray) -> DevBuf:
        a = np.ascontiguousarray(a)
        return self.alloc(max(a.nbytes, 4)).upload(a)

    def empty(self, shape, dtype=np.float32) -> DevBuf:
        return self.alloc(max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 4))

    def sync(self):
        self._check(self.lib.thz_sync(self.ctx))

    @property
    def stream(self) -> int:
        return self.lib.thz_stream(self.ctx) or 0

    # -- plan
    def set_time_axis(self, time: np.ndarray):
        t = np.ascontiguousarray(time, np.float32)
        self._check(self.lib.thz_set_time_axis(self.ctx, t.ctypes.data, t.size))
        self.nt = int(self.lib.thz_nt(self.ctx))
        self.nf = int(self.lib.thz_nf(self.ctx))

    def set_kernel_family(self, family: int):
        """0 = auto (F kernels where available), 1 = G kernels everywhere"""
        self._check(self.lib.thz_set_kernel_family(self.ctx, int(family)))

    def frequency(self) -> np.ndarray:
        f = np.empty(self.nf, np.float32)
        self._check(self.lib.thz_get_frequency(self.ctx, f.ctypes.data))
        return f

    def kernel_variant(self) -> str:
        return self.lib.thz_kernel_variant(self.ctx).decode()

    # -- stages
    def fft(self, npix, d_in, win_a=None, win_b=None, data_out=None, fft=None, amp=None,
            phase=None, fd_mask=None):
        self._check(self.lib.thz_fft(self.ctx, npix, _dp(d_in), _dp(win_a), _dp(win_b),
                                     _dp(data_out), _dp(fft), _dp(amp), _dp(phase), _dp(fd_mask)))

    def apply_fd_mask(self, npix, fft, amp, mask):
        self._check(self.lib.thz_apply_fd_mask(self.ctx, npix, _dp(fft), _dp(amp), _dp(mask)))

    def apply_fd_cmask(self, npix, fft, amp, cmask):
        self._check(self.lib.thz_apply_fd_cmask(self.ctx, npix, _dp(fft), _dp(amp), _dp(cmask)))

    def ifft(self, npix, fft, td_win, data_out, img=None):
        self._check(self.lib.thz_ifft(self.ctx, npix, _dp(fft), _dp(td_win), _dp(data_out), _dp(img)))

    def pipeline_ex(self, npix, raw, pre_win, fd_mask, fd_cmask, post_win, fft, amp, phase, data_out, img=None, sums=None, band=None):
        """thz_pipeline_ex: the fused chain with a complex per-bin multiplier and / or in-launch pixel sums; band = (lo, hi):
        the bins outside are zero in fd_mask (thz_host_fd_bandpass's index range)"""
        io = PipelineIo(*[_dp(x) for x in (raw, pre_win, fd_mask, fd_cmask, post_win, fft, amp, phase, data_out, img, sums)],
                        *(band if band else (0, 0)))
        self._check(self.lib.thz_pipeline_ex(self.ctx, npix, C.byref(io)))

    def pipeline_tilted(self, npix, src, nt_in, taper, insert_index, pre_win, fd_mask, fd_cmask, post_win, fft, amp, phase,
                        data_out, img=None, sums=None, src_sum=None):
        """thz_pipeline_tilted: pipeline_ex on (npix, nt_in) traces that are re-laid on the context's extended axis while
        they are read (taper, insert_index as for tilt_apply); src_sum: (nt) sums of the re-laid, tapered samples"""
        io = PipelineIo(*[_dp(x) for x in (None, pre_win, fd_mask, fd_cmask, post_win, fft, amp, phase, data_out, img, sums)], 0, 0)
        ts = TiltSrc(_dp(src), nt_in, _dp(taper), _dp(insert_index), _dp(src_sum))
        self._check(self.lib.thz_pipeline_tilted(self.ctx, npix, C.byref(io), C.byref(ts)))

    def pipeline(self, npix, raw, pre_win, fd_mask, post_win, fft, amp, phase, data_out, img):
        self._check(self.lib.thz_pipeline(self.ctx, npix, _dp(raw), _dp(pre_win), _dp(fd_mask),
                                          _dp(post_win), _dp(fft), _dp(amp), _dp(phase),
                                          _dp(data_out), _dp(img)))

    def apply_td_window(self, npix, d_in, win, d_out):
        self._check(self.lib.thz_apply_td_window(self.ctx, npix, _dp(d_in), _dp(win), _dp(d_out)))

    def peak_map(self, npix, nt, data, mode, index=None, offset=None, value=None):
        """per-trace arrival: index (int32), sub-sample offset and signed value of the extreme sample"""
        self._check(self.lib.thz_peak_map(self.ctx, npix, nt, _dp(data), int(mode), _dp(index), _dp(offset), _dp(value)))

    def optical_maps(self, npix, nf, amp, phase, ref_amp, ref_phase, freq, cfg: "OpticalCfg", thickness=None, n=None,
                     alpha=None, kappa=None, wraps=None, slope=None):
        """thz_optical_maps: amp, phase (npix, nf), thickness (npix) and the outputs are device pointers / DevBufs;
        ref_amp, ref_phase, freq host vectors of nf floats"""
        host = [np.ascontiguousarray(x, np.float32) for x in (ref_amp, ref_phase, freq)]
        if any(h.size != nf for h in host):
            raise ValueError("ref_amp, ref_phase and freq hold nf values each")
        self._check(self.lib.thz_optical_maps(self.ctx, npix, nf, _dp(amp), _dp(phase), *[h.ctypes.data for h in host],
                                              C.byref(cfg), _dp(thickness), _dp(n), _dp(alpha), _dp(kappa), _dp(wraps), _dp(slope)))

    def echo_map(self, npix, nt, data, cfg: "EchoCfg", index=None, offset=None, value=None, count=None):
        """thz_echo_map: data (npix, nt); index, offset, value (n_echoes, npix) and count (npix) are device pointers /
        DevBufs or None"""
        self._check(self.lib.thz_echo_map(self.ctx, npix, nt, _dp(data), C.byref(cfg), _dp(index), _dp(offset), _dp(value),
                                          _dp(count)))

    def layer_map(self, npix, n_echoes, index, offset, cfg: "LayerCfg", thickness=None, delay=None):
        """thz_layer_map: index, offset (n_echoes, npix) -> thickness, delay (n_echoes - 1 or 1, npix), all on the device"""
        self._check(self.lib.thz_layer_map(self.ctx, npix, int(n_echoes), _dp(index), _dp(offset), C.byref(cfg), _dp(thickness),
                                           _dp(delay)))

    def pca_sums(self, npix, n, x, row_stride, col_step=1, mask=None):
        """thz_pca_sums of the (npix, n) matrix x[p * row_stride + j * col_step] -> (sum f64 (n), count)"""
        s, cnt = np.zeros(max(int(n), 1), np.float64), C.c_uint64()
        self._check(self.lib.thz_pca_sums(self.ctx, npix, n, _dp(x), row_stride, col_step, _dp(mask), s.ctypes.data, C.byref(cnt)))
        return s[:n], cnt.value

    def pca_gram(self, npix, n, x, row_stride, col_step=1, mask=None, mu=None):
        """thz_pca_gram -> f64 (n, n): the Gram matrix of x - mu over the unmasked pixels"""
        g = np.zeros((max(int(n), 1),) * 2, np.float64)
        m = None if mu is None else np.ascontiguousarray(mu, np.float32)
        self._check(self.lib.thz_pca_gram(self.ctx, npix, n, _dp(x), row_stride, col_step, _dp(mask),
                                          None if m is None else m.ctypes.data, g.ctypes.data))
        return g[:n, :n]

    def pca_scores(self, npix, n, x, row_stride, col_step, mu, components, scores):
        """thz_pca_scores: scores (K, npix) on the device from host mu (or None) and components (K, n)"""
        m = None if mu is None else np.ascontiguousarray(mu, np.float32)
        v = np.ascontiguousarray(components, np.float32)
        self._check(self.lib.thz_pca_scores(self.ctx, npix, n, _dp(x), row_stride, col_step, None if m is None else m.ctypes.data,
                                            v.ctypes.data, v.shape[0] if v.ndim == 2 else 1, _dp(scores)))

    def cluster_step(self, npix, n, x, row_stride, col_step, mask, centroids, label, dist2, want_sums=True):
        """thz_cluster_step on device label (int32, read and written) and dist2 (f32) -> (sums f64 (K, n) or None,
        counts (K), inertia, changed, farthest)"""
        m = np.ascontiguousarray(centroids, np.float32)
        k = m.shape[0] if m.ndim == 2 else 1
        sums = np.zeros((max(k, 1), max(int(n), 1)), np.float64) if want_sums else None
        counts, inertia, changed, far = np.zeros(max(k, 1), np.uint64), C.c_double(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.thz_cluster_step(self.ctx, npix, n, _dp(x), row_stride, col_step, _dp(mask), m.ctypes.data, k, _dp(label),
                                              _dp(dist2), None if sums is None else sums.ctypes.data, counts.ctypes.data,
                                              C.byref(inertia), C.byref(changed), C.byref(far)))
        return (None if sums is None else sums[:k, :n]), counts[:k], inertia.value, changed.value, far.value

    def sparse_deconv(self, npix, nt, data, taps, cfg: "SparseCfg", out, resid=None, nnz=None):
        """thz_sparse_deconv on device buffers: out (npix, nt) f32 (may be data itself), resid (npix) f32 and nnz (npix)
        int32 or None"""
        h = np.ascontiguousarray(taps, np.float32).ravel()
        self._check(self.lib.thz_sparse_deconv(self.ctx, npix, nt, _dp(data), h.ctypes.data, C.byref(cfg), _dp(out), _dp(resid),
                                               _dp(nnz)))

    def wavelet_denoise(self, npix, nt, data, hn, gn, scale, cfg: "WaveletCfg", out, sigma=None, kept=None):
        """thz_wavelet_denoise on device buffers: out (npix, nt) f32 (may be data itself), sigma (npix) f32 and kept (npix)
        int32 or None"""
        h, g, s = _wavelet_vectors(hn, gn, scale)
        self._check(self.lib.thz_wavelet_denoise(self.ctx, npix, nt, _dp(data), h.ctypes.data, g.ctypes.data, s.ctypes.data,
                                                 C.byref(cfg), _dp(out), _dp(sigma), _dp(kept)))

    def unmix(self, npix, n, x, row_stride, col_step, endmembers, abund, n_sweeps=256, ref=None, absorbance=None, proj=None, resid=None,
              kkt=None):
        """thz_unmix on device buffers: abund and proj (K, npix), resid and kkt (npix), the last three or None; endmembers
        (K, n) and ref (n, or None) host floats.  A reference turns the absorbance mode on unless `absorbance` says otherwise"""
        e = np.ascontiguousarray(endmembers, np.float32)
        r = None if ref is None else np.ascontiguousarray(ref, np.float32)
        on = r is not None if absorbance is None else bool(absorbance)
        cfg = UnmixCfg(e.shape[0] if e.ndim == 2 else 1, int(n_sweeps), int(on))
        self._check(self.lib.thz_unmix(self.ctx, npix, n, _dp(x), row_stride, col_step, e.ctypes.data, None if r is None else r.ctypes.data,
                                       C.byref(cfg), _dp(abund), _dp(proj), _dp(resid), _dp(kkt)))

    def arrival_plane_moments(self, nx, ny, dx, dy, dt_ps, index, offset, value, rel_threshold) -> np.ndarray:
        m = np.zeros(10, np.float64)
        self._check(self.lib.thz_arrival_plane_moments(self.ctx, nx, ny, dx, dy, dt_ps, _dp(index), _dp(offset), _dp(value),
                                                       rel_threshold, m.ctypes.data))
        return m

    def intensity(self, npix, data, img):
        self._check(self.lib.thz_intensity(self.ctx, npix, _dp(data), _dp(img)))

    def subtract_bias(self, npix, data, img=None):
        self._check(self.lib.thz_subtract_bias(self.ctx, npix, _dp(data), _dp(img)))

    def pixel_mean(self, nx, ny, length, ncomp, arr, out):
        self._check(self.lib.thz_pixel_mean(self.ctx, nx, ny, length, ncomp, _dp(arr), _dp(out)))

    def pixel_sum(self, npix, length, ncomp, arr, out):
        self._check(self.lib.thz_pixel_sum(self.ctx, npix, length, ncomp, _dp(arr), _dp(out)))

    def roi_mask(self, poly_xy, scaling, shape0, shape1, mask):
        poly = np.ascontiguousarray(poly_xy, np.uint64).reshape(-1, 2)
        self._check(self.lib.thz_roi_mask(self.ctx, poly.ctypes.data if poly.size else None,
                                          poly.shape[0], scaling, shape0, shape1, _dp(mask)))

    def roi_mean(self, arr, shape0, shape1, length, mask, out, count=None, sum_only=False):
        self._check(self.lib.thz_roi_mean(self.ctx, _dp(arr), shape0, shape1, length, _dp(mask),
                                          _dp(out), _dp(count), int(sum_only)))

    def scale3d(self, arr, nx, ny, length, ncomp, s, out):
        self._check(self.lib.thz_scale3d(self.ctx, _dp(arr), nx, ny, length, ncomp, s, _dp(out)))

    def tilt_apply(self, npix, d_in, nt_in, d_taper, d_insert, nt_out, d_out):
        self._check(self.lib.thz_tilt_apply(self.ctx, npix, _dp(d_in), nt_in, _dp(d_taper), _dp(d_insert),
                                            nt_out, _dp(d_out)))

    def polar_ifft(self, amp, phase, zero_dc_imag=False):
        """ifft's avg_in_fourier_space branch: from_polar(avg amplitude, avg phase) -> C2R / nt (host vectors)"""
        a, p = (np.ascontiguousarray(x, np.float32) for x in (amp, phase))
        out = np.empty(self.nt, np.float32)
        self._check(self.lib.thz_polar_ifft(self.ctx, a.ctypes.data, p.ctypes.data, int(zero_dc_imag), out.ctypes.data))
        return out

    def deconvolve(self, psf: Psf, cfg: DeconvCfg, nx, ny, dx, dy, d_in, d_out, d_img=None, d_gains=None,
                   abort=None, progress=None):
        """-> status (0 applied, 1 skipped by one of the reference's guards).  abort: ctypes.c_int polled
        between iteration batches (the reference's AtomicBool); progress: ctypes.c_float written 0..1"""
        rc = self.lib.thz_deconvolve(self.ctx, C.byref(psf), C.byref(cfg), nx, ny, dx, dy, _dp(d_in), _dp(d_out),
                                     _dp(d_img), _dp(d_gains), C.byref(abort) if abort is not None else None,
                                     C.byref(progress) if progress is not None else None)
        if rc < 0:
            self._check(rc)
        return rc

    def reference_spectrum(self, scan_time, ref_time, ref_signal, window_type=0, lower=1.0, upper=7.0):
        """OpenRef -> (aligned + windowed reference, amplitudes, unwrapped phases)"""
        st, rt, rs = (np.ascontiguousarray(x, np.float32) for x in (scan_time, ref_time, ref_signal))
        nf = st.size // 2 + 1
        ref, amp, ph = np.empty(st.size, np.float32), np.empty(nf, np.float32), np.empty(nf, np.float32)
        w = WindowCfg(window_type, lower, upper)
        self._check(self.lib.thz_reference_spectrum(self.ctx, st.ctypes.data, st.size, rt.ctypes.data, rs.ctypes.data,
                                                    rs.size, C.byref(w), ref.ctypes.data, amp.ctypes.data,
                                                    ph.ctypes.data))
        return ref, amp, ph

    def voxel_opacity(self, npix, nt, d_data, cfg: VoxelCfg, d_opacity):
        self._check(self.lib.thz_voxel_opacity(self.ctx, npix, nt, _dp(d_data), C.byref(cfg), _dp(d_opacity)))

    def select_histogram(self, d_vals, n, level, prefix, d_hist):
        self._check(self.lib.thz_select_histogram(self.ctx, _dp(d_vals), n, level, prefix, _dp(d_hist)))

    def kth_largest(self, d_vals, n, k) -> float:
        v = C.c_float()
        self._check(self.lib.thz_kth_largest(self.ctx, _dp(d_vals), n, k, C.byref(v)))
        return v.value

    def voxel_threshold(self, d_opacity, n, max_instances=VOXEL_MAX_INSTANCES) -> float:
        v = C.c_float()
        self._check(self.lib.thz_voxel_threshold(self.ctx, _dp(d_opacity), n, max_instances, C.byref(v)))
        return v.value

    def voxel_instances(self, d_opacity, gw, gh, gd, threshold, time_span, scaling, orig_dims, d_out, capacity,
                        x0=0, gw_total=None):
        """-> (count, (cube_width, cube_height, cube_depth))"""
        n = C.c_uint64()
        dims = np.zeros(3, np.float32)
        self._check(self.lib.thz_voxel_instances(self.ctx, _dp(d_opacity), gw, gh, gd, x0,
                                                 gw if gw_total is None else gw_total, threshold, time_span,
                                                 scaling, orig_dims[0], orig_dims[1], orig_dims[2], _dp(d_out),
                                                 capacity, C.byref(n), dims.ctypes.data))
        return n.value, tuple(float(x) for x in dims)

    def traffic_probe(self, npix, nt, d_in, d_fft, d_amp, d_phase, d_out):
        self._check(self.lib.thz_traffic_probe(self.ctx, npix, nt, _dp(d_in), _dp(d_fft), _dp(d_amp), _dp(d_phase),
                                               _dp(d_out)))

    def synth_cube(self, d_out, ntraces, first_trace, d_time, seed=0x7A3D2026, subtract_bias=True):
        self._check(self.lib.thz_synth_cube(self.ctx, _dp(d_out), ntraces, first_trace, _dp(d_time),
                                            seed, int(subtract_bias)))

    def enable_timing(self, mode=1):
        self._check(self.lib.thz_enable_timing(self.ctx, int(mode)))

    def timing_collect(self, stage: int):
        """-> (total_ns, calls) of `stage` since the last collect (deferred mode)"""
        t, n = C.c_uint64(), C.c_uint64()
        self._check(self.lib.thz_timing_collect(self.ctx, stage, C.byref(t), C.byref(n)))
        return t.value, n.value

    def stage_time_ns(self, stage: int) -> int:
        v = C.c_uint64()
        self._check(self.lib.thz_stage_time_ns(self.ctx, stage, C.byref(v)))
        return v.value
