"""MI355X-native engine for the thz-image-explorer recompute path.

The product is `libthzgpu.so` (C ABI, include/thzgpu.h) built from `csrc/`.
This package only carries the ctypes binding used by tests and bench.py.
"""
from .binding import (Engine, DevBuf, ThzError, load_library, LIB_PATH, SYMBOLS,  # noqa: F401
                      host_frequency_axis, host_fft_window, host_adapted_blackman,
                      host_td_bandpass, host_fd_bandpass, host_tilt_plan,
                      host_water_line_mask, host_wiener_filter, host_psf_eval, host_filter_bank, host_band_psf, psf_from_npz, Psf, DeconvCfg, ChainCfg, Session, chain_cfg_default,
                      BUF_RAW, BUF_FFT, BUF_AMPLITUDES, BUF_PHASES, BUF_DATA, BUF_IMG, BUF_AVG_FFT,
                      BUF_AVG_AMPLITUDES, BUF_AVG_PHASES, BUF_OPACITY, VoxelCfg, VOXEL_INSTANCE, VOXEL_MAX_INSTANCES,
                      voxel_cfg_default, Group, GroupSession, host_slab, group_unique_id, GATHER_SMALL, GATHER_TIME, GATHER_ALL, PipelineIo,
                      host_optical_properties, host_align_reference, PlotOut, host_gaussian_kernel1d, host_select_step, host_select_value,
                      TiltFit, host_arrival_plane_fit, BUF_PEAK_INDEX, BUF_PEAK_OFFSET, BUF_PEAK_VALUE, PEAK_ABS, PEAK_MAX, PEAK_MIN,
                      OpticalCfg, optical_cfg, OPTICAL_MAX_BANDS, STAGE_OPTICAL, BUF_OPT_N, BUF_OPT_ALPHA, BUF_OPT_KAPPA,
                      BUF_OPT_WRAPS, BUF_OPT_SLOPE,
                      EchoCfg, LayerCfg, echo_cfg, layer_cfg, host_echo_trace, ECHO_MAX, LAYER_BETWEEN, LAYER_REFERENCE, STAGE_ECHO,
                      BUF_ECHO_INDEX, BUF_ECHO_OFFSET, BUF_ECHO_VALUE, BUF_ECHO_COUNT, BUF_LAYER_THICKNESS, BUF_LAYER_DELAY,
                      PcaCfg, PcaOut, pca_cfg, host_pca_components, PCA_MAX_LEN, PCA_MAX_COMPONENTS, PCA_CHAIN, STAGE_PCA,
                      BUF_PCA_SCORES, BUF_PCA_COMPONENTS, BUF_PCA_MEAN,
                      ClusterCfg, ClusterOut, cluster_cfg, host_cluster_update, CLUSTER_MAX, CLUSTER_INIT_GIVEN, CLUSTER_INIT_FARTHEST,
                      BUF_CLUSTER_LABELS, BUF_CLUSTER_DIST, BUF_CLUSTER_CENTROIDS,
                      SparseCfg, sparse_cfg, host_sparse_trace, host_sparse_kernel, SPARSE_MAX_TAPS, SPARSE_MAX_NT, SPARSE_MAX_ITER,
                      BUF_SPARSE, BUF_SPARSE_RESID, BUF_SPARSE_NNZ,
                      UnmixCfg, UnmixSessionCfg, unmix_session_cfg, host_unmix_prepare, host_unmix_solve, UNMIX_MAX, UNMIX_MAX_SWEEPS,
                      BUF_UNMIX_ABUNDANCE, BUF_UNMIX_PROJ, BUF_UNMIX_RESID, BUF_UNMIX_KKT,
                      WaveletCfg, wavelet_cfg, host_wavelet_trace, host_wavelet_filter, host_wavelet_universal,
                      WAVELET_MAX_TAPS, WAVELET_MAX_LEVELS, WAVELET_MAX_NT, WAVELET_MAX_WORDS,
                      BUF_DENOISED, BUF_DENOISE_SIGMA, BUF_DENOISE_KEPT)
from . import binding  # noqa: F401
