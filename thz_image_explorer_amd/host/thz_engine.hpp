// thz_engine.hpp — the record-and-flush engine the reference-side binding is built around, in C++.
//
// rust/engine.rs, rust/math_tools_gpu.rs and rust/filters/*.rs are the same code in the reference's
// language; no Rust toolchain exists in the build image, so the logic a maintainer would otherwise have to
// take on trust is written — and run, tests/test_gpu_engine.py — here first, and the Rust files are its
// transliteration (same names, same order of calls).
//
// The reference walks its stage chain one stage at a time, each stage returning a complete new container
// (data_thread.rs:1090-1191).  The device engine computes the whole chain in one launch, so on this path a stage
// call only RECORDS its parameters (or, for a plugin the walk passes through, its inactivity) and returns a
// container without the big arrays; after the loop one `flush()` runs `thz_group_session_recompute` from the
// lowest chain position the walk touched, and everything the code behind the loop reads — image, averages,
// per-region means, the selected pixel's traces, each filter's `show_data` plot — is fetched from the device then.
#pragma once

#include "thz_host.hpp"

namespace thzhost {

// chain positions of thz_session_recompute_from: the reference's filter_chain (main.rs:182-247) with all
// FilterDomain::Frequency plugins on one position
enum ChainPosition { kPosScaling = 1, kPosTilt = 2, kPosTdBefore = 3, kPosFft = 4, kPosFrequency = 5, kPosIfft = 6, kPosTdAfter = 7, kPosDeconvolution = 8 };
int chain_position(FilterDomain d);
int chain_position(const std::string &hard_wired_id);  // "scaling" / "fft" / "ifft", else 0

class GpuEngine {
public:
    // devices: the GPUs to tile the x rows over (THZGPU_DEVICES=0,1,... for the process-global instance; the same
    // device several times = slabs side by side on one GPU, what the tests use)
    explicit GpuEngine(const std::vector<int> &devices);
    ~GpuEngine();
    GpuEngine(const GpuEngine &) = delete;
    GpuEngine &operator=(const GpuEngine &) = delete;
    static GpuEngine &instance();
    bool available() const { return group_ != nullptr; }
    std::string last_error() const;

    // ConfigCommand::OpenFile (io.rs:576-628): the cube goes to the device(s) once
    bool open_scan(const float *cube, size_t nx, size_t ny, const std::vector<float> &time, float dx, float dy,
                   bool subtract_bias = true);

    // ---- the stage walk of UpdateType::Filter(start_idx)
    void begin_walk(int start_position);
    void record_scaling(size_t scale_factor);
    void record_tilt(bool active, double tilt_x, double tilt_y);
    void record_td_before(bool active, double low, double high, double width);
    void record_fft(int window_type, float lower, float upper);
    void record_fd(bool active, double low, double high, double width);
    void record_water_lines(bool active, std::vector<float> mask);   // K14, real per-bin multiplier (nf)
    void record_wiener(bool active, std::vector<float> cmask);       // K13, complex per-bin multiplier (2 nf)
    void record_ifft(bool avg_in_fourier_space, const std::vector<std::pair<std::string, Polygon>> &rois);
    void record_td_after(bool active, double low, double high, double width);
    // the walk passed an inactive plugin's input through (data_thread.rs:1185-1188): its stage is off in the chain
    void note_inactive(const FilterConfig &cfg);
    // after the loop (and in front of the Deconvolution stage): one recompute from the lowest touched position
    bool flush();
    // the Deconvolution stage over the whole group; progress and abort forwarded live.  THZ_OK / THZ_SKIPPED / < 0
    int deconvolve(const thz_psf &psf, const thz_deconv_cfg &cfg, ProgressLock &progress, const std::atomic<bool> &abort_flag);

    // ---- results of the last flush
    bool image(std::vector<float> &img, size_t &gx, size_t &gy);   // on the outputs' grid (nx / s, ny / s)
    bool averages(std::vector<std::complex<float>> &avg_fft, std::vector<float> &avg_amp, std::vector<float> &avg_phase);
    bool plot(size_t px, size_t py, const thz_plot_out &out);      // px, py: pixel of the RAW grid
    bool roi(const std::string &uuid, const thz_roi_out &out);
    size_t nt_out() const;
    std::vector<float> time_out() const;
    // the 3-D tab's instances over the WHOLE grid (thz_group_session_voxels; data_thread.rs:82-101): threshold from
    // the whole cube, every slab's instances in x, y, z order — what one GPU gives for the same cube
    bool voxels(const thz_voxel_cfg &cfg, uint64_t max_instances, size_t scaling, size_t orig_w, size_t orig_h,
                size_t orig_d, std::vector<thz_voxel_instance> &out, float &threshold, float cube_dims[3]);
    // The angles that flatten the pulse's arrival plane over the WHOLE grid (thz_group_session_estimate_tilt): of the raw
    // cube (which = THZ_BUF_RAW) or of the chain's final traces (THZ_BUF_DATA; whatever the walk has recorded is
    // flushed first).  mode 0 largest |x|, 1 maximum, 2 minimum.  THZ_OK, THZ_SKIPPED (no plane: `out` is zeros) or < 0
    int estimate_tilt(int which, int mode, float rel_threshold, thz_tilt_fit &out);
    // Refractive index, absorption and extinction over every pixel this process holds, as means over cfg's bands
    // (thz_session_optical_maps on each local member's resident spectra, the slabs' rows one after the other; whatever
    // the walk has recorded is flushed first).  ref_amp / ref_phase: a reference's roi_signal_fft / roi_phase_fft
    // (nt_out / 2 + 1 values, OpenRef); cfg: sample_thickness, the anchor and the bands as bin ranges.
    // n, alpha, kappa: (n_bands, gx, gy); wraps, slope: (gx, gy)
    bool optical_maps(const std::vector<float> &ref_amp, const std::vector<float> &ref_phase, const thz_optical_cfg &cfg,
                      std::vector<float> &n, std::vector<float> &alpha, std::vector<float> &kappa, std::vector<int32_t> &wraps,
                      std::vector<float> &slope, size_t &gx, size_t &gy);
    // The cfg.n_echoes strongest separated pulses of every trace this process holds (thz_session_echo_map on each local
    // member, slab after slab: every pixel is independent), of the raw cube (which = THZ_BUF_RAW) or of the chain's final
    // traces (THZ_BUF_DATA; whatever the walk has recorded is flushed first), or of the spike trains of the last
    // sparse_deconv (THZ_BUF_SPARSE, on the grid of the cube they were taken of).
    // index, offset, value: (n_echoes, gx, gy), rank-major with index -1 for a rank that was not found; count: (gx, gy)
    bool echo_map(int which, const thz_echo_cfg &cfg, std::vector<int32_t> &index, std::vector<float> &offset,
                  std::vector<float> &value, std::vector<int32_t> &count, size_t &gx, size_t &gy);
    // Delays and thicknesses from the last echo_map (thz_session_layer_map on each local member): (rows, gx, gy) with
    // rows = n_echoes - 1 between consecutive pulses (cfg.mode 0) and 1 against a fixed arrival (cfg.mode 1).  A member's
    // THZ_BUF_LAYER_THICKNESS stays resident: a row of it is a valid d_thickness of thz_session_optical_maps
    bool layer_map(const thz_layer_cfg &cfg, std::vector<float> &thickness, std::vector<float> &delay, size_t &rows,
                   size_t &gx, size_t &gy);
    // Sparse deconvolution of every trace this process holds (thz_session_sparse_deconv on each local
    // member, slab after slab: every pixel is independent), of the raw cube (which = THZ_BUF_RAW) or of the chain's final
    // traces (THZ_BUF_DATA; whatever the walk has recorded is flushed first).  taps: cfg.n_taps values, e.g. what
    // thz_host_sparse_kernel cuts out of a reference pulse.  Every member's THZ_BUF_SPARSE / _SPARSE_RESID / _SPARSE_NNZ
    // stay resident: echo_map(THZ_BUF_SPARSE, ...) and layer_map then turn the spikes of a thin coating into its thickness.
    // x: (gx, gy, nt_src) spike trains; resid, nnz: (gx, gy)
    bool sparse_deconv(int which, const std::vector<float> &taps, const thz_sparse_cfg &cfg, std::vector<float> &x,
                       std::vector<float> &resid, std::vector<int32_t> &nnz, size_t &gx, size_t &gy, size_t &nt_src);
    // Wavelet shrinkage of every trace this process holds (thz_session_wavelet_denoise on each local
    // member, slab after slab: every pixel is independent), of the raw cube (which = THZ_BUF_RAW) or of the chain's final
    // traces (THZ_BUF_DATA; whatever the walk has recorded is flushed first).  hn, gn: cfg.n_taps analysis taps each, e.g.
    // thz_host_wavelet_filter's; scale: cfg.n_levels thresholds, e.g. thz_host_wavelet_universal's.  Every member's
    // THZ_BUF_DENOISED / _DENOISE_SIGMA / _DENOISE_KEPT stay resident.
    // x: (gx, gy, nt_src) denoised traces; sigma, kept: (gx, gy)
    bool wavelet_denoise(int which, const std::vector<float> &hn, const std::vector<float> &gn, const std::vector<float> &scale,
                         const thz_wavelet_cfg &cfg, std::vector<float> &x, std::vector<float> &sigma, std::vector<int32_t> &kept,
                         size_t &gx, size_t &gy, size_t &nt_src);
    // Principal components of everything this process holds: the covariance is not pixel-independent, so
    // thz_session_pca_sums and thz_session_pca_gram run on each local member, the members' sums and Gram matrices are
    // added here in member order (f64), thz_host_pca_components runs once, and thz_session_pca_project fills each
    // member's THZ_BUF_PCA_SCORES / _COMPONENTS / _MEAN with the common mean and components.  which: THZ_BUF_AMPLITUDES,
    // _PHASES, _DATA (whatever the walk has recorded is flushed first) or _RAW; cfg.d_mask is not read: mask is empty or
    // one byte per pixel of the whole (gx, gy) grid, 0 leaving the pixel out of mean and covariance.
    // scores: (n_components, gx, gy); components: (n_components, count); mean: (count), zeros when cfg.center == 0
    bool pca(int which, const thz_pca_cfg &cfg, const std::vector<uint8_t> &mask, thz_pca_out &out, std::vector<float> &scores,
             std::vector<float> &components, std::vector<float> &mean, size_t &gx, size_t &gy);
    // k-means of everything this process holds: clustering is not pixel-independent, so
    // thz_session_cluster_step runs on each local member and the members' sums, counts, inertia and changed are added here
    // in member order (f64); the farthest pixel is the largest THZ_BUF_CLUSTER_DIST entry among the members' candidates,
    // the lowest global index winning a tie, and thz_session_cluster_row fetches its row; thz_host_cluster_update runs
    // once per step, and every member iterates with the common centroids.  The mean the seeding starts from is the sum of
    // a K = 1 step about the zero vector (rows with a NaN are left out of it).  which: what thz_session_cluster takes;
    // THZ_BUF_PCA_SCORES means the score images of the last pca() of the recompute's grid and takes no mask.
    // cfg.d_mask is not read: mask is empty or one byte per pixel of the whole (gx, gy) grid.  Every member's
    // THZ_BUF_CLUSTER_LABELS / _DIST / _CENTROIDS stay resident.
    // labels, dist2: (gx, gy); centroids: (n_clusters, count)
    bool cluster(int which, const thz_cluster_cfg &cfg, const std::vector<uint8_t> &mask, thz_cluster_out &out,
                 std::vector<int32_t> &labels, std::vector<float> &dist2, std::vector<float> &centroids, size_t &gx, size_t &gy);
    // Non-negative least squares of every pixel this process holds against cfg.n_endmembers spectra (DESIGN.md 4.12;
    // thz_session_unmix on each local member, slab after slab: every pixel is independent).  which: THZ_BUF_AMPLITUDES,
    // _PHASES, _DATA (whatever the walk has recorded is flushed first) or _RAW.  cfg.endmembers NULL takes each member's
    // resident THZ_BUF_CLUSTER_CENTROIDS — the ones cluster() left on every member.  Every member's THZ_BUF_UNMIX_* stay
    // resident.  abundance: (n_endmembers, gx, gy); resid, kkt: (gx, gy)
    bool unmix(int which, const thz_unmix_session_cfg &cfg, std::vector<float> &abundance, std::vector<float> &resid,
               std::vector<float> &kkt, size_t &gx, size_t &gy);
    bool download_final(std::vector<float> &cube);                 // the whole final trace cube, rank order (tests)

    const thz_chain_cfg &pending() const { return pending_; }
    int dirty_from() const { return dirty_from_; }
    size_t nx = 0, ny = 0, nt = 0;

private:
    void touch(int position) { if (position < dirty_from_) dirty_from_ = position < 1 ? 1 : position; }
    thz_session *owner_of(size_t px, size_t *local_px) const;
    thz_group *group_ = nullptr;
    thz_group_session *session_ = nullptr;
    thz_chain_cfg pending_{};
    int dirty_from_ = 1;
    std::vector<float> fd_real_, fd_cmask_;  // empty = that plugin is off
    bool plugins_dirty_ = true;
    std::vector<size_t> echo_rows_;          // the last echo_map: rows per local member, columns and ranks (0: none)
    size_t echo_gy_ = 0, echo_k_ = 0;
    std::vector<size_t> sparse_rows_;        // the last sparse_deconv: rows per local member (empty: none) and columns
    size_t sparse_gy_ = 0;
    std::vector<std::pair<std::string, Polygon>> rois_;
    bool rois_dirty_ = false;
};

// ---- math_tools::{scaling, fft, ifft} on the engine (rust/math_tools_gpu.rs) -----------------------------------
namespace math_tools_gpu {
// metadata, axes, regions and plans of `input`; the five big arrays stay empty (they are resident on the device)
ScannedImageFilterData shallow_clone(const ScannedImageFilterData &input);
ScannedImageFilterData scaling(GpuEngine &eng, const ScannedImageFilterData &input, const ConfigContainer &config);
ScannedImageFilterData fft(GpuEngine &eng, const ScannedImageFilterData &input, const ConfigContainer &config);
ScannedImageFilterData ifft(GpuEngine &eng, const ScannedImageFilterData &input, const ConfigContainer &config);
// after the stage loop (data_thread.rs:1229): flush, then fill what the code behind the loop reads from the LAST
// container: img (expanded s x s when scaled, :1243-1285), the three averages, avg_data, and the regions' maps
bool finish_stage_walk(GpuEngine &eng, ScannedImageFilterData &last, const ConfigContainer &config);
}  // namespace math_tools_gpu

// ---- the plugins on the engine (rust/filters/*.rs): same structs, `filter()` records ------------------------
struct GpuTiltCompensation : TiltCompensation {
    // the "Estimate" action of the plugin's panel: the raw cube's arrival plane -> tilt_x / tilt_y; the caller then
    // requests UpdateFilter(<this filter>) as for a moved slider.  false (fields untouched) when there is no plane
    int estimate_mode = 1;                 // the pulse's main peak is its maximum
    float estimate_threshold = 0.25f;      // pixels below a quarter of the strongest peak take no part
    bool estimate(GpuEngine &eng);
    ScannedImageFilterData filter(const ScannedImageFilterData &, GuiSettingsContainer &, ProgressLock &,
                                  const std::atomic<bool> &) override;
    std::unique_ptr<Filter> clone_box() const override { return std::make_unique<GpuTiltCompensation>(*this); }
};
struct GpuTimeDomainBandPassBeforeFFT : TimeDomainBandPassBeforeFFT {
    void show_data(const ScannedImageFilterData &) override;
    ScannedImageFilterData filter(const ScannedImageFilterData &, GuiSettingsContainer &, ProgressLock &,
                                  const std::atomic<bool> &) override;
    std::unique_ptr<Filter> clone_box() const override { return std::make_unique<GpuTimeDomainBandPassBeforeFFT>(*this); }
};
struct GpuTimeDomainBandPassAfterFFT : TimeDomainBandPassAfterFFT {
    void show_data(const ScannedImageFilterData &) override;
    ScannedImageFilterData filter(const ScannedImageFilterData &, GuiSettingsContainer &, ProgressLock &,
                                  const std::atomic<bool> &) override;
    std::unique_ptr<Filter> clone_box() const override { return std::make_unique<GpuTimeDomainBandPassAfterFFT>(*this); }
};
struct GpuFrequencyDomainBandPass : FrequencyDomainBandPass {
    void show_data(const ScannedImageFilterData &) override;
    ScannedImageFilterData filter(const ScannedImageFilterData &, GuiSettingsContainer &, ProgressLock &,
                                  const std::atomic<bool> &) override;
    std::unique_ptr<Filter> clone_box() const override { return std::make_unique<GpuFrequencyDomainBandPass>(*this); }
};
struct GpuDeconvolution : Deconvolution {
    ScannedImageFilterData filter(const ScannedImageFilterData &, GuiSettingsContainer &, ProgressLock &,
                                  const std::atomic<bool> &) override;
    std::unique_ptr<Filter> clone_box() const override { return std::make_unique<GpuDeconvolution>(*this); }
};
// K14 / K13 (build-defined)
struct WaterLineNotch : Filter {
    float sigma_thz = 0.01f;
    std::vector<float> lines_thz;
    FilterConfig config() const override;
    ScannedImageFilterData filter(const ScannedImageFilterData &, GuiSettingsContainer &, ProgressLock &,
                                  const std::atomic<bool> &) override;
    std::unique_ptr<Filter> clone_box() const override { return std::make_unique<WaterLineNotch>(*this); }
};
struct WienerDeconvolution : Filter {
    float eps_rel = 1e-2f;
    std::vector<float> reference_spectrum;  // (nf, 2) interleaved: what OpenRef leaves (thz_reference_spectrum)
    FilterConfig config() const override;
    ScannedImageFilterData filter(const ScannedImageFilterData &, GuiSettingsContainer &, ProgressLock &,
                                  const std::atomic<bool> &) override;
    std::unique_ptr<Filter> clone_box() const override { return std::make_unique<WienerDeconvolution>(*this); }
};

// ---- the patched stage walk (rust/data_thread.patch) ---------------------------------------------------------
// data_thread.rs:1023-1334 with the engine in it: begin_walk at the top, note_inactive where the reference clones an
// inactive plugin's input, show_data deferred until the results exist, finish_stage_walk where the image was summed.
struct GpuPipeline {
    explicit GpuPipeline(GpuEngine &eng);
    GpuEngine &eng;
    std::vector<std::pair<std::string, std::unique_ptr<Filter>>> filters;  // this pipeline's registry: (uuid, filter)
    std::vector<std::string> filter_chain;
    std::map<std::string, size_t> filter_uuid_to_index;
    std::map<std::string, bool> filters_active;
    std::vector<ScannedImageFilterData> filter_data;
    ConfigContainer config;
    GuiSettingsContainer gui_settings;
    std::atomic<bool> abort_flag{false};
    bool reset_filters = true;
    size_t fft_index = 0;

    void open(const float *cube, size_t nx, size_t ny, const std::vector<float> &time, float dx, float dy);
    void update_filter(size_t start_idx);                 // UpdateType::Filter(start_idx)
    size_t index_of(const std::string &description_or_name) const;   // chain index of a filter
    Filter *filter_by(const std::string &description_or_name);
};

}  // namespace thzhost
