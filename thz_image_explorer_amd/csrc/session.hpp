// session.hpp — the resident-cube session behind thz_session* (session_api.cpp) and the pieces of its
// recompute that the multi-GPU group (group_session.cpp) drives slab by slab.
#pragma once
#include "ctx.hpp"

#include <initializer_list>
#include <vector>

// One region of interest of a session (thz_session_set_rois) and its pixel list for the grid of the last recompute
struct SessionRoi {
    std::vector<uint64_t> poly;   // (x, y) pairs as the reference keeps them: pixels of the raw grid
    DevBuf<uint32_t> d_list;      // THIS slab's pixels inside, in the reference's visiting order (y outer, x inner;
                                  //   mask position (x, y) samples pixel [shape0 - y - 1, x], math_tools.rs:640-651)
    uint32_t count = 0;           // ... how many
    uint32_t total = 0;           // pixels of the WHOLE grid inside (= count unless the session is a group's slab)
    size_t for_rows = 0, for_cols = 0, for_scale = 0, for_x0 = 0, for_grid_rows = 0;  // what the list was built for
};

// A cube of a session with its grid, trace length, pixel pitch and the mean step of its time axis (session_cube)
struct SessionCube {
    const float *d = nullptr;
    size_t nx = 0, ny = 0, nt = 0;
    float dx = 1.0f, dy = 1.0f;
    double dt_ps = 0.0;
};

// One family of per-pixel results that stays resident in a session and is read through thz_session_buffer /
// thz_session_download: one grow-only device block of 4-byte words, cut into the planes of the family's last call.
// A call is  maps_begin (the family is absent, the block holds the new layout)  ->  the launch on ptr(i)  ->
// maps_commit (the stream has drained: resident).  Whatever fails in between leaves the family absent; a call refused
// for its arguments never gets as far as maps_begin and leaves what was resident.  An upload voids every family.
struct MapPlane {
    size_t entries = 0;  // what thz_session_download bounds pix0 + npix against; 0: the plane is empty (NULL to a reader)
    size_t per = 1;      // words per entry
    size_t off = 0;      // where it starts in the block, in words: the planes follow one another (set by maps_begin)
};
struct ResidentMaps {
    static constexpr int kMaxPlanes = 5;
    DevBuf<float> d;         // grow-only
    bool resident = false;
    MapPlane plane[kMaxPlanes];
    // plane i of the layout of the last maps_begin, resident or not: what the call's launch writes
    template <class T = float>
    T *ptr(int i) const { return reinterpret_cast<T *>(d + plane[i].off); }
    size_t entries(int i) const { return resident ? plane[i].entries : 0; }
};
// Marks the family absent, lays `planes` out one behind the other and makes sure of max(their words, min_words) words:
// a block that is too small is replaced by a larger one (DevBuf::grow; a failed allocation leaves no block).
int maps_begin(thz_ctx *ctx, ResidentMaps *m, std::initializer_list<MapPlane> planes, size_t min_words = 0);
// the call's closing synchronisation; the planes are resident when it has succeeded
int maps_commit(thz_ctx *ctx, ResidentMaps *m);
// A new family is a member here, its row in kMapIds (session_api.cpp) and its own *_api.cpp.
enum MapFamily { kMapPeak, kMapOptical, kMapEcho, kMapLayer, kMapPca, kMapCluster, kMapSparse, kMapUnmix, kMapDenoise, kMapFamilies };

struct thz_session {
    thz_ctx *ctx = nullptr;
    size_t nx = 0, ny = 0, nt = 0, nf = 0;
    float dx = 1.0f, dy = 1.0f;
    // grid of everything behind the scaling stage (math_tools.rs:242-310): nx / s, ny / s, dx * s, dy * s
    size_t nx_cur = 0, ny_cur = 0, scale = 1, out_pix = 0;
    float dx_cur = 1.0f, dy_cur = 1.0f;
    DevBuf<float> d_scaled;                    // block-averaged raw cube when scale > 1
    std::vector<float> time, time_out;
    size_t nt_out = 0, nf_out = 0;
    DevBuf<float> d_raw, d_fft, d_amp, d_ph, d_data, d_img, d_avg;  // d_avg: [2 nf | nf | nf]
    DevBuf<float> d_vec;                       // pre | mask | post multipliers (+ tilt scratch)
    PinnedBuf<float> h_vec;                    // pinned host image of d_vec: the multipliers go up in one asynchronous copy
    DevBuf<float> d_tilt;                      // extended cube when tilt != 0 (kept while its size stays the same): built by
                                               //   the staged path, or on demand behind a one-launch chain (session_extended_src)
    std::vector<int32_t> ins_host;             // the insert indices d_ins holds (a recompute with the same plan does not copy them again)
    // a tilted chain that ran as ONE launch from the untilted cube (FBP plans, thz_pipeline_tilted): what the launch
    // gathered from, so that the extended traces can still be built for whoever needs them
    bool tilt_fused = false;
    const float *tilt_from = nullptr;          // d_raw or d_scaled
    size_t tilt_nt_in = 0;
    const float *d_taper = nullptr;            // the Tilt stage's tail taper (tilt_nt_in floats inside d_vec)
    bool src_sum_own = false;                  // d_msum[0, nt_out) is THIS session's sum of source traces (a group adds the slabs')
    // ... the re-laid traces' sum depends on the source cube, the scale factor and the tilt only (src_gen): kept, like
    // d_rawsum, so that a recompute that moves another slider does not read the raw cube for it again
    DevBuf<float> d_tiltsum;
    unsigned long tiltsum_gen = 0;             // the src_gen it belongs to, 0 = none
    std::vector<float> fd_real, fd_cmask;      // further Frequency-domain plugins: K14 real (nf), K13 complex (2 nf)
    thz_chain_cfg last_cfg{};                  // configuration of the last full recompute (decides whether a
    bool have_last_cfg = false;                // start position >= 6 may reuse the resident spectrum)
    DevBuf<float> d_deconv, d_deconv_img;      // output of the Deconvolution stage (thz_session_deconvolve)
    bool deconv_current = false;               // ... and whether it is the chain's final output right now
    DevBuf<float> d_opacity;                   // voxel opacities of the final cube (thz_session_voxels)
    DevBuf<int32_t> d_ins;
    // the analysis maps of the last call of each family (ResidentMaps above): the planes are those of the family's
    // THZ_BUF_* ids, in their order (kMapIds in session_api.cpp)
    ResidentMaps maps[kMapFamilies];
    SessionCube sparse_cube;     // kMapSparse: the spike trains as a cube, on the grid, pitch and time step of the cube they were taken of
    SessionCube denoised_cube;   // kMapDenoise: the denoised traces as a cube, likewise
    DevBuf<float> d_rawsum;      // (nt) sum over the pixels of the raw (bias-subtracted) traces, taken at upload
    DevBuf<float> d_msum;        // [Σ source trace: nt_out | Σ amplitudes: nf | Σ phases: nf] of the last recompute, undivided
    bool msum_fast = false;      // the last recompute left its undivided sums in d_msum (want_means == 1)
    bool have_means = false;
    bool have_outputs = false;   // a recompute has run
    // Which bins of d_fft / d_amp hold zeros in every row: those outside [zero_lo, zero_hi), left there by fused
    // launches whose multiplier is zero outside the Frequency Band Pass's range — the next such launch stores only the
    // hull of its own range and this one (fft_f.hpp, "keep range").  zeros_known = false: nothing is known, the next
    // launch writes every bin.  session_enqueue is the two arrays' only writer; whatever may change their contents or
    // their shape behind its back drops the knowledge (session_forget_zeros).
    bool zeros_known = false;
    size_t zero_lo = 0, zero_hi = 0;
    unsigned long zero_gen = 0;  // the src_gen the knowledge belongs to
    // Whether d_ph holds the unwrapped phases of the current source traces under the pre-transform multiplier
    // phase_pre: they are those of FFT(pre x), in front of every Frequency-domain multiplier, so a recompute that moves
    // the Frequency Band Pass, a plugin or the post Time Band Pass would write the bits that are there already.  The
    // next fused launch is then told to leave them alone (fft_f.hpp, "kept phases"); where it carries the in-launch sums
    // it leaves the phase half of d_msum out as well, which comes from d_phsum — a copy apart, like d_tiltsum, because
    // session_means works on d_msum in place and a group all-reduces it.  phases_known = false: nothing is known, the
    // next launch computes and writes them.  session_enqueue is d_ph's only writer; thz_session_buffer drops the
    // knowledge when it hands out d_ph or the raw cube.
    bool phases_known = false;
    unsigned long phase_gen = 0;     // the src_gen the knowledge belongs to
    std::vector<float> phase_pre;    // the pre-transform multiplier of the launch that wrote them
    DevBuf<float> d_phsum;           // (nf) that launch's in-launch sums of the phases, if it carried sums
    bool phsum_valid = false;
    const float *d_src = nullptr;  // what the fft stage read: d_raw, d_scaled or d_tilt (extended axis); null while a
                                   //   one-launch tilted chain's extended cube has not been asked for
    // ---- regions of interest (session_roi.cpp)
    std::vector<SessionRoi> rois;
    DevBuf<float> d_roi_sum;       // [amplitudes R x nf | phases R x nf | stage-input traces R x nt | final traces R x nt]:
    DevBuf<float> d_roi;           //   this session's (after a group's all-reduce: the grid's) sums, and the means
    DevBuf<float> d_wsep;          // the three time multipliers in front of the transform, one by one (reference-order
                                   //   roi_data): [tilt taper | Time Band Pass | fft window], nt_out each
    bool wsep_on[3] = {false, false, false};
    std::vector<float> roi_polar;  // avg_in_fourier_space: per region the polar inverse transform (nt_out each), host
    std::vector<char> roi_polar_ok;  //   0: realfft would have refused the spectrum (the reference falls back to the traces)
    std::vector<float> avg_data;   // avg_in_fourier_space: the ifft stage's avg_data (nt_out), host
    bool have_rois = false;        // d_roi holds the means of the last recompute
    // The regions' sums of the SOURCE traces (parallel sums) do not depend on the sliders: they are kept for as long as
    // the source cube, the grid and the regions stay what they were (src_gen counts uploads, scale / tilt changes and
    // list rebuilds; roi_src_gen is the generation the kept sums belong to, 0 = none)
    unsigned long src_gen = 1, roi_src_gen = 0;
    bool roi_src_fresh = false;    // the last session_roi_sums renewed the source block (a group all-reduces it then)
    int last_sf = -1, last_tilt_active = -1;
    double last_tilt_x = 0.0, last_tilt_y = 0.0;
    // Placement in a group's grid (group_session.cpp).  raw_grid_rows == 0: the session is the whole grid.  Otherwise it
    // holds rows raw_grid_x0 .. + nx of the raw_grid_rows rows of the RAW grid (slab `slab_rank` of `slab_world`, all
    // slabs cut by thz_host_slab), and session_enqueue derives grid_x0 / grid_rows: the same for the CURRENT grid —
    // behind a scaling stage the block grid, whose rows belong to the slab that holds a block's LAST raw row.
    size_t raw_grid_x0 = 0, raw_grid_rows = 0;
    int slab_rank = 0, slab_world = 1;
    size_t grid_x0 = 0, grid_rows = 0;
    // scaling over slab edges: the undivided partial sums of the block this slab only holds the first rows of (handed
    // to the next slab by the group), and the previous slab's for the block this one completes; (ny / s) x nt each
    DevBuf<float> d_carry_out, d_carry_in;
    bool carry_out_valid = false;
    bool msum_passes = false;    // a group's slab, tilted: d_msum = [unused nt | sum fft 2 nf | sum amplitudes nf | sum phases nf]
};


// first half of a recompute: everything up to and including the fused launch, enqueued on the context's
// stream (tail_only: chain positions >= 6 were served from the resident spectrum)
int session_enqueue(thz_session *s, const thz_chain_cfg *cfg, int start_stage, bool *tail_only);
// thz_session_buffer for readers inside the library: hands out no right to write, so the session keeps what it knows
// of its spectrum's zeros
const void *session_buffer_ro(thz_session *s, int which);
// What `which` (THZ_BUF_AMPLITUDES, _PHASES, _DATA, _RAW) and the columns of cfg name in a session (pca_api.cpp): the
// strided matrix the PCA and cluster kernels read, or the error, whose message `what` starts
struct SessionMatrix {
    const float *d = nullptr;
    size_t npix = 0, L = 0, row_stride = 0, col_step = 0;
};
int session_matrix(thz_session *s, int which, const thz_pca_cfg *cfg, const char *what, SessionMatrix *m);
// the argument rules of every call on such a matrix: the reason for THZ_ERR_INVALID, or null
const char *pca_view_error(size_t L, const float *d_x, size_t row_stride, size_t col_step);
// The extended (re-laid) traces of a tilted chain that ran as one launch: the whole cube into d_tilt (and d_src) when
// it is not there yet — for the regions of interest's source sums; never on the recompute path of a session without
// regions.  A no-op for every other chain.
int session_extended_src(thz_session *s);
// Scaling over slab edges (group_session.cpp; math_tools.rs:273-301 adds a block's s x s inputs row by row): which rows
// of the block grid slab `rank` of `world` owns when the raw grid's nx rows are cut by thz_host_slab.
struct SlabScale {
    size_t head = 0;       // leading raw rows that complete the block the previous slab started (0: none)
    bool head_valid = false;  // ... and that block lies inside the block grid
    size_t full = 0;       // blocks that lie wholly inside the slab
    size_t tail = 0;       // trailing raw rows that start a block the next slab completes (0: none, or beyond the block grid)
    size_t rows = 0;       // rows of the block grid this slab owns = head_valid + full
    size_t x0 = 0;         // ... and where they start in the block grid
};
// The one rule for scaling a grid of nx x ny cut into `world` slabs by sf, the same on every rank: refused when the
// scaling is not the identity (sf > 1, nx / sf > 0, ny / sf > 0) and the smallest slab thz_host_slab cuts (nx / world
// rows) is shorter than sf — a block would span three slabs.  slab_scale is only called for splits it admits.
bool slab_scale_refused(size_t nx_total, size_t ny, int world, size_t sf);
SlabScale slab_scale(size_t nx_total, int world, int rank, size_t sf);
// before session_enqueue of a scaled group recompute: the partial sums of this slab's trailing block into d_carry_out
int session_scale_tail(thz_session *s, const thz_chain_cfg *cfg);
// second half: pixel means from the sums in d_msum, which cover total_pix pixels (the slab's own, or all
// slabs' after the group's all-reduce)
int session_means(thz_session *s, const thz_chain_cfg *cfg, size_t total_pix);
// Regions of interest, in two halves like the means: session_roi_sums enqueues the masked sums of this session's
// pixels into d_roi_sum (*data_only: the chain's tail or the Deconvolution stage changed the final traces only —
// cleared when the buffers are new and everything is summed after all);
// a group all-reduces d_roi (thz_session_roi_floats floats) in between; session_roi_finish divides by the
// regions' pixel counts over the whole grid and, with avg_in_fourier_space, takes the polar inverse transforms.
int session_roi_sums(thz_session *s, const thz_chain_cfg *cfg, bool *data_only);
int session_roi_finish(thz_session *s, const thz_chain_cfg *cfg, bool data_only);
size_t session_roi_floats(const thz_session *s);
// peak_api.cpp: the cube `which` names (THZ_BUF_RAW / THZ_BUF_DATA, or THZ_BUF_SPARSE / THZ_BUF_DENOISED: the spike trains
// or the denoised traces, on the grid and time axis of the cube they were taken of) with its grid, trace length and the mean step of its time axis;
// THZ_ERR_NOT_READY when it is absent
int session_cube(thz_session *s, int which, SessionCube *out);
// the ifft stage's avg_data (avg_in_fourier_space; needs the means): host-side, after session_means
int session_avg_data(thz_session *s, const thz_chain_cfg *cfg);
// The two buffers of a session that a group's stages size as well.  session_size_deconv: the Deconvolution stage's
// outputs (d_deconv, d_deconv_img) for the current grid; a resize clears deconv_current.  session_size_opacity: the
// opacity cube of the current grid.
int session_size_deconv(thz_session *s);
int session_size_opacity(thz_session *s);
