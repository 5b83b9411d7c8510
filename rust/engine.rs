//! Process-global record-and-flush engine behind the data thread (`src/gpu/engine.rs`).
//!
//! TRANSLITERATION of `thz_image_explorer_amd/host/thz_engine.{hpp,cpp}` (class `GpuEngine`): same fields, same
//! methods, same order of calls.  No Rust toolchain exists in the image this repository is built in, so the logic
//! is written, built and tested in C++ first (`tests/test_gpu_engine.py` drives it through the patched stage walk
//! against the oracle); this file is that code in the reference's language and is UNVERIFIED BY A COMPILER.
//!
//! Why an engine object at all: `Filter` objects are cloned before every run and only `#[static_field]` members are
//! copied back (`data_thread.rs:1069-1078, 1322-1334`), so device state cannot live in a plugin struct; it lives
//! here, behind a `once_cell::Lazy` (`once_cell` is already a dependency, `Cargo.toml:69`).  One `thz_group` drives
//! every GPU of the node from the single data thread (`data_thread.rs:162-174`); with one GPU the group is trivial
//! and RCCL is never loaded.
//!
//! How it meets the stage walk (`data_thread.rs:1090-1191`, as `rust/data_thread.patch` leaves it): the device
//! computes the whole chain in one launch, so a stage call only RECORDS its parameters — or, for a plugin the walk
//! passes through, its inactivity (`note_inactive`) — and returns a container without the big arrays; behind the
//! loop one `flush()` runs `thz_group_session_recompute` from the lowest chain position the walk touched, and
//! everything the code behind the loop reads is fetched from the device then.
use super::ffi::*;
use crate::filters::filter::{FilterConfig, FilterDomain};
use num_complex::Complex32;
use once_cell::sync::Lazy;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};
use std::ptr;
use std::sync::atomic::{AtomicBool, AtomicI32, Ordering};
use std::sync::{Arc, Mutex, RwLock};

/// chain positions of `thz_session_recompute_from`: the reference's `filter_chain` (`main.rs:182-247`) with all
/// `FilterDomain::Frequency` plugins on one position
pub const POS_SCALING: usize = 1;
pub const POS_TILT: usize = 2;
pub const POS_TD_BEFORE: usize = 3;
pub const POS_FFT: usize = 4;
pub const POS_FREQUENCY: usize = 5;
pub const POS_IFFT: usize = 6;
pub const POS_TD_AFTER: usize = 7;
pub const POS_DECONVOLUTION: usize = 8;

pub fn chain_position_of_domain(d: &FilterDomain) -> usize {
    match d {
        FilterDomain::TimeBeforeFFTPrioFirst => POS_TILT,
        FilterDomain::TimeBeforeFFT => POS_TD_BEFORE,
        FilterDomain::Frequency => POS_FREQUENCY,
        FilterDomain::TimeAfterFFT => POS_TD_AFTER,
        FilterDomain::TimeAfterFFTPrioLast => POS_DECONVOLUTION,
    }
}
/// "scaling" / "fft" / "ifft", else 0
pub fn chain_position_of_id(id: &str) -> usize {
    match id {
        "scaling" => POS_SCALING,
        "fft" => POS_FFT,
        "ifft" => POS_IFFT,
        _ => 0,
    }
}

/// `THZGPU_DEVICES=0,1,2,3` selects the GPUs; default: device 0.
fn devices_from_env() -> Vec<c_int> {
    std::env::var("THZGPU_DEVICES")
        .ok()
        .map(|s| s.split(',').filter_map(|t| t.trim().parse().ok()).collect::<Vec<c_int>>())
        .filter(|v| !v.is_empty())
        .unwrap_or_else(|| vec![0])
}

pub static ENGINE: Lazy<Mutex<GpuEngine>> = Lazy::new(|| Mutex::new(GpuEngine::new(&devices_from_env())));

pub type Polygon = Vec<(usize, usize)>;

pub struct GpuEngine {
    group: *mut ThzGroup,
    session: *mut ThzGroupSession,
    /// what the stage calls of the current walk have recorded
    pub pending: ThzChainCfg,
    /// lowest chain position touched since the last flush: the `start_stage` of the recompute
    dirty_from: usize,
    pub nx: usize,
    pub ny: usize,
    pub nt: usize,
    /// K14 / K13 per-bin multipliers; empty = that plugin is off
    fd_real: Vec<f32>,
    fd_cmask: Vec<f32>,
    plugins_dirty: bool,
    /// (uuid, polygon) of the ifft stage's regions, in the order the device holds them
    rois: Vec<(String, Polygon)>,
    rois_dirty: bool,
    /// the last `echo_map`: rows per local member, columns and ranks (0: none)
    echo_rows: Vec<usize>,
    echo_gy: usize,
    echo_k: usize,
    sparse_rows: Vec<usize>,
    sparse_gy: usize,
}

// the raw handles are only touched under the Mutex around the engine
unsafe impl Send for GpuEngine {}

impl GpuEngine {
    pub fn new(devices: &[c_int]) -> Self {
        let mut group = ptr::null_mut();
        let rc = unsafe { thz_group_create(devices.as_ptr(), devices.len() as c_int, &mut group) };
        if rc != THZ_OK {
            // no CPU compute path exists in the engine: the caller keeps the reference's own path
            let why = unsafe { CStr::from_ptr(thz_group_last_error(ptr::null())) }.to_string_lossy().into_owned();
            log::error!("thz_group_create({devices:?}) failed ({why}): GPU path disabled");
            group = ptr::null_mut();
        }
        let mut pending: ThzChainCfg = unsafe { std::mem::zeroed() };
        pending.scale_factor = 1;
        pending.want_means = 1;
        GpuEngine { group, session: ptr::null_mut(), pending, dirty_from: 1, nx: 0, ny: 0, nt: 0, fd_real: vec![], fd_cmask: vec![],
                    plugins_dirty: true, rois: vec![], rois_dirty: false, echo_rows: vec![], echo_gy: 0, echo_k: 0,
                    sparse_rows: vec![], sparse_gy: 0 }
    }

    pub fn available(&self) -> bool { !self.group.is_null() }

    pub fn last_error(&self) -> String {
        if self.group.is_null() { return "no GPU group".into(); }
        unsafe { CStr::from_ptr(thz_group_last_error(self.group)) }.to_string_lossy().into_owned()
    }

    /// `ConfigCommand::OpenFile` (`io.rs:576-628`): the cube goes to the device(s) once.  `subtract_bias`: false when
    /// the loader already did it (`open_scan_from_thz` does, `io.rs:578-586`).
    pub fn open_scan(&mut self, cube: &[f32], nx: usize, ny: usize, time: &[f32], dx: f32, dy: f32, subtract_bias: bool) -> bool {
        if self.group.is_null() { return false; }
        unsafe {
            if !self.session.is_null() { thz_group_session_destroy(self.session); self.session = ptr::null_mut(); }
            if thz_group_session_create(self.group, nx, ny, time.len(), time.as_ptr(), dx, dy, &mut self.session) != THZ_OK
                || thz_group_session_upload(self.session, cube.as_ptr(), subtract_bias as c_int) != THZ_OK
            {
                log::error!("open_scan: {}", self.last_error());
                if !self.session.is_null() { thz_group_session_destroy(self.session); }
                self.session = ptr::null_mut();
                return false;
            }
            thz_chain_cfg_default(time.as_ptr(), time.len(), &mut self.pending);
        }
        self.nx = nx; self.ny = ny; self.nt = time.len();
        self.dirty_from = 1;
        self.fd_real.clear();
        self.fd_cmask.clear();
        self.plugins_dirty = true;
        self.rois.clear();
        self.rois_dirty = false;
        true
    }

    fn touch(&mut self, position: usize) { if position < self.dirty_from { self.dirty_from = position.max(1); } }

    // ---- the stage walk of UpdateType::Filter(start_idx)
    pub fn begin_walk(&mut self, start_position: usize) { self.touch(start_position); }
    pub fn record_scaling(&mut self, scale_factor: usize) { self.pending.scale_factor = scale_factor as i32; self.touch(POS_SCALING); }
    pub fn record_tilt(&mut self, active: bool, tilt_x: f64, tilt_y: f64) {
        self.pending.tilt_active = active as i32;
        if active { self.pending.tilt_x_deg = tilt_x; self.pending.tilt_y_deg = tilt_y; }
        self.touch(POS_TILT);
    }
    pub fn record_td_before(&mut self, active: bool, low: f64, high: f64, width: f64) {
        self.pending.td_before_active = active as i32;
        if active { self.pending.td_before_low = low; self.pending.td_before_high = high; self.pending.td_before_width = width; }
        self.touch(POS_TD_BEFORE);
    }
    pub fn record_fft(&mut self, window_type: i32, lower: f32, upper: f32) {
        self.pending.fft_window = ThzWindowCfg { type_: window_type, lower, upper };
        self.touch(POS_FFT);
    }
    pub fn record_fd(&mut self, active: bool, low: f64, high: f64, width: f64) {
        self.pending.fd_active = active as i32;
        if active { self.pending.fd_low = low; self.pending.fd_high = high; self.pending.fd_width = width; }
        self.touch(POS_FREQUENCY);
    }
    /// K14: real per-bin multiplier (nf).  An unchanged multiplier does not invalidate the resident spectrum.
    pub fn record_water_lines(&mut self, active: bool, mask: Vec<f32>) {
        let mask = if active { mask } else { vec![] };
        if mask != self.fd_real { self.fd_real = mask; self.plugins_dirty = true; }
        self.touch(POS_FREQUENCY);
    }
    /// K13: complex per-bin multiplier (2 nf, interleaved)
    pub fn record_wiener(&mut self, active: bool, cmask: Vec<f32>) {
        let cmask = if active { cmask } else { vec![] };
        if cmask != self.fd_cmask { self.fd_cmask = cmask; self.plugins_dirty = true; }
        self.touch(POS_FREQUENCY);
    }
    /// the ifft stage: its regions (`input.rois`, `math_tools.rs:473-475`) and `config.avg_in_fourier_space` go with it
    pub fn record_ifft(&mut self, avg_in_fourier_space: bool, rois: Vec<(String, Polygon)>) {
        self.pending.avg_in_fourier_space = avg_in_fourier_space as i32;
        if rois != self.rois { self.rois = rois; self.rois_dirty = true; }
        self.touch(POS_IFFT);
    }
    pub fn record_td_after(&mut self, active: bool, low: f64, high: f64, width: f64) {
        self.pending.td_after_active = active as i32;
        if active { self.pending.td_after_low = low; self.pending.td_after_high = high; self.pending.td_after_width = width; }
        self.touch(POS_TD_AFTER);
    }
    /// the walk passed an inactive plugin's input through (`data_thread.rs:1185-1188`): its stage is off in the chain
    pub fn note_inactive(&mut self, cfg: &FilterConfig) {
        match cfg.domain {
            FilterDomain::TimeBeforeFFTPrioFirst => self.record_tilt(false, 0.0, 0.0),
            FilterDomain::TimeBeforeFFT => self.record_td_before(false, 0.0, 0.0, 0.0),
            FilterDomain::Frequency => {
                if cfg.name == "Water Line Notch" { self.record_water_lines(false, vec![]) }
                else if cfg.name == "Reference Wiener Filter" { self.record_wiener(false, vec![]) }
                else { self.record_fd(false, 0.0, 0.0, 0.0) }
            }
            FilterDomain::TimeAfterFFT => self.record_td_after(false, 0.0, 0.0, 0.0),
            // the stage hands its input on: an earlier deconvolved cube must not stay the chain's output.  The tail of
            // the chain (C2R, Time Band Pass, image) is what restores the stage's input as the final cube.
            FilterDomain::TimeAfterFFTPrioLast => self.touch(POS_TD_AFTER),
        }
    }

    /// Behind the stage loop (and in front of the Deconvolution stage): one recompute from the lowest touched position.
    pub fn flush(&mut self) -> bool {
        if self.session.is_null() { return false; }
        unsafe {
            if self.plugins_dirty {
                for i in 0..thz_group_local_count(self.group) {
                    let s = thz_group_session_member(self.session, i);
                    let nf = if !self.fd_real.is_empty() { self.fd_real.len() } else { self.fd_cmask.len() / 2 };
                    let r = if self.fd_real.is_empty() { ptr::null() } else { self.fd_real.as_ptr() };
                    let c = if self.fd_cmask.is_empty() { ptr::null() } else { self.fd_cmask.as_ptr() };
                    if thz_session_set_fd_filters(s, r, c, nf) != THZ_OK { log::error!("flush: set_fd_filters failed"); return false; }
                }
                self.plugins_dirty = false;
            }
            if self.rois_dirty {
                let counts: Vec<usize> = self.rois.iter().map(|r| r.1.len()).collect();
                let flat: Vec<u64> = self.rois.iter().flat_map(|r| r.1.iter().flat_map(|v| [v.0 as u64, v.1 as u64])).collect();
                if thz_group_session_set_rois(self.session, self.rois.len(), counts.as_ptr(), flat.as_ptr()) != THZ_OK {
                    log::error!("flush: set_rois: {}", self.last_error());
                    return false;
                }
                self.rois_dirty = false;
                self.touch(POS_IFFT);
            }
            if self.dirty_from > POS_DECONVOLUTION { return true; } // nothing recorded since the last flush
            if thz_group_session_recompute(self.session, &self.pending, self.dirty_from as c_int, THZ_GATHER_SMALL) != THZ_OK {
                log::error!("flush: {}", self.last_error());
                return false;
            }
        }
        self.dirty_from = POS_DECONVOLUTION + 1;
        true
    }

    /// The Deconvolution stage over the WHOLE group (`thz_group_session_deconvolve`: on one GPU the session's own
    /// stage, on several the phased form: per-pixel parts on every member's rows, per-band iterations); everything in front of the stage is flushed first.  Progress
    /// and abort are forwarded live: the engine polls a plain `int` between iteration batches and writes its
    /// progress into a `float`; a watcher thread bridges them to `abort_flag` / `progress_lock`.
    pub fn deconvolve(&mut self, psf: &ThzPsf, cfg: &ThzDeconvCfg, progress_lock: &Arc<RwLock<Option<f32>>>,
                      abort_flag: &Arc<AtomicBool>) -> c_int {
        if !self.flush() { return THZ_ERR_NOT_READY; }
        let abort_i32 = Arc::new(AtomicI32::new(abort_flag.load(Ordering::Relaxed) as i32));
        let progress = Box::into_raw(Box::new(0f32));
        let stop = Arc::new(AtomicBool::new(false));
        let (a2, src, lock, stop2, p_addr) = (abort_i32.clone(), abort_flag.clone(), progress_lock.clone(), stop.clone(), progress as usize);
        let watcher = std::thread::spawn(move || {
            while !stop2.load(Ordering::Acquire) {
                if src.load(Ordering::Relaxed) { a2.store(1, Ordering::Relaxed); }
                let p = unsafe { std::ptr::read_volatile(p_addr as *const f32) };
                if let Ok(mut g) = lock.write() { *g = Some(p); }
                std::thread::sleep(std::time::Duration::from_millis(1));
            }
        });
        let rc = unsafe { thz_group_session_deconvolve(self.session, psf, cfg, abort_i32.as_ptr() as *const c_int, progress) };
        stop.store(true, Ordering::Release);
        let _ = watcher.join();
        unsafe { drop(Box::from_raw(progress)); }
        if let Ok(mut g) = progress_lock.write() { *g = None; }
        rc
    }

    // ---- results of the last flush
    /// image on the outputs' grid (`nx / s` x `ny / s`) -> (values, gx, gy)
    pub fn image(&self) -> Option<(Vec<f32>, usize, usize)> {
        if self.session.is_null() { return None; }
        unsafe {
            let (mut gx, mut gy) = (self.nx, self.ny);
            let (mut rows, mut cols) = (0usize, 0usize);
            for i in 0..thz_group_local_count(self.group) {
                let (mut r, mut c) = (0usize, 0usize);
                thz_session_grid(thz_group_session_member(self.session, i), &mut r, &mut c, ptr::null_mut(), ptr::null_mut());
                rows += r; cols = c;
            }
            if thz_group_local_count(self.group) == thz_group_world(self.group) { gx = rows; gy = cols; }
            let mut img = vec![0f32; gx * gy];
            let mut rc = thz_group_session_download(self.session, THZ_BUF_IMG, 0, gx * gy, img.as_mut_ptr() as *mut c_void);
            if rc == THZ_ERR_NOT_READY { // before the first recompute: the upload's image of the raw grid
                rc = thz_session_download(thz_group_session_member(self.session, 0), THZ_BUF_IMG, 0, gx * gy, img.as_mut_ptr() as *mut c_void);
            }
            if rc == THZ_OK { Some((img, gx, gy)) } else { None }
        }
    }

    /// pixel means of the ifft stage (`math_tools.rs:421-440`): (avg_fft, avg_signal_fft, avg_phase_fft)
    pub fn averages(&self) -> Option<(Vec<Complex32>, Vec<f32>, Vec<f32>)> {
        if self.session.is_null() { return None; }
        let nf = self.nt_out() / 2 + 1;
        let mut f = vec![Complex32::new(0.0, 0.0); nf];
        let (mut a, mut p) = (vec![0f32; nf], vec![0f32; nf]);
        let ok = unsafe {
            thz_group_session_download(self.session, THZ_BUF_AVG_FFT, 0, 1, f.as_mut_ptr() as *mut c_void) == THZ_OK
                && thz_group_session_download(self.session, THZ_BUF_AVG_AMPLITUDES, 0, 1, a.as_mut_ptr() as *mut c_void) == THZ_OK
                && thz_group_session_download(self.session, THZ_BUF_AVG_PHASES, 0, 1, p.as_mut_ptr() as *mut c_void) == THZ_OK
        };
        if ok { Some((f, a, p)) } else { None }
    }

    /// the member whose slab holds raw row `px` (`thz_host_slab`: the partition the library itself uses)
    fn owner_of(&self, px: usize) -> Option<(*mut ThzSession, usize)> {
        unsafe {
            let world = thz_group_world(self.group);
            for i in 0..thz_group_local_count(self.group) {
                let (mut x0, mut n) = (0usize, 0usize);
                thz_host_slab(self.nx, world, thz_group_rank(self.group, i), &mut x0, &mut n);
                if px >= x0 && px < x0 + n { return Some((thz_group_session_member(self.session, i), px - x0)); }
            }
        }
        None
    }

    /// `UpdateType::Plot` copy-out for pixel (px, py) of the RAW grid (`data_thread.rs:1337-1432`)
    pub fn plot(&self, px: usize, py: usize, out: &ThzPlotOut) -> bool {
        if self.session.is_null() { return false; }
        let (s, lx) = match self.owner_of(px) { Some(v) => v, None => return false };
        let sf = if self.pending.scale_factor > 1 { self.pending.scale_factor as usize } else { 1 };
        unsafe {
            if sf == 1 || thz_group_world(self.group) == 1 { return thz_session_plot(s, lx, py, out) == THZ_OK; }
            // Several slabs behind a scaling stage: the raw trace comes from the slab that holds row px, everything else
            // from the slab that holds the pixel's BLOCK — the one with the block's last raw row
            let mut raw = crate::math_tools_gpu::empty_plot_out();
            raw.signal = out.signal;
            if !out.signal.is_null() && thz_session_plot(s, lx, py, &raw) != THZ_OK { return false; }
            let mut rest = ThzPlotOut { ..*out };
            rest.signal = ptr::null_mut();
            match self.owner_of((px / sf) * sf + sf - 1) {
                Some((sb, lb)) => thz_session_plot(sb, lb, py, &rest) == THZ_OK,
                None => false,
            }
        }
    }

    /// one region's vectors (`math_tools.rs:473-543`, `data_thread.rs:1442-1482`)
    pub fn roi(&self, uuid: &str, out: &ThzRoiOut) -> bool {
        if self.session.is_null() { return false; }
        match self.rois.iter().position(|r| r.0 == uuid) {
            Some(i) => unsafe { thz_group_session_roi(self.session, i, out) == THZ_OK },
            None => false,
        }
    }

    pub fn nt_out(&self) -> usize {
        if self.session.is_null() { 0 } else { unsafe { thz_session_nt_out(thz_group_session_member(self.session, 0)) } }
    }
    pub fn time_out(&self) -> Vec<f32> {
        let mut t = vec![0f32; self.nt_out()];
        if !self.session.is_null() && !t.is_empty() { unsafe { thz_session_time_out(thz_group_session_member(self.session, 0), t.as_mut_ptr()); } }
        t
    }

    /// The angles that flatten the pulse's arrival plane over the WHOLE grid (`thz_group_session_estimate_tilt`): of the
    /// raw cube (`which = THZ_BUF_RAW`) or of the chain's final traces (`THZ_BUF_DATA`; whatever the walk has recorded
    /// is flushed first).  `mode` 0 largest |x|, 1 maximum, 2 minimum.  `None`: no session, no plane, or an error.
    pub fn estimate_tilt(&mut self, which: c_int, mode: c_int, rel_threshold: f32) -> Option<ThzTiltFit> {
        if self.session.is_null() { return None; }
        if which == THZ_BUF_DATA && !self.flush() { return None; }
        let mut fit: ThzTiltFit = unsafe { std::mem::zeroed() };
        let rc = unsafe { thz_group_session_estimate_tilt(self.session, which, mode, rel_threshold, &mut fit) };
        if rc < 0 { log::error!("estimate_tilt: {}", self.last_error()); }
        if rc == THZ_OK { Some(fit) } else { None }
    }

    /// Refractive index, absorption and extinction over every pixel this process holds, as means over `cfg`'s bands
    /// (`thz_session_optical_maps` on each local member's resident spectra, the slabs' rows one after the other; whatever
    /// the walk has recorded is flushed first).  `ref_amp` / `ref_phase`: a reference's `roi_signal_fft` /
    /// `roi_phase_fft` (`nt_out / 2 + 1` values, `OpenRef`); `cfg`: `sample_thickness`, the anchor and the bands as bin
    /// ranges.  -> (n, alpha, kappa: (n_bands, gx, gy); wraps, slope: (gx, gy); gx; gy)
    pub fn optical_maps(&mut self, ref_amp: &[f32], ref_phase: &[f32], cfg: &ThzOpticalCfg)
                        -> Option<(Vec<f32>, Vec<f32>, Vec<f32>, Vec<i32>, Vec<f32>, usize, usize)> {
        if self.session.is_null() || ref_amp.len() != ref_phase.len() || !self.flush() { return None; }
        unsafe {
            let members = thz_group_local_count(self.group);
            let mut rows = vec![0usize; members as usize];
            let (mut gx, mut gy) = (0usize, 0usize);
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                if thz_session_optical_maps(s, ref_amp.as_ptr(), ref_phase.as_ptr(), ref_amp.len(), cfg, ptr::null()) != THZ_OK { return None; }
                thz_session_grid(s, &mut rows[i as usize], &mut gy, ptr::null_mut(), ptr::null_mut());
                gx += rows[i as usize];
            }
            let (nb, npix) = (cfg.n_bands as usize, gx * gy);
            let (mut n, mut alpha, mut kappa) = (vec![0f32; nb * npix], vec![0f32; nb * npix], vec![0f32; nb * npix]);
            let (mut wraps, mut slope) = (vec![0i32; npix], vec![0f32; npix]);
            let mut at = 0usize; // pixels of the members in front
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                let mine = rows[i as usize] * gy;
                if mine == 0 { continue; }
                for b in 0..nb { // a member's maps are band-major over ITS pixels
                    if thz_session_download(s, THZ_BUF_OPT_N, b * mine, mine, n.as_mut_ptr().add(b * npix + at) as *mut c_void) != THZ_OK
                        || thz_session_download(s, THZ_BUF_OPT_ALPHA, b * mine, mine, alpha.as_mut_ptr().add(b * npix + at) as *mut c_void) != THZ_OK
                        || thz_session_download(s, THZ_BUF_OPT_KAPPA, b * mine, mine, kappa.as_mut_ptr().add(b * npix + at) as *mut c_void) != THZ_OK {
                        return None;
                    }
                }
                if thz_session_download(s, THZ_BUF_OPT_WRAPS, 0, mine, wraps.as_mut_ptr().add(at) as *mut c_void) != THZ_OK
                    || thz_session_download(s, THZ_BUF_OPT_SLOPE, 0, mine, slope.as_mut_ptr().add(at) as *mut c_void) != THZ_OK {
                    return None;
                }
                at += mine;
            }
            Some((n, alpha, kappa, wraps, slope, gx, gy))
        }
    }

    /// The `cfg.n_echoes` strongest separated pulses of every trace this process holds (`thz_session_echo_map` on each
    /// local member, slab after slab: every pixel is independent), of the raw cube (`which = THZ_BUF_RAW`) or of the
    /// chain's final traces (`THZ_BUF_DATA`; whatever the walk has recorded is flushed first), or of the spike trains of
    /// the last `sparse_deconv` (`THZ_BUF_SPARSE`, on the grid of the cube they were taken of).
    /// -> (index, offset, value: (n_echoes, gx, gy), rank-major with index -1 for a rank that was not found;
    /// count: (gx, gy); gx; gy)
    pub fn echo_map(&mut self, which: c_int, cfg: &ThzEchoCfg) -> Option<(Vec<i32>, Vec<f32>, Vec<f32>, Vec<i32>, usize, usize)> {
        self.echo_k = 0;
        if self.session.is_null() || (which != THZ_BUF_RAW && which != THZ_BUF_DATA && which != THZ_BUF_SPARSE) { return None; }
        if which == THZ_BUF_DATA && !self.flush() { return None; }
        unsafe {
            let members = thz_group_local_count(self.group);
            if which == THZ_BUF_SPARSE && self.sparse_rows.len() != members as usize { return None; } // no sparse_deconv has run
            self.echo_rows = vec![0usize; members as usize];
            let (mut gx, mut gy) = (0usize, 0usize);
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                if thz_session_echo_map(s, which, cfg) != THZ_OK { return None; }
                if which == THZ_BUF_SPARSE { // the grid of the cube the spike trains were taken of
                    self.echo_rows[i as usize] = self.sparse_rows[i as usize];
                    gy = self.sparse_gy;
                } else if which == THZ_BUF_RAW { // the member's slab of the raw grid
                    let mut x0 = 0usize;
                    thz_host_slab(self.nx, thz_group_world(self.group), thz_group_rank(self.group, i), &mut x0, &mut self.echo_rows[i as usize]);
                    gy = self.ny;
                } else {
                    thz_session_grid(s, &mut self.echo_rows[i as usize], &mut gy, ptr::null_mut(), ptr::null_mut());
                }
                gx += self.echo_rows[i as usize];
            }
            let (k, npix) = (cfg.n_echoes as usize, gx * gy);
            let (mut index, mut offset, mut value, mut count) = (vec![-1i32; k * npix], vec![0f32; k * npix], vec![0f32; k * npix], vec![0i32; npix]);
            let mut at = 0usize; // pixels of the members in front
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                let mine = self.echo_rows[i as usize] * gy;
                if mine == 0 { continue; }
                for j in 0..k { // a member's maps are rank-major over ITS pixels
                    if thz_session_download(s, THZ_BUF_ECHO_INDEX, j * mine, mine, index.as_mut_ptr().add(j * npix + at) as *mut c_void) != THZ_OK
                        || thz_session_download(s, THZ_BUF_ECHO_OFFSET, j * mine, mine, offset.as_mut_ptr().add(j * npix + at) as *mut c_void) != THZ_OK
                        || thz_session_download(s, THZ_BUF_ECHO_VALUE, j * mine, mine, value.as_mut_ptr().add(j * npix + at) as *mut c_void) != THZ_OK {
                        return None;
                    }
                }
                if thz_session_download(s, THZ_BUF_ECHO_COUNT, 0, mine, count.as_mut_ptr().add(at) as *mut c_void) != THZ_OK { return None; }
                at += mine;
            }
            self.echo_gy = gy;
            self.echo_k = k;
            Some((index, offset, value, count, gx, gy))
        }
    }

    /// Sparse deconvolution of every trace this process holds (`thz_session_sparse_deconv` on each local
    /// member, slab after slab: every pixel is independent), of the raw cube (`which = THZ_BUF_RAW`) or of the chain's
    /// final traces (`THZ_BUF_DATA`; whatever the walk has recorded is flushed first).  `taps`: `cfg.n_taps` values, e.g.
    /// what `thz_host_sparse_kernel` cuts out of a reference pulse.  Every member's `THZ_BUF_SPARSE / _SPARSE_RESID /
    /// _SPARSE_NNZ` stay resident: `echo_map(THZ_BUF_SPARSE, ..)` and `layer_map` then turn the spikes of a thin coating
    /// into its thickness.
    /// -> (x: (gx, gy, nt_src) spike trains; resid, nnz: (gx, gy); gx; gy; nt_src)
    pub fn sparse_deconv(&mut self, which: c_int, taps: &[f32], cfg: &ThzSparseCfg) -> Option<(Vec<f32>, Vec<f32>, Vec<i32>, usize, usize, usize)> {
        self.sparse_rows.clear();
        if self.session.is_null() || (which != THZ_BUF_RAW && which != THZ_BUF_DATA) || cfg.n_taps < 1 || taps.len() != cfg.n_taps as usize { return None; }
        if which == THZ_BUF_DATA && !self.flush() { return None; }
        unsafe {
            let members = thz_group_local_count(self.group);
            let mut rows = vec![0usize; members as usize];
            let (mut gx, mut gy, mut nt_src) = (0usize, 0usize, 0usize);
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                if thz_session_sparse_deconv(s, which, taps.as_ptr(), cfg) != THZ_OK { return None; }
                if which == THZ_BUF_RAW { // the member's slab of the raw grid
                    let mut x0 = 0usize;
                    thz_host_slab(self.nx, thz_group_world(self.group), thz_group_rank(self.group, i), &mut x0, &mut rows[i as usize]);
                    gy = self.ny;
                    nt_src = self.nt;
                } else {
                    thz_session_grid(s, &mut rows[i as usize], &mut gy, ptr::null_mut(), ptr::null_mut());
                    nt_src = thz_session_nt_out(s);
                }
                gx += rows[i as usize];
            }
            let npix = gx * gy;
            let (mut x, mut resid, mut nnz) = (vec![0f32; npix * nt_src], vec![0f32; npix], vec![0i32; npix]);
            let mut at = 0usize; // pixels of the members in front
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                let mine = rows[i as usize] * gy;
                if mine == 0 { continue; }
                if thz_session_download(s, THZ_BUF_SPARSE, 0, mine, x.as_mut_ptr().add(at * nt_src) as *mut c_void) != THZ_OK
                    || thz_session_download(s, THZ_BUF_SPARSE_RESID, 0, mine, resid.as_mut_ptr().add(at) as *mut c_void) != THZ_OK
                    || thz_session_download(s, THZ_BUF_SPARSE_NNZ, 0, mine, nnz.as_mut_ptr().add(at) as *mut c_void) != THZ_OK {
                    return None;
                }
                at += mine;
            }
            self.sparse_rows = rows;
            self.sparse_gy = gy;
            Some((x, resid, nnz, gx, gy, nt_src))
        }
    }

    /// Wavelet shrinkage of every trace this process holds (`thz_session_wavelet_denoise` on each local
    /// member, slab after slab: every pixel is independent), of the raw cube (`which = THZ_BUF_RAW`) or of the chain's
    /// final traces (`THZ_BUF_DATA`; whatever the walk has recorded is flushed first).  `hn`, `gn`: `cfg.n_taps` analysis
    /// taps each, e.g. `thz_host_wavelet_filter`'s; `scale`: `cfg.n_levels` thresholds, e.g.
    /// `thz_host_wavelet_universal`'s.  Every member's `THZ_BUF_DENOISED / _DENOISE_SIGMA / _DENOISE_KEPT` stay resident.
    /// -> (x: (gx, gy, nt_src) denoised traces; sigma, kept: (gx, gy); gx; gy; nt_src)
    pub fn wavelet_denoise(&mut self, which: c_int, hn: &[f32], gn: &[f32], scale: &[f32], cfg: &ThzWaveletCfg) -> Option<(Vec<f32>, Vec<f32>, Vec<i32>, usize, usize, usize)> {
        if self.session.is_null() || (which != THZ_BUF_RAW && which != THZ_BUF_DATA) || cfg.n_taps < 1 || cfg.n_levels < 1
            || hn.len() != cfg.n_taps as usize || gn.len() != hn.len() || scale.len() != cfg.n_levels as usize { return None; }
        if which == THZ_BUF_DATA && !self.flush() { return None; }
        unsafe {
            let members = thz_group_local_count(self.group);
            let mut rows = vec![0usize; members as usize];
            let (mut gx, mut gy, mut nt_src) = (0usize, 0usize, 0usize);
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                if thz_session_wavelet_denoise(s, which, hn.as_ptr(), gn.as_ptr(), scale.as_ptr(), cfg) != THZ_OK { return None; }
                if which == THZ_BUF_RAW { // the member's slab of the raw grid
                    let mut x0 = 0usize;
                    thz_host_slab(self.nx, thz_group_world(self.group), thz_group_rank(self.group, i), &mut x0, &mut rows[i as usize]);
                    gy = self.ny;
                    nt_src = self.nt;
                } else {
                    thz_session_grid(s, &mut rows[i as usize], &mut gy, ptr::null_mut(), ptr::null_mut());
                    nt_src = thz_session_nt_out(s);
                }
                gx += rows[i as usize];
            }
            let npix = gx * gy;
            let (mut x, mut sigma, mut kept) = (vec![0f32; npix * nt_src], vec![0f32; npix], vec![0i32; npix]);
            let mut at = 0usize; // pixels of the members in front
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                let mine = rows[i as usize] * gy;
                if mine == 0 { continue; }
                if thz_session_download(s, THZ_BUF_DENOISED, 0, mine, x.as_mut_ptr().add(at * nt_src) as *mut c_void) != THZ_OK
                    || thz_session_download(s, THZ_BUF_DENOISE_SIGMA, 0, mine, sigma.as_mut_ptr().add(at) as *mut c_void) != THZ_OK
                    || thz_session_download(s, THZ_BUF_DENOISE_KEPT, 0, mine, kept.as_mut_ptr().add(at) as *mut c_void) != THZ_OK {
                    return None;
                }
                at += mine;
            }
            Some((x, sigma, kept, gx, gy, nt_src))
        }
    }

    /// Delays and thicknesses from the last `echo_map` (`thz_session_layer_map` on each local member): (rows, gx, gy)
    /// with rows = n_echoes - 1 between consecutive pulses (`cfg.mode` 0) and 1 against a fixed arrival (`cfg.mode` 1).
    /// A member's `THZ_BUF_LAYER_THICKNESS` stays resident: a row of it is a valid `d_thickness` of
    /// `thz_session_optical_maps`.  -> (thickness, delay, rows, gx, gy)
    pub fn layer_map(&mut self, cfg: &ThzLayerCfg) -> Option<(Vec<f32>, Vec<f32>, usize, usize, usize)> {
        if self.session.is_null() || self.echo_k == 0 || (cfg.mode == 0 && self.echo_k < 2) { return None; }
        unsafe {
            let members = thz_group_local_count(self.group);
            if members as usize != self.echo_rows.len() { return None; }
            for i in 0..members {
                if thz_session_layer_map(thz_group_session_member(self.session, i), cfg) != THZ_OK { return None; }
            }
            let rows = if cfg.mode == 0 { self.echo_k - 1 } else { 1 };
            let gy = self.echo_gy;
            let gx: usize = self.echo_rows.iter().sum();
            let npix = gx * gy;
            let (mut thickness, mut delay) = (vec![0f32; rows * npix], vec![0f32; rows * npix]);
            let mut at = 0usize;
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                let mine = self.echo_rows[i as usize] * gy;
                if mine == 0 { continue; }
                for l in 0..rows {
                    if thz_session_download(s, THZ_BUF_LAYER_THICKNESS, l * mine, mine, thickness.as_mut_ptr().add(l * npix + at) as *mut c_void) != THZ_OK
                        || thz_session_download(s, THZ_BUF_LAYER_DELAY, l * mine, mine, delay.as_mut_ptr().add(l * npix + at) as *mut c_void) != THZ_OK {
                        return None;
                    }
                }
                at += mine;
            }
            Some((thickness, delay, rows, gx, gy))
        }
    }

    /// Principal components of everything this process holds: the covariance is not pixel-independent, so
    /// `thz_session_pca_sums` and `thz_session_pca_gram` run on each local member, the members' sums and Gram matrices
    /// are added here in member order (f64), `thz_host_pca_components` runs once, and `thz_session_pca_project` fills
    /// each member's `THZ_BUF_PCA_SCORES / _COMPONENTS / _MEAN` with the common mean and components.  `which`:
    /// `THZ_BUF_AMPLITUDES`, `_PHASES`, `_DATA` (whatever the walk has recorded is flushed first) or `_RAW`;
    /// `cfg.d_mask` is not read: `mask` is empty or one byte per pixel of the whole (gx, gy) grid, 0 leaving the pixel
    /// out of mean and covariance.
    /// -> (out; scores (n_components, gx, gy); components (n_components, count); mean (count), zeros when
    /// `cfg.center == 0`; gx; gy)
    pub fn pca(&mut self, which: c_int, cfg: &ThzPcaCfg, mask: &[u8]) -> Option<(ThzPcaOut, Vec<f32>, Vec<f32>, Vec<f32>, usize, usize)> {
        if self.session.is_null() || cfg.count < 1 || cfg.count > THZ_PCA_MAX_LEN as u32 || cfg.n_components < 1
            || cfg.n_components > THZ_PCA_MAX_COMPONENTS || cfg.n_components as u32 > cfg.count { return None; }
        if which != THZ_BUF_RAW && !self.flush() { return None; }
        unsafe {
            let members = thz_group_local_count(self.group);
            let mut rows = vec![0usize; members as usize];
            let (mut gx, mut gy) = (0usize, 0usize);
            for i in 0..members {
                if which == THZ_BUF_RAW { // the member's slab of the raw grid
                    let mut x0 = 0usize;
                    thz_host_slab(self.nx, thz_group_world(self.group), thz_group_rank(self.group, i), &mut x0, &mut rows[i as usize]);
                    gy = self.ny;
                } else {
                    thz_session_grid(thz_group_session_member(self.session, i), &mut rows[i as usize], &mut gy, ptr::null_mut(), ptr::null_mut());
                }
                gx += rows[i as usize];
            }
            let (l, k, npix) = (cfg.count as usize, cfg.n_components as usize, gx * gy);
            if !mask.is_empty() && mask.len() != npix { return None; }
            // every member's rows of the mask on that member's device, for the length of this call
            let mut d_mask: Vec<*mut c_void> = vec![ptr::null_mut(); members as usize];
            let mut cfgs = vec![*cfg; members as usize];
            let mut ok = true;
            let mut at = 0usize; // pixels of the members in front
            for i in 0..members {
                let mine = rows[i as usize] * gy;
                cfgs[i as usize].d_mask = ptr::null();
                if ok && !mask.is_empty() && mine > 0 {
                    let ctx = thz_group_ctx(self.group, i);
                    ok = thz_malloc(ctx, &mut d_mask[i as usize], mine) == THZ_OK
                        && thz_memcpy_h2d(ctx, d_mask[i as usize], mask.as_ptr().add(at) as *const c_void, mine) == THZ_OK;
                    cfgs[i as usize].d_mask = d_mask[i as usize] as *const u8;
                }
                at += mine;
            }
            // calls 1 and 2 on every member, added in member order
            let (mut sum, mut gram, mut part) = (vec![0f64; l], vec![0f64; l * l], vec![0f64; l * l]);
            let mut count = 0u64;
            for i in 0..members {
                if !ok || rows[i as usize] == 0 { continue; }
                let mut n = 0u64;
                ok = thz_session_pca_sums(thz_group_session_member(self.session, i), which, &cfgs[i as usize], part.as_mut_ptr(), &mut n) == THZ_OK;
                if ok { for j in 0..l { sum[j] += part[j]; } }
                count += n;
            }
            ok = ok && count >= 2;
            let mut mean = vec![0f32; l];
            if ok && cfg.center != 0 { for j in 0..l { mean[j] = (sum[j] / count as f64) as f32; } }
            let mu: *const f32 = if cfg.center != 0 { mean.as_ptr() } else { ptr::null() };
            for i in 0..members {
                if !ok || rows[i as usize] == 0 { continue; }
                ok = thz_session_pca_gram(thz_group_session_member(self.session, i), which, &cfgs[i as usize], mu, part.as_mut_ptr()) == THZ_OK;
                if ok { for j in 0..l * l { gram[j] += part[j]; } }
            }
            // the components once, then call 4 per member
            let mut out: ThzPcaOut = std::mem::zeroed();
            out.count = count;
            let mut components = vec![0f32; k * l];
            ok = ok && thz_host_pca_components(gram.as_ptr(), l, count, k as c_int, components.as_mut_ptr(), out.eigenvalues.as_mut_ptr(), &mut out.total_variance) == THZ_OK;
            let mut scores = vec![0f32; k * npix];
            at = 0;
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                let mine = rows[i as usize] * gy;
                if !ok || mine == 0 { continue; }
                ok = thz_session_pca_project(s, which, &cfgs[i as usize], mu, components.as_ptr()) == THZ_OK;
                for c in 0..k { // a member's scores are component-major over ITS pixels
                    ok = ok && thz_session_download(s, THZ_BUF_PCA_SCORES, c * mine, mine, scores.as_mut_ptr().add(c * npix + at) as *mut c_void) == THZ_OK;
                }
                at += mine;
            }
            for i in 0..members {
                if !d_mask[i as usize].is_null() { thz_free(thz_group_ctx(self.group, i), d_mask[i as usize]); }
            }
            if ok { Some((out, scores, components, mean, gx, gy)) } else { None }
        }
    }

    /// k-means of everything this process holds: clustering is not pixel-independent, so `thz_session_cluster_step` runs on
    /// each local member and the members' sums, counts, inertia and changed are added here in member order (f64); the
    /// farthest pixel is the largest `THZ_BUF_CLUSTER_DIST` entry among the members' candidates, the lowest global index
    /// winning a tie, and `thz_session_cluster_row` fetches its row; `thz_host_cluster_update` runs once per step, and every
    /// member iterates with the common centroids.  The mean the seeding starts from is the sum of a K = 1 step about the
    /// zero vector (rows with a NaN are left out of it).  `which`: what `thz_session_cluster` takes;
    /// `THZ_BUF_PCA_SCORES` means the score images of the last `pca()` of the recompute's grid and takes no mask.
    /// `cfg.d_mask` is not read: `mask` is empty or one byte per pixel of the whole (gx, gy) grid.  Every member's
    /// `THZ_BUF_CLUSTER_LABELS / _DIST / _CENTROIDS` stay resident.
    /// -> (out; labels (gx, gy); dist2 (gx, gy); centroids (n_clusters, count); gx; gy)
    pub fn cluster(&mut self, which: c_int, cfg: &ThzClusterCfg, mask: &[u8]) -> Option<(ThzClusterOut, Vec<i32>, Vec<f32>, Vec<f32>, usize, usize)> {
        if self.session.is_null() || cfg.count < 1 || cfg.count > THZ_PCA_MAX_LEN as u32 || cfg.n_clusters < 1
            || cfg.n_clusters > THZ_CLUSTER_MAX || (cfg.init != 0 && cfg.init != 1) || cfg.max_iter < 1 || cfg.max_iter > 1000
            || (cfg.init == 0 && cfg.centroids.is_null()) || (which == THZ_BUF_PCA_SCORES && !mask.is_empty()) { return None; }
        if which != THZ_BUF_RAW && !self.flush() { return None; }
        unsafe {
            let members = thz_group_local_count(self.group);
            let mut rows = vec![0usize; members as usize];
            let (mut gx, mut gy) = (0usize, 0usize);
            for i in 0..members {
                if which == THZ_BUF_RAW { // the member's slab of the raw grid
                    let mut x0 = 0usize;
                    thz_host_slab(self.nx, thz_group_world(self.group), thz_group_rank(self.group, i), &mut x0, &mut rows[i as usize]);
                    gy = self.ny;
                } else {
                    thz_session_grid(thz_group_session_member(self.session, i), &mut rows[i as usize], &mut gy, ptr::null_mut(), ptr::null_mut());
                }
                gx += rows[i as usize];
            }
            let (l, k_all, npix) = (cfg.count as usize, cfg.n_clusters as usize, gx * gy);
            if npix == 0 || (!mask.is_empty() && mask.len() != npix) { return None; }
            // every member's rows of the mask on that member's device, for the length of this call
            let mut d_mask: Vec<*mut c_void> = vec![ptr::null_mut(); members as usize];
            let mut cfgs = vec![*cfg; members as usize];
            let pix: Vec<usize> = rows.iter().map(|r| r * gy).collect();
            let mut ok = true;
            let mut at = 0usize; // pixels of the members in front
            for i in 0..members as usize {
                cfgs[i].d_mask = ptr::null();
                if ok && !mask.is_empty() && pix[i] > 0 {
                    let ctx = thz_group_ctx(self.group, i as c_int);
                    ok = thz_malloc(ctx, &mut d_mask[i], pix[i]) == THZ_OK
                        && thz_memcpy_h2d(ctx, d_mask[i], mask.as_ptr().add(at) as *const c_void, pix[i]) == THZ_OK;
                    cfgs[i].d_mask = d_mask[i] as *const u8;
                }
                at += pix[i];
            }
            // one step on every member with k rows of `cent`, added in member order
            // -> (sums, counts, inertia, changed, the farthest pixel's global index or npix)
            let session = self.session;
            let step = |cent: &[f32], k: usize, reset: bool, want_sums: bool| -> Option<(Vec<f64>, [u64; 16], f64, u64, usize)> {
                let (mut sums, mut part) = (vec![0f64; k * l], vec![0f64; k * l]);
                let (mut counts, mut inertia, mut changed, mut far, mut best, mut before) = ([0u64; 16], 0f64, 0u64, npix, -1f32, 0usize);
                for i in 0..members as usize {
                    if pix[i] == 0 { continue; }
                    let s = thz_group_session_member(session, i as c_int);
                    let mut c = cfgs[i];
                    c.n_clusters = k as i32;
                    c.init = reset as i32;
                    let (mut n, mut e, mut ch, mut f) = ([0u64; 16], 0f64, 0u64, 0u64);
                    let p = if want_sums { part.as_mut_ptr() } else { ptr::null_mut() };
                    if thz_session_cluster_step(s, which, &c, cent.as_ptr(), p, n.as_mut_ptr(), &mut e, &mut ch, &mut f) != THZ_OK { return None; }
                    if want_sums { for j in 0..k * l { sums[j] += part[j]; } }
                    for j in 0..k { counts[j] += n[j]; }
                    inertia += e;
                    changed += ch;
                    if (f as usize) < pix[i] {
                        let mut v = 0f32;
                        if thz_session_download(s, THZ_BUF_CLUSTER_DIST, f as usize, 1, &mut v as *mut f32 as *mut c_void) != THZ_OK { return None; }
                        if v > best { best = v; far = before + f as usize; } // members ascend in the global index: the first stays
                    }
                    before += pix[i];
                }
                Some((sums, counts, inertia, changed, far))
            };
            let row = |mut p: usize, dst: &mut [f32]| -> bool {
                for i in 0..members as usize {
                    if p < pix[i] { return thz_session_cluster_row(thz_group_session_member(session, i as c_int), which, &cfgs[i], p as u64, dst.as_mut_ptr()) == THZ_OK; }
                    p -= pix[i];
                }
                false
            };
            let mut centroids = vec![0f32; k_all * l];
            if ok && cfg.init == 0 {
                ptr::copy_nonoverlapping(cfg.centroids, centroids.as_mut_ptr(), k_all * l);
            } else if ok {
                // farthest-first: the mean from the sums about the zero vector, then the farthest pixel each time
                let mut mean = vec![0f32; l];
                match step(&mean, 1, true, true) {
                    Some((sums, counts, _, _, _)) if counts[0] > 0 => { for j in 0..l { mean[j] = (sums[j] / counts[0] as f64) as f32; } }
                    _ => ok = false,
                }
                for k in 0..k_all {
                    if !ok { break; }
                    let got = if k == 0 { step(&mean, 1, true, false) } else { step(&centroids[..k * l], k, true, false) };
                    match got {
                        Some((_, _, _, _, far)) if far < npix => ok = row(far, &mut centroids[k * l..(k + 1) * l]),
                        Some(_) if k > 0 => centroids.copy_within((k - 1) * l..k * l, k * l),
                        _ => ok = false,
                    }
                }
            }
            let mut out: ThzClusterOut = std::mem::zeroed();
            let mut next = vec![0f32; k_all * l];
            for it in 1..=cfg.max_iter {
                if !ok { break; }
                match step(&centroids, k_all, it == 1, true) {
                    Some((sums, counts, inertia, changed, _)) => {
                        out.iterations = it;
                        out.converged = (changed == 0) as i32;
                        out.inertia = inertia;
                        out.count = 0;
                        for c in 0..k_all { out.counts[c] = counts[c]; out.count += counts[c]; }
                        if changed == 0 || it == cfg.max_iter { break; }
                        ok = thz_host_cluster_update(sums.as_ptr(), counts.as_ptr(), k_all as c_int, l, centroids.as_ptr(), next.as_mut_ptr()) == THZ_OK;
                        std::mem::swap(&mut centroids, &mut next);
                    }
                    None => ok = false,
                }
            }
            let (mut labels, mut dist2) = (vec![-1i32; npix], vec![0f32; npix]);
            at = 0;
            for i in 0..members as usize {
                if !ok || pix[i] == 0 { continue; }
                let s = thz_group_session_member(self.session, i as c_int);
                ok = thz_session_download(s, THZ_BUF_CLUSTER_LABELS, 0, pix[i], labels.as_mut_ptr().add(at) as *mut c_void) == THZ_OK
                    && thz_session_download(s, THZ_BUF_CLUSTER_DIST, 0, pix[i], dist2.as_mut_ptr().add(at) as *mut c_void) == THZ_OK;
                at += pix[i];
            }
            for i in 0..members as usize {
                if !d_mask[i].is_null() { thz_free(thz_group_ctx(self.group, i as c_int), d_mask[i]); }
            }
            if ok { Some((out, labels, dist2, centroids, gx, gy)) } else { None }
        }
    }

    /// Non-negative least squares of every pixel this process holds against `cfg.n_endmembers` spectra (DESIGN.md 4.12;
    /// `thz_session_unmix` on each local member, slab after slab: every pixel is independent).  `which`:
    /// `THZ_BUF_AMPLITUDES`, `_PHASES`, `_DATA` (whatever the walk has recorded is flushed first) or `_RAW`.
    /// `cfg.endmembers` null takes each member's resident `THZ_BUF_CLUSTER_CENTROIDS` — the ones `cluster` left on every
    /// member.  Every member's `THZ_BUF_UNMIX_*` stay resident.
    /// -> (abundance (n_endmembers, gx, gy); resid, kkt (gx, gy); gx; gy)
    pub fn unmix(&mut self, which: c_int, cfg: &ThzUnmixSessionCfg) -> Option<(Vec<f32>, Vec<f32>, Vec<f32>, usize, usize)> {
        if self.session.is_null() || cfg.n_endmembers < 1 || cfg.n_endmembers > THZ_UNMIX_MAX { return None; }
        if which != THZ_BUF_RAW && !self.flush() { return None; }
        unsafe {
            let members = thz_group_local_count(self.group);
            let mut rows = vec![0usize; members as usize];
            let (mut gx, mut gy) = (0usize, 0usize);
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                if which == THZ_BUF_RAW { // the member's slab of the raw grid
                    let mut x0 = 0usize;
                    thz_host_slab(self.nx, thz_group_world(self.group), thz_group_rank(self.group, i), &mut x0, &mut rows[i as usize]);
                    gy = self.ny;
                } else {
                    thz_session_grid(s, &mut rows[i as usize], &mut gy, ptr::null_mut(), ptr::null_mut());
                }
                if rows[i as usize] != 0 && thz_session_unmix(s, which, cfg) != THZ_OK { return None; }
                gx += rows[i as usize];
            }
            let (k, npix) = (cfg.n_endmembers as usize, gx * gy);
            let (mut abundance, mut resid, mut kkt) = (vec![0f32; k * npix], vec![0f32; npix], vec![0f32; npix]);
            let mut at = 0usize; // pixels of the members in front
            for i in 0..members {
                let s = thz_group_session_member(self.session, i);
                let mine = rows[i as usize] * gy;
                if mine == 0 { continue; }
                for c in 0..k { // a member's abundances are endmember-major over ITS pixels
                    if thz_session_download(s, THZ_BUF_UNMIX_ABUNDANCE, c * mine, mine, abundance.as_mut_ptr().add(c * npix + at) as *mut c_void) != THZ_OK { return None; }
                }
                if thz_session_download(s, THZ_BUF_UNMIX_RESID, 0, mine, resid.as_mut_ptr().add(at) as *mut c_void) != THZ_OK
                    || thz_session_download(s, THZ_BUF_UNMIX_KKT, 0, mine, kkt.as_mut_ptr().add(at) as *mut c_void) != THZ_OK {
                    return None;
                }
                at += mine;
            }
            Some((abundance, resid, kkt, gx, gy))
        }
    }

    /// the 3-D tab's instances (`update_intensity_image`, `data_thread.rs:48-101`; `gui/threed_plot.rs:132-276`) over
    /// the WHOLE grid of the group (`thz_group_session_voxels`: threshold from the whole cube, every slab's instances in
    /// x, y, z order, gathered on rank 0) — what one GPU gives for the same cube.  `InstanceData` and
    /// `ThzVoxelInstance` share their layout.
    pub fn voxels(&self, cfg: &ThzVoxelCfg, max_instances: u64, scaling: usize, orig: (usize, usize, usize))
                  -> Option<(Vec<ThzVoxelInstance>, f32, [f32; 3])> {
        if self.session.is_null() { return None; }
        unsafe {
            let (mut n, mut thr, mut dims) = (0u64, 0f32, [0f32; 3]);
            if thz_group_session_voxels(self.session, cfg, max_instances, scaling as c_int, orig.0, orig.1, orig.2, ptr::null_mut(), 0, &mut n, &mut thr, dims.as_mut_ptr()) != THZ_OK {
                return None;
            }
            let mut out: Vec<ThzVoxelInstance> = Vec::with_capacity(n as usize);
            let cap = n;
            if thz_group_session_voxels(self.session, cfg, max_instances, scaling as c_int, orig.0, orig.1, orig.2, out.as_mut_ptr(), cap, &mut n, &mut thr, dims.as_mut_ptr()) != THZ_OK {
                return None;
            }
            out.set_len(n.min(cap) as usize);
            Some((out, thr, dims))
        }
    }
}

impl Drop for GpuEngine {
    fn drop(&mut self) {
        unsafe {
            if !self.session.is_null() { thz_group_session_destroy(self.session); }
            if !self.group.is_null() { thz_group_destroy(self.group); }
        }
    }
}
