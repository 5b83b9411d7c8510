//! "Tilt Compensation" on the engine — REPLACES ONLY the body of `filter()` in `src/filters/tilt_compensation.rs`
//! (`:97-226`).  The struct, `new`, `reset`, `show_data`, `config`, `ui` and the unit tests of that file stay
//! VERBATIM.  Transliteration of `GpuTiltCompensation::filter` (`thz_image_explorer_amd/host/thz_engine.cpp`, tested by
//! `tests/test_gpu_engine.py`); UNVERIFIED BY A COMPILER.
//!
//! ... and ADDS an "Estimate" action to `ui()` (`:237-271`), in front of `final_response`'s return: the two angles
//! the reference has typed in by hand until the image looks flat, fitted instead to when the pulse arrives at each
//! pixel of the raw cube (`GpuTiltCompensation::estimate`, same file).
//!
//! Add to the file's imports:
//!     use crate::gpu::engine::ENGINE;
//!     use crate::gpu::ffi::{thz_host_frequency_axis, thz_host_tilt_plan, THZ_BUF_RAW};
//!     use crate::math_tools_gpu::shallow_clone;

    fn filter(&mut self, input_data: &ScannedImageFilterData, gui_settings: &mut GuiSettingsContainer,
              progress_lock: &mut Arc<RwLock<Option<f32>>>, abort_flag: &Arc<AtomicBool>) -> ScannedImageFilterData {
        let mut eng = ENGINE.lock().unwrap();
        if !eng.available() { drop(eng); return self.filter_cpu(input_data, gui_settings, progress_lock, abort_flag); } // the reference's body, kept as `filter_cpu`
        let (dx, dy) = match (input_data.dx, input_data.dy) { (Some(dx), Some(dy)) => (dx, dy), _ => return input_data.clone() }; // :111
        eng.record_tilt(true, self.tilt_x, self.tilt_y);
        let mut output = shallow_clone(input_data);
        // the extended axis (:104-170, 206-217): the containers behind this stage carry it; the device lays the cube
        // out on it with the same plan (thz_host_tilt_plan: extension, per-pixel insert index)
        let t = input_data.time.as_slice().unwrap();
        let steps = unsafe { thz_host_tilt_plan(t.as_ptr(), t.len(), input_data.width, input_data.height, self.tilt_x, self.tilt_y, dx, dy,
                                                std::ptr::null_mut(), std::ptr::null_mut()) };
        if steps > 0 {
            let mut new_time = vec![0f32; t.len() + 2 * steps];
            unsafe { thz_host_tilt_plan(t.as_ptr(), t.len(), input_data.width, input_data.height, self.tilt_x, self.tilt_y, dx, dy,
                                        new_time.as_mut_ptr(), std::ptr::null_mut()); }
            let mut freq = vec![0f32; new_time.len() / 2 + 1];
            unsafe { thz_host_frequency_axis(new_time.as_ptr(), new_time.len(), freq.as_mut_ptr()); }
            output.time = Array1::from(new_time);
            output.frequency = Array1::from(freq);
            // (the data thread re-plans r2c / c2r for the new length itself, data_thread.rs:1194-1227)
        }
        output
    }

    // ---- in `ui()`, behind the two sliders (`:261-268`) and in front of `final_response` (`:270`):
        // the pulse's main peak is its maximum (mode 1); pixels below a quarter of the strongest peak take no part
        let estimate = ui.button("Estimate").on_hover_text("Fit both angles to the pulse's arrival time over the raw scan");
        if estimate.clicked() {
            let fit = ENGINE.lock().unwrap().estimate_tilt(THZ_BUF_RAW, 1, 0.25);
            if let Some(fit) = fit {
                self.tilt_x = fit.tilt_x_deg.clamp(-15.0, 15.0); // the sliders' range
                self.tilt_y = fit.tilt_y_deg.clamp(-15.0, 15.0);
                // a changed response is how a filter's panel requests ConfigCommand::UpdateFilter(uuid) (filter.rs:650-658)
                final_response.mark_changed();
            }
        }
        final_response |= estimate;
