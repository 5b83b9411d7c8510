"""Race and bounds detection for the half-length chain with its extras (fft_ph.hpp: the complex multiplier read from
memory in the finish loop, the pixel sums in ticket-ordered accumulators behind the waves' buffers) on the CPU: the
emulation (every lane a host thread, tests/emu/) built with a sanitizer and driven by tests/emu/tsan_ph_driver.cpp — the
cmask + sums variant at 2002 samples (19 traces on one block) and at 4000 (10 traces).  A ThreadSanitizer report is a pair
of LDS / global accesses of two lanes that no barrier or ticket orders; under AddressSanitizer the emulation's LDS is a
heap block of exactly the launch's dynamic-LDS size, so a lane outside it, or outside the caller's arrays, is an error."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "thz_image_explorer_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
LAST_LINE = "ph driver finished rc=0"
REACHED = ("ph chain nt=2002 npix=19 rows=1", "ph chain nt=4000 npix=10 rows=2", LAST_LINE)


def _build_and_run(san, tmp_path):
    exe = str(tmp_path / "tsan_ph_driver")
    build = subprocess.run(
        [CLANG, "-std=c++17", "-O1", "-g", f"-fsanitize={san}", "-fno-sanitize=float-divide-by-zero", "-DTHZ_EMU", f"-I{EMU}",
         f"-I{CSRC}", "-x", "c++", os.path.join(CSRC, "kernels.hip"), os.path.join(CSRC, "voxel.hip"),
         os.path.join(EMU, "emu_harness.cpp"), os.path.join(EMU, "emu_ph_harness.cpp"),
         os.path.join(EMU, "tsan_ph_driver.cpp"), "-lpthread", "-lm", "-o", exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    if build.returncode != 0:
        return build, None
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 second_deadlock_stack=0 history_size=2 exitcode=0",
               ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    return build, run


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs clang with the sanitizer runtimes")
def test_ph_chain_is_race_free(tmp_path):
    build, run = _build_and_run("thread", tmp_path)
    if run is None:
        out = build.stdout
        if "unsupported option '-fsanitize=thread'" in out or "cannot find" in out and "tsan" in out:
            pytest.skip("ThreadSanitizer runtime not available")
        pytest.fail(out[-4000:])
    out = run.stdout
    assert run.returncode == 0, out[-4000:]
    for tag in REACHED:
        assert tag in out, f"driver did not reach: {tag}\n{out[-2000:]}"
    reports = [l for l in out.splitlines() if "WARNING: ThreadSanitizer" in l]
    assert not reports, out[-6000:]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs clang with the sanitizer runtimes")
@pytest.mark.skipif(os.environ.get("THZ_SANITIZE_ALL") != "1",
                    reason="four more minutes of build + run; set THZ_SANITIZE_ALL=1")
def test_ph_chain_stays_in_bounds(tmp_path):
    build, run = _build_and_run("address,undefined", tmp_path)
    if run is None:
        out = build.stdout
        if "unsupported option" in out or "cannot find" in out and "asan" in out:
            pytest.skip("sanitizer runtime not available")
        pytest.fail(out[-4000:])
    out = run.stdout
    assert run.returncode == 0, out[-4000:]
    for tag in REACHED:
        assert tag in out, f"driver did not reach: {tag}\n{out[-2000:]}"
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-6000:]
