"""The owner type of every persistent device buffer (csrc/dev_buf.hpp) on the host: tests/emu/dev_buf_driver.cpp
walks each of its transitions under AddressSanitizer + UBSan against HIP calls of its own over malloc / free, and
counts live blocks and synchronisations.  Built against that header alone: no HIP runtime, no GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs clang with the sanitizer runtimes")
def test_dev_buf_transitions_under_sanitizers(tmp_path):
    csrc = os.path.join(HERE, "..", "thz_image_explorer_amd", "csrc")
    exe = str(tmp_path / "dev_buf")
    b = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc,
                        os.path.join(HERE, "emu", "dev_buf_driver.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "unsupported option" in b.stdout:
        pytest.skip("sanitizer runtime not available")
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "dev_buf done" in r.stdout, r.stdout[-4000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-4000:]
