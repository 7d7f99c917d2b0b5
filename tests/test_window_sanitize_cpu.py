"""The range math of a window load under AddressSanitizer + UndefinedBehaviorSanitizer,
without a GPU: tests/sanitize/window_sanitize.cpp, a stand-alone program, is built with
the product's pure-host sources, all instrumented, and run (as tests/test_region_cpu.py
runs region_sanitize.cpp).  It checks region_chunk_ranges pixel by pixel and
dec::blocks_of_range block by block; nothing is loaded into Python."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "acquire-zarr_amd", "csrc")


def test_window_range_math_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "window_sanitize")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-pthread"]
    srcs = [os.path.join(REPO, "tests", "sanitize", "window_sanitize.cpp")] + [
        os.path.join(CSRC, f) for f in ("aqz_geometry.cpp", "aqz_copy.cpp", "aqz_hostsplit.cpp",
                                        "aqz_region.cpp")]
    r = subprocess.run(["g++", "-std=c++20", *flags, "-I", CSRC, *srcs, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    # the (geometry, element size, region) cases of region_sanitize.cpp; 4000 headers
    # with 14 ranges each
    assert "clean: 424 hull cases, 4000 headers, 56000 ranges" in r.stdout
    assert "runtime error" not in r.stderr
