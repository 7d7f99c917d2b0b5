"""The host side of pitched appends (aqz_stage_append_strided) under AddressSanitizer +
UndefinedBehaviorSanitizer, without a GPU: tests/sanitize/strided_sanitize.cpp, a
stand-alone program, is built with csrc/aqz_copy.cpp and csrc/aqz_strided.hh, all
instrumented, and run (as tests/test_window_sanitize_cpu.py runs window_sanitize.cpp).
CopyPool::copy_rows packs pitched frames out of canvases that end at the last byte of
the last row into destinations of exactly the packed size and must equal a naive loop;
strided::refusal must refuse every invalid argument of the entry point and accept its
neighbours; strided::plan_device_batch must give the route of every (alignment, XY, 2-D /
2x2x2, group-aligned or not) combination.  Nothing is loaded into Python."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "acquire-zarr_amd", "csrc")


def test_strided_host_logic_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "strided_sanitize")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-pthread"]
    srcs = [os.path.join(REPO, "tests", "sanitize", "strided_sanitize.cpp"),
            os.path.join(CSRC, "aqz_copy.cpp")]
    r = subprocess.run(["g++", "-std=c++20", *flags, "-I", CSRC, *srcs, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    # 2 pools x 4 element sizes x 3 pitches x 3 frame strides; the refusals of four
    # element sizes; 2 x 3 x 2 x 5 x 4 x 2 x 5 plans + 8 unit and route checks
    assert "clean: 72 copies, 70 refusal cases, 2408 plan cases" in r.stdout
    assert "runtime error" not in r.stderr
