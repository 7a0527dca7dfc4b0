"""The stand-alone C++ programs of tests/cpp/ that a layer's host test builds
and runs: once with g++ against the built library, once with hipcc with the
layer's .hip itself compiled in and its host side under AddressSanitizer +
UndefinedBehaviorSanitizer (device code is not instrumented).  Each program has
its own main and prints `token` when every check in it passed."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpp_cmd(program: str, exe: str, with_library: bool, extra=()) -> list:
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    link = ["-L", lib_dir, "-lsccsum", "-Wl,-rpath," + lib_dir] if with_library else []
    return ["-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), *extra,
            os.path.join(REPO, "tests", "cpp", program + ".cc"), "-o", exe, *link]


def build_and_run(tmp_path, program: str, token: str) -> None:
    exe = str(tmp_path / program)
    r = subprocess.run(["g++", "-O2", *_cpp_cmd(program, exe, True)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # warning-free
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert token in r.stdout


def build_and_run_sanitized(tmp_path, program: str, layer: str, token: str) -> None:
    """`layer` is the .hip in seastar_amd/csrc whose entry points the program calls."""
    exe = str(tmp_path / (program + "_san"))
    host_san = []
    for f in ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"):
        host_san += ["-Xarch_host", f]
    stub = tmp_path / "strerror.cc"  # the one symbol the C++ header needs from the rest of the library
    stub.write_text('extern "C" const char* sccsum_strerror(int) { return "error"; }\n')
    cmd = ["/opt/rocm/bin/hipcc", "-O1", "-g", "--offload-arch=gfx950", *host_san,
           *_cpp_cmd(program, exe, False, extra=[os.path.join(REPO, "seastar_amd", "csrc", layer), str(stub)])]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env, cwd=tmp_path)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert token in r.stdout and "runtime error" not in r.stderr
