"""sccsum_ipv4_fill_desc / sccsum_burst_set_fill without a device: the entries
are exported and bound, refuse bad modes and bad arrays before any device
call, the C++ header names them, and the Python wrapper checks its arrays
before any launch."""
import os
import subprocess

import pytest
import torch

from seastar_amd import batch, burst, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = native.FILL_IP | native.FILL_L4


def test_symbols_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = native.load()
    for name in ("sccsum_ipv4_fill_desc", "sccsum_burst_set_fill"):
        assert name in exported
        assert name in native.header_symbols()
        assert name in native._PROTOS and getattr(lib, name).argtypes is not None
    assert len(native._PROTOS["sccsum_ipv4_fill_desc"][1]) == 11
    assert lib.sccsum_abi_version() == 4  # additive


def test_mode_is_checked_first_then_empty_batches_pass():
    lib = native.load()
    p = 0x10000
    bad_modes = (0, 0x20, native.FILL_L4 | native.FILL_L4_PSEUDO, native.FILL_TSO, native.FILL_TSO | native.FILL_L4,
                 native.FILL_ICMP_ECHO | native.FILL_L4_PSEUDO, 0x100 | native.FILL_IP)
    for m in bad_modes:
        assert lib.sccsum_ipv4_fill_desc(None, None, None, None, None, None, None, 0, 0, m, None) == native.SCCSUM_EINVAL
        assert lib.sccsum_ipv4_fill_desc(p, p, p, p, None, p, p, 4, 64, m, None) == native.SCCSUM_EINVAL
    for m in (native.FILL_IP, native.FILL_L4, GOOD, native.FILL_L4_PSEUDO, native.FILL_L4_PSEUDO | native.FILL_TSO,
              native.FILL_IP | native.FILL_L4_PSEUDO | native.FILL_TSO, native.FILL_ICMP_ECHO,
              GOOD | native.FILL_ICMP_ECHO):
        assert lib.sccsum_ipv4_fill_desc(None, None, None, None, None, None, None, 0, 0, m, None) == native.SCCSUM_OK


def test_null_and_misaligned_arrays_are_refused_before_any_device_call():
    lib = native.load()
    p = 0x10000

    def call(desc=p, first=p, off=p, length=p, stage=None, out2=p, status=None):
        return lib.sccsum_ipv4_fill_desc(desc, first, off, length, stage, out2, status, 4, 64, GOOD, None)

    assert call(first=None) == native.SCCSUM_EINVAL
    assert call(off=None) == native.SCCSUM_EINVAL
    assert call(length=None) == native.SCCSUM_EINVAL
    assert call(desc=p + 4) == native.SCCSUM_EINVAL
    assert call(first=p + 2) == native.SCCSUM_EINVAL
    assert call(off=p + 4) == native.SCCSUM_EINVAL
    assert call(length=p + 1) == native.SCCSUM_EINVAL
    assert call(out2=p + 2) == native.SCCSUM_EINVAL
    # a NULL descriptor array is accepted as by sccsum_ipv4_frames_desc; the other arrays are still checked
    assert call(desc=None, first=None) == native.SCCSUM_EINVAL
    assert call(desc=None, out2=None, off=p + 4) == native.SCCSUM_EINVAL


def test_burst_set_fill_refuses_a_null_queue():
    lib = native.load()
    assert lib.sccsum_burst_set_fill(None, GOOD) == native.SCCSUM_EINVAL
    assert lib.sccsum_burst_set_fill(None, 0) == native.SCCSUM_EINVAL
    assert callable(burst.BurstQueue.set_fill)


def test_batch_header_names_the_new_members(tmp_path):
    src = tmp_path / "f.cc"
    src.write_text(
        '#include <seastar/net/ip_checksum_batch.hh>\n'
        'void fill(const seastar::net::batch_checksummer& e, const sccsum_gather_desc* d, const uint32_t* first,\n'
        '          const uint64_t* off, const uint32_t* len, uint64_t n, void* stage, uint16_t* out2, uint8_t* st) {\n'
        '    e.ipv4_fill_desc(d, first, off, len, n, 1500, SCCSUM_FILL_IP | SCCSUM_FILL_L4, stage, out2, st, nullptr);\n'
        '}\n'
        'int main() {\n'
        '    auto done = [](uint64_t, uint32_t, const uint16_t*, const uint8_t*) {};\n'
        '    try {\n'
        '        seastar::net::burst_queue<decltype(done)> q(0, SCCSUM_PIPE_IPV4, 1 << 20, 128, 20000, 2, done);\n'
        '        if (!q.set_fill(SCCSUM_FILL_IP | SCCSUM_FILL_L4)) return 1;\n'
        '        q.drain();\n'
        '    } catch (const std::exception&) {\n'
        '    }\n'
        '    return 0;\n'
        '}\n')
    exe = str(tmp_path / "f")
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", exe,
           "-L", lib_dir, "-lsccsum", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _args(n=8):
    return dict(desc=torch.zeros(16 * n, dtype=torch.uint8), first=torch.arange(n + 1, dtype=torch.int32),
                off=torch.arange(n, dtype=torch.int64) * 64, length=torch.full((n,), 64, dtype=torch.int32),
                max_len=64, mode=GOOD)


@pytest.mark.parametrize("bad", ["first_count", "first_dtype", "desc_dtype", "off_dtype", "len_dtype", "len_count",
                                 "out2_short", "out2_dtype", "status_short", "stage_dtype", "out2_device"])
def test_wrapper_refuses_bad_arrays_before_any_launch(bad):
    kw = _args()
    if bad == "first_count":
        kw["first"] = kw["first"][:-1]
    elif bad == "first_dtype":
        kw["first"] = kw["first"].to(torch.int64)
    elif bad == "desc_dtype":
        kw["desc"] = kw["desc"].view(torch.int64)
    elif bad == "off_dtype":
        kw["off"] = kw["off"].to(torch.int32)
    elif bad == "len_dtype":
        kw["length"] = kw["length"].to(torch.int64)
    elif bad == "len_count":
        kw["length"] = kw["length"][:-1]
    elif bad == "out2_short":
        kw["out2"] = torch.empty(15, dtype=torch.int16)
    elif bad == "out2_dtype":
        kw["out2"] = torch.empty(16, dtype=torch.int32)
    elif bad == "status_short":
        kw["status"] = torch.empty(7, dtype=torch.uint8)
    elif bad == "stage_dtype":
        kw["stage"] = torch.empty(64, dtype=torch.int8)
    elif bad == "out2_device":
        kw["out2"] = torch.empty(16, dtype=torch.int16, device="meta")
    with pytest.raises(ValueError):
        batch.ipv4_fill_desc(**kw)


def test_wrapper_refuses_host_arrays():
    """Well-formed arrays that are not on a device never reach the library."""
    with pytest.raises(ValueError, match="device tensors"):
        batch.ipv4_fill_desc(**_args())
