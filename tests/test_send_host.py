"""Tx send, the host side (no device needed): the new C-ABI symbols, the host
arithmetic (sccsum_ipv4_send_plan) against synth.ipv4_fragment, and every
argument error, which the library reports before any device work.

The expectation of a whole batch (expected_send) is built here from
synth.ipv4_fragment per datagram — the project's Python restatement of
ipv4::send (src/net/ip.cc:244-299 of the reference tree) — with the header
checksums from oracle.ip_checksum over each 20-byte header, never from the
code under test; tests/test_gpu_send.py compares the device's outputs with it."""
import ctypes
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle
from seastar_amd import batch, native, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = native.SCCSUM_EINVAL
TSO, UFO, NO_IP_CSUM, SEND_L4 = native.SEND_TSO, native.SEND_UFO, native.SEND_NO_IP_CSUM, native.SEND_L4

L4_LENS = (0, 1, 7, 8, 47, 48, 49, 548, 556, 557, 1479, 1480, 1481, 2960, 2961, 8980, 8981, 65514, 65515)
MTUS = (68, 576, 1500, 9000, 65535)
PROTOS = (6, 17, 1)
FLAG_SETS = (0, TSO, UFO, TSO | UFO)


# ---------------------------------------------------------------- the restatement

def effective_mtu(mtu: int, proto: int, flags: int) -> int:
    """needs_frag (ip.cc:100-111): with tx_tso a TCP datagram, with tx_ufo a UDP
    datagram is never cut — the same as an MTU every datagram fits."""
    exempt = (proto == 6 and flags & TSO) or (proto == 17 and flags & UFO)
    return 65535 if exempt else mtu


@functools.lru_cache(maxsize=None)
def ref_frame_lens(l4_len: int, mtu: int) -> tuple:
    """Frame lengths synth.ipv4_fragment makes of a datagram of l4_len bytes."""
    return tuple(int(f.size) for f in synth.ipv4_fragment(np.zeros(l4_len, np.uint8), 17, 1, 2, mtu=mtu))


def ref_plan(l4_len: int, mtu: int, proto: int, flags: int) -> tuple:
    lens = ref_frame_lens(l4_len, effective_mtu(mtu, proto, flags))
    return len(lens), sum(lens)


def expected_send(buf, off, length, dst, proto, mtu, src_host, ids=None, flags=0, max_frames=0x7FFFFFFF,
                  max_out_bytes=0xFFFFFFFF):
    """What sccsum_ipv4_send must write for the datagrams buf[off[i] .. + length[i])
    (after any SEND_L4 store): a dict of
      frames       the wire frames of the emitted datagrams, in order
      owner        (datagram, offset of the piece in it) per frame
      status       uint8 [n]
      dgram_first  uint32 [n + 1]
      total        (frames needed, bytes needed, datagrams emitted)
    and, from them, packed / out_off / out_len / first / hdr."""
    n = int(off.size)
    per, status = [], np.zeros(n, np.uint8)
    for i in range(n):
        o, ln = int(off[i]), int(length[i])
        bad = 0
        if o > buf.size or ln > buf.size - o:
            bad |= native.ST_RANGE
        if ln > native.SEND_L4_MAX:
            bad |= native.ST_MALFORMED
        status[i] = bad or native.ST_OK
        if bad:
            per.append([])
            continue
        fr = synth.ipv4_fragment(buf[o:o + ln], int(proto[i]), int(src_host), int(dst[i]),
                                 mtu=effective_mtu(mtu, int(proto[i]), flags), ident=0 if ids is None else int(ids[i]))
        if not flags & NO_IP_CSUM:
            for f in fr:
                f[10:12] = np.frombuffer(np.uint16(oracle.ip_checksum(f[:20])).tobytes(), np.uint8)
        per.append(fr)
    need_frames = sum(len(fr) for fr in per)
    need_bytes = sum(int(f.size) for fr in per for f in fr)
    # the prefix rule: datagram i is emitted only if datagrams 0..i fit both caps
    prefix, cf, cb = n, 0, 0
    for i, fr in enumerate(per):
        cf += len(fr)
        cb += sum(int(f.size) for f in fr)
        if cf > max_frames or cb > max_out_bytes:
            prefix = i
            break
    status[prefix:] = 0
    frames, owner, dgram_first = [], [], np.zeros(n + 1, np.uint32)
    for i in range(n):
        dgram_first[i] = len(frames)
        if i < prefix:
            at = 0
            for f in per[i]:
                owner.append((i, at))
                at += int(f.size) - 20
                frames.append(f)
    dgram_first[n] = len(frames)
    out_len = np.array([f.size for f in frames], np.uint32)
    out_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(out_len, dtype=np.uint64)])[: len(frames)]
    return dict(frames=frames, owner=owner, status=status, dgram_first=dgram_first,
                total=(need_frames, need_bytes, prefix), out_len=out_len, out_off=out_off,
                first=(2 * np.arange(len(frames) + 1)).astype(np.uint32),
                packed=np.concatenate(frames) if frames else np.zeros(0, np.uint8),
                hdr=np.concatenate([f[:20] for f in frames]) if frames else np.zeros(0, np.uint8))


def _opts(mtu=1500, flags=0, src=0x0A000001):
    return native.SendOpts(src, mtu, flags)


def _plan(lib, opts, l4_len, proto):
    nf, nb = ctypes.c_uint32(0xEEEEEEEE), ctypes.c_uint64(0xEEEEEEEE)
    rc = lib.sccsum_ipv4_send_plan(ctypes.addressof(opts), l4_len, proto, ctypes.byref(nf), ctypes.byref(nb))
    return rc, nf.value, nb.value


# ---------------------------------------------------------------- tests

SEND_SYMBOLS = ["sccsum_ipv4_send_plan", "sccsum_ipv4_send_workspace", "sccsum_ipv4_send",
                "sccsum_send_tile_datagrams", "sccsum_send_emit_tile_frames"]


def test_symbols_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    declared = native.header_symbols()
    lib = native.load()
    for s in SEND_SYMBOLS:
        assert s in declared and s in exported and s in native._PROTOS, s
        assert getattr(lib, s).argtypes is not None
    assert lib.sccsum_abi_version() == native.ABI_VERSION == 4
    assert lib.sccsum_send_tile_datagrams() >= 64 and lib.sccsum_send_tile_datagrams() % 64 == 0
    assert lib.sccsum_send_emit_tile_frames() >= 64 and lib.sccsum_send_emit_tile_frames() % 64 == 0


def test_send_opts_layout_and_flags_match_the_header(tmp_path):
    fields = [name for name, _ in native.SendOpts._fields_]
    body = "\n".join(f'    printf("{f} %zu\\n", offsetof(sccsum_send_opts, {f}));' for f in fields)
    flags = "\n".join(f'    printf("{f} %u\\n", SCCSUM_{f});' for f in ("SEND_TSO", "SEND_UFO", "SEND_NO_IP_CSUM",
                                                                         "SEND_L4"))
    src = tmp_path / "opts.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <sccsum.h>\n"
                   "int main(void) {\n    printf(\"size %zu\\n\", sizeof(sccsum_send_opts));\n"
                   f"{body}\n{flags}\n    return 0;\n}}\n")
    exe = str(tmp_path / "opts")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", exe],
                   check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(native.SendOpts)
    for f in fields:
        assert int(got[f]) == getattr(native.SendOpts, f).offset, f
    for f in ("SEND_TSO", "SEND_UFO", "SEND_NO_IP_CSUM", "SEND_L4"):
        assert int(got[f]) == getattr(native, f), f


def test_plan_matches_ipv4_fragment():
    lib = native.load()
    cases = 0
    for mtu, flags in itertools.product(MTUS, FLAG_SETS):
        opts = _opts(mtu, flags)
        for l4_len, proto in itertools.product(L4_LENS, PROTOS):
            want = ref_plan(l4_len, mtu, proto, flags)
            assert _plan(lib, opts, l4_len, proto) == (0, *want), (l4_len, mtu, proto, flags)
            cases += 1
    assert cases == len(L4_LENS) * len(MTUS) * len(PROTOS) * len(FLAG_SETS)
    # the other flags change no count
    assert _plan(lib, _opts(1500, NO_IP_CSUM | SEND_L4), 2961, 17) == (0, *ref_plan(2961, 1500, 17, 0))


def test_plan_refusals():
    lib = native.load()
    for l4_len in (65516, 2**32 - 1):
        for mtu in MTUS:
            assert _plan(lib, _opts(mtu, TSO | UFO), l4_len, 6) == (0, 0, 0), (l4_len, mtu)
    for mtu in (67, 65536, 0, 2**32 - 1):
        rc, nf, nb = _plan(lib, _opts(mtu), 100, 17)
        assert (rc, nf, nb) == (EINVAL, 0, 0), mtu
    assert _plan(lib, _opts(1500, 0x10), 100, 17) == (EINVAL, 0, 0)  # an unknown flag
    nf, nb = ctypes.c_uint32(7), ctypes.c_uint64(7)
    o = _opts()
    assert lib.sccsum_ipv4_send_plan(None, 100, 17, ctypes.byref(nf), ctypes.byref(nb)) == EINVAL
    assert (nf.value, nb.value) == (0, 0)
    assert lib.sccsum_ipv4_send_plan(ctypes.addressof(o), 100, 17, None, ctypes.byref(nb)) == EINVAL
    assert lib.sccsum_ipv4_send_plan(ctypes.addressof(o), 100, 17, ctypes.byref(nf), None) == EINVAL


def test_workspace_is_sane():
    lib = native.load()
    ws = lib.sccsum_ipv4_send_workspace
    sizes = [ws(n) for n in (0, 1, 2, 1023, 1024, 1025, 4096, 10**6, 2**32 - 1)]
    assert sizes[0] >= 16
    assert all(s % 16 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert 8 * 10**6 <= ws(10**6) <= 9 * 10**6        # one 64-bit word per datagram and little else
    assert ws(2**32 - 1) < 2**36


# the argument list of sccsum_ipv4_send after opts, as a dict of valid-looking values: integers stand in
# for device pointers (every call below must be refused before anything is dereferenced)
P = 0x10000
ARGS = ("d_l4", "l4_bytes_len", "d_off", "d_len", "d_dst", "d_proto", "d_id", "d_l4sum", "n", "max_frames",
        "max_out_bytes", "d_hdr", "d_desc", "d_first", "d_out_off", "d_out_len", "d_dgram_first", "d_status",
        "d_total", "d_workspace", "stream")


def _send(lib, opts, **over):
    a = dict(d_l4=P, l4_bytes_len=4096, d_off=P, d_len=P, d_dst=P, d_proto=P, d_id=P, d_l4sum=None, n=8,
             max_frames=64, max_out_bytes=1 << 20, d_hdr=P, d_desc=P, d_first=P, d_out_off=P, d_out_len=P,
             d_dgram_first=P, d_status=P, d_total=P, d_workspace=P, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.sccsum_ipv4_send(None if opts is None else ctypes.addressof(opts), *[a[k] for k in ARGS])


def test_send_argument_errors_without_device():
    """Every argument error is SCCSUM_EINVAL before any device work (this
    machine has no device: a call that got past its checks would fail otherwise,
    and on a machine with one it would fault on the made-up pointers)."""
    lib = native.load()
    ok = _opts()
    assert _send(lib, None) == EINVAL
    for mtu in (0, 67, 65536):
        assert _send(lib, _opts(mtu)) == EINVAL, mtu
    assert _send(lib, _opts(1500, 0x10)) == EINVAL
    assert _send(lib, _opts(1500, 0x80000000)) == EINVAL
    for name in ("d_l4", "d_off", "d_len", "d_dst", "d_proto", "d_hdr", "d_desc", "d_first", "d_out_off",
                 "d_out_len", "d_dgram_first", "d_status", "d_total", "d_workspace"):
        assert _send(lib, ok, **{name: None}) == EINVAL, name
    for name, step in (("d_off", 4), ("d_len", 2), ("d_dst", 2), ("d_id", 1), ("d_desc", 4),
                       ("d_first", 2), ("d_out_off", 4), ("d_out_len", 2), ("d_dgram_first", 2), ("d_total", 4),
                       ("d_workspace", 8)):
        assert _send(lib, ok, **{name: P + step}) == EINVAL, name
    assert _send(lib, _opts(1500, SEND_L4), d_l4sum=P + 1) == EINVAL
    assert _send(lib, _opts(1500, SEND_L4), d_l4sum=None) == EINVAL   # the flag without the values
    assert _send(lib, ok, d_l4sum=P) == EINVAL                        # the values without the flag
    assert _send(lib, ok, max_frames=1 << 31) == EINVAL
    assert _send(lib, ok, max_out_bytes=1 << 32) == EINVAL
    assert _send(lib, ok, n=1 << 32) == EINVAL
    # n == 0 still needs the two arrays it writes, and its scratch
    for name in ("d_total", "d_dgram_first", "d_workspace"):
        assert _send(lib, ok, n=0, **{name: None}) == EINVAL, name
    assert _send(lib, ok, n=0, d_total=P + 4) == EINVAL
    assert _send(lib, _opts(67), n=0) == EINVAL


def test_python_wrapper_validation():
    """batch.ipv4_send's checks (batch.send_check) refuse wrong dtypes, devices,
    strides, sizes, flags and caps before any launch."""
    n = 10
    l4 = batch.PacketBatch(data=torch.zeros(1024, dtype=torch.uint8), off=torch.arange(n, dtype=torch.int64) * 100,
                           length=torch.full((n,), 100, dtype=torch.int32), bytes_len=1000, max_len=100)
    ok = dict(dst=torch.zeros(n, dtype=torch.int32), proto=torch.zeros(n, dtype=torch.uint8), mtu=1500,
              src_host=0x0A000001, ids=torch.zeros(n, dtype=torch.int16), l4sum=None, flags=0, max_frames=None,
              max_out_bytes=None)
    assert batch.send_check(l4, **ok) == (n, 2 * n + 1000 // 1480, 1000 + 20 * (2 * n + 1000 // 1480))
    assert batch.send_check(l4, **dict(ok, mtu=68)) == (n, 2 * n + 1000 // 48, 1000 + 20 * (2 * n + 1000 // 48))
    assert batch.send_check(l4, **dict(ok, ids=None, max_frames=5, max_out_bytes=7)) == (n, 5, 7)
    assert batch.send_check(l4, **dict(ok, flags=SEND_L4, l4sum=torch.zeros(n, dtype=torch.int16)))[0] == n
    bad = [("dst", torch.zeros(n, dtype=torch.int64)), ("dst", torch.zeros(n - 1, dtype=torch.int32)),
           ("dst", torch.zeros(2 * n, dtype=torch.int32)[::2]), ("dst", torch.zeros(n, 1, dtype=torch.int32)),
           ("dst", np.zeros(n, np.int32)), ("dst", None), ("proto", torch.zeros(n, dtype=torch.int8)),
           ("proto", torch.zeros(n - 1, dtype=torch.uint8)), ("proto", 17), ("ids", torch.zeros(n, dtype=torch.int32)),
           ("ids", torch.zeros(n - 1, dtype=torch.int16)), ("ids", torch.zeros(2 * n, dtype=torch.int16)[::2]),
           ("l4sum", torch.zeros(n, dtype=torch.int16)),  # without the flag
           ("mtu", 67), ("mtu", 65536), ("flags", 0x10), ("flags", SEND_L4),  # the flag without l4sum
           ("src_host", -1), ("src_host", 1 << 32), ("max_frames", -1), ("max_frames", 1 << 31),
           ("max_out_bytes", -1), ("max_out_bytes", 1 << 32)]
    for name, value in bad:
        with pytest.raises(ValueError, match="l4sum" if (name, value) == ("flags", SEND_L4) else name):
            batch.send_check(l4, **dict(ok, **{name: value}))
        with pytest.raises(ValueError):
            batch.ipv4_send(l4, **dict(ok, **{name: value}))
    with pytest.raises(ValueError, match="l4sum"):
        batch.send_check(l4, **dict(ok, flags=SEND_L4, l4sum=torch.zeros(n, dtype=torch.int32)))
    with pytest.raises(ValueError, match="l4"):
        batch.send_check(None, **ok)
    with pytest.raises(ValueError, match="dst"):
        batch.send_check(l4, **dict(ok, dst=torch.zeros(n, dtype=torch.int32, device="meta")))


def _cpp_cases(tmp_path):
    """The case file of tests/cpp/send_host.cc and the line it must print."""
    lines, nplan = [], 0
    for mtu, flags in itertools.product(MTUS, FLAG_SETS):
        for l4_len, proto in itertools.product(L4_LENS, PROTOS):
            f, b = ref_plan(l4_len, mtu, proto, flags)
            lines.append(f"P {mtu} {flags} {proto} {l4_len} {f} {b}")
            nplan += 1
    for l4_len in (65516, 2**32 - 1):
        lines.append(f"P 1500 0 17 {l4_len} 0 0")
        nplan += 1
    bad = ("67 0", "65536 0", "0 0", "1500 16", "1500 2147483648")
    lines += ["X " + b for b in bad]
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    return str(cases), f"send_host: OK ({nplan} plans, {len(bad)} refused)"


def test_cpp_tx_sender_host_arithmetic(tmp_path):
    """seastar::net::tx_sender::plan (tests/cpp/send_host.cc) against
    synth.ipv4_fragment's counts, passed in through a case file."""
    cases, want = _cpp_cases(tmp_path)
    exe = str(tmp_path / "send_host")
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "send_host.cc"), "-o", exe, "-L", lib_dir, "-lsccsum",
           "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # warning-free
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert want in r.stdout


def test_cpp_tx_sender_host_arithmetic_sanitized(tmp_path):
    """The same stand-alone program with send.hip itself compiled in, its host
    side under AddressSanitizer + UndefinedBehaviorSanitizer (device code is
    not instrumented), as tests/test_steer_host.py builds steer.hip."""
    cases, want = _cpp_cases(tmp_path)
    exe = str(tmp_path / "send_host_san")
    host_san = []
    for f in ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"):
        host_san += ["-Xarch_host", f]
    stub = tmp_path / "strerror.cc"  # the one symbol the C++ header needs from the rest of the library
    stub.write_text('extern "C" const char* sccsum_strerror(int) { return "error"; }\n')
    cmd = ["/opt/rocm/bin/hipcc", "-O1", "-g", "--offload-arch=gfx950", "-std=c++17", *host_san,
           "-I", os.path.join(REPO, "include"), os.path.join(REPO, "seastar_amd", "csrc", "send.hip"),
           os.path.join(REPO, "tests", "cpp", "send_host.cc"), str(stub), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300, env=env, cwd=tmp_path)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert want in r.stdout and "runtime error" not in r.stderr
