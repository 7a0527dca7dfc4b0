"""Rx reassembly, the host side (no device needed): the new C-ABI symbols, the
struct layouts, the workspace function, every argument error — which the
library reports before any device work — the Python wrappers' validation, the
C++ header, and the Python restatement of the reference's merger
(tests/reasm_model.py) against the results recorded from the reference's own
packet_merger (tests/golden/reasm.json)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import reasm_model
from seastar_amd import batch, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = native.SCCSUM_EINVAL
REASM_SYMBOLS = ["sccsum_ipv4_frag_records", "sccsum_ipv4_reasm_workspace", "sccsum_ipv4_reasm",
                 "sccsum_reasm_key_mix", "sccsum_reasm_sort_tile_records", "sccsum_reasm_scan_tile_records"]


def test_symbols_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    declared = native.header_symbols()
    lib = native.load()
    for s in REASM_SYMBOLS:
        assert s in declared and s in exported and s in native._PROTOS, s
        assert getattr(lib, s).argtypes is not None
    assert lib.sccsum_abi_version() == native.ABI_VERSION == 4
    for tile in (lib.sccsum_reasm_sort_tile_records(), lib.sccsum_reasm_scan_tile_records()):
        assert tile >= 64 and tile % 64 == 0


def test_struct_layouts_match_the_header(tmp_path):
    structs = (("sccsum_frag_rec", native.FragRec), ("sccsum_reasm_out", native.ReasmOut))
    body = []
    for cname, cls in structs:
        body.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        body += [f'    printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    consts = ("REASM_COMPLETE", "REASM_PENDING", "REASM_HOST")
    body += [f'    printf("{c} %d\\n", SCCSUM_{c});' for c in consts]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <sccsum.h>\nint main(void) {\n"
                   + "\n".join(body) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", exe],
                   check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    for cname, cls in structs:
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    for c in consts:
        assert int(got[c]) == getattr(native, c), c
    # the numpy view of a record is the same 32 bytes
    assert batch.REC_DTYPE.itemsize == ctypes.sizeof(native.FragRec) == 32
    for f, _ in native.FragRec._fields_:
        assert batch.REC_DTYPE.fields[f][1] == getattr(native.FragRec, f).offset, f


def test_workspace_is_sane():
    lib = native.load()
    ws = lib.sccsum_ipv4_reasm_workspace
    sizes = [ws(m) for m in (0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 10**6, 2**31 - 1)]
    assert sizes[0] >= 16
    assert all(s % 16 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert 32 * 10**6 <= ws(10**6) <= 96 * 10**6   # a few words per record and little else
    assert ws(2**40) == ws(2**31 - 1)              # past the most records a call takes


def _fmix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def key_mix(src, dst, ident, proto):
    """sccsum_reasm_key_mix restated: three rounds of the murmur3 finaliser."""
    h = _fmix((src + 0x9E3779B9) & 0xFFFFFFFF)
    h = _fmix(h ^ dst)
    return _fmix((h + ((ident << 8) | proto) * 0x9E3779B1) & 0xFFFFFFFF)


def test_key_mix_is_the_documented_function():
    lib = native.load()
    rng = np.random.Generator(np.random.PCG64(3))
    keys = [(0, 0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFF, 0xFF), (0x0A000001, 0x0A000002, 1, 17)]
    keys += [(int(a), int(b), int(c), int(d)) for a, b, c, d in
             zip(rng.integers(0, 2**32, 500), rng.integers(0, 2**32, 500), rng.integers(0, 65536, 500),
                 rng.integers(0, 256, 500))]
    for k in keys:
        assert lib.sccsum_reasm_key_mix(*k) == key_mix(*k), k
    # one address pair: (id, proto) -> mix is a bijection, so a flow's datagrams never collide with each other
    mixes = {key_mix(0x0A000001, 0x0A000002, i, p) for i in range(4096) for p in (6, 17)}
    assert len(mixes) == 2 * 4096


P = 0x10000
REC_ARGS = ("d_bytes", "bytes_len", "d_off", "d_len", "d_status", "need", "reject", "n", "host_address", "tag",
            "d_rec", "d_count", "d_workspace", "stream")


def _records(lib, **over):
    a = dict(d_bytes=P, bytes_len=4096, d_off=P, d_len=P, d_status=P, need=0x11, reject=0x0C, n=8, host_address=0,
             tag=0, d_rec=P, d_count=P, d_workspace=P, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return lib.sccsum_ipv4_frag_records(*[a[k] for k in REC_ARGS])


def test_frag_records_argument_errors_without_device():
    """Every argument error is SCCSUM_EINVAL before any device work (the
    pointers are made up: a call that got past its checks would fault)."""
    lib = native.load()
    for name in ("d_bytes", "d_off", "d_len", "d_status", "d_rec", "d_count", "d_workspace"):
        assert _records(lib, **{name: None}) == EINVAL, name
    for name, step in (("d_off", 4), ("d_len", 2), ("d_rec", 4), ("d_count", 2), ("d_workspace", 8)):
        assert _records(lib, **{name: P + step}) == EINVAL, name
    assert _records(lib, n=1 << 31) == EINVAL
    assert _records(lib, need=0x100) == EINVAL
    assert _records(lib, reject=0x80000000) == EINVAL
    # n == 0 still needs the count it writes, and its scratch
    for name in ("d_count", "d_workspace"):
        assert _records(lib, n=0, **{name: None}) == EINVAL, name
    assert _records(lib, n=0, d_count=P + 2) == EINVAL


OUT_FIELDS = [f for f, _ in native.ReasmOut._fields_]


def _reasm(lib, m=8, max_out_bytes=1 << 20, key=None, key_len=0, d_rec=P, d_workspace=P, no_out=False, **fields):
    f = {name: P for name in OUT_FIELDS}
    f["d_dgram_hash"] = None
    assert set(fields) <= set(f), fields
    f.update(fields)
    out = native.ReasmOut(*[f[name] for name in OUT_FIELDS])
    kb = None if key is None else (ctypes.c_uint8 * len(key)).from_buffer_copy(key)
    return lib.sccsum_ipv4_reasm(d_rec, m, max_out_bytes, None if kb is None else ctypes.addressof(kb), key_len,
                                 None if no_out else ctypes.addressof(out), d_workspace, None)


def test_reasm_argument_errors_without_device():
    lib = native.load()
    assert _reasm(lib, no_out=True) == EINVAL
    assert _reasm(lib, d_rec=None) == EINVAL
    assert _reasm(lib, d_workspace=None) == EINVAL
    for name in OUT_FIELDS:
        if name != "d_dgram_hash":
            assert _reasm(lib, **{name: None}) == EINVAL, name
    for name, step in (("d_desc", 4), ("d_dgram_first", 2), ("d_dgram_off", 4), ("d_dgram_len", 2), ("d_dgram_seed", 2),
                       ("d_dgram_head", 2), ("d_dgram_last", 2), ("d_pending", 4), ("d_host", 4), ("d_total", 4)):
        assert _reasm(lib, **{name: P + step}) == EINVAL, name
    assert _reasm(lib, d_rec=P + 4) == EINVAL
    assert _reasm(lib, d_workspace=P + 8) == EINVAL
    assert _reasm(lib, m=1 << 31) == EINVAL
    assert _reasm(lib, max_out_bytes=1 << 32) == EINVAL
    key = bytes(range(40))
    assert _reasm(lib, key=key, key_len=40) == EINVAL                          # a key without the hash array
    assert _reasm(lib, d_dgram_hash=P) == EINVAL                               # the hash array without a key
    assert _reasm(lib, key=key, key_len=3, d_dgram_hash=P) == EINVAL
    assert _reasm(lib, key=key, key_len=40, d_dgram_hash=P + 2) == EINVAL
    assert _reasm(lib, key_len=40) == EINVAL                                   # a length without a key
    # m == 0 may pass NULL arrays, but not the two it writes
    nulls = {name: None for name in OUT_FIELDS if name not in ("d_total", "d_dgram_first")}
    for name in ("d_total", "d_dgram_first"):
        assert _reasm(lib, m=0, d_rec=None, d_workspace=None, **dict(nulls, **{name: None})) == EINVAL, name
    assert _reasm(lib, m=0, d_rec=None, d_workspace=None, **dict(nulls, d_total=P + 4)) == EINVAL
    assert _reasm(lib, m=0, max_out_bytes=1 << 32, d_rec=None, d_workspace=None, **nulls) == EINVAL


def test_python_wrapper_validation():
    """batch.frag_records / batch.reassemble refuse wrong dtypes, devices,
    strides, sizes and caps before any launch."""
    n = 10
    b = batch.PacketBatch(data=torch.zeros(1024, dtype=torch.uint8), off=torch.arange(n, dtype=torch.int64) * 100,
                          length=torch.full((n,), 100, dtype=torch.int32), bytes_len=1000, max_len=100)
    ok = dict(status=torch.zeros(n, dtype=torch.uint8), need=batch.FRAG_NEED, reject=batch.FRAG_REJECT,
              host_address=0x0A000001, tag=7)
    assert batch.frag_records_check(b, **ok) == n
    assert (batch.FRAG_NEED, batch.FRAG_REJECT) == (0x11, 0x0C)
    bad = [("status", None), ("status", torch.zeros(n, dtype=torch.int8)), ("status", torch.zeros(n - 1, dtype=torch.uint8)),
           ("status", torch.zeros(2 * n, dtype=torch.uint8)[::2]), ("status", torch.zeros(n, 1, dtype=torch.uint8)),
           ("status", np.zeros(n, np.uint8)), ("status", torch.zeros(n, dtype=torch.uint8, device="meta")),
           ("need", -1), ("need", 0x100), ("reject", 0x100), ("host_address", -1), ("host_address", 1 << 32),
           ("tag", 1 << 32)]
    for name, value in bad:
        with pytest.raises(ValueError, match=name):
            batch.frag_records_check(b, **dict(ok, **{name: value}))
        with pytest.raises(ValueError):
            batch.frag_records(b, **dict(ok, **{name: value}))
    with pytest.raises(ValueError, match="b:"):
        batch.frag_records_check(None, **ok)
    for recs in (None, np.zeros(64, np.uint8), torch.zeros(64, dtype=torch.int8), torch.zeros(33, dtype=torch.uint8),
                 torch.zeros(2, 32, dtype=torch.uint8), torch.zeros(128, dtype=torch.uint8)[::2],
                 torch.zeros(64, dtype=torch.uint8)):          # the last: not on a device
        with pytest.raises(ValueError, match="records"):
            batch.reasm_check(recs, None, 0xFFFFFFFF)
        with pytest.raises(ValueError):
            batch.reassemble(recs)
    meta = torch.zeros(64, dtype=torch.uint8, device="meta")
    with pytest.raises(ValueError, match="records"):
        batch.reasm_check(meta, None, 0xFFFFFFFF)


def test_cpp_rx_reassembler_host_side(tmp_path):
    """seastar::net::rx_reassembler compiles warning-free, its host arithmetic
    is the library's, and a bad argument throws."""
    src = tmp_path / "reasm_host.cc"
    src.write_text(r'''
#include <seastar/net/ip_checksum_batch.hh>
#include <cstdio>
int main() {
    using seastar::net::rx_reassembler;
    rx_reassembler rx(0x0A000001u);
    if (rx.host_address() != 0x0A000001u) return 1;
    if (rx_reassembler::workspace(4096) != sccsum_ipv4_reasm_workspace(4096)) return 2;
    if (rx_reassembler::key_mix(1, 2, 3, 17) != sccsum_reasm_key_mix(1, 2, 3, 17)) return 3;
    sccsum_reasm_out out{};
    try {
        rx.run(nullptr, 0, 0, nullptr, 0, out, nullptr, nullptr);   // no d_total: refused before any device work
        return 4;
    } catch (const std::runtime_error&) {
    }
    try {
        rx.records({}, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
        return 5;
    } catch (const std::runtime_error&) {
    }
    std::printf("reasm_host: OK\n");
    return 0;
}
''')
    exe = str(tmp_path / "reasm_host")
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"), str(src), "-o", exe,
           "-L", lib_dir, "-lsccsum", "-Wl,-rpath," + lib_dir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not r.stderr.strip(), r.stderr  # warning-free
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "reasm_host: OK" in r.stdout


# ---------------------------------------------------------------- the model against the recorded reference

def _golden():
    with open(os.path.join(REPO, "tests", "golden", "reasm.json")) as f:
        return json.load(f)


def test_model_matches_the_recorded_reference_merger():
    doc = _golden()
    cases = doc["cases"]
    assert len(cases) >= 300
    assert {c["kind"] for c in cases} >= {"plain", "plain_hole", "overlap", "duplicate", "nested", "zero", "late"}
    for c in cases:
        seq = [tuple(x) for x in c["seq"]]
        assert reasm_model.trace_summary(reasm_model.merge_trace(seq)) == c["steps"], (c["kind"], seq)


def test_golden_sequences_are_the_generators():
    """reasm.json's inputs are what its generator makes today (the recorded
    results are the reference's; only the inputs can be rebuilt here)."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import make_reasm
    seqs = reasm_model.seeded_sequences(make_reasm.SEED, make_reasm.COUNT)
    assert [(k, [list(x) for x in s]) for k, s in seqs] == [(c["kind"], c["seq"]) for c in _golden()["cases"]]


def test_model_delivery_and_buckets_agree_on_plain_keys():
    """ip.cc:164-220 restated (reasm_model.run) delivers exactly the keys the
    interface calls complete, whenever the key is plain, for the golden inputs
    taken as one key each; non-plain ones are host."""
    seen = set()
    for c in _golden()["cases"]:
        seq = c["seq"]
        r = np.zeros(len(seq), dtype=batch.REC_DTYPE)
        for i, (o, ln, mf) in enumerate(seq):
            r[i] = (0, 1, 2, 3, 17, mf, o, 20, ln, 0, 0)
        st = reasm_model.buckets(r)
        assert len(set(st.tolist())) == 1
        seen.add(int(st[0]))
        out, held = reasm_model.run(r)
        if st[0] == native.REASM_COMPLETE:
            assert len(out) == 1 and not held and out[0].last == len(seq) - 1
            assert [p[0] for p in out[0].pieces] == sorted(range(len(seq)), key=lambda i: seq[i][0])
            assert out[0].length == max(o + ln for o, ln, _ in seq)
        elif st[0] == native.REASM_PENDING:
            assert not out and len(held) == 1
        assert c["kind"] not in ("plain", "plain_hole") or st[0] != native.REASM_HOST
    assert seen == {native.REASM_COMPLETE, native.REASM_PENDING, native.REASM_HOST}
