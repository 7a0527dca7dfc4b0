"""The UDP layer, the host side (no device needed): the new C-ABI symbols, the
port table's lookup against a dict, argument errors (reported before any
device work), the C++ classes, the per-datagram model tests/udp_model.py
pinned by frames written out byte by byte, its array form pinned to it, the
offload-seed identity through the oracle, and a coverage check of the traffic
tests/test_gpu_udp.py runs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import cpp_host
import oracle
import stack_model as sm
import udp_model
import udp_traffic
from seastar_amd import batch, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = native.SCCSUM_EINVAL
SKIP, SHORT, NOPORT = native.UDP_SKIP, native.UDP_SHORT, native.UDP_NOPORT

UDP_SYMBOLS = ["sccsum_udp_ports_create", "sccsum_udp_ports_create_host", "sccsum_udp_ports_destroy",
               "sccsum_udp_ports_lookup", "sccsum_udp_ports_channels", "sccsum_udp_rx_workspace", "sccsum_udp_rx",
               "sccsum_udp_rx_reasm_workspace", "sccsum_udp_rx_reasm", "sccsum_udp_send"]


def test_symbols_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    declared = native.header_symbols()
    lib = native.load()
    for s in UDP_SYMBOLS:
        assert s in declared and s in exported and s in native._PROTOS, s
        assert getattr(lib, s).argtypes is not None
    assert lib.sccsum_abi_version() == native.ABI_VERSION == 4
    header = open(native.HEADER_PATH).read()
    for name, value in (("SCCSUM_UDP_SKIP", native.UDP_SKIP), ("SCCSUM_UDP_SHORT", native.UDP_SHORT),
                        ("SCCSUM_UDP_NOPORT", native.UDP_NOPORT)):
        assert f"0x{value:02X}u" in header.split(f"#define {name}")[1].split("\n")[0]
    assert (SKIP, SHORT, NOPORT) == (udp_model.SKIP, udp_model.SHORT, udp_model.NOPORT) == (0xFD, 0xFE, 0xFF)
    assert "#define SCCSUM_UDP_MAX_CHANNELS 252" in header and native.UDP_MAX_CHANNELS == 252
    assert native.UDP_PAYLOAD_MAX == udp_model.PAYLOAD_MAX == 65507
    assert native.UDP_QUEUE_SIZE == udp_model.QUEUE_SIZE == 1024
    assert os.path.join(REPO, "seastar_amd", "csrc", "udp.hip") in __import__("seastar_amd.build").build.SOURCES


def test_opts_layout_matches_the_header(tmp_path):
    lines = ['    printf("size %zu\\n", sizeof(sccsum_udp_opts));']
    lines += [f'    printf("{f} %zu\\n", offsetof(sccsum_udp_opts, {f}));' for f, _ in native.UdpOpts._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <sccsum.h>\nint main(void) {\n"
                   + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(native.UdpOpts)
    for f, _ in native.UdpOpts._fields_:
        assert int(got[f]) == getattr(native.UdpOpts, f).offset, f


@pytest.mark.parametrize("channels", [0, 1, 252])
def test_ports_lookup_against_a_dict(channels):
    rng = np.random.default_rng(channels)
    ports = rng.permutation(65536)[:channels].tolist()
    if channels == 252:
        ports[0], ports[1] = 0, 65535
        ports = list(dict.fromkeys(ports))
        channels = len(ports)
    want = {p: k for k, p in enumerate(ports)}
    t = batch.UdpPorts(ports, device=None)
    assert t.channels == channels and t.ports == tuple(ports)
    for port in range(65536):
        assert t.lookup(port) == want.get(port), port
    t.close()
    with pytest.raises(ValueError, match="closed"):
        t.lookup(1)


def test_ports_create_argument_errors():
    lib = native.load()
    h = ctypes.c_void_p()
    two = (ctypes.c_uint16 * 2)(53, 10000)
    twice = (ctypes.c_uint16 * 3)(53, 10000, 53)
    many = (ctypes.c_uint16 * 253)(*range(253))
    for create in (lambda *a: lib.sccsum_udp_ports_create(0, *a), lib.sccsum_udp_ports_create_host):
        assert create(ctypes.addressof(two), 2, None) == EINVAL
        assert create(None, 2, ctypes.byref(h)) == EINVAL and not h.value
        assert create(ctypes.addressof(twice), 3, ctypes.byref(h)) == EINVAL and not h.value
        assert create(ctypes.addressof(many), 253, ctypes.byref(h)) == EINVAL and not h.value
    assert lib.sccsum_udp_ports_create_host(ctypes.addressof(many), 252, ctypes.byref(h)) == 0 and h.value
    assert lib.sccsum_udp_ports_channels(h) == 252 and lib.sccsum_udp_ports_lookup(h, 251) == 251
    assert lib.sccsum_udp_ports_lookup(h, 252) == -1
    assert lib.sccsum_udp_ports_destroy(h) == 0
    rc = lib.sccsum_udp_ports_create(-1, ctypes.addressof(two), 2, ctypes.byref(h))
    assert rc != 0
    assert lib.sccsum_udp_ports_destroy(None) == 0 and lib.sccsum_udp_ports_channels(None) == 0
    assert lib.sccsum_udp_ports_lookup(None, 53) == -1
    for bad in ((1, 1), (-1,), (65536,), range(253)):
        with pytest.raises(ValueError, match="ports"):
            batch.UdpPorts(bad, device=None)


def test_device_calls_argument_errors_without_device():
    """A sample of each device call's argument errors through the Python
    binding (tests/cpp/udp_host.cc lists every one)."""
    lib = native.load()
    p = 0x10000
    table = batch.UdpPorts((53, 10000), device=None)

    def rx(tab=table.handle, nbatch=8, n=8, need=1, reject=0x1C, off=p, st=p, index=p, first=p, order=p, pay_off=p,
           sport=p, ws=p):
        return lib.sccsum_udp_rx(p, 1 << 20, off, p, nbatch, st, need, reject, 1, tab, index, n, None, first, order,
                                 pay_off, p, p, sport, ws, None)

    assert rx() == native.SCCSUM_ENODEV  # valid: only the host-only table's missing device copy stops it
    for bad in (dict(tab=None), dict(need=0x100), dict(reject=0x100), dict(n=1 << 32), dict(nbatch=1 << 32),
                dict(index=None, n=9), dict(off=None), dict(off=p + 4), dict(st=None), dict(index=p + 2),
                dict(first=None), dict(first=p + 2), dict(order=None), dict(pay_off=p + 4), dict(sport=p + 1),
                dict(ws=None), dict(ws=p + 8), dict(n=0, nbatch=0, first=None)):
        assert rx(**bad) == EINVAL, bad

    def reasm(tab=table.handle, m=8, nrec=20, need=1, reject=8, desc=p, dfirst=p, rec=p, l4=p, first=p, order=p,
              sport=p, ws=p):
        return lib.sccsum_udp_rx_reasm(desc, dfirst, p, p, p, m, rec, nrec, l4, need, reject, 1, tab, None, first,
                                       order, p, p, sport, ws, None)

    assert reasm() == native.SCCSUM_ENODEV
    assert reasm(l4=None, need=0, reject=0) == native.SCCSUM_ENODEV
    for bad in (dict(tab=None), dict(need=0x100), dict(m=1 << 31), dict(nrec=1 << 31), dict(l4=None), dict(desc=None),
                dict(desc=p + 4), dict(dfirst=p + 2), dict(rec=None), dict(rec=p + 4), dict(first=None),
                dict(order=p + 2), dict(sport=p + 1), dict(ws=None), dict(ws=p + 8), dict(m=0, first=None)):
        assert reasm(**bad) == EINVAL, bad

    def send(src=1, mtu=1500, flags=3, n=8, off=p, dport=p, l4_off=p, seed=p, needs=p, st=p, opts=True):
        o = native.UdpOpts(src, mtu, flags)
        return lib.sccsum_udp_send(ctypes.addressof(o) if opts else None, p, 1 << 20, off, p, p, dport, p, n, l4_off, p,
                                   p, seed, None, needs, st, None)

    for bad in (dict(opts=False), dict(mtu=67), dict(mtu=65536), dict(flags=4), dict(n=1 << 32), dict(off=None),
                dict(off=p + 4), dict(dport=None), dict(dport=p + 1), dict(l4_off=None), dict(l4_off=p + 4),
                dict(seed=p + 2), dict(needs=None), dict(st=None)):
        assert send(**bad) == EINVAL, bad
    for fn in (lib.sccsum_udp_rx_workspace, lib.sccsum_udp_rx_reasm_workspace):
        for n in (0, 1, 1024, 1025, 1 << 20):
            assert fn(n) >= 16 + 253 * 4 * ((n + 1023) // 1024) and fn(n) % 16 == 0


class _FakeDevicePorts(batch.UdpPorts):
    """A UdpPorts that claims the CPU tensors' device, so that the checks
    behind the table's are reached without a GPU."""

    def __init__(self, ports=(53, 10000)):
        super().__init__(ports, device=None)
        self.device = torch.device("cpu")


def test_python_wrapper_validation():
    """udp_rx_check / udp_rx_reasm_check / udp_send_check refuse wrong dtypes,
    devices, strides and sizes before any launch."""
    n = 40
    b = batch.PacketBatch(data=torch.zeros(4096, dtype=torch.uint8), off=torch.zeros(n, dtype=torch.int64),
                          length=torch.zeros(n, dtype=torch.int32), bytes_len=4096, max_len=0)
    ports = _FakeDevicePorts()
    ok = dict(status=torch.zeros(n, dtype=torch.uint8), ports=ports, host=1, need=1, reject=0x1C)
    assert batch.udp_rx_check(b, **ok) == (n, n)
    assert batch.udp_rx_check(b, index=torch.zeros(7, dtype=torch.int32), **ok) == (7, n)
    assert batch.udp_rx_check(b, index=torch.zeros(90, dtype=torch.int32), **ok) == (90, n)
    for name, value in (("status", torch.zeros(n - 1, dtype=torch.uint8)), ("status", torch.zeros(n, dtype=torch.int8)),
                        ("status", np.zeros(n, np.uint8)), ("need", 0x100), ("reject", -1), ("host", 1 << 32),
                        ("ports", object()), ("ports", batch.UdpPorts((1,), device=None)),
                        ("index", torch.zeros(5, dtype=torch.int64)), ("index", torch.zeros(10, dtype=torch.int32)[::2]),
                        ("cls", torch.zeros(n - 1, dtype=torch.uint8)), ("cls", torch.zeros(n, dtype=torch.int32))):
        with pytest.raises(ValueError, match=name):
            batch.udp_rx_check(b, **dict(ok, **{name: value}))
    with pytest.raises(ValueError, match="^ports: need a UdpPorts$"):   # the wording is part of the interface
        batch.udp_rx_check(b, **dict(ok, ports=object()))
    with pytest.raises(ValueError, match="^ports: the table lives on None, the data on cpu$"):
        batch.udp_rx_check(b, **dict(ok, ports=batch.UdpPorts((1,), device=None)))
    with pytest.raises(ValueError, match="PacketBatch"):
        batch.udp_rx_check(None, **ok)
    with pytest.raises(ValueError, match="ReasmResult"):
        batch.udp_rx_reasm_check(None, torch.zeros(64, dtype=torch.uint8), ports, 1, None, 0, 0)

    sk = dict(dst=torch.zeros(n, dtype=torch.int32), dport=torch.zeros(n, dtype=torch.int16),
              sport=torch.zeros(n, dtype=torch.int16), src_host=1, mtu=1500, flags=3)
    assert batch.udp_send_check(b, **sk) == n
    for name, value in (("dst", torch.zeros(n, dtype=torch.int64)), ("dst", torch.zeros(n - 1, dtype=torch.int32)),
                        ("dport", torch.zeros(n, dtype=torch.int32)), ("dport", torch.zeros(2 * n, dtype=torch.int16)[::2]),
                        ("sport", torch.zeros(n - 1, dtype=torch.int16)), ("sport", [0] * n), ("src_host", -1),
                        ("mtu", 67), ("mtu", 65536), ("flags", 4)):
        with pytest.raises(ValueError, match=name):
            batch.udp_send_check(b, **dict(sk, **{name: value}))
    with pytest.raises(ValueError, match="payloads"):
        batch.udp_send_check(None, **sk)


# ---------------------------------------------------------------- the model, byte by byte

def _ip(total: int, proto: int, payload: bytes, ihl: int = 5, frag: int = 0) -> bytes:
    """A header written field by field: src 10.0.1.16, dst 10.0.0.1."""
    h = bytes([0x40 | ihl, 0x00, total >> 8, total & 0xFF, 0x12, 0x34, frag >> 8, frag & 0xFF, 0x40, proto, 0x00, 0x00,
               0x0A, 0x00, 0x01, 0x10, 0x0A, 0x00, 0x00, 0x01]) + bytes([1] * (4 * (ihl - 5)))
    return h + payload


KAT_UDP = bytes([0x04, 0xD2, 0x16, 0x2E, 0x00, 0x0D, 0x00, 0x00,      # 1234 -> 5678, len 13, no checksum
                 0x68, 0x65, 0x6C, 0x6C, 0x6F])                        # "hello"
PORTS = {5678: 0, 53: 1}
SRC = 0x0A000110


def test_model_known_answers():
    # a datagram to a bound port
    p = _ip(33, 17, KAT_UDP)
    assert udp_model.atomic(p, True, PORTS) == dict(cls=0, payload=b"hello", src=SRC, sport=1234, at=28)
    assert udp_model.atomic(p, True, {53: 0, 5678: 1})["cls"] == 1
    # ... that stack_model did not deliver (another host, a bad header), or another protocol
    assert udp_model.atomic(p, False, PORTS)["cls"] == SKIP
    assert udp_model.atomic(_ip(33, 6, KAT_UDP), True, PORTS)["cls"] == SKIP
    # to an unbound port: dropped silently
    assert udp_model.atomic(p, True, {5679: 0}) == dict(cls=NOPORT, payload=b"", src=0, sport=0, at=0)
    assert udp_model.atomic(p, True, {}) ["cls"] == NOPORT
    # a 7-byte L4: get_header<udp_hdr> is null
    assert udp_model.atomic(_ip(27, 17, KAT_UDP[:7]), True, PORTS)["cls"] == SHORT
    assert udp_model.atomic(_ip(20, 17, b""), True, PORTS)["cls"] == SHORT
    r = udp_model.atomic(_ip(28, 17, KAT_UDP[:8]), True, PORTS)
    assert (r["cls"], r["payload"]) == (0, b"")
    # a frame padded past its IP length: the padding is trimmed
    r = udp_model.atomic(p + bytes([0xEE] * 6), True, PORTS)
    assert (r["cls"], r["payload"], r["at"]) == (0, b"hello", 28)
    # the IP length cuts into the datagram: what is behind it is gone, whatever udp_hdr::len says
    assert udp_model.atomic(_ip(31, 17, KAT_UDP), True, PORTS)["payload"] == b"hel"
    # a len field that disagrees with the packet is not consulted: too small, too large, zero
    for field in (8, 9, 200, 0):
        dg = KAT_UDP[:4] + field.to_bytes(2, "big") + KAT_UDP[6:]
        assert udp_model.atomic(_ip(33, 17, dg), True, PORTS)["payload"] == b"hello", field
    # ihl 6: the UDP header starts at 24
    r = udp_model.atomic(_ip(37, 17, KAT_UDP, ihl=6), True, PORTS)
    assert (r["cls"], r["payload"], r["sport"], r["at"]) == (0, b"hello", 1234, 32)
    # a reassembled datagram whose header was cut 3 + 5 over two fragments: the merged bytes are what counts
    rx = sm.Rx(sm.rx_cfg())
    big = KAT_UDP + bytes(range(11))          # 24 bytes: 3 | 5 + 16 is no legal cut (offsets are multiples of 8),
    f1 = sm._hand_frame(SRC, sm.HOST, 9, 17, 1, 0, big[:8])   # so the wire has 8 + 16 and the list is cut below
    f2 = sm._hand_frame(SRC, sm.HOST, 9, 17, 0, 1, big[8:])
    out = rx.batch([f2, f1])
    assert len(out["delivered"]) == 1 and out["delivered"][0]["data"] == big
    r = udp_model.reassembled(out["delivered"][0], PORTS)
    assert r == dict(cls=0, payload=big[8:], src=SRC, sport=1234)
    d = dict(out["delivered"][0], data=big[:3] + big[3:8])    # the same datagram as pieces of 3 and 5 bytes: E = 8
    assert udp_model.reassembled(d, PORTS) == dict(cls=0, payload=b"", src=SRC, sport=1234)
    assert udp_model.reassembled(dict(d, data=big[:7]), PORTS)["cls"] == SHORT
    assert udp_model.reassembled(dict(d, proto=6), PORTS)["cls"] == SKIP
    assert udp_model.reassembled(d, {53: 0})["cls"] == NOPORT
    # the queue: a channel keeps the first room[k] of its datagrams
    assert udp_model.queue([0, 1, 0, NOPORT, 0, 1, SKIP, 0], 2, [3, 1]) == [[0, 2, 4], [1]]
    assert udp_model.queue([0, 0], 3, [0, 5, 5]) == [[], [], []]


def test_model_send_known_answers():
    me, peer = 0x0A000001, 0x0A000110
    s = udp_model.send(b"hello", 1234, 5678, me, peer, 1500)
    assert s["zero"] == KAT_UDP and not s["needs_csum"]
    # the pseudo-header: 0a00 0001 0a00 0110 0011 000d; the datagram's words; folded, complemented
    words = [0x0A00, 0x0001, 0x0A00, 0x0110, 0x0011, 0x000D, 0x04D2, 0x162E, 0x000D, 0x0000, 0x6865, 0x6C6C, 0x6F00]
    total = sum(words)
    total = (total & 0xFFFF) + (total >> 16)
    assert s["l4"] == KAT_UDP[:6] + (~total & 0xFFFF).to_bytes(2, "big") + KAT_UDP[8:]
    assert sm.csum(s["l4"], sm.pseudo(me, peer, 17, 13)) == 0
    # offload and no cut: the folded pseudo-header sum itself, not complemented
    pseudo = sum(words[:6])
    pseudo = (pseudo & 0xFFFF) + (pseudo >> 16)
    o = udp_model.send(b"hello", 1234, 5678, me, peer, 1500, offload=True)
    assert o["needs_csum"] and o["l4"][6:8] == pseudo.to_bytes(2, "big") and o["zero"] == KAT_UDP
    assert pseudo == udp_model.pseudo_sum(me, peer, 13) == native.load().sccsum_pseudo_seed(me, peer, 17, 13)
    # offload but the datagram is cut (no UFO): the full sum; with UFO it is never cut
    big = bytes(100)
    assert not udp_model.send(big, 1, 2, me, peer, 68, offload=True)["needs_csum"]
    assert udp_model.send(big, 1, 2, me, peer, 68, offload=True, ufo=True)["needs_csum"]
    assert udp_model.send(bytes(40), 1, 2, me, peer, 68, offload=True)["needs_csum"]       # 48 + 20 == mtu
    assert not udp_model.send(bytes(41), 1, 2, me, peer, 68, offload=True)["needs_csum"]
    # what stack_model.tx makes of the zero form is the full-sum datagram
    t = sm.tx([(s["zero"], 17, peer, 7)], sm.tx_cfg(1500))
    assert t["l4"] == [s["l4"]]


def test_offload_seed_identity_through_the_oracle():
    """An empty span seeded with 0xFFFF ^ P sums to P, for every 16-bit P: the
    form in which udp_send asks the checksum pass for the bare pseudo-header
    sum.  The result convention is network order (its two bytes as stored)."""
    want = np.arange(65536, dtype=np.uint32)
    seeds = (0xFFFF ^ want).astype(np.uint32)
    got = oracle.batch_spans(np.zeros(16, np.uint8), np.zeros(65536, np.uint64), np.zeros(65536, np.uint32), seeds)
    assert np.array_equal(got.view(np.uint8).reshape(-1, 2), want.astype(">u2").view(np.uint8).reshape(-1, 2))
    for p in (0, 1, 0x1234, 0xFFFF):
        assert oracle.batch_spans(np.zeros(16, np.uint8), np.array([5], np.uint64), np.zeros(1, np.uint32),
                                  np.array([0xFFFF ^ p], np.uint32)).view(np.uint8).tolist() == [p >> 8, p & 0xFF]


# ---------------------------------------------------------------- the traffic of the GPU tests

def _classes(seed: int, nch: int):
    c = udp_traffic.case(seed)
    ports = {p: k for k, p in enumerate(udp_traffic.PORTS[:nch])}
    at = [udp_model.atomic(p, info["delivered"], ports) for p, info in zip(c["ip"], c["info"])]
    re = [udp_model.reassembled(d, ports) for d in c["delivered"]]
    return c, at, re


@pytest.mark.parametrize("seed", udp_traffic.SEEDS)
def test_traffic_coverage(seed):
    """Every seed holds every class, an empty channel and a channel with more
    datagrams than its room, on the atomic path; the reassembled path holds
    datagrams with and without a channel."""
    c, at, re = _classes(seed, 252)
    assert len(c["ip"]) >= 2 * 1024 + 7
    cls = [a["cls"] for a in at]
    for want in (SKIP, SHORT, NOPORT, 0, 1, 250):
        assert want in cls, want
    assert 251 not in cls                                        # an empty channel
    assert cls.count(0) > udp_traffic.room_for(0) == 1024        # more than the queue holds
    assert any(cls.count(k) > udp_traffic.room_for(k) for k in range(1, 251))
    assert any(0 < cls.count(k) <= udp_traffic.room_for(k) for k in range(1, 251))
    rc = [r["cls"] for r in re]
    assert len(rc) >= 40 and NOPORT in rc and any(k < 252 for k in rc)
    assert c["not_plain"] >= 6                                   # the MTU 576 keys are the host's
    # the oddities are there: options, padding, len fields that disagree
    ihl = {p[0] & 0xF for p, a in zip(c["ip"], at) if a["cls"] < 252}
    assert ihl == set(range(5, 16))
    padded = [a for p, a in zip(c["ip"], at) if a["cls"] < 252 and len(p) > sm.be16(p, 2)]
    assert len(padded) >= 3
    lying = [a for p, a in zip(c["ip"], at)
             if a["cls"] < 252 and sm.be16(p, 4 * (p[0] & 0xF) + 4) != len(a["payload"]) + 8]
    assert len(lying) >= 5
    assert any(sm.be16(d["data"], 4) != len(d["data"]) for d, r in zip(c["delivered"], re) if r["cls"] < 252)


@pytest.mark.parametrize("nch", [0, 1, 65, 252])
def test_fast_rx_is_the_model(nch):
    """udp_model.fast_rx (the scale test's yardstick) against the per-datagram
    model on a seed's IPv4 bucket, with and without an index."""
    c, at, _ = _classes(1, nch)
    data = np.frombuffer(b"".join(c["ip"]), dtype=np.uint8)
    length = np.array([len(p) for p in c["ip"]], dtype=np.uint32)
    off = (np.cumsum(length, dtype=np.uint64) - length).astype(np.uint64)
    status = np.array([i["status"] for i in c["info"]], dtype=np.uint8)
    rng = np.random.default_rng(nch)
    for index in (None, rng.permutation(off.size)[:700], np.concatenate([np.arange(5, 900, 3), [off.size, 1 << 31]])):
        items = at if index is None else [at[int(j)] if j < off.size else dict(cls=SKIP, payload=b"", src=0, sport=0, at=0)
                                          for j in index]
        want = udp_traffic.expect_rx(items, nch, index)
        got = udp_model.fast_rx(data, data.size, off, length, status, native.ST_OK,
                                native.ST_MALFORMED | native.ST_RANGE | native.ST_IPFRAG, sm.HOST,
                                udp_traffic.PORTS[:nch], index)
        for name in ("cls", "first", "order", "pay_len", "src", "sport"):
            assert np.array_equal(got[name], want[name]), name
        idx = np.arange(off.size) if index is None else np.asarray(index)
        pay_off = [int(off[idx[j]]) + items[j]["at"] if idx[j] < off.size else 0 for j in want["pos"]]
        assert got["pay_off"].tolist() == pay_off


# ---------------------------------------------------------------- the C++ classes

def test_cpp_classes_on_the_host(tmp_path):
    """seastar::net::udp_ports, udp_rx and udp_tx (tests/cpp/udp_host.cc): the
    table against a std::map, workspace() and taken(), and every argument
    error of the three device calls."""
    cpp_host.build_and_run(tmp_path, "udp_host", "udp_host: OK")


def test_cpp_classes_on_the_host_sanitized(tmp_path):
    """The same stand-alone program with udp.hip itself compiled in, its host
    side under AddressSanitizer + UndefinedBehaviorSanitizer (device code is
    not instrumented): the table's build and lookup and the argument checks."""
    cpp_host.build_and_run_sanitized(tmp_path, "udp_host", "udp.hip", "udp_host: OK")
