"""The TCP layer, the host side (no device needed): the new C-ABI symbols, the
connection table's lookup against a dict (colliding keys, a probe run that
wraps), argument errors (reported before any device work), the per-segment
model tests/tcp_model.py pinned by frames written out byte by byte, both RST
checksum forms and the three tcp_send forms through the oracle, the model's
array form pinned to it, and a coverage check of the traffic
tests/test_gpu_tcp.py runs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import cpp_host
import oracle
import stack_model as sm
import tcp_model as tm
import tcp_traffic
from seastar_amd import batch, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = native.SCCSUM_EINVAL, native.SCCSUM_ENODEV

TCP_SYMBOLS = ["sccsum_tcp_conns_create", "sccsum_tcp_conns_create_host", "sccsum_tcp_conns_destroy",
               "sccsum_tcp_conns_lookup", "sccsum_tcp_conns_listening", "sccsum_tcp_conns_slot", "sccsum_tcp_conns_bits",
               "sccsum_tcp_conns_count", "sccsum_tcp_rx_workspace", "sccsum_tcp_rx", "sccsum_tcp_send"]


def test_symbols_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    declared = native.header_symbols()
    lib = native.load()
    for s in TCP_SYMBOLS:
        assert s in declared and s in exported and s in native._PROTOS, s
        assert getattr(lib, s).argtypes is not None
    assert lib.sccsum_abi_version() == native.ABI_VERSION == 4
    header = open(native.HEADER_PATH).read()
    for name, value, model in (("SKIP", native.TCP_SKIP, tm.SKIP), ("SHORT", native.TCP_SHORT, tm.SHORT),
                               ("CONN", native.TCP_CONN, tm.CONN), ("LISTEN", native.TCP_LISTEN, tm.LISTEN),
                               ("RESET", native.TCP_RESET, tm.RESET), ("NOCONN", native.TCP_NOCONN, tm.NOCONN)):
        assert value == model
        assert f"0x{value:02X}u" in header.split(f"#define SCCSUM_TCP_{name}")[1].split("\n")[0]
    assert "#define SCCSUM_TCP_MAX_CONNS (1u << 20)" in header and native.TCP_MAX_CONNS == 1 << 20
    assert batch.TCP_NEED == tm.NEED and batch.TCP_REJECT == tm.REJECT
    assert batch.TCP_SEG_DTYPE == tm.SEG_DTYPE and tm.SEG_DTYPE.itemsize == 32
    assert os.path.join(REPO, "seastar_amd", "csrc", "tcp.hip") in __import__("seastar_amd.build").build.SOURCES


def test_struct_layouts_match_the_header(tmp_path):
    structs = (("sccsum_tcp_conn", native.TcpConn), ("sccsum_tcp_seg", native.TcpSeg), ("sccsum_tcp_out", native.TcpOut),
               ("sccsum_tcp_opts", native.TcpOpts))
    lines = []
    for cname, cls in structs:
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <sccsum.h>\nint main(void) {\n"
                   + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs:
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert ctypes.sizeof(native.TcpSeg) == 32 and ctypes.sizeof(native.TcpOut) == 24
    for f, _ in native.TcpSeg._fields_:
        assert getattr(native.TcpSeg, f).offset == tm.SEG_DTYPE.fields[f][1]
    for f, _ in native.TcpOut._fields_:
        assert getattr(native.TcpOut, f).offset == batch.TCP_OUT_DTYPE.fields[f][1]


# ---------------------------------------------------------------- the table

@pytest.mark.parametrize("nconns", [0, 1, 8, 9, 253, 5000])
def test_lookup_against_a_dict(nconns):
    """Every entry, misses that differ in exactly one field, and every port."""
    conns = tcp_traffic.conn_array(nconns)
    if nconns >= 8:
        conns[3] = (0, 0, 0, 0)                       # any 96-bit key is valid
        conns[4] = (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFF, 0xFFFF)
    listen = [0, 80, 65535][:min(nconns, 3)]
    t = batch.TcpConns(conns, listen, device=None)
    assert t.count == nconns
    bits = 4
    while (1 << bits) < 2 * nconns:
        bits += 1
    assert t.bits == bits
    for c, (a, b, p, q) in enumerate(conns.tolist()):
        assert t.lookup(a, b, p, q) == c
    want = {tuple(r): c for c, r in enumerate(conns.tolist())}
    for c, (a, b, p, q) in enumerate(conns.tolist()[:300]):
        for miss in ((a ^ 1, b, p, q), (a, b ^ 0x10000, p, q), (a, b, p ^ 1, q), (a, b, p, q ^ 0x8000), (b, a, q, p)):
            assert t.lookup(*miss) == want.get(miss), (c, miss)
    assert [port for port in range(65536) if t.listening(port)] == sorted(listen)
    t.close()
    with pytest.raises(ValueError, match="closed"):
        t.lookup(1, 2, 3, 4)


def _colliding(bits: int, home: int, count: int, start: int = 1) -> list:
    """`count` keys whose home slot in a 2^bits table is `home`."""
    lib = native.load()
    out, b = [], start
    while len(out) < count:
        if lib.sccsum_tcp_conns_slot(sm.HOST, b, 80, 5000, bits) == home:
            out.append((sm.HOST, b, 80, 5000))
        b += 1
    return out


def test_colliding_keys_and_a_probe_run_that_wraps():
    lib = native.load()
    # slot() is the low bits of one 32-bit mix
    full = lib.sccsum_tcp_conns_slot(1, 2, 3, 4, 32)
    for bits in (4, 5, 17, 21):
        assert lib.sccsum_tcp_conns_slot(1, 2, 3, 4, bits) == full & ((1 << bits) - 1)
    # 8 connections -> 16 slots; six keys homed at the last slot: the run wraps to slots 0..4
    keys = _colliding(4, 15, 6) + _colliding(4, 2, 2, start=100000)     # ... and pushes two keys of slot 2 further
    t = batch.TcpConns(keys, device=None)
    assert t.bits == 4
    for c, k in enumerate(keys):
        assert t.lookup(*k) == c
    others = _colliding(4, 15, 9)[6:] + _colliding(4, 0, 2, start=200000) + _colliding(4, 7, 1)
    for k in others:
        assert t.lookup(*k) is None
    # every field is compared: a key that differs from an entry in one field only and shares its home slot misses
    base = (sm.HOST, 0x0B000001, 80, 5000)
    home = lib.sccsum_tcp_conns_slot(*base, 4)
    t = batch.TcpConns([base], device=None)
    for field, limit in enumerate((1 << 32, 1 << 32, 1 << 16, 1 << 16)):
        twins = []
        for step in range(1, 400):
            k = list(base)
            k[field] = (k[field] + step) % limit
            if lib.sccsum_tcp_conns_slot(*k, 4) == home:
                twins.append(tuple(k))
        assert len(twins) >= 5
        assert [t.lookup(*k) for k in twins] == [None] * len(twins), field
    assert t.lookup(*base) == 0


def test_create_argument_errors():
    lib = native.load()
    h = ctypes.c_void_p()
    two = (native.TcpConn * 2)(native.TcpConn(1, 2, 3, 4), native.TcpConn(1, 2, 3, 5))
    twice = (native.TcpConn * 3)(native.TcpConn(1, 2, 3, 4), native.TcpConn(1, 2, 3, 5), native.TcpConn(1, 2, 3, 4))
    ports = (ctypes.c_uint16 * 2)(80, 443)
    ports_twice = (ctypes.c_uint16 * 3)(80, 443, 80)
    a = ctypes.addressof
    for create in (lambda *x: lib.sccsum_tcp_conns_create(0, *x), lib.sccsum_tcp_conns_create_host):
        assert create(a(two), 2, a(ports), 2, None) == EINVAL
        assert create(None, 2, a(ports), 2, ctypes.byref(h)) == EINVAL and not h.value
        assert create(a(two), 2, None, 2, ctypes.byref(h)) == EINVAL and not h.value
        assert create(a(twice), 3, None, 0, ctypes.byref(h)) == EINVAL and not h.value
        assert create(a(two), 2, a(ports_twice), 3, ctypes.byref(h)) == EINVAL and not h.value
        assert create(a(two), (1 << 20) + 1, None, 0, ctypes.byref(h)) == EINVAL and not h.value
        assert create(None, 0, a(ports), 65537, ctypes.byref(h)) == EINVAL and not h.value
    assert lib.sccsum_tcp_conns_create_host(None, 0, None, 0, ctypes.byref(h)) == 0 and h.value
    assert lib.sccsum_tcp_conns_count(h) == 0 and lib.sccsum_tcp_conns_bits(h) == 4
    assert lib.sccsum_tcp_conns_lookup(h, 0, 0, 0, 0) == -1 and lib.sccsum_tcp_conns_listening(h, 0) == 0
    assert lib.sccsum_tcp_conns_destroy(h) == 0
    assert lib.sccsum_tcp_conns_create(-1, a(two), 2, None, 0, ctypes.byref(h)) == ENODEV and not h.value
    assert lib.sccsum_tcp_conns_destroy(None) == 0 and lib.sccsum_tcp_conns_count(None) == 0
    assert lib.sccsum_tcp_conns_bits(None) == 0 and lib.sccsum_tcp_conns_lookup(None, 1, 2, 3, 4) == -1
    assert lib.sccsum_tcp_conns_listening(None, 80) == 0
    for bad in (dict(conns=[(1, 2, 3, 4), (1, 2, 3, 4)]), dict(conns=[(1 << 32, 2, 3, 4)]), dict(conns=[(1, 2, 65536, 4)]),
                dict(conns=[(1, 2, 3, -4)]), dict(listen=[80, 80]), dict(listen=[65536])):
        with pytest.raises(ValueError, match="conns|listen"):
            batch.TcpConns(device=None, **bad)


def test_device_calls_argument_errors_without_device():
    """Every argument error of the two device calls, through the Python binding."""
    lib = native.load()
    p = 0x10000
    table = batch.TcpConns([(1, 2, 3, 4)], [80], device=None)

    def rx(tab=table.handle, nbatch=8, n=8, need=3, reject=0x1C, flags=0, off=p, ln=p, st=p, index=p, first=p, order=p,
           seg=p, src=p, run_conn=p, run_first=p, rst=p, rst_dst=p, total=p, ws=p, data=p):
        return lib.sccsum_tcp_rx(data, 1 << 20, off, ln, nbatch, st, need, reject, 1, tab, index, n, flags, None, first,
                                 order, seg, src, run_conn, run_first, rst, rst_dst, total, ws, None)

    assert rx() == ENODEV     # valid: only the host-only table's missing device copy stops it
    assert rx(seg=p + 8, flags=1) == ENODEV
    for bad in (dict(tab=None), dict(need=0x100), dict(reject=0x100), dict(flags=2), dict(n=1 << 32),
                dict(nbatch=1 << 32), dict(index=None, n=9), dict(off=None), dict(off=p + 4), dict(ln=None),
                dict(ln=p + 2), dict(st=None), dict(data=None), dict(index=p + 2), dict(first=None), dict(first=p + 2),
                dict(order=None), dict(order=p + 2), dict(seg=None), dict(seg=p + 4), dict(src=None), dict(src=p + 2),
                dict(run_conn=None), dict(run_conn=p + 1), dict(run_first=None), dict(run_first=p + 2), dict(rst=None),
                dict(rst=p + 2), dict(rst_dst=None), dict(rst_dst=p + 2), dict(total=None), dict(total=p + 4),
                dict(ws=None), dict(ws=p + 8), dict(n=0, nbatch=0, first=None), dict(n=0, nbatch=0, total=None),
                dict(n=0, nbatch=0, run_first=None)):
        assert rx(**bad) == EINVAL, bad
    assert rx(n=0, nbatch=0, order=None, seg=None, src=None, run_conn=None, rst=None, rst_dst=None, off=None, ln=None,
              st=None, index=None) == ENODEV

    def send(src=1, mtu=1500, flags=3, n=8, off=p, ln=p, out=p, l4_off=p, l4_len=p, sum_len=p, seed=p, tso=p, needs=p,
             st=p, opts=True, data=p):
        o = native.TcpOpts(src, mtu, flags)
        return lib.sccsum_tcp_send(ctypes.addressof(o) if opts else None, data, 1 << 20, off, ln, out, n, l4_off, l4_len,
                                   sum_len, seed, tso, None, needs, st, None)

    for bad in (dict(opts=False), dict(mtu=67), dict(mtu=65536), dict(flags=4), dict(n=1 << 32), dict(data=None),
                dict(off=None), dict(off=p + 4), dict(ln=None), dict(ln=p + 2), dict(out=None), dict(out=p + 2),
                dict(l4_off=None), dict(l4_off=p + 4), dict(l4_len=None), dict(l4_len=p + 2), dict(sum_len=None),
                dict(sum_len=p + 2), dict(seed=None), dict(seed=p + 2), dict(tso=None), dict(tso=p + 1),
                dict(needs=None), dict(st=None)):
        assert send(**bad) == EINVAL, bad
    for n in (0, 1, 1024, 1025, 1 << 20):
        for nconns in (0, 253, 1 << 20):
            w = lib.sccsum_tcp_rx_workspace(n, nconns)
            assert w >= 56 * n + 256 * 4 * ((n + 1023) // 1024) and w % 16 == 0


class _FakeDeviceConns(batch.TcpConns):
    """A TcpConns that claims the CPU tensors' device, so that the checks
    behind the table's are reached without a GPU."""

    def __init__(self):
        super().__init__([(1, 2, 3, 4)], [80], device=None)
        self.device = torch.device("cpu")


def test_python_wrapper_validation():
    n = 40
    b = batch.PacketBatch(data=torch.zeros(4096, dtype=torch.uint8), off=torch.zeros(n, dtype=torch.int64),
                          length=torch.zeros(n, dtype=torch.int32), bytes_len=4096, max_len=0)
    ok = dict(status=torch.zeros(n, dtype=torch.uint8), conns=_FakeDeviceConns(), host=1, need=3, reject=0x1C)
    assert batch.tcp_rx_check(b, **ok) == (n, n)
    assert batch.tcp_rx_check(b, index=torch.zeros(90, dtype=torch.int32), **ok) == (90, n)
    for name, value in (("status", torch.zeros(n - 1, dtype=torch.uint8)), ("status", torch.zeros(n, dtype=torch.int8)),
                        ("need", 0x100), ("reject", -1), ("host", 1 << 32), ("conns", object()),
                        ("conns", batch.TcpConns(device=None)), ("index", torch.zeros(5, dtype=torch.int64)),
                        ("index", torch.zeros(10, dtype=torch.int32)[::2]), ("flags", 2),
                        ("cls", torch.zeros(n - 1, dtype=torch.uint8)), ("cls", torch.zeros(n, dtype=torch.int32))):
        with pytest.raises(ValueError, match=name):
            batch.tcp_rx_check(b, **dict(ok, **{name: value}))
    with pytest.raises(ValueError, match="^conns: need a TcpConns$"):
        batch.tcp_rx_check(b, **dict(ok, conns=object()))
    with pytest.raises(ValueError, match="PacketBatch"):
        batch.tcp_rx_check(None, **ok)
    sk = dict(out=torch.zeros((n, 24), dtype=torch.uint8), src_host=1, mtu=1500, flags=3)
    assert batch.tcp_send_check(b, **sk) == n
    for name, value in (("out", torch.zeros((n, 6), dtype=torch.int32)), ("out", torch.zeros((n - 1, 24), dtype=torch.uint8)),
                        ("out", torch.zeros(24 * n, dtype=torch.uint8)), ("src_host", -1), ("mtu", 67), ("mtu", 65536),
                        ("flags", 4)):
        with pytest.raises(ValueError, match=name):
            batch.tcp_send_check(b, **dict(sk, **{name: value}))
    with pytest.raises(ValueError, match="payloads"):
        batch.tcp_send_check(None, **sk)


# ---------------------------------------------------------------- the model, byte by byte

SRC, DST = 0x0A000110, 0x0A000001


def _ip(total: int, l4: bytes, ihl: int = 5, proto: int = 6) -> bytes:
    """A header written field by field: src 10.0.1.16, dst 10.0.0.1."""
    h = bytes([0x40 | ihl, 0x00, total >> 8, total & 0xFF, 0x12, 0x34, 0x00, 0x00, 0x40, proto, 0x00, 0x00,
               0x0A, 0x00, 0x01, 0x10, 0x0A, 0x00, 0x00, 0x01]) + bytes([1] * (4 * (ihl - 5)))
    return h + l4


def _seg(flags: int, data_offset: int = 5, dport=(0x00, 0x50), tail: bytes = b"") -> bytes:
    """49152 -> dport, seq 0x01020304, ack 0x0A0B0C0D, window 0x2000, checksum and urgent as they come."""
    return bytes([0xC0, 0x00, dport[0], dport[1], 0x01, 0x02, 0x03, 0x04, 0x0A, 0x0B, 0x0C, 0x0D, data_offset << 4,
                  flags, 0x20, 0x00, 0xBE, 0xEF, 0x00, 0x07]) + tail


OK = dict(status=sm.ST_OK | sm.ST_L4_OK, delivered=True)
TCBS = {(DST, SRC, 80, 49152): 7}
HDR = dict(sport=49152, dport=80, seq=0x01020304, ack=0x0A0B0C0D, rsvd1=0, data_offset=5, flags=0x18, window=0x2000,
           checksum=0xBEEF, urgent=7)


def test_model_known_answers():
    a = lambda p, tcbs=TCBS, listening=(22,), info=OK, **kw: tm.atomic(p, info, tcbs, listening, **kw)  # noqa: E731
    # a segment of a known connection, five bytes of payload
    r = a(_ip(45, _seg(0x18, tail=b"hello")))
    assert r == dict(cls=tm.CONN, conn=7, hdr=HDR, H=20, pay_len=5, src=SRC, dst=DST, at=40)
    assert tm.seg_record(r, 1000) == (1040, 5, 0x01020304, 0x0A0B0C0D, 7, 0x2000, 49152, 80, 0x18, 20)
    assert tm.hdr_write(49152, 80, 0x01020304, 0x0A0B0C0D, 5, 0x18, 0x2000, 0xBEEF, 7) == _seg(0x18)
    # the same four-tuple with local and foreign swapped: a miss (here: a closed port, answered)
    assert a(_ip(40, _seg(0x18)), tcbs={(SRC, DST, 49152, 80): 7})["cls"] == tm.RESET
    assert a(_ip(40, _seg(0x18)), tcbs={(DST, SRC, 49152, 80): 7})["cls"] == tm.RESET
    # the masks, not delivered, another protocol
    assert a(_ip(40, _seg(0x18)), info=dict(OK, status=sm.ST_OK))["cls"] == tm.SKIP           # the checksum failed
    assert a(_ip(40, _seg(0x18)), info=dict(OK, status=sm.ST_OK), need=sm.ST_OK)["cls"] == tm.CONN   # rx_csum_offload
    assert a(_ip(40, _seg(0x18)), info=dict(OK, delivered=False))["cls"] == tm.SKIP
    assert a(_ip(40, _seg(0x18), proto=17))["cls"] == tm.SKIP
    assert a(_ip(40, _seg(0x18)), info=dict(OK, status=sm.ST_OK | sm.ST_L4_OK | sm.ST_IPFRAG))["cls"] == tm.SKIP
    # a SYN to a listening port
    r = a(_ip(40, _seg(0x02, dport=(0x00, 0x16))))
    assert (r["cls"], r["conn"], r["hdr"]["flags"], r["at"]) == (tm.LISTEN, tm.NO_CONN, 2, 40)
    # a SYN, an ACK, a SYN|ACK and a bare RST to a closed port
    closed = (0x01, 0xBB)
    want = {0x02: bytes([0x01, 0xBB, 0xC0, 0x00, 0, 0, 0, 0, 0x01, 0x02, 0x03, 0x05, 0x50, 0x14, 0, 0]),
            0x10: bytes([0x01, 0xBB, 0xC0, 0x00, 0x0A, 0x0B, 0x0C, 0x0D, 0, 0, 0, 0, 0x50, 0x04, 0, 0]),
            0x12: bytes([0x01, 0xBB, 0xC0, 0x00, 0x0A, 0x0B, 0x0C, 0x0D, 0x01, 0x02, 0x03, 0x05, 0x50, 0x14, 0, 0])}
    pseudo_words = [0x0A00, 0x0001, 0x0A00, 0x0110, 0x0006, 0x0014]           # local = dst, foreign = src, 6, 20
    pseudo = sum(pseudo_words)
    pseudo = (pseudo & 0xFFFF) + (pseudo >> 16)
    for flags, head in want.items():
        r = a(_ip(40, _seg(flags, dport=closed)))
        assert r["cls"] == tm.RESET
        full = tm.respond_with_reset(r["hdr"], r["dst"], r["src"])
        off = tm.respond_with_reset(r["hdr"], r["dst"], r["src"], offload=True)
        assert full[:16] == off[:16] == head and full[18:] == off[18:] == b"\0\0"
        # the full one verifies under the oracle's sum over pseudo-header + segment; the offload one is the folded sum
        c = oracle.new()
        oracle.sum_bytes(c, b"".join(w.to_bytes(2, "big") for w in pseudo_words) + full)
        assert oracle.get(c) == 0
        assert off[16:18] == pseudo.to_bytes(2, "big")
        assert pseudo == native.load().sccsum_pseudo_seed(DST, SRC, 6, 20) == oracle.pseudo_seed(DST, SRC, 6, 20)
    r = a(_ip(40, _seg(0x04, dport=closed)))
    assert r["cls"] == tm.NOCONN and tm.respond_with_reset(r["hdr"], DST, SRC) is None
    assert a(_ip(40, _seg(0x14, dport=closed)))["cls"] == tm.NOCONN
    # the sequence number wraps
    wrap = dict(HDR, seq=0xFFFFFFFF, flags=2)
    assert tm.respond_with_reset(wrap, DST, SRC)[8:12] == b"\0\0\0\0"
    # E = 19 and E = 20
    assert a(_ip(39, _seg(0x18)[:19])) == dict(cls=tm.SHORT, conn=tm.NO_CONN, hdr=None, H=0, pay_len=0, src=0, dst=0, at=0)
    assert tm.seg_record(a(_ip(39, _seg(0x18)[:19])), 64) == (64, 0, 0, 0, tm.NO_CONN, 0, 0, 0, 0, 0)
    assert tm.seg_record(a(_ip(39, _seg(0x18)[:19])), None)[0] == 0
    assert a(_ip(40, _seg(0x18)))["cls"] == tm.CONN and a(_ip(40, _seg(0x18)))["pay_len"] == 0
    # the IP length cuts the L4 to 19 bytes though the frame has more
    assert a(_ip(39, _seg(0x18, tail=b"hello")))["cls"] == tm.SHORT
    # H = 16
    assert a(_ip(45, _seg(0x18, data_offset=4, tail=b"hello")))["cls"] == tm.SHORT
    # H = 24 with E = 20: to a connection, to a listener (dropped), to a closed port (answered: only 20 bytes are read)
    assert a(_ip(40, _seg(0x18, data_offset=6)))["cls"] == tm.SHORT
    assert a(_ip(40, _seg(0x02, data_offset=6, dport=(0x00, 0x16))))["cls"] == tm.SHORT
    r = a(_ip(40, _seg(0x02, data_offset=6, dport=closed)))
    assert (r["cls"], r["H"], r["pay_len"], r["at"]) == (tm.RESET, 24, 0, 44)
    assert tm.respond_with_reset(r["hdr"], DST, SRC)[:16] == want[0x02]
    # H = 24 with E = 24: four option bytes, no payload; with E = 29 five bytes
    r = a(_ip(49, _seg(0x18, data_offset=6, tail=b"\1\1\1\1hello")))
    assert (r["cls"], r["H"], r["pay_len"], r["at"]) == (tm.CONN, 24, 5, 44)
    # ihl 6: the TCP header starts at 24
    r = a(_ip(49, _seg(0x18, tail=b"hello"), ihl=6))
    assert (r["cls"], r["pay_len"], r["at"], r["hdr"]["sport"]) == (tm.CONN, 5, 44, 49152)
    # a padded frame: the padding is trimmed
    r = a(_ip(45, _seg(0x18, tail=b"hello")) + bytes([0xEE] * 6))
    assert (r["cls"], r["pay_len"], r["at"]) == (tm.CONN, 5, 40)
    # the header round trip, every flag bit and the reserved ones
    for flags in range(256):
        h = tm.hdr_read(_seg(flags))
        assert h["flags"] == flags and tm.hdr_write(**h) == _seg(flags)
    assert tm.hdr_read(bytes([0] * 12 + [0xAB] + [0] * 7))["rsvd1"] == 0xB


def test_model_send_known_answers_and_the_offload_seed_identity():
    """The three forms of output_one; an empty span seeded with 0xFFFF ^ P sums
    to P under the oracle, which is how tcp_send asks for the bare sum."""
    me, peer = DST, SRC
    o = dict(dst=peer, seq=0x01020304, ack=0x0A0B0C0D, sport=49152, dport=80, window=0x2000, flags=0x18, mss=1460)
    s = tm.send(b"hello", o, me)
    assert s["zero"] == _seg(0x18)[:16] + b"\0\0\0\0" + b"hello" and not s["needs_csum"] and s["tso_seg"] == 0
    assert sm.csum(s["l4"], sm.pseudo(me, peer, 6, 25)) == 0
    c = oracle.new()
    oracle.sum_bytes(c, bytes([0x0A, 0, 0, 1, 0x0A, 0, 1, 0x10, 0, 6, 0, 25]) + s["l4"])
    assert oracle.get(c) == 0
    opt = tm.send(b"hello", dict(o, flags=2), me, options=bytes([2, 4, 5, 0xB4]))
    assert opt["zero"][12] == 0x60 and opt["zero"][20:24] == bytes([2, 4, 5, 0xB4]) and len(opt["zero"]) == 29
    assert sm.tx([(s["zero"], 6, peer, 7)], dict(sm.tx_cfg(1500), host=me))["l4"] == [s["l4"]]
    forms = [(tm.send(b"hello", o, me, offload=True), 25, 0),
             (tm.send(b"hello", o, me, offload=True, tso=True), 25, 0),              # 5 <= mss
             (tm.send(b"hello", dict(o, mss=4), me, offload=True, tso=True), 0, 4),  # 5 > mss: length 0
             (tm.send(b"hello", dict(o, mss=5), me, offload=True, tso=True), 25, 0)]
    for got, plen, seg in forms:
        p = oracle.pseudo_seed(me, peer, 6, plen)
        assert got["needs_csum"] and got["tso_seg"] == seg and got["l4"][16:18] == p.to_bytes(2, "big")
        assert oracle.batch_spans(np.zeros(16, np.uint8), np.array([3], np.uint64), np.zeros(1, np.uint32),
                                  np.array([0xFFFF ^ p], np.uint32)).view(np.uint8).tolist() == [p >> 8, p & 0xFF]
    assert not tm.send(b"hello", dict(o, mss=4), me, tso=True)["needs_csum"]          # TSO alone changes nothing
    full = oracle.batch_spans(np.frombuffer(s["zero"], np.uint8), np.zeros(1, np.uint64), np.array([25], np.uint32),
                              np.array([oracle.pseudo_seed(me, peer, 6, 25)], np.uint32))
    assert full.view(np.uint8).tobytes() == s["l4"][16:18]
    assert tm.send_status(20, 5, 20, 25, False, 0) == 0
    assert tm.send_status(19, 5, 20, 100, False, 0) == sm.ST_RANGE
    assert tm.send_status(20, 5, 20, 24, False, 0) == sm.ST_RANGE
    assert tm.send_status(60, 5, 64, 100, False, 0) == sm.ST_RANGE | sm.ST_MALFORMED
    assert tm.send_status(60, 5, 22, 100, False, 0) == sm.ST_MALFORMED
    assert tm.send_status(60, 65515 - 19, 20, 1 << 20, False, 0) == sm.ST_MALFORMED
    assert tm.send_status(60, 65515 - 20, 20, 1 << 20, False, 0) == 0
    assert tm.send_status(60, 5, 20, 100, True, 0) == sm.ST_MALFORMED


# ---------------------------------------------------------------- the traffic of the GPU tests

@pytest.mark.parametrize("nconns", [0, 1, 253, 254, 65533, 65534])
def test_traffic_coverage(nconns):
    """The mixed batch holds every class and every reset form under every
    table size, connections on both sides of the sort's pass boundaries, the
    header shapes and a connection with several interleaved segments."""
    c = tcp_traffic.case(0)
    assert len(c["ip"]) >= tcp_traffic.FULL
    items = tcp_traffic.items(c, nconns)
    cls = [it["cls"] for it in items]
    for want in (tm.LISTEN, tm.RESET, tm.NOCONN, tm.SHORT, tm.SKIP) + ((tm.CONN,) if nconns else ()):
        assert cls.count(want) >= 5, want
    resets = [it["hdr"]["flags"] & (tm.SYN | tm.ACK) for it in items if it["cls"] == tm.RESET]
    assert set(resets) == {0, tm.SYN, tm.ACK, tm.SYN | tm.ACK}
    assert any(it["cls"] == tm.RESET and it["H"] > 20 and it["pay_len"] == 0 for it in items)   # H > E, answered
    conns = {it["conn"] for it in items if it["cls"] == tm.CONN}
    assert conns == {k for k in set(tcp_traffic.HOT) | conns if k < nconns}
    if nconns:
        assert nconns - 1 in conns or nconns > 65536
    if nconns >= 253:
        assert {it["hdr"]["flags"] & 0x3F for it in items if it["cls"] == tm.CONN} == set(range(64))
        assert {p[0] & 0xF for p, it in zip(c["ip"], items) if it["cls"] == tm.CONN} == set(range(5, 16))
        assert {it["H"] for it in items if it["cls"] == tm.CONN} >= {20, 24, 60}
        assert any(len(p) > sm.be16(p, 2) for p, it in zip(c["ip"], items) if it["cls"] == tm.CONN)
        assert max(sum(1 for it in items if it["conn"] == k) for k in conns) >= 20
    assert {it["hdr"]["flags"] & 0x3F for it in items if it["cls"] in (tm.RESET, tm.NOCONN)} == set(range(64))
    # rx_csum_offload: the frame with the bad checksum is a segment again
    loose = tcp_traffic.items(c, nconns, need=sm.ST_OK)
    assert sum(a["cls"] == tm.SKIP and b["cls"] != tm.SKIP for a, b in zip(items, loose)) >= 1


@pytest.mark.parametrize("nconns", [0, 1, 254, 65534])
def test_fast_rx_is_the_model(nconns):
    """tcp_model.fast_rx (the scale test's yardstick) against the per-segment
    model on the mixed batch, with and without an index."""
    c = tcp_traffic.case(0)
    at = tcp_traffic.items(c, nconns)
    data = np.frombuffer(b"".join(c["ip"]) + bytes(64), dtype=np.uint8)
    length = np.array([len(p) for p in c["ip"]], dtype=np.uint32)
    off = (np.cumsum(length, dtype=np.uint64) - length).astype(np.uint64)
    status = np.array([i["status"] for i in c["info"]], dtype=np.uint8)
    rng = np.random.default_rng(nconns)
    skip = dict(cls=tm.SKIP, conn=tm.NO_CONN, hdr=None, H=0, pay_len=0, src=0, dst=0, at=0)
    for index in (None, rng.permutation(off.size)[:700], np.concatenate([np.arange(5, 900, 3), [off.size, 1 << 31]])):
        items = at if index is None else [at[int(j)] if j < off.size else skip for j in index]
        want = tm.expect_rx(items, off, index)
        got = tm.fast_rx(data, data.size - 64, off, length, status, tm.NEED, tm.REJECT, sm.HOST,
                         tcp_traffic.conn_array(nconns), tcp_traffic.LISTEN, index)
        for name in ("cls", "first", "order", "seg", "src", "run_conn", "run_first"):
            assert np.array_equal(got[name], want[name]), name


# ---------------------------------------------------------------- the C++ classes

def test_cpp_classes_on_the_host(tmp_path):
    """seastar::net::tcp_conns, tcp_rx and tcp_tx (tests/cpp/tcp_host.cc): the
    table against a std::map, workspace() and taken(), and the argument errors
    of the two device calls."""
    cpp_host.build_and_run(tmp_path, "tcp_host", "tcp_host: OK")


def test_cpp_classes_on_the_host_sanitized(tmp_path):
    """The same stand-alone program with tcp.hip itself compiled in, its host
    side under AddressSanitizer + UndefinedBehaviorSanitizer (device code is
    not instrumented): the table's build and lookup and the argument checks."""
    cpp_host.build_and_run_sanitized(tmp_path, "tcp_host", "tcp.hip", "tcp_host: OK")
