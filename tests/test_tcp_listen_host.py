"""The TCP passive open without a GPU: the per-segment model pinned on buckets
written out by hand, the numpy restatement pinned to the model byte for byte,
the ISN against hashlib.md5, the option parse and fill against literals, every
argument error of sccsum_tcp_listen and of batch.tcp_listen, the record
layouts, the C++ class, and the coverage of the traffic that
tests/test_gpu_tcp_listen.py runs."""
import ctypes
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import cpp_host
import tcp_listen_fast as fast
import tcp_listen_model as lm
import tcp_listen_traffic as tr
from seastar_amd import batch, native
from tcp_listen_model import ACK, RST, SYN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = native.SCCSUM_EINVAL, native.SCCSUM_ENODEV
NAMES = ("cls", "new", "synack", "sa_off", "sa_len", "sa_out", "rst", "rst_dst", "total")
# the interface's words for the model's: every test here is about that interface
assert (native.TCP_LISTEN_NEW, native.TCP_LISTEN_RESET, native.TCP_LISTEN_DROP, native.TCP_LISTEN_LATER) == \
    (lm.NEW, lm.RESET, lm.DROP, lm.LATER)


def test_symbols_constants_and_layouts(tmp_path):
    lib = native.load()
    declared = native.header_symbols()
    for s in ("sccsum_tcp_listen", "sccsum_tcp_listen_workspace"):
        assert s in declared and s in native._PROTOS and getattr(lib, s).argtypes is not None
    assert lib.sccsum_abi_version() == native.ABI_VERSION == 4
    assert native._PROTOS["sccsum_tcp_listen"][1][0] is native.TcpListenOpts
    assert os.path.join(REPO, "seastar_amd", "csrc", "tcp_listen.hip") in __import__("seastar_amd.build").build.SOURCES
    header = open(native.HEADER_PATH).read()
    for name, value, model in (("LISTEN_NEW", native.TCP_LISTEN_NEW, lm.NEW), ("LISTEN_RESET", native.TCP_LISTEN_RESET, lm.RESET),
                               ("LISTEN_DROP", native.TCP_LISTEN_DROP, lm.DROP), ("LISTEN_LATER", native.TCP_LISTEN_LATER, lm.LATER),
                               ("NEW_MSS", native.TCP_NEW_MSS, lm.F_MSS), ("NEW_WSCALE", native.TCP_NEW_WSCALE, lm.F_WSCALE),
                               ("NEW_SACK", native.TCP_NEW_SACK, lm.F_SACK),
                               ("NEW_WSCALE_BIG", native.TCP_NEW_WSCALE_BIG, lm.F_BIG)):
        assert value == model
        assert int(header.split(f"#define SCCSUM_TCP_{name} ")[1].split()[0].rstrip("u"), 0) == value, name
    assert native.TCP_LISTEN_MAX == 1 << 30 and native.TCP_RCV_WINDOW == lm.RCV_WINDOW == 29200
    assert batch.TCP_NEW_DTYPE == lm.NEW_DTYPE and batch.TCP_OUT_DTYPE == lm.OUT_DTYPE
    assert ctypes.sizeof(native.TcpNew) == 64 and ctypes.sizeof(native.TcpListenOpts) == 76
    opts_dt = np.dtype([("isn_key", "<u4", (16,)), ("isn_m", "<u4"), ("mtu", "<u4"), ("flags", "<u4")])
    structs = (("sccsum_tcp_new", lm.NEW_DTYPE, native.TcpNew, 64), ("sccsum_tcp_listen_opts", opts_dt, native.TcpListenOpts, 76))
    lines = []
    for cname, dt, _, _ in structs:
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in dt.names]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <sccsum.h>\nint main(void) {\n"
                   + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    for cname, dt, ct, size in structs:
        assert int(got[cname]) == dt.itemsize == size
        assert [f for f, _ in ct._fields_] == list(dt.names)
        for f in dt.names:
            assert int(got[f"{cname}.{f}"]) == dt.fields[f][1] == getattr(ct, f).offset, (cname, f)


# ---------------------------------------------------------------- the model on buckets written out by hand

def _both(segs, space, offload=False, strict=False) -> dict:
    """The model's arrays, and the numpy restatement's, byte for byte."""
    want = lm.expect(segs, space, tr.KEY, tr.ISN_M, tr.MTU, offload, strict)
    got = fast.expect(tr.arrays(segs, seed=len(segs)), tr.space_array(space), tr.KEY, tr.ISN_M, tr.MTU, offload)
    for name in NAMES:
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    return want


def test_every_row_of_the_table():
    segs, space, classes = tr.table_case()
    assert len(segs) <= 64 and sorted(space.values()) == [0, 1, 3, 5]
    for offload in (True, False):
        w = _both(segs, space, offload, strict=True)
        assert w["cls"].tolist() == classes
        assert w["total"].tolist() == [len(segs), classes.count(lm.NEW), classes.count(lm.RESET), classes.count(lm.DROP)]
    branches = w["walk"]["branches"]
    assert set(branches) == set(lm.BRANCH_CLASS)                      # every branch of tcp.hh:888-929
    # the listener's counter moved once per created tcb, and a full one refuses
    st = w["walk"]["stack"]
    assert {p: li.pending for p, li in st.listening.items()} == {80: 1, 81: 3, 82: 0, 83: 2}
    assert st.listening[80].full() and st.listening[81].full() and st.listening[82].full() and not st.listening[83].full()
    # a reset's bytes, written out: SYN to the full port 82 from peer 0 (seq 1000): <SEQ=0><ACK=1001><CTL=RST,ACK>
    first = bytes(w["rst"][:20])
    assert first[:16] == struct.pack(">HHIIBBH", 82, 1024, 0, 1001, 0x50, 0x14, 0) and w["rst_dst"][0] == tr.PEER
    assert lm.tm.ones_sum(first, lm.tm.pseudo_sum(tr.HOST, tr.PEER, 20)) == 0xFFFF


@pytest.mark.parametrize("name", sorted(tr.duplicate_cases()))
def test_duplicate_connids(name):
    segs, space, taken, classes = tr.duplicate_cases()[name]
    w = _both(segs, space, strict=True)
    assert int(w["total"][0]) == taken and w["cls"].tolist() == classes + [lm.LATER] * (len(segs) - taken)
    if taken < len(segs):
        # the stop is where the reference's walk meets a tcb made by this batch
        assert w["walk"]["stack"].received(segs[taken]) == "tcb"


def test_option_layouts_and_the_parse_against_literals():
    segs, space, names = tr.option_case()
    tr.check_strict(segs, names)
    w = _both(segs, space)
    assert int(w["total"][1]) == len(segs)
    got = {n: (int(r["snd_mss"]), int(r["snd_wscale"]), int(r["rcv_wscale"]), int(r["flags"])) for n, r in zip(names, w["new"])}
    M, W, S, B = lm.F_MSS, lm.F_WSCALE, lm.F_SACK, lm.F_BIG
    assert got["none"] == (536, 0, 0, 0) and got["mss"] == (1460, 0, 0, M) and got["ws"] == (536, 7, 7, W)
    assert got["both"] == (1460, 2, 7, M | W) and got["both_reversed"] == (9000, 9, 7, M | W)
    assert got["linux"] == got["forty"] == (1460, 7, 7, M | W | S) and got["sack_only"] == (536, 0, 0, S)
    assert got["timestamp"] == (1200, 0, 0, M) and got["unknown_kinds"] == (700, 3, 7, M | W)
    assert got["length_0"] == (536, 0, 0, 0) and got["length_0_mss"] == (1460, 0, 0, M)
    assert got["length_1_ws"] == (536, 5, 7, W) and got["overrun"] == (1400, 0, 0, M)
    assert got["overrun_mss"] == (536, 1, 7, W) and got["eol_in_the_middle"] == (1000, 0, 0, M)
    assert got["sack_advance"] == (1460, 0, 0, M | S) and got["forty_unknown"] == (536, 0, 0, 0)
    assert got["repeated"] == (200, 2, 7, M | W) and got["mss_0"] == (0, 0, 0, M)
    # where the reference would read past opt_end, what was parsed before stays
    assert got["kind_last"] == got["sack_last"] == got["ws_value_cut"] == (1300, 0, 0, M)
    assert got["kind_last_mss"] == got["mss_value_cut"] == got["mss_value_cut_2"] == (536, 6, 7, W)
    assert got["shift_14"] == (536, 14, 7, W) and got["shift_15"] == (536, 15, 7, W | B)
    rec = dict(zip(names, w["new"]))
    assert [int(rec[f"mss_{v}"]["cwnd"]) for v in tr.MSS_VALUES] == [4 * 536, 4 * 1095, 3 * 1096, 3 * 2190, 2 * 2191]
    assert int(rec["shift_14"]["snd_window"]) == int(rec["shift_14"]["ssthresh"]) == 3 << 14
    assert int(rec["shift_15"]["snd_window"]) == int(rec["shift_15"]["ssthresh"]) == 0xFFFF   # unshifted
    assert names.index("mss_65535_ws_14") % 2 == 1 and int(rec["mss_65535_ws_14"]["snd_window"]) == 0xFFFF << 14
    assert int(rec["ws"]["rcv_window"]) == 29200 << 7 and int(rec["mss"]["rcv_window"]) == 29200
    # tcp_option::fill for SYN|ACK, and the record tcp_send takes
    mss = bytes([2, 4, 1460 >> 8, 1460 & 0xFF])
    staged = {n: (bytes(s), int(o["hdr_len"])) for n, s, o in zip(names, w["synack"], w["sa_out"])}
    assert staged["none"] == (bytes(12), 20) and staged["mss"] == (mss + bytes([1, 1, 1, 0]) + bytes(4), 28)
    assert staged["ws"] == (bytes([3, 3, 7, 0]) + bytes(8), 24) and staged["both"] == (mss + bytes([3, 3, 7, 0]) + bytes(4), 28)
    k = names.index("both")
    o, r = w["sa_out"][k], w["new"][k]
    assert (o["dst"], o["seq"], o["ack"], o["sport"], o["dport"], o["window"], o["flags"], o["mss"]) == \
        (r["foreign_ip"], r["iss"], (int(r["irs"]) + 1) & lm.M32, 80, r["foreign_port"], 29200, 0x12, 1460)
    assert w["sa_off"].tolist() == [32 * j + int(h) for j, h in enumerate(w["sa_out"]["hdr_len"])]
    with pytest.raises(lm.PastEnd):
        lm.parse(tr.OPTION_LAYOUTS["kind_last"], strict=True)


def test_isn_against_hashlib_md5():
    key = bytes(range(64))
    # one digest written out: MD5 of twelve zero bytes and the key 00 01 .. 3f
    assert hashlib.md5(bytes(12) + key).hexdigest() == hashlib.md5(struct.pack("<III", 0, 0, 0) + key).hexdigest()
    vectors = [(0, 0, 0, 0), (tr.HOST, tr.PEER, 80, 1024), (0xFFFFFFFF, 0xFFFFFFFF, 65535, 65535), (1, 2, 3, 4),
               (0x0A000001, 0x0A000002, 65535, 1), (0x80000000, 0x7FFFFFFF, 32768, 32767)]
    for isn_m in (0, 1, 0xFFFFFFFF, tr.ISN_M):
        for k in (key, tr.KEY, bytes(64), b"\xff" * 64):
            cols = [np.array(c, dtype=np.int64) for c in zip(*vectors)]
            got = fast.isn(*cols, k, isn_m).tolist()
            for v, g in zip(vectors, got):
                lip, fip, lp, fp = v
                msg = struct.pack("<III", lip, fip, ((lp << 16) + fp) & lm.M32) + k
                assert len(msg) == 76
                want = (int.from_bytes(hashlib.md5(msg).digest()[:4], "little") + isn_m) & lm.M32
                assert g == want == lm.get_isn(v, k, isn_m), (v, isn_m)
    assert fast._K[0] == 0xD76AA478 and fast._K[63] == 0xEB86D391


@pytest.mark.parametrize("m", [1, 63, tr.TILE - 1, tr.TILE, tr.TILE + 1, 2 * tr.TILE + 7])
def test_the_restatement_equals_the_model_on_seeded_buckets(m):
    segs, space = tr.mixed(m % 5, m)
    w = _both(segs, space, offload=bool(m % 2), strict=True)
    assert int(w["total"][0]) == m
    if m > 1000:
        t = w["total"].tolist()
        assert t[1] > m // 4 and t[2] > m // 4 and t[3] > m // 20          # created, reset and dropped all occur
        assert len({bytes(s) for s in w["synack"]}) == 4                    # every SYN-ACK form


def test_traffic_coverage():
    """What the GPU tests run, under the model alone."""
    segs, space = tr.mixed(1, 2 * tr.TILE + 7, stop_at=1500)
    w = _both(segs, space, strict=True)
    assert w["total"].tolist()[0] == 1500 and w["cls"][1500:].tolist() == [lm.LATER] * (len(segs) - 1500)
    repeats = len(segs) - len({s.connid for s in segs})
    assert repeats > 20                                                    # refused connids come again without a stop
    segs, space = tr.many_ports(0)
    w = _both(segs, space, strict=True)
    assert w["total"].tolist() == [1200, 900, 300, 0]
    segs, space = tr.colliding(64)
    bits = tr.table_bits(64)
    assert bits == 7 and len(segs) <= 64
    lib = native.load()
    homes = [lib.sccsum_tcp_conns_slot(*s.connid, bits) for s in segs]
    assert homes == [tr.slot(s.connid, bits) for s in segs]
    distinct = {s.connid: h for s, h in zip(segs, homes)}
    assert sorted(distinct.values()).count(126) == 10 and sorted(distinct.values()).count(0) == 6   # the run wraps past slot 127
    w = _both(segs, space, strict=True)
    assert int(w["total"][0]) == len(segs) - 1 and int(w["total"][1]) > 5
    for m_max, want in ((0, 4), (1, 4), (8, 4), (9, 5), (64, 7), (65, 8), (1 << 18, 19), ((1 << 18) + 1, 20)):
        assert tr.table_bits(m_max) == want


# ---------------------------------------------------------------- argument errors

def _opts(mtu=1500, flags=0):
    return native.TcpListenOpts((ctypes.c_uint32 * 16)(*range(16)), 5, mtu, flags)


def test_c_call_argument_errors_without_device():
    lib = native.load()
    p = 0x10000

    def call(opts=None, data=p, bytes_len=4096, off=p, nbatch=64, first=p, order=p, seg=p, src=p, m_max=64, space=p, cls=p + 1,
             rec=p, synack=p + 4, sa_off=p + 8, sa_len=p + 4, sa_out=p + 4, rst=p + 4, rst_dst=p + 4, total=p + 8, ws=p):
        return lib.sccsum_tcp_listen(opts or _opts(), data, bytes_len, off, nbatch, first, order, seg, src, m_max, space, cls,
                                     rec, synack, sa_off, sa_len, sa_out, rst, rst_dst, total, ws, None)

    if not torch.cuda.is_available():  # valid arguments get as far as the device
        assert call() == ENODEV
        assert call(data=None, bytes_len=0) == ENODEV and call(off=None, nbatch=0) == ENODEV
        assert call(m_max=0, first=None, order=None, seg=None, src=None, space=None, cls=None, rec=None, synack=None,
                    sa_off=None, sa_len=None, sa_out=None, rst=None, rst_dst=None) == ENODEV
        assert call(m_max=1 << 30, nbatch=0xFFFFFFFF) == ENODEV
        assert call(opts=_opts(68, native.TCP_CSUM_OFFLOAD)) == ENODEV and call(opts=_opts(65535)) == ENODEV
    for bad in (dict(data=None), dict(off=None), dict(off=p + 4), dict(first=None), dict(first=p + 2), dict(order=None),
                dict(order=p + 1), dict(seg=None), dict(seg=p + 4), dict(src=None), dict(src=p + 2), dict(space=None),
                dict(space=p + 2), dict(cls=None), dict(rec=None), dict(rec=p + 8), dict(synack=None), dict(synack=p + 2),
                dict(sa_off=None), dict(sa_off=p + 4), dict(sa_len=None), dict(sa_len=p + 2), dict(sa_out=None),
                dict(sa_out=p + 2), dict(rst=None), dict(rst=p + 1), dict(rst_dst=None), dict(rst_dst=p + 2), dict(total=None),
                dict(total=p + 4), dict(ws=None), dict(ws=p + 8), dict(m_max=(1 << 30) + 1), dict(nbatch=1 << 32),
                dict(opts=_opts(67)), dict(opts=_opts(65536)), dict(opts=_opts(1500, native.TCP_TSO)), dict(opts=_opts(1500, 4)),
                dict(m_max=0, total=None), dict(m_max=0, ws=None), dict(m_max=0, opts=_opts(0))):
        assert call(**bad) == EINVAL, bad
    before = 0
    for m in (0, 1, 1023, 1025, 1 << 18, 1 << 20):
        w = lib.sccsum_tcp_listen_workspace(m)
        assert w % 16 == 0 and before < w <= (1 << 20) + 80 * m
        before = w
    assert lib.sccsum_tcp_listen_workspace((1 << 30) + 1) == 0


def _rx(n=6, dev="cpu") -> batch.TcpRxResult:
    z32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)   # noqa: E731
    return batch.TcpRxResult(source=None, order=z32(n), first=z32(5), seg=torch.zeros((n, 32), dtype=torch.uint8, device=dev),
                             src_all=z32(n), run_conn=z32(1), run_first=z32(1), rst=z32(1), rst_dst=z32(n),
                             total=torch.zeros(4, dtype=torch.int64, device=dev), cls=None)


def test_python_wrapper_validation():
    b = batch.PacketBatch(data=torch.zeros(64, dtype=torch.uint8), off=torch.zeros(6, dtype=torch.int64),
                          length=torch.zeros(6, dtype=torch.int32), bytes_len=64, max_len=0)
    good = dict(rx=_rx(), b=b, space={80: 3, 65535: 0}, key=bytes(64), isn_m=7, mtu=1500, flags=0)
    words = tuple([0] * 16)
    assert batch.tcp_listen_check(**good) == (6, 6, words)
    assert batch.tcp_listen_check(**dict(good, m_max=2, key=list(range(16)))) == (2, 6, tuple(range(16)))
    assert batch.tcp_listen_check(**dict(good, space=torch.zeros(65536, dtype=torch.int32), isn_m=0xFFFFFFFF,
                                         flags=native.TCP_CSUM_OFFLOAD, mtu=68)) == (6, 6, words)
    assert batch._isn_key(bytes(range(64)))[:2] == (0x03020100, 0x07060504)
    for name, kw in (("rx", dict(rx=None)), ("b", dict(b=None)), ("m_max", dict(m_max=7)), ("m_max", dict(m_max=-1)),
                     ("space", dict(space=None)), ("space", dict(space={65536: 1})), ("space", dict(space={80: -1})),
                     ("space", dict(space={80: 1 << 32})), ("space", dict(space=torch.zeros(65535, dtype=torch.int32))),
                     ("space", dict(space=torch.zeros(65536, dtype=torch.int64))),
                     ("space", dict(space=torch.zeros((2, 32768), dtype=torch.int32))),
                     ("space", dict(space=torch.zeros(131072, dtype=torch.int32)[::2])),
                     ("key", dict(key=bytes(63))), ("key", dict(key=[0] * 15)), ("key", dict(key=[1 << 32] * 16)),
                     ("isn_m", dict(isn_m=1 << 32)), ("isn_m", dict(isn_m=-1)), ("mtu", dict(mtu=67)),
                     ("mtu", dict(mtu=65536)), ("flags", dict(flags=native.TCP_TSO))):
        with pytest.raises(ValueError, match=name):
            batch.tcp_listen_check(**dict(good, **kw))
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="b:"):        # the frames live where the records do
            batch.tcp_listen_check(**dict(good, rx=_rx(dev="cuda:0")))


# ---------------------------------------------------------------- the C++ class

def test_cpp_class_on_the_host(tmp_path):
    """seastar::net::tcp_listen (tests/cpp/tcp_listen_host.cc): workspace() and
    the argument errors of the call, through the class and directly."""
    cpp_host.build_and_run(tmp_path, "tcp_listen_host", "tcp_listen_host: OK")


def test_cpp_class_on_the_host_sanitized(tmp_path):
    """The same stand-alone program with tcp_listen.hip itself compiled in, its
    host side under AddressSanitizer + UndefinedBehaviorSanitizer (device code
    is not instrumented): the workspace layout and the argument checks."""
    cpp_host.build_and_run_sanitized(tmp_path, "tcp_listen_host", "tcp_listen.hip", "tcp_listen_host: OK")
