"""The TCP transmit fast path without a GPU: the per-segment model and the
closed form pinned on connections written out by hand, the capacity rule,
every argument error of sccsum_tcp_tx_data and of batch.tcp_tx_data, the
record layouts, the C++ class, and the coverage of the traffic that
tests/test_gpu_tcp_tx_data.py runs."""
import copy
import os
import subprocess

import numpy as np
import pytest
import torch

import cpp_host
import tcp_tx_fast as fast
import tcp_tx_model as tm
import tcp_tx_traffic as tr
from seastar_amd import batch, native
from tcp_tx_model import Hw, Tcb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = native.SCCSUM_EINVAL, native.SCCSUM_ENODEV


def test_symbols_constants_and_layouts(tmp_path):
    lib = native.load()
    declared = native.header_symbols()
    for s in ("sccsum_tcp_tx_data", "sccsum_tcp_tx_data_workspace", "sccsum_tcp_tx_data_seg_tile",
              "sccsum_tcp_tx_data_max_blocks"):
        assert s in declared and s in native._PROTOS and getattr(lib, s).argtypes is not None
    assert os.path.join(REPO, "seastar_amd", "csrc", "tcp_tx_data.hip") in __import__("seastar_amd.build").build.SOURCES
    header = open(native.HEADER_PATH).read()
    for name, value, model in (("SND_ELIGIBLE", native.TCP_SND_ELIGIBLE, tm.ELIGIBLE),
                               ("SND_RTX_ARMED", native.TCP_SND_RTX_ARMED, tm.RTX_ARMED),
                               ("SND_RTX_ARM", native.TCP_SND_RTX_ARM, tm.RTX_ARM),
                               ("STOP_END", native.TCP_STOP_END, tm.STOP_END),
                               ("STOP_INELIGIBLE", native.TCP_STOP_INELIGIBLE, tm.STOP_INELIGIBLE),
                               ("STOP_WINDOW", native.TCP_STOP_WINDOW, tm.STOP_WINDOW),
                               ("STOP_CAPACITY", native.TCP_STOP_CAPACITY, tm.STOP_CAPACITY),
                               ("STOP_QUEUE", native.TCP_STOP_QUEUE, tm.STOP_QUEUE)):
        assert value == model == getattr(fast, name.split("_", 1)[1] if name.startswith("SND") else name)
        assert int(header.split(f"#define SCCSUM_TCP_{name} ")[1].split()[0].rstrip("u"), 0) == value, name
    assert batch.TCP_SND_DTYPE == tr.SND_DTYPE and batch.TCP_SND_RUN_DTYPE == tr.RUN_DTYPE
    assert batch.TCP_OUT_DTYPE == fast.OUT_DTYPE
    structs = (("sccsum_tcp_snd", tr.SND_DTYPE, 48), ("sccsum_tcp_snd_run", tr.RUN_DTYPE, 32))
    lines = ['    printf("opts %zu %zu %zu\\n", sizeof(sccsum_tcp_tx_opts), offsetof(sccsum_tcp_tx_opts, headroom), '
             'offsetof(sccsum_tcp_tx_opts, flags));']
    for cname, dt, _ in structs:
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in dt.names]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <sccsum.h>\nint main(void) {\n"
                   + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", exe], check=True)
    rows = [line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert rows[0] == ["opts", str(ctypes_size()), "12", "16"]
    got = dict(rows[1:])
    for cname, dt, size in structs:
        assert int(got[cname]) == dt.itemsize == size
        for f in dt.names:
            assert int(got[f"{cname}.{f}"]) == dt.fields[f][1], (cname, f)


def ctypes_size() -> int:
    import ctypes
    return ctypes.sizeof(native.TcpTxOpts)


# ---------------------------------------------------------------- connections written out by hand

def _run(t: Tcb, hw: Hw = Hw(1500)):
    """The loop and the closed form on one tcb; they agree, and the loop's segments come back."""
    r = tm.closed_form(t, hw)
    after = copy.deepcopy(t)
    segs, cut = tm.chain(after, hw, limit=64)
    if not cut:
        assert [s["seq"] for s in segs] == r.seq and [len(s["payload"]) for s in segs] == r.length
        assert after.snd_next == r.next
    return r, segs, after


def _tcb(sizes=(3000,), **kw) -> Tcb:
    t = Tcb(**dict(dict(snd_next=1000, snd_unacknowledged=1000, snd_window=65535, cwnd=14600, mss=1460), **kw))
    return t.queue(bytes([j + 1]) * n for j, n in enumerate(sizes))


def test_one_connection_per_stop():
    r, segs, after = _run(_tcb())                                     # the queue is exhausted
    assert (r.segs, r.bytes, r.next, r.stop, r.flags) == (3, 3000, 4000, tm.STOP_END, tm.RTX_ARM)
    assert r.seq == [1000, 2460, 3920] and r.length == [1460, 1460, 80] and not after.unsent
    r, segs, after = _run(_tcb(snd_window=2000, rtx_armed=True))      # the window closes first
    assert (r.segs, r.bytes, r.stop, r.flags) == (2, 2000, tm.STOP_WINDOW, 0) and r.length == [1460, 540]
    assert b"".join(after.unsent) == bytes([1]) * 1000 and after.unsent_len == 1000
    for t in (_tcb(dupacks=1), _tcb(dupacks=3), _tcb(window_probe=True), _tcb(packetq=1), _tcb(state="FIN_WAIT_1")):
        r = tm.closed_form(t, Hw())
        assert (r.segs, r.bytes, r.next, r.stop, r.flags) == (0, 0, 1000, tm.STOP_INELIGIBLE, 0)
    r = tm.closed_form(_tcb(), Hw(), unsent_len=1 << 32)              # a queue the reference's uint32_t cannot count
    assert (r.segs, r.stop, r.next) == (0, tm.STOP_QUEUE, 1000)
    assert tm.closed_form(_tcb(snd_window=5000), Hw(), unsent_len=tm.M32).stop == tm.STOP_WINDOW
    assert _run(_tcb(state=tm.CLOSE_WAIT))[0].segs == 3


def test_window_against_what_is_in_flight():
    r, segs, _ = _run(_tcb(snd_window=0))                             # a closed window: the pure ACK
    assert (r.segs, r.bytes, r.length, r.stop, r.flags) == (1, 0, [0], tm.STOP_WINDOW, 0) and segs[0]["flags"] == 0x10
    t = _tcb(snd_window=500)
    t.snd_unacknowledged = 1000 - 501                                 # used > window
    assert _run(t)[0].length == [0]
    t.snd_unacknowledged = 1000 - 500                                 # used == window: nothing fits either
    r, _, _ = _run(t)
    assert (r.segs, r.bytes, r.stop) == (1, 0, tm.STOP_WINDOW)
    t.snd_unacknowledged = 1000 - 499                                 # one byte of window left
    r, _, _ = _run(t)
    assert (r.segs, r.bytes, r.length) == (1, 1, [1])
    t = _tcb(snd_window=3000)
    t.snd_unacknowledged = (1000 - 0xFFFFFFFF) & tm.M32               # next - una as a uint32_t
    assert _run(t)[0].length == [0]


def test_cwnd_and_mss_limit_a_segment_not_the_trip():
    r, _, _ = _run(_tcb(cwnd=1000))                                   # can_send() is limited by cwnd at every call
    assert r.length == [1000, 1000, 1000] and r.stop == tm.STOP_END   # ... not by the flight size
    r, segs, after = _run(_tcb(cwnd=0))
    assert (r.segs, r.bytes, r.length, r.stop, r.flags) == (1, 0, [0], tm.STOP_WINDOW, 0) and after.unsent_len == 3000
    t = _tcb(mss=0)                                                   # the reference never stops: one per poll
    r = tm.closed_form(t, Hw())
    segs, cut = tm.chain(copy.deepcopy(t), Hw(), limit=7)
    assert cut and len(segs) == 7 and (r.segs, r.bytes, r.stop) == (1, 0, tm.STOP_WINDOW)
    assert _run(_tcb(mss=0), Hw(1500, True, 65521))[0].length == [3000]   # TSO does not ask the mss


@pytest.mark.parametrize("total,want", [(2919, [1460, 1459]), (2920, [1460, 1460]), (2921, [1460, 1460, 1]),
                                         (1, [1]), (1459, [1459]), (1460, [1460]), (1461, [1460, 1])])
def test_lengths_around_a_multiple_of_the_segment(total, want):
    assert _run(_tcb((total,)))[0].length == want
    assert _run(_tcb((5000,), snd_window=total))[0].length == want


def test_seq_crosses_the_wrap_and_the_pure_ack():
    t = _tcb((4000,))
    t.snd_next = t.snd_unacknowledged = tm.M32 - 1459
    r, _, _ = _run(t)
    assert r.seq == [tm.M32 - 1459, 0, 1460] and r.next == 2540
    r, segs, _ = _run(_tcb(()))                                       # nothing queued: the ACK output() was called for
    assert (r.segs, r.bytes, r.length, r.stop, r.flags) == (1, 0, [0], tm.STOP_END, 0)
    assert (segs[0]["seq"], segs[0]["ack"], segs[0]["payload"], segs[0]["pieces"]) == (1000, 77, b"", [])
    assert _run(_tcb((0, 0)))[0].stop == tm.STOP_END


@pytest.mark.parametrize("sizes,pieces", [
    ((1460, 1460), [[(0, 0, 1460)], [(1, 0, 1460)]]),                            # boundaries on the cuts
    ((1459, 1461), [[(0, 0, 1459), (1, 0, 1)], [(1, 1, 1460)]]),                 # one byte before
    ((1461, 1459), [[(0, 0, 1460)], [(0, 1460, 1), (1, 0, 1459)]]),              # one byte behind
    ((0, 1460, 0, 0, 1460, 0), [[(1, 0, 1460)], [(4, 0, 1460)]]),                # buffers of no bytes are no pieces
    ((1, 0, 1), [[(0, 0, 1), (2, 0, 1)]]),
    ((4000,), [[(0, 0, 1460)], [(0, 1460, 1460)], [(0, 2920, 1080)]]),
    ((700, 700, 700), [[(0, 0, 700), (1, 0, 700), (2, 0, 60)], [(2, 60, 640)]]),
])
def test_pieces_follow_the_deque_walk(sizes, pieces):
    t = _tcb(sizes)
    bufs = list(t.unsent)
    r, segs, _ = _run(t)
    assert [s["pieces"] for s in segs] == pieces
    at = 0
    for s in segs:
        assert tm.pieces_of(bufs, at, len(s["payload"])) == s["pieces"]
        assert s["payload"] == b"".join(bufs[j][i:i + n] for j, i, n in s["pieces"])
        at += len(s["payload"])
    a = tr.arrays([t])
    want = fast.expect(a["snd"], a["buf_len"], a["buf_first"], 1500, 20)
    flat = [p for seg in pieces for p in seg]
    assert want["desc_buf"].tolist() == [p[0] for p in flat] and want["desc_inner"].tolist() == [p[1] for p in flat]
    assert want["desc_len"].tolist() == [p[2] for p in flat]
    assert want["seg_first"].tolist() == np.concatenate([[0], np.cumsum([len(s) for s in pieces])]).tolist()


@pytest.mark.parametrize("hw,mss,want", [
    (Hw(68), 1460, 28), (Hw(576), 1460, 536), (Hw(1500), 1460, 1460), (Hw(9000), 8960, 8960), (Hw(9000), 1460, 1460),
    (Hw(1500), 536, 536), (Hw(65535), 65535, 65495), (Hw(1500, True, 65521), 1460, 65481), (Hw(1500, True, 41), 1460, 1),
])
def test_segment_length_by_mtu_mss_and_tso(hw, mss, want):
    assert hw.seg_len(mss) == want
    t = Tcb(snd_window=1 << 20, cwnd=1 << 20, mss=mss).queue([bytes(3 * want + 1)])
    assert _run(t, hw)[0].length == [want, want, want, 1]
    assert int(fast.seg_len(hw.mtu, hw.tx_tso, hw.max_packet_len, np.array([mss]))[0]) == want


def test_the_cast_of_mtu_minus_the_headers():
    # uint16_t(mtu - 40): inside 68..65535 it changes nothing, and the model takes it as the reference writes it
    assert Hw(65535).seg_len(65535) == 65495 == (65535 - 40) & 0xFFFF and Hw(68).seg_len(65535) == 28
    assert Hw(65576).seg_len(1460) == 0                               # what the cast would do past the range


# ---------------------------------------------------------------- the capacity rule

def test_capacity_is_a_prefix_rule():
    cases = [_tcb((2000,)), _tcb(dupacks=1), _tcb(()), _tcb((100,)), _tcb((3000,)), _tcb((10,))]
    hw = Hw()

    def cut(max_segs, max_bytes):
        w = tr.expect(cases, hw, 20, max_segs, max_bytes)
        return w["run"]["stop"].tolist(), w["run"]["segs"].tolist(), w["total"].tolist()

    end, inel, cap = tm.STOP_END, tm.STOP_INELIGIBLE, tm.STOP_CAPACITY
    need = 2000 + 40 + 20 + 100 + 20 + 3000 + 60 + 10 + 20
    assert cut(8, need) == ([end, inel, end, end, end, end], [2, 0, 1, 1, 3, 1], [8, need, 7, need])   # exactly equal
    assert cut(7, need) == ([end, inel, end, end, end, cap], [2, 0, 1, 1, 3, 0], [7, need - 30, 6, need])
    assert cut(8, need - 1)[0] == [end, inel, end, end, end, cap]
    # a prefix: the small connection behind the one that does not fit is not taken either
    assert cut(6, need) == ([end, inel, end, end, cap, cap], [2, 0, 1, 1, 0, 0], [4, 2180, 3, need])
    assert cut(8, 2180 + 3059)[0] == [end, inel, end, end, cap, cap]
    assert cut(1, need) == ([cap] * 6, [0] * 6, [0, 0, 0, need])       # at the first connection
    assert cut(8, 2039)[0] == [cap] * 6
    assert cut(0, need)[0] == [cap] * 6 and cut(8, 0)[0] == [cap] * 6
    # a connection that is not taken anyway does not open the cut, one behind it is cut all the same
    assert tr.expect(cases[1:2] + cases[:1], hw, 20, 0, 0)["run"]["stop"].tolist() == [inel, cap]
    w = tr.expect(cases, hw, 20, 6, need)
    assert w["run"]["seg_first"].tolist() == [0, 2, 2, 3, 4, 4] and w["run"]["next"][4] == 1000
    assert w["run"]["flags"].tolist() == [tm.RTX_ARM, 0, 0, tm.RTX_ARM, 0, 0]


# ---------------------------------------------------------------- argument errors

def test_c_call_argument_errors_without_device():
    lib = native.load()
    p = 0x10000

    def call(opts=(1, 1500, 65535, 20, 0), snd=p, nconns=4, src=p, length=p, first=p, nbuf=8, max_segs=64,
             max_bytes=1 << 20, run=p, off=p, out_len=p, out=p, seg_first=p, desc=p, total=p, ws=p):
        import ctypes
        o = native.TcpTxOpts(*opts) if opts is not None else None
        return lib.sccsum_tcp_tx_data(None if o is None else ctypes.addressof(o), snd, nconns, src, length, first, nbuf,
                                      max_segs, max_bytes, run, off, out_len, out, seg_first, desc, total, ws, None)

    if not torch.cuda.is_available():  # valid arguments get as far as the device
        assert call() == ENODEV and call(opts=(1, 68, 0, 65535, 0)) == ENODEV
        assert call(opts=(1, 65535, 41, 20, native.TCP_TSO)) == ENODEV
        assert call(nbuf=0, src=None, length=None) == ENODEV
        assert call(max_segs=0, off=None, out_len=None, out=None, desc=None) == ENODEV
        assert call(nconns=0, snd=None, first=None, run=None, src=None, length=None, off=None) == ENODEV
        assert call(nconns=1 << 20, nbuf=1 << 31, max_segs=0x7FFFFFFF, max_bytes=0xFFFFFFFF) == ENODEV
        assert call(snd=p + 16, run=p + 16, out=p + 4, desc=p + 8, off=p + 8) == ENODEV
    for bad in (dict(opts=None), dict(opts=(1, 67, 65535, 20, 0)), dict(opts=(1, 65536, 65535, 20, 0)),
                dict(opts=(1, 1500, 65535, 19, 0)), dict(opts=(1, 1500, 65535, 65536, 0)),
                dict(opts=(1, 1500, 65535, 20, native.TCP_CSUM_OFFLOAD)), dict(opts=(1, 1500, 65535, 20, 4)),
                dict(opts=(1, 1500, 40, 20, native.TCP_TSO)), dict(opts=(1, 1500, 65536, 20, native.TCP_TSO)),
                dict(snd=None), dict(snd=p + 8), dict(src=None), dict(src=p + 4), dict(length=None), dict(length=p + 2),
                dict(first=None), dict(first=p + 2), dict(run=None), dict(run=p + 8), dict(off=None), dict(off=p + 4),
                dict(out_len=None), dict(out_len=p + 1), dict(out=None), dict(out=p + 2), dict(seg_first=None),
                dict(seg_first=p + 2), dict(desc=None), dict(desc=p + 4), dict(total=None), dict(total=p + 4),
                dict(ws=None), dict(ws=p + 8), dict(nconns=(1 << 20) + 1), dict(nbuf=(1 << 31) + 1),
                dict(max_segs=1 << 31), dict(max_bytes=1 << 32), dict(nconns=0, total=None),
                dict(nconns=0, seg_first=None), dict(nconns=0, ws=None)):
        assert call(**bad) == EINVAL, bad
    before = 0
    for nconns, nbuf in ((0, 0), (1, 0), (1, 1), (1024, 1025), (1025, 1 << 20), (1 << 20, 1 << 22)):
        w = lib.sccsum_tcp_tx_data_workspace(nconns, nbuf)
        assert w % 16 == 0 and before < w <= 256 + 25 * nconns + 13 * nbuf   # per connection and buffer, none per segment
        before = w
    assert lib.sccsum_tcp_tx_data_seg_tile() == 1024 and lib.sccsum_tcp_tx_data_max_blocks() == 1024


def test_python_wrapper_validation():
    snd = torch.zeros((5, 48), dtype=torch.uint8)
    src, length = torch.zeros(7, dtype=torch.int64), torch.zeros(7, dtype=torch.int32)
    first = torch.zeros(6, dtype=torch.int32)
    good = dict(snd=snd, buf_src=src, buf_len=length, buf_first=first, src_host=1, mtu=1500, headroom=20, flags=0,
                max_packet_len=65535, max_segs=100, max_out_bytes=1 << 20)
    assert batch.tcp_tx_data_check(**good) == (5, 7)
    assert batch.tcp_tx_data_check(**dict(good, snd=snd[:0], buf_first=first[:1])) == (0, 7)
    assert batch.tcp_tx_data_check(**dict(good, max_packet_len=0, max_segs=0, max_out_bytes=0)) == (5, 7)
    assert batch.tcp_tx_data_check(**dict(good, flags=native.TCP_TSO, max_packet_len=41, headroom=65535)) == (5, 7)
    for name, kw in (("snd", dict(snd=None)), ("snd", dict(snd=torch.zeros(240, dtype=torch.uint8))),
                     ("snd", dict(snd=torch.zeros((5, 12), dtype=torch.int32))),
                     ("snd", dict(snd=torch.zeros((5, 96), dtype=torch.uint8)[:, ::2])),
                     ("snd", dict(snd=torch.zeros(5 * 48 + 16, dtype=torch.uint8)[8:8 + 240].view(5, 48))),
                     ("snd", dict(snd=torch.zeros((5, 32), dtype=torch.uint8))),
                     ("buf_src", dict(buf_src=None)), ("buf_src", dict(buf_src=src.to(torch.int32))),
                     ("buf_src", dict(buf_src=torch.zeros(14, dtype=torch.int64)[::2])),
                     ("buf_src", dict(buf_src=src.view(1, 7))),
                     ("buf_len", dict(buf_len=length.to(torch.int64))), ("buf_len", dict(buf_len=length[:6])),
                     ("buf_first", dict(buf_first=first[:5])), ("buf_first", dict(buf_first=first.to(torch.int64))),
                     ("buf_first", dict(buf_first=None)),
                     ("mtu", dict(mtu=67)), ("mtu", dict(mtu=65536)), ("headroom", dict(headroom=19)),
                     ("headroom", dict(headroom=65536)), ("flags", dict(flags=native.TCP_CSUM_OFFLOAD)),
                     ("max_packet_len", dict(flags=native.TCP_TSO, max_packet_len=40)),
                     ("max_packet_len", dict(flags=native.TCP_TSO, max_packet_len=65536)),
                     ("src_host", dict(src_host=-1)), ("src_host", dict(src_host=1 << 32)),
                     ("max_segs", dict(max_segs=-1)), ("max_segs", dict(max_segs=1 << 31)),
                     ("max_out_bytes", dict(max_out_bytes=-1)), ("max_out_bytes", dict(max_out_bytes=1 << 32))):
        with pytest.raises(ValueError, match=name):
            batch.tcp_tx_data_check(**dict(good, **kw))
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="buf_len"):   # every array lives where the records do
            batch.tcp_tx_data_check(**dict(good, snd=snd.cuda(), buf_src=src.cuda(), buf_first=first.cuda()))


# ---------------------------------------------------------------- what the GPU tests run

def test_traffic_coverage():
    """The mixed traffic of the GPU tests, under the model alone: every stop
    occurs (the capacity one under a cap), every kind of connection, and 30 %
    to 90 % of the connections are eligible."""
    cases = tr.mixed(0, 2 * tr.TILE + 7)
    hw = Hw(1500)
    runs = [tm.closed_form(t, hw) for t in cases]
    stops = {r.stop for r in runs}
    assert stops == {tm.STOP_END, tm.STOP_WINDOW, tm.STOP_INELIGIBLE}
    share = sum(1 for t in cases if t.flags() & tm.ELIGIBLE) / len(cases)
    assert 0.3 <= share <= 0.9, share
    assert {t.why_not_eligible() for t in cases} == {None, "state", "limited_transmit", "fast_retransmit", "window_probe",
                                                    "packetq"}
    want = tr.expect(cases, hw, 20, max_segs=int(sum(r.segs for r in runs)) // 2)
    assert set(want["run"]["stop"].tolist()) == stops | {tm.STOP_CAPACITY}
    a = tr.arrays(cases)
    big = a["buf_len"].copy()
    k = int(np.flatnonzero(((a["snd"]["flags"] & 1) != 0) & (np.diff(a["buf_first"].astype(np.int64)) >= 2))[5])
    big[a["buf_first"][k]:a["buf_first"][k + 1]] = 0xFFFFFFFF
    assert fast.expect(a["snd"], big, a["buf_first"], 1500, 20)["run"]["stop"][k] == tm.STOP_QUEUE
    assert any(r.segs == 1 and r.bytes == 0 for r in runs) and any(r.segs > 3 for r in runs)      # pure ACKs, long trips
    assert any(r.next < t.snd_next and r.bytes for t, r in zip(cases, runs))                       # seq crosses 2^32
    assert any(0 in [len(b) for b in t.unsent] and r.bytes for t, r in zip(cases, runs))           # empty buffers
    assert any(r.flags & tm.RTX_ARM for r in runs) and any(r.bytes and not r.flags for r in runs)
    assert (want["seg_first"][1:] - want["seg_first"][:-1]).max() > 3                              # many pieces in one


# ---------------------------------------------------------------- the C++ class

def test_cpp_class_on_the_host(tmp_path):
    """seastar::net::tcp_tx_data (tests/cpp/tcp_tx_data_host.cc): workspace()
    and the argument errors of the call, through the class and directly."""
    cpp_host.build_and_run(tmp_path, "tcp_tx_data_host", "tcp_tx_data_host: OK")


def test_cpp_class_on_the_host_sanitized(tmp_path):
    """The same stand-alone program with tcp_tx_data.hip itself compiled in,
    its host side under AddressSanitizer + UndefinedBehaviorSanitizer (device
    code is not instrumented): the workspace layout and the argument checks."""
    cpp_host.build_and_run_sanitized(tmp_path, "tcp_tx_data_host", "tcp_tx_data.hip", "tcp_tx_data_host: OK")
