"""The TCP receive fast path without a GPU: the per-segment model pinned on
runs written out by hand, the capacity rule's arithmetic, every argument
error of sccsum_tcp_rx_data and of batch.tcp_rx_data, the record layouts, and
the coverage of the traffic that tests/test_gpu_tcp_data.py runs."""
import copy
import os
import subprocess

import numpy as np
import pytest
import torch

import cpp_host
import tcp_data_model as dm
import tcp_data_traffic as tr
from seastar_amd import batch, native
from tcp_data_model import ACK, FIN, PSH, RST, SYN, URG, Tcb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = native.SCCSUM_EINVAL, native.SCCSUM_ENODEV


def test_symbols_constants_and_layouts(tmp_path):
    lib = native.load()
    declared = native.header_symbols()
    for s in ("sccsum_tcp_rx_data", "sccsum_tcp_rx_data_workspace"):
        assert s in declared and s in native._PROTOS and getattr(lib, s).argtypes is not None
    assert os.path.join(REPO, "seastar_amd", "csrc", "tcp_data.hip") in __import__("seastar_amd.build").build.SOURCES
    header = open(native.HEADER_PATH).read()
    for name, value, model in (("RCV_ELIGIBLE", native.TCP_RCV_ELIGIBLE, dm.ELIGIBLE),
                               ("RCV_NR_FULL", native.TCP_RCV_NR_FULL, dm.NR_FULL),
                               ("RCV_ACK_ARMED", native.TCP_RCV_ACK_ARMED, dm.ACK_ARMED),
                               ("RCV_ACK_REARMED", native.TCP_RCV_ACK_REARMED, dm.ACK_REARMED),
                               ("RCV_ACK_NOW", native.TCP_RCV_ACK_NOW, dm.ACK_NOW),
                               ("STOP_END", native.TCP_STOP_END, dm.STOP_END),
                               ("STOP_INELIGIBLE", native.TCP_STOP_INELIGIBLE, dm.STOP_INELIGIBLE),
                               ("STOP_WINDOW", native.TCP_STOP_WINDOW, dm.STOP_WINDOW),
                               ("STOP_SEQ", native.TCP_STOP_SEQ, dm.STOP_SEQ),
                               ("STOP_FLAGS", native.TCP_STOP_FLAGS, dm.STOP_FLAGS),
                               ("STOP_ACK", native.TCP_STOP_ACK, dm.STOP_ACK),
                               ("STOP_EMPTY", native.TCP_STOP_EMPTY, dm.STOP_EMPTY),
                               ("STOP_CAPACITY", native.TCP_STOP_CAPACITY, dm.STOP_CAPACITY)):
        assert value == model
        assert int(header.split(f"#define SCCSUM_TCP_{name} ")[1].split()[0].rstrip("u"), 0) == value, name
    assert batch.TCP_RCV_DTYPE == tr.RCV_DTYPE and batch.TCP_RCV_RUN_DTYPE == tr.RUN_DTYPE
    assert batch.TCP_SEG_DTYPE == tr.SEG_DTYPE and batch.DESC_DTYPE == tr.DESC_DTYPE
    structs = (("sccsum_tcp_rcv", tr.RCV_DTYPE), ("sccsum_tcp_rcv_run", tr.RUN_DTYPE))
    lines = []
    for cname, dt in structs:
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in dt.names]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <sccsum.h>\nint main(void) {\n"
                   + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    for cname, dt in structs:
        assert int(got[cname]) == dt.itemsize == 32
        for f in dt.names:
            assert int(got[f"{cname}.{f}"]) == dt.fields[f][1], (cname, f)


# ---------------------------------------------------------------- the model on runs written out by hand

def _tcb(**kw) -> Tcb:
    t = Tcb(rcv_next=1000, rcv_window=29200, max_receive_buf_size=100000, mss=1000, snd_unacknowledged=500,
            snd_next=900, snd_window=4000)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _seg(seq, length, flags=ACK, ack=500, window=100, off=0) -> dict:
    return dict(pay_off=off, pay_len=length, seq=seq, ack=ack, flags=flags, window=window, sport=1, dport=2, hdr_len=20)


def _walk(t, segs):
    return dm.walk(t, segs)


def test_model_straight_run_and_every_field():
    r = _walk(_tcb(), [_seg(1000, 10, off=7), _seg(1010, 20, ACK | PSH, off=50), _seg(1030, 5, ACK | 0x40 | 0x80)])
    assert (r.taken, r.bytes, r.next, r.room, r.window, r.stop) == (3, 35, 1035, 99965, 29200, dm.STOP_END)
    assert r.data == [(7, 10), (50, 20), (0, 5)] and r.branches == []
    assert r.flags == dm.ACK_ARMED | dm.ACK_REARMED        # short segments: the timer armed once, no ACK yet


@pytest.mark.parametrize("segs,tcb,taken,stop,branch", [
    ([_seg(1000, 10)], dict(established=False), 0, dm.STOP_INELIGIBLE, "premise"),
    ([_seg(1000, 10)], dict(out_of_order_empty=False), 0, dm.STOP_INELIGIBLE, "premise"),
    ([_seg(1000, 10)], dict(snd_window=0), 0, dm.STOP_INELIGIBLE, "premise"),
    ([_seg(1000, 10)], dict(snd_unacknowledged=901), 0, dm.STOP_INELIGIBLE, "premise"),
    ([_seg(1000, 10)], dict(rcv_window=0), 0, dm.STOP_WINDOW, "zero_window"),
    ([_seg(1000, 0)], dict(rcv_window=0), 0, dm.STOP_EMPTY, "empty"),          # acceptable: SEG.SEQ = RCV.NXT
    ([_seg(1001, 0)], dict(rcv_window=0), 0, dm.STOP_SEQ, "unacceptable"),
    ([_seg(1000, 10), _seg(1011, 10)], {}, 1, dm.STOP_SEQ, "out_of_order"),
    ([_seg(1000, 10), _seg(1000, 10)], {}, 1, dm.STOP_SEQ, "unacceptable"),     # a duplicate: all of it is old
    ([_seg(1000, 10), _seg(1000, 11)], {}, 1, dm.STOP_SEQ, "trim"),             # ... with one new byte behind
    ([_seg(1000, 10), _seg(1005, 10)], {}, 1, dm.STOP_SEQ, "trim"),             # a retransmission overlapping next
    ([_seg(1000, 10), _seg(990, 10)], {}, 1, dm.STOP_SEQ, "unacceptable"),      # entirely old
    ([_seg(1000, 10), _seg(1010 + 29200, 10)], {}, 1, dm.STOP_SEQ, "unacceptable"),
    ([_seg(1000, 10, ACK | FIN)], {}, 0, dm.STOP_FLAGS, "fin"),
    ([_seg(1000, 10, ACK | SYN)], {}, 0, dm.STOP_FLAGS, "syn"),
    ([_seg(1000, 10, ACK | RST)], {}, 0, dm.STOP_FLAGS, "rst"),
    ([_seg(1000, 10, ACK | URG)], {}, 0, dm.STOP_FLAGS, "urg"),
    ([_seg(1000, 10, PSH)], {}, 0, dm.STOP_FLAGS, "no_ack"),
    ([_seg(1000, 10, ACK | FIN, ack=600)], {}, 0, dm.STOP_FLAGS, "fin"),        # FLAGS is tested before ACK
    ([_seg(1000, 10, ack=501)], {}, 0, dm.STOP_ACK, "ack_advances"),
    ([_seg(1000, 10, ack=900)], {}, 0, dm.STOP_ACK, "ack_advances"),
    ([_seg(1000, 10, ack=901)], {}, 0, dm.STOP_ACK, "ack_beyond"),
    ([_seg(1000, 10, ack=499)], {}, 0, dm.STOP_ACK, "ack_old"),
    ([_seg(1000, 10), _seg(1010, 0)], {}, 1, dm.STOP_EMPTY, "empty"),
    ([_seg(1000, 10), _seg(1010, 0, window=4000)], dict(snd_data_empty=False), 1, dm.STOP_EMPTY, "dup_ack"),
    ([_seg(0xFFFFFFF0, 0x20), _seg(0x10, 5)], dict(rcv_next=0xFFFFFFF0), 2, dm.STOP_END, None),
])
def test_model_one_run_per_stop(segs, tcb, taken, stop, branch):
    t = _tcb(**tcb)
    before = copy.deepcopy(t)
    r = _walk(t, copy.deepcopy(segs))
    assert (r.taken, r.stop) == (taken, stop)
    assert (branch in r.branches) if branch else not r.branches
    if taken == 0:
        assert (r.next, r.window, r.room, r.flags) == (before.rcv_next, before.rcv_window, before.room(), before.flags())
    else:
        assert r.next == (before.rcv_next + r.bytes) & 0xFFFFFFFF and r.window == min(r.room, 29200)


def test_model_window_follows_the_buffer():
    # room 25 against segments of 10: the third overshoots (room clamps to 0), the fourth meets window 0
    t = _tcb(max_receive_buf_size=25)
    t.rcv_window = 25
    r = _walk(t, [_seg(1000 + 10 * k, 10) for k in range(5)])
    assert (r.taken, r.bytes, r.room, r.window, r.stop) == (3, 30, 0, 0, dm.STOP_WINDOW)
    t = _tcb(max_receive_buf_size=30)                      # S = room exactly
    r = _walk(t, [_seg(1000 + 10 * k, 10) for k in range(5)])
    assert (r.taken, r.room, r.window, r.stop) == (3, 0, 0, dm.STOP_WINDOW)
    t = _tcb(max_receive_buf_size=31)                      # S = room - 1: one further segment
    r = _walk(t, [_seg(1000 + 10 * k, 10) for k in range(5)])
    assert (r.taken, r.bytes, r.room, r.stop) == (4, 40, 0, dm.STOP_WINDOW)
    t = _tcb(max_receive_buf_size=10 ** 6, window_scale=0)  # cap < room: the window is the cap
    r = _walk(t, [_seg(1000, 10)])
    assert (r.room, r.window) == (10 ** 6 - 10, 29200)
    t = _tcb(data_size=200000)                             # more buffered than the limit: room 0
    assert t.room() == 0 and t.rcv_record()["room"] == 0


FULL, SHORT, OVER = 1000, 999, 1001


@pytest.mark.parametrize("state,lens,want", [
    # should_send_ack branch by branch (tcp.hh:1845-1872): (nr_full, armed) before, the lengths, the flags after
    ((0, False), [OVER], dm.ACK_NOW),                                   # larger than the mss: ACK at once
    ((1, True), [OVER], dm.ACK_NOW),                                    # ... the count and the timer reset
    ((0, False), [FULL], dm.NR_FULL | dm.ACK_ARMED | dm.ACK_REARMED),   # the first full one: counted, timer armed
    ((0, True), [FULL], dm.NR_FULL | dm.ACK_ARMED),                     # ... the timer was running: not anew
    ((1, False), [FULL], dm.ACK_NOW),                                   # the second full one: nr++ >= 1
    ((1, True), [FULL], dm.ACK_NOW),
    ((0, False), [SHORT], dm.ACK_ARMED | dm.ACK_REARMED),
    ((1, False), [SHORT], dm.NR_FULL | dm.ACK_ARMED | dm.ACK_REARMED),
    ((0, True), [SHORT], dm.ACK_ARMED),
    ((1, True), [SHORT], dm.NR_FULL | dm.ACK_ARMED),
    ((0, False), [FULL, FULL], dm.ACK_NOW | dm.ACK_REARMED),            # armed by the first, cancelled by the second
    ((0, False), [FULL, FULL, SHORT], dm.ACK_NOW | dm.ACK_REARMED | dm.ACK_ARMED),
    ((0, False), [FULL, SHORT, FULL], dm.ACK_NOW | dm.ACK_REARMED),     # a short one between does not reset the count
    ((0, True), [FULL, FULL, FULL], dm.ACK_NOW | dm.NR_FULL | dm.ACK_ARMED | dm.ACK_REARMED),
])
def test_model_delayed_ack(state, lens, want):
    t = _tcb(nr_full_seg_received=state[0], armed=state[1])
    seq, segs = 1000, []
    for n in lens:
        segs.append(_seg(seq, n))
        seq += n
    r = _walk(t, segs)
    assert r.taken == len(lens) and r.flags == want


def test_should_send_ack_takes_sixteen_bits():
    t = _tcb(mss=4, max_receive_buf_size=1 << 30)
    r = _walk(t, [_seg(1000, 65536 + 3)])                  # uint16_t seg_len: 3 < mss
    assert r.taken == 1 and r.flags == dm.ACK_ARMED | dm.ACK_REARMED


# ---------------------------------------------------------------- the capacity rule

def _result(taken, nbytes):
    return dm.RunResult(taken, nbytes, 1, 2, 3, dm.NR_FULL, dm.STOP_END, [], [(0, nbytes)] if taken else [])


def test_capacity_is_a_prefix_rule():
    runs = [(2, 100), (0, 0), (3, 50), (1, 10), (0, 0)]
    initial = [dm.RunResult(0, 0, 9, 8, 7, dm.ACK_ARMED, dm.STOP_END, [], []) for _ in runs]

    def cut(max_bytes):
        out, totals = dm.capacity([_result(*r) for r in runs], initial, max_bytes)
        return [(r.taken, r.stop == dm.STOP_CAPACITY, r.desc_first, r.dst_off) for r in out], totals

    rows, totals = cut(160)                                 # exactly equal: everything fits
    assert totals == (6, 160, 160) and not any(r[1] for r in rows)
    assert [r[2:] for r in rows] == [(0, 0), (2, 100), (2, 100), (5, 150), (6, 160)]
    rows, totals = cut(159)                                 # the last run with text does not fit, nor what follows
    assert totals == (5, 150, 160) and [r[1] for r in rows] == [False, False, False, True, True]
    assert rows[3][2:] == rows[4][2:] == (5, 150)
    rows, totals = cut(149)                                 # a prefix: the small run behind the cut is not taken either
    assert totals == (2, 100, 160) and [r[1] for r in rows] == [False, False, True, True, True]
    rows, totals = cut(99)                                  # at the first run
    assert totals == (0, 0, 160) and all(r[1] for r in rows)
    rows, totals = cut(0)
    assert totals == (0, 0, 160) and all(r[1] for r in rows)
    out, _ = dm.capacity([_result(*r) for r in runs], initial, 99)
    assert (out[0].next, out[0].window, out[0].room, out[0].flags) == (9, 8, 7, dm.ACK_ARMED)
    # runs without text in front of the first that does not fit are kept
    out, totals = dm.capacity([_result(0, 0), _result(1, 5)], initial[:2], 0)
    assert [r.stop for r in out] == [dm.STOP_END, dm.STOP_CAPACITY] and totals == (0, 0, 5)


# ---------------------------------------------------------------- argument errors

def test_c_call_argument_errors_without_device():
    lib = native.load()
    p = 0x10000

    def call(data=p, seg=p, first=p, run_conn=p, run_first=p, rx_total=p, n=8, rcv=p, nconns=4, max_bytes=1 << 20,
             run=p, desc=p, total=p, ws=p):
        return lib.sccsum_tcp_rx_data(data, seg, first, run_conn, run_first, rx_total, n, rcv, nconns, max_bytes, run,
                                      desc, total, ws, None)

    ok = ENODEV if not torch.cuda.is_available() else None  # valid arguments get as far as the device
    if ok is not None:
        assert call() == ok and call(data=None) == ok and call(seg=p + 8, run=p + 8, desc=p + 8, rcv=p + 16) == ok
        assert call(max_bytes=0xFFFFFFFF, n=0xFFFFFFFF, nconns=1 << 20) == ok
        assert call(n=0, seg=None, first=None, run_conn=None, run_first=None, rx_total=None, rcv=None, run=None,
                    desc=None) == ok
        assert call(nconns=0, rcv=None) == ok
    for bad in (dict(seg=None), dict(seg=p + 4), dict(first=None), dict(first=p + 2), dict(run_conn=None),
                dict(run_conn=p + 2), dict(run_first=None), dict(run_first=p + 1), dict(rx_total=None),
                dict(rx_total=p + 4), dict(rcv=None), dict(rcv=p + 8), dict(run=None), dict(run=p + 4), dict(desc=None),
                dict(desc=p + 4), dict(total=None), dict(total=p + 4), dict(ws=None), dict(ws=p + 8),
                dict(n=1 << 32), dict(nconns=(1 << 20) + 1), dict(max_bytes=1 << 32), dict(n=0, total=None),
                dict(n=0, ws=None)):
        assert call(**bad) == EINVAL, bad
    for n in (0, 1, 1024, 1025, 1 << 20):
        w = lib.sccsum_tcp_rx_data_workspace(n, 7)
        assert w % 16 == 0 and 0 < w <= 256 + 96 * ((n + 1023) // 1024 + 1)   # per tile, nothing per record


def _fake_rx(n=40, runs=5):
    b = batch.PacketBatch(data=torch.zeros(4096, dtype=torch.uint8), off=torch.zeros(n, dtype=torch.int64),
                          length=torch.zeros(n, dtype=torch.int32), bytes_len=4096, max_len=0)
    i32 = lambda k: torch.zeros(k, dtype=torch.int32)  # noqa: E731
    return batch.TcpRxResult(source=b, order=i32(n), first=i32(5), seg=torch.zeros((n, 32), dtype=torch.uint8),
                             src_all=i32(n), run_conn=i32(runs + 1), run_first=i32(runs + 1),
                             rst=torch.zeros(20 * n, dtype=torch.uint8), rst_dst=i32(n),
                             total=torch.zeros(4, dtype=torch.int64), cls=None)


def test_python_wrapper_validation():
    rx = _fake_rx()
    rcv = torch.zeros((5, 32), dtype=torch.uint8)
    assert batch.tcp_rx_data_check(rx, rcv, 1000) == (40, 5)
    assert batch.tcp_rx_data_check(rx, rcv[:0], 0) == (40, 0)
    for name, kw in (("rx", dict(rx=None)), ("rcv", dict(rcv=None)), ("rcv", dict(rcv=torch.zeros(160, dtype=torch.uint8))),
                     ("rcv", dict(rcv=torch.zeros((5, 8), dtype=torch.int32))),
                     ("rcv", dict(rcv=torch.zeros((5, 64), dtype=torch.uint8)[:, ::2])),
                     ("rcv", dict(rcv=torch.zeros(5 * 32 + 16, dtype=torch.uint8)[8:8 + 160].view(5, 32))),
                     ("rcv", dict(rcv=torch.zeros((6, 32), dtype=torch.uint8))),   # more connections than rx's table
                     ("max_bytes", dict(max_bytes=-1)), ("max_bytes", dict(max_bytes=1 << 32))):
        with pytest.raises(ValueError, match=name):
            batch.tcp_rx_data_check(**dict(dict(rx=rx, rcv=rcv, max_bytes=10), **kw))


# ---------------------------------------------------------------- what the GPU tests run

def test_traffic_coverage():
    """The mixed traffic of the GPU tests, under the model alone: every stop
    at a run head, mid-run and at a run's last segment (a connection that is
    not eligible stops its run's head, nothing else), every transition of the
    delayed-ACK rule, and 30 % to 90 % of the segments taken."""
    cases = tr.mixed(0, 2 * tr.TILE + 7)
    results, _ = tr.walk_all(cases)
    where = {}
    for (t, segs), r in zip(cases, results):
        if r.stop == dm.STOP_END:
            assert r.taken == len(segs)
            continue
        at = "head" if r.taken == 0 and len(segs) > 1 else "last" if r.taken == len(segs) - 1 else "mid"
        where.setdefault(r.stop, set()).add(at)
    for stop in (dm.STOP_WINDOW, dm.STOP_SEQ, dm.STOP_FLAGS, dm.STOP_ACK, dm.STOP_EMPTY):
        assert where[stop] == {"head", "mid", "last"}, (stop, where[stop])
    assert where[dm.STOP_INELIGIBLE] == {"head", "last"}
    branches = {b for r in results for b in r.branches}
    assert branches >= set(dm.STOP_OF) - {"window_update", "dup_ack"}
    seen = set()
    for (t, segs), r in zip(cases, results):
        t = copy.deepcopy(t)
        for s in segs[:r.taken]:
            kind = (s["pay_len"] > t.mss) - (s["pay_len"] < t.mss)
            seen.add((t.nr_full_seg_received, t.armed, kind))
            t.take(s)
    assert len(seen) == 12, sorted(seen)
    total = sum(len(segs) for _, segs in cases)
    assert total == 2 * tr.TILE + 7
    share = sum(r.taken for r in results) / total
    assert 0.3 <= share <= 0.9, share
    assert any(((t.rcv_next + r.bytes) >> 32) and r.taken for (t, _), r in zip(cases, results))   # seq crosses 2^32
    assert any(s["pay_len"] == 65515 for _, segs in cases for s in segs)


def test_arrays_are_what_tcp_rx_leaves():
    cases = tr.mixed(3, 300)
    a = tr.arrays(cases)
    assert a["n0"] == 300 and a["first"][1] == 300 and a["rx_total"][0] == len(cases)
    conn = a["seg"]["conn"][:300]
    heads = np.flatnonzero(np.concatenate([[True], conn[1:] != conn[:-1]]))
    assert np.array_equal(heads, a["run_first"][:-1]) and np.array_equal(conn[heads], a["run_conn"])
    assert (np.diff(a["run_conn"].astype(np.int64)) > 0).all() and a["run_conn"].max() < a["nconns"]
    want = tr.expect(cases, 10 ** 9, base=0x1000)
    assert want["total"][0] == want["run"]["taken"].sum() == want["desc"].size
    assert want["total"][1] == want["run"]["bytes"].sum() == want["desc"]["len"].sum()


# ---------------------------------------------------------------- the C++ class

def test_cpp_class_on_the_host(tmp_path):
    """seastar::net::tcp_rx_data (tests/cpp/tcp_data_host.cc): workspace() and
    the argument errors of the call, through the class and directly."""
    cpp_host.build_and_run(tmp_path, "tcp_data_host", "tcp_data_host: OK")


def test_cpp_class_on_the_host_sanitized(tmp_path):
    """The same stand-alone program with tcp_data.hip itself compiled in, its
    host side under AddressSanitizer + UndefinedBehaviorSanitizer (device code
    is not instrumented): the workspace layout and the argument checks."""
    cpp_host.build_and_run_sanitized(tmp_path, "tcp_data_host", "tcp_data.hip", "tcp_data_host: OK")
