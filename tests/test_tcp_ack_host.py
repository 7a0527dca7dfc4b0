"""The TCP ACK fast path without a GPU: the per-segment model pinned on
connections written out by hand, every argument error of sccsum_tcp_rx_acks
and of batch.tcp_rx_acks, the record layouts, the C++ class, and the coverage
of the traffic that tests/test_gpu_tcp_ack.py runs."""
import collections
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import cpp_host
import tcp_ack_fast as fast
import tcp_ack_model as am
import tcp_ack_traffic as tr
from seastar_amd import batch, native
from tcp_ack_model import ACK, FIN, M32, PSH, RST, SYN, URG, Seg, Tcb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = native.SCCSUM_EINVAL, native.SCCSUM_ENODEV
MS = 1_000_000
NOW = 10_000 * MS


def test_symbols_constants_and_layouts(tmp_path):
    lib = native.load()
    declared = native.header_symbols()
    for s in ("sccsum_tcp_rx_acks", "sccsum_tcp_rx_acks_workspace"):
        assert s in declared and s in native._PROTOS and getattr(lib, s).argtypes is not None
    assert os.path.join(REPO, "seastar_amd", "csrc", "tcp_ack.hip") in __import__("seastar_amd.build").build.SOURCES
    header = open(native.HEADER_PATH).read()
    for name, value, model in (("ACK_ELIGIBLE", native.TCP_ACK_ELIGIBLE, am.ELIGIBLE),
                               ("ACK_CLOSE_WAIT", native.TCP_ACK_CLOSE_WAIT, am.CLOSE_WAIT),
                               ("ACK_FIRST_SAMPLE", native.TCP_ACK_FIRST_SAMPLE, am.FIRST_SAMPLE),
                               ("ACK_ALL_ACKED", native.TCP_ACK_ALL_ACKED, am.ALL_ACKED),
                               ("ACK_RTX_REARM", native.TCP_ACK_RTX_REARM, am.RTX_REARM),
                               ("ACK_POLL", native.TCP_ACK_POLL, am.POLL),
                               ("STOP_END", native.TCP_STOP_END, am.STOP_END),
                               ("STOP_INELIGIBLE", native.TCP_STOP_INELIGIBLE, am.STOP_INELIGIBLE),
                               ("STOP_WINDOW", native.TCP_STOP_WINDOW, am.STOP_WINDOW),
                               ("STOP_SEQ", native.TCP_STOP_SEQ, am.STOP_SEQ),
                               ("STOP_FLAGS", native.TCP_STOP_FLAGS, am.STOP_FLAGS),
                               ("STOP_ACK", native.TCP_STOP_ACK, am.STOP_ACK),
                               ("STOP_QUEUE", native.TCP_STOP_QUEUE, am.STOP_QUEUE),
                               ("STOP_DATA", native.TCP_STOP_DATA, am.STOP_DATA),
                               ("STOP_WL", native.TCP_STOP_WL, am.STOP_WL)):
        assert value == model
        assert int(header.split(f"#define SCCSUM_TCP_{name} ")[1].split()[0].rstrip("u"), 0) == value, name
    assert (am.STOP_DATA, am.STOP_WL) == (9, 10)
    assert batch.TCP_ACK_DTYPE == tr.ACK_DTYPE and batch.TCP_ACK_RUN_DTYPE == tr.RUN_DTYPE
    assert batch.TCP_SEG_DTYPE == tr.SEG_DTYPE
    assert ctypes.sizeof(native.TcpAck) == 64 and ctypes.sizeof(native.TcpAckRun) == 64
    structs = (("sccsum_tcp_ack", tr.ACK_DTYPE, native.TcpAck), ("sccsum_tcp_ack_run", tr.RUN_DTYPE, native.TcpAckRun))
    lines = []
    for cname, dt, _ in structs:
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in dt.names]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <sccsum.h>\nint main(void) {\n"
                   + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    for cname, dt, ct in structs:
        assert int(got[cname]) == dt.itemsize == 64 and dt.itemsize % 16 == 0
        assert [f for f, _ in ct._fields_] == list(dt.names)
        for f in dt.names:
            assert int(got[f"{cname}.{f}"]) == dt.fields[f][1] == getattr(ct, f).offset, (cname, f)


# ---------------------------------------------------------------- connections written out by hand

def _tcb(lens=(1000, 1000, 1000), **kw) -> Tcb:
    """una 1000, entries of `lens` sent 100 ms ago, rcv_next 5000, wl1 5000, wl2 1000."""
    kw = dict(dict(una=1000, wl1=5000, wl2=1000, unsent_len=10000), **kw)
    tx = kw.pop("tx", NOW - 100 * MS)
    retransmitted = kw.pop("retransmitted", ())
    data_len = kw.pop("data_len", None)
    t = Tcb(**kw)
    nxt = kw.get("next")
    t.queue(lens, data_len=data_len, tx=tx, retransmitted=retransmitted)
    if nxt is not None:
        t.next = nxt
    return t


def _acks(t: Tcb, *offsets, window=2000):
    return [Seg(seq=t.rcv_next, ack=(t.una + o) & M32, window=window) for o in offsets]


def _run(t: Tcb, segs, **kw):
    """The rule on one run, the numpy restatement with it, and the host's
    hand-off: the record applied to the tcb is the tcb the walk left."""
    rec, after = am.expect_run(t, segs, NOW, **kw)
    cases = [(t, segs, dict(eligible=kw.get("eligible"), lens=kw.get("lens")))]
    a = tr.arrays(cases, others=0, now=NOW)
    got = fast.expect(a)
    assert got["run"].tobytes() == np.array([tr.record(rec)], dtype=tr.RUN_DTYPE).tobytes(), (got["run"], rec)
    if kw.get("lens") is None:
        back = am.apply(t, rec)
        for name in ("una", "window", "cwnd", "srtt", "rttvar", "rto", "first_rto_sample"):
            assert getattr(back, name) == getattr(after, name), name
        assert [e.len for e in back.data] == [e.len for e in after.data]
        if rec["taken"]:
            assert (back.wl1, back.wl2, back.dupacks) == (after.wl1, after.wl2, after.dupacks)
    return rec, after


def test_one_connection_per_stop():
    t = _tcb()
    rec, after = _run(t, _acks(t, 500, 1000, 3000))
    assert (rec["taken"], rec["stop"], rec["una"], rec["acked"], rec["popped"], rec["trim"]) == (3, am.STOP_END, 4000, 3000, 3, 0)
    assert rec["flags"] == am.ALL_ACKED | am.POLL and after.rtx == "stopped" and after.all_acked == 1
    for change, stop in ((dict(state="FIN_WAIT_1"), am.STOP_INELIGIBLE), (dict(dupacks=3), am.STOP_INELIGIBLE),
                         (dict(window_probe=True), am.STOP_INELIGIBLE),
                         (dict(zero_window_probing_out=1), am.STOP_INELIGIBLE),
                         (dict(window=0), am.STOP_INELIGIBLE), (dict(window_scale=15), am.STOP_INELIGIBLE)):
        t = _tcb(**change)
        rec, _ = _run(t, _acks(t, 500))
        assert (rec["taken"], rec["stop"], rec["una"], rec["flags"]) == (0, stop, 1000, am.FIRST_SAMPLE), change
    # what the device checks whatever the host says
    for change in (dict(cwnd=0), dict(cwnd=1 << 31), dict(window_scale=15), dict(next=999), dict(window=0)):
        t = _tcb(**change)
        assert _run(t, _acks(t, 500), eligible=True)[0]["stop"] == am.STOP_INELIGIBLE, change
    t = _tcb()
    assert _run(t, _acks(t, 500), eligible=False)[0]["stop"] == am.STOP_INELIGIBLE
    assert _run(t, _acks(t, 500), lens=[1000, 1000, 999])[0]["stop"] == am.STOP_QUEUE
    assert _run(t, _acks(t, 500), lens=[1000, 1000, 1001])[0]["stop"] == am.STOP_QUEUE
    assert _run(t, _acks(t, 500), lens=[1000, 0, 2000])[0]["stop"] == am.STOP_QUEUE
    assert _run(t, _acks(t, 500), lens=[1000, 2000, 0])[0]["stop"] == am.STOP_QUEUE
    assert _run(t, _acks(t, 500), lens=[])[0]["stop"] == am.STOP_QUEUE
    assert _run(t, _acks(t, 500), lens=[1 << 31, 1 << 31, 1 << 31, 1 << 31, 3000])[0]["stop"] == am.STOP_QUEUE  # 64-bit sum

    def one(mutate, stop, branch, at=1):
        t = _tcb()
        segs = _acks(t, 500, 1500, 2500)
        mutate(t, segs[at])
        rec, after = _run(t, segs)
        assert (rec["taken"], rec["stop"]) == (at, stop), (stop, branch)
        whole = copy.deepcopy(after)
        assert whole.input(segs[at], NOW) == branch, (stop, branch)   # why the reference leaves the straight path there
        return rec

    one(lambda t, s: setattr(s, "seq", 5001), am.STOP_SEQ, "out_of_order")
    one(lambda t, s: setattr(s, "seq", 4999), am.STOP_SEQ, "unacceptable")
    one(lambda t, s: setattr(s, "flags", ACK | FIN), am.STOP_FLAGS, "fin")
    one(lambda t, s: setattr(s, "flags", ACK | SYN), am.STOP_FLAGS, "syn")
    one(lambda t, s: setattr(s, "flags", ACK | RST), am.STOP_FLAGS, "rst")
    one(lambda t, s: setattr(s, "flags", ACK | URG), am.STOP_FLAGS, "urg")
    one(lambda t, s: setattr(s, "flags", PSH), am.STOP_FLAGS, "no_ack")
    one(lambda t, s: setattr(s, "pay_len", 100), am.STOP_DATA, "text")
    one(lambda t, s: setattr(s, "ack", 1500), am.STOP_ACK, "dupack")
    one(lambda t, s: setattr(s, "ack", 1499), am.STOP_ACK, "old_ack")
    one(lambda t, s: setattr(s, "ack", 4001), am.STOP_ACK, "ack_beyond_next")
    rec = one(lambda t, s: setattr(s, "window", 0), am.STOP_WINDOW, "advance_window_closed")
    assert rec["flags"] == am.RTX_REARM | am.FIRST_SAMPLE and rec["una"] == 1500 and rec["trim"] == 500
    one(lambda t, s: setattr(t, "wl1", 5001), am.STOP_WL, "advance_window_kept", at=0)
    # PSH rides along
    t = _tcb()
    segs = _acks(t, 500)
    segs[0].flags = ACK | PSH
    assert _run(t, segs)[0]["taken"] == 1


@pytest.mark.parametrize("off,popped,trim", [(999, 0, 999), (1000, 1, 0), (1001, 1, 1), (1, 0, 1), (2999, 2, 999),
                                             (3000, 3, 0)])
def test_an_ack_around_an_entry_boundary(off, popped, trim):
    t = _tcb(data_len=1010)
    rec, after = _run(t, _acks(t, off))
    assert (rec["taken"], rec["una"], rec["acked"], rec["popped"], rec["trim"]) == (1, 1000 + off, off, popped, trim)
    assert rec["queue_freed"] == 1010 * popped
    assert rec["flags"] & (am.ALL_ACKED | am.RTX_REARM) == (am.ALL_ACKED if off == 3000 else am.RTX_REARM)
    assert after.rtx == ("stopped" if off == 3000 else "restarted")


def test_one_ack_popping_many_entries_and_many_acks_inside_one():
    t = _tcb(lens=[10] * 50 + [7])
    rec, _ = _run(t, _acks(t, 503))
    assert (rec["popped"], rec["trim"], rec["acked"], rec["taken"]) == (50, 3, 503, 1)
    t = _tcb(lens=[1] * 9)                       # 1-byte entries
    rec, _ = _run(t, _acks(t, 1, 2, 5, 9))
    assert (rec["popped"], rec["trim"], rec["flags"] & am.ALL_ACKED) == (9, 0, am.ALL_ACKED)
    t = _tcb(lens=[5000], cwnd=1000, ssthresh=M32)
    rec, _ = _run(t, _acks(t, 1, 2, 10, 100, 4999))
    assert (rec["popped"], rec["trim"], rec["taken"]) == (0, 4999, 5)
    assert rec["cwnd"] == 1000 + 1 + 1 + 8 + 90 + 1460      # min(bytes, mss) per partial ACK
    rec, _ = _run(t, _acks(t, 1, 2, 10, 100, 4999, 5000))
    assert (rec["popped"], rec["trim"]) == (1, 0) and rec["cwnd"] == 1000 + 1 + 1 + 8 + 90 + 1460 + 1


def test_slow_start_crosses_ssthresh_inside_one_acks_pops():
    t = _tcb(lens=[1000] * 4, cwnd=2000, ssthresh=3500, mss=1460)
    rec, _ = _run(t, _acks(t, 4000))
    # 2000 -> 3000 -> 4000 in slow start (the test is before the increment), then 1460^2 / 4000 = 532, then / 4532 = 470
    assert rec["cwnd"] == 4000 + 532 + 470


@pytest.mark.parametrize("cwnd,want", [(1460 * 1460 + 1, 1), (1460 * 1460, 1), (1460 * 1460 - 1, 1), (1460 * 730, 2),
                                       (14600, 146)])
def test_congestion_avoidance_quotients(cwnd, want):
    t = _tcb(lens=[3000], cwnd=cwnd, ssthresh=2920)
    assert _run(t, _acks(t, 100))[0]["cwnd"] == cwnd + want


def test_rtt_samples_first_later_skipped_and_clamped():
    t = _tcb(lens=[100, 100, 100], tx=[NOW - 101 * MS - 999_999, NOW - 51 * MS, NOW - 300 * MS], first_rto_sample=True)
    rec, _ = _run(t, _acks(t, 100))
    assert (rec["srtt"], rec["rttvar"], rec["rto"], rec["flags"] & am.FIRST_SAMPLE) == (101, 50, 1000, 0)   # the low clamp
    rec, _ = _run(t, _acks(t, 200))
    assert (rec["srtt"], rec["rttvar"]) == (101 * 7 // 8 + 51 // 8, 50 * 3 // 4 + 50 // 4)
    t = _tcb(lens=[100, 100], retransmitted=(0, 1), first_rto_sample=True, srtt=7, rttvar=9, rto=2222)
    rec, _ = _run(t, _acks(t, 200))
    assert (rec["srtt"], rec["rttvar"], rec["rto"], rec["flags"]) == (7, 9, 2222, am.FIRST_SAMPLE | am.ALL_ACKED | am.POLL)
    t = _tcb(lens=[100], tx=NOW - 50_000 * MS, first_rto_sample=True)
    assert _run(t, _acks(t, 100))[0]["rto"] == 60000                                                       # the high clamp
    t = _tcb(lens=[100], tx=NOW - 1500 * MS, first_rto_sample=False, srtt=1000, rttvar=100)
    rec, _ = _run(t, _acks(t, 100))
    assert (rec["srtt"], rec["rttvar"], rec["rto"]) == (875 + 187, 75 + 125, 1062 + 800)                  # between them


def test_tx_later_than_now_truncates_towards_zero():
    t = _tcb(lens=[100, 100], tx=[NOW + 1_999_999, NOW + 5 * MS + 1], first_rto_sample=True)
    rec, _ = _run(t, _acks(t, 100))
    assert (rec["srtt"], rec["rttvar"]) == (-1, 0)         # floor would give -2 and -1
    rec, _ = _run(t, _acks(t, 200))
    assert (rec["srtt"], rec["rttvar"]) == (0, 1)          # -1 * 7 / 8 = 0, -5 / 8 = 0; |(-1) - (-5)| / 4 = 1
    t = _tcb(lens=[100], tx=NOW + 9 * MS, first_rto_sample=False, srtt=-9, rttvar=-7)
    rec, _ = _run(t, _acks(t, 100))
    assert (rec["srtt"], rec["rttvar"], rec["rto"]) == (-7 - 1, -5, 1000)   # -63/8 = -7, -9/8 = -1, -21/4 = -5


def test_una_and_ack_across_the_wrap():
    t = _tcb(lens=[1000, 1000, 1000], una=M32 - 1499, wl2=M32 - 1499)
    rec, _ = _run(t, _acks(t, 999, 1500, 1501, 3000))
    assert (rec["taken"], rec["una"], rec["acked"], rec["popped"]) == (4, 1500, 3000, 3)
    rec, _ = _run(t, _acks(t, 1499, 1500))
    assert (rec["una"], rec["acked"], rec["popped"], rec["trim"]) == (0, 1500, 1, 500)


def test_wl1_wl2_on_each_side():
    for wl1, wl2, taken in ((4999, 9999, 1), (5000, 1499, 1), (5000, 1500, 1), (5000, 1501, 0), (5001, 0, 0),
                            (5000 + (1 << 31) - 1, 0, 0), (5000 + (1 << 31), 0, 1)):
        t = _tcb(wl1=wl1, wl2=wl2)
        rec, _ = _run(t, _acks(t, 500, 600))
        assert rec["taken"] == 2 * taken and rec["stop"] == (am.STOP_END if taken else am.STOP_WL), (wl1, wl2)


def test_poll_close_wait_unsent_and_the_window():
    t = _tcb(first_rto_sample=False)
    rec, after = _run(t, _acks(t, 500))
    assert rec["flags"] == am.RTX_REARM and after.outputs == 0          # used 2500 >= window 2000
    rec, after = _run(t, _acks(t, 500, window=2500))
    assert rec["flags"] == am.RTX_REARM and after.outputs == 0          # used at the window
    rec, after = _run(t, _acks(t, 500, window=2501))
    assert rec["flags"] == am.RTX_REARM | am.POLL and after.outputs == 1  # one below
    t = _tcb(first_rto_sample=False, window_scale=3)
    assert _run(t, _acks(t, 500, window=313))[0]["flags"] == am.RTX_REARM | am.POLL      # 2504
    assert _run(t, _acks(t, 500, window=312))[0]["window"] == 2496
    t = _tcb(first_rto_sample=False, unsent_len=0)
    assert _run(t, _acks(t, 500, window=60000))[0]["flags"] == am.RTX_REARM
    t = _tcb(first_rto_sample=False, state="CLOSE_WAIT")
    rec, after = _run(t, _acks(t, 500, window=60000))
    assert rec["flags"] == am.RTX_REARM and after.outputs == 0 and am.in_flags(t) & am.CLOSE_WAIT
    # one ACK that could send among others that could not
    t = _tcb(first_rto_sample=False)
    segs = _acks(t, 500, 600, 700)
    segs[1].window = 60000
    rec, after = _run(t, segs)
    assert rec["flags"] == am.RTX_REARM | am.POLL and after.outputs == 1 and rec["window"] == 2000
    # limited transmit counts are gone with the first taken ACK
    t = _tcb(first_rto_sample=False, dupacks=2)
    rec, after = _run(t, _acks(t, 500, window=60000))
    assert after.dupacks == 0 and rec["flags"] & am.POLL


# ---------------------------------------------------------------- argument errors

def test_c_call_argument_errors_without_device():
    lib = native.load()
    p = 0x10000

    def call(seg=p, first=p, run_conn=p, run_first=p, rx_total=p, n=64, ack=p, nconns=4, q_first=p, q_len=p, q_meta=p,
             q_tx=p, nq=8, now=0, run=p, total=p, ws=p):
        return lib.sccsum_tcp_rx_acks(seg, first, run_conn, run_first, rx_total, n, ack, nconns, q_first, q_len, q_meta,
                                      q_tx, nq, now, run, total, ws, None)

    if not torch.cuda.is_available():  # valid arguments get as far as the device
        assert call() == ENODEV
        assert call(nq=0, q_len=None, q_meta=None, q_tx=None) == ENODEV
        assert call(nconns=0, ack=None, q_first=None) == ENODEV
        assert call(n=0, seg=None, first=None, run_conn=None, run_first=None, rx_total=None, ack=None, run=None,
                    q_len=None, q_meta=None, q_tx=None) == ENODEV
        assert call(n=0xFFFFFFFF, nconns=1 << 20, nq=1 << 31, now=-(1 << 63)) == ENODEV
        assert call(seg=p + 8, ack=p + 16, run=p + 16, q_tx=p + 8, total=p + 8, q_first=p + 4) == ENODEV
    for bad in (dict(seg=None), dict(seg=p + 4), dict(first=None), dict(first=p + 2), dict(run_conn=None),
                dict(run_conn=p + 2), dict(run_first=None), dict(run_first=p + 1), dict(rx_total=None),
                dict(rx_total=p + 4), dict(ack=None), dict(ack=p + 8), dict(q_first=None), dict(q_first=p + 2),
                dict(q_len=None), dict(q_len=p + 2), dict(q_meta=None), dict(q_meta=p + 1), dict(q_tx=None),
                dict(q_tx=p + 4), dict(run=None), dict(run=p + 8), dict(total=None), dict(total=p + 4), dict(ws=None),
                dict(ws=p + 8), dict(n=1 << 32), dict(nconns=(1 << 20) + 1), dict(nq=(1 << 31) + 1),
                dict(n=0, total=None), dict(n=0, ws=None), dict(n=0, q_first=None)):
        assert call(**bad) == EINVAL, bad
    before = 0
    for n, nconns, nq in ((0, 0, 0), (1, 1, 0), (1, 1, 1), (1024, 1024, 1025), (1 << 20, 1025, 1 << 20),
                          (1 << 20, 1 << 20, 1 << 22)):
        w = lib.sccsum_tcp_rx_acks_workspace(n, nconns, nq)
        assert w % 16 == 0 and before < w <= 256 + 9 * n + 13 * nq   # a pair per record, two scans per entry
        before = w


def _rx(n=6, runs=4, dev="cpu") -> batch.TcpRxResult:
    z32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)   # noqa: E731
    return batch.TcpRxResult(source=None, order=z32(n), first=z32(5), seg=torch.zeros((n, 32), dtype=torch.uint8, device=dev),
                             src_all=z32(n), run_conn=z32(runs), run_first=z32(runs), rst=z32(1), rst_dst=z32(n),
                             total=torch.zeros(4, dtype=torch.int64, device=dev), cls=None)


def test_python_wrapper_validation():
    state = torch.zeros((3, 64), dtype=torch.uint8)
    q = batch.TcpAckQueues(first=torch.zeros(4, dtype=torch.int32), length=torch.zeros(7, dtype=torch.int32),
                           meta=torch.zeros(7, dtype=torch.int32), tx=torch.zeros(7, dtype=torch.int64))
    good = dict(rx=_rx(), ack_state=state, queue=q, now_ns=5)
    assert batch.tcp_rx_acks_check(**good) == (6, 3, 7)
    assert batch.tcp_rx_acks_check(**dict(good, now_ns=-(1 << 63))) == (6, 3, 7)
    none = batch.TcpAckQueues(first=q.first[:1], length=q.length[:0], meta=q.meta[:0], tx=q.tx[:0])
    assert batch.tcp_rx_acks_check(**dict(good, ack_state=state[:0], queue=none)) == (6, 0, 0)

    def qq(**kw):
        return batch.TcpAckQueues(**dict(dict(first=q.first, length=q.length, meta=q.meta, tx=q.tx), **kw))

    for name, kw in (("rx", dict(rx=None)), ("ack_state", dict(ack_state=None)),
                     ("ack_state", dict(ack_state=torch.zeros(192, dtype=torch.uint8))),
                     ("ack_state", dict(ack_state=torch.zeros((3, 16), dtype=torch.int32))),
                     ("ack_state", dict(ack_state=torch.zeros((3, 128), dtype=torch.uint8)[:, ::2])),
                     ("ack_state", dict(ack_state=torch.zeros(3 * 64 + 16, dtype=torch.uint8)[8:8 + 192].view(3, 64))),
                     ("ack_state", dict(ack_state=torch.zeros((3, 32), dtype=torch.uint8))),
                     ("ack_state", dict(ack_state=torch.zeros((5, 64), dtype=torch.uint8))),   # rx made for fewer
                     ("queue", dict(queue=None)), ("queue", dict(queue=(q.first, q.length, q.meta, q.tx))),
                     ("queue.first", dict(queue=qq(first=q.first[:3]))),
                     ("queue.first", dict(queue=qq(first=q.first.to(torch.int64)))),
                     ("queue.first", dict(queue=qq(first=None))),
                     ("queue.length", dict(queue=qq(length=q.length.to(torch.int64)))),
                     ("queue.length", dict(queue=qq(length=torch.zeros(14, dtype=torch.int32)[::2]))),
                     ("queue.meta", dict(queue=qq(meta=q.meta[:6]))), ("queue.meta", dict(queue=qq(meta=q.meta.view(1, 7)))),
                     ("queue.tx", dict(queue=qq(tx=q.tx[:6]))), ("queue.tx", dict(queue=qq(tx=q.tx.to(torch.int32)))),
                     ("now_ns", dict(now_ns=1 << 63)), ("now_ns", dict(now_ns=-(1 << 63) - 1))):
        with pytest.raises(ValueError, match=name):
            batch.tcp_rx_acks_check(**dict(good, **kw))
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="queue"):   # every array lives where the records do
            batch.tcp_rx_acks_check(**dict(good, rx=_rx(dev="cuda:0"), ack_state=state.cuda()))


# ---------------------------------------------------------------- what the GPU tests run

def test_traffic_coverage_and_the_restatement():
    """The mixed traffic of the GPU tests, under the model alone: every stop
    at a run's head, mid-run and at a last segment (_STOP_WL and the
    connection-level stops at heads only), 30 % to 90 % of the ACKs taken; the
    stops are exactly the segments the reference walks another way; and the
    numpy restatement the scale tests use gives the model's bytes."""
    cases = tr.mixed(0, 2 * tr.TILE + 7)
    want = tr.expect(cases)
    where = collections.defaultdict(set)
    for (t, segs, opts), r, after in zip(cases, want["run"], want["after"]):
        k, stop = int(r["taken"]), int(r["stop"])
        assert (stop == am.STOP_END) == (k == len(segs))
        if stop:
            where[stop].add("head" if k == 0 else "last" if k == len(segs) - 1 else "mid")
        if stop in (am.STOP_SEQ, am.STOP_FLAGS, am.STOP_DATA, am.STOP_ACK, am.STOP_WL, am.STOP_WINDOW):
            branch = copy.deepcopy(after).input(segs[k], tr.NOW)
            # conservative: CLOSE_WAIT returns before the FIN step (tcp.hh:1522-1526), so a FIN there only advances
            assert branch != "advance" or (t.state == "CLOSE_WAIT" and segs[k].flags & FIN), (stop, branch)
    everywhere = {"head", "mid", "last"}
    assert dict(where) == {am.STOP_INELIGIBLE: {"head"}, am.STOP_QUEUE: {"head"}, am.STOP_WL: {"head"},
                           am.STOP_SEQ: everywhere, am.STOP_FLAGS: everywhere, am.STOP_DATA: everywhere,
                           am.STOP_ACK: everywhere, am.STOP_WINDOW: everywhere}
    n = sum(len(segs) for _, segs, _ in cases)
    assert n == 2 * tr.TILE + 7 and 0.3 * n <= int(want["total"][1]) <= 0.9 * n
    flags = set(want["run"]["flags"].tolist())
    assert {am.ALL_ACKED, am.RTX_REARM, am.RTX_REARM | am.POLL, am.FIRST_SAMPLE} <= flags
    assert any(int(r["una"]) < t.una and r["taken"] for (t, _, _), r in zip(cases, want["run"]))   # una crosses 2^32
    assert any(r["popped"] > 5 for r in want["run"]) and any(r["trim"] for r in want["run"])
    assert any(r["srtt"] < 0 or r["rttvar"] != 0 for r in want["run"])
    got = fast.expect(tr.arrays(cases))
    assert got["run"].tobytes() == want["run"].tobytes() and got["total"].tolist() == want["total"].tolist()
    for seed, lengths in ((1, [1, 700, 3, 3]), (2, [3] * 40)):
        cases = tr.by_lengths(seed, lengths, stops=[None, 650, 1, None] if seed == 1 else None)
        want = tr.expect(cases)
        got = fast.expect(tr.arrays(cases))
        assert got["run"].tobytes() == want["run"].tobytes() and got["total"].tolist() == want["total"].tolist()


# ---------------------------------------------------------------- the C++ class

def test_cpp_class_on_the_host(tmp_path):
    """seastar::net::tcp_rx_acks (tests/cpp/tcp_ack_host.cc): workspace() and
    the argument errors of the call, through the class and directly."""
    cpp_host.build_and_run(tmp_path, "tcp_ack_host", "tcp_ack_host: OK")


def test_cpp_class_on_the_host_sanitized(tmp_path):
    """The same stand-alone program with tcp_ack.hip itself compiled in, its
    host side under AddressSanitizer + UndefinedBehaviorSanitizer (device code
    is not instrumented): the workspace layout and the argument checks."""
    cpp_host.build_and_run_sanitized(tmp_path, "tcp_ack_host", "tcp_ack.hip", "tcp_ack_host: OK")
