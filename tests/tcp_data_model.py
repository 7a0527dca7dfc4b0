"""A per-segment model of the receive side of tcb::input_handle_other_state for
a tcb in ESTABLISHED, written from the reference's text (include/seastar/net/
tcp.hh), over Python ints.  It walks one connection's run of sccsum_tcp_seg
records until the first segment that takes any path but the straight one —
acceptable, exactly at RCV.NXT, with text, no control flag besides ACK / PSH,
acknowledging nothing new — and says which branches that segment would take.
tcp_rx_data's results are compared with it (tests/test_gpu_tcp_data.py).

tcp_seq compares modulo 2^32 (tcp.hh:60-72: the sign of the difference)."""
from __future__ import annotations

from dataclasses import dataclass, field

M32 = 0xFFFFFFFF
FIN, SYN, RST, PSH, ACK, URG = 1, 2, 4, 8, 16, 32

# sccsum.h
ELIGIBLE, NR_FULL, ACK_ARMED, ACK_REARMED, ACK_NOW = 0x01, 0x02, 0x04, 0x08, 0x10
STOP_END, STOP_INELIGIBLE, STOP_WINDOW, STOP_SEQ, STOP_FLAGS, STOP_ACK, STOP_EMPTY, STOP_CAPACITY = range(8)

# the branch a segment leaves the straight path by -> the stop the call's contract gives it;
# a segment that leaves by several gets the lowest (the contract tests them in that order)
STOP_OF = {
    "premise": STOP_INELIGIBLE,      # not ESTABLISHED, out-of-order data pending, _snd.window == 0, una > nxt
    "zero_window": STOP_WINDOW,      # segment_acceptable's last case, tcp.hh:1072-1075
    "unacceptable": STOP_SEQ,        # segment_acceptable's other cases, tcp.hh:1224-1227
    "trim": STOP_SEQ,                # tcp.hh:1231-1237
    "out_of_order": STOP_SEQ,        # tcp.hh:1240-1245
    "rst": STOP_FLAGS,               # 4.2, tcp.hh:1248
    "syn": STOP_FLAGS,               # 4.4
    "no_ack": STOP_FLAGS,            # 4.5: a segment without ACK is dropped
    "urg": STOP_FLAGS,               # 4.6, tcp.hh:1492 (a TODO in the reference; the host's to decide)
    "fin": STOP_FLAGS,               # 4.8
    "ack_advances": STOP_ACK,        # tcp.hh:1336
    "ack_beyond": STOP_ACK,          # tcp.hh:1437
    "ack_old": STOP_ACK,             # SEG.ACK < SND.UNA: no branch fires, the host's to ignore
    "dup_ack": STOP_EMPTY,           # tcp.hh:1401
    "window_update": STOP_ACK,       # tcp.hh:1441: never with the premise _snd.window > 0
    "empty": STOP_EMPTY,             # no text: 4.7 has nothing to do (tcp.hh:1498)
}


def seq_lt(a: int, b: int) -> bool:
    return ((a - b) & M32) >= 0x80000000


def seq_le(a: int, b: int) -> bool:
    return a == b or seq_lt(a, b)


@dataclass
class Tcb:
    """What the walk reads of a tcb, named as in the reference."""
    rcv_next: int = 0
    rcv_window: int = 29200
    data_size: int = 0
    max_receive_buf_size: int = 3737600
    window_scale: int = 0                  # _rcv.window_scale
    mss: int = 1460                        # _rcv.mss
    snd_unacknowledged: int = 0
    snd_next: int = 0
    snd_window: int = 65535
    snd_window_scale: int = 0
    snd_data_empty: bool = True
    zero_window_probing_out: int = 0
    established: bool = True
    out_of_order_empty: bool = True
    nr_full_seg_received: int = 0
    armed: bool = False
    # what the walk adds
    rearmed: bool = False
    output_called: bool = False
    data: list = field(default_factory=list)   # (pay_off, pay_len) appended to _rcv.data

    def default_window(self) -> int:       # tcp.hh:418-422
        return 29200 << self.window_scale

    def modified_window(self) -> int:      # tcp.hh:424-427
        left = 0 if self.data_size > self.max_receive_buf_size else self.max_receive_buf_size - self.data_size
        return min(left, self.default_window())

    def room(self) -> int:
        return 0 if self.data_size > self.max_receive_buf_size else self.max_receive_buf_size - self.data_size

    def eligible(self) -> bool:
        return (self.established and self.out_of_order_empty and self.snd_window > 0 and
                seq_le(self.snd_unacknowledged, self.snd_next))

    def rcv_record(self) -> dict:
        """The sccsum_tcp_rcv the host writes for this tcb."""
        return dict(next=self.rcv_next, window=self.rcv_window, room=self.room(), cap=self.default_window(),
                    snd_una=self.snd_unacknowledged, mss=self.mss,
                    flags=(ELIGIBLE if self.eligible() else 0) | (NR_FULL if self.nr_full_seg_received else 0) |
                    (ACK_ARMED if self.armed else 0))

    def flags(self) -> int:
        return ((NR_FULL if self.nr_full_seg_received else 0) | (ACK_ARMED if self.armed else 0) |
                (ACK_REARMED if self.rearmed else 0) | (ACK_NOW if self.output_called else 0))

    def segment_acceptable(self, seg_seq: int, seg_len: int) -> bool:   # tcp.hh:1058-1076
        nxt, wnd = self.rcv_next, self.rcv_window
        if seg_len == 0 and wnd == 0:
            return seg_seq == nxt
        if seg_len == 0 and wnd > 0:
            return seq_le(nxt, seg_seq) and seq_lt(seg_seq, (nxt + wnd) & M32)
        if seg_len > 0 and wnd > 0:
            end = (seg_seq + seg_len - 1) & M32
            x = seq_le(nxt, seg_seq) and seq_lt(seg_seq, (nxt + wnd) & M32)
            y = seq_le(nxt, end) and seq_lt(end, (nxt + wnd) & M32)
            return x or y
        return False

    def should_send_ack(self, seg_len: int) -> bool:                    # tcp.hh:1845-1872
        seg_len &= 0xFFFF                  # the parameter is a uint16_t
        if seg_len > self.mss:
            self.nr_full_seg_received = 0
            self.armed = False             # _delayed_ack.cancel()
            return True
        if seg_len == self.mss:
            full = self.nr_full_seg_received
            self.nr_full_seg_received += 1
            if full >= 1:
                self.nr_full_seg_received = 0
                self.armed = False
                return True
        if self.armed:
            return False
        self.armed = True                  # _delayed_ack.arm(200ms)
        self.rearmed = True
        return False

    def departures(self, seg: dict) -> list:
        """The branches by which the segment leaves the straight path, none if it takes it."""
        if not self.eligible():
            return ["premise"]
        seq, ack, length, fl = seg["seq"], seg["ack"], seg["pay_len"], seg["flags"]
        if not self.segment_acceptable(seq, length):                    # tcp.hh:1224
            return ["zero_window" if length > 0 and self.rcv_window == 0 else "unacceptable"]
        if seq_lt(seq, self.rcv_next):                                  # tcp.hh:1231
            return ["trim"]
        if seq != self.rcv_next:                                        # tcp.hh:1240
            return ["out_of_order"]
        out = []
        for bit, name in ((RST, "rst"), (SYN, "syn"), (URG, "urg"), (FIN, "fin")):
            if fl & bit:
                out.append(name)
        if not fl & ACK:
            out.append("no_ack")
            return out
        # 4.5 against the send state as it stands (tcp.hh:1334-1444)
        una, nxt = self.snd_unacknowledged, self.snd_next
        packets_out = (nxt - una - self.zero_window_probing_out) & M32
        if seq_lt(una, ack) and seq_le(ack, nxt):
            out.append("ack_advances")
        elif (packets_out > 0 and not self.snd_data_empty and length == 0 and not fl & (FIN | SYN) and ack == una and
              ((seg["window"] << self.snd_window_scale) & M32) == self.snd_window):
            out.append("dup_ack")
        elif seq_lt(nxt, ack):
            out.append("ack_beyond")
        elif self.snd_window == 0 and seg["window"] > 0:
            out.append("window_update")
        elif ack != una:
            out.append("ack_old")
        if length == 0 and "dup_ack" not in out:
            out.append("empty")
        return out

    def take(self, seg: dict) -> None:
        """Step 4.7 for a segment on the straight path (tcp.hh:1497-1521) and the close (tcp.hh:1570-1574)."""
        length = seg["pay_len"]
        self.data_size += length
        self.data.append((seg["pay_off"], length))
        self.rcv_next = (self.rcv_next + length) & M32
        self.rcv_window = self.modified_window()
        if self.should_send_ack(length):
            self.armed = False             # clear_delayed_ack()
            self.output_called = True      # output()


@dataclass
class RunResult:
    taken: int
    bytes: int
    next: int
    window: int
    room: int
    flags: int
    stop: int
    branches: list
    data: list
    desc_first: int = 0
    dst_off: int = 0


def walk(tcb: Tcb, segs) -> RunResult:
    """Walk the run with the tcb (changed in place) until a segment leaves the straight path."""
    taken = nbytes = 0
    stop, branches = STOP_END, []
    for seg in segs:
        branches = tcb.departures(seg)
        if branches:
            stop = min(STOP_OF[b] for b in branches)
            break
        tcb.take(seg)
        taken += 1
        nbytes += seg["pay_len"]
    return RunResult(taken, nbytes, tcb.rcv_next, tcb.rcv_window, tcb.room(), tcb.flags(), stop, branches,
                     list(tcb.data))


def capacity(results: list, initial: list, max_bytes: int) -> tuple:
    """The prefix rule: runs are kept while the packed text of runs 0..r is <=
    max_bytes; from the first that does not fit onward nothing is taken and
    the state is initial[r] (a RunResult of an empty walk).  Fills desc_first /
    dst_off; returns (results, (taken, bytes, needed))."""
    out, cnt, total, cut = [], 0, 0, False
    needed = sum(r.bytes for r in results)
    for r, r0 in zip(results, initial):
        if not cut and total + r.bytes > max_bytes:
            cut = True
        if cut:
            r = RunResult(0, 0, r0.next, r0.window, r0.room, r0.flags, STOP_CAPACITY, [], [])
        r.desc_first, r.dst_off = cnt, total
        cnt += r.taken
        total += r.bytes
        out.append(r)
    return out, (cnt, total, needed)
