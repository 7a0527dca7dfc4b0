"""The reference's send-side ACK processing per segment, over Python ints and
a deque of entries, written from the reference's text (include/seastar/net/
tcp.hh): segment_acceptable (1058-1076), input_handle_other_state (1215-1575)
with all four branches of its ACK step (1336-1444), data_segment_acked
(1026-1055), update_cwnd (2042-2052), update_rto (2016-2039) with C++'s
truncating division, update_window (1316-1329), the CLOSE_WAIT return
(1522-1526) and the closing can_send() (515-549, 1570-1574).

Tcb.input() walks ONE segment and names the branch by which it leaves the
straight path ("advance" is the straight path).  expect_run() is the rule of
include/sccsum.h ("TCP ACK fast path") for one run, stated on top of it: the
stops from the rule's table, the effect from Tcb.input() itself.
"""
from __future__ import annotations

import copy
from collections import deque
from dataclasses import dataclass, field

M32 = 0xFFFFFFFF

ELIGIBLE, CLOSE_WAIT, FIRST_SAMPLE, ALL_ACKED, RTX_REARM, POLL = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
STOP_END, STOP_INELIGIBLE, STOP_WINDOW, STOP_SEQ, STOP_FLAGS, STOP_ACK = 0, 1, 2, 3, 4, 5
STOP_QUEUE, STOP_DATA, STOP_WL = 8, 9, 10
FIN, SYN, RST, PSH, ACK, URG = 1, 2, 4, 8, 16, 32


def lt(a: int, b: int) -> bool:
    """tcp_seq's a < b (tcp.hh:220-226): int32(a - b) < 0."""
    return ((a - b) & M32) >= 0x80000000


def le(a: int, b: int) -> bool:
    return a == b or lt(a, b)


def tdiv(a: int, b: int) -> int:
    """C++'s integer division: towards zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


@dataclass
class Entry:
    """One unacked_segment of _snd.data."""
    len: int              # p.len() as it stands
    data_len: int
    nr_transmits: int = 0
    tx_time: int = 0      # ns


@dataclass
class Seg:
    seq: int
    ack: int
    window: int = 1000
    flags: int = ACK
    pay_len: int = 0


@dataclass
class Tcb:
    state: str = "ESTABLISHED"
    una: int = 1000
    next: int = 1000
    window: int = 65535
    wl1: int = 0
    wl2: int = 0
    cwnd: int = 14600
    ssthresh: int = M32
    unsent_len: int = 0
    dupacks: int = 0
    window_probe: bool = False
    zero_window_probing_out: int = 0
    window_scale: int = 0
    mss: int = 1460
    first_rto_sample: bool = True
    srtt: int = 0         # ms
    rttvar: int = 0
    rto: int = 1000
    rcv_next: int = 5000
    rcv_window: int = 29200
    recover: int = 0
    partial_ack: int = 0
    limited_transfer: int = 0
    data: deque = field(default_factory=deque)
    # what the walk did besides moving the fields above
    outputs: int = 0              # output() calls
    queue_freed: int = 0          # current_queue_space given back
    all_acked: int = 0            # signal_all_data_acked()
    rtx: str = "as_given"         # the retransmit timer: as_given / stopped / restarted
    persist: str = "as_given"     # the persist timer: as_given / stopped / armed
    persist_rto: int = 0
    popped: int = 0
    trim: int = 0                 # trimmed off the entry now at the front, by this walk
    text: int = 0                 # bytes of text appended

    def queue(self, lens, data_len=None, tx=0, retransmitted=()) -> "Tcb":
        """Fills _snd.data and sets next = una + their sum."""
        self.data = deque(Entry(n, n if data_len is None else data_len, 1 if j in retransmitted else 0,
                                tx[j] if isinstance(tx, (list, tuple)) else tx) for j, n in enumerate(lens))
        self.next = (self.una + sum(lens)) & M32
        return self

    # ---- tcp.hh:515-549
    def can_send(self) -> int:
        if self.window_probe:
            return 1
        if self.window == 0:
            return 0
        used = (self.next - self.una) & M32
        if used > self.window:
            return 0
        x = min(self.window - used, self.unsent_len)
        x = min(self.cwnd, x)
        if self.dupacks in (1, 2):
            flight = sum(e.len for e in self.data) & M32
            mx = (self.cwnd + 2 * self.mss) & M32
            x = min(x, mx - flight) if flight <= mx else 0
            self.limited_transfer = (self.limited_transfer + x) & M32
        elif self.dupacks >= 3:
            x = min(self.mss, x)
        return x

    # ---- tcp.hh:2016-2039
    def update_rto(self, tx_time: int, now: int) -> None:
        r = tdiv(now - tx_time, 1000000)
        if self.first_rto_sample:
            self.first_rto_sample = False
            self.rttvar = tdiv(r, 2)
            self.srtt = r
        else:
            delta = self.srtt - r if self.srtt > r else r - self.srtt
            self.rttvar = tdiv(self.rttvar * 3, 4) + tdiv(delta, 4)
            self.srtt = tdiv(self.srtt * 7, 8) + tdiv(r, 8)
        self.rto = min(max(self.srtt + max(1, 4 * self.rttvar), 1000), 60000)

    # ---- tcp.hh:2042-2052
    def update_cwnd(self, acked: int) -> None:
        if self.cwnd < self.ssthresh:
            self.cwnd = (self.cwnd + min(acked, self.mss)) & M32
        else:
            self.cwnd = (self.cwnd + max(1, ((self.mss * self.mss) & M32) // self.cwnd)) & M32

    # ---- tcp.hh:1026-1055
    def data_segment_acked(self, ack: int, now: int) -> int:
        total = 0
        while self.data and le((self.una + self.data[0].len) & M32, ack):
            e = self.data[0]
            self.una = (self.una + e.len) & M32
            if e.nr_transmits == 0:
                self.update_rto(e.tx_time, now)
            self.update_cwnd(e.len)
            total += e.len
            self.queue_freed += e.data_len
            self.data.popleft()
            self.popped += 1
            self.trim = 0
        if lt(self.una, ack):
            acked = (ack - self.una) & M32
            if self.data:
                self.data[0].len -= acked
                self.trim += acked
            self.una = ack
            self.update_cwnd(acked)
            total += acked
        return total

    # ---- tcp.hh:1058-1076
    def segment_acceptable(self, seq: int, seg_len: int) -> bool:
        end = (self.rcv_next + self.rcv_window) & M32
        if seg_len == 0 and self.rcv_window == 0:
            return seq == self.rcv_next
        if seg_len == 0:
            return le(self.rcv_next, seq) and lt(seq, end)
        if self.rcv_window > 0:
            last = (seq + seg_len - 1) & M32
            return (le(self.rcv_next, seq) and lt(seq, end)) or (le(self.rcv_next, last) and lt(last, end))
        return False

    def _update_window(self, s: Seg) -> None:
        self.window = (s.window << self.window_scale) & M32
        self.wl1, self.wl2 = s.seq, s.ack
        self.zero_window_probing_out = 0
        if self.window == 0:
            self.persist, self.persist_rto = "armed", self.rto
        else:
            self.persist = "stopped"

    def _set_retransmit_timer(self) -> None:
        if not self.data:
            self.rtx = "stopped"
            self.all_acked += 1
        else:
            self.rtx = "restarted"

    def _output(self) -> None:
        self.outputs += 1

    # ---- tcp.hh:1215-1575 for a tcb past the handshake
    def input(self, s: Seg, now: int) -> str:
        """One segment; returns the branch by which it leaves the straight
        path, "advance" for the straight path itself."""
        if self.state == "CLOSED":
            return "closed"
        seg_len, seq = s.pay_len, s.seq
        if not self.segment_acceptable(seq, seg_len):
            self._output()
            return "unacceptable"
        if lt(seq, self.rcv_next):
            dup = min((self.rcv_next - seq) & M32, seg_len)
            seg_len -= dup
            seq = (seq + dup) & M32
        if seq != self.rcv_next:
            self._output()
            return "out_of_order"
        if s.flags & RST:
            self.state = "CLOSED"
            return "rst"
        if s.flags & SYN:
            self.state = "CLOSED"
            return "syn"
        if not s.flags & ACK:
            return "no_ack"
        branch = "old_ack"
        do_output = do_output_data = False
        if self.state in ("ESTABLISHED", "CLOSE_WAIT"):
            packets_out = (self.next - self.una - self.zero_window_probing_out) & M32
            if lt(self.una, s.ack) and le(s.ack, self.next):
                acked = self.data_segment_acked(s.ack, now)
                updated = lt(self.wl1, seq) or (self.wl1 == seq and le(self.wl2, s.ack))
                if updated:
                    self._update_window(s)
                do_output_data = True
                branch = "advance"
                if self.dupacks >= 3:
                    branch = "fast_recovery"
                    if lt(self.recover, s.ack):
                        flight = sum(e.len for e in self.data) & M32
                        self.cwnd = min(self.ssthresh, (max(flight, self.mss) + self.mss) & M32)
                        self.dupacks = self.limited_transfer = self.partial_ack = 0
                        self._set_retransmit_timer()
                    else:
                        self._output()   # fast_retransmit
                        self.cwnd = (self.cwnd - acked) & M32
                        if acked >= self.mss:
                            self.cwnd = (self.cwnd + self.mss) & M32
                        self.partial_ack += 1
                        if self.partial_ack == 1:
                            self.rtx = "restarted"
                else:
                    self.dupacks = self.limited_transfer = self.partial_ack = 0   # exit_fast_recovery
                    self._set_retransmit_timer()
                    if not updated:
                        branch = "advance_window_kept"
                    elif self.window == 0:
                        branch = "advance_window_closed"
            elif (packets_out > 0 and self.data and seg_len == 0 and not s.flags & (FIN | SYN) and s.ack == self.una
                  and ((s.window << self.window_scale) & M32) == self.window):
                branch = "dupack"
                self.dupacks += 1
                if self.dupacks in (1, 2):
                    do_output_data = True
                elif self.dupacks == 3:
                    if lt(self.recover, (s.ack - 1) & M32):
                        self.recover = (self.next - 1) & M32
                        flight = sum(e.len for e in self.data) & M32
                        self.ssthresh = max(((flight - self.limited_transfer) & M32) // 2, 2 * self.mss)
                        self._output()   # fast_retransmit
                    self.cwnd = (self.ssthresh + 3 * self.mss) & M32
                else:
                    self.cwnd = (self.cwnd + self.mss) & M32
                    do_output_data = True
            elif lt(self.next, s.ack):
                self._output()
                return "ack_beyond_next"
            elif self.window == 0 and s.window > 0:
                self._update_window(s)
                do_output_data = True
                branch = "window_reopened"
        if s.flags & URG:
            branch = branch if branch != "advance" else "urg"
        if self.state == "ESTABLISHED":
            if seg_len:
                self.text += seg_len
                self.rcv_next = (self.rcv_next + seg_len) & M32
                do_output = True   # the delayed-ACK rule is the receive path's (tests/tcp_data_model.py)
                branch = "text" if branch in ("advance", "old_ack") else branch
        elif self.state == "CLOSE_WAIT":
            return branch   # tcp.hh:1522-1526: before the FIN step and the closing output()
        if s.flags & FIN:
            if ((seq + seg_len) & M32) == self.rcv_next:
                self.rcv_next = (self.rcv_next + 1) & M32
                do_output = False
                self._output()
                if self.state == "ESTABLISHED":
                    self.state = "CLOSE_WAIT"
            branch = "fin"
        if do_output or (do_output_data and self.can_send()):
            self._output()
        return branch


# ---------------------------------------------------------------- the rule of sccsum.h on top of the walk

def conn_stop(t: Tcb, eligible: bool = True, lens=None) -> int:
    """The connection-level stops.  `lens`: the queue as the device is given it
    (defaults to the tcb's own)."""
    lens = [e.len for e in t.data] if lens is None else lens
    if (not eligible or t.window == 0 or t.cwnd == 0 or t.cwnd >= 1 << 31 or t.window_scale > 14
            or lt(t.next, t.una)):
        return STOP_INELIGIBLE
    if sum(lens) != ((t.next - t.una) & M32) or 0 in lens:
        return STOP_QUEUE
    return 0


def seg_stop(t: Tcb, prev: int, s: Seg, head: bool) -> int:
    """The per-segment stops, in the table's order; t is the tcb AS GIVEN."""
    if s.seq != t.rcv_next:
        return STOP_SEQ
    if (s.flags & 0x37) != 0x10:
        return STOP_FLAGS
    if s.pay_len != 0:
        return STOP_DATA
    if not (lt(prev, s.ack) and le(s.ack, t.next)):
        return STOP_ACK
    if head and not (lt(t.wl1, s.seq) or (t.wl1 == s.seq and le(t.wl2, s.ack))):
        return STOP_WL
    if ((s.window << t.window_scale) & M32) == 0:
        return STOP_WINDOW
    return 0


def host_eligible(t: Tcb) -> bool:
    """When the host sets SCCSUM_TCP_ACK_ELIGIBLE."""
    return (t.state in ("ESTABLISHED", "CLOSE_WAIT") and t.dupacks < 3 and not t.window_probe
            and t.zero_window_probing_out == 0 and t.window != 0 and t.window_scale <= 14)


def in_flags(t: Tcb) -> int:
    return ((ELIGIBLE if host_eligible(t) else 0) | (CLOSE_WAIT if t.state == "CLOSE_WAIT" else 0)
            | (FIRST_SAMPLE if t.first_rto_sample else 0))


def expect_run(t: Tcb, segs, now: int, eligible=None, lens=None):
    """One run: (record as a dict, the tcb after the taken ACKs).  Every taken
    segment goes through Tcb.input() and must take the straight path."""
    eligible = host_eligible(t) if eligible is None else eligible
    after = copy.deepcopy(t)
    stop, taken, poll = conn_stop(t, eligible, lens), 0, False
    if not stop:
        prev = t.una
        for k, s in enumerate(segs):
            stop = seg_stop(t, prev, s, k == 0)
            if stop:
                break
            before = after.outputs
            branch = after.input(s, now)
            assert branch == "advance", branch
            poll |= after.outputs != before
            prev = s.ack
            taken += 1
    flags = FIRST_SAMPLE if after.first_rto_sample else 0
    if taken:
        flags |= (ALL_ACKED if not after.data else RTX_REARM) | (POLL if poll else 0)
    rec = dict(taken=taken, una=after.una, acked=(after.una - t.una) & M32, popped=after.popped, trim=after.trim,
               queue_freed=after.queue_freed & M32, window=after.window, cwnd=after.cwnd, srtt=after.srtt,
               rttvar=after.rttvar, rto=after.rto, flags=flags, stop=stop)
    return rec, after


def apply(t: Tcb, rec: dict) -> Tcb:
    """What the host does with a run record: the tcb after the taken ACKs,
    from the record alone (and its own queue)."""
    t = copy.deepcopy(t)
    if not rec["taken"]:
        return t
    for _ in range(rec["popped"]):
        t.data.popleft()
    if rec["trim"]:
        t.data[0].len -= rec["trim"]
    t.una, t.window, t.cwnd = rec["una"], rec["window"], rec["cwnd"]
    t.wl1, t.wl2 = t.rcv_next, rec["una"]   # every taken ACK has seq == rcv_next; the last one's ack is una
    t.srtt, t.rttvar, t.rto = rec["srtt"], rec["rttvar"], rec["rto"]
    t.first_rto_sample = bool(rec["flags"] & FIRST_SAMPLE)
    t.dupacks = t.limited_transfer = t.partial_ack = 0
    t.zero_window_probing_out = 0
    t.persist = "stopped"                              # update_window with a window that is not 0
    t.rtx = "stopped" if rec["flags"] & ALL_ACKED else "restarted"
    t.all_acked += 1 if rec["flags"] & ALL_ACKED else 0
    return t
