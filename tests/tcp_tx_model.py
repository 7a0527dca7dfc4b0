"""The reference's transmit chain for one tcb, per segment, over Python ints
and deques of bytes (paths relative to the reference tree):

  tcb::get_packet's continuation   include/seastar/net/tcp.hh:2089-2111
  tcb::can_send                    tcp.hh:515-549, all of it: the window probe,
                                   limited transmit (dupacks 1 or 2) and the
                                   dupacks >= 3 branch too
  tcb::get_transmit_packet         tcp.hh:1578-1606: whole buffers while they
                                   fit, then share(0, rest) of the next one
  tcb::output_one                  tcp.hh:1609-1718: seq, ack, the window, the
                                   flags, the retransmit timer, _snd.data

chain(t, hw) runs one trip: output() put the tcb into the poll set, and
get_packet() is called for it until it no longer calls output() itself.  It
yields the segments as (seq, payload bytes, piece list) and leaves the tcb as
the reference would.  closed_form(t, hw) is what sccsum_tcp_tx_data computes
instead (include/sccsum.h, "TCP transmit fast path"); tests/test_tcp_tx_fast.py
compares the two on seeded sweeps.

The chain as the reference has it need not end: with _snd.mss == 0 (and
cwnd > 0, data and window) every get_packet() sends an empty segment and
can_send() stays positive.  chain() stops at `limit` segments and says so.
"""
from __future__ import annotations

import copy
from collections import deque
from dataclasses import dataclass, field

M32 = 0xFFFFFFFF
ESTABLISHED, CLOSE_WAIT = "ESTABLISHED", "CLOSE_WAIT"
ELIGIBLE, RTX_ARMED, RTX_ARM = 0x01, 0x02, 0x04
STOP_END, STOP_INELIGIBLE, STOP_WINDOW, STOP_CAPACITY, STOP_QUEUE = 0, 1, 2, 7, 8
ACK = 0x10


@dataclass
class Hw:
    """hw_features() as get_transmit_packet reads it."""
    mtu: int = 1500
    tx_tso: bool = False
    max_packet_len: int = 65535

    def seg_len(self, mss: int) -> int:
        if self.tx_tso:
            return self.max_packet_len - 40
        return min((self.mtu - 40) & 0xFFFF, mss)     # uint16_t(mtu - 20 - 20)


@dataclass
class Tcb:
    state: str = ESTABLISHED
    dst: int = 0x0A000002
    sport: int = 5000
    dport: int = 80
    snd_next: int = 1000
    snd_unacknowledged: int = 1000
    snd_window: int = 65535
    cwnd: int = 14600
    mss: int = 1460
    dupacks: int = 0
    window_probe: bool = False
    limited_transfer: int = 0
    rcv_next: int = 77
    rcv_window: int = 29200
    window_scale: int = 0
    rtx_armed: bool = False
    packetq: int = 0                                # packets already queued
    unsent: deque = field(default_factory=deque)    # of bytes; the model's buffer j is (id j, its bytes)
    unsent_len: int = 0
    data: list = field(default_factory=list)        # _snd.data: (seq, payload) per unacked_segment
    _ids: deque = field(default_factory=deque)      # (buffer index, bytes already taken from it)
    _popped: int = 0                                # buffers that have left the queue

    def queue(self, bufs) -> "Tcb":
        """connection::send for each buffer: _snd.unsent.push_back, unsent_len += len (a uint32_t)."""
        for b in bufs:
            self._ids.append([len(self._ids) + self._popped, 0])
            self.unsent.append(bytes(b))
            self.unsent_len = (self.unsent_len + len(b)) & M32
        return self

    # ---- tcp.hh:550-554
    def flight_size(self) -> int:
        return sum(len(p) for _, p in self.data) & M32

    # ---- tcp.hh:515-549
    def can_send(self) -> int:
        if self.window_probe:
            return 1
        if self.snd_window == 0:
            return 0
        window_used = (self.snd_next - self.snd_unacknowledged) & M32
        if window_used > self.snd_window:
            return 0
        x = min(self.snd_window - window_used, self.unsent_len)
        x = min(self.cwnd, x)
        if self.dupacks in (1, 2):
            flight = self.flight_size()
            most = (self.cwnd + 2 * self.mss) & M32
            x = min(x, most - flight) if flight <= most else 0
            self.limited_transfer = (self.limited_transfer + x) & M32
        elif self.dupacks >= 3:
            x = min(self.mss, x)
        return x

    # ---- tcp.hh:1578-1606; returns the payload and its pieces (buffer, inner offset, length)
    def get_transmit_packet(self, hw: Hw):
        if not self.unsent:
            return b"", []
        can = min(self.can_send(), hw.seg_len(self.mss))
        out, pieces = [], []
        while self.unsent and len(self.unsent[0]) <= can:
            front = self.unsent.popleft()
            ident = self._ids.popleft()
            self._popped += 1
            can -= len(front)
            out.append(front)
            if front:                                # an empty fragment changes nothing on the wire
                pieces.append((ident[0], ident[1], len(front)))
        if self.unsent and can:
            q = self.unsent[0]
            out.append(q[:can])                      # q.share(0, can_send)
            pieces.append((self._ids[0][0], self._ids[0][1], can))
            self.unsent[0] = q[can:]                 # q.trim_front(can_send)
            self._ids[0][1] += can
        p = b"".join(out)
        self.unsent_len = (self.unsent_len - len(p)) & M32
        return p, pieces

    def syn_needs_on(self) -> bool:
        return self.state in ("SYN_SENT", "SYN_RECEIVED")

    def fin_needs_on(self) -> bool:                  # tcp.hh:631-636, with an empty queue only
        return self.state in ("FIN_WAIT_1", "CLOSING", "LAST_ACK") and not self.unsent

    def ack_needs_on(self) -> bool:
        return self.state not in ("CLOSED", "LISTEN", "SYN_SENT")

    # ---- tcp.hh:1609-1718 (data_retransmit false)
    def output_one(self, hw: Hw):
        p, pieces = self.get_transmit_packet(hw)
        length = len(p) & 0xFFFF                     # uint16_t len = p.len()
        seq = self.snd_next
        self.snd_next = (self.snd_next + length) & M32
        seg = dict(seq=seq, ack=self.rcv_next, window=(self.rcv_window >> self.window_scale) & 0xFFFF,
                   flags=(ACK if self.ack_needs_on() else 0) | (0x02 if self.syn_needs_on() else 0)
                   | (0x01 if self.fin_needs_on() else 0), hdr_len=20, payload=p, pieces=pieces, dst=self.dst,
                   sport=self.sport, dport=self.dport, mss=self.mss, armed_here=False)
        if length or self.syn_needs_on() or self.fin_needs_on():
            if length:
                self.data.append((seq, p))
            if not self.rtx_armed:
                self.rtx_armed = True
                seg["armed_here"] = True
        assert self.snd_window > 0 or length <= 1    # tcp.hh:1716
        return seg

    # ---- tcp.hh:2089-2111; returns (the packet, whether output() was called again)
    def get_packet(self, hw: Hw):
        sent = None
        if self.packetq == 0:
            sent = self.output_one(hw)
        else:
            self.packetq -= 1
        again = self.packetq > 0 or (self.dupacks < 3 and self.can_send() > 0 and self.snd_window > 0)
        return sent, again

    def why_not_eligible(self):
        """Which of the closed form's premises the tcb misses; None when it holds them all."""
        if self.state not in (ESTABLISHED, CLOSE_WAIT):
            return "state"
        if self.dupacks in (1, 2):
            return "limited_transmit"
        if self.dupacks >= 3:
            return "fast_retransmit"
        if self.window_probe:
            return "window_probe"
        if self.packetq:
            return "packetq"
        return None

    def flags(self) -> int:
        return (0 if self.why_not_eligible() else ELIGIBLE) | (RTX_ARMED if self.rtx_armed else 0)


def chain(t: Tcb, hw: Hw, limit: int = 1 << 22):
    """One trip through the poll set: the segments sent, and whether the chain
    was cut at `limit` (the reference's would have gone on)."""
    segs = []
    while True:
        seg, again = t.get_packet(hw)
        if seg is not None:
            segs.append(seg)
        if not again:
            return segs, False
        if len(segs) >= limit:
            return segs, True


@dataclass
class Run:
    segs: int
    bytes: int
    next: int
    flags: int
    stop: int
    seq: list
    length: list


def closed_form(t: Tcb, hw: Hw, unsent_len: int | None = None) -> Run:
    """What sccsum_tcp_tx_data computes for the tcb's record: sccsum.h's rule."""
    u = sum(len(b) for b in t.unsent) if unsent_len is None else unsent_len
    if t.why_not_eligible():
        return Run(0, 0, t.snd_next, 0, STOP_INELIGIBLE, [], [])
    if u > M32:
        return Run(0, 0, t.snd_next, 0, STOP_QUEUE, [], [])
    used = (t.snd_next - t.snd_unacknowledged) & M32
    can = 0 if t.snd_window == 0 or used > t.snd_window else min(t.snd_window - used, u)
    p = min(t.cwnd, hw.seg_len(t.mss))
    sent = can if p else 0
    if sent == 0:
        seq, length = [t.snd_next], [0]
    else:
        n = -(-sent // p)
        seq = [(t.snd_next + k * p) & M32 for k in range(n)]
        length = [min(p, sent - k * p) for k in range(n)]
    arm = RTX_ARM if sent and not t.rtx_armed else 0
    return Run(len(seq), sent, (t.snd_next + sent) & M32, arm, STOP_END if sent == u else STOP_WINDOW, seq, length)


def pieces_of(bufs, start: int, length: int) -> list:
    """The (buffer, inner offset, length) overlaps of stream bytes [start,
    start + length) with the buffers, those of no bytes left out."""
    out, at = [], 0
    for j, b in enumerate(bufs):
        n = len(b) if not isinstance(b, int) else b
        lo, hi = max(at, start), min(at + n, start + length)
        if n and lo < hi:
            out.append((j, lo - at, hi - lo))
        at += n
    return out


def continue_from(t: Tcb, run: Run) -> Tcb:
    """The tcb the host holds after it applied a run record: the queue popped
    by run.bytes, next and the timer from the record, one _snd.data entry per
    segment with bytes.  What it then does itself starts from here."""
    t = copy.deepcopy(t)
    stream = b"".join(t.unsent)
    left, at = run.bytes, 0
    for s, n in zip(run.seq, run.length):
        if n:
            t.data.append((s, stream[at:at + n]))
            at += n
    while left and t.unsent:
        front = t.unsent[0]
        if len(front) <= left:
            left -= len(front)
            t.unsent.popleft()
            t._ids.popleft()
            t._popped += 1
        else:
            t.unsent[0] = front[left:]
            t._ids[0][1] += left
            left = 0
    t.unsent_len = (t.unsent_len - run.bytes) & M32
    t.snd_next = run.next
    if run.flags & RTX_ARM:
        t.rtx_armed = True
    return t
