"""The reference's passive open, one segment at a time over Python ints and
bytes (paths relative to the reference tree):

  received   tcp::received for a segment whose connid has no tcb: the listener
             found, full() -> respond_with_reset; else RST dropped, ACK ->
             respond_with_reset, SYN -> a tcb is made, put into _tcbs,
             inc_pending(), input_handle_listen_state; else dropped
                                                include/seastar/net/tcp.hh:888-929
  listen     input_handle_listen_state: irs, do_setup_isn, init_from_options,
             do_syn_received -> output_one's SYN-ACK     tcp.hh:1115-1141, 1079-1112
  parse      tcp_option::parse, its fixed advances included    src/net/tcp.cc:34-79
  fill       tcp_option::fill / get_size for SYN|ACK            tcp.cc:81-138
  get_isn    MD5 over {local_ip, foreign_ip, (local_port << 16) + foreign_port}
             and the 64 key bytes, its first word + microseconds / 4
                                                               tcp.hh:2067-2086

Stack holds a real dict for _tcbs and a Listener per port with the counters
full() reads.  walk() feeds it a LISTEN bucket in arrival order and names the
branch every segment takes; the first segment that finds a tcb made by the
same walk is where the batch interface stops (`taken`, include/sccsum.h, "TCP
passive open"): from there on the classes are LATER.  Where parse would read a
byte at or past opt_end the reference's behaviour is undefined; parse(strict=
True) raises there, parse(strict=False) is the interface's definition: the
parse ends and keeps what it had.  Nothing here reads the code under test."""
from __future__ import annotations

import hashlib
import struct
from dataclasses import dataclass, field

import numpy as np

import tcp_model as tm

FIN, SYN, RST, PSH, ACK, URG = tm.FIN, tm.SYN, tm.RST, tm.PSH, tm.ACK, tm.URG
M32 = 0xFFFFFFFF
NEW, RESET, DROP, LATER = 0, 1, 2, 3
F_MSS, F_WSCALE, F_SACK, F_BIG = 1, 2, 4, 8
RCV_WINDOW = 29200
NEW_DTYPE = np.dtype([("local_ip", "<u4"), ("foreign_ip", "<u4"), ("local_port", "<u2"), ("foreign_port", "<u2"),
                      ("pos", "<u4"), ("irs", "<u4"), ("iss", "<u4"), ("snd_window", "<u4"), ("cwnd", "<u4"),
                      ("ssthresh", "<u4"), ("rcv_window", "<u4"), ("wl1", "<u4"), ("wl2", "<u4"), ("snd_mss", "<u2"),
                      ("local_mss", "<u2"), ("snd_wscale", "u1"), ("rcv_wscale", "u1"), ("flags", "u1"), ("pad", "u1"),
                      ("reserved", "<u4", (2,))])
OUT_DTYPE = np.dtype([("dst", "<u4"), ("seq", "<u4"), ("ack", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
                      ("window", "<u2"), ("flags", "u1"), ("hdr_len", "u1"), ("mss", "<u4")])
BRANCH_CLASS = dict(full_reset=RESET, full_rst=DROP, listen_rst=DROP, listen_ack=RESET, listen_syn=NEW,
                    listen_other=DROP)


class PastEnd(Exception):
    """tcp_option::parse would read a byte at or past opt_end."""


@dataclass
class Seg:
    """A segment of the LISTEN bucket as tcp::received sees it: from = foreign_ip, to = local_ip."""
    local_ip: int
    foreign_ip: int
    local_port: int
    foreign_port: int
    seq: int = 0
    ack: int = 0
    flags: int = SYN
    window: int = 1000
    options: bytes = b""
    pay_len: int = 0

    @property
    def connid(self) -> tuple:
        return (self.local_ip, self.foreign_ip, self.local_port, self.foreign_port)


# ---------------------------------------------------------------- tcp_option

@dataclass
class Option:
    """tcp_option's members (tcp.hh:183-192)."""
    mss_received: bool = False
    win_scale_received: bool = False
    sack_received: bool = False
    remote_mss: int = 536
    local_mss: int = 0
    remote_win_scale: int = 0
    local_win_scale: int = 0


def parse(opt: bytes, strict: bool = False) -> Option:
    """tcp.cc:34-79 over opt[beg .. end)."""
    o = Option()
    beg, end = 0, len(opt)

    def at(k: int) -> int:
        if k >= end:
            raise PastEnd(k)
        return opt[k]

    try:
        while beg < end:
            kind = opt[beg]
            if kind not in (1, 0):                     # not nop, not eol
                length = at(beg + 1)
                if beg + length > end:
                    return o
            if kind == 2:                              # mss
                value = (at(beg + 2) << 8) | at(beg + 3)
                o.mss_received, o.remote_mss = True, value
                beg += 4
            elif kind == 3:                            # win_scale
                value = at(beg + 2)
                o.win_scale_received, o.remote_win_scale, o.local_win_scale = True, value, 7
                beg += 3
            elif kind == 4:                            # sack
                o.sack_received = True
                beg += 2
            elif kind == 1:
                beg += 1
            elif kind == 0:
                return o
            else:
                length = at(beg + 1)
                beg += length
                if length == 0:
                    return o
    except PastEnd:
        if strict:
            raise
    return o


def get_size(o: Option, syn_on: bool, ack_on: bool) -> int:
    """tcp.cc:122-138."""
    size = 0
    if syn_on:
        if o.mss_received or not ack_on:
            size += 4
        if o.win_scale_received or not ack_on:
            size += 3
    if size > 0:
        size += 1
        size = (size + 3) & ~3
    return size


def fill(o: Option, syn_on: bool, ack_on: bool) -> bytes:
    """tcp.cc:81-120: the option bytes behind the twenty fixed ones."""
    out = b""
    if syn_on:
        if o.mss_received or not ack_on:
            out += bytes([2, 4]) + struct.pack(">H", o.local_mss)
        if o.win_scale_received or not ack_on:
            out += bytes([3, 3, o.local_win_scale])
    size = len(out)
    if size > 0:
        size_max = (size + 1 + 3) & ~3
        while size < size_max - 1:
            out += bytes([1])
            size += 1
        out += bytes([0])
        size += 1
    assert size == get_size(o, syn_on, ack_on) == len(out)
    return out


def get_isn(connid: tuple, key: bytes, isn_m: int) -> int:
    """tcp.hh:2067-2086 with m.count() / 4 given."""
    lip, fip, lp, fp = connid
    assert len(key) == 64
    digest = hashlib.md5(struct.pack("<III", lip, fip, ((lp << 16) + fp) & M32) + key).digest()
    return (struct.unpack("<I", digest[:4])[0] + isn_m) & M32


# ---------------------------------------------------------------- the tcb of a passive open

@dataclass
class Tcb:
    connid: tuple
    state: str = "CLOSED"
    irs: int = 0
    rcv_next: int = 0
    iss: int = 0
    snd_una: int = 0
    snd_next: int = 0
    snd_mss: int = 536
    local_mss: int = 0
    snd_wscale: int = 0
    rcv_wscale: int = 0
    snd_window: int = 0
    rcv_window: int = 0
    cwnd: int = 0
    ssthresh: int = 0
    wl1: int = 0
    wl2: int = 0
    option: Option = field(default_factory=Option)
    wscale_big: bool = False
    synack: dict | None = None

    def input_handle_listen_state(self, s: Seg, key: bytes, isn_m: int, mtu: int, strict: bool) -> None:
        self.rcv_next, self.irs = (s.seq + 1) & M32, s.seq              # tcp.hh:1123-1124
        self.iss = get_isn(self.connid, key, isn_m)                      # do_setup_isn
        self.snd_una, self.snd_next = self.iss, (self.iss + 1) & M32
        o = self.option = parse(s.options, strict)                       # init_from_options
        self.snd_wscale, self.rcv_wscale = o.remote_win_scale, o.local_win_scale
        self.snd_mss = o.remote_mss
        self.local_mss = o.local_mss = (mtu - 40) & 0xFFFF
        self.rcv_window = RCV_WINDOW << self.rcv_wscale
        # uint16 << shift is undefined from some values on: the interface keeps the window unshifted above 14
        self.wscale_big = self.snd_wscale > 14
        self.snd_window = s.window if self.wscale_big else s.window << self.snd_wscale
        self.wl1, self.wl2 = s.seq, s.ack
        if 2190 < self.snd_mss:
            self.cwnd = 2 * self.snd_mss
        elif 1095 < self.snd_mss <= 2190:
            self.cwnd = 3 * self.snd_mss
        else:
            self.cwnd = 4 * self.snd_mss
        self.ssthresh = self.snd_window
        self.state = "SYN_RECEIVED"                                      # do_syn_received -> output()
        options = fill(o, True, True)
        lip, fip, lp, fp = self.connid
        self.synack = dict(dst=fip, seq=self.iss, ack=self.rcv_next, sport=lp, dport=fp,
                           window=(self.rcv_window >> self.rcv_wscale) & 0xFFFF, flags=SYN | ACK,
                           hdr_len=20 + len(options), mss=self.snd_mss, options=options)


@dataclass
class Listener:
    """tcp::listener's counters (tcp.hh:745-790): full() is _pending + _q.size() >= max_size."""
    max_size: int
    pending: int = 0
    q: int = 0

    def full(self) -> bool:
        return self.pending + self.q >= self.max_size


class Stack:
    """_tcbs, _listening and the answers of one tcp."""

    def __init__(self, listeners: dict, key: bytes, isn_m: int, mtu: int, offload: bool = False):
        self.tcbs: dict = {}
        self.listening = listeners
        self.key, self.isn_m, self.mtu, self.offload = key, isn_m, mtu, offload
        self.resets: list = []

    def received(self, s: Seg, strict: bool = False) -> str:
        """tcp.hh:884-942 for a segment of the LISTEN bucket: the branch it takes."""
        cid = s.connid
        if cid in self.tcbs:
            return "tcb"                                # input_handle_other_state: not this layer's
        listener = self.listening.get(s.local_port)
        h = dict(sport=s.foreign_port, dport=s.local_port, seq=s.seq, ack=s.ack, flags=s.flags)
        if listener is None or listener.full():
            answer = tm.respond_with_reset(h, s.local_ip, s.foreign_ip, self.offload)
            if answer is None:
                return "full_rst"
            self.resets.append((answer, s.foreign_ip))
            return "full_reset"
        if s.flags & RST:
            return "listen_rst"
        if s.flags & ACK:
            self.resets.append((tm.respond_with_reset(h, s.local_ip, s.foreign_ip, self.offload), s.foreign_ip))
            return "listen_ack"
        if s.flags & SYN:
            t = Tcb(cid)
            self.tcbs[cid] = t
            listener.pending += 1                       # inc_pending
            t.input_handle_listen_state(s, self.key, self.isn_m, self.mtu, strict)
            return "listen_syn"
        return "listen_other"


def walk(segs: list, space: dict, key: bytes, isn_m: int, mtu: int, offload: bool = False, strict: bool = False) -> dict:
    """The bucket through Stack.received up to the first segment that meets a
    tcb of this batch.  space: {port: room}, a listener's max_size - (_pending
    + _q.size()) at the start; every dport of the bucket listens (tcp_rx put
    it there), with room 0 when space does not name it."""
    listeners = {s.local_port: Listener(max_size=int(space.get(s.local_port, 0))) for s in segs}
    st = Stack(listeners, key, isn_m, mtu, offload)
    branches, created = [], []
    taken = len(segs)
    for i, s in enumerate(segs):
        b = st.received(s, strict)
        if b == "tcb":
            taken = i
            break
        branches.append(b)
        if b == "listen_syn":
            created.append((i, st.tcbs[s.connid]))
    return dict(branches=branches, taken=taken, created=created, resets=st.resets, stack=st)


def record(pos: int, t: Tcb) -> tuple:
    """sccsum_tcp_new of a created tcb."""
    o = t.option
    flags = (F_MSS if o.mss_received else 0) | (F_WSCALE if o.win_scale_received else 0) | \
        (F_SACK if o.sack_received else 0) | (F_BIG if t.wscale_big else 0)
    lip, fip, lp, fp = t.connid
    return (lip, fip, lp, fp, pos, t.irs, t.iss, t.snd_window, t.cwnd, t.ssthresh, t.rcv_window, t.wl1, t.wl2, t.snd_mss,
            t.local_mss, t.snd_wscale, t.rcv_wscale, flags, 0, (0, 0))


def expect(segs: list, space: dict, key: bytes, isn_m: int, mtu: int, offload: bool = False, strict: bool = False) -> dict:
    """Every array sccsum_tcp_listen writes for the bucket.  synack: the
    twelve bytes [32 k + 20, 32 k + 32) of every slot (the options, then 0)."""
    w = walk(segs, space, key, isn_m, mtu, offload, strict)
    m, taken = len(segs), w["taken"]
    cls = np.array([BRANCH_CLASS[b] for b in w["branches"]] + [LATER] * (m - taken), dtype=np.uint8)
    k = len(w["created"])
    new = np.zeros(k, dtype=NEW_DTYPE)
    out = np.zeros(k, dtype=OUT_DTYPE)
    synack = np.zeros((k, 12), dtype=np.uint8)
    sa_off = np.zeros(k, dtype=np.uint64)
    for j, (pos, t) in enumerate(w["created"]):
        new[j] = record(pos, t)
        s = t.synack
        out[j] = (s["dst"], s["seq"], s["ack"], s["sport"], s["dport"], s["window"], s["flags"], s["hdr_len"], s["mss"])
        synack[j, :len(s["options"])] = np.frombuffer(s["options"], np.uint8)
        sa_off[j] = 32 * j + s["hdr_len"]
    rst = np.frombuffer(b"".join(a for a, _ in w["resets"]), dtype=np.uint8)
    resets = len(w["resets"])
    return dict(cls=cls, new=new, synack=synack, sa_off=sa_off, sa_len=np.zeros(k, dtype=np.uint32), sa_out=out, rst=rst,
                rst_dst=np.array([d for _, d in w["resets"]], dtype=np.uint32),
                total=np.array([taken, k, resets, taken - k - resets], dtype=np.uint64), walk=w)
