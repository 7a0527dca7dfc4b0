"""LISTEN buckets for tests/test_gpu_tcp_listen.py and the host tests: segments
written out by hand for every row of the rule's table, the duplicate-connid
cases and every option layout; seeded buckets of any size; connids whose home
slots collide and wrap in the de-duplication table; and the same buckets as
the arrays sccsum_tcp_rx leaves (arrays) or as wire frames (frames).

DEVIATES names the hand-written cases in which tcp_option::parse would read at
or past opt_end, where the interface defines the outcome (the parse ends);
every other case parses under parse(strict=True): check_strict."""
from __future__ import annotations

import numpy as np

import stack_model as sm
import tcp_listen_model as lm
import tcp_model as tm
import tcp_traffic
from tcp_listen_model import ACK, FIN, M32, PSH, RST, SYN, URG, Seg

HOST = sm.HOST
KEY = bytes((37 * k + 11) & 0xFF for k in range(64))
ISN_M = 0xFFFFFF00                     # the sum with the digest wraps for most connids
MTU = 1500
TILE = 1024
PEER = 0x0A000110
AMPLE = 1 << 20

NOP, EOL = b"\x01", b"\x00"


def mss_opt(v: int) -> bytes:
    return bytes([2, 4, v >> 8, v & 0xFF])


def ws_opt(shift: int) -> bytes:
    return bytes([3, 3, shift])


SACK_OK = bytes([4, 2])
TSTAMP = bytes([8, 10]) + bytes(range(8))


def pad4(opt: bytes, with_byte: bytes = NOP) -> bytes:
    return opt + with_byte * (-len(opt) % 4)


def syn(k: int, port: int = 80, flags: int = SYN, options: bytes = b"", **kw) -> Seg:
    """A segment of peer k: distinct k are distinct connids."""
    return Seg(HOST, PEER + (k >> 12), port, 1024 + (k & 0xFFF), seq=kw.pop("seq", 1000 + 7 * k), ack=kw.pop("ack", 5 * k),
               flags=flags, window=kw.pop("window", 1000 + k), options=options, **kw)


# ---------------------------------------------------------------- written out by hand

def table_case() -> tuple:
    """Every row of the table with space 0, 1 and 3: (segs, space, the classes by hand)."""
    N, R, D = lm.NEW, lm.RESET, lm.DROP
    rows = [
        # port 82 has no room from the start
        (syn(0, 82), R), (syn(1, 82, RST), D), (syn(2, 82, ACK), R), (syn(3, 82, 0), R), (syn(4, 82, SYN | RST), D),
        # port 80, room for one: before it fills
        (syn(10, 80, RST), D), (syn(11, 80, ACK), R), (syn(12, 80, 0), D), (syn(13, 80, FIN | PSH), D),
        (syn(14, 80, RST | ACK), D), (syn(15, 80, SYN | ACK), R), (syn(16, 80, SYN | RST), D),
        (syn(17, 80, SYN), N),
        # ... and behind
        (syn(18, 80, SYN), R), (syn(19, 80, RST), D), (syn(20, 80, ACK), R), (syn(21, 80, 0), R), (syn(22, 80, FIN), R),
        (syn(23, 80, SYN | RST), D),
        # port 81, room for three: FIN, PSH, URG and a payload do not matter
        (syn(30, 81, SYN | FIN), N), (syn(31, 81, SYN, pay_len=9), N), (syn(32, 81, ACK), R),
        (syn(33, 81, SYN | PSH | URG, pay_len=3), N), (syn(34, 81, SYN), R), (syn(35, 81, RST), D),
        # another local address on port 80 is the same listener
        (Seg(sm.OTHER_HOST, PEER, 80, 999, flags=SYN), R),
        # port 83 never fills
        (syn(40, 83, SYN), N), (syn(41, 83, RST | ACK), D), (syn(42, 83, SYN | FIN | PSH | URG), N),
    ]
    return [s for s, _ in rows], {80: 1, 81: 3, 82: 0, 83: 5}, [c for _, c in rows]


def duplicate_cases() -> dict:
    """name -> (segs, space, taken, the classes before taken by hand)."""
    N, R, D = lm.NEW, lm.RESET, lm.DROP
    a, b, c = syn(1), syn(2), syn(3)
    return {
        # a duplicate SYN of a created connid: the stop
        "dup_created": ([a, b, syn(4, flags=ACK), a, c, syn(5)], {80: 9}, 3, [N, N, R]),
        # a duplicate SYN of a connid refused because the port was full: no stop, a second RST
        "dup_refused": ([a, b, b, c, b, syn(6, flags=RST)], {80: 1}, 6, [N, R, R, R, R, D]),
        # ineligible segments of a connid before its candidate, then one behind it
        "ineligible_first": ([syn(1, flags=ACK), syn(1, flags=RST), syn(1, flags=0), a, b, syn(1, flags=ACK), c],
                             {80: 9}, 5, [R, D, D, N, N]),
        # an RST chasing its SYN
        "rst_chases": ([a, syn(1, flags=RST), b], {80: 9}, 1, [N]),
        # the duplicate is the bucket's last segment; a refused candidate's duplicate on a port without room
        "dup_last": ([syn(7, 82), syn(7, 82), a, b, a], {80: 9, 82: 0}, 4, [R, R, N, N]),
        # the stop comes from the earliest such position, not from the earliest candidate
        "two_stops": ([a, b, c, c, a], {80: 9}, 3, [N, N, N]),
    }


# name -> the option bytes (a multiple of four)
OPTION_LAYOUTS = {
    "none": b"",
    "mss": mss_opt(1460),
    "ws": pad4(ws_opt(7)),
    "both": pad4(mss_opt(1460) + ws_opt(2)),
    "both_reversed": pad4(ws_opt(9) + mss_opt(9000), EOL),
    "linux": mss_opt(1460) + SACK_OK + TSTAMP + NOP + ws_opt(7),
    "sack_only": pad4(SACK_OK, EOL),
    "timestamp": pad4(TSTAMP + mss_opt(1200)),
    "unknown_kinds": pad4(bytes([30, 6, 1, 2, 3, 4]) + bytes([254, 2]) + mss_opt(700) + ws_opt(3)),
    "length_0": pad4(bytes([30, 0]) + mss_opt(700), EOL),          # ends the parse: the MSS behind is not seen
    "length_0_mss": bytes([2, 0, 5, 0xB4]),                        # the MSS's own length byte is not consulted
    "length_1_ws": bytes([3, 1, 5, 1]),
    "overrun": pad4(mss_opt(1400) + bytes([30, 9, 0, 0]) + ws_opt(4)),   # 4 + 9 > 12: the window scale is not seen
    "overrun_mss": pad4(ws_opt(1)) + bytes([2, 5, 1, 2]),         # an MSS that says 5 with 4 left: refused whole
    "eol_in_the_middle": mss_opt(1000) + EOL + ws_opt(5),
    "nops": NOP * 3 + mss_opt(536) + NOP + ws_opt(0) + NOP * 5,
    "sack_advance": bytes([4, 1]) + mss_opt(1460) + EOL * 2,      # SACK advances by 2 whatever its length byte says
    "forty": mss_opt(1460) + SACK_OK + TSTAMP + NOP + ws_opt(7) + NOP * 20,
    "forty_unknown": bytes([99, 40]) + bytes(38),
    "repeated": mss_opt(100) + mss_opt(200) + pad4(ws_opt(1) + ws_opt(2) + NOP * 2),
    "mss_0": mss_opt(0),
    "mss_65535_ws_14": pad4(mss_opt(65535) + ws_opt(14)),
    # the reference would read opt_end or beyond: the interface ends the parse there
    "kind_last": mss_opt(1300) + NOP * 3 + bytes([30]),
    "kind_last_mss": pad4(ws_opt(6)) + NOP * 3 + bytes([2]),
    "mss_value_cut": pad4(ws_opt(6)) + NOP + bytes([2, 3, 9]),      # length 3 fits, the second value byte does not
    "mss_value_cut_2": pad4(ws_opt(6)) + NOP * 2 + bytes([2, 2]),
    "ws_value_cut": mss_opt(1300) + NOP * 2 + bytes([3, 2]),
    "sack_last": mss_opt(1300) + NOP * 3 + bytes([4]),
}
DEVIATES = ("kind_last", "kind_last_mss", "mss_value_cut", "mss_value_cut_2", "ws_value_cut", "sack_last")
MSS_VALUES = (536, 1095, 1096, 2190, 2191)
SHIFTS = (0, 1, 14, 15, 16, 255)


def option_case() -> tuple:
    """One SYN per layout, per MSS band and per shift, each its own peer: (segs, space, names)."""
    segs, names = [], []
    for k, (name, opt) in enumerate(OPTION_LAYOUTS.items()):
        assert len(opt) % 4 == 0 and len(opt) <= 40, name
        segs.append(syn(100 + k, options=opt, window=0xFFFF if k % 2 else 1 + k))
        names.append(name)
    for k, v in enumerate(MSS_VALUES):
        segs.append(syn(200 + k, options=mss_opt(v)))
        names.append(f"mss_{v}")
    for k, sh in enumerate(SHIFTS):
        segs.append(syn(300 + k, options=pad4(ws_opt(sh)), window=(0xFFFF, 0x8000, 3)[k % 3]))
        names.append(f"shift_{sh}")
    return segs, {80: AMPLE}, names


def check_strict(segs: list, names: list) -> None:
    """No compared case outside DEVIATES reads past opt_end; every one in it does."""
    for s, name in zip(segs, names):
        try:
            lm.parse(s.options, strict=True)
            assert name not in DEVIATES, name
        except lm.PastEnd:
            assert name in DEVIATES, name


# ---------------------------------------------------------------- seeded buckets

PALETTE = [OPTION_LAYOUTS[n] for n in ("none", "mss", "ws", "both", "linux", "unknown_kinds", "eol_in_the_middle", "forty",
                                       "overrun", "length_0")]


def mixed(seed: int, m: int, ports=(80, 8080, 22), stop_at: int | None = None, fill_after: float = 0.6) -> tuple:
    """m segments: about three quarters SYNs of fresh peers with options of
    the palette, the rest RSTs, ACKs, flagless ones and repeats of connids that
    a full port refused (no stop).  Every port has room for about fill_after of
    its SYNs.  stop_at: that position repeats a created connid; nothing else
    stops.  Returns (segs, space)."""
    rng = np.random.default_rng(4200 + seed)
    ports = list(ports)
    space = {p: int(0.75 * m / len(ports) * fill_after) for p in ports}
    cands = {p: 0 for p in ports}
    segs, created, refused = [], [], []
    for i in range(m):
        port = ports[int(rng.integers(0, len(ports)))]
        kind = rng.random()
        seq, ack = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        if i == stop_at:
            assert created, "nothing created before stop_at"
            twin = created[len(created) // 2]
            segs.append(Seg(**{**twin.__dict__, "flags": [SYN, RST, ACK][seed % 3], "seq": seq}))
        elif kind < 0.75:
            opt = PALETTE[int(rng.integers(0, len(PALETTE)))]
            fl = SYN | [0, 0, 0, FIN, PSH, URG][int(rng.integers(0, 6))]
            s = syn(i, port, fl, opt, seq=seq, ack=ack, window=int(rng.integers(0, 1 << 16)),
                    pay_len=int(rng.integers(0, 3)))
            (created if cands[port] < space[port] else refused).append(s)
            cands[port] += 1
            segs.append(s)
        elif kind < 0.82 and refused:
            twin = refused[int(rng.integers(0, len(refused)))]
            segs.append(Seg(**{**twin.__dict__, "seq": seq}))
        else:
            fl = [RST, ACK, 0, SYN | ACK, RST | ACK, FIN, ACK | PSH][int(rng.integers(0, 7))]
            segs.append(syn(i, port, fl, seq=seq, ack=ack))
    return segs, space


def many_ports(seed: int, nports: int = 300, per_port: int = 4) -> tuple:
    """SYNs to nports listening ports spread over both digits, room for all but the last of each."""
    rng = np.random.default_rng(4300 + seed)
    ports = [int(p) for p in (np.arange(nports) * 211 + 7) % 65536]
    assert len(set(ports)) == nports and len({p >> 8 for p in ports}) > 200 and len({p & 0xFF for p in ports}) > 200
    pairs = [(p, r) for p in ports for r in range(per_port)]
    order = rng.permutation(len(pairs))
    segs = [syn(int(k), pairs[int(k)][0], options=PALETTE[int(k) % 4]) for k in order]
    return segs, {p: per_port - 1 for p in ports}


# ---------------------------------------------------------------- the de-duplication table

def slot(connid: tuple, bits: int) -> int:
    """sccsum_tcp_conns_slot, restated."""
    lip, fip, lp, fp = connid
    h = (lip * 0x9E3779B1) & M32
    h = ((h ^ fip) * 0x85EBCA6B) & M32
    h ^= (lp << 16) | fp
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h & ((1 << bits) - 1)


def table_bits(m_max: int) -> int:
    bits = 4
    while (1 << bits) < max(16, 2 * m_max):
        bits += 1
    return bits


def colliding(m_max: int = 64) -> tuple:
    """A bucket for a call with this m_max whose connids share home slots: ten
    at the table's last but one slot (the probe run wraps), six at slot 0
    (pushed along by the wrapped run), four at slot 1.  Some come with an
    ineligible segment first, those of port 82 (no room) twice, and the last
    segment repeats a created one: the stop.  Returns (segs, space)."""
    bits = table_bits(m_max)
    last = (1 << bits) - 1
    want = {last - 1: 10, 0: 6, 1: 4}
    found = {h: [] for h in want}
    k = 0
    while any(len(found[h]) < n for h, n in want.items()):
        s = syn(k, 80 + k % 3)
        h = slot(s.connid, bits)
        if h in want and len(found[h]) < want[h]:
            found[h].append(k)
        k += 1
    peers = [p for pair in zip(found[last - 1], found[0] + found[1]) for p in pair]
    segs = []
    for j, p in enumerate(peers):
        port = 80 + p % 3
        if j % 4 == 0:
            segs.append(syn(p, port, ACK))
        segs.append(syn(p, port, SYN))
        if port == 82:
            segs.append(syn(p, port, SYN, seq=77))
    first_made = next(p for p in peers if p % 3 == 0)
    segs.append(syn(first_made, 80, SYN, seq=78))
    assert len(segs) <= m_max
    return segs, {80: AMPLE, 81: 3, 82: 0}


# ---------------------------------------------------------------- the arrays tcp_rx leaves, wire frames

def l4_bytes(s: Seg) -> bytes:
    return tcp_traffic.segment(s.foreign_ip, s.local_ip, s.foreign_port, s.local_port, seq=s.seq, ack=s.ack, flags=s.flags,
                               window=s.window, payload=bytes((s.seq + j) & 0xFF for j in range(s.pay_len)),
                               options=s.options)


def frames(segs: list) -> list:
    """Wire frames (Ethernet) of the segments, in order."""
    return [tcp_traffic.frame(s.foreign_ip, s.local_ip, l4_bytes(s), ident=i) for i, s in enumerate(segs)]


def arrays(segs: list, lead: int = 3, trail: int = 2, seed: int = 0) -> dict:
    """The bucket as sccsum_tcp_rx leaves it: lead segments of bucket 0 in
    front, trail of bucket 2 behind, the frames in another order in the
    buffer (d_order leads to them) at every alignment."""
    rng = np.random.default_rng(4400 + seed)
    others = [Seg(HOST, 0x0B000000 + j, 443, 2000 + j, flags=ACK) for j in range(lead + trail)]
    grouped = others[:lead] + list(segs) + others[lead:]
    n, m = len(grouped), len(segs)
    ip = [tcp_traffic.frame(s.foreign_ip, s.local_ip, l4_bytes(s), ident=j)[14:] for j, s in enumerate(grouped)]
    place = rng.permutation(n)                      # grouped position p is batch frame place[p]
    length = np.zeros(n, dtype=np.uint32)
    for p in range(n):
        length[place[p]] = len(ip[p])
    gaps = (np.arange(n) % 5).astype(np.uint32)
    off = (np.cumsum(length + gaps, dtype=np.uint64) - length).astype(np.uint64)
    buf = np.zeros(int(off[-1] + length[-1]) if n else 0, dtype=np.uint8)
    seg = np.zeros(n, dtype=tm.SEG_DTYPE)
    for p, s in enumerate(grouped):
        o = int(off[place[p]])
        buf[o:o + len(ip[p])] = np.frombuffer(ip[p], np.uint8)
        H = 20 + len(s.options)
        seg[p] = (o + 20 + H, s.pay_len, s.seq, s.ack, p if p < lead else tm.NO_CONN, s.window, s.foreign_port,
                  s.local_port, s.flags, H)
    return dict(buf=buf, off=off, nbatch=n, n=n, m=m, first=np.array([0, lead, lead + m, n, n], dtype=np.uint32),
                order=place.astype(np.uint32), seg=seg, src=np.array([s.foreign_ip for s in grouped], dtype=np.uint32),
                local=np.array([s.local_ip for s in grouped], dtype=np.uint32), lead=lead)


def space_array(space: dict) -> np.ndarray:
    a = np.zeros(65536, dtype=np.uint32)
    for p, r in space.items():
        a[p] = r
    return a


# ---------------------------------------------------------------- large buckets, made as arrays

def scale_arrays(n_syn: int, n_other: int, seed: int = 0, ports=(80, 8080, 22, 443, 8443), lead: int = 2,
                 trail: int = 1) -> tuple:
    """n_syn SYNs of distinct peers with eight option bytes (an MSS, a window
    scale or both, in four arrangements) and n_other scattered segments that are
    no SYN, as the arrays sccsum_tcp_rx leaves; minimal 48-byte IP packets at
    every alignment, in another order in the buffer.  The second port has room
    for 1 % of its SYNs, the third for none.  Returns (arrays, space)."""
    rng = np.random.default_rng(4500 + seed)
    m = n_syn + n_other
    n = lead + m + trail
    other = np.zeros(n, dtype=bool)
    other[lead + rng.choice(m, n_other, replace=False)] = True
    other[:lead] = other[lead + m:] = True
    idx = np.arange(n, dtype=np.int64)
    port = np.array(ports, dtype=np.int64)[rng.integers(0, len(ports), n)]
    flags = np.where(other, np.array([RST, ACK, 0, SYN | ACK, RST | ACK, FIN, ACK | PSH])[rng.integers(0, 7, n)],
                     SYN | np.array([0, 0, 0, FIN, PSH, URG])[rng.integers(0, 6, n)])
    mss = rng.integers(0, 65536, n)
    mss[idx % 7 == 0] = np.array(MSS_VALUES)[rng.integers(0, 5, n)][idx % 7 == 0]
    shift = rng.integers(0, 17, n)
    hi, lo, one, zero = mss >> 8, mss & 0xFF, np.ones(n, np.int64), np.zeros(n, np.int64)
    layouts = [np.stack(x, axis=1) for x in (
        (2 * one, 4 * one, hi, lo, 3 * one, 3 * one, shift, one),        # MSS, window scale, NOP
        (3 * one, 3 * one, shift, one, 2 * one, 4 * one, hi, lo),        # window scale, NOP, MSS
        (one, one, one, one, one, 3 * one, 3 * one, shift),              # NOPs, window scale
        (2 * one, 4 * one, hi, lo, zero, 3 * one, 3 * one, shift))]      # MSS, EOL: the window scale is not seen
    pick = rng.integers(0, 4, n)
    opts = np.select([pick[:, None] == k for k in range(4)], layouts).astype(np.uint8)
    place = rng.permutation(n)
    off = np.zeros(n, dtype=np.uint64)
    off[place] = (place * 52 + place % 4).astype(np.uint64)
    off_p = off[place].astype(np.int64)                               # grouped position p lies at off_p[p]
    buf = np.zeros(n * 52 + 64, dtype=np.uint8)
    buf[off_p] = 0x45
    for k in range(4):
        buf[off_p + 16 + k] = (HOST >> (24 - 8 * k)) & 0xFF
    for k in range(8):
        buf[off_p + 40 + k] = opts[:, k]
    seg = np.zeros(n, dtype=tm.SEG_DTYPE)
    seg["pay_off"], seg["seq"], seg["ack"] = off_p + 48, rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n)
    seg["conn"], seg["window"] = tm.NO_CONN, rng.integers(0, 1 << 16, n)
    seg["sport"], seg["dport"], seg["flags"], seg["hdr_len"] = 1024 + idx % 50000, port, flags, 28
    src = (0x0B000000 + idx // 50000).astype(np.uint32)
    syns = {p: int(((port[lead:lead + m] == p) & ~other[lead:lead + m]).sum()) for p in ports}
    space = {p: AMPLE for p in ports}
    space[ports[1]], space[ports[2]] = syns[ports[1]] // 100, 0
    a = dict(buf=buf[:int(off.max()) + 48], off=off, nbatch=n, n=n, m=m,
             first=np.array([0, lead, lead + m, n, n], dtype=np.uint32), order=place.astype(np.uint32), seg=seg, src=src,
             lead=lead)
    return a, space


def segs_of(a: dict) -> list:
    """The bucket of an arrays dict as the model's segments."""
    lo, hi = int(a["first"][1]), int(a["first"][2])
    out = []
    for p in range(lo, hi):
        s = a["seg"][p]
        at = int(a["off"][int(a["order"][p])])
        end = int(s["pay_off"])
        out.append(Seg(int.from_bytes(a["buf"][at + 16:at + 20].tobytes(), "big"), int(a["src"][p]), int(s["dport"]),
                       int(s["sport"]), seq=int(s["seq"]), ack=int(s["ack"]), flags=int(s["flags"]), window=int(s["window"]),
                       options=a["buf"][end - (int(s["hdr_len"]) - 20):end].tobytes(), pay_len=int(s["pay_len"])))
    return out
