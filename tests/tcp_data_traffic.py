"""Seeded input for sccsum_tcp_rx_data: runs written as sccsum_tcp_seg records
directly (the call reads nothing else), laid out as sccsum_tcp_rx leaves
them, and what tests/tcp_data_model.py makes of them.

A case is (Tcb, [segment dicts]): one connection's state before the batch and
its run in arrival order.  stream() makes an in-order run and splices one
departure from the straight path in at a chosen segment; the kinds are KINDS."""
from __future__ import annotations

import copy

import numpy as np

import tcp_data_model as dm
from tcp_data_model import ACK, FIN, PSH, RST, SYN, URG, M32, Tcb

SEG_DTYPE = np.dtype([("pay_off", "<u8"), ("pay_len", "<u4"), ("seq", "<u4"), ("ack", "<u4"), ("conn", "<u4"),
                      ("window", "<u2"), ("sport", "<u2"), ("dport", "<u2"), ("flags", "u1"), ("hdr_len", "u1")])
RCV_DTYPE = np.dtype([("next", "<u4"), ("window", "<u4"), ("room", "<u4"), ("cap", "<u4"), ("snd_una", "<u4"),
                      ("mss", "<u2"), ("flags", "u1"), ("pad", "u1"), ("reserved", "<u4", (2,))])
RUN_DTYPE = np.dtype([("taken", "<u4"), ("bytes", "<u4"), ("next", "<u4"), ("window", "<u4"), ("room", "<u4"),
                      ("desc_first", "<u4"), ("dst_off", "<u4"), ("flags", "u1"), ("stop", "u1"), ("pad", "<u2")])
DESC_DTYPE = np.dtype([("src", "<u8"), ("dst_off", "<u4"), ("len", "<u4")])
TILE = 1024

# a departure spliced into the stream at segment `at` (none: the run stays straight)
SEGMENT_KINDS = ("none", "reorder", "dup", "gap", "overlap", "pure_ack", "ack_advances", "ack_beyond", "ack_old",
                 "fin", "syn", "rst", "urg", "no_ack", "room", "room_minus", "room_plus")
# what the connection brings along
CONN_KINDS = ("window0", "not_established", "ooo_pending", "snd_window0", "una_past_next", "cap_small")
KINDS = SEGMENT_KINDS + CONN_KINDS
STATES = ((0, False), (1, False), (0, True), (1, True))


def _len(rng, mss: int) -> int:
    k = int(rng.integers(0, 10))
    return (mss - 1, mss, mss + 1, 1, 65515, mss, mss, mss - 1)[k] if k < 8 else int(rng.integers(1, 2 * mss))


def stream(rng, count: int, kind: str = "none", at: int = 0, state: int = 0, wrap: bool = False,
           lens=None) -> tuple:
    """(Tcb, segs): `count` segments; without a departure all of them are taken."""
    mss = (1460, 536, 8960)[int(rng.integers(0, 3))]
    nr, armed = STATES[state % 4]
    una = int(rng.integers(0, 1 << 32))
    t = Tcb(rcv_next=(M32 - 3000) if wrap else int(rng.integers(0, 1 << 32)), mss=mss, snd_unacknowledged=una,
            snd_next=(una + 5000) & M32, nr_full_seg_received=nr, armed=armed, window_scale=7,
            max_receive_buf_size=1 << 30)
    t.rcv_window = t.modified_window()
    lens = [_len(rng, mss) for _ in range(count)] if lens is None else list(lens)
    at = min(at, count - 1)
    if kind == "window0":
        t.rcv_window = 0                       # as it stands: the buffer has room again, the window not yet
    elif kind == "not_established":
        t.established = False
    elif kind == "ooo_pending":
        t.out_of_order_empty = False
    elif kind == "snd_window0":
        t.snd_window = 0
    elif kind == "una_past_next":
        t.snd_next = (una - 1) & M32
    elif kind == "cap_small":
        t.window_scale = 0                     # cap = 29 200 < room
        t.max_receive_buf_size = 29200 * 4
        t.rcv_window = t.modified_window()
    elif kind in ("room", "room_minus", "room_plus"):
        # the buffer is exhausted by the segments before `at`: S = room, room - 1 (one more fits), room + 1
        at = max(at, 1)                        # == count in a run of one segment: all of it fits
        s = sum(lens[:at])
        if kind == "room_plus":
            s -= 1
        t.max_receive_buf_size = t.data_size + s + (1 if kind == "room_minus" else 0)
        t.rcv_window = max(t.modified_window(), 1)
    segs, seq = [], t.rcv_next
    for k in range(count):
        fl = ACK | (PSH if rng.random() < 0.3 else 0) | (0x40 if rng.random() < 0.1 else 0) | \
            (0x80 if rng.random() < 0.1 else 0)
        segs.append(dict(pay_off=0, pay_len=lens[k], seq=seq, ack=una, flags=fl, window=int(rng.integers(1, 65536)),
                         sport=4000, dport=80, hdr_len=20))
        seq = (seq + lens[k]) & M32
    s = segs[min(at, count - 1)]
    if kind == "reorder" and at + 1 < count:
        segs[at], segs[at + 1] = segs[at + 1], segs[at]
    elif kind == "reorder" or kind == "gap":
        s["seq"] = (s["seq"] + 1 + int(rng.integers(0, 3000))) & M32
    elif kind == "dup":
        s["seq"] = (s["seq"] - s["pay_len"]) & M32           # the bytes before RCV.NXT once more
    elif kind == "overlap":
        s["seq"] = (s["seq"] - 1 - int(rng.integers(0, max(s["pay_len"] - 1, 1)))) & M32
    elif kind == "pure_ack":
        for later in segs[at + 1:]:
            later["seq"] = (later["seq"] - s["pay_len"]) & M32
        s["pay_len"] = 0
    elif kind == "ack_advances":
        s["ack"] = (una + 1 + int(rng.integers(0, 5000))) & M32
    elif kind == "ack_beyond":
        s["ack"] = (una + 5001 + int(rng.integers(0, 1000))) & M32
    elif kind == "ack_old":
        s["ack"] = (una - 1 - int(rng.integers(0, 1000))) & M32
    elif kind in ("fin", "syn", "rst", "urg"):
        s["flags"] |= dict(fin=FIN, syn=SYN, rst=RST, urg=URG)[kind]
    elif kind == "no_ack":
        s["flags"] &= ~ACK
    return t, segs


def mixed(seed: int, n: int, max_run: int = 40) -> list:
    """Cases that hold n segments in all: every kind at a head, mid-run and at
    the last segment, all four delayed-ACK states, sequence numbers crossing 2^32."""
    rng = np.random.default_rng(7100 + seed)
    out, left, k, used = [], n, 0, {}
    while left > 0:
        count = min(left, 1 if k % 11 == 10 else int(rng.integers(2, max_run + 1)))
        kind = KINDS[k % len(KINDS)] if k % 3 else "none"
        used[kind] = used.get(kind, -1) + 1                 # a kind's first run leaves at the head, its next mid-run, ...
        at = (0, count // 2, count - 1)[used[kind] % 3]
        out.append(stream(rng, count, kind, at, state=k, wrap=k % 7 == 3))
        left -= count
        k += 1
    return out


def by_lengths(seed: int, lengths, stops=None) -> list:
    """Runs of the given lengths; stops[k] is None (straight to the end) or
    the segment at which run k leaves the path."""
    rng = np.random.default_rng(7200 + seed)
    out = []
    for k, count in enumerate(lengths):
        at = None if stops is None else stops[k]
        kinds = ("gap", "fin", "ack_advances", "pure_ack", "dup")
        out.append(stream(rng, count, "none" if at is None else kinds[k % len(kinds)], at or 0, state=k))
    return out


def arrays(cases: list, spare: int = 3, others: int = 5, base_off: int = 0) -> dict:
    """The cases as sccsum_tcp_rx leaves them: run k is connection spare * k + 1
    of nconns = spare * R + 2; `others` records of the other buckets follow
    bucket 0.  pay_off counts up with gaps."""
    r = len(cases)
    nconns = spare * r + 2
    n0 = sum(len(segs) for _, segs in cases)
    seg = np.zeros(n0 + others, dtype=SEG_DTYPE)
    rcv = np.zeros(nconns, dtype=RCV_DTYPE)
    rcv.view(np.uint8)[:] = 0xA7                              # connections without a run: never read
    run_conn = np.zeros(r, dtype=np.uint32)
    run_first = np.zeros(r + 1, dtype=np.uint32)
    p, off = 0, base_off
    for k, (t, segs) in enumerate(cases):
        c = spare * k + 1
        run_conn[k], run_first[k] = c, p
        rec = t.rcv_record()
        for name, v in rec.items():
            rcv[c][name] = v
        rcv[c]["pad"], rcv[c]["reserved"] = 0x5A, 0xDEADBEEF   # ignored
        for s in segs:
            s["pay_off"] = off
            off += s["pay_len"] + (p % 5)
            for name in ("pay_off", "pay_len", "seq", "ack", "window", "sport", "dport", "flags", "hdr_len"):
                seg[p][name] = s[name]
            seg[p]["conn"] = c
            p += 1
    run_first[r] = n0
    seg[n0:]["conn"] = 0xFFFFFFFF
    seg[n0:]["pay_len"] = 99
    first = np.array([0, n0, n0 + others // 2, n0 + others, n0 + others], dtype=np.uint32)
    return dict(seg=seg, rcv=rcv, run_conn=run_conn, run_first=run_first, first=first, n=n0 + others, n0=n0,
                nconns=nconns, rx_total=np.array([r, others - others // 2 if others else 0, 0, 0], dtype=np.uint64))


def walk_all(cases: list) -> tuple:
    """(results, initial): every case walked by the model from a copy of its
    tcb, and the empty walk of the same tcb (the state as given)."""
    results = [dm.walk(copy.deepcopy(t), segs) for t, segs in cases]
    initial = [dm.walk(copy.deepcopy(t), []) for t, _ in cases]
    return results, initial


def expect(cases: list, max_bytes: int = M32, base: int = 0) -> dict:
    """What the call must write: the run records, the descriptors, d_total."""
    results, initial = walk_all(cases)
    results, totals = dm.capacity(results, initial, max_bytes)
    run = np.zeros(len(cases), dtype=RUN_DTYPE)
    desc = np.zeros(totals[0], dtype=DESC_DTYPE)
    k = 0
    for j, (r, r0) in enumerate(zip(results, initial)):
        # the flags of a run that took nothing are the connection's own
        fl = r.flags if r.taken or r.stop != dm.STOP_CAPACITY else r0.flags
        run[j] = (r.taken, r.bytes, r.next, r.window, min(r.room, 1 << 30), r.desc_first, r.dst_off, fl, r.stop, 0)
        at = r.dst_off
        for off, length in r.data:
            desc[k] = (base + off, at, length)
            at += length
            k += 1
    return dict(run=run, desc=desc, total=np.array(list(totals) + [0], dtype=np.uint64), results=results)
