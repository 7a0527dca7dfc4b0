"""Seeded traffic for the TCP ACK fast path: connections with a retransmit
queue and the run of segments that reaches them, in the arrays sccsum_tcp_rx
leaves and sccsum_tcp_rx_acks takes, and what the call must write
(tests/tcp_ack_model.py).  Shared by tests/test_tcp_ack_host.py (the coverage)
and tests/test_gpu_tcp_ack.py."""
from __future__ import annotations

import copy

import numpy as np

import tcp_ack_model as am
from tcp_ack_model import ACK, FIN, M32, PSH, RST, SYN, URG, Seg, Tcb

TILE = 1024          # array_scan.h's tile of queue entries
BLOCK = 256          # tcp_ack.hip's block of records and of runs
NOW = 5_000_000_000  # the batch's clock_type::now(), ns

SEG_DTYPE = np.dtype([("pay_off", "<u8"), ("pay_len", "<u4"), ("seq", "<u4"), ("ack", "<u4"), ("conn", "<u4"),
                      ("window", "<u2"), ("sport", "<u2"), ("dport", "<u2"), ("flags", "u1"), ("hdr_len", "u1")])
ACK_DTYPE = np.dtype([("una", "<u4"), ("next", "<u4"), ("window", "<u4"), ("wl1", "<u4"), ("wl2", "<u4"),
                      ("cwnd", "<u4"), ("ssthresh", "<u4"), ("unsent_len", "<u4"), ("rcv_next", "<u4"), ("rto", "<u4"),
                      ("srtt", "<i8"), ("rttvar", "<i8"), ("mss", "<u2"), ("window_scale", "u1"), ("flags", "u1"),
                      ("reserved", "<u4")])
RUN_DTYPE = np.dtype([("taken", "<u4"), ("una", "<u4"), ("acked", "<u4"), ("popped", "<u4"), ("trim", "<u4"),
                      ("queue_freed", "<u4"), ("window", "<u4"), ("cwnd", "<u4"), ("srtt", "<i8"), ("rttvar", "<i8"),
                      ("rto", "<u4"), ("flags", "u1"), ("stop", "u1"), ("pad", "<u2"), ("reserved", "<u4", (2,))])

# how a run leaves the straight path; the first block at a run's head only
HEAD_KINDS = ("state", "dupacks3", "window_probe", "zwp_out", "snd_window_zero", "cwnd_zero", "cwnd_huge", "scale_15",
              "next_before_una", "queue_sum", "queue_zero_entry", "wl1_after", "wl2_after")
SEG_KINDS = ("gap", "fin", "syn", "rst", "urg", "no_ack", "text", "dup_ack", "old_ack", "beyond_next", "window_zero")
KINDS = HEAD_KINDS + SEG_KINDS


def stream(rng, count: int, kind: str = "none", at: int = 0, k: int = 0, entry_max: int = 3000) -> tuple:
    """(tcb, segs, opts): a connection whose run of `count` advancing pure ACKs
    leaves the straight path at segment `at` by `kind`.  opts: what the device
    is told against the tcb's own truth (eligible, lens)."""
    wrap = k % 7 == 3
    una = (M32 - int(rng.integers(0, 4000))) if wrap else int(rng.integers(1, 1 << 32))
    mss = int((536, 1460, 1460, 8960, 100)[k % 5])
    t = Tcb(una=una & M32, mss=mss, window_scale=int((0, 7, 2, 14)[k % 4]), rcv_next=int(rng.integers(0, 1 << 32)),
            state="CLOSE_WAIT" if k % 6 == 5 else "ESTABLISHED", unsent_len=0 if k % 5 == 4 else int(rng.integers(1, 1 << 20)),
            dupacks=int((0, 0, 1, 2)[k % 4]), first_rto_sample=k % 3 == 0, srtt=int(rng.integers(0, 300)),
            rttvar=int(rng.integers(0, 80)), rto=int(rng.integers(1000, 3000)))
    # slow start that crosses ssthresh, congestion avoidance with mss^2 / cwnd at 0, 1 and above, far slow start
    mode = k % 4
    if mode == 0:
        t.cwnd, t.ssthresh = 2 * mss, 2 * mss + int(rng.integers(1, 4 * mss))
    elif mode == 1:
        t.cwnd, t.ssthresh = mss * mss + int(rng.integers(1, 1000)), 2 * mss
    elif mode == 2:
        t.cwnd, t.ssthresh = max(mss * mss - int(rng.integers(0, 40)), 1), 2
    else:
        t.cwnd, t.ssthresh = 10 * mss, M32
    nent = max(1, int(rng.integers(1, 2 * count + 2)))
    lens = [1 if rng.integers(0, 6) == 0 else int(rng.integers(1, entry_max)) for _ in range(nent)]
    while sum(lens) < count:
        lens.append(count)
    t.queue(lens, tx=[NOW - int(rng.integers(-3, 400)) * 1_000_000 - int(rng.integers(0, 1_000_000)) for _ in lens],
            retransmitted={j for j in range(len(lens)) if rng.integers(0, 5) == 0})
    for e in t.data:
        e.data_len = min(e.len + int(rng.integers(0, 3)), 0xFFFF)
    total = sum(lens)
    t.window = max(total, 1) + int(rng.integers(0, 1000))
    t.wl1, t.wl2 = (t.rcv_next - int(rng.integers(0, 2))) & M32, t.una
    # ACK points: entry boundaries, one before and one after, and anywhere
    ends = np.cumsum(lens)
    pool = np.unique(np.clip(np.concatenate([ends, ends - 1, ends + 1, rng.integers(1, total + 1, size=count)]), 1, total))
    pts = np.sort(rng.choice(pool, size=count, replace=False)) if pool.size >= count else np.arange(1, count + 1)
    if k % 2 == 0:
        pts[-1] = total          # the queue emptied exactly
    pts = np.unique(pts)
    while pts.size < count:      # (the replacement collided)
        pts = np.unique(np.concatenate([pts, rng.integers(1, total + 1, size=count - pts.size)]))
    shift = t.window_scale
    segs = [Seg(seq=t.rcv_next, ack=(t.una + int(p)) & M32, window=int(rng.integers(1, 0x10000)),
                flags=ACK | (PSH if rng.integers(0, 4) == 0 else 0)) for p in pts]
    if k % 9 == 8:               # used at the window, and one below
        segs[-1].window = max(1, ((t.next - segs[-1].ack) & M32) >> shift) or 1
    opts = dict(eligible=None, lens=None)
    if kind == "none":
        return t, segs, opts
    s = segs[at]
    prev = segs[at - 1].ack if at else t.una
    if kind == "state":
        t.state = "FIN_WAIT_1"
    elif kind == "dupacks3":
        t.dupacks = 3
    elif kind == "window_probe":
        t.window_probe = True
    elif kind == "zwp_out":
        t.zero_window_probing_out = 1
    elif kind == "snd_window_zero":
        t.window = 0
    elif kind == "cwnd_zero":
        t.cwnd, opts["eligible"] = 0, True
    elif kind == "cwnd_huge":
        t.cwnd, opts["eligible"] = 1 << 31, True
    elif kind == "scale_15":
        t.window_scale, opts["eligible"] = 15, True
    elif kind == "next_before_una":
        t.next, opts["eligible"] = (t.una - 1) & M32, True
    elif kind == "queue_sum":
        opts["lens"] = [e.len for e in t.data]
        opts["lens"][-1] += 1
    elif kind == "queue_zero_entry":
        opts["lens"] = [e.len for e in t.data]
        if len(opts["lens"]) == 1:
            opts["lens"] = [opts["lens"][0], 0]
        else:
            opts["lens"][0] += opts["lens"][1]
            opts["lens"][1] = 0
    elif kind == "wl1_after":
        t.wl1 = (s.seq + 1) & M32
    elif kind == "wl2_after":
        t.wl1, t.wl2 = s.seq, (s.ack + 1) & M32
    elif kind == "gap":
        s.seq = (s.seq + 1 + int(rng.integers(0, 100))) & M32
    elif kind in ("fin", "syn", "rst", "urg"):
        s.flags |= dict(fin=FIN, syn=SYN, rst=RST, urg=URG)[kind]
    elif kind == "no_ack":
        s.flags &= ~ACK
    elif kind == "text":
        s.pay_len = int(rng.integers(1, 1460))
    elif kind == "dup_ack":
        s.ack = prev
    elif kind == "old_ack":
        s.ack = (prev - int(rng.integers(1, 50))) & M32
    elif kind == "beyond_next":
        s.ack = (t.next + 1 + int(rng.integers(0, 50))) & M32
    elif kind == "window_zero":
        s.window = 0
    return t, segs, opts


def mixed(seed: int, n: int, max_run: int = 16) -> list:
    """Cases that hold n segments in all: every kind at a head, and the
    per-segment ones mid-run and at the last segment too."""
    rng = np.random.default_rng(9100 + seed)
    out, left, k, used = [], n, 0, {}
    while left > 0:
        count = min(left, 1 if k % 11 == 10 else int(rng.integers(2, max_run + 1)))
        kind = KINDS[(k // 2) % len(KINDS)] if k % 2 else "none"
        used[kind] = used.get(kind, -1) + 1
        at = 0 if kind in HEAD_KINDS else (0, count // 2, count - 1)[used[kind] % 3]
        out.append(stream(rng, count, kind, at, k))
        left -= count
        k += 1
    return out


def by_lengths(seed: int, lengths, stops=None, entry_max: int = 3000) -> list:
    """Runs of the given lengths; stops[k] is None (straight to the end) or the
    segment at which run k leaves the path."""
    rng = np.random.default_rng(9200 + seed)
    out = []
    for k, count in enumerate(lengths):
        at = None if stops is None else stops[k]
        out.append(stream(rng, count, "none" if at is None else SEG_KINDS[k % len(SEG_KINDS)], at or 0, k, entry_max))
    return out


def arrays(cases: list, spare: int = 3, others: int = 5, seed: int = 0, now: int = NOW) -> dict:
    """The cases as sccsum_tcp_rx leaves them and as the host states its tcbs:
    run k is connection spare * k + 1 of nconns = spare * R + 2; `others`
    records of the other buckets follow bucket 0.  The connections without a
    run have queues too (never walked)."""
    rng = np.random.default_rng(9300 + seed)
    r = len(cases)
    nconns = spare * r + 2
    n0 = sum(len(segs) for _, segs, _ in cases)
    seg = np.zeros(n0 + others, dtype=SEG_DTYPE)
    ack = np.zeros(nconns, dtype=ACK_DTYPE)
    ack.view(np.uint8)[:] = 0xA7                              # connections without a run: never read
    run_conn = np.zeros(r, dtype=np.uint32)
    run_first = np.zeros(r + 1, dtype=np.uint32)
    q_first = np.zeros(nconns + 1, dtype=np.uint32)
    q_len, q_meta, q_tx = [], [], []
    by_conn = {spare * k + 1: case for k, case in enumerate(cases)}
    p = 0
    for c in range(nconns):
        q_first[c] = len(q_len)
        if c not in by_conn:
            for _ in range(int(rng.integers(0, 3))):
                q_len.append(int(rng.integers(0, 5000)))
                q_meta.append(int(rng.integers(0, 1 << 17)))
                q_tx.append(int(rng.integers(0, NOW)))
            continue
        t, segs, opts = by_conn[c]
        k = (c - 1) // spare
        run_conn[k], run_first[k] = c, p
        a = ack[c]
        for name in ("una", "next", "window", "wl1", "wl2", "cwnd", "ssthresh", "unsent_len", "rcv_next", "rto", "srtt",
                     "rttvar", "mss", "window_scale"):
            a[name] = getattr(t, name)
        a["flags"] = am.in_flags(t)
        if opts["eligible"] is not None:
            a["flags"] = (int(a["flags"]) & ~am.ELIGIBLE) | (am.ELIGIBLE if opts["eligible"] else 0)
        a["reserved"] = 0xDEADBEEF   # ignored
        lens = opts["lens"] if opts["lens"] is not None else [e.len for e in t.data]
        entries = list(t.data) + ([t.data[-1]] * (len(lens) - len(t.data)) if t.data else [])
        for length, e in zip(lens, entries):
            q_len.append(length)
            q_meta.append(e.data_len | (0x10000 if e.nr_transmits else 0))
            q_tx.append(e.tx_time)
        for s in segs:
            seg[p] = (0x1000 + 7 * p, s.pay_len, s.seq, s.ack, c, s.window, 80, 5000 + k % 100, s.flags, 20)
            p += 1
    q_first[nconns] = len(q_len)
    run_first[r] = n0
    seg[n0:]["conn"] = 0xFFFFFFFF
    seg[n0:]["flags"] = ACK
    first = np.array([0, n0, n0 + others // 2, n0 + others, n0 + others], dtype=np.uint32)
    return dict(seg=seg, ack=ack, run_conn=run_conn, run_first=run_first, first=first, n=n0 + others, n0=n0,
                nconns=nconns, rx_total=np.array([r, others - others // 2 if others else 0, 0, 0], dtype=np.uint64),
                q_first=q_first, q_len=np.array(q_len, dtype=np.uint32),
                q_meta=(np.array(q_meta, dtype=np.uint64) & M32).astype(np.uint32),
                q_tx=np.array(q_tx, dtype=np.int64), nq=len(q_len), now=now)


def record(rec: dict) -> tuple:
    return (rec["taken"], rec["una"], rec["acked"], rec["popped"], rec["trim"], rec["queue_freed"], rec["window"],
            rec["cwnd"], rec["srtt"], rec["rttvar"], rec["rto"], rec["flags"], rec["stop"], 0, (0, 0))


def expect(cases: list, now: int = NOW) -> dict:
    """What the call must write: the run records and d_total; `after`: every
    tcb behind its taken ACKs."""
    run = np.zeros(len(cases), dtype=RUN_DTYPE)
    after = []
    for j, (t, segs, opts) in enumerate(cases):
        rec, a = am.expect_run(copy.deepcopy(t), segs, now, opts["eligible"], opts["lens"])
        run[j] = record(rec)
        after.append(a)
    total = np.array([len(cases), int(run["taken"].sum()), int(run["popped"].sum()), int(run["acked"].sum())],
                     dtype=np.uint64)
    return dict(run=run, total=total, after=after)


def bulk(lengths, seed: int = 0, dup_every: int = 0) -> dict:
    """arrays()' dict for runs of the given lengths, built with numpy alone (no
    Tcb, for batches of a million ACKs): run r is connection r, every ACK
    advances, but in every dup_every-th run of three or more the second ACK is
    a duplicate.  Entries of 2..2000 bytes, run r has lengths[r] // 2 + 3."""
    rng = np.random.default_rng(9400 + seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    r = int(lengths.size)
    n0 = int(lengths.sum())
    run_first = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    nent = lengths // 2 + 3
    q_first = np.concatenate([[0], np.cumsum(nent)]).astype(np.uint32)
    nq = int(q_first[-1])
    q_len = rng.integers(2, 2001, size=nq).astype(np.uint32)
    q_len[rng.integers(0, nq, size=nq // 16)] = 1
    csum = np.concatenate([[0], np.cumsum(q_len.astype(np.int64))])
    flight = csum[q_first[1:].astype(np.int64)] - csum[q_first[:-1].astype(np.int64)]
    assert int(flight.max()) < 1 << 31 and np.all(flight >= lengths)
    ack = np.zeros(r, dtype=ACK_DTYPE)
    k = np.arange(r)
    ack["una"] = rng.integers(0, 1 << 32, size=r, dtype=np.uint64).astype(np.uint32)
    ack["una"][::7] = M32 - 100
    ack["next"] = (ack["una"].astype(np.int64) + flight) & M32
    ack["window"] = 65535
    ack["rcv_next"] = rng.integers(0, 1 << 32, size=r, dtype=np.uint64).astype(np.uint32)
    ack["wl1"], ack["wl2"] = ack["rcv_next"], ack["una"]
    mss = np.array([1460, 536, 8960], dtype=np.int64)[k % 3]
    ack["mss"] = mss
    ack["cwnd"] = np.where(k % 2, 2 * mss, mss * mss - 20)
    ack["ssthresh"] = np.where(k % 2, 2 * mss + 5000, 2)
    ack["unsent_len"] = np.where(k % 5 == 0, 0, 100000)
    ack["rto"], ack["srtt"], ack["rttvar"] = 1000, rng.integers(0, 300, size=r), rng.integers(0, 80, size=r)
    ack["window_scale"] = k % 15
    ack["flags"] = am.ELIGIBLE | np.where(k % 4 == 0, am.FIRST_SAMPLE, 0) | np.where(k % 6 == 5, am.CLOSE_WAIT, 0)
    # the ACK points of run r: ascending steps of 1 .. flight // length
    of_run = np.repeat(k, lengths)
    step = 1 + (rng.integers(0, 1 << 62, size=n0) % (flight // lengths)[of_run])
    at = np.cumsum(step)
    at -= np.repeat(at[run_first[:-1].astype(np.int64)] - step[run_first[:-1].astype(np.int64)], lengths)
    seg = np.zeros(n0, dtype=SEG_DTYPE)
    seg["conn"], seg["seq"], seg["hdr_len"] = of_run, ack["rcv_next"][of_run], 20
    seg["ack"] = (ack["una"].astype(np.int64)[of_run] + at) & M32
    seg["window"] = rng.integers(1, 0x10000, size=n0)
    seg["flags"] = ACK | np.where(np.arange(n0) % 5 == 0, PSH, 0)
    if dup_every:
        heads = run_first[:-1].astype(np.int64)[(k % dup_every == dup_every - 1) & (lengths >= 3)]
        seg["ack"][heads + 1] = seg["ack"][heads]
    return dict(seg=seg, ack=ack, run_conn=k.astype(np.uint32), run_first=run_first,
                first=np.array([0, n0, n0, n0, n0], dtype=np.uint32), n=n0, n0=n0, nconns=r,
                rx_total=np.array([r, 0, 0, 0], dtype=np.uint64), q_first=q_first, q_len=q_len,
                q_meta=(np.minimum(q_len, 0xFFFF) | np.where(rng.integers(0, 4, size=nq) == 0, 0x10000, 0)).astype(np.uint32),
                q_tx=(NOW - rng.integers(0, 400, size=nq) * 1_000_000 - rng.integers(0, 1_000_000, size=nq)).astype(np.int64),
                nq=nq, now=NOW)
