"""The rule of sccsum_tcp_rx_acks restated on the arrays themselves, for
batches too large for the per-segment model: every record's stop with numpy,
then one plain loop per run over its taken ACKs and popped entries.
tests/test_tcp_ack_host.py pins it to tests/tcp_ack_model.py byte for byte."""
from __future__ import annotations

import numpy as np

import tcp_ack_model as am
from tcp_ack_traffic import RUN_DTYPE

M32 = 0xFFFFFFFF


def _lt(a, b):
    return ((a - b) & M32) >= 0x80000000


def expect(a: dict) -> dict:
    """a: tcp_ack_traffic.arrays' dict.  Returns run [R] and total [4]."""
    n0, nconns, nq = int(a["first"][1]), int(a["nconns"]), int(a["nq"])
    seg, ack = a["seg"][:n0], a["ack"]
    r = int(a["rx_total"][0])
    g = np.concatenate([[0], np.cumsum(a["q_len"].astype(np.uint64))]).astype(np.uint64)
    z = np.concatenate([[0], np.cumsum(a["q_len"] == 0)])
    qa = np.minimum(a["q_first"][:-1].astype(np.int64), nq)
    qb = np.minimum(np.maximum(a["q_first"][1:].astype(np.int64), qa), nq)
    # the connection-level stops
    fl = ack["flags"].astype(np.int64)
    una, nxt = ack["una"].astype(np.int64), ack["next"].astype(np.int64)
    flight = (nxt - una) & M32
    inel = (((fl & am.ELIGIBLE) == 0) | (ack["window"] == 0) | (ack["cwnd"] == 0) | (ack["cwnd"] >= 1 << 31)
            | (ack["window_scale"] > 14) | (flight >= 0x80000000))
    bad_q = ((g[qb] - g[qa]) != flight.astype(np.uint64)) | (z[qb] != z[qa])
    cstop = np.where(inel, am.STOP_INELIGIBLE, np.where(bad_q, am.STOP_QUEUE, 0))
    # the per-record stops
    conn = seg["conn"].astype(np.int64)
    known = conn < nconns
    c = np.where(known, conn, 0)
    head = np.ones(n0, dtype=bool)
    head[1:] = conn[1:] != conn[:-1]
    s_ack, s_seq = seg["ack"].astype(np.int64), seg["seq"].astype(np.int64)
    prev = np.where(head, una[c], np.concatenate([[0], s_ack[:-1]]))
    window = (seg["window"].astype(np.int64) << ack["window_scale"][c].astype(np.int64)) & M32
    wl1, wl2 = ack["wl1"].astype(np.int64)[c], ack["wl2"].astype(np.int64)[c]
    stop = np.zeros(n0, dtype=np.int64)
    for cond, code in ((window == 0, am.STOP_WINDOW),
                       (head & ~(_lt(wl1, s_seq) | ((wl1 == s_seq) & ~_lt(s_ack, wl2))), am.STOP_WL),
                       (~(_lt(prev, s_ack) & ~_lt(nxt[c], s_ack)), am.STOP_ACK),
                       (seg["pay_len"] != 0, am.STOP_DATA),
                       ((seg["flags"] & 0x37) != 0x10, am.STOP_FLAGS),
                       (s_seq != ack["rcv_next"][c], am.STOP_SEQ),
                       (cstop[c] != 0, 0), (~known, am.STOP_INELIGIBLE)):
        stop = np.where(cond, code if code else cstop[c], stop)      # the last one written is the first in the table
    can_send = (ack["unsent_len"][c] > 0) & (((nxt[c] - s_ack) & M32) < window)
    off_of = ((s_ack - una[c]) & M32).tolist()
    stop_l, window_l, can_l = stop.tolist(), window.tolist(), can_send.tolist()
    g_l, meta, tx = g.tolist(), a["q_meta"].tolist(), a["q_tx"].tolist()
    now = int(a["now"])
    col = {name: ack[name].tolist() for name in ("una", "window", "cwnd", "rto", "srtt", "rttvar", "ssthresh", "mss", "flags")}
    run_conn, run_first, qa_l, qb_l = a["run_conn"].tolist(), a["run_first"].tolist(), qa.tolist(), qb.tolist()
    rows = []
    for j in range(r):
        k = run_conn[j]
        lo, hi = run_first[j], run_first[j + 1]
        if k >= nconns:
            rows.append((0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, am.STOP_INELIGIBLE, 0, (0, 0)))
            continue
        off = trim = freed = popped = taken = 0
        poll = False
        win, cwnd, rto, srtt, rttvar = col["window"][k], col["cwnd"][k], col["rto"][k], col["srtt"][k], col["rttvar"][k]
        ssthresh, mss = col["ssthresh"][k], col["mss"][k]
        first = bool(col["flags"][k] & am.FIRST_SAMPLE)
        e, e_end, base = qa_l[k], qb_l[k], g_l[qa_l[k]]
        code = am.STOP_END
        for i in range(lo, hi):
            if stop_l[i]:
                code = stop_l[i]
                break
            at = off_of[i]
            while e < e_end and g_l[e + 1] - base <= at:
                length = g_l[e + 1] - base - off
                off += length
                if not meta[e] & 0x10000:
                    sample = am.tdiv(now - tx[e], 1000000)
                    if first:
                        first, rttvar, srtt = False, am.tdiv(sample, 2), sample
                    else:
                        delta = abs(srtt - sample)
                        rttvar = am.tdiv(rttvar * 3, 4) + am.tdiv(delta, 4)
                        srtt = am.tdiv(srtt * 7, 8) + am.tdiv(sample, 8)
                    rto = min(max(srtt + max(1, 4 * rttvar), 1000), 60000)
                cwnd = (cwnd + (min(length, mss) if cwnd < ssthresh else max(1, ((mss * mss) & M32) // cwnd))) & M32
                freed += meta[e] & 0xFFFF
                trim = 0
                popped += 1
                e += 1
            if off < at:
                part = at - off
                trim += part
                off = at
                cwnd = (cwnd + (min(part, mss) if cwnd < ssthresh else max(1, ((mss * mss) & M32) // cwnd))) & M32
            win = window_l[i]
            poll |= can_l[i]
            taken += 1
        flags = am.FIRST_SAMPLE if first else 0
        if taken:
            flags |= am.ALL_ACKED if e == e_end else am.RTX_REARM
            if poll and not col["flags"][k] & am.CLOSE_WAIT:
                flags |= am.POLL
        rows.append((taken, (col["una"][k] + off) & M32, off, popped, trim, freed & M32, win, cwnd, srtt, rttvar, rto, flags,
                     code, 0, (0, 0)))
    run = np.array(rows, dtype=RUN_DTYPE) if rows else np.zeros(0, dtype=RUN_DTYPE)
    total = np.array([r, int(run["taken"].sum()), int(run["popped"].sum()), int(run["acked"].sum())], dtype=np.uint64)
    return dict(run=run, total=total)
