"""sccsum_tcp_rx_data's contract (include/sccsum.h, "TCP receive fast path")
restated over whole numpy arrays, for batches too large for the per-segment
model (tests/test_gpu_tcp_data_scale.py).  tests/test_tcp_data_fast.py pins it
to tests/tcp_data_model.py on the traffic of the GPU tests.

The delayed-ACK rule is the one piece of the model restated here in another
form: a segment's step is a table state -> (state, armed anew, ACK sent), and
the tables of a run are composed by a segmented doubling scan."""
from __future__ import annotations

import numpy as np

import tcp_data_traffic as tr

M32 = 0xFFFFFFFF
CLAMP = 1 << 30
BIG = np.iinfo(np.int64).max
# state = nr_full | armed << 1; an entry = the next state | 4 armed anew | 8 ACK sent (tcp.hh:1845-1872)
OVER = np.array([8, 8, 8, 8], dtype=np.uint8)        # seg_len > mss
FULL = np.array([7, 8, 3, 8], dtype=np.uint8)        # seg_len == mss
SHORT = np.array([6, 7, 2, 3], dtype=np.uint8)       # seg_len < mss
IDENT = np.array([0, 1, 2, 3], dtype=np.uint8)


def compose(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Tables [k, 4]: first a, then b."""
    eb = np.take_along_axis(b, (a & 3).astype(np.int64), axis=1)
    return (eb & 3) | ((a | eb) & 12)


def rx_data(seg: np.ndarray, first, run_conn, run_first, rcv: np.ndarray, max_bytes: int = M32, base: int = 0) -> dict:
    """The run records, the descriptors and d_total for tcp_rx's outputs as arrays."""
    n0, r = int(first[1]), int(run_conn.size)
    seg = seg[:n0]
    start = run_first[:r].astype(np.int64)
    end = run_first[1:r + 1].astype(np.int64)
    run_of = np.repeat(np.arange(r), end - start)
    st = rcv[run_conn.astype(np.int64)]
    length = seg["pay_len"].astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(length)])
    before = cs[:-1] - cs[start][run_of]                            # the run's bytes before the segment
    room0 = np.minimum(st["room"].astype(np.int64), CLAMP)
    cap = np.minimum(st["cap"].astype(np.int64), CLAMP)
    room = np.maximum(room0[run_of] - before, 0)
    head = np.arange(n0) == start[run_of]
    window = np.where(head, st["window"].astype(np.int64)[run_of], np.minimum(room, cap[run_of]))
    nxt = (st["next"].astype(np.int64)[run_of] + before) & M32
    fl = seg["flags"].astype(np.int64)
    stop = np.zeros(n0, dtype=np.int64)
    for code, cond in ((6, length == 0), (5, seg["ack"] != st["snd_una"][run_of]), (4, (fl & 0x37) != 0x10),
                       (3, seg["seq"].astype(np.int64) != nxt), (2, (length > 0) & (window == 0)),
                       (1, (st["flags"][run_of] & 1) == 0)):
        stop[cond] = code                                           # the last written is the first tested
    pos = np.where(stop != 0, np.arange(n0), BIG)
    fail = np.minimum.reduceat(pos, start) if r else np.zeros(0, dtype=np.int64)
    fail = np.where(end > start, fail, BIG)                         # (no run is empty; reduceat would lie)
    taken = np.minimum(fail, end) - start
    why = np.where(fail < end, stop[np.minimum(fail, max(n0 - 1, 0))] if n0 else 0, 0)
    nbytes = cs[start + taken] - cs[start]
    # the composed tables, inclusive, by doubling inside the runs
    seg_len, mss = length & 0xFFFF, st["mss"].astype(np.int64)[run_of]
    tab = np.where((seg_len > mss)[:, None], OVER, np.where((seg_len == mss)[:, None], FULL, SHORT)).astype(np.uint8)
    idx, d = np.arange(n0), 1
    while n0 and d < int((end - start).max()):
        ok = idx - d >= start[run_of]
        tab[ok] = compose(tab[idx[ok] - d], tab[ok])
        d *= 2
    s0 = ((st["flags"] >> 1) & 3).astype(np.int64)                  # NR_FULL 2, ACK_ARMED 4 -> nr | armed << 1
    last = np.maximum(start + taken - 1, 0)
    entry = np.where(taken > 0, tab[last, s0] if n0 else 0, s0).astype(np.int64)
    flags = ((entry & 3) << 1) | ((entry & 12) << 1)
    # the capacity: a prefix of the runs
    ends = np.cumsum(nbytes)
    over = np.flatnonzero(ends > max_bytes)
    cut = int(over[0]) if over.size else r
    kept = np.arange(r) < cut
    run = np.zeros(r, dtype=tr.RUN_DTYPE)
    room_after = np.maximum(room0 - nbytes, 0)
    run["taken"] = np.where(kept, taken, 0)
    run["bytes"] = np.where(kept, nbytes, 0)
    run["next"] = np.where(kept, (st["next"].astype(np.int64) + nbytes) & M32, st["next"])
    run["window"] = np.where(kept & (taken > 0), np.minimum(room_after, cap), st["window"])
    run["room"] = np.where(kept, room_after, room0)
    run["flags"] = np.where(kept, flags, (s0 << 1))
    run["stop"] = np.where(kept, why, 7)
    run["desc_first"] = np.cumsum(run["taken"]) - run["taken"]
    run["dst_off"] = np.cumsum(run["bytes"].astype(np.int64)) - run["bytes"]
    emit = (np.arange(n0) < (start + taken)[run_of]) & kept[run_of] if n0 else np.zeros(0, dtype=bool)
    desc = np.zeros(int(emit.sum()), dtype=tr.DESC_DTYPE)
    desc["src"] = seg["pay_off"][emit] + np.uint64(base)
    desc["len"] = seg["pay_len"][emit]
    desc["dst_off"] = np.cumsum(length[emit]) - length[emit]
    total = np.array([desc.size, int(run["bytes"].astype(np.int64).sum()), int(nbytes.sum()), 0], dtype=np.uint64)
    return dict(run=run, desc=desc, total=total)
