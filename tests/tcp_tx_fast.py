"""sccsum_tcp_tx_data's contract (include/sccsum.h, "TCP transmit fast path")
over numpy arrays: the closed form of tests/tcp_tx_model.py for a whole batch,
with the capacity prefix, the packed layout and the descriptors.  It is written
from the contract, not from the kernels: the pieces come from two searches of a
segment's first and last byte in the starts of the buffers that hold bytes.
tests/test_tcp_tx_fast.py pins it to the per-segment model."""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
ELIGIBLE, RTX_ARMED, RTX_ARM = 0x01, 0x02, 0x04
STOP_END, STOP_INELIGIBLE, STOP_WINDOW, STOP_CAPACITY, STOP_QUEUE = 0, 1, 2, 7, 8
NEED_CLAMP = 1 << 43

SND_DTYPE = np.dtype([("dst", "<u4"), ("next", "<u4"), ("una", "<u4"), ("window", "<u4"), ("cwnd", "<u4"),
                      ("rcv_next", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("mss", "<u2"), ("wnd", "<u2"),
                      ("flags", "u1"), ("pad", "u1", (3,)), ("reserved", "<u4", (3,))])
RUN_DTYPE = np.dtype([("segs", "<u4"), ("bytes", "<u4"), ("seg_first", "<u4"), ("next", "<u4"), ("flags", "u1"),
                      ("stop", "u1"), ("pad", "<u2"), ("reserved", "<u4", (3,))])
OUT_DTYPE = np.dtype([("dst", "<u4"), ("seq", "<u4"), ("ack", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
                      ("window", "<u2"), ("flags", "u1"), ("hdr_len", "u1"), ("mss", "<u4")])


def seg_len(mtu: int, tso: bool, max_packet_len: int, mss):
    if tso:
        return np.full(np.shape(mss), max_packet_len - 40, dtype=np.int64)
    return np.minimum((mtu - 40) & 0xFFFF, np.asarray(mss, dtype=np.int64))


def connections(snd: np.ndarray, buf_len: np.ndarray, buf_first: np.ndarray, mtu: int, headroom: int, tso: bool = False,
                max_packet_len: int = 65535) -> dict:
    """Per connection, without the caps: segs, bytes, P, stop, flags, the layout bytes."""
    g = np.concatenate([[0], np.cumsum(buf_len.astype(np.uint64), dtype=np.uint64)]).astype(np.int64)
    first = buf_first.astype(np.int64)
    base, u = g[first[:-1]], g[first[1:]] - g[first[:-1]]
    nxt, una, window = (snd[k].astype(np.int64) for k in ("next", "una", "window"))
    eligible = (snd["flags"] & ELIGIBLE) != 0
    taken = eligible & (u <= M32)
    used = (nxt - una) & M32
    can = np.where((window == 0) | (used > window), 0, np.minimum(window - used, u))
    p = np.minimum(snd["cwnd"].astype(np.int64), seg_len(mtu, tso, max_packet_len, snd["mss"]))
    sent = np.where(taken & (p > 0), can, 0)
    segs = np.where(taken, np.where(sent > 0, -(-sent // np.maximum(p, 1)), 1), 0)
    stop = np.where(~eligible, STOP_INELIGIBLE, np.where(~taken, STOP_QUEUE, np.where(sent == u, STOP_END, STOP_WINDOW)))
    arm = np.where((sent > 0) & ((snd["flags"] & RTX_ARMED) == 0), RTX_ARM, 0)
    return dict(g=g, base=base, u=u, p=p, sent=sent, segs=segs, stop=stop, arm=arm,
                need=np.minimum(sent + headroom * segs, NEED_CLAMP))


def expect(snd: np.ndarray, buf_len: np.ndarray, buf_first: np.ndarray, mtu: int, headroom: int, tso: bool = False,
           max_packet_len: int = 65535, max_segs: int = 0x7FFFFFFF, max_bytes: int = M32) -> dict:
    """Everything the call writes: run, off, len, out, seg_first, the
    descriptors as (buffer, inner offset, dst_off, len), total."""
    c = connections(snd, buf_len, buf_first, mtu, headroom, tso, max_packet_len)
    nconn = snd.size
    segs, need = c["segs"].copy(), c["need"].copy()
    fits = (np.cumsum(segs) <= max_segs) & (np.cumsum(need) <= max_bytes)
    prefix = int(np.argmin(fits)) if not fits.all() else nconn
    needed = int(need.sum())
    segs[prefix:] = 0
    need[prefix:] = 0
    sent = np.where(np.arange(nconn) < prefix, c["sent"], 0)
    seg_first = np.concatenate([[0], np.cumsum(segs)])
    lay_first = np.concatenate([[0], np.cumsum(need)])
    run = np.zeros(nconn, dtype=RUN_DTYPE)
    run["segs"], run["bytes"], run["seg_first"] = segs, sent, seg_first[:-1]
    run["next"] = (snd["next"].astype(np.int64) + sent) & M32
    run["flags"] = np.where(np.arange(nconn) < prefix, c["arm"], 0)
    run["stop"] = np.where(np.arange(nconn) < prefix, c["stop"], STOP_CAPACITY)

    nseg = int(seg_first[-1])
    conn = np.repeat(np.arange(nconn), segs)
    k = np.arange(nseg) - seg_first[conn]
    p = c["p"][conn]
    start = k * p
    length = np.where(sent[conn] > 0, np.minimum(p, sent[conn] - start), 0)
    off = lay_first[conn] + k * (p + headroom) + headroom
    out = np.zeros(nseg, dtype=OUT_DTYPE)
    s = snd[conn]
    out["dst"], out["ack"], out["sport"], out["dport"], out["window"], out["mss"] = (
        s["dst"], s["rcv_next"], s["sport"], s["dport"], s["wnd"], s["mss"])
    out["seq"] = (s["next"].astype(np.int64) + start) & M32
    out["flags"], out["hdr_len"] = 0x10, 20

    # the pieces: the buffers that hold bytes, by their first byte in the concatenation of all queues
    holds = np.flatnonzero(buf_len != 0)
    lo_of, hi_of = c["g"][holds], c["g"][holds + 1]
    lo = c["base"][conn] + start
    hi = lo + length
    with_bytes = length > 0
    ja = np.searchsorted(lo_of, lo, side="right") - 1
    jb = np.searchsorted(lo_of, np.maximum(hi, 1) - 1, side="right") - 1
    count = np.where(with_bytes, jb - ja + 1, 0)
    desc_first = np.concatenate([[0], np.cumsum(count)])
    seg_of = np.repeat(np.arange(nseg), count)
    j = ja[seg_of] + np.arange(int(desc_first[-1])) - desc_first[seg_of]
    a = np.maximum(lo_of[j], lo[seg_of]) if j.size else np.zeros(0, np.int64)
    b = np.minimum(hi_of[j], hi[seg_of]) if j.size else np.zeros(0, np.int64)
    return dict(run=run, off=off.astype(np.uint64), len=length.astype(np.uint32), out=out, conn=conn,
                seg_first=desc_first.astype(np.uint32), desc_buf=holds[j] if j.size else np.zeros(0, np.int64),
                desc_inner=a - lo_of[j] if j.size else a, desc_dst=(off[seg_of] + a - lo[seg_of]).astype(np.uint32),
                desc_len=(b - a).astype(np.uint32),
                total=np.array([nseg, int(lay_first[-1]), int(desc_first[-1]), needed], dtype=np.uint64))
