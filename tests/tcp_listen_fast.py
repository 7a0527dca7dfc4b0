"""The rule of sccsum_tcp_listen restated on the arrays themselves (numpy), for
buckets too large for the per-segment model: candidates by a stable sort of
the connids, ranks by a stable sort of the ports, MD5 over whole arrays, the
option parse as one masked step per loop turn.  tests/test_tcp_listen_host.py
pins it to tests/tcp_listen_model.py byte for byte on the small cases."""
from __future__ import annotations

import numpy as np

import tcp_listen_model as lm

M32 = 0xFFFFFFFF
SYN, RST, ACK = lm.SYN, lm.RST, lm.ACK

_S = [7, 12, 17, 22] * 4 + [5, 9, 14, 20] * 4 + [4, 11, 16, 23] * 4 + [6, 10, 15, 21] * 4
_K = [int(abs(np.sin(i + 1)) * 2 ** 32) & M32 for i in range(64)]


def _md5_block(h, w):
    """One MD5 block (RFC 1321) over arrays: h four uint64 arrays holding 32-bit values, w sixteen."""
    a, b, c, d = h
    for r in range(64):
        if r < 16:
            f, g = (b & c) | (~b & M32 & d), r
        elif r < 32:
            f, g = (d & b) | (~d & M32 & c), (5 * r + 1) % 16
        elif r < 48:
            f, g = b ^ c ^ d, (3 * r + 5) % 16
        else:
            f, g = c ^ (b | (~d & M32)), (7 * r) % 16
        t = (a + f + _K[r] + w[g]) & M32
        a, d, c = d, c, b
        b = (b + (((t << _S[r]) | (t >> (32 - _S[r]))) & M32)) & M32
    return [(x + y) & M32 for x, y in zip(h, (a, b, c, d))]


def isn(local, foreign, lport, fport, key: bytes, isn_m: int) -> np.ndarray:
    """get_isn for arrays of connids."""
    kw = [int(x) for x in np.frombuffer(key, dtype="<u4")]
    n = local.shape[0]
    const = lambda v: np.full(n, v, dtype=np.uint64)   # noqa: E731
    h = [const(0x67452301), const(0xEFCDAB89), const(0x98BADCFE), const(0x10325476)]
    ports = ((lport.astype(np.uint64) << np.uint64(16)) + fport.astype(np.uint64)) & np.uint64(M32)
    w = [local.astype(np.uint64), foreign.astype(np.uint64), ports] + [const(v) for v in kw[:13]]
    h = _md5_block(h, w)
    w = [const(v) for v in kw[13:]] + [const(0x80)] + [const(0)] * 10 + [const(76 * 8), const(0)]
    h = _md5_block(h, w)
    return ((h[0] + np.uint64(isn_m)) & np.uint64(M32)).astype(np.uint32)


def parse(buf: np.ndarray, start: np.ndarray, length: np.ndarray) -> tuple:
    """tcp_option::parse with the interface's two deviations, for arrays of
    option ranges buf[start .. start + length): (mss, shift, flags)."""
    n = start.shape[0]
    beg = np.zeros(n, dtype=np.int64)
    end = length.astype(np.int64)
    live = beg < end
    mss = np.full(n, 536, dtype=np.int64)
    shift = np.zeros(n, dtype=np.int64)
    flags = np.zeros(n, dtype=np.int64)
    base = start.astype(np.int64)
    pad = np.concatenate([buf, np.zeros(8, dtype=np.uint8)]).astype(np.int64)

    def at(k):
        return pad[np.where(live, base + np.minimum(k, end), 0)]

    while live.any():
        kind = at(beg)
        plain = (kind == 0) | (kind == 1)
        live &= plain | (beg + 1 < end)                # the length byte is not there
        size = np.where(plain, 0, at(beg + 1))
        live &= plain | (beg + size <= end)
        live &= kind != 0
        is_mss, is_ws, is_sack, is_nop = live & (kind == 2), live & (kind == 3), live & (kind == 4), live & (kind == 1)
        other = live & ~(is_mss | is_ws | is_sack | is_nop)
        cut = (is_mss & (beg + 3 >= end)) | (is_ws & (beg + 2 >= end)) | (other & (size == 0))
        live &= ~cut
        is_mss, is_ws, is_sack, is_nop, other = (x & live for x in (is_mss, is_ws, is_sack, is_nop, other))
        mss = np.where(is_mss, (at(beg + 2) << 8) | at(beg + 3), mss)
        shift = np.where(is_ws, at(beg + 2), shift)
        flags |= np.where(is_mss, lm.F_MSS, 0) | np.where(is_ws, lm.F_WSCALE, 0) | np.where(is_sack, lm.F_SACK, 0)
        beg = beg + np.where(is_mss, 4, 0) + np.where(is_ws, 3, 0) + np.where(is_sack, 2, 0) + np.where(is_nop, 1, 0) \
            + np.where(other, size, 0)
        live &= beg < end
    return mss, shift, flags


def _fold(s):
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    return (s & 0xFFFF) + (s >> 16)


def _be32(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.int64)
    return np.stack([(v >> 24) & 0xFF, (v >> 16) & 0xFF, (v >> 8) & 0xFF, v & 0xFF], axis=1).astype(np.uint8)


def resets(local, foreign, lport, fport, seq, ack, flags, offload: bool) -> np.ndarray:
    """respond_with_reset for arrays (none of them has RST set): uint8 [k, 20]."""
    seq_out = np.where(flags & ACK, ack, 0)
    syn_on = (flags & SYN) != 0
    ack_out = np.where(syn_on, (seq + 1) & M32, 0)
    w3 = (5 << 12) | lm.RST | np.where(syn_on, ACK, 0)
    pseudo = _fold((local >> 16) + (local & 0xFFFF) + (foreign >> 16) + (foreign & 0xFFFF) + 6 + 20)
    body = lport + fport + (seq_out >> 16) + (seq_out & 0xFFFF) + (ack_out >> 16) + (ack_out & 0xFFFF) + w3
    field = pseudo if offload else (~_fold(pseudo + body)) & 0xFFFF
    ports = (lport << 16) | fport
    tail = (field << 16)
    return np.concatenate([_be32(ports), _be32(seq_out), _be32(ack_out), _be32(w3 << 16), _be32(tail)], axis=1)


def expect(a: dict, space: np.ndarray, key: bytes, isn_m: int, mtu: int, offload: bool = False) -> dict:
    """a: tcp_listen_traffic.arrays' dict; space: uint32 [65536].  Every array of tcp_listen_model.expect."""
    lo, hi = int(a["first"][1]), int(a["first"][2])
    m = hi - lo
    seg, buf = a["seg"][lo:hi], a["buf"]
    frame = a["order"][lo:hi].astype(np.int64)
    at = a["off"][frame].astype(np.int64) + 16
    local = np.zeros(m, dtype=np.int64)
    for k in range(4):
        local = (local << 8) | buf[at + k].astype(np.int64)
    foreign = a["src"][lo:hi].astype(np.int64)
    lport, fport = seg["dport"].astype(np.int64), seg["sport"].astype(np.int64)
    flags = seg["flags"].astype(np.int64)
    idx = np.arange(m, dtype=np.int64)
    space = np.asarray(space).astype(np.int64)

    # a connid's candidate: its first eligible segment
    elig = (flags & (SYN | RST | ACK)) == SYN
    ids = np.stack([local, foreign, (lport << 16) | fport], axis=1)
    _, inv = np.unique(ids, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.full(int(inv.max()) + 1 if m else 0, m, dtype=np.int64)
    np.minimum.at(first, inv[elig], idx[elig])
    cand = elig & (first[inv] == idx)
    # rank: the earlier candidates on the same port
    ci = idx[cand]
    by_port = ci[np.argsort(lport[ci], kind="stable")]
    sp = lport[by_port]
    head = np.concatenate([[True], sp[1:] != sp[:-1]]) if sp.size else np.zeros(0, dtype=bool)
    start = np.maximum.accumulate(np.where(head, np.arange(sp.size), 0)) if sp.size else np.zeros(0, dtype=np.int64)
    rank = np.arange(sp.size) - start
    made = np.zeros(m, dtype=bool)
    made[by_port] = rank < space[sp]
    # a port is full behind its space-th candidate
    full_pos = np.full(65536, m, dtype=np.int64)
    last = rank == space[sp] - 1
    full_pos[sp[last]] = by_port[last]
    full = (space[lport] == 0) | (idx > full_pos[lport])
    # the stop
    c = first[inv] if m else np.zeros(0, dtype=np.int64)
    stops = (c < idx) & made[np.minimum(c, max(m - 1, 0))]
    taken = int(idx[stops].min()) if stops.any() else m

    rst_on, ack_on, syn_on = (flags & RST) != 0, (flags & ACK) != 0, (flags & SYN) != 0
    cls = np.where(full, np.where(rst_on, lm.DROP, lm.RESET),
                   np.where(rst_on, lm.DROP, np.where(ack_on, lm.RESET, np.where(syn_on, lm.NEW, lm.DROP))))
    cls = np.where(idx >= taken, lm.LATER, cls).astype(np.uint8)

    new_i = idx[cls == lm.NEW]
    k = new_i.size
    s = seg[new_i]
    hdr_in = s["hdr_len"].astype(np.int64)
    opt_len = np.maximum(hdr_in - 20, 0)
    mss, shift, oflags = parse(buf, s["pay_off"].astype(np.int64) - opt_len, opt_len)
    window = s["window"].astype(np.int64)
    big = shift > 14
    snd_window = np.where(big, window, window << np.minimum(shift, 14))
    rcv_wscale = np.where(oflags & lm.F_WSCALE, 7, 0)
    local_mss = (mtu - 40) & 0xFFFF
    new = np.zeros(k, dtype=lm.NEW_DTYPE)
    new["local_ip"], new["foreign_ip"], new["local_port"], new["foreign_port"] = local[new_i], foreign[new_i], \
        lport[new_i], fport[new_i]
    new["pos"], new["irs"] = new_i, s["seq"]
    new["iss"] = isn(local[new_i], foreign[new_i], lport[new_i], fport[new_i], key, isn_m)
    new["snd_window"] = new["ssthresh"] = snd_window
    new["cwnd"] = np.where(mss > 2190, 2, np.where(mss > 1095, 3, 4)) * mss
    new["rcv_window"] = lm.RCV_WINDOW << rcv_wscale
    new["wl1"], new["wl2"] = s["seq"], s["ack"]
    new["snd_mss"], new["local_mss"], new["snd_wscale"], new["rcv_wscale"] = mss, local_mss, shift, rcv_wscale
    new["flags"] = oflags | np.where(big, lm.F_BIG, 0)
    has_mss, has_ws = (oflags & lm.F_MSS) != 0, (oflags & lm.F_WSCALE) != 0
    synack = np.zeros((k, 12), dtype=np.uint8)
    synack[has_mss, :4] = [2, 4, local_mss >> 8, local_mss & 0xFF]
    synack[has_mss & ~has_ws, 4:8] = [1, 1, 1, 0]
    synack[has_mss & has_ws, 4:8] = [3, 3, 7, 0]
    synack[~has_mss & has_ws, :4] = [3, 3, 7, 0]
    hdr = np.where(has_mss, 28, np.where(has_ws, 24, 20))
    out = np.zeros(k, dtype=lm.OUT_DTYPE)
    out["dst"], out["seq"], out["ack"] = foreign[new_i], new["iss"], (s["seq"].astype(np.int64) + 1) & M32
    out["sport"], out["dport"], out["window"], out["flags"], out["hdr_len"], out["mss"] = \
        lport[new_i], fport[new_i], lm.RCV_WINDOW, SYN | ACK, hdr, mss

    ri = idx[cls == lm.RESET]
    rs = seg[ri]
    rst = resets(local[ri], foreign[ri], lport[ri], fport[ri], rs["seq"].astype(np.int64), rs["ack"].astype(np.int64),
                 flags[ri], offload)
    return dict(cls=cls, new=new, synack=synack, sa_off=(32 * np.arange(k) + hdr).astype(np.uint64),
                sa_len=np.zeros(k, dtype=np.uint32), sa_out=out, rst=rst.reshape(-1),
                rst_dst=foreign[ri].astype(np.uint32),
                total=np.array([taken, k, ri.size, taken - k - ri.size], dtype=np.uint64))
