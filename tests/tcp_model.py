"""The reference's TCP layer, its stateless part, for one segment at a time
over Python ints and bytes (paths relative to the reference tree):

  hdr    tcp_hdr::read / write: ports, seq, ack, data_offset << 4 | rsvd1, the
         flags byte (FIN 1, SYN 2, RST 4, PSH 8, ACK 16, URG 32, rsvd2 << 6),
         window, checksum, urgent, all big-endian   include/seastar/net/tcp.hh:228-286
  rx     tcp::received: get_header(0, 20) null -> drop; data_offset * 4 < 20 ->
         drop; (the checksum: the frames call's L4 bit, through `need`); the
         connid {to, from, dst_port, src_port} in _tcbs; else _listening; else
         respond_with_reset                                  tcp.hh:865-942
         respond_with_reset: nothing for a RST; ports swapped, seq = SEG.ACK
         with ACK, ack = SEG.SEQ + 1 and ACK with SYN, RST, data_offset 5; the
         checksum over the pseudo-header {local, foreign, 6, 20}: ~csum.get()
         with tx_csum_l4_offload, else the full sum            tcp.hh:981-1023
         the pseudo-header                                     ip.hh:105-129
  tx     tcb::output_one: the header in front of the payload, options between;
         the three checksum forms                              tcp.hh:1620-1698

It consumes what stack_model.Rx.batch says of an IPv4 frame (its status byte
and its `delivered` flag).  tests/test_tcp_host.py pins it with frames written
out byte by byte.  fast_rx is the same rx over numpy arrays for the scale
test, pinned to the per-segment model there.  Where the batch interface has a
word the reference lacks — SHORT for a header longer than its segment, where
the reference asserts; the bucket numbers; SKIP — the model states the
interface's definition (include/sccsum.h, "TCP layer").  Nothing here reads
the code under test."""
from __future__ import annotations

import struct

import numpy as np

from stack_model import ST_IPFRAG, ST_L4_OK, ST_MALFORMED, ST_OK, ST_RANGE, TCP, be16, be32, csum, ones_sum

CONN, LISTEN, RESET, NOCONN, SHORT, SKIP = 0, 1, 2, 3, 0xFE, 0xFD
FIN, SYN, RST, PSH, ACK, URG = 1, 2, 4, 8, 16, 32
TCP_HDR = 20
NO_CONN = 0xFFFFFFFF
NEED, REJECT = ST_OK | ST_L4_OK, ST_MALFORMED | ST_RANGE | ST_IPFRAG
L4_MAX = 65515
SEG_DTYPE = np.dtype([("pay_off", "<u8"), ("pay_len", "<u4"), ("seq", "<u4"), ("ack", "<u4"), ("conn", "<u4"),
                      ("window", "<u2"), ("sport", "<u2"), ("dport", "<u2"), ("flags", "u1"), ("hdr_len", "u1")])


def pseudo_sum(src: int, dst: int, length: int) -> int:
    """ipv4_traits::tcp_pseudo_header_checksum folded (ip.hh:70-75)."""
    return ones_sum(struct.pack(">IIBBH", src, dst, 0, TCP, length & 0xFFFF))


# ---------------------------------------------------------------- the header

def hdr_read(p: bytes) -> dict:
    """tcp_hdr::read (tcp.hh:246-265)."""
    return dict(sport=be16(p, 0), dport=be16(p, 2), seq=be32(p, 4), ack=be32(p, 8), rsvd1=p[12] & 15,
                data_offset=p[12] >> 4, flags=p[13], window=be16(p, 14), checksum=be16(p, 16), urgent=be16(p, 18))


def hdr_write(sport=0, dport=0, seq=0, ack=0, data_offset=5, flags=0, window=0, checksum=0, urgent=0, rsvd1=0) -> bytes:
    """tcp_hdr::write (tcp.hh:266-282)."""
    return struct.pack(">HHIIBBHHH", sport, dport, seq & 0xFFFFFFFF, ack & 0xFFFFFFFF, rsvd1 | (data_offset << 4),
                       flags, window, checksum, urgent)


def bucket_of(cls: int) -> int:
    """The interface's buckets: 0 CONN, 1 LISTEN, 2 RESET, 3 everything dropped."""
    return cls if cls in (CONN, LISTEN, RESET) else 3


# ---------------------------------------------------------------- rx

def respond_with_reset(h: dict, local_ip: int, foreign_ip: int, offload: bool = False):
    """tcp.hh:981-1023: the twenty bytes sent to foreign_ip, or None for a RST."""
    if h["flags"] & RST:
        return None
    seq = h["ack"] if h["flags"] & ACK else 0
    ack, fl = 0, RST
    if h["flags"] & SYN:
        ack, fl = (h["seq"] + 1) & 0xFFFFFFFF, RST | ACK
    zero = hdr_write(h["dport"], h["sport"], seq, ack, 5, fl, 0, 0, 0)
    seed = pseudo_sum(local_ip, foreign_ip, TCP_HDR)
    field = seed if offload else csum(zero, seed)      # ~csum.get() is the folded sum itself
    return zero[:16] + field.to_bytes(2, "big") + zero[18:]


def received(l4: bytes, src: int, dst: int, tcbs: dict, listening) -> dict:
    """tcp::received on the packet behind its IP header (from = src, to = dst):
    cls; for the classes that parse the header the fields of it, H, and the
    payload length E - H (0 where H > E); conn for a known connection."""
    out = dict(cls=SHORT, conn=NO_CONN, hdr=None, H=0, pay_len=0, src=0, dst=0)
    E = len(l4)
    if E < TCP_HDR:                                    # get_header(0, tcp_hdr::len) is null
        return out
    H = 4 * (l4[12] >> 4)
    if H < TCP_HDR:
        return out
    h = hdr_read(l4)
    cid = (dst, src, h["dport"], h["sport"])           # connid{to, from, h.dst_port, h.src_port}
    full = dict(hdr=h, H=H, pay_len=max(E - H, 0), src=src, dst=dst)
    if cid in tcbs:
        if H > E:                                      # the reference asserts in trim_front: the interface drops it
            return out
        return dict(full, cls=CONN, conn=tcbs[cid])
    if h["dport"] in listening:
        if H > E:
            return out
        return dict(full, cls=LISTEN, conn=NO_CONN)
    return dict(full, cls=NOCONN if h["flags"] & RST else RESET, conn=NO_CONN)


def atomic(p: bytes, info: dict, tcbs: dict, listening, need: int = NEED, reject: int = REJECT) -> dict:
    """A frame of the IPv4 bucket (p: the bytes behind its Ethernet header)
    with what stack_model says of it.  SKIP is the interface's word: the
    masks, not delivered to an L4 (ip.cc:121-162, fragments are reassembly's),
    not TCP.  at: where the payload starts in p."""
    out = dict(cls=SKIP, conn=NO_CONN, hdr=None, H=0, pay_len=0, src=0, dst=0, at=0)
    st = info["status"]
    if (st & need) != need or (st & reject) != 0 or not info["delivered"] or p[9] != TCP:
        return out
    ihl, ip_len = p[0] & 0xF, be16(p, 2)
    l4 = p[:ip_len][4 * ihl:]                          # trim_back to the IP length, trim_front(ip_hdr_len)
    out.update(received(l4, be32(p, 12), be32(p, 16), tcbs, listening))
    if out["hdr"] is not None:
        out["at"] = 4 * ihl + out["H"]
    return out


def seg_record(it: dict, off: int) -> tuple:
    """sccsum_tcp_seg of an item whose frame lies at `off` (None: index out of range)."""
    base = 0 if off is None else off
    h = it["hdr"]
    if h is None:
        return (base, 0, 0, 0, NO_CONN, 0, 0, 0, 0, 0)
    return (base + it["at"], it["pay_len"], h["seq"], h["ack"], it["conn"], h["window"], h["sport"], h["dport"],
            h["flags"], it["H"])


def expect_rx(items: list, off, index=None, offload: bool = False) -> dict:
    """items: atomic() results in the call's order (item j belongs to batch
    frame index[j]); off: the batch's frame offsets.  Every array
    sccsum_tcp_rx writes; pos: the call positions in grouped order."""
    n = len(items)
    idx = list(range(n)) if index is None else [int(x) for x in index]
    key = [(bucket_of(it["cls"]), it["conn"] if it["cls"] == CONN else 0) for it in items]
    pos = sorted(range(n), key=lambda j: key[j])       # stable
    first = [sum(1 for k in key if k[0] < b) for b in range(4)] + [n]
    seg = np.zeros(n, dtype=SEG_DTYPE)
    for p, j in enumerate(pos):
        seg[p] = seg_record(items[j], int(off[idx[j]]) if idx[j] < len(off) else None)
    run_conn, run_first = [], []
    for p in range(first[1]):
        c = items[pos[p]]["conn"]
        if not run_conn or run_conn[-1] != c:
            run_conn.append(c)
            run_first.append(p)
    run_first.append(first[1])
    rst = b"".join(respond_with_reset(items[j]["hdr"], items[j]["dst"], items[j]["src"], offload)
                   for j in pos[first[2]:first[3]])
    return dict(cls=np.array([it["cls"] for it in items], dtype=np.uint8), first=np.array(first, dtype=np.uint32),
                order=np.array([idx[j] for j in pos], dtype=np.uint32), pos=pos, seg=seg,
                src=np.array([items[j]["src"] for j in pos], dtype=np.uint32),
                run_conn=np.array(run_conn, dtype=np.uint32), run_first=np.array(run_first, dtype=np.uint32),
                rst=np.frombuffer(rst, dtype=np.uint8), rst_dst=np.array([items[j]["src"] for j in pos[first[2]:first[3]]],
                                                                        dtype=np.uint32),
                total=np.array([len(run_conn), first[3] - first[2], 0, 0], dtype=np.uint64))


# ---------------------------------------------------------------- tx

def send(payload: bytes, o: dict, src: int, options: bytes = b"", offload: bool = False, tso: bool = False) -> dict:
    """tcb::output_one's header and checksum forms.  o: dst, seq, ack, sport,
    dport, window, flags, mss.  l4 = the segment as it leaves, zero = the same
    with the field zero (what stack_model.tx takes)."""
    hdr_len = TCP_HDR + len(options)
    zero = hdr_write(o["sport"], o["dport"], o["seq"], o["ack"], hdr_len // 4, o["flags"], o["window"]) + options \
        + bytes(payload)
    if offload:
        big = tso and len(payload) > o["mss"]
        field = pseudo_sum(src, o["dst"], 0 if big else len(zero))
        tso_seg, needs = (o["mss"] if big else 0), True
    else:
        field, tso_seg, needs = csum(zero, pseudo_sum(src, o["dst"], len(zero))), 0, False
    return dict(l4=zero[:16] + field.to_bytes(2, "big") + zero[18:], zero=zero, needs_csum=needs, tso_seg=tso_seg)


def send_status(off: int, length: int, hdr_len: int, bytes_len: int, tso_flag: bool, mss: int) -> int:
    """The interface's refusals (include/sccsum.h, "TCP layer")."""
    st = 0
    if off < hdr_len or off > bytes_len or length > bytes_len - off:
        st |= ST_RANGE
    if hdr_len < 20 or hdr_len > 60 or hdr_len % 4 or length + hdr_len > L4_MAX or (tso_flag and mss == 0):
        st |= ST_MALFORMED
    return st


# ---------------------------------------------------------------- the same rx over arrays

def _at(data: np.ndarray, idx: np.ndarray) -> np.ndarray:
    return data[idx.astype(np.int64)].astype(np.int64)


def _be(data, a, nbytes):
    v = np.zeros(a.shape, dtype=np.int64)
    for k in range(nbytes):
        v = (v << 8) | _at(data, a + k)
    return v


def _lookup(conns: np.ndarray, lip, fip, lport, fport) -> np.ndarray:
    """_tcbs.find for arrays: the index of (lip, fip, lport, fport) in conns, or -1.
    Exact: the address pairs are ranked first, rank << 32 | ports then fits 64 bits."""
    if conns.shape[0] == 0:
        return np.full(lip.shape, -1, dtype=np.int64)
    pair = (conns[:, 0].astype(np.uint64) << np.uint64(32)) | conns[:, 1].astype(np.uint64)
    upair, rank = np.unique(pair, return_inverse=True)
    key = (rank.astype(np.uint64) << np.uint64(32)) | ((conns[:, 2] << 16) | conns[:, 3]).astype(np.uint64)
    by_key = np.argsort(key, kind="stable")
    skey = key[by_key]
    fpair = (lip.astype(np.uint64) << np.uint64(32)) | fip.astype(np.uint64)
    r = np.minimum(np.searchsorted(upair, fpair), upair.size - 1)
    fkey = (r.astype(np.uint64) << np.uint64(32)) | ((lport << 16) | fport).astype(np.uint64)
    at = np.minimum(np.searchsorted(skey, fkey), skey.size - 1)
    hit = (upair[r] == fpair) & (skey[at] == fkey)
    return np.where(hit, by_key[at], -1).astype(np.int64)


def fast_rx(data: np.ndarray, bytes_len: int, off, length, status, need: int, reject: int, host: int, conns, listen,
            index=None) -> dict:
    """sccsum_tcp_rx's contract over numpy arrays (no resets: the scale test's
    traffic has few and compares them through the per-segment model).  conns:
    int64 [nconns, 4] (local_ip, foreign_ip, local_port, foreign_port)."""
    off, length = np.asarray(off).astype(np.uint64), np.asarray(length).astype(np.uint64)
    nbatch = int(off.size)
    idx = np.arange(nbatch, dtype=np.int64) if index is None else np.asarray(index).astype(np.int64)
    n = int(idx.size)
    known = idx < nbatch
    i = np.where(known, idx, 0)
    o, ln = off[i], length[i]
    st = np.asarray(status).astype(np.int64)[i]
    blen = np.uint64(bytes_len)
    inside = o <= blen
    inside &= ln <= blen - np.where(inside, o, blen)
    ok = known & ((st & need) == need) & ((st & reject) == 0) & inside & (ln >= 20)
    a = np.where(ok, o, 0).astype(np.int64)
    ihl4 = 4 * (_at(data, a) & 0xF)
    ip_len = _be(data, a + 2, 2)
    ok &= (ln.astype(np.int64) >= ip_len) & (ihl4 <= ip_len)
    frag = _be(data, a + 6, 2) & 0x3FFF
    src, dst = _be(data, a + 12, 4), _be(data, a + 16, 4)
    ok &= (frag == 0) & ((dst == host) | (host == 0)) & (_at(data, a + 9) == TCP)
    E = ip_len - ihl4
    t = np.where(ok & (E >= 20), a + ihl4, 0)
    H = 4 * (_at(data, t + 12) >> 4)
    parsed = ok & (E >= 20) & (H >= 20)
    sport, dport = _be(data, t, 2), _be(data, t + 2, 2)
    flags = _at(data, t + 13)
    conns = np.asarray(conns, dtype=np.int64).reshape(-1, 4)
    nconns = conns.shape[0]
    conn = np.where(parsed, _lookup(conns, dst, src, dport, sport), -1)
    lis = np.zeros(65536, dtype=bool)
    lis[np.asarray(listen, dtype=np.int64)] = True
    cls = np.full(n, SKIP, dtype=np.int64)
    cls[ok] = SHORT
    owned = parsed & ((conn >= 0) | lis[dport])
    cls[parsed & (conn >= 0) & (H <= E)] = CONN
    cls[parsed & (conn < 0) & lis[dport] & (H <= E)] = LISTEN
    cls[parsed & ~owned & ((flags & RST) == 0)] = RESET
    cls[parsed & ~owned & ((flags & RST) != 0)] = NOCONN
    has = cls <= NOCONN
    key = np.where(cls == CONN, conn, nconns + np.where(cls == LISTEN, 0, np.where(cls == RESET, 1, 2)))
    order = np.argsort(key, kind="stable")
    bucket = np.where(cls <= RESET, cls, 3)
    first = np.concatenate([[0], np.cumsum(np.bincount(bucket, minlength=4))]).astype(np.uint32)
    seg = np.zeros(n, dtype=SEG_DTYPE)
    seg["pay_off"] = np.where(has, o + (ihl4 + H).astype(np.uint64), np.where(known, o, 0))[order]
    seg["pay_len"] = np.where(has, np.maximum(E - H, 0), 0)[order]
    seg["seq"] = np.where(has, _be(data, t + 4, 4), 0)[order]
    seg["ack"] = np.where(has, _be(data, t + 8, 4), 0)[order]
    seg["conn"] = np.where(cls == CONN, conn, NO_CONN)[order]
    seg["window"] = np.where(has, _be(data, t + 14, 2), 0)[order]
    seg["sport"] = np.where(has, sport, 0)[order]
    seg["dport"] = np.where(has, dport, 0)[order]
    seg["flags"] = np.where(has, flags, 0)[order]
    seg["hdr_len"] = np.where(has, H, 0)[order]
    sk = key[order][:first[1]]
    heads = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]])) if sk.size else np.zeros(0, np.int64)
    return dict(cls=cls.astype(np.uint8), first=first, order=idx[order].astype(np.uint32), seg=seg,
                src=np.where(has, src, 0)[order].astype(np.uint32), run_conn=sk[heads].astype(np.uint32),
                run_first=np.concatenate([heads, [first[1]]]).astype(np.uint32))
