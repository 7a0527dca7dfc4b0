"""Vectorised expectations for batches too large for the per-record models
(reasm_model.run, test_send_host.expected_send, test_gpu_reasm._expected_records
take about 20 s per million entries).  numpy only; the header checksums come
from the oracle.  Each function covers the part of its interface a large
generated input needs and says so; tests/test_fast_models.py pins each one to
the slow model on inputs small enough for it.  Nothing here reads the code
under test."""
from __future__ import annotations

import numpy as np

import oracle

REC_DTYPE = np.dtype([("frame", "<u8"), ("src", "<u4"), ("dst", "<u4"), ("id", "<u2"), ("proto", "u1"), ("mf", "u1"),
                      ("offset", "<u2"), ("hdr_len", "<u2"), ("len", "<u2"), ("reserved", "<u2"), ("tag", "<u4")])
DESC_DTYPE = np.dtype([("src", "<u8"), ("dst_off", "<u4"), ("len", "<u4")])
COMPLETE, PENDING, HOST = 1, 2, 3
ST_OK = 1


def key_mix(src, dst, ident, proto):
    """sccsum_reasm_key_mix (include/sccsum.h) over uint32 arrays: three rounds
    of the murmur3 finaliser."""
    src, dst, ident, proto = (np.asarray(a).astype(np.uint32) for a in (src, dst, ident, proto))

    def fmix(h):
        h = h ^ (h >> np.uint32(16))
        h = h * np.uint32(0x85EBCA6B)
        h = h ^ (h >> np.uint32(13))
        h = h * np.uint32(0xC2B2AE35)
        return h ^ (h >> np.uint32(16))
    with np.errstate(over="ignore"):
        h = fmix(src + np.uint32(0x9E3779B9))
        h = fmix(h ^ dst)
        return fmix(h + ((ident << np.uint32(8)) | proto) * np.uint32(0x9E3779B1))


def pseudo_seeds(src, dst, proto, length):
    """The folded pseudo-header sum of ip.hh:70-75 per row (what
    oracle.pseudo_seed gives for one), 0 for protocols other than TCP / UDP."""
    s = src.astype(np.uint64) + dst.astype(np.uint64) + proto.astype(np.uint64) + (length.astype(np.uint64) & 0xFFFF)
    for _ in range(3):
        s = (s & np.uint64(0xFFFF)) + (s >> np.uint64(16))
    return np.where((proto == 6) | (proto == 17), s, 0).astype(np.uint32)


def reasm_plain(recs: np.ndarray, mix=key_mix, cap: int = 0xFFFFFFFF) -> dict:
    """Everything sccsum_ipv4_reasm writes for records (REC_DTYPE, arrival
    order) whose keys are all PLAIN: no empty piece, no overlap, at most one
    MF-clear record and that one last in offset order (asserted).  Such a key
    completes when its records tile [0, E) and the MF-clear one is there, at
    the last of them to arrive (sccsum.h, "Rx reassembly").

    Records are ordered by the full key, then offset, then arrival — never by
    the mix.  mix(src, dst, id, proto): keys that share a value go to the host
    whole (None: no key does).  cap: the prefix rule; the keys of the datagrams
    that do not fit are pending.

    Returns state [m], and for the D emitted datagrams in completion order
    first [D + 1], off, len, head, last, seed, rows (the K records behind the
    descriptors, in order), desc [K], then pending / host (records in arrival
    order) and total = (D, K, pending, host)."""
    m = recs.size
    out = dict(state=np.zeros(m, np.uint8), first=np.zeros(1, np.uint32), off=np.zeros(0, np.uint64),
               len=np.zeros(0, np.uint32), head=np.zeros(0, np.uint32), last=np.zeros(0, np.uint32),
               seed=np.zeros(0, np.uint32), rows=np.zeros(0, np.int64), desc=np.zeros(0, DESC_DTYPE),
               pending=recs[:0], host=recs[:0], total=(0, 0, 0, 0))
    if m == 0:
        return out
    arrival = np.arange(m, dtype=np.int64)
    order = np.lexsort((arrival, recs["offset"], recs["proto"], recs["id"], recs["dst"], recs["src"]))
    s = recs[order]
    beg = s["offset"].astype(np.int64)
    end = beg + s["len"].astype(np.int64)
    same = np.zeros(m, bool)
    same[1:] = ((s["src"][1:] == s["src"][:-1]) & (s["dst"][1:] == s["dst"][:-1]) & (s["id"][1:] == s["id"][:-1])
                & (s["proto"][1:] == s["proto"][:-1]))
    start = np.flatnonzero(~same)                       # a key's first sorted position
    count = np.diff(np.append(start, m))
    tail = start + count - 1
    prev_end = np.concatenate([[0], end[:-1]])
    prev_mf = np.concatenate([[1], s["mf"][:-1]])
    assert np.all(s["len"] > 0), "not plain: an empty piece"
    assert np.all(~same | ((prev_end <= beg) & (prev_mf != 0))), "not plain: an overlap, or a record after the MF-clear one"
    gap = np.where(same, prev_end != beg, beg != 0)
    whole = (np.add.reduceat(gap.astype(np.int64), start) == 0) & (s["mf"][tail] == 0)
    last = np.maximum.reduceat(order, start)            # the key's latest arrival
    gstate = np.where(whole, COMPLETE, PENDING).astype(np.uint8)
    if mix is not None:
        g = s[start]
        mx = mix(g["src"], g["dst"], g["id"], g["proto"])
        by_mix = np.argsort(mx, kind="stable")
        ms = mx[by_mix]
        dup = np.zeros(ms.size, bool)
        dup[1:] = ms[1:] == ms[:-1]
        dup[:-1] |= dup[1:]
        gstate[by_mix[dup]] = HOST
    # datagrams: the complete keys by their completing record, then the capacity prefix
    done = np.flatnonzero(gstate == COMPLETE)
    done = done[np.argsort(last[done], kind="stable")]
    length = end[tail[done]]
    fits = int(np.searchsorted(np.cumsum(length), int(cap), side="right"))  # lengths > 0: the sums strictly grow
    gstate[done[fits:]] = PENDING
    done, length = done[:fits], length[:fits]
    state = np.empty(m, np.uint8)
    state[order] = np.repeat(gstate, count)
    D = done.size
    cnt = count[done]
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(length)]).astype(np.uint64)[:D]
    K = int(first[-1])
    pos = np.repeat(start[done], cnt) + (np.arange(K, dtype=np.int64) - np.repeat(first[:-1], cnt))
    rows = order[pos]
    desc = np.zeros(K, DESC_DTYPE)
    r = recs[rows]
    desc["src"] = r["frame"] + r["hdr_len"].astype(np.uint64)
    desc["dst_off"] = ((np.repeat(off, cnt) + r["offset"].astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    desc["len"] = r["len"]
    h = s[start[done]]
    pend, host = recs[state == PENDING], recs[state == HOST]
    out.update(state=state, first=first.astype(np.uint32), off=off, len=length.astype(np.uint32),
               head=order[start[done]].astype(np.uint32), last=last[done].astype(np.uint32),
               seed=pseudo_seeds(h["src"], h["dst"], h["proto"], length), rows=rows, desc=desc, pending=pend,
               host=host, total=(D, K, pend.size, host.size))
    return out


def plain_udp_records(rng, n: int, dsts=(0xC0A80A63, 0xC0A80B63), open_share: float = 0.1):
    """Exactly n hand-built records of UDP datagrams with plain keys, in a random
    arrival order, and the payload buffer they point into: keys of 1, 2, 3, 5 or
    9 pieces, every piece but a key's last 8, 16, 24, 32 or 40 bytes, the last
    8-40; about `open_share` of the keys open (one piece left out, or the last
    one still MF).  hdr_len is 20, frame = 44 + the piece's position in the
    buffer (add the buffer's address), tag = the key's number.  Returns (records, buffer)."""
    nk = n // 2 + 16                                     # more keys than n records need
    pieces = rng.choice([1, 2, 3, 5, 9], size=nk)
    first = np.concatenate([[0], np.cumsum(pieces)])
    total = int(first[-1])
    key_of = np.repeat(np.arange(nk), pieces)
    j = np.arange(total) - first[key_of]                 # the piece's number in its key
    is_last = j == pieces[key_of] - 1
    ln = np.where(is_last, rng.integers(8, 41, total), 8 * rng.integers(1, 6, total))
    run = np.cumsum(ln)
    kbeg = np.concatenate([[0], run[first[1:-1] - 1]])   # bytes before each key's datagram
    offset = run - ln - kbeg[key_of]
    mf = (~is_last).astype(np.uint8)
    kind = rng.random(nk)
    still_mf = kind < open_share / 2                     # open: the last piece says more follow
    mf[is_last & still_mf[key_of]] = 1
    hole = (kind >= open_share / 2) & (kind < open_share) & (pieces > 1)   # open: one piece never arrives
    gone = first[:-1] + rng.integers(0, 9, nk) % pieces
    keep = np.ones(total, bool)
    keep[gone[hole]] = False
    have = np.cumsum(np.add.reduceat(keep.astype(np.int64), first[:-1]))
    nkeys = int(np.searchsorted(have, n, side="right"))  # whole keys only; single-piece keys make up the rest
    short = n - (int(have[nkeys - 1]) if nkeys else 0)
    assert nkeys < nk - short
    sel = keep & (key_of < nkeys)
    pad = np.flatnonzero((pieces == 1) & (np.arange(nk) >= nkeys))[:short]
    assert pad.size == short
    sel[first[pad]] = True
    idx = np.flatnonzero(sel)
    recs = np.zeros(n, REC_DTYPE)
    recs["frame"] = (44 + run - ln - 20)[idx]
    recs["src"] = rng.integers(1, 2**32, nk, dtype=np.uint64).astype(np.uint32)[key_of[idx]]
    recs["dst"] = np.asarray(dsts, np.uint32)[rng.integers(0, len(dsts), nk)][key_of[idx]]
    recs["id"] = rng.integers(0, 65536, nk).astype(np.uint16)[key_of[idx]]
    recs["proto"], recs["hdr_len"] = 17, 20
    recs["mf"], recs["offset"], recs["len"], recs["tag"] = mf[idx], offset[idx], ln[idx], key_of[idx]
    recs = recs[rng.permutation(n)]
    buf = rng.integers(0, 256, 44 + int(run[-1]) + 16, dtype=np.uint8)
    return recs, buf


def send_headers(total_len, ident, frag, proto, src, dst) -> np.ndarray:
    """[E, 20] IPv4 headers as ipv4::send writes them (ip.cc:249-281): version
    4, ihl 5, ttl 64, the checksum over the 20 bytes from the oracle."""
    e = total_len.size
    h = np.zeros((e, 20), np.uint8)
    h[:, 0] = 0x45
    for at, v in ((2, total_len), (4, ident), (6, frag)):
        h[:, at], h[:, at + 1] = v >> 8, v & 0xFF
    h[:, 8], h[:, 9] = 64, proto
    for at, v in ((12, np.broadcast_to(np.uint32(src), (e,))), (16, dst)):
        for b in range(4):
            h[:, at + b] = (v >> (24 - 8 * b)) & 0xFF
    if e:
        c = oracle.batch_spans(h.reshape(-1), 20 * np.arange(e, dtype=np.uint64), np.full(e, 20, np.uint32))
        h[:, 10:12] = c.view(np.uint8).reshape(e, 2)
    return h


def send_plain(lens, dst, proto, ids, mtu, src, max_frames=0x7FFFFFFF, max_out_bytes=0xFFFFFFFF) -> dict:
    """What sccsum_ipv4_send writes for datagrams that are all in range
    (len <= 65515, inside the buffer), flags 0 and (mtu - 20) % 8 == 0
    (sccsum.h, "Tx send").  Returns dgram_first [n + 1], per emitted frame
    owner / piece_off / out_off / out_len / hdr [E, 20], first [E + 1],
    status [n], total = (frames needed, bytes needed, prefix)."""
    lens = np.asarray(lens).astype(np.int64)
    dst, proto, ids = np.asarray(dst, np.uint32), np.asarray(proto, np.uint8), np.asarray(ids, np.uint16)
    n, room = lens.size, int(mtu) - 20
    assert room % 8 == 0 and (n == 0 or lens.max() <= 65515)
    cut = lens + 20 > mtu
    nf = np.where(cut, -(-lens // room), 1)
    nb = lens + 20 * nf
    cf, cb = np.cumsum(nf), np.cumsum(nb)
    prefix = int(np.count_nonzero((cf <= max_frames) & (cb <= max_out_bytes)))  # both sums strictly grow
    emitted = int(cf[prefix - 1]) if prefix else 0
    dgram_first = np.full(n + 1, emitted, np.int64)
    dgram_first[:prefix] = cf[:prefix] - nf[:prefix]
    status = np.zeros(n, np.uint8)
    status[:prefix] = ST_OK
    owner = np.repeat(np.arange(prefix, dtype=np.int64), nf[:prefix])
    k = np.arange(emitted, dtype=np.int64) - dgram_first[owner]
    ln, c = lens[owner], cut[owner]
    o = np.where(c, k * room, 0)
    piece = np.where(c, np.minimum(room, ln - o), ln)
    frag = np.where(c, np.where(o + piece < ln, 0x2000, 0) | (o >> 3), 0)
    out_len = (20 + piece).astype(np.uint32)
    out_off = np.concatenate([[0], np.cumsum(out_len, dtype=np.uint64)]).astype(np.uint64)[:emitted]
    hdr = send_headers(20 + piece, ids[owner].astype(np.int64), frag, proto[owner], src, dst[owner])
    return dict(dgram_first=dgram_first.astype(np.uint32), owner=owner, piece_off=o, out_off=out_off, out_len=out_len,
                hdr=hdr, first=(2 * np.arange(emitted + 1)).astype(np.uint32), status=status,
                total=(int(cf[-1]) if n else 0, int(cb[-1]) if n else 0, prefix), emitted=emitted)


def frag_records_plain(frames2d, off, lens, status, need, reject, host, base, tag):
    """The records sccsum_ipv4_frag_records writes for frames2d[i, :lens[i]]
    lying at address base + off[i], by the rules of ip.cc:128-166 as
    test_gpu_reasm._expected_records states them, with the status an input: a
    frame is accepted when (status & need) == need and (status & reject) == 0 —
    the masks stand for the header checksum and "is a fragment", which the
    frames call records in the status — it holds its 20-byte header and its IP
    total length, 4 * ihl is inside that length, offset + length is at most
    65535, and its destination is `host` (0: any).  Returns (records, accepted
    mask, header mask): accepted = status mask & header mask."""
    f = np.asarray(frames2d, np.uint8)
    lens, status = np.asarray(lens).astype(np.int64), np.asarray(status, np.uint8)
    assert f.shape[1] >= 20
    by_status = ((status & np.uint8(need)) == np.uint8(need)) & ((status & np.uint8(reject)) == 0)

    def be16(at):
        return (f[:, at].astype(np.int64) << 8) | f[:, at + 1]

    def be32(at):
        return ((f[:, at].astype(np.uint32) << 24) | (f[:, at + 1].astype(np.uint32) << 16)
                | (f[:, at + 2].astype(np.uint32) << 8) | f[:, at + 3])
    hdr_len = 4 * (f[:, 0].astype(np.int64) & 0xF)
    ip_len, w = be16(2), be16(6)
    offset = (w & 0x1FFF) << 3
    dst = be32(16)
    by_header = ((lens >= 20) & (lens >= ip_len) & (hdr_len <= ip_len) & (offset + ip_len <= 65535)
                 & ((dst == np.uint32(host)) | (host == 0)))
    ok = by_status & by_header
    rec = np.zeros(int(np.count_nonzero(ok)), REC_DTYPE)
    rec["frame"] = np.uint64(base) + np.asarray(off, np.uint64)[ok]
    rec["src"], rec["dst"] = be32(12)[ok], dst[ok]
    rec["id"], rec["proto"] = be16(4)[ok], f[ok, 9]
    rec["mf"], rec["offset"] = ((w >> 13) & 1)[ok], offset[ok]
    rec["hdr_len"], rec["len"] = hdr_len[ok], (ip_len - hdr_len)[ok]
    rec["tag"] = tag
    return rec, by_status, by_header
