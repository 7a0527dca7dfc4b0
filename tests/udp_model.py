"""The reference's UDP layer for one datagram at a time, over Python ints and
bytes (paths relative to the reference tree):

  rx   ipv4::handle_received_packet, its end: dst != _host_address is dropped;
       _l4[h.ip_proto]; the trim to the IP total length (lines 134-136) and
       trim_front(ip_hdr_len)                                 src/net/ip.cc:159-162, 222-227
       native_datagram: hdr = get_header<udp_hdr>() (null below 8 bytes, and
       dereferenced), ntoh, trim_front(8); the rest is the datagram, whatever
       hdr.len says                                           src/net/udp.cc:45-53
       ipv4_udp::received: _channels.find(dst_port), unknown: dropped;
       chan->_queue.push (drops when the queue is full)       udp.cc:164-173, queue.hh:184-192
  tx   ipv4_udp::send: prepend_header<udp_hdr>, src_port, dst_port, len =
       p.len(), hton; the pseudo-header sum; with tx_csum_l4_offload and no
       fragmentation cksum = ~csum.get() and needs_csum, otherwise the full
       sum                                                    udp.cc:175-197
       ipv4::needs_frag                                       ip.cc:100-111

It consumes what stack_model.Rx.batch delivers — an atomic frame's info with
its `delivered` flag, and the `delivered` list of reassembled datagrams — and
its send() feeds stack_model.tx.  tests/test_udp_host.py pins it with frames
written out byte by byte.  fast_rx is the same rx over numpy arrays for the
scale test, pinned to the per-datagram model there.  Where the batch interface
has a word the reference lacks (a class for a dropped frame) the model states
the interface's definition (include/sccsum.h, "UDP layer").  Nothing here
reads the code under test."""
from __future__ import annotations

import struct

import numpy as np

from stack_model import UDP, be16, be32, csum, ones_sum

SKIP, SHORT, NOPORT = 0xFD, 0xFE, 0xFF      # classes of dropped frames (sccsum.h, "UDP layer")
UDP_HDR = 8
QUEUE_SIZE = 1024                            # ipv4_udp::default_queue_size
PAYLOAD_MAX = 65515 - UDP_HDR


def pseudo_sum(src: int, dst: int, length: int) -> int:
    """ipv4_traits::udp_pseudo_header_checksum folded (ip.hh:70-75)."""
    return ones_sum(struct.pack(">IIBBH", src, dst, 0, UDP, length & 0xFFFF))


# ---------------------------------------------------------------- rx

def received(l4: bytes, src: int, ports: dict) -> dict:
    """ipv4_udp::received on the packet behind its IP header: cls, and for a
    datagram with a channel its payload, source address and source port."""
    out = dict(cls=SHORT, payload=b"", src=0, sport=0)
    if len(l4) < UDP_HDR:                    # get_header<udp_hdr> is null; the interface drops the frame
        return out
    sport, dport = be16(l4, 0), be16(l4, 2)
    k = ports.get(dport)
    if k is None:
        out["cls"] = NOPORT
        return out
    return dict(cls=k, payload=bytes(l4[UDP_HDR:]), src=src, sport=sport)   # hdr.len is not consulted


def atomic(p: bytes, delivered: bool, ports: dict) -> dict:
    """A frame of the IPv4 bucket (p: the bytes behind its Ethernet header)
    that stack_model delivered to its L4 (or did not).  at: where the payload
    starts in p."""
    out = dict(cls=SKIP, payload=b"", src=0, sport=0, at=0)
    if not delivered or p[9] != UDP:
        return out
    ihl, ip_len = p[0] & 0xF, be16(p, 2)
    l4 = p[:ip_len][4 * ihl:]                # trim_back to the IP length, trim_front(ip_hdr_len)
    out.update(received(l4, be32(p, 12), ports))
    if out["cls"] < SKIP:
        out["at"] = 4 * ihl + UDP_HDR
    return out


def reassembled(d: dict, ports: dict) -> dict:
    """A datagram of stack_model's `delivered` list (ip.cc:186-189)."""
    if d["proto"] != UDP:
        return dict(cls=SKIP, payload=b"", src=0, sport=0)
    return received(d["data"], d["src"], ports)


def queue(classes, nchannels: int, room) -> list:
    """_queue.push per channel: the positions (into classes) of the datagrams
    each channel accepts with room[k] free slots, in order."""
    out = [[] for _ in range(nchannels)]
    for j, c in enumerate(classes):
        if c < nchannels and len(out[c]) < room[c]:
            out[c].append(j)
    return out


# ---------------------------------------------------------------- tx

def needs_frag(l4_len: int, mtu: int, ufo: bool) -> bool:
    return l4_len + 20 > mtu and not ufo


def send(payload: bytes, sport: int, dport: int, src: int, dst: int, mtu: int, offload: bool = False,
         ufo: bool = False) -> dict:
    """ipv4_udp::send: l4 = the datagram as it leaves (header + payload, the
    checksum field as send stores it), zero = the same with the field zero
    (what stack_model.tx takes), needs_csum = oi.needs_csum."""
    length = len(payload) + UDP_HDR
    zero = struct.pack(">HHHH", sport, dport, length & 0xFFFF, 0) + bytes(payload)
    seed = pseudo_sum(src, dst, length)
    if offload and not needs_frag(length, mtu, ufo):
        field, needs = seed, True            # ~csum.get(): the folded sum itself
    else:
        field, needs = csum(zero, seed), False
    return dict(l4=zero[:6] + field.to_bytes(2, "big") + zero[8:], zero=zero, needs_csum=needs)


# ---------------------------------------------------------------- the same rx over arrays

def _u64(a) -> np.ndarray:
    return np.asarray(a).astype(np.uint64)


def _at(data: np.ndarray, idx: np.ndarray) -> np.ndarray:
    return data[idx.astype(np.int64)].astype(np.int64)


def fast_rx(data: np.ndarray, bytes_len: int, off, length, status, need: int, reject: int, host: int, ports,
            index=None) -> dict:
    """sccsum_udp_rx's contract over numpy arrays: cls [n] in the call's order;
    first [C + 2]; order, pay_off, pay_len, src, sport [n] in grouped order."""
    off, length = _u64(off), _u64(length)
    nbatch, nch = int(off.size), len(ports)
    idx = np.arange(nbatch, dtype=np.int64) if index is None else np.asarray(index).astype(np.int64)
    n = int(idx.size)
    known = idx < nbatch
    i = np.where(known, idx, 0)
    if nbatch == 0:
        off, length, status = np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint8)
    o, ln = off[i], length[i]
    st = np.asarray(status).astype(np.int64)[i]
    blen = np.uint64(bytes_len)
    inside = o <= blen
    inside &= ln <= blen - np.where(inside, o, blen)
    ok = known & ((st & need) == need) & ((st & reject) == 0) & inside & (ln >= 20)
    a = np.where(ok, o, 0).astype(np.int64)
    if data.size < 20:
        data = np.zeros(20, np.uint8)
    hdr_len = 4 * (_at(data, a) & 0xF)
    ip_len = (_at(data, a + 2) << 8) | _at(data, a + 3)
    ok &= (ln.astype(np.int64) >= ip_len) & (hdr_len <= ip_len)
    frag = ((_at(data, a + 6) << 8) | _at(data, a + 7)) & 0x3FFF
    dst = (_at(data, a + 16) << 24) | (_at(data, a + 17) << 16) | (_at(data, a + 18) << 8) | _at(data, a + 19)
    src = (_at(data, a + 12) << 24) | (_at(data, a + 13) << 16) | (_at(data, a + 14) << 8) | _at(data, a + 15)
    ok &= (frag == 0) & ((dst == host) | (host == 0)) & (_at(data, a + 9) == UDP)
    l4_len = ip_len - hdr_len
    short = ok & (l4_len < UDP_HDR)
    full = ok & ~short
    u = np.where(full, a + hdr_len, 0)
    sport = (_at(data, u) << 8) | _at(data, u + 1)
    dport = (_at(data, u + 2) << 8) | _at(data, u + 3)
    table = np.full(65536, NOPORT, dtype=np.int64)
    table[np.asarray(ports, dtype=np.int64)] = np.arange(nch)
    cls = np.full(n, SKIP, dtype=np.int64)
    cls[short] = SHORT
    cls[full] = table[dport[full]]
    has = cls < nch
    bucket = np.where(has, cls, nch)
    order = np.argsort(bucket, kind="stable")
    first = np.concatenate([[0], np.cumsum(np.bincount(bucket, minlength=nch + 1))]).astype(np.uint32)
    return dict(cls=cls.astype(np.uint8), first=first, order=idx[order].astype(np.uint32),
                pay_off=np.where(has, o + _u64(hdr_len + UDP_HDR), np.where(known, o, 0))[order].astype(np.uint64),
                pay_len=np.where(has, l4_len - UDP_HDR, 0)[order].astype(np.uint32),
                src=np.where(has, src, 0)[order].astype(np.uint32),
                sport=np.where(has, sport, 0)[order].astype(np.uint16))
