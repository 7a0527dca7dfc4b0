"""The reference stack for one frame at a time: what the reference does with a
wire frame from the NIC to the shard, and with an L4 datagram from the L4
writer to the NIC, restated as one loop per frame over Python ints and bytes
(paths relative to the reference tree):

  tx   L4 checksum over pseudo-header + datagram            src/net/udp.cc:184-195,
       (stored at UDP +6 / TCP +16)                          include/seastar/net/tcp.hh:1656-1694
       ipv4::send: needs_frag, pieces of mtu - 20, MF,       src/net/ip.cc:100-111, 244-299
       offset / 8, the header checksum per frame
       get_l2_dst_address, the packet provider's eth_hdr     ip.cc:231-242, src/net/net.cc:266-284
  rx   dispatch_packet                                       net.cc:324-357
       ipv4::forward (the dispatch hash)                     ip.cc:77-94
       ipv4::handle_received_packet up to delivery           ip.cc:114-229
       frag::merge / is_complete                             ip.cc:412-437
       the pseudo-header seed of the L4 verify               include/seastar/net/ip.hh:70-75
       forward_dst / hash2cpu                                include/seastar/net/net.hh:287-305

It is not composed from the per-call restatements (test_eth_host.ref_*,
fast_models, the steer restatement): it shares none of their conventions for
buckets, indices or order, so two layers that agree with their own models and
disagree with each other show up against it.  It reuses reasm_model.Merger
(pinned to the reference's own packet_merger) and oracle.toeplitz.
tests/test_stack_model.py pins it with frames written out byte by byte.

Where the batch interface reports something the reference has no word for (a
status byte, a class for a dropped frame, which keys go to the host), the
model states the interface's definition (include/sccsum.h) from what the
reference did with the frame.  Nothing here reads the code under test."""
from __future__ import annotations

import itertools
import struct

import numpy as np

import oracle
from reasm_model import Merger, plen

IPV4, ARP = 0x0800, 0x0806
TCP, UDP, ICMP = 6, 17, 1
ST_OK, ST_L4_OK, ST_MALFORMED, ST_RANGE, ST_IPFRAG, ST_NOARP = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
CLS_UNKNOWN, CLS_SHORT, CLS_RANGE = 0xFF, 0xFE, 0xFD   # classes of dropped frames (sccsum.h, "Link layer")
L4_MAX = 65515                                           # ip_packet_len_max - 20
RSS_KEY = oracle.RSS_KEY_40


# ---------------------------------------------------------------- checksums

def ones_sum(data: bytes, seed: int = 0) -> int:
    """RFC 1071: the folded 16-bit one's complement sum of big-endian words, an odd last byte padded with 0."""
    if len(data) & 1:
        data = bytes(data) + b"\0"
    s = seed + sum(struct.unpack(f">{len(data) // 2}H", data))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def csum(data: bytes, seed: int = 0) -> int:
    """checksummer::get(): the complement of the sum; its two bytes go on the wire big-endian."""
    return ~ones_sum(data, seed) & 0xFFFF


def pseudo(src: int, dst: int, proto: int, length: int) -> int:
    """ip.hh:70-75: src, dst, 0, proto, uint16_t(len), folded; 0 for protocols without a pseudo-header."""
    if proto not in (TCP, UDP):
        return 0
    return ones_sum(struct.pack(">IIBBH", src, dst, 0, proto, length & 0xFFFF))


def be16(b: bytes, at: int) -> int:
    return (b[at] << 8) | b[at + 1]


def be32(b: bytes, at: int) -> int:
    return int.from_bytes(b[at:at + 4], "big")


def l4_field(proto: int, length: int):
    """Where the L4 writer stores its checksum, when the datagram holds the header."""
    if proto == UDP and length >= 8:
        return 6
    if proto == TCP and length >= 20:
        return 16
    return None


# ---------------------------------------------------------------- tx

def ip_header(total_len: int, ident: int, frag: int, proto: int, src: int, dst: int, ihl: int = 5,
              options: bytes = b"") -> bytes:
    """ip.cc:248-278: the header with its checksum over sizeof(ip_hdr) = 20 bytes (options are not summed)."""
    h = struct.pack(">BBHHHBBHII", 0x40 | ihl, 0, total_len, ident, frag, 64, proto, 0, src, dst)
    h = h[:10] + csum(h).to_bytes(2, "big") + h[12:]
    return h + options


def eth_header(dst_mac: int, src_mac: int, proto: int) -> bytes:
    return dst_mac.to_bytes(6, "big") + src_mac.to_bytes(6, "big") + proto.to_bytes(2, "big")


def tx(datagrams, cfg: dict) -> dict:
    """datagrams: (bytes or None, proto, dst, id) each, the L4 field zero; None: the
    datagram is not in the buffer.  cfg: host, netmask, gw, hw, mtu, arp {ip: mac}.
    Returns frames (wire bytes, in order), owner (the datagram of each frame),
    l4 (the datagrams as sent, checksum stored), send_status (what ipv4::send's
    batch form reports: OK, RANGE, MALFORMED), status (OK / NOARP / 0: no
    frame) and unresolved [(datagram, next hop)]."""
    host, mask, gw, mtu, arp = cfg["host"], cfg["netmask"], cfg["gw"], cfg["mtu"], cfg["arp"]
    out = dict(frames=[], owner=[], l4=[], send_status=[], status=[], unresolved=[])
    for i, (data, proto, dst, ident) in enumerate(datagrams):
        if data is None or len(data) > L4_MAX:   # the reference's uint16_t arithmetic would wrap: refused
            out["l4"].append(data)
            out["send_status"].append(ST_RANGE if data is None else ST_MALFORMED)
            out["status"].append(0)
            continue
        p = bytearray(data)
        at = l4_field(proto, len(p))
        if at is not None:
            p[at:at + 2] = csum(bytes(p), pseudo(host, dst, proto, len(p))).to_bytes(2, "big")
        p = bytes(p)
        out["l4"].append(p)
        out["send_status"].append(ST_OK)
        pieces = []
        if len(p) + 20 <= mtu:                    # needs_frag (no TSO / UFO)
            pieces.append((0, p, 0))
        else:
            offset, remaining = 0, len(p)
            while remaining:
                can_send = min(mtu - 20, remaining)
                remaining -= can_send
                pieces.append((((1 if remaining else 0) << 13) | (offset // 8), p[offset:offset + can_send], offset))
                offset = (offset + can_send) & 0xFFFF
        hop = dst if not ((dst ^ host) & mask) else gw     # get_l2_dst_address
        mac = arp.get(hop)
        if mac is None:
            out["status"].append(ST_NOARP)
            out["unresolved"].append((i, hop))
            continue
        out["status"].append(ST_OK)
        for frag, piece, _ in pieces:
            out["frames"].append(eth_header(mac, cfg["hw"], IPV4)
                                 + ip_header(20 + len(piece), ident, frag, proto, host, dst) + piece)
            out["owner"].append(i)
    return out


# ---------------------------------------------------------------- rx

class _Frag:
    def __init__(self):
        self.data = Merger()
        self.last_frag_received = False
        self.header = None      # the frame whose IP header frag::merge keeps
        self.recs = []          # (frame, offset, len, mf) in arrival order


def plain(recs) -> bool:
    """sccsum.h, "Rx reassembly": over the records in offset order every len >
    0, neighbours do not overlap, at most one MF-clear record and it is last."""
    s = sorted(recs, key=lambda r: r[1])
    return (all(r[2] > 0 for r in s) and all(a[1] + a[2] <= b[1] for a, b in zip(s, s[1:]))
            and all(r[3] for r in s[:-1]))


class Rx:
    """cfg: host, netmask, key (RSS), reta (the 128-entry software
    redirection table), table_bits, arp {ip: mac} (copied), protos.  State kept
    between batches: the fragment map and the ARP dict."""

    def __init__(self, cfg: dict):
        self.host, self.mask = cfg["host"], cfg["netmask"]
        self.key = cfg.get("key", RSS_KEY)
        self.reta, self.table_bits = [int(x) for x in cfg["reta"]], cfg.get("table_bits", 0)
        self.protos = tuple(cfg.get("protos", (IPV4, ARP)))
        self.arp = dict(cfg.get("arp", {}))
        self.frags = {}
        self.host_owned = set()  # keys handed to the host whole and not complete: the host's own _frags from then on
        self.payload = []       # the fragments' payloads the mergers' pieces point into
        self.nbatch = 0

    def shard(self, h: int) -> int:
        """hash2cpu with one hardware queue: forward_dst(0, hash)."""
        return self.reta[(h >> self.table_bits) % len(self.reta)]

    def batch(self, frames) -> dict:
        """frames: wire frames as bytes, None for one outside the buffer."""
        b = self.nbatch
        self.nbatch += 1
        known = dict(self.arp)   # the table the device call is given: the one at the batch's start
        out = dict(cls=[], buckets=[[] for _ in range(len(self.protos) + 1)], src_mac=[[] for _ in self.protos],
                   ip=[], learn=[], delivered=[], host={}, late_host=[], frags=[])
        touched = set()
        for idx, f in enumerate(frames):
            # dispatch_packet: get_header<eth_hdr>, the protocol map, from = src_mac, trim_front(14)
            if f is None or len(f) < 14:
                out["cls"].append(CLS_RANGE if f is None else CLS_SHORT)
                out["buckets"][-1].append(idx)
                continue
            proto = be16(f, 12)
            if proto not in self.protos:
                out["cls"].append(CLS_UNKNOWN)
                out["buckets"][-1].append(idx)
                continue
            k = self.protos.index(proto)
            out["cls"].append(k)
            out["buckets"][k].append(idx)
            frm = int.from_bytes(f[6:12], "big")
            out["src_mac"][k].append(frm)
            if proto == IPV4:
                out["ip"].append(self._ipv4(bytes(f[14:]), frm, (b, idx), known, out, touched))
        # the keys the device hands to the host whole, with their records of this batch and the carry
        for key in touched:
            fr = self.frags.get(key)
            if fr is not None and not plain(fr.recs):
                out["host"][key] = list(fr.recs)
                self.host_owned.add(key)
                del self.frags[key]
        out["pending"] = {key for key, fr in self.frags.items() if plain(fr.recs)}
        return out

    def _ipv4(self, p: bytes, frm: int, where, known, out, touched) -> dict:
        info = dict(frame=where, status=ST_MALFORMED, hash=0, shard=self.shard(0), ihl=0, to_host=False, frag=False,
                    delivered=False)
        if len(p) < 20:          # get_header<ip_hdr> is null: dropped; nothing to hash
            return info
        ihl, ip_len, ident, fragw, proto = p[0] & 0xF, be16(p, 2), be16(p, 4), be16(p, 6), p[9]
        src, dst = be32(p, 12), be32(p, 16)
        mf, offset = bool(fragw & 0x2000), ((fragw & 0x1FFF) << 3) & 0xFFFF
        is_frag = mf or offset != 0
        need = 20 if proto == TCP else 8 if proto == UDP else 0
        # ipv4::forward: src, dst as stored, then for an atomic datagram the ports at IP offset 20
        data = p[12:20]
        if need and not is_frag and len(p) >= 20 + need:
            data += p[20:24]
        info["hash"] = oracle.toeplitz(self.key, data)
        info["shard"] = self.shard(info["hash"])
        info["ihl"], info["frag"] = ihl, is_frag
        # the status byte of the frames call: every bit, whichever check drops the frame first
        ok = csum(p[:20]) == 0
        l4_end = min(ip_len, len(p))
        malformed = len(p) < ip_len or offset + l4_end > 65535 or 4 * ihl > l4_end
        st = (ST_OK if ok else 0) | (ST_MALFORMED if malformed else 0) | (ST_IPFRAG if is_frag else 0)
        l4 = p[4 * ihl:l4_end] if 4 * ihl <= l4_end else b""
        if not is_frag and csum(l4, pseudo(src, dst, proto, len(l4))) == 0:
            st |= ST_L4_OK
        info["status"] = st
        # handle_received_packet
        if not ok or malformed:
            return info
        p = p[:ip_len]                                      # trim_back
        if not ((src ^ self.host) & self.mask) and src != self.host:
            if known.get(src) != frm:                       # a pair the batch's table does not hold
                out["learn"].append((src, where[1], frm))
            self.arp[src] = frm                             # _arp.learn(from, h.src_ip)
        if dst != self.host:
            return info
        info["to_host"] = True
        if not is_frag:
            info["delivered"] = True                        # l4->received(p behind its header)
            return info
        key = (src, dst, ident, proto)
        if key in self.host_owned:                          # the host routes it to its own merger
            out["late_host"].append(where)
            return info
        touched.add(key)
        fr = self.frags.setdefault(key, _Frag())
        if not mf:
            fr.last_frag_received = True
        if offset == 0:
            fr.header = where
        body = p[4 * ihl:]
        ref = len(self.payload)
        self.payload.append((where, body))
        fr.recs.append((where, offset, len(body), int(mf)))
        out["frags"].append((where, key, offset, len(body), int(mf), 4 * ihl))   # what merge() was given
        fr.data.merge(offset, [(ref, 0, len(body))])
        whole = fr.data.whole()
        if fr.last_frag_received and whole is not None:     # is_complete
            dgram = b"".join(self.payload[r][1][a:a + n] for r, a, n in whole)
            assert len(dgram) == plen(whole)
            hd = p[12:20]                                   # ip.cc:186-197: src, dst, then l4->forward at 0
            if need and len(dgram) >= need:
                hd += dgram[:4]
            h = oracle.toeplitz(self.key, hd)
            seed = pseudo(src, dst, proto, len(dgram))
            c = csum(dgram, seed)
            is_plain = plain(fr.recs)
            out["delivered"].append(dict(src=src, dst=dst, id=ident, proto=proto, data=dgram, seed=seed, l4=c,
                                         l4_ok=c == 0, hash=h, shard=self.shard(h), last=where, head=fr.header,
                                         plain=is_plain, nrecs=len(fr.recs)))
            if not is_plain:
                out["host"][key] = list(fr.recs)
                touched.discard(key)
            del self.frags[key]
        return info


def partition(dest, nbuckets: int):
    """The per-shard lists forward() fills: (order, first) — the indices grouped
    by destination in arrival order, and the nbuckets + 1 bounds."""
    order = [i for d in range(nbuckets) for i, x in enumerate(dest) if x == d]
    first = [0]
    for d in range(nbuckets):
        first.append(first[-1] + sum(1 for x in dest if x == d))
    return order, first


# ---------------------------------------------------------------- seeded traffic

HOST, NETMASK, GW = 0x0A000001, 0xFFFF0000, 0x0A0000FE
HW, GW_MAC = 0x02AB12CD34EF, 0x02000000FFFE
OTHER_HOST = 0x0A000002
TILE = 1024   # sccsum_eth_tile_packets(); tests/test_gpu_stack.py asserts it
# three successive wire batches a case; among the counts 0, 1, one tile - 1, one tile, one tile + 1, 2 tiles + 7
BATCH_SIZES = [(TILE - 1, TILE, TILE + 1), (0, 2 * TILE + 7, 1), (1, TILE, 0), (2 * TILE + 7, 1, TILE - 1),
               (TILE + 1, 0, TILE), (TILE, TILE - 1, 1), (700, 900, 600), (1, 2 * TILE + 7, 0),
               (TILE - 1, 1, TILE + 1), (300, TILE, 500), (TILE + 1, TILE + 1, 0), (0, TILE - 1, TILE)]
SEEDS = list(range(len(BATCH_SIZES)))


def peer_mac(ip: int) -> int:
    return (0x020000000000 + ip * 0x10003) & 0xFFFFFFFFFFFF


def rx_cfg(ncpu: int = 8) -> dict:
    """The receiving host: three of the six on-link peers known (one under another MAC)."""
    arp = {0x0A000110: peer_mac(0x0A000110), 0x0A000111: peer_mac(0x0A000111),
           0x0A000112: peer_mac(0x0A000112) ^ 0x100, GW: GW_MAC}
    reta = [(7 * k + k // 16) % ncpu for k in range(128)]
    return dict(host=HOST, netmask=NETMASK, gw=GW, hw=HW, key=RSS_KEY, reta=reta, table_bits=0, arp=arp, ncpu=ncpu)


ON_LINK = [0x0A000110, 0x0A000111, 0x0A000112, 0x0A000113, 0x0A000114, 0x0A00F115]
OFF_LINK = [0xC0A80105, 0x08080808]


def _l4(rng, proto: int, length: int) -> bytes:
    d = bytearray(rng.integers(0, 256, length, dtype=np.uint8).tobytes())
    at = l4_field(proto, length)
    if at is not None:
        d[at:at + 2] = b"\0\0"
    return bytes(d)


def _peer_frames(rng, peer: int, mtu: int, lens, dst: int = HOST, proto=None, ident=None, ids=None) -> list:
    """The wire frames `peer` sends for datagrams of the given lengths: one list per datagram."""
    on_link = not ((peer ^ HOST) & NETMASK)
    cfg = dict(host=peer, netmask=NETMASK, gw=GW, hw=peer_mac(peer) if on_link else GW_MAC, mtu=mtu,
               arp={HOST: HW, OTHER_HOST: 0x02000000B0B0, GW: HW})   # off the link: the last hop's frame
    out = []
    for ln in lens:
        pr = int(rng.choice([UDP, UDP, TCP, ICMP])) if proto is None else proto
        dg = [(_l4(rng, pr, int(ln)), pr, dst, (next(ids) & 0xFFFF if ident is None else ident))]
        t = tx(dg, cfg)
        assert t["status"] == [ST_OK]
        out.append(t["frames"])
    return out


def _hand_frame(src, dst, ident, proto, mf, off8, payload: bytes, ihl: int = 5, pad: bytes = b"") -> bytes:
    options = bytes([1] * (4 * (ihl - 5)))   # NOPs
    ip = ip_header(4 * ihl + len(payload), ident, (int(mf) << 13) | off8, proto, src, dst, ihl, options)
    on_link = not ((src ^ HOST) & NETMASK)
    return eth_header(HW, peer_mac(src) if on_link else GW_MAC, IPV4) + ip + payload + pad


def _udp_with_sum(rng, src: int, dst: int, length: int) -> bytes:
    d = bytearray(_l4(rng, UDP, length))
    d[6:8] = csum(bytes(d), pseudo(src, dst, UDP, length)).to_bytes(2, "big")
    return bytes(d)


def _flip(f: bytes, at: int) -> bytes:
    return f[:at] + bytes([f[at] ^ 0x5A]) + f[at + 1:]


def rx_traffic(seed: int) -> list:
    """Three successive wire batches (lists of bytes / None) of BATCH_SIZES[seed]
    frames: datagrams of several peers at MTU 68, 576 and 1500 cut by tx(),
    their fragments interleaved and partly reordered, and every item of the mix
    tests/test_stack_model.py asserts, spliced in."""
    rng = np.random.default_rng(1000 + seed)
    sizes = BATCH_SIZES[seed]
    ids = itertools.count(1000)   # distinct identifications: no two datagrams share a key

    def sent(peer, mtu, lens, **kw):
        return _peer_frames(rng, peer, mtu, lens, ids=ids, **kw)
    total = sum(sizes)
    seqs = []      # each a list of frames kept in this order
    mtus = {ON_LINK[0]: 68, ON_LINK[1]: 576, ON_LINK[2]: 1500, ON_LINK[3]: 68, ON_LINK[4]: 576, ON_LINK[5]: 1500,
            OFF_LINK[0]: 1500, OFF_LINK[1]: 576}

    def shuffled(frames):
        frames = list(frames)
        if rng.random() < 0.6:
            frames = [frames[int(k)] for k in rng.permutation(len(frames))]
        return frames

    # the datagram whose first fragment opens the case and whose last closes it
    straddler = sent(ON_LINK[2], 1500, [3500], proto=UDP)[0]
    assert len(straddler) == 3
    seqs.append(straddler[1:-1])
    # --- the mix (each at least once in every seed)
    a, c = ON_LINK[3], OFF_LINK[0]
    single = []    # single frames
    single.append(eth_header(0xFFFFFFFFFFFF, peer_mac(a), ARP) + bytes([0, 1, 8, 0, 6, 4, 0, 1]) + bytes(20))
    single.append(eth_header(HW, peer_mac(ON_LINK[0]), ARP) + bytes([0, 1, 8, 0, 6, 4, 0, 2]) + bytes(20))
    single.append(eth_header(HW, peer_mac(a), 0x86DD) + bytes(range(40)))
    single.append(eth_header(HW, peer_mac(a), 0x8100) + bytes(30))
    single += [bytes(rng.integers(0, 256, k, dtype=np.uint8)) for k in (0, 1, 7, 13)]
    single += [None, None]
    single.append(_flip(sent(a, 1500, [300], proto=UDP)[0][0], 14 + 10))        # a corrupted IP header checksum
    single.append(sent(a, 1500, [200], proto=TCP)[0][0][:-9])                   # shorter than its IP total length
    single.append(sent(c, 1500, [64], proto=UDP)[0][0] + bytes(6))              # longer: trimmed
    single.append(_hand_frame(a, HOST, 77, UDP, 0, 0, _udp_with_sum(rng, a, HOST, 120), ihl=7))   # IP options
    single.append(_hand_frame(c, HOST, 78, TCP, 0, 0, _l4(rng, TCP, 40), ihl=15))
    single += [fr[0] for fr in sent(a, 1500, [90, 700], dst=OTHER_HOST)]        # for another host
    single.append(_flip(sent(ON_LINK[4], 1500, [400], proto=UDP)[0][0], 14 + 20 + 100))   # L4 corrupted
    single.append(_flip(sent(ON_LINK[2], 1500, [400], proto=TCP)[0][0], 14 + 20 + 17))
    seqs += [[f] for f in single]
    seqs.append(shuffled(sent(a, 68, [300], dst=OTHER_HOST)[0]))                # fragments for another host
    bad = sent(ON_LINK[2], 1500, [4000], proto=UDP)[0]
    bad[1] = _flip(bad[1], 14 + 20 + 50)                                         # L4 corrupted in a fragment
    seqs.append(shuffled(bad))
    bad = sent(c, 1500, [3800], proto=TCP)[0]
    bad[1] = _flip(bad[1], 14 + 8)                                               # a fragment's header corrupted: dropped
    seqs.append(bad)
    missing = sent(ON_LINK[3], 68, [400])[0]
    del missing[int(rng.integers(0, len(missing)))]                              # a fragment never arrives
    seqs.append(shuffled(missing))
    body = _udp_with_sum(rng, c, HOST, 200)                                      # options on fragments, padding
    seqs.append(shuffled([_hand_frame(c, HOST, 79, UDP, 1, 0, body[:96], ihl=6),
                          _hand_frame(c, HOST, 79, UDP, 1, 12, body[96:160], ihl=8, pad=bytes(4)),
                          _hand_frame(c, HOST, 79, UDP, 0, 20, body[160:], ihl=5)]))
    # The keys the device hands to the host whole.  The host keeps such a key from then on (INTEGRATION.md,
    # "Host bucket"), so each lies inside one batch.  Two are written by hand, their frames next to each other;
    # the rest are what ipv4::send itself makes at MTU 576: 556 is no multiple of 8, the offsets are
    # truncated (ip.cc:259) and every piece overlaps the one before it by 4 bytes.
    body = _udp_with_sum(rng, a, HOST, 160)
    overlap = [_hand_frame(a, HOST, 80, UDP, 1, 0, body[:64]), _hand_frame(a, HOST, 80, UDP, 1, 6, body[48:112]),
               _hand_frame(a, HOST, 80, UDP, 0, 14, body[112:])]
    dup = sent(ON_LINK[0], 68, [150], proto=UDP, ident=81)[0]
    dup = [dup[0], dup[1], dup[1]] + dup[2:]
    blocks = [overlap, dup]
    pinned = []    # sequences that stay inside one batch, interleaved with the rest of it
    # --- the bulk: datagrams of 1..4 000 bytes, a few of 65 515
    reserve = sum(len(b) for b in blocks) + 2
    have = sum(len(s) for s in seqs)
    big = 2 if total > 1500 else 1 if total > 1100 else 0
    for _ in range(big):
        fr = sent(ON_LINK[2] if rng.random() < 0.5 else OFF_LINK[0], 1500, [L4_MAX])[0]
        seqs.append(shuffled(fr))
        have += len(fr)
    peers = list(mtus)
    while True:
        peer = peers[int(rng.integers(0, len(peers)))]
        mtu = mtus[peer]
        hi = {68: 500, 576: 3000, 1500: 4000}[mtu]
        ln = int(rng.integers(1, hi + 1)) if rng.random() < 0.97 else 4000
        fr = sent(peer, mtu, [ln])[0]
        if have + len(fr) + reserve > total:
            break
        (pinned if mtu == 576 and len(fr) > 1 else seqs).append(shuffled(fr))
        have += len(fr)
    while have + reserve < total:                                                # single frames fill the rest
        peer = peers[int(rng.integers(0, len(peers)))]
        seqs.append(sent(peer, 1500, [int(rng.integers(1, 1400))])[0])
        have += 1
    # the places: the straddler's ends, the blocks and the pinned sequences first
    cuts = [int(x) for x in np.cumsum((0,) + sizes)]
    slots = [False] * total
    stream = [None] * total
    stream[0], stream[-1] = straddler[0], straddler[-1]
    slots[0] = slots[-1] = True
    j = int(np.argmax(sizes))
    pos = cuts[j] + 10
    for blk in blocks:
        stream[pos:pos + len(blk)] = blk
        slots[pos:pos + len(blk)] = [True] * len(blk)
        pos += len(blk) + 5
    assert pos < cuts[j + 1] - 1
    roomy = [k for k in range(3) if sizes[k] >= 600]
    for fr in pinned:
        k = roomy[int(rng.integers(0, len(roomy)))]
        free = [x for x in range(cuts[k], cuts[k + 1]) if not slots[x]]
        for x, f in zip(sorted(rng.choice(free, size=len(fr), replace=False).tolist()), fr):
            stream[x], slots[x] = f, True
    # the rest: a random merge that keeps each sequence's own order, into the places left
    tags = np.repeat(np.arange(len(seqs)), [len(s) for s in seqs])
    rng.shuffle(tags)
    at = [0] * len(seqs)
    free = [x for x in range(total) if not slots[x]]
    assert len(free) == tags.size
    for x, t in zip(free, tags.tolist()):
        stream[x] = seqs[t][at[t]]
        slots[x] = True
        at[t] += 1
    assert all(slots)
    return [stream[cuts[k]:cuts[k + 1]] for k in range(3)]


def tx_cfg(mtu: int) -> dict:
    """The sending host: some on-link peers and the gateway resolved."""
    arp = {ip: peer_mac(ip) for ip in ON_LINK[:4]}
    arp[GW] = GW_MAC
    return dict(host=HOST, netmask=NETMASK, gw=GW, hw=HW, mtu=mtu, arp=arp)


TX_OTHER_GW = 0x0A0000FD   # a gateway the table does not know


def tx_traffic(seed: int, n: int = 260) -> list:
    """(bytes or None, proto, dst, id) L4 datagrams: destinations known on the
    link, unknown on the link, behind the gateway; lengths 1..4 000, two of
    65 515 and one above; every 23rd outside the buffer (None)."""
    rng = np.random.default_rng(2000 + seed)
    dsts = ON_LINK + [0xC0A80105, 0x08080808, 0xFFFFFFFF, 0]
    base = int(rng.integers(0, 65536))
    out = []
    for i in range(n):
        ln = int(rng.integers(1, 4001))
        if i in (40, 170):
            ln = L4_MAX
        if i == 90:
            ln = L4_MAX + 1
        if i in (3, 4, 5):
            ln = (7, 8, 19)[i - 3]     # around the UDP / TCP header lengths
        proto = (UDP, TCP, ICMP, UDP)[i % 4] if i > 5 else (UDP, TCP, UDP, UDP, UDP, TCP)[i]
        dst = dsts[int(rng.integers(0, len(dsts)))]
        data = None if i % 23 == 11 else _l4(rng, proto, ln)
        out.append((data, proto, dst, (base + 7 * i) & 0xFFFF))   # distinct: no two datagrams share a key
    return out
