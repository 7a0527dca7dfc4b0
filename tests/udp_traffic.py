"""Seeded UDP traffic for tests/test_gpu_udp.py, and what the per-datagram
models (stack_model.Rx, udp_model) make of it.  tests/test_udp_host.py checks
that every seed holds every class, an empty channel and a channel with more
datagrams than its room.

One wire batch a seed, its frames in random order: datagrams of on- and
off-link peers to the 252 ports of PORTS, cut by stack_model.tx at MTU 68, 576
and 1500 (at 576 the reference's truncated offsets make the pieces overlap, so
those keys are the host's and reassembly delivers none of them), with
 - more than 1 024 atomic datagrams to PORTS[0], none to PORTS[251];
 - datagrams to unbound ports, atomic and in fragments;
 - UDP packets whose L4 is 0..7 bytes, frames padded past their IP length,
   udp_hdr::len fields that disagree with the packet, ihl 5..15;
 - TCP and ICMP, packets for another host, a corrupted IP header."""
from __future__ import annotations

import itertools

import numpy as np

import stack_model as sm
import udp_model

PORTS = [1024 + 61 * k for k in range(252)]      # channel k is PORTS[k]; any prefix is a table
UNBOUND = [7, 1023, 1024 + 61 * 252, 65535, 1025]
SEEDS = [0, 1, 2, 3]
HOT = 1100                                       # atomic datagrams to PORTS[0]: more than a queue holds
PEERS = sm.ON_LINK[:5] + sm.OFF_LINK


def room_for(k: int) -> int:
    """The free slots of channel k's queue in the tests: a whole queue for the hot channel, little for the rest."""
    return udp_model.QUEUE_SIZE if k == 0 else 2 + k % 3


def _payload(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _frames(rng, ids, peer: int, mtu: int, sport: int, dport: int, payload: bytes, bad_len=None, dst: int = sm.HOST):
    """The wire frames `peer` sends for one datagram (stack_model.tx does the cut and the checksums)."""
    zero = udp_model.send(payload, sport, dport, peer, dst, mtu)["zero"]
    if bad_len is not None:
        zero = zero[:4] + int(bad_len).to_bytes(2, "big") + zero[6:]
    on_link = not ((peer ^ sm.HOST) & sm.NETMASK)
    cfg = dict(host=peer, netmask=sm.NETMASK, gw=sm.GW, hw=sm.peer_mac(peer) if on_link else sm.GW_MAC, mtu=mtu,
               arp={sm.HOST: sm.HW, sm.OTHER_HOST: 0x02000000B0B0, sm.GW: sm.HW})
    t = sm.tx([(zero, sm.UDP, dst, next(ids) & 0xFFFF)], cfg)
    assert t["status"] == [sm.ST_OK]
    return t["frames"]


def wire(seed: int) -> list:
    """The seed's wire frames (bytes each)."""
    rng = np.random.default_rng(7000 + seed)
    ids = itertools.count(100 + 1000 * seed)
    out = []

    def peer():
        return PEERS[int(rng.integers(0, len(PEERS)))]

    def sport():
        return int(rng.integers(0, 65536))

    for _ in range(HOT):
        out += _frames(rng, ids, peer(), 1500, sport(), PORTS[0], _payload(rng, int(rng.integers(0, 41))))
    for _ in range(500):                                       # the other channels, atomic
        k = int(rng.integers(1, 251))
        out += _frames(rng, ids, peer(), 1500, sport(), PORTS[k], _payload(rng, int(rng.integers(0, 300))))
    for _ in range(40):                                        # in fragments of 48 bytes: reassembled
        k = int(rng.integers(0, 251))
        out += _frames(rng, ids, peer(), 68, sport(), PORTS[k], _payload(rng, int(rng.integers(41, 400))))
    for _ in range(6):                                         # overlapping pieces: the host's keys
        out += _frames(rng, ids, peer(), 576, sport(), PORTS[int(rng.integers(0, 251))],
                       _payload(rng, int(rng.integers(600, 1500))))
    for k in range(30):                                        # unbound ports
        mtu = 68 if k % 3 == 0 else 1500
        out += _frames(rng, ids, peer(), mtu, sport(), UNBOUND[k % len(UNBOUND)], _payload(rng, 10 + 7 * k))
    a = sm.ON_LINK[3]
    for n in range(8):                                         # an L4 of 0..7 bytes
        out.append(sm._hand_frame(a, sm.HOST, next(ids) & 0xFFFF, sm.UDP, 0, 0, _payload(rng, n)))
    for ihl in range(5, 16):                                   # IP options, padding behind the IP length
        zero = udp_model.send(_payload(rng, 3 * ihl), sport(), PORTS[ihl], a, sm.HOST, 1500)["zero"]
        out.append(sm._hand_frame(a, sm.HOST, next(ids) & 0xFFFF, sm.UDP, 0, 0, zero, ihl=ihl,
                                  pad=_payload(rng, ihl - 5)))
    for pad in (1, 6, 18):
        zero = udp_model.send(_payload(rng, 20), sport(), PORTS[2], a, sm.HOST, 1500)["zero"]
        out.append(sm._hand_frame(a, sm.HOST, next(ids) & 0xFFFF, sm.UDP, 0, 0, zero, pad=_payload(rng, pad)))
    for bad in (0, 8, 9, 27, 29, 65535):                       # udp_hdr::len disagrees (the packet has 8 + 20 bytes)
        out += _frames(rng, ids, peer(), 1500, sport(), PORTS[3], _payload(rng, 20), bad_len=bad)
    out += _frames(rng, ids, peer(), 68, sport(), PORTS[4], _payload(rng, 100), bad_len=50)
    for proto in (sm.TCP, sm.ICMP):
        for fr in sm._peer_frames(rng, peer(), 1500, [40, 90, 200], proto=proto, ids=ids):
            out += fr
    out += _frames(rng, ids, a, 1500, sport(), PORTS[0], _payload(rng, 30), dst=sm.OTHER_HOST)
    out += _frames(rng, ids, a, 68, sport(), PORTS[0], _payload(rng, 90), dst=sm.OTHER_HOST)
    out.append(sm._flip(_frames(rng, ids, a, 1500, sport(), PORTS[0], _payload(rng, 30))[0], 14 + 10))
    while len(out) < 2 * 1024 + 7 + 64:
        out += _frames(rng, ids, peer(), 1500, sport(), PORTS[int(rng.integers(0, 251))], _payload(rng, 12))
    return [out[int(k)] for k in rng.permutation(len(out))]


_CACHE = {}


def case(seed: int) -> dict:
    """frames: the wire batch; ip: the IPv4 bucket's packets (bytes behind the
    Ethernet header) with stack_model's info for each; delivered: the
    reassembled datagrams of plain keys, in delivery order.  Computed once."""
    if seed not in _CACHE:
        frames = wire(seed)
        rx = sm.Rx(sm.rx_cfg())
        out = rx.batch(frames)
        ip = [bytes(frames[i][14:]) for i in out["buckets"][0]]
        assert len(ip) == len(out["ip"])
        _CACHE[seed] = dict(frames=frames, ip=ip, info=out["ip"], delivered=[d for d in out["delivered"] if d["plain"]],
                            not_plain=sum(1 for d in out["delivered"] if not d["plain"]) + len(out["host"]))
    return _CACHE[seed]


def expect_rx(items: list, nchannels: int, index=None) -> dict:
    """items: udp_model.atomic / reassembled results in the call's order (item
    j belongs to batch index index[j]).  The arrays sccsum_udp_rx writes."""
    n = len(items)
    idx = list(range(n)) if index is None else [int(x) for x in index]
    cls = [it["cls"] for it in items]
    bucket = [c if c < nchannels else nchannels for c in cls]
    order, first = sm.partition(bucket, nchannels + 1)
    return dict(cls=np.array(cls, dtype=np.uint8), first=np.array(first, dtype=np.uint32),
                order=np.array([idx[j] for j in order], dtype=np.uint32), pos=order,
                pay_len=np.array([len(items[j]["payload"]) if cls[j] < nchannels else 0 for j in order], dtype=np.uint32),
                src=np.array([items[j]["src"] if cls[j] < nchannels else 0 for j in order], dtype=np.uint32),
                sport=np.array([items[j]["sport"] if cls[j] < nchannels else 0 for j in order], dtype=np.uint16))
