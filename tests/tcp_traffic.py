"""Seeded TCP traffic for tests/test_gpu_tcp.py, and what the per-segment
models (stack_model.Rx, tcp_model) make of it.  tests/test_tcp_host.py checks
that the mixed batch holds every class and every reset form.

Connection c of every table is conn_tuple(c), so any prefix of the same
formula is a table and one wire batch serves every table size: a segment to
connection c is CONN where c < nconns, and otherwise LISTEN (local port 80 or
8080 listens) or RESET / NOCONN (443 does not)."""
from __future__ import annotations

import numpy as np

import stack_model as sm
import tcp_model as tm

LOCAL_PORTS = (80, 443, 8080)
LISTEN = (80, 8080, 22)
CLOSED = (443, 7, 65535)
FULL = 2 * 1024 + 7
# connections the mixed batch aims at: both sides of every sort-pass boundary of the key
HOT = (0, 1, 2, 5, 17, 252, 253, 254, 255, 256, 300, 4095, 65532, 65533, 65534, 65535, 65536)


def conn_tuple(c: int) -> tuple:
    """(local_ip, foreign_ip, local_port, foreign_port) of connection c: distinct for distinct c."""
    return (sm.HOST, 0x0B000000 + c // 3, LOCAL_PORTS[c % 3], 1024 + (c * 40503) % 60000)


def conn_array(nconns: int) -> np.ndarray:
    c = np.arange(nconns, dtype=np.int64)
    return np.stack([np.full(nconns, sm.HOST, dtype=np.int64), 0x0B000000 + c // 3,
                     np.array(LOCAL_PORTS, dtype=np.int64)[c % 3], 1024 + (c * 40503) % 60000], axis=1)


def tcbs(nconns: int) -> dict:
    return {tuple(r): c for c, r in enumerate(conn_array(nconns).tolist())}


def fix_sum(l4: bytes, src: int, dst: int, at: int) -> bytes:
    """l4 with the two bytes at the even offset `at` chosen so that the checksum verifies."""
    z = l4[:at] + b"\0\0" + l4[at + 2:]
    return z[:at] + sm.csum(z, tm.pseudo_sum(src, dst, len(z))).to_bytes(2, "big") + z[at + 2:]


def segment(src, dst, sport, dport, seq=0, ack=0, flags=tm.ACK, window=1000, payload=b"", options=b"",
            data_offset=None) -> bytes:
    """A segment src -> dst with its checksum stored."""
    do = (20 + len(options)) // 4 if data_offset is None else data_offset
    return fix_sum(tm.hdr_write(sport, dport, seq, ack, do, flags, window) + options + payload, src, dst, 16)


def to_conn(c: int, **kw) -> tuple:
    """(src, dst, l4) of a segment the peer of connection c sends."""
    lip, fip, lp, fp = conn_tuple(c)
    return fip, lip, segment(fip, lip, fp, lp, **kw)


def frame(src: int, dst: int, l4: bytes, ident: int = 1, ihl: int = 5, pad: bytes = b"", proto: int = sm.TCP,
          mf: int = 0) -> bytes:
    return sm._hand_frame(src, dst, ident & 0xFFFF, proto, mf, 0, l4, ihl=ihl, pad=pad)


def _bytes(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def mixed(seed: int = 0, n: int = FULL + 64) -> list:
    """The mixed wire batch: every class, every reset form, the header shapes."""
    rng = np.random.default_rng(9100 + seed)
    out = []
    seqs = {}

    def conn_frame(c, **kw):
        seqs[c] = seqs.get(c, 1000 * c) + 1            # a connection's segments are numbered in arrival order
        s, d, l4 = to_conn(c, seq=seqs[c], ack=int(rng.integers(0, 1 << 32)), **kw)
        return frame(s, d, l4, ident=len(out))

    peer = 0x0A000110
    for f in range(64):                                # all 64 flag combinations: to a closed port, to a connection
        out.append(frame(peer, sm.HOST, segment(peer, sm.HOST, 5000 + f, 443, seq=0xFFFFFFFF - (f % 3), ack=77 + f,
                                                flags=f), ident=f))
        out.append(conn_frame(HOT[f % 4], flags=f, payload=_bytes(rng, f % 7)))
    for k in range(40):                                # SYN / ACK to listening ports
        out.append(frame(peer + k % 3, sm.HOST, segment(peer + k % 3, sm.HOST, 6000 + k, LISTEN[k % 3],
                                                        seq=k, flags=tm.SYN if k % 2 else tm.ACK), ident=k))
    for c in HOT[:6]:                                  # a connection's ports swapped, its peer's neighbour: misses
        lip, fip, lp, fp = conn_tuple(c)
        out.append(frame(fip, lip, segment(fip, lip, lp, fp), ident=c))
        out.append(frame(fip ^ 1, lip, segment(fip ^ 1, lip, fp, lp), ident=c))
    for e in range(0, 20):                             # E < 20, the sum made to verify where two bytes fit
        l4 = _bytes(rng, e)
        out.append(frame(peer, sm.HOST, fix_sum(l4, peer, sm.HOST, 0) if e >= 2 else l4, ident=e))
    for do in range(0, 5):                             # H < 20
        s, d, l4 = to_conn(HOT[1], data_offset=do, payload=_bytes(rng, 8))
        out.append(frame(s, d, l4, ident=do))
    for do in (6, 10, 15):                             # H > E: to a connection, a listener, a closed port
        s, d, l4 = to_conn(HOT[0], data_offset=do)
        out.append(frame(s, d, l4))
        out.append(frame(peer, sm.HOST, segment(peer, sm.HOST, 6100, 80, flags=tm.SYN, data_offset=do)))
        out.append(frame(peer, sm.HOST, segment(peer, sm.HOST, 6100, 443, flags=tm.SYN, seq=do, data_offset=do)))
        out.append(frame(peer, sm.HOST, segment(peer, sm.HOST, 6100, 443, flags=tm.RST, data_offset=do)))
    for ihl in range(5, 16):                           # IP options, TCP options, padding behind the IP length
        for optlen in (0, 4, 40):
            s, d, l4 = to_conn(HOT[ihl % 5], options=_bytes(rng, optlen), payload=_bytes(rng, ihl), seq=ihl)
            out.append(frame(s, d, l4, ihl=ihl, pad=_bytes(rng, (ihl + optlen) % 7)))
    s, d, l4 = to_conn(HOT[0], payload=_bytes(rng, 5))
    out.append(frame(s, d, l4[:16] + bytes([l4[16] ^ 1]) + l4[17:]))       # a bad TCP checksum
    out.append(frame(s, sm.OTHER_HOST, segment(s, sm.OTHER_HOST, 1, 80)))  # another host's
    out.append(frame(s, d, l4, mf=1))                                      # a fragment
    out.append(frame(s, d, l4, proto=sm.UDP))
    out.append(sm._flip(frame(s, d, l4), 14 + 10))                         # a corrupted IP header
    while len(out) < n:
        kind = rng.random()
        if kind < 0.7:
            c = HOT[int(rng.integers(0, len(HOT)))] if kind < 0.5 else int(rng.integers(0, 300))
            out.append(conn_frame(c, payload=_bytes(rng, int(rng.integers(0, 30))), flags=tm.ACK | tm.PSH))
        elif kind < 0.8:
            out.append(frame(peer, sm.HOST, segment(peer, sm.HOST, int(rng.integers(0, 65536)), 80, flags=tm.SYN,
                                                    seq=int(rng.integers(0, 1 << 32)))))
        else:
            fl = [tm.SYN, tm.ACK, tm.SYN | tm.ACK, tm.RST, tm.FIN][int(rng.integers(0, 5))]
            out.append(frame(peer + 1, sm.HOST, segment(peer + 1, sm.HOST, int(rng.integers(0, 65536)),
                                                        CLOSED[int(rng.integers(0, 3))], flags=fl,
                                                        seq=int(rng.integers(0, 1 << 32)), ack=int(rng.integers(0, 1 << 32)))))
    return [out[int(k)] for k in rng.permutation(len(out))][:n]


def pattern(kind: str, n: int, nconns: int) -> list:
    """Only segments of known connections: "one" (a single run), "each" (every
    segment its own connection, R = n), "descending", "interleaved" (four
    connections in turn; seq counts a connection's arrivals), "twins" (pairs
    of identical headers whose payloads lie elsewhere)."""
    out = []
    for j in range(n):
        c = dict(one=nconns - 1, each=(j * 7) % nconns if nconns >= 7 * n else j, descending=nconns - 1 - j,
                 interleaved=(0, nconns - 1, nconns // 2, 1)[j % 4], twins=(j // 2) % 3)[kind]
        seq = j // 4 if kind == "interleaved" else 5 if kind == "twins" else j
        s, d, l4 = to_conn(c, seq=seq, payload=b"" if kind == "twins" else bytes([j & 0xFF]) * (j % 5))
        out.append(frame(s, d, l4, ident=j))
    return out


_CACHE = {}


def case(name, frames=None) -> dict:
    """frames: the wire batch; ip: the IPv4 bucket's packets (bytes behind the
    Ethernet header) with stack_model's info for each.  Computed once a name."""
    if name not in _CACHE:
        frames = mixed(name) if frames is None else frames
        out = sm.Rx(sm.rx_cfg()).batch(frames)
        ip = [bytes(frames[i][14:]) for i in out["buckets"][0]]
        assert len(ip) == len(out["ip"]) == len(frames)
        _CACHE[name] = dict(frames=frames, ip=ip, info=out["ip"])
    return _CACHE[name]


def items(c: dict, nconns: int, need: int = tm.NEED, reject: int = tm.REJECT, table=None) -> list:
    t = tcbs(nconns) if table is None else table
    return [tm.atomic(p, info, t, LISTEN, need, reject) for p, info in zip(c["ip"], c["info"])]
