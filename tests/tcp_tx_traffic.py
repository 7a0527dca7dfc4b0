"""Seeded transmit traffic for the TCP transmit fast path: tcbs of
tests/tcp_tx_model.py with their unsent queues, and the arrays
sccsum_tcp_tx_data takes for them.  No GPU, no library."""
from __future__ import annotations

import numpy as np

import tcp_tx_fast as fast
import tcp_tx_model as tm
from tcp_tx_fast import RUN_DTYPE, SND_DTYPE  # noqa: F401

TILE = 1024
KINDS = ("bulk", "window", "used_over", "used_equal", "window_zero", "small_cwnd", "cwnd_zero", "empty", "tiny_bufs",
         "wrap", "dupacks1", "dupacks2", "dupacks3", "probe", "packetq", "closing", "syn")


def one(rng: np.random.Generator, kind: str) -> tm.Tcb:
    t = tm.Tcb(dst=int(rng.integers(1, 1 << 32)), sport=int(rng.integers(1, 65536)), dport=int(rng.integers(1, 65536)),
               snd_next=int(rng.integers(0, 1 << 32)), snd_window=int(rng.integers(20000, 65536)),
               cwnd=int(rng.integers(1460, 30000)), mss=int(rng.choice([536, 1460, 1448, 8960])),
               rcv_next=int(rng.integers(0, 1 << 32)), rcv_window=int(rng.integers(0, 1 << 20)),
               window_scale=int(rng.integers(0, 8)), rtx_armed=bool(rng.integers(0, 2)))
    used = int(rng.integers(0, 3000))
    t.snd_unacknowledged = (t.snd_next - used) & tm.M32
    nbuf = int(rng.integers(1, 6))
    sizes = [int(x) for x in rng.integers(1, 2500, size=nbuf)]
    if rng.random() < 0.3:
        sizes.insert(int(rng.integers(0, len(sizes) + 1)), 0)          # a buffer of no bytes
    if kind == "window":
        t.snd_window = used + int(rng.integers(1, max(2, sum(sizes))))
    elif kind == "used_over":
        t.snd_window = max(1, used - 1)
        t.snd_unacknowledged = (t.snd_next - t.snd_window - 1) & tm.M32
    elif kind == "used_equal":
        t.snd_window = max(used, 1)
        t.snd_unacknowledged = (t.snd_next - t.snd_window) & tm.M32
    elif kind == "window_zero":
        t.snd_window = 0
    elif kind == "small_cwnd":
        t.cwnd = int(rng.integers(1, 500))
    elif kind == "cwnd_zero":
        t.cwnd = 0
    elif kind == "empty":
        sizes = [0] if rng.random() < 0.3 else []
    elif kind == "tiny_bufs":
        sizes = [int(x) for x in rng.integers(0, 3, size=int(rng.integers(1, 40)))]
    elif kind == "wrap":
        t.snd_next = (-int(rng.integers(1, 2000))) & tm.M32
        t.snd_unacknowledged = (t.snd_next - used) & tm.M32
    elif kind.startswith("dupacks"):
        t.dupacks = int(kind[-1]) + (int(rng.integers(0, 3)) if kind[-1] == "3" else 0)
    elif kind == "probe":
        t.window_probe = True
    elif kind == "packetq":
        t.packetq = int(rng.integers(1, 3))
    elif kind == "closing":
        t.state = str(rng.choice(["FIN_WAIT_1", "CLOSING", "LAST_ACK", tm.CLOSE_WAIT]))
    elif kind == "syn":
        t.state = str(rng.choice(["SYN_SENT", "SYN_RECEIVED"]))
    return t.queue(bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in sizes)


def mixed(seed: int, nconns: int) -> list:
    """nconns tcbs: the straight kinds three times as often as the others."""
    rng = np.random.default_rng(seed)
    weights = np.array([6.0 if k in ("bulk", "window") else 1.0 for k in KINDS])
    kinds = rng.choice(len(KINDS), size=nconns, p=weights / weights.sum())
    return [one(rng, KINDS[k]) for k in kinds]


def snd_record(t: tm.Tcb) -> tuple:
    return (t.dst, t.snd_next, t.snd_unacknowledged, t.snd_window, t.cwnd, t.rcv_next, t.sport, t.dport, t.mss,
            (t.rcv_window >> t.window_scale) & 0xFFFF, t.flags(), (0, 0, 0), (0, 0, 0))


def arrays(cases: list) -> dict:
    """snd, the CSR and every buffer's bytes back to back (`blob`, buffer j at blob_off[j])."""
    snd = np.array([snd_record(t) for t in cases], dtype=SND_DTYPE)
    bufs = [b for t in cases for b in t.unsent]
    buf_len = np.array([len(b) for b in bufs], dtype=np.uint32)
    buf_first = np.concatenate([[0], np.cumsum([len(t.unsent) for t in cases])]).astype(np.uint32)
    blob_off = np.concatenate([[0], np.cumsum(buf_len, dtype=np.uint64)]).astype(np.uint64)
    blob = np.frombuffer(b"".join(bufs), dtype=np.uint8).copy() if bufs else np.zeros(0, np.uint8)
    return dict(snd=snd, buf_len=buf_len, buf_first=buf_first, blob=blob, blob_off=blob_off[:-1])


def expect(cases: list, hw: tm.Hw, headroom: int, max_segs: int = 0x7FFFFFFF, max_bytes: int = tm.M32) -> dict:
    """fast.expect for the cases' arrays."""
    a = arrays(cases)
    return fast.expect(a["snd"], a["buf_len"], a["buf_first"], hw.mtu, headroom, hw.tx_tso, hw.max_packet_len, max_segs,
                       max_bytes)
