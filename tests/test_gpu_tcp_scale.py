"""sccsum_tcp_rx at scale: 1 024 tiles + 1 tile + 7 segments over 2^20 - 3
connections, so the sort takes three passes, every bucket row is scanned in
five chunks of 256 tiles and the one-block carry kernel runs into its second
chunk of 1 024 tiles.  The yardstick is tcp_model.fast_rx, which
tests/test_tcp_host.py pins to the per-segment model; the arrays are compared
on the device.  The resets (about one segment in a hundred) are compared
through the per-segment model's respond_with_reset."""
import numpy as np
import pytest
import torch

import stack_model as sm
import tcp_model as tm
import tcp_traffic
from seastar_amd import batch, native

pytestmark = pytest.mark.gpu

SLOT = 64
NCONNS = (1 << 20) - 3


def _frames(n: int, seed: int, conns: np.ndarray):
    """n IPv4 packets of 40-64 bytes in 64-byte slots, written column by
    column: mostly TCP segments of known connections (a skewed choice: some
    connections take hundreds of segments, most none), some to listening and to
    closed ports, headers shorter than 20 bytes or longer than the segment, an
    L4 below 20 bytes, padded ones, UDP, other hosts, fragments; the status
    bytes mostly OK | L4_OK; every other byte random (the flags among them)."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, n * SLOT, dtype=np.uint8)
    f = data.reshape(n, SLOT)
    kind = rng.random(n)
    length = rng.integers(40, SLOT + 1, n).astype(np.uint32)
    pad = np.where(kind < 0.05, np.minimum(length - 40, 3), 0)
    ip_len = length - pad
    ip_len = np.where((kind >= 0.05) & (kind < 0.07), rng.integers(20, 40, n), ip_len)      # an L4 of 0..19 bytes
    ip_len = np.where((kind >= 0.07) & (kind < 0.08), length + 1, ip_len)                   # longer than the frame
    f[:, 0] = 0x45
    f[:, 2], f[:, 3] = ip_len >> 8, ip_len & 0xFF
    f[:, 6] = np.where((kind >= 0.08) & (kind < 0.09), 0x20, 0)                             # MF
    f[:, 7] = np.where((kind >= 0.09) & (kind < 0.10), 3, 0)                                # a fragment offset
    f[:, 9] = np.where((kind >= 0.10) & (kind < 0.12), sm.UDP, sm.TCP)
    c = np.minimum((rng.random(n) ** 3 * NCONNS).astype(np.int64), NCONNS - 1)              # low indices are hot
    c = np.where(rng.random(n) < 0.5, rng.integers(0, NCONNS, n), c)
    lip, fip, lport, fport = (conns[c, k].copy() for k in range(4))
    lip = np.where((kind >= 0.12) & (kind < 0.14), sm.OTHER_HOST, lip)
    fip = np.where((kind >= 0.14) & (kind < 0.20), fip ^ 0x40000000, fip)                    # nobody's peer: 80 / 8080 listen, 443 not
    lport = np.where((kind >= 0.20) & (kind < 0.205), 7, lport)                              # a closed port
    for k in range(4):
        f[:, 12 + k] = (fip >> (24 - 8 * k)) & 0xFF
        f[:, 16 + k] = (lip >> (24 - 8 * k)) & 0xFF
    f[:, 20], f[:, 21] = fport >> 8, fport & 0xFF
    f[:, 22], f[:, 23] = lport >> 8, lport & 0xFF
    do = np.where((kind >= 0.21) & (kind < 0.23), 4, np.where((kind >= 0.23) & (kind < 0.26), 12, 5))
    do = np.where((kind >= 0.26) & (kind < 0.30), 6, do)                                     # four option bytes (or H > E)
    f[:, 32] = (do << 4) | (f[:, 32] & 0xF)
    f[:, 33] = np.where((kind >= 0.14) & (kind < 0.205) & (rng.random(n) < 0.85), f[:, 33] | tm.RST, f[:, 33])
    status = np.where(rng.random(n) < 0.95, tm.NEED, rng.integers(0, 32, n)).astype(np.uint8)
    off = np.arange(n, dtype=np.uint64) * np.uint64(SLOT)
    return data, off, length, status


def test_tcp_rx_three_passes_past_one_scan_chunk(dev):
    lib = native.load()
    tile = int(lib.sccsum_eth_tile_packets())
    n = 1025 * tile + 7
    assert (n + tile - 1) // tile > 1024 and NCONNS + 2 >= 1 << 16
    conns = tcp_traffic.conn_array(NCONNS)
    data, off, length, status = _frames(n, 43, conns)
    want = tm.fast_rx(data, data.size, off, length, status, tm.NEED, tm.REJECT, sm.HOST, conns, tcp_traffic.LISTEN)
    counts = np.diff(want["first"].astype(np.int64))
    assert counts[0] > n // 2 and counts[1] > n // 100 and 1000 < counts[2] < n // 50 and counts[3] > n // 10
    assert set(np.unique(want["cls"]).tolist()) == {tm.CONN, tm.LISTEN, tm.RESET, tm.NOCONN, tm.SKIP, tm.SHORT}
    runs = np.diff(want["run_first"].astype(np.int64))
    assert runs.size > 200000 and runs.max() > 100 and want["run_conn"][-1] > NCONNS - 100
    a, e = int(want["first"][2]), int(want["first"][3])
    rst = b"".join(tm.respond_with_reset(dict(sport=int(s["sport"]), dport=int(s["dport"]), seq=int(s["seq"]),
                                              ack=int(s["ack"]), flags=int(s["flags"])), sm.HOST, int(src))
                   for s, src in zip(want["seg"][a:e], want["src"][a:e]))
    b = batch.PacketBatch.from_host(data, off, length, device=dev)
    d_status = torch.from_numpy(status).to(dev)
    t = batch.TcpConns(conns, tcp_traffic.LISTEN, device=dev.index)
    assert t.bits == 21
    r = batch.tcp_rx(b, d_status, t, sm.HOST)
    nruns = want["run_conn"].size
    assert r.totals() == (nruns, e - a)
    got = dict(cls=r.cls, first=r.first, order=r.order, seg=r.seg.reshape(-1), src=r.src_all, run_conn=r.run_conn[:nruns],
               run_first=r.run_first[:nruns + 1], rst=r.rst[:20 * (e - a)], rst_dst=r.rst_dst[:e - a])
    signed = dict(cls=np.uint8, first=np.int32, order=np.int32, seg=np.uint8, src=np.int32, run_conn=np.int32,
                  run_first=np.int32, rst=np.uint8, rst_dst=np.int32)
    want = dict(want, rst=np.frombuffer(rst, dtype=np.uint8), rst_dst=want["src"][a:e])
    for name, g in got.items():
        assert torch.equal(g, torch.from_numpy(np.array(want[name]).view(signed[name])).to(dev)), name
    # a second run gives the same bytes
    r2 = batch.tcp_rx(b, d_status, t, sm.HOST)
    assert torch.equal(r.order, r2.order) and torch.equal(r.seg, r2.seg) and torch.equal(r.first, r2.first)
    assert torch.equal(r.run_first[:nruns + 1], r2.run_first[:nruns + 1]) and torch.equal(r.rst[:20 * (e - a)], r2.rst[:20 * (e - a)])
    t.close()
