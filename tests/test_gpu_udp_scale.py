"""sccsum_udp_rx past one scan chunk: 1 024 tiles + 1 tile + 7 frames of 28-64
bytes with 252 channels, so that every one of the 253 bucket rows is scanned
in five chunks of 256 tiles with the sum carried along, and the rows are
spread over the device (the many-bucket scan).  The yardstick is
udp_model.fast_rx, which tests/test_udp_host.py pins to the per-datagram
model; the arrays are compared on the device."""
import numpy as np
import pytest
import torch

import stack_model as sm
import udp_model
import udp_traffic
from seastar_amd import batch, native

pytestmark = pytest.mark.gpu

SLOT = 64


def _frames(n: int, seed: int):
    """n IPv4 packets of 28-64 bytes in 64-byte slots, written column by
    column: mostly UDP for the host to one of 252 ports (a skewed choice: the
    buckets differ in size by orders of magnitude), some to unbound ports, some
    with an L4 below 8 bytes, padded ones, TCP, other hosts, fragments; the
    status bytes mostly OK."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, n * SLOT, dtype=np.uint8)
    f = data.reshape(n, SLOT)
    kind = rng.random(n)
    length = rng.integers(28, SLOT + 1, n).astype(np.uint32)
    pad = np.where(kind < 0.1, np.minimum(length - 28, 3), 0)
    ip_len = length - pad
    ip_len = np.where((kind >= 0.1) & (kind < 0.13), rng.integers(20, 28, n), ip_len)       # an L4 of 0..7 bytes
    ip_len = np.where((kind >= 0.13) & (kind < 0.14), length + 1, ip_len)                   # longer than the frame
    f[:, 0] = 0x45
    f[:, 2], f[:, 3] = ip_len >> 8, ip_len & 0xFF
    f[:, 6] = np.where((kind >= 0.14) & (kind < 0.16), 0x20, 0)                             # MF
    f[:, 7] = np.where((kind >= 0.16) & (kind < 0.17), 3, 0)                                # a fragment offset
    f[:, 9] = np.where((kind >= 0.17) & (kind < 0.20), sm.TCP, sm.UDP)
    dst = np.where((kind >= 0.20) & (kind < 0.23), sm.OTHER_HOST, sm.HOST)
    for k in range(4):
        f[:, 16 + k] = (dst >> (24 - 8 * k)) & 0xFF
    ch = np.minimum((rng.random(n) ** 4 * 252).astype(np.int64), 251)                       # channel 0 is hot
    port = np.array(udp_traffic.PORTS)[ch]
    port = np.where((kind >= 0.23) & (kind < 0.30), np.array(udp_traffic.UNBOUND)[ch % 5], port)
    f[:, 22], f[:, 23] = port >> 8, port & 0xFF
    status = np.where(rng.random(n) < 0.95, native.ST_OK, rng.integers(0, 32, n)).astype(np.uint8)
    off = np.arange(n, dtype=np.uint64) * np.uint64(SLOT)
    return data, off, length, status


def test_udp_rx_rows_past_one_scan_chunk(dev):
    lib = native.load()
    tile = int(lib.sccsum_eth_tile_packets())
    n = 1025 * tile + 7
    assert (n + tile - 1) // tile > 4 * 256
    data, off, length, status = _frames(n, 41)
    want = udp_model.fast_rx(data, data.size, off, length, status, batch.UDP_NEED, batch.UDP_REJECT, sm.HOST,
                             udp_traffic.PORTS)
    counts = np.diff(want["first"].astype(np.int64))
    assert counts.size == 253 and counts[:252].min() > 0 and counts[0] > 50 * counts[251] and counts[252] > n // 5
    assert {native.UDP_SKIP, native.UDP_SHORT, native.UDP_NOPORT} <= set(np.unique(want["cls"]).tolist())
    b = batch.PacketBatch.from_host(data, off, length, device=dev)
    d_status = torch.from_numpy(status).to(dev)
    ports = batch.UdpPorts(udp_traffic.PORTS, device=dev.index)
    r = batch.udp_rx(b, d_status, ports, sm.HOST)
    got = dict(cls=r.cls, first=r.first, order=r.order, pay_off=r.pay_off, pay_len=r.pay_len, src=r.src_all,
               sport=r.sport_all)
    signed = dict(cls=np.uint8, first=np.int32, order=np.int32, pay_off=np.int64, pay_len=np.int32, src=np.int32,
                  sport=np.int16)
    for name, t in got.items():
        assert torch.equal(t, torch.from_numpy(want[name].view(signed[name])).to(dev)), name
    # a second run gives the same bytes
    r2 = batch.udp_rx(b, d_status, ports, sm.HOST)
    assert torch.equal(r.order, r2.order) and torch.equal(r.pay_off, r2.pay_off) and torch.equal(r.first, r2.first)
    ports.close()
