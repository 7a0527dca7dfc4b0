"""The UDP layer's three device calls timed on the shapes of a full rx / tx
batch, next to the checksum pass and the link-layer demux on the same box:
  rx   1 048 576 wire frames of 1 514 bytes in 2 304-byte slots (IPv4 / UDP from
       4 096 peers to `channels` bound ports):
         sccsum_ipv4_frames_rss    the pass over the frames' L3 parts
         sccsum_eth_rx             count, scan, scatter over 3 buckets
         sccsum_udp_rx             the same over channels + 1 buckets (64 and 252
                                   channels: the one-block and the spread scan)
       524 288 datagrams of 2 952 bytes reassembled from two fragments each:
         sccsum_udp_rx_reasm       on reassembly's lists
  tx   1 048 576 payloads of 1 472 bytes behind 8 bytes of headroom:
         sccsum_udp_send           the headers, the spans and the seeds
         sccsum_spans              the checksum pass over those spans
Every call is timed alone by stream events after a warm-up and reported as
the median of `reps` runs; outputs rotate over two sets.

usage: python tools/udp_probe.py [reps]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eth_probe import FRAME, HOST, L4, N, PEERS, SETS, SLOT, peer_ips, report, wire_batch
from seastar_amd import batch, native

PORTS = [1024 + 61 * k for k in range(252)]
PAYLOAD = L4             # tx: 1 472 bytes of payload, the datagram 1 480, the frame 1 500
DGRAM = 2952             # rx, reassembled: two fragments at mtu 1500


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    lib = native.load()
    native.check(lib.sccsum_init(0), "sccsum_init")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    print(f"box: {torch.cuda.get_device_name(0)}, {N} frames of {FRAME} B in {SLOT} B slots, {PEERS} peers", flush=True)

    def empty(numel, dtype=torch.uint8):
        return torch.empty(numel, dtype=dtype, device=dev)

    # ---- rx, atomic frames
    wire = wire_batch(dev)
    port = torch.tensor(PORTS, dtype=torch.int64, device=dev)[torch.arange(N, device=dev) % 252]
    view = wire.data[: N * SLOT].view(N, SLOT)
    view[:, 14 + 22] = (port >> 8).to(torch.uint8)
    view[:, 14 + 23] = (port & 0xFF).to(torch.uint8)
    rx = batch.eth_rx(wire, (0x0800, 0x0806))
    ip = rx.bucket(0)
    batch.ipv4_fill(ip)  # valid checksums, so that the frames pass takes its usual path
    key = (ctypes.c_uint8 * 40)(*batch.RSS_KEY_40)
    status = [empty(N) for _ in range(SETS)]
    fr_calls = [batch.prepare_call(
        "sccsum_ipv4_frames_rss", wire.data, wire.bytes_len, ip.off, ip.length, empty(2 * N, torch.int16), status[k], N,
        FRAME - 14, ctypes.addressof(key), 40, native.RSS_DISPATCH, empty(N, torch.int32)) for k in range(SETS)]
    t_fr = report("sccsum_ipv4_frames_rss", s, fr_calls, reps, N, "frames")
    assert bool(torch.all((status[0] & (native.ST_OK | native.ST_L4_OK)) == 3))
    protos = (ctypes.c_uint16 * 2)(0x0800, 0x0806)
    er_calls = [batch.prepare_call(
        "sccsum_eth_rx", wire.data, wire.bytes_len, wire.off, wire.length, N, ctypes.addressof(protos), 2, empty(N),
        empty(4, torch.int32), empty(N, torch.int32), empty(N, torch.int64), empty(N, torch.int32),
        empty(N, torch.int64), empty(int(lib.sccsum_eth_rx_workspace(N)))) for _ in range(SETS)]
    t_er = report("sccsum_eth_rx", s, er_calls, reps, N, "frames")
    t_ur = {}
    for channels in (64, 252):
        table = batch.UdpPorts(PORTS[:channels])
        firsts = [empty(channels + 2, torch.int32) for _ in range(SETS)]
        ur_calls = [batch.prepare_call(
            "sccsum_udp_rx", wire.data, wire.bytes_len, ip.off, ip.length, N, status[0], batch.UDP_NEED, batch.UDP_REJECT,
            HOST, table.handle, None, N, empty(N), firsts[k], empty(N, torch.int32), empty(N, torch.int64),
            empty(N, torch.int32), empty(N, torch.int32), empty(N, torch.int16),
            empty(int(lib.sccsum_udp_rx_workspace(N)))) for k in range(SETS)]
        t_ur[channels] = report(f"sccsum_udp_rx C={channels}", s, ur_calls, reps, N, "frames")
        f = firsts[0].cpu().numpy()
        assert f[-1] == N and f[channels] == (N if channels == 252 else (N // 252) * 64 + min(N % 252, 64))
        del ur_calls
        table.close()
    print(f"rx: udp_rx {t_ur[64]:.1f} us (64 channels) / {t_ur[252]:.1f} us (252) next to frames_rss {t_fr:.1f} us "
          f"({100 * t_ur[64] / t_fr:.1f} % / {100 * t_ur[252] / t_fr:.1f} %) and eth_rx {t_er:.1f} us", flush=True)
    del wire, rx, ip, view, fr_calls, er_calls
    torch.cuda.empty_cache()

    # ---- rx, reassembled datagrams: built by the send path, two frames each
    m = N // 2
    l4 = batch.PacketBatch(data=torch.zeros(m * DGRAM + 16, dtype=torch.uint8, device=dev),
                           off=torch.arange(m, dtype=torch.int64, device=dev) * DGRAM,
                           length=torch.full((m,), DGRAM, dtype=torch.int32, device=dev), bytes_len=m * DGRAM,
                           max_len=DGRAM)
    port = torch.tensor(PORTS, dtype=torch.int64, device=dev)[torch.arange(m, device=dev) % 252]
    dv = l4.data[: m * DGRAM].view(m, DGRAM)
    dv[:, 2] = (port >> 8).to(torch.uint8)
    dv[:, 3] = (port & 0xFF).to(torch.uint8)
    src = torch.from_numpy(peer_ips()).to(dev)[torch.arange(m, device=dev) % PEERS].to(torch.int32)
    ids = (torch.arange(m, device=dev) // PEERS).to(torch.int16)
    sent = batch.ipv4_send(l4, src, torch.full((m,), 17, dtype=torch.uint8, device=dev), 1500, HOST, ids=ids).pack()
    assert sent.n == N
    st = empty(N)
    batch.ipv4_frames(sent, status=st)
    recs = batch.frag_records(sent, st)
    rr = batch.reassemble(recs)
    d, _, pending, host_recs = rr.totals()
    # a few dozen of the 2^19 keys share their 32-bit mix with another one and are the host's (two records each)
    assert pending == 0 and d + host_recs // 2 == m and host_recs < 1000
    m = d
    table = batch.UdpPorts(PORTS)
    firsts = [empty(254, torch.int32) for _ in range(SETS)]
    um_calls = [batch.prepare_call(
        "sccsum_udp_rx_reasm", rr.desc, rr.dgram_first, rr.dgram_off, rr.dgram_len, rr.dgram_head, m, recs, N, None, 0,
        0, 0, table.handle, empty(m), firsts[k], empty(m, torch.int32), empty(m, torch.int32), empty(m, torch.int32),
        empty(m, torch.int16), empty(int(lib.sccsum_udp_rx_reasm_workspace(m)))) for k in range(SETS)]
    t_um = report("sccsum_udp_rx_reasm C=252", s, um_calls, reps, m, "datagrams")
    f = firsts[0].cpu().numpy()
    assert f[252] == m and f[253] == m
    print(f"rx: udp_rx_reasm {t_um:.1f} us for {m} datagrams of {DGRAM} B", flush=True)
    del l4, dv, sent, recs, rr, um_calls
    table.close()
    torch.cuda.empty_cache()

    # ---- tx
    slot = PAYLOAD + 8
    pay = batch.PacketBatch(data=empty(N * slot + 16), off=torch.arange(N, dtype=torch.int64, device=dev) * slot + 8,
                            length=torch.full((N,), PAYLOAD, dtype=torch.int32, device=dev), bytes_len=N * slot,
                            max_len=PAYLOAD)
    dst = torch.from_numpy(peer_ips()).to(dev)[torch.arange(N, device=dev) % PEERS].to(torch.int32)
    dport = (torch.arange(N, device=dev) % 50000).to(torch.int16)
    sport = torch.full((N,), 4000, dtype=torch.int16, device=dev)
    opts = native.UdpOpts(HOST, 1500, 0)
    outs = [dict(l4_off=empty(N, torch.int64), l4_len=empty(N, torch.int32), sum_len=empty(N, torch.int32),
                 seed=empty(N, torch.int32), status=empty(N)) for _ in range(SETS)]
    us_calls = [batch.prepare_call(
        "sccsum_udp_send", ctypes.addressof(opts), pay.data, pay.bytes_len, pay.off, pay.length, dst, dport, sport, N,
        o["l4_off"], o["l4_len"], o["sum_len"], o["seed"], empty(N), empty(N), o["status"]) for o in outs]
    t_us = report("sccsum_udp_send", s, us_calls, reps, N, "datagrams")
    assert bool(torch.all(outs[0]["status"] == native.ST_OK)) and bool(torch.all(outs[0]["sum_len"] == slot))
    sp_calls = [batch.prepare_call(
        "sccsum_spans", pay.data, pay.bytes_len, o["l4_off"], o["sum_len"], o["seed"], empty(N, torch.int16), None, N,
        slot) for o in outs]
    t_sp = report("sccsum_spans", s, sp_calls, reps, N, "datagrams")
    print(f"tx: udp_send {t_us:.1f} us next to the checksum pass over its spans {t_sp:.1f} us "
          f"({100 * t_us / t_sp:.1f} %)", flush=True)


if __name__ == "__main__":
    main()
