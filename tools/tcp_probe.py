"""The TCP layer's two device calls timed on the shapes of a full rx / tx
batch, next to the checksum pass, the link-layer demux and the UDP demux on
the same box:
  rx   1 048 576 wire frames of 1 514 bytes in 2 304-byte slots (IPv4 / TCP from
       4 096 peers; frame i belongs to connection i mod nconns):
         sccsum_ipv4_frames_rss    the pass over the frames' L3 parts
         sccsum_eth_rx             count, scan, scatter over 3 buckets
         sccsum_udp_rx             the 8-bit bucket pass, 252 channels (same frames, UDP)
         sccsum_tcp_rx             253, 65 533 and 1 048 576 connections: one, two and
                                   three passes of the sort
  tx   1 048 576 payloads of 1 460 bytes behind 20 bytes of headroom:
         sccsum_tcp_send           the headers, the spans and the seeds
         sccsum_spans              the checksum pass over those spans
Every call is timed alone by stream events after a warm-up and reported as
the median of `reps` runs; outputs rotate over two sets.

usage: python tools/tcp_probe.py [reps]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eth_probe import FRAME, HOST, N, PEERS, SETS, SLOT, peer_ips, report, wire_batch
from seastar_amd import batch, native
from udp_probe import PORTS

PAYLOAD = 1460           # tx: the segment 1 480, the frame 1 500
TABLES = (253, 65533, 1 << 20)


def conn_of(c: np.ndarray) -> np.ndarray:
    """(local_ip, foreign_ip, local_port, foreign_port) of connection c: peer c mod 4096, a port pair of its own."""
    return np.stack([np.full(c.size, HOST, dtype=np.int64), peer_ips()[c % PEERS], 80 + (c // PEERS) % 3,
                     1024 + c // (3 * PEERS) + 512 * (c % 7)], axis=1)


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

    # ---- rx: the UDP frames first (the yardstick), then the same slots as TCP
    wire = wire_batch(dev)
    view = wire.data[: N * SLOT].view(N, SLOT)
    port = torch.tensor(PORTS, dtype=torch.int64, device=dev)[torch.arange(N, device=dev) % 252]
    view[:, 14 + 22] = (port >> 8).to(torch.uint8)
    view[:, 14 + 23] = (port & 0xFF).to(torch.uint8)
    rx = batch.eth_rx(wire, (0x0800, 0x0806))
    ip = rx.bucket(0)
    batch.ipv4_fill(ip)
    key = (ctypes.c_uint8 * 40)(*batch.RSS_KEY_40)
    status = [empty(N) for _ in range(SETS)]

    def frames_calls():
        return [batch.prepare_call(
            "sccsum_ipv4_frames_rss", wire.data, wire.bytes_len, ip.off, ip.length, empty(2 * N, torch.int16), status[k],
            N, FRAME - 14, ctypes.addressof(key), 40, native.RSS_DISPATCH, empty(N, torch.int32)) for k in range(SETS)]

    report("sccsum_ipv4_frames_rss UDP", s, frames_calls(), reps, N, "frames")
    protos = (ctypes.c_uint16 * 2)(0x0800, 0x0806)
    er_calls = [batch.prepare_call(
        "sccsum_eth_rx", wire.data, wire.bytes_len, wire.off, wire.length, N, ctypes.addressof(protos), 2, empty(N),
        empty(4, torch.int32), empty(N, torch.int32), empty(N, torch.int64), empty(N, torch.int32),
        empty(N, torch.int64), empty(int(lib.sccsum_eth_rx_workspace(N)))) for _ in range(SETS)]
    t_er = report("sccsum_eth_rx", s, er_calls, reps, N, "frames")
    table = batch.UdpPorts(PORTS)
    ur_calls = [batch.prepare_call(
        "sccsum_udp_rx", wire.data, wire.bytes_len, ip.off, ip.length, N, status[0], batch.UDP_NEED, batch.UDP_REJECT,
        HOST, table.handle, None, N, empty(N), empty(254, torch.int32), empty(N, torch.int32), empty(N, torch.int64),
        empty(N, torch.int32), empty(N, torch.int32), empty(N, torch.int16),
        empty(int(lib.sccsum_udp_rx_workspace(N)))) for k in range(SETS)]
    t_ur = report("sccsum_udp_rx C=252", s, ur_calls, reps, N, "frames")
    del ur_calls, er_calls
    table.close()

    t_tr = {}
    for nconns in TABLES:
        conns = conn_of(np.arange(nconns, dtype=np.int64))
        mine = torch.from_numpy(conn_of(np.arange(N, dtype=np.int64) % nconns)).to(dev)
        view[:, 14 + 9] = 6
        for k in range(4):
            view[:, 14 + 12 + k] = ((mine[:, 1] >> (24 - 8 * k)) & 0xFF).to(torch.uint8)
        view[:, 14 + 20], view[:, 14 + 21] = (mine[:, 3] >> 8).to(torch.uint8), (mine[:, 3] & 0xFF).to(torch.uint8)
        view[:, 14 + 22], view[:, 14 + 23] = (mine[:, 2] >> 8).to(torch.uint8), (mine[:, 2] & 0xFF).to(torch.uint8)
        view[:, 14 + 24:14 + 40] = 0
        view[:, 14 + 10:14 + 12] = 0                       # the fill generates over zero fields
        view[:, 14 + 32], view[:, 14 + 33] = 0x50, 0x10
        batch.ipv4_fill(ip)
        t_fr = report("sccsum_ipv4_frames_rss TCP", s, frames_calls(), reps, N, "frames")
        assert bool(torch.all((status[0] & (native.ST_OK | native.ST_L4_OK)) == 3))
        t = batch.TcpConns(conns, (22,))
        runs = min(N, nconns) + 1
        outs = [dict(first=empty(5, torch.int32), total=empty(4, torch.int64), order=empty(N, torch.int32))
                for _ in range(SETS)]
        tr_calls = [batch.prepare_call(
            "sccsum_tcp_rx", wire.data, wire.bytes_len, ip.off, ip.length, N, status[0], batch.TCP_NEED, batch.TCP_REJECT,
            HOST, t.handle, None, N, 0, empty(N), o["first"], o["order"], empty(4 * N, torch.int64),
            empty(N, torch.int32), empty(runs, torch.int32), empty(runs, torch.int32), empty(5 * N, torch.int32),
            empty(N, torch.int32), o["total"], empty(int(lib.sccsum_tcp_rx_workspace(N, nconns)))) for o in outs]
        t_tr[nconns] = report(f"sccsum_tcp_rx conns={nconns}", s, tr_calls, reps, N, "frames")
        assert outs[0]["first"].cpu().tolist() == [0, N, N, N, N]
        assert outs[0]["total"].cpu().tolist()[:2] == [min(N, nconns), 0]
        del tr_calls, outs, mine
        t.close()
        print(f"rx: tcp_rx {t_tr[nconns]:.1f} us ({nconns} connections) next to frames_rss {t_fr:.1f} us "
              f"({100 * t_tr[nconns] / t_fr:.1f} %), eth_rx {t_er:.1f} us, udp_rx {t_ur:.1f} us", flush=True)
    del wire, rx, ip, view
    torch.cuda.empty_cache()

    # ---- tx
    slot = PAYLOAD + 20
    pay = batch.PacketBatch(data=empty(N * slot + 16), off=torch.arange(N, dtype=torch.int64, device=dev) * slot + 20,
                            length=torch.full((N,), PAYLOAD, dtype=torch.int32, device=dev), bytes_len=N * slot,
                            max_len=PAYLOAD)
    rec = np.zeros(N, dtype=batch.TCP_OUT_DTYPE)
    rec["dst"], rec["seq"], rec["sport"] = peer_ips()[np.arange(N) % PEERS], np.arange(N), 80
    rec["dport"], rec["window"], rec["flags"], rec["hdr_len"], rec["mss"] = np.arange(N) % 50000, 4096, 0x18, 20, 1460
    d_out = torch.from_numpy(rec.view(np.uint8)).to(dev)
    opts = native.TcpOpts(HOST, 1500, 0)
    outs = [dict(l4_off=empty(N, torch.int64), l4_len=empty(N, torch.int32), sum_len=empty(N, torch.int32),
                 seed=empty(N, torch.int32), status=empty(N)) for _ in range(SETS)]
    ts_calls = [batch.prepare_call(
        "sccsum_tcp_send", ctypes.addressof(opts), pay.data, pay.bytes_len, pay.off, pay.length, d_out, N, o["l4_off"],
        o["l4_len"], o["sum_len"], o["seed"], empty(N, torch.int16), empty(N), empty(N), o["status"]) for o in outs]
    t_ts = report("sccsum_tcp_send", s, ts_calls, reps, N, "segments")
    assert bool(torch.all(outs[0]["status"] == native.ST_OK)) and bool(torch.all(outs[0]["sum_len"] == slot))
    sp_calls = [batch.prepare_call(
        "sccsum_spans", pay.data, pay.bytes_len, o["l4_off"], o["sum_len"], o["seed"], empty(N, torch.int16), None, N,
        slot) for o in outs]
    t_sp = report("sccsum_spans", s, sp_calls, reps, N, "segments")
    print(f"tx: tcp_send {t_ts:.1f} us next to the checksum pass over its spans {t_sp:.1f} us "
          f"({100 * t_ts / t_sp:.1f} %)", flush=True)


if __name__ == "__main__":
    main()
