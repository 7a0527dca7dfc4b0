"""The TCP receive fast path timed on the rx batches of tools/tcp_probe.py,
next to the calls in front of it on the same box:
  1 048 576 wire frames of 1 514 bytes in 2 304-byte slots (IPv4 / TCP from
  4 096 peers; frame i is segment i div nconns of connection i mod nconns, 1 460
  bytes of text each, every connection in sequence):
    sccsum_ipv4_frames_rss    the pass over the frames' L3 parts
    sccsum_tcp_rx             253, 65 533 and 1 048 576 connections
    sccsum_tcp_rx_data        over tcp_rx's outputs as they stand: every run
                              straight to its end, and the same with every
                              eighth run broken (a FIN) at a random segment
    sccsum_gather             the descriptors' text packed (what pack() does)
Every call is timed alone by stream events after a warm-up and reported as
the median of `reps` runs; outputs rotate over two sets.

usage: python tools/tcp_data_probe.py [reps]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eth_probe import FRAME, HOST, N, PEERS, SETS, SLOT, report, wire_batch
from seastar_amd import batch, native
from tcp_probe import TABLES, conn_of

TEXT = FRAME - 14 - 20 - 20


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

    wire = wire_batch(dev)
    view = wire.data[: N * SLOT].view(N, SLOT)
    ip = batch.eth_rx(wire, (0x0800, 0x0806)).bucket(0)
    key = (ctypes.c_uint8 * 40)(*batch.RSS_KEY_40)
    status = [empty(N) for _ in range(SETS)]
    idx = torch.arange(N, device=dev)
    for nconns in TABLES:
        mine = torch.from_numpy(conn_of(np.arange(N, dtype=np.int64) % nconns)).to(dev)
        seq = (idx // nconns) * TEXT
        view[:, 14 + 9] = 6
        for k in range(4):
            view[:, 14 + 12 + k] = ((mine[:, 1] >> (24 - 8 * k)) & 0xFF).to(torch.uint8)
        view[:, 14 + 20], view[:, 14 + 21] = (mine[:, 3] >> 8).to(torch.uint8), (mine[:, 3] & 0xFF).to(torch.uint8)
        view[:, 14 + 22], view[:, 14 + 23] = (mine[:, 2] >> 8).to(torch.uint8), (mine[:, 2] & 0xFF).to(torch.uint8)
        view[:, 14 + 24:14 + 40] = 0
        for k in range(4):
            view[:, 14 + 24 + k] = ((seq >> (24 - 8 * k)) & 0xFF).to(torch.uint8)
        view[:, 14 + 10:14 + 12] = 0                       # the fill generates over zero fields
        view[:, 14 + 32], view[:, 14 + 33] = 0x50, 0x10
        batch.ipv4_fill(ip)
        fr_calls = [batch.prepare_call(
            "sccsum_ipv4_frames_rss", wire.data, wire.bytes_len, ip.off, ip.length, empty(2 * N, torch.int16), status[k],
            N, FRAME - 14, ctypes.addressof(key), 40, native.RSS_DISPATCH, empty(N, torch.int32)) for k in range(SETS)]
        t_fr = report("sccsum_ipv4_frames_rss TCP", s, fr_calls, reps, N, "frames")
        assert bool(torch.all((status[0] & (native.ST_OK | native.ST_L4_OK)) == 3))
        t = batch.TcpConns(conn_of(np.arange(nconns, dtype=np.int64)), (22,))
        runs = min(N, nconns) + 1
        rx = [dict(first=empty(5, torch.int32), total=empty(4, torch.int64), order=empty(N, torch.int32),
                   seg=empty(4 * N, torch.int64), run_conn=empty(runs, torch.int32), run_first=empty(runs, torch.int32))
              for _ in range(SETS)]
        tr_calls = [batch.prepare_call(
            "sccsum_tcp_rx", wire.data, wire.bytes_len, ip.off, ip.length, N, status[0], batch.TCP_NEED, batch.TCP_REJECT,
            HOST, t.handle, None, N, 0, empty(N), o["first"], o["order"], o["seg"], empty(N, torch.int32), o["run_conn"],
            o["run_first"], empty(5 * N, torch.int32), empty(N, torch.int32), o["total"],
            empty(int(lib.sccsum_tcp_rx_workspace(N, nconns)))) for o in rx]
        t_tr = report(f"sccsum_tcp_rx conns={nconns}", s, tr_calls, reps, N, "frames")
        assert rx[0]["first"].cpu().tolist() == [0, N, N, N, N]
        t.close()

        rcv = np.zeros(nconns, dtype=batch.TCP_RCV_DTYPE)
        rcv["window"], rcv["room"], rcv["cap"], rcv["mss"] = 29200 << 7, 1 << 30, 29200 << 7, TEXT
        rcv["flags"] = native.TCP_RCV_ELIGIBLE
        d_rcv = torch.from_numpy(rcv.view(np.uint8)).to(dev)
        for broken in (False, True):
            if broken:   # every eighth run gets a FIN at a random segment (byte 30 of the record: the flags)
                rf = rx[0]["run_first"].cpu().numpy().view(np.uint32).astype(np.int64)
                r8 = np.arange(0, runs - 1, 8)
                at = rf[r8] + np.random.default_rng(17).integers(0, 1 << 30, r8.size) % (rf[r8 + 1] - rf[r8])
                for o in rx:
                    o["seg"].view(torch.uint8).view(N, 32)[torch.from_numpy(at).to(dev), 30] |= 1
            outs = [dict(run=empty(4 * runs, torch.int64), desc=empty(2 * N, torch.int64), total=empty(4, torch.int64))
                    for _ in range(SETS)]
            rd_calls = [batch.prepare_call(
                "sccsum_tcp_rx_data", wire.data, o["seg"], o["first"], o["run_conn"], o["run_first"], o["total"], N, d_rcv,
                nconns, 0xFFFFFFFF, q["run"], q["desc"], q["total"],
                empty(int(lib.sccsum_tcp_rx_data_workspace(N, nconns)))) for o, q in zip(rx, outs)]
            what = "every eighth run broken" if broken else "all in sequence"
            t_rd = report(f"sccsum_tcp_rx_data conns={nconns} {what}", s, rd_calls, reps, N, "segments")
            total = outs[0]["total"].cpu().tolist()
            assert total[0] == N or broken, total
            assert total[1] == total[2] == total[0] * TEXT, total
            dst = empty(total[1] + 16)
            ga_calls = [batch.prepare_call("sccsum_gather", q["desc"], total[0], dst) for q in outs]
            t_ga = report(f"sccsum_gather of {total[0]} descriptors", s, ga_calls, reps, total[0], "segments")
            print(f"rx: tcp_rx_data {t_rd:.1f} us ({nconns} connections, {what}: {total[0]} of {N} segments taken) "
                  f"next to tcp_rx {t_tr:.1f} us ({100 * t_rd / t_tr:.1f} %), frames_rss {t_fr:.1f} us; the gather of "
                  f"their {total[1] >> 20} MiB {t_ga:.1f} us", flush=True)
            del rd_calls, ga_calls, outs, dst
        del tr_calls, rx, mine, d_rcv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
