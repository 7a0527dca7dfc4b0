"""The TCP ACK fast path timed on rx batches of pure ACKs, next to the calls in
front of it on the same box:
  1 048 576 wire frames of 60 bytes in 2 304-byte slots (IPv4 / TCP from 4 096
  peers; frame i is ACK i div nconns of connection i mod nconns, each one
  acknowledging one more 1 460-byte entry of the connection's retransmit queue):
    sccsum_ipv4_frames_rss    the pass over the frames' L3 parts
    sccsum_tcp_rx             253, 65 533 and 1 048 576 connections
    sccsum_tcp_rx_data        over tcp_rx's outputs as they stand (it refuses
                              every pure ACK at the head of its run)
    sccsum_tcp_rx_acks        over the same outputs: every run straight to its end
  and 65 536 ACKs of ONE connection (the records written as tcp_rx leaves
  them): the serial walk's cost, one lane walking every ACK and every entry.
Every call is timed alone by stream events after a warm-up and reported as
the median of `reps` runs; outputs rotate over two sets.

usage: python tools/tcp_ack_probe.py [reps]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eth_probe import HOST, N, PEERS, SETS, SLOT, report, wire_batch
from seastar_amd import batch, native
from tcp_probe import TABLES, conn_of

FRAME, TEXT, ONE = 60, 1460, 1 << 16
NOW = 5_000_000_000


def state_and_queues(dev, per_conn: np.ndarray):
    """Connection c holds per_conn[c] entries of TEXT bytes sent 40 ms ago; una = 1000 c."""
    nconns = int(per_conn.size)
    st = np.zeros(nconns, dtype=batch.TCP_ACK_DTYPE)
    st["una"] = (np.arange(nconns, dtype=np.int64) * 1000) & 0xFFFFFFFF
    st["next"] = (st["una"].astype(np.int64) + per_conn * TEXT) & 0xFFFFFFFF
    st["wl2"] = st["una"]
    st["window"], st["cwnd"], st["ssthresh"], st["mss"], st["rto"] = 1 << 20, 10 * TEXT, 64 * TEXT, TEXT, 1000
    st["unsent_len"], st["window_scale"] = 1 << 20, 7
    st["flags"] = native.TCP_ACK_ELIGIBLE | native.TCP_ACK_FIRST_SAMPLE
    nq = int(per_conn.sum())
    first = np.concatenate([[0], np.cumsum(per_conn)]).astype(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return (up(st.view(np.uint8)), up(first), torch.full((nq,), TEXT, dtype=torch.int32, device=dev),
            torch.full((nq,), TEXT, dtype=torch.int32, device=dev),
            torch.full((nq,), NOW - 40_000_000, dtype=torch.int64, device=dev), nq)


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
    wire.length.fill_(FRAME)
    wire.max_len = FRAME
    view = wire.data[: N * SLOT].view(N, SLOT)
    view[:, 14 + 2], view[:, 14 + 3] = 0, 40                  # the IP length: the two headers
    ip = batch.eth_rx(wire, (0x0800, 0x0806)).bucket(0)
    key = (ctypes.c_uint8 * 40)(*batch.RSS_KEY_40)
    status = [empty(N) for _ in range(SETS)]
    idx = torch.arange(N, device=dev)
    for nconns in TABLES:
        mine = torch.from_numpy(conn_of(np.arange(N, dtype=np.int64) % nconns)).to(dev)
        ack = ((idx % nconns) * 1000 + (idx // nconns + 1) * TEXT) & 0xFFFFFFFF
        view[:, 14 + 9] = 6
        for k in range(4):
            view[:, 14 + 12 + k] = ((mine[:, 1] >> (24 - 8 * k)) & 0xFF).to(torch.uint8)
        view[:, 14 + 20], view[:, 14 + 21] = (mine[:, 3] >> 8).to(torch.uint8), (mine[:, 3] & 0xFF).to(torch.uint8)
        view[:, 14 + 22], view[:, 14 + 23] = (mine[:, 2] >> 8).to(torch.uint8), (mine[:, 2] & 0xFF).to(torch.uint8)
        view[:, 14 + 24:14 + 40] = 0
        for k in range(4):
            view[:, 14 + 28 + k] = ((ack >> (24 - 8 * k)) & 0xFF).to(torch.uint8)
        view[:, 14 + 10:14 + 12] = 0                       # the fill generates over zero fields
        view[:, 14 + 32], view[:, 14 + 33] = 0x50, 0x10
        view[:, 14 + 34], view[:, 14 + 35] = 0x20, 0x00    # the header window: 8 192 << 7
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
        outs = [dict(run=empty(4 * runs, torch.int64), desc=empty(2 * N, torch.int64), total=empty(4, torch.int64))
                for _ in range(SETS)]
        rd_calls = [batch.prepare_call(
            "sccsum_tcp_rx_data", wire.data, o["seg"], o["first"], o["run_conn"], o["run_first"], o["total"], N, d_rcv,
            nconns, 0xFFFFFFFF, q["run"], q["desc"], q["total"],
            empty(int(lib.sccsum_tcp_rx_data_workspace(N, nconns)))) for o, q in zip(rx, outs)]
        t_rd = report(f"sccsum_tcp_rx_data conns={nconns} pure ACKs", s, rd_calls, reps, N, "segments")
        assert outs[0]["total"].cpu().tolist()[0] == 0

        per_conn = np.full(nconns, N // nconns, dtype=np.int64)
        per_conn[:N % nconns] += 1
        d_st, q_first, q_len, q_meta, q_tx, nq = state_and_queues(dev, per_conn)
        aouts = [dict(run=empty(8 * runs, torch.int64), total=empty(4, torch.int64)) for _ in range(SETS)]
        ws = int(lib.sccsum_tcp_rx_acks_workspace(N, nconns, nq))
        ra_calls = [batch.prepare_call(
            "sccsum_tcp_rx_acks", o["seg"], o["first"], o["run_conn"], o["run_first"], o["total"], N, d_st, nconns, q_first,
            q_len, q_meta, q_tx, nq, NOW, q["run"], q["total"], empty(ws)) for o, q in zip(rx, aouts)]
        t_ra = report(f"sccsum_tcp_rx_acks conns={nconns}", s, ra_calls, reps, N, "ACKs")
        total = aouts[0]["total"].cpu().tolist()
        assert total == [min(N, nconns), N, N, N * TEXT], total
        print(f"rx: tcp_rx_acks {t_ra:.1f} us ({nconns} connections: {total[1]} of {N} ACKs taken, {total[2]} entries "
              f"popped, workspace {ws >> 10} KiB) next to tcp_rx {t_tr:.1f} us ({100 * t_ra / t_tr:.1f} %), tcp_rx_data "
              f"{t_rd:.1f} us, frames_rss {t_fr:.1f} us", flush=True)
        del tr_calls, rd_calls, ra_calls, rx, outs, aouts, mine, d_rcv, d_st, q_first, q_len, q_meta, q_tx
        torch.cuda.empty_cache()

    # ONE connection: the records as tcp_rx leaves them, written here
    seg = np.zeros(ONE, dtype=batch.TCP_SEG_DTYPE)
    seg["ack"], seg["window"], seg["flags"], seg["hdr_len"] = (np.arange(ONE, dtype=np.int64) + 1) * TEXT, 0x2000, 0x10, 20
    up = lambda a, as_type: torch.from_numpy(np.ascontiguousarray(a).view(as_type)).to(dev)   # noqa: E731
    d_seg, d_first = up(seg, np.int64), up(np.array([0, ONE, ONE, ONE, ONE], dtype=np.uint32), np.int32)
    d_rc, d_rf = up(np.array([0, 0], dtype=np.uint32), np.int32), up(np.array([0, ONE], dtype=np.uint32), np.int32)
    d_rt = up(np.array([1, 0, 0, 0], dtype=np.uint64), np.int64)
    d_st, q_first, q_len, q_meta, q_tx, nq = state_and_queues(dev, np.array([ONE], dtype=np.int64))
    aouts = [dict(run=empty(8 * 2, torch.int64), total=empty(4, torch.int64)) for _ in range(SETS)]
    ws = int(lib.sccsum_tcp_rx_acks_workspace(ONE, 1, nq))
    calls = [batch.prepare_call("sccsum_tcp_rx_acks", d_seg, d_first, d_rc, d_rf, d_rt, ONE, d_st, 1, q_first, q_len, q_meta,
                                q_tx, nq, NOW, q["run"], q["total"], empty(ws)) for q in aouts]
    t_one = report("sccsum_tcp_rx_acks conns=1", s, calls, reps, ONE, "ACKs")
    total = aouts[0]["total"].cpu().tolist()
    assert total == [1, ONE, ONE, ONE * TEXT], total
    print(f"rx: tcp_rx_acks {t_one:.1f} us for {ONE} ACKs of ONE connection popping {ONE} entries: the serial walk, "
          f"{1e3 * t_one / ONE:.1f} ns per ACK", flush=True)


if __name__ == "__main__":
    main()
