"""The TCP transmit fast path timed next to the calls behind it on the same box:
  1 048 576 segments of 1 460 bytes from 253, 65 533 and 1 048 576 connections
  (every queue holds exactly its window: the chain sends all of it), the queues
  as one buffer per segment, one 64 KiB buffer per 45 segments, and 91-byte
  buffers, sixteen to a segment:
    sccsum_tcp_tx_data        the cut: run records, segment arrays, descriptors
    sccsum_gather             the descriptors' payloads into the packed layout
                              (what pack() does: the _snd.data clones)
    sccsum_tcp_send           the headers into the layout's headroom
    sccsum_spans              the checksum pass over the same segments
Every call is timed alone by stream events after a warm-up and reported as
the median of `reps` runs; outputs rotate over two sets.

usage: python tools/tcp_tx_data_probe.py [reps]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eth_probe import HOST, N, SETS, report
from seastar_amd import batch, native

TEXT, HEADROOM, MTU = 1460, 20, 1500
TABLES = (253, 65533, 1 << 20)
LAYOUTS = (("one buffer per segment", TEXT), ("one 64 KiB buffer per 45 segments", 65536),
           ("91-byte buffers, sixteen to a segment", 91))


def queues(segs: np.ndarray, size: int):
    """The CSR of queues of segs[c] * TEXT bytes in buffers of `size` bytes (the last one of a queue shorter)."""
    nbytes = segs * TEXT
    count = -(-nbytes // size)
    first = np.concatenate([[0], np.cumsum(count)])
    conn = np.repeat(np.arange(segs.size), count)
    k = np.arange(int(first[-1])) - first[conn]
    length = np.minimum(size, nbytes[conn] - k * size)
    start = np.concatenate([[0], np.cumsum(nbytes)])[conn] + k * size
    return first.astype(np.uint32), length.astype(np.uint32), start.astype(np.uint64)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    lib = native.load()
    native.check(lib.sccsum_init(0), "sccsum_init")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    print(f"box: {torch.cuda.get_device_name(0)}, {N} segments of {TEXT} B, headroom {HEADROOM}", flush=True)

    def empty(numel, dtype=torch.uint8):
        return torch.empty(numel, dtype=dtype, device=dev)

    def up(a, as_type):
        return torch.from_numpy(np.ascontiguousarray(a).view(as_type)).to(dev)

    blob = torch.randint(0, 256, (N * TEXT,), dtype=torch.uint8, device=dev)
    opts = native.TcpTxOpts(HOST, MTU, 65535, HEADROOM, 0)
    send_opts = native.TcpOpts(HOST, MTU, 0)
    lay_bytes = N * (TEXT + HEADROOM)
    staging = empty(lay_bytes + 16)
    for nconns in TABLES:
        segs = np.full(nconns, N // nconns, dtype=np.int64)
        segs[:N % nconns] += 1
        snd = np.zeros(nconns, dtype=batch.TCP_SND_DTYPE)
        snd["dst"] = 0x0A000100 + np.arange(nconns) % 4096
        snd["next"] = snd["una"] = (np.arange(nconns, dtype=np.int64) * 2654435761) & 0xFFFFFFFF
        snd["window"], snd["cwnd"], snd["mss"], snd["wnd"] = segs * TEXT, 1 << 30, TEXT, 512
        snd["sport"], snd["dport"] = 1024 + np.arange(nconns) % 60000, 80
        snd["flags"] = native.TCP_SND_ELIGIBLE
        d_snd = up(snd, np.uint8)
        for what, size in LAYOUTS:
            first, length, start = queues(segs, size)
            nbuf = int(length.size)
            d_first, d_len = up(first, np.int32), up(length, np.int32)
            d_src = up(start + np.uint64(blob.data_ptr()), np.int64)
            outs = [dict(run=empty(4 * nconns, torch.int64), off=empty(N, torch.int64), len=empty(N, torch.int32),
                         out=empty(3 * N, torch.int64), seg_first=empty(N + 1, torch.int32),
                         desc=empty(2 * (N + nbuf), torch.int64), total=empty(4, torch.int64)) for _ in range(SETS)]
            ws = int(lib.sccsum_tcp_tx_data_workspace(nconns, nbuf))
            calls = [batch.prepare_call(
                "sccsum_tcp_tx_data", ctypes.addressof(opts), d_snd, nconns, d_src, d_len, d_first, nbuf, N, 0xFFFFFFFF,
                o["run"], o["off"], o["len"], o["out"], o["seg_first"], o["desc"], o["total"], empty(ws)) for o in outs]
            t_cut = report(f"sccsum_tcp_tx_data conns={nconns}", s, calls, reps, N, "segments")
            total = outs[0]["total"].cpu().tolist()
            assert total[0] == N and total[1] == total[3] == lay_bytes, total
            ga = [batch.prepare_call("sccsum_gather", o["desc"], total[2], staging) for o in outs]
            t_ga = report(f"sccsum_gather of {total[2]} descriptors", s, ga, reps, N, "segments")
            print(f"tx: tcp_tx_data {t_cut:.1f} us ({nconns} connections, {what}: {nbuf} buffers, {total[2]} descriptors, "
                  f"workspace {ws >> 10} KiB); the gather of their {N * TEXT >> 20} MiB {t_ga:.1f} us", flush=True)
            if size == TEXT:
                # the calls behind it, over the same segments
                o = outs[0]
                se = [batch.prepare_call(
                    "sccsum_tcp_send", ctypes.addressof(send_opts), staging, lay_bytes, o["off"], o["len"], o["out"], N,
                    empty(N, torch.int64), empty(N, torch.int32), q["sum_len"], q["seed"], empty(N, torch.int16), empty(N),
                    empty(N), empty(N)) for q in [dict(sum_len=empty(N, torch.int32), seed=empty(N, torch.int32))
                                                 for _ in range(SETS)]]
                t_se = report(f"sccsum_tcp_send conns={nconns}", s, se, reps, N, "segments")
                t = batch.tcp_send(batch.PacketBatch(data=staging, off=o["off"], length=o["len"], bytes_len=lay_bytes,
                                                     max_len=TEXT), o["out"].view(torch.uint8).view(-1, 24), HOST, MTU)
                sp = [batch.prepare_call("sccsum_spans", staging, lay_bytes, t.sum_batch.off, t.sum_batch.length, t.seeds,
                                         empty(N, torch.int16), None, N, TEXT + 20) for _ in range(SETS)]
                t_sp = report(f"sccsum_spans conns={nconns}", s, sp, reps, N, "segments")
                print(f"tx: tcp_tx_data {t_cut:.1f} us next to tcp_send {t_se:.1f} us ({100 * t_cut / t_se:.1f} %) and the "
                      f"checksum pass {t_sp:.1f} us ({100 * t_cut / t_sp:.1f} %) over the same {N} segments", flush=True)
                del se, sp, t
            del calls, ga, outs, d_first, d_len, d_src
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
