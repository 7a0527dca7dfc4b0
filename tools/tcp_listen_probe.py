"""The TCP passive open timed on rx batches of SYNs, next to the calls in front
of it on the same box:
  1 048 576 wire frames of 62 bytes in 2 304-byte slots (IPv4 / TCP SYNs with an
  MSS and a window-scale option; frame i comes from peer i mod 4 096 and source
  port 1 024 + i div 4 096, so every frame is its own connid):
    sccsum_ipv4_frames_rss    the pass over the frames' L3 parts
    sccsum_tcp_rx             no connection, the ports listening: all LISTEN
    sccsum_tcp_listen         one listening port with ample room
                              256 listening ports
                              one port whose room ends after 1 % of the batch
                              (the flood: almost all answered with a RST)
                              the second frame repeating the first connid
                              (taken = 1: what refusing the batch costs)
Every call is timed alone by stream events after a warm-up and reported as
the median of `reps` runs; outputs rotate over two sets.

usage: python tools/tcp_listen_probe.py [reps]
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

FRAME = 14 + 20 + 28
AMPLE = 1 << 30


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    lib = native.load()
    native.check(lib.sccsum_init(0), "sccsum_init")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    print(f"box: {torch.cuda.get_device_name(0)}, {N} SYN frames of {FRAME} B in {SLOT} B slots, {PEERS} peers", flush=True)

    def empty(numel, dtype=torch.uint8):
        return torch.empty(numel, dtype=dtype, device=dev)

    wire = wire_batch(dev)
    wire.length.fill_(FRAME)
    wire.max_len = FRAME
    view = wire.data[: N * SLOT].view(N, SLOT)
    idx = torch.arange(N, device=dev)
    view[:, 14 + 2], view[:, 14 + 3] = 0, FRAME - 14            # the IP length
    view[:, 14 + 9] = 6
    sport = 1024 + idx // PEERS
    view[:, 14 + 20], view[:, 14 + 21] = (sport >> 8).to(torch.uint8), (sport & 0xFF).to(torch.uint8)
    view[:, 14 + 24:14 + 40] = 0
    for k in range(4):
        view[:, 14 + 24 + k] = ((idx >> (24 - 8 * k)) & 0xFF).to(torch.uint8)   # SEG.SEQ
    view[:, 14 + 32], view[:, 14 + 33] = 0x70, 0x02              # data_offset 7, SYN
    view[:, 14 + 34], view[:, 14 + 35] = 0x20, 0x00
    view[:, 14 + 40:14 + 48] = torch.tensor([2, 4, 0x05, 0xB4, 3, 3, 7, 1], dtype=torch.uint8, device=dev)
    ip = batch.eth_rx(wire, (0x0800, 0x0806)).bucket(0)
    key = (ctypes.c_uint8 * 40)(*batch.RSS_KEY_40)
    status = [empty(N) for _ in range(SETS)]
    opts = native.TcpListenOpts((ctypes.c_uint32 * 16)(*range(1, 17)), 123456789, 1500, 0)
    ws = int(lib.sccsum_tcp_listen_workspace(N))
    print(f"sccsum_tcp_listen_workspace({N}) = {ws >> 20} MiB", flush=True)

    def ports(nports: int):
        dport = 2000 + (idx * 7) % nports
        view[:, 14 + 22], view[:, 14 + 23] = (dport >> 8).to(torch.uint8), (dport & 0xFF).to(torch.uint8)
        view[:, 14 + 10:14 + 12] = 0                            # the fill generates over zero fields
        view[:, 14 + 36:14 + 38] = 0
        batch.ipv4_fill(ip)
        torch.cuda.synchronize()                                # the timed calls run on a stream of their own

    def rx_outputs():
        return [dict(first=empty(5, torch.int32), total=empty(4, torch.int64), order=empty(N, torch.int32),
                     seg=empty(4 * N, torch.int64), src=empty(N, torch.int32)) for _ in range(SETS)]

    def tcp_rx_calls(t, rx):
        return [batch.prepare_call(
            "sccsum_tcp_rx", wire.data, wire.bytes_len, ip.off, ip.length, N, status[0], batch.TCP_NEED, batch.TCP_REJECT,
            HOST, t.handle, None, N, 0, empty(N), o["first"], o["order"], o["seg"], o["src"], empty(2, torch.int32),
            empty(2, torch.int32), empty(5 * N, torch.int32), empty(N, torch.int32), o["total"],
            empty(int(lib.sccsum_tcp_rx_workspace(N, 0)))) for o in rx]

    def listen(name: str, rx, space: torch.Tensor, want):
        outs = [dict(cls=empty(N), rec=empty(8 * N, torch.int64), synack=empty(8 * N, torch.int32),
                     sa_off=empty(N, torch.int64), sa_len=empty(N, torch.int32), sa_out=empty(6 * N, torch.int32),
                     rst=empty(5 * N, torch.int32), rst_dst=empty(N, torch.int32), total=empty(4, torch.int64))
                for _ in range(SETS)]
        calls = [batch.prepare_call(
            "sccsum_tcp_listen", opts, wire.data, wire.bytes_len, ip.off, N, o["first"], o["order"], o["seg"], o["src"], N,
            space, q["cls"], q["rec"], q["synack"], q["sa_off"], q["sa_len"], q["sa_out"], q["rst"], q["rst_dst"],
            q["total"], empty(ws)) for o, q in zip(rx, outs)]
        t = report(f"sccsum_tcp_listen {name}", s, calls, reps, N, "SYNs")
        total = outs[0]["total"].cpu().tolist()
        assert total == want, (total, want)
        return t, total

    def space_of(room: dict) -> torch.Tensor:
        a = np.zeros(65536, dtype=np.int32)
        for p, r in room.items():
            a[p] = r
        return torch.from_numpy(a).to(dev)

    # one listening port
    ports(1)
    fr_calls = [batch.prepare_call(
        "sccsum_ipv4_frames_rss", wire.data, wire.bytes_len, ip.off, ip.length, empty(2 * N, torch.int16), status[k],
        N, FRAME - 14, ctypes.addressof(key), 40, native.RSS_DISPATCH, empty(N, torch.int32)) for k in range(SETS)]
    t_fr = report("sccsum_ipv4_frames_rss TCP", s, fr_calls, reps, N, "frames")
    assert bool(torch.all((status[0] & (native.ST_OK | native.ST_L4_OK)) == 3))
    t = batch.TcpConns((), (2000,))
    rx = rx_outputs()
    t_rx = report("sccsum_tcp_rx listen", s, tcp_rx_calls(t, rx), reps, N, "frames")
    assert rx[0]["first"].cpu().tolist() == [0, 0, N, N, N]
    t_one, _ = listen("1 port", rx, space_of({2000: AMPLE}), [N, N, 0, 0])
    room = N // 100
    t_flood, _ = listen("1 port, 1 % room", rx, space_of({2000: room}), [N, room, N - room, 0])
    t.close()
    print(f"rx: tcp_listen {t_one:.1f} us with room for all ({1e3 * t_one / N:.2f} ns a SYN), {t_flood:.1f} us with room for "
          f"1 % (the rest answered with a RST), next to tcp_rx {t_rx:.1f} us and frames_rss {t_fr:.1f} us", flush=True)

    # the second frame repeats the first connid
    keep = view[1, :FRAME].clone()
    view[1, :FRAME] = view[0, :FRAME]
    torch.cuda.synchronize()
    t = batch.TcpConns((), (2000,))
    for call in tcp_rx_calls(t, rx):
        call(s)
    s.synchronize()
    t_stop, _ = listen("taken = 1", rx, space_of({2000: AMPLE}), [1, 1, 0, 0])
    t.close()
    view[1, :FRAME] = keep
    torch.cuda.synchronize()
    print(f"rx: tcp_listen {t_stop:.1f} us when the second segment repeats the first connid (one connection made, the rest "
          f"left to the host)", flush=True)

    # 256 listening ports
    ports(256)
    for call in fr_calls:
        call(s)
    t = batch.TcpConns((), tuple(range(2000, 2256)))
    for call in tcp_rx_calls(t, rx):
        call(s)
    s.synchronize()
    assert rx[0]["first"].cpu().tolist() == [0, 0, N, N, N]
    t_many, _ = listen("256 ports", rx, space_of({p: AMPLE for p in range(2000, 2256)}), [N, N, 0, 0])
    t.close()
    print(f"rx: tcp_listen {t_many:.1f} us with 256 listening ports", flush=True)


if __name__ == "__main__":
    main()
