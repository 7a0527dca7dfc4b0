"""The link layer's three device calls timed on the shapes of a full rx / tx
batch, next to the calls they sit in front of and behind:
  rx   1 048 576 wire frames of 1 514 bytes in 2 304-byte slots (IPv4 / UDP from
       4 096 peers of the host's subnet):
         sccsum_eth_rx             count, scan, scatter
         sccsum_ipv4_frames_rss    the pass over the same frames' L3 parts
         sccsum_arp_learn_records  steady state: the table knows every peer
  tx   1 048 576 UDP datagrams of 1 472 bytes to those peers at mtu 1500:
         sccsum_ipv4_send          one frame each
         sccsum_eth_send           on send's lists, a 4 096-entry table
Every call is timed alone by stream events after a warm-up and reported as
the median of `reps` runs; outputs rotate over two sets.

usage: python tools/eth_probe.py [reps]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seastar_amd import batch, native

N = 1 << 20
SLOT, FRAME, L4 = 2304, 1514, 1472
PEERS = 4096
HOST, NETMASK, GW = 0x0A000001, 0xFFFF0000, 0x0A0000FE
HW = 0x02AB12CD34EF
SETS = 2


def timed(s, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def report(name, s, launches, reps, items, what):
    for k in range(2 * SETS):
        launches[k % SETS](s)
    s.synchronize()
    t = np.array([timed(s, lambda k=k: launches[k % SETS](s)) for k in range(reps)])
    m = float(np.median(t))
    print(f"{name:26s} {items} {what}: median {m:8.1f} us (min {t.min():.1f} max {t.max():.1f}, reps {reps}) = "
          f"{items / m:7.1f} {what}/us", flush=True)
    return m


def peer_ips():
    return 0x0A000100 + np.arange(PEERS, dtype=np.int64)


def peer_macs():
    return 0x020000000000 + peer_ips() * 0x10003 % (1 << 40)


def wire_batch(dev):
    """The rx frames, built on the device: one template frame in every slot,
    each with its peer's source MAC and address."""
    hdr = np.zeros(FRAME, dtype=np.uint8)
    hdr[0:6] = list(HW.to_bytes(6, "big"))
    hdr[12:14] = [0x08, 0x00]
    ip = hdr[14:]
    ip[0], ip[2:4], ip[8], ip[9] = 0x45, [(FRAME - 14) >> 8, (FRAME - 14) & 0xFF], 64, 17
    ip[16:20] = list(HOST.to_bytes(4, "big"))
    ip[20:28] = [0x04, 0xD2, 0x16, 0x2E, (L4 >> 8), L4 & 0xFF, 0, 0]
    data = torch.zeros(N * SLOT + 16, dtype=torch.uint8, device=dev)
    view = data[: N * SLOT].view(N, SLOT)
    view[:, :FRAME] = torch.from_numpy(hdr).to(dev)
    who = torch.arange(N, device=dev) % PEERS
    ips = torch.from_numpy(peer_ips()).to(dev)[who]
    macs = torch.from_numpy(peer_macs()).to(dev)[who]
    for k in range(6):
        view[:, 6 + k] = ((macs >> (40 - 8 * k)) & 0xFF).to(torch.uint8)
    for k in range(4):
        view[:, 26 + k] = ((ips >> (24 - 8 * k)) & 0xFF).to(torch.uint8)
    off = torch.arange(N, dtype=torch.int64, device=dev) * SLOT
    length = torch.full((N,), FRAME, dtype=torch.int32, device=dev)
    return batch.PacketBatch(data=data, off=off, length=length, bytes_len=N * SLOT, max_len=FRAME)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    lib = native.load()
    native.check(lib.sccsum_init(0), "sccsum_init")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    print(f"box: {torch.cuda.get_device_name(0)}, {N} frames of {FRAME} B in {SLOT} B slots, {PEERS} peers", flush=True)
    table = batch.ArpTable(dict(zip(peer_ips().tolist(), peer_macs().tolist())))

    def empty(numel, dtype=torch.uint8):
        return torch.empty(numel, dtype=dtype, device=dev)

    # ---- rx
    wire = wire_batch(dev)
    rx = batch.eth_rx(wire, (0x0800, 0x0806))
    assert rx.bounds().tolist() == [0, N, N, N]
    ip = rx.bucket(0)
    batch.ipv4_fill(ip)  # valid checksums, so that the frames pass takes its usual path
    protos = (ctypes.c_uint16 * 2)(0x0800, 0x0806)
    rx_calls = [batch.prepare_call(
        "sccsum_eth_rx", wire.data, wire.bytes_len, wire.off, wire.length, N, ctypes.addressof(protos), 2, empty(N),
        empty(4, torch.int32), empty(N, torch.int32), empty(N, torch.int64), empty(N, torch.int32),
        empty(N, torch.int64), empty(int(lib.sccsum_eth_rx_workspace(N)))) for _ in range(SETS)]
    t_rx = report("sccsum_eth_rx", s, rx_calls, reps, N, "frames")

    key = (ctypes.c_uint8 * 40)(*batch.RSS_KEY_40)
    status = [empty(N) for _ in range(SETS)]
    fr_calls = [batch.prepare_call(
        "sccsum_ipv4_frames_rss", wire.data, wire.bytes_len, ip.off, ip.length, empty(2 * N, torch.int16), status[k], N,
        FRAME - 14, ctypes.addressof(key), 40, native.RSS_DISPATCH, empty(N, torch.int32)) for k in range(SETS)]
    t_fr = report("sccsum_ipv4_frames_rss", s, fr_calls, reps, N, "frames")
    assert bool(torch.all((status[0] & native.ST_OK) != 0))

    counts = [empty(1, torch.int32) for _ in range(SETS)]
    ln_calls = [batch.prepare_call(
        "sccsum_arp_learn_records", wire.data, wire.bytes_len, ip.off, ip.length, status[k], native.ST_OK,
        native.ST_MALFORMED | native.ST_RANGE, rx.src_mac(0), N, HOST, NETMASK, table.handle, empty(16 * N), counts[k],
        empty(int(lib.sccsum_arp_learn_workspace(N)))) for k in range(SETS)]
    t_ln = report("sccsum_arp_learn_records", s, ln_calls, reps, N, "frames")
    assert int(counts[0].item()) == 0  # the steady state: nothing to learn
    print(f"rx: eth_rx + learn = {t_rx + t_ln:.1f} us next to frames_rss {t_fr:.1f} us "
          f"({100 * (t_rx + t_ln) / t_fr:.1f} %)", flush=True)
    del wire, rx, ip, rx_calls, fr_calls, ln_calls
    torch.cuda.empty_cache()

    # ---- tx
    l4 = batch.PacketBatch(data=empty(N * L4 + 16), off=torch.arange(N, dtype=torch.int64, device=dev) * L4,
                           length=torch.full((N,), L4, dtype=torch.int32, device=dev), bytes_len=N * L4, max_len=L4)
    dst = torch.from_numpy(peer_ips()).to(dev)[torch.arange(N, device=dev) % PEERS].to(torch.int32)
    proto = torch.full((N,), 17, dtype=torch.uint8, device=dev)
    r = batch.ipv4_send(l4, dst, proto, 1500, HOST)
    desc, first, off, length, _ = r.lists()
    frames = int(off.numel())
    assert frames == N
    nbytes = N * (L4 + 20)
    sopts = native.SendOpts(HOST, 1500, 0)
    sd_calls = [batch.prepare_call(
        "sccsum_ipv4_send", ctypes.addressof(sopts), l4.data, l4.bytes_len, l4.off, l4.length, dst, proto, None, None, N,
        N, nbytes, empty(20 * N), empty(32 * N), empty(N + 1, torch.int32), empty(N, torch.int64), empty(N, torch.int32),
        empty(N + 1, torch.int32), empty(N), empty(3, torch.int64), empty(int(lib.sccsum_ipv4_send_workspace(N))))
        for _ in range(SETS)]
    t_sd = report("sccsum_ipv4_send", s, sd_calls, reps, N, "frames")
    eopts = native.EthOpts(HW, HOST, NETMASK, GW, 0x0800)
    totals = [empty(6, torch.int64) for _ in range(SETS)]
    es_calls = [batch.prepare_call(
        "sccsum_eth_send", ctypes.addressof(eopts), table.handle, dst, r.dgram_first, N, desc, first, off, length, N,
        nbytes + 14 * N, empty(14 * N), empty(16 * 3 * N), empty(N + 1, torch.int32), empty(N, torch.int64),
        empty(N, torch.int32), empty(N, torch.int32), empty(N), empty(8 * N), totals[k],
        empty(int(lib.sccsum_eth_send_workspace(N)))) for k in range(SETS)]
    t_es = report("sccsum_eth_send", s, es_calls, reps, N, "frames")
    assert totals[0].cpu().numpy().tolist() == [N, nbytes + 14 * N, N, 0, N, 3 * N]
    print(f"tx: eth_send {t_es:.1f} us next to ipv4_send {t_sd:.1f} us ({100 * t_es / t_sd:.1f} %)", flush=True)


if __name__ == "__main__":
    main()
