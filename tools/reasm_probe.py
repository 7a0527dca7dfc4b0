"""Rx reassembly (sccsum_ipv4_frag_records + sccsum_ipv4_reasm) timed next to
the frames pass over the same frames (sccsum_ipv4_frames_rss), on three shapes:
  pairs   1 048 576 fragments: 524 288 datagrams of 2 fragments (24 + 16 bytes)
  jumbo   65 536 datagrams of 65 507 bytes in 45 fragments each, as ipv4::send
          cuts them at mtu 1500 (2 949 120 frames, 4.4 GB)
  whole   1 048 576 whole datagrams, no fragment at all: the records call finds
          none and the reassembly call has nothing to do
The frames are built on the device (headers with valid checksums, payload as
allocated) and arrive in a random order.  Every call is timed alone by stream
events after a warm-up; the counts each call reports are checked.

usage: python tools/reasm_probe.py [reps]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seastar_amd import batch, native

HOST = 0x0A000002
KEY = batch.RSS_KEY_40


def timed(s, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def headers(dev, total_len, ident, frag, src):
    """[n, 20] IPv4/UDP headers to HOST with their checksums (int64 columns in)."""
    n = total_len.numel()
    h = torch.zeros((n, 20), dtype=torch.int64, device=dev)
    h[:, 0], h[:, 8], h[:, 9] = 0x45, 64, 17
    for col, v in ((2, total_len), (4, ident), (6, frag)):
        h[:, col], h[:, col + 1] = v >> 8, v & 0xFF
    for k in range(4):
        h[:, 12 + k] = (src >> (24 - 8 * k)) & 0xFF
        h[:, 16 + k] = (HOST >> (24 - 8 * k)) & 0xFF
    s = (h[:, 0::2] * 256 + h[:, 1::2]).sum(dim=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    c = ~s & 0xFFFF
    h[:, 10], h[:, 11] = c >> 8, c & 0xFF
    return h.to(torch.uint8)


def make(dev, dgrams, pieces, piece, last, pitch):
    """dgrams datagrams of `pieces` fragments (piece bytes each, the last `last`)
    as frames at one pitch, in a random arrival order."""
    n = dgrams * pieces
    d = torch.arange(n, dtype=torch.int64, device=dev) // pieces
    j = torch.arange(n, dtype=torch.int64, device=dev) % pieces
    is_last = j == pieces - 1
    pay = torch.where(is_last, torch.full_like(j, last), torch.full_like(j, piece))
    frag = torch.where(is_last, torch.zeros_like(j), torch.full_like(j, 0x2000)) | (j * piece // 8)
    if pieces == 1:
        frag = torch.zeros_like(j)
    data = torch.empty(n * pitch + 16, dtype=torch.uint8, device=dev)
    data[: n * pitch].view(n, pitch)[:, :20] = headers(dev, pay + 20, d & 0xFFFF, frag, 0x0B000000 + (d >> 16))
    perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(10))
    return batch.PacketBatch(data=data, off=(perm * pitch).contiguous(), length=(pay[perm] + 20).to(torch.int32),
                             bytes_len=n * pitch, max_len=piece + 20)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    lib = native.load()
    native.check(lib.sccsum_init(0), "sccsum_init")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    kb = (ctypes.c_uint8 * len(KEY)).from_buffer_copy(KEY)
    shapes = (("pairs", 1 << 19, 2, 24, 16, 48), ("jumbo", 1 << 16, 45, 1480, 65507 - 44 * 1480, 1500),
              ("whole", 1 << 20, 1, 24, 24, 48))
    for name, dgrams, pieces, piece, last, pitch in shapes:
        with torch.cuda.stream(s):
            b = make(dev, dgrams, pieces, piece, last, pitch)
            n = b.n
            status = torch.empty(n, dtype=torch.uint8, device=dev)
            hashes = torch.empty(n, dtype=torch.int32, device=dev)
            rec = torch.empty(32 * n, dtype=torch.uint8, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            ws = torch.empty(int(lib.sccsum_ipv4_reasm_workspace(n)), dtype=torch.uint8, device=dev)
            o = dict(desc=torch.empty(16 * n, dtype=torch.uint8, device=dev),
                     first=torch.empty(n + 1, dtype=torch.int32, device=dev),
                     off=torch.empty(n, dtype=torch.int64, device=dev),
                     **{k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("len", "seed", "head", "last", "hash")},
                     pending=torch.empty(32 * n, dtype=torch.uint8, device=dev),
                     host=torch.empty(32 * n, dtype=torch.uint8, device=dev),
                     state=torch.empty(n, dtype=torch.uint8, device=dev),
                     total=torch.empty(4, dtype=torch.int64, device=dev))
        out = native.ReasmOut(*[o[k].data_ptr() for k in ("desc", "first", "off", "len", "seed", "head", "last", "hash",
                                                          "pending", "host", "state", "total")])
        st = s.cuda_stream

        def frames_rss():
            native.check(lib.sccsum_ipv4_frames_rss(b.data.data_ptr(), b.bytes_len, b.off.data_ptr(),
                                                    b.length.data_ptr(), None, status.data_ptr(), n, b.max_len,
                                                    ctypes.addressof(kb), len(KEY), native.RSS_DISPATCH,
                                                    hashes.data_ptr(), st), "sccsum_ipv4_frames_rss")

        def records():
            native.check(lib.sccsum_ipv4_frag_records(b.data.data_ptr(), b.bytes_len, b.off.data_ptr(),
                                                      b.length.data_ptr(), status.data_ptr(), batch.FRAG_NEED,
                                                      batch.FRAG_REJECT, n, HOST, 1, rec.data_ptr(), count.data_ptr(),
                                                      ws.data_ptr(), st), "sccsum_ipv4_frag_records")

        frames_rss()
        records()
        s.synchronize()
        m = int(count.item())
        assert m == (n if pieces > 1 else 0), (m, n)

        def reasm():
            native.check(lib.sccsum_ipv4_reasm(rec.data_ptr() if m else None, m, 0xFFFFFFFF, ctypes.addressof(kb),
                                               len(KEY), ctypes.addressof(out), ws.data_ptr(), st), "sccsum_ipv4_reasm")

        reasm()
        s.synchronize()
        # every key is complete; two keys that share the 32-bit mix (a few among 2^19 keys of several
        # sources) are in the host bucket whole
        got = o["total"].cpu().numpy().tolist()
        assert got[2] == 0 and got[0] * pieces == got[1] and got[1] + got[3] == m, got
        assert got[3] <= m // 1000 and (got[3] == 0 or name == "pairs"), got
        t = {f.__name__: np.array([timed(s, f) for _ in range(reps)]) for f in (frames_rss, records, reasm)}
        assert o["total"].cpu().numpy().tolist() == got
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(f"reasm {name}: {n} frames ({b.bytes_len / 1e6:.0f} MB), {m} records, {got[0]} datagrams of {pieces} "
              f"fragment(s) + {got[3]} records to the host: frames_rss {med['frames_rss']:8.1f} us, "
              f"frag_records {med['records']:7.1f} us "
              f"(min {t['records'].min():.1f} max {t['records'].max():.1f}), reasm {med['reasm']:8.1f} us "
              f"(min {t['reasm'].min():.1f} max {t['reasm'].max():.1f}, reps {reps})"
              + (f" = {m / med['reasm']:6.1f} records/us" if m else ""), flush=True)
        del b, rec, ws, o
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
