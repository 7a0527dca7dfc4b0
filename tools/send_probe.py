"""Tx send (sccsum_ipv4_send: count, scan, place, emit — four launches) timed
on two shapes at mtu 1500:
  small   1 048 576 datagrams of 1 472 bytes: one frame each
  large   65 536 datagrams of 65 507 bytes: 45 frames each.  Their packed layout
          is 4.35 GB, past the 2^32 - 1 bytes one call's 32-bit descriptor
          offsets reach, so the shape runs as two calls of 32 768 datagrams
          queued back to back and the pair is timed.
The kernels read no payload byte, so the datagram buffer is left as allocated.

Outputs are rotated: each timed run takes the next of `sets` output sets, so no
run finds its own last run's lines in the L2s.  Every run is timed alone by
stream events after a warm-up; "chain" is the time per run of 8 runs queued
back to back.  The rate is against the bytes the kernels must move: 19 bytes
read per datagram (offset, length, destination, protocol, id) + 68 bytes
written per frame (header 20, two descriptors 32, d_first 4, d_out_off 8,
d_out_len 4).

usage: python tools/send_probe.py [reps] [sets]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seastar_amd import batch, native

MTU = 1500
SRC = 0x0A000001


def timed(s, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def shape(lib, dev, n, l4_len, calls, sets, opts):
    """`calls` prepared launches per output set over n datagrams of l4_len bytes
    in all; returns (run(k), frames of a run, check())."""
    per = n // calls
    nf, nb = ctypes.c_uint32(), ctypes.c_uint64()
    native.check(lib.sccsum_ipv4_send_plan(ctypes.addressof(opts), l4_len, 17, ctypes.byref(nf), ctypes.byref(nb)),
                 "sccsum_ipv4_send_plan")
    frames, nbytes = per * nf.value, per * nb.value
    assert nbytes <= 0xFFFFFFFF
    data = torch.empty(n * l4_len + 16, dtype=torch.uint8, device=dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * l4_len
    length = torch.full((n,), l4_len, dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    dst = (torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device=dev, generator=g) - (1 << 31)).to(torch.int32)
    proto = torch.full((n,), 17, dtype=torch.uint8, device=dev)
    ids = torch.arange(n, dtype=torch.int32, device=dev).to(torch.int16)
    launches, totals = [], []
    for _ in range(sets):
        row = []
        for c in range(calls):
            lo = c * per
            out = dict(hdr=torch.empty(20 * frames, dtype=torch.uint8, device=dev),
                       desc=torch.empty(32 * frames, dtype=torch.uint8, device=dev),
                       first=torch.empty(frames + 1, dtype=torch.int32, device=dev),
                       out_off=torch.empty(frames, dtype=torch.int64, device=dev),
                       out_len=torch.empty(frames, dtype=torch.int32, device=dev),
                       dgram_first=torch.empty(per + 1, dtype=torch.int32, device=dev),
                       status=torch.empty(per, dtype=torch.uint8, device=dev),
                       total=torch.empty(3, dtype=torch.int64, device=dev),
                       ws=torch.empty(int(lib.sccsum_ipv4_send_workspace(per)), dtype=torch.uint8, device=dev))
            row.append(batch.prepare_call(
                "sccsum_ipv4_send", ctypes.addressof(opts), data, n * l4_len, off[lo:lo + per], length[lo:lo + per],
                dst[lo:lo + per], proto[lo:lo + per], ids[lo:lo + per], None, per, frames, nbytes, out["hdr"],
                out["desc"], out["first"], out["out_off"], out["out_len"], out["dgram_first"], out["status"],
                out["total"], out["ws"]))
            totals.append(out["total"])
        launches.append(row)

    def run(s, k):
        for launch in launches[k % sets]:
            launch(s)

    def check():
        for t in totals:
            assert t.cpu().numpy().tolist() == [frames, nbytes, per], t
    return run, calls * frames, check


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    sets = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    lib = native.load()
    native.check(lib.sccsum_init(0), "sccsum_init")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    opts = native.SendOpts(SRC, MTU, 0)
    for name, n, l4_len, calls in (("small", 1 << 20, 1472, 1), ("large", 1 << 16, 65507, 2)):
        run, frames, check = shape(lib, dev, n, l4_len, calls, sets, opts)
        for k in range(2 * sets):
            run(s, k)
        s.synchronize()
        check()
        one = np.array([timed(s, lambda k=k: run(s, k)) for k in range(reps)])

        def chain(k0):
            for k in range(8):
                run(s, k0 + k)

        ch = np.array([timed(s, lambda k=k: chain(8 * k)) for k in range(max(reps // 4, 4))]) / 8
        check()
        moved = 19 * n + 68 * frames
        m1, mc = float(np.median(one)), float(np.median(ch))
        print(f"send {name}: {n} datagrams x {l4_len} B, mtu {MTU}, {frames} frames, {calls} call(s) a run, "
              f"{moved / 1e6:.1f} MB to move: one run median {m1:7.1f} us (min {one.min():.1f} max {one.max():.1f}, "
              f"reps {reps}) = {moved / m1 / 1e3:6.1f} GB/s, {frames / m1:6.1f} frames/us;   chain {mc:7.1f} us/run "
              f"(min {ch.min():.1f} max {ch.max():.1f}) = {moved / mc / 1e3:6.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
