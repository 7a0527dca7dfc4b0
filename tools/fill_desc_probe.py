"""Fill against verify on the same fragment lists, kernel alone:
sccsum_ipv4_fill_desc (FILL_IP | FILL_L4: generate and store where the
fragments lie) and sccsum_ipv4_frames_desc (values only) on the same
descriptors, alternating, one timed launch each per repetition.  1500 B UDP
frames, one per 2304-byte mbuf slot at +256 ("slots", one fragment per packet)
or as the L4 writers build them ("3frag": a 40 B header fragment from a header
area + two 730 B payload fragments of the slot), in HBM and in a pinned host
pool.  Every timed launch follows a 256 MiB device read that evicts the L2s
(tools/desc_probe.py).  Prints the median of each call, the fill / verify
ratio and the spread of the verify's own repetitions.

usage: python tools/fill_desc_probe.py [packets] [reps]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seastar_amd import batch, native, pipeline, synth


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    lib = native.load()
    native.check(lib.sccsum_init(0), "sccsum_init")
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream()
    mode = native.FILL_IP | native.FILL_L4
    flush = torch.ones(64 << 20, dtype=torch.float32, device=dev)
    frames = synth.udp_ipv4_frames(min(n, 4096), 1500, seed=9)[0].reshape(-1, 1500)
    lens = np.full(n, 1500, np.uint32)
    lay = np.arange(n, dtype=np.uint64) * 1504
    hdr_area = n * 64
    slot = hdr_area + np.arange(n, dtype=np.uint64) * 2304 + 256
    pool_len = hdr_area + n * 2304 + 64
    image = np.zeros(pool_len, np.uint8)
    pieces = {"slots": [(0, 1500, slot)],
              "3frag": [(0, 40, np.arange(n, dtype=np.uint64) * 64), (40, 730, slot), (770, 730, slot + 1024)]}
    for where in ("hbm", "pinned"):
        for layout, parts in pieces.items():
            for a, ln, at in parts:
                for i in range(n):
                    image[int(at[i]):int(at[i]) + ln] = frames[i % frames.shape[0], a:a + ln]
            if where == "pinned":
                pool = pipeline.pinned_empty(pool_len)
                pool[:] = image
                base = pool.ctypes.data
            else:
                pool = torch.from_numpy(image).to(dev)
                base = pool.data_ptr()
            k = len(parts)
            src = np.stack([base + at for _, _, at in parts], axis=1).reshape(-1)
            dst = np.stack([lay + a for a, _, _ in parts], axis=1).reshape(-1)
            ln = np.tile(np.array([p[1] for p in parts], np.uint32), n)
            desc = batch.make_desc(src, dst, ln)
            d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
            d_first = torch.from_numpy(np.arange(n + 1, dtype=np.int32) * k).to(dev)
            d_off = torch.from_numpy(lay.view(np.int64)).to(dev)
            d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
            out = torch.empty(2 * n, dtype=torch.int16, device=dev)

            def fill():
                batch.ipv4_fill_desc(d_desc, d_first, d_off, d_len, 1500, mode, out2=out, stream=s)

            def verify():
                batch.ipv4_frames_desc(d_desc, d_first, d_off, d_len, 1500, out2=out, stream=s)

            calls = (("fill", fill), ("verify", verify))
            for _, fn in calls:
                for _ in range(3):
                    fn()
            us = {name: [] for name, _ in calls}
            for _ in range(reps):
                for name, fn in calls:  # alternating, each after an eviction of the L2s
                    with torch.cuda.stream(s):
                        flush.sum()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    fn()
                    e1.record(s)
                    e1.synchronize()
                    us[name].append(e0.elapsed_time(e1) * 1e3)
            f, v = np.array(us["fill"]), np.array(us["verify"])
            mf, mv = float(np.median(f)), float(np.median(v))
            nbytes = int(lens.sum())
            print(f"{layout:>5} in {where:>6} n={n} reps={reps}: fill {mf:7.1f} us ({nbytes / mf / 1e3:6.1f} GB/s)   "
                  f"verify {mv:7.1f} us ({nbytes / mv / 1e3:6.1f} GB/s)   fill/verify {mf / mv:5.3f}   "
                  f"verify spread min {v.min():.1f} max {v.max():.1f} us ({(v.max() - v.min()) / mv * 100:.1f} % of "
                  f"the median; fill min {f.min():.1f} max {f.max():.1f})", flush=True)


if __name__ == "__main__":
    main()
