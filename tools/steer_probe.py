"""Rx steering against the frames pass that feeds it, same process, same box:
sccsum_steer_run (count, scan, scatter: three launches) on 1 048 576 hashes,
ncpu 16 and 255, with and without a status array (about 10 % dropped), and
sccsum_ipv4_frames_rss on a batch of as many 1500-byte frames.

Inputs are rotated: each timed call takes the next of `sets` input / output
sets (the frames pass alternates two 1.5 GB batches), so no call finds its
own last run's lines in the L2s.  Every call is timed alone by stream events
after a warm-up of every shape; "chain" is the time per call of 16 calls
queued back to back (what a shard that steers batch after batch pays, the
host's enqueue hidden behind the device).  Prints the median, the minimum
and the maximum of each, and the steer / frames_rss ratio.

usage: python tools/steer_probe.py [packets] [reps] [sets]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seastar_amd import batch, devsynth, native


def timed(s, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    sets = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    lib = native.load()
    native.check(lib.sccsum_init(0), "sccsum_init")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    g = torch.Generator(device=dev)
    g.manual_seed(5)

    frames = [devsynth.udp_frames(n, 1500, seed=11 + k, device=dev) for k in range(2)]
    f_out = [(torch.empty(2 * n, dtype=torch.int16, device=dev), torch.empty(n, dtype=torch.uint8, device=dev),
              torch.empty(n, dtype=torch.int32, device=dev)) for _ in range(2)]

    def frames_rss(k):
        out2, st, h = f_out[k % 2]
        batch.ipv4_frames_rss(frames[k % 2], out2=out2, status=st, hash_out=h, stream=s)

    for k in range(4):
        frames_rss(k)
    s.synchronize()
    fr = np.array([timed(s, lambda k=k: frames_rss(k)) for k in range(reps)])
    mfr = float(np.median(fr))
    print(f"frames_rss n={n} x 1500 B: median {mfr:7.1f} us (min {fr.min():.1f} max {fr.max():.1f}, reps {reps})",
          flush=True)

    # set 0 steers the hashes the frames pass wrote; the others are random
    hashes = [f_out[0][2]] + [(torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device=dev, generator=g)
                               - (1 << 31)).to(torch.int32) for _ in range(sets - 1)]
    r = torch.rand(n, device=dev, generator=g)
    st0 = torch.where(r < 0.1, 0, native.ST_OK | native.ST_L4_OK).to(torch.uint8)
    status = [st0.roll(k * 977) for k in range(sets)]
    for ncpu in (16, 255):
        reta = np.stack([batch.build_reta({c: 1.0 for c in range(ncpu)}) for _ in range(8)])
        for q in range(8):
            reta[q] = np.roll(reta[q], 16 * q)
        st = batch.Steer(ncpu, reta, hw_queues=8)
        outs = [(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                 torch.empty(ncpu + 2, dtype=torch.int32, device=dev),
                 torch.empty(st.workspace_bytes(n), dtype=torch.uint8, device=dev)) for _ in range(sets)]
        for with_status in (False, True):
            for order_too in (True, False):

                def run(k):
                    cpu, order, first, ws = outs[k % sets]
                    if with_status:
                        st.run(hashes[k % sets], status[k % sets], need=native.ST_OK,
                               reject=native.ST_MALFORMED | native.ST_RANGE, cpu=cpu, order=order if order_too else None,
                               first=first, workspace=ws, stream=s, want_order=order_too)
                    else:
                        st.run(hashes[k % sets], cpu=cpu, order=order if order_too else None, first=first,
                               workspace=ws, stream=s, want_order=order_too)

                for k in range(sets):
                    run(k)
                s.synchronize()
                one = np.array([timed(s, lambda k=k: run(k)) for k in range(reps)])

                def chain(k0):
                    for k in range(16):
                        run(k0 + k)

                ch = np.array([timed(s, lambda k=k: chain(16 * k)) for k in range(max(reps // 4, 4))]) / 16
                m1, mc = float(np.median(one)), float(np.median(ch))
                what = "cpu+order+first" if order_too else "cpu+first (no scatter)"
                print(f"steer ncpu={ncpu:3d} status={'yes' if with_status else 'no ':3} {what:22}: one call median "
                      f"{m1:6.1f} us (min {one.min():.1f} max {one.max():.1f})   chain {mc:6.1f} us/call (min "
                      f"{ch.min():.1f} max {ch.max():.1f})   one call / frames_rss {m1 / mfr * 100:5.1f} %   chain / "
                      f"frames_rss {mc / mfr * 100:5.1f} %", flush=True)
        first = outs[0][2].cpu().numpy()
        print(f"  ncpu={ncpu}: last first[] ends at {first[-1]} (n={n}), dropped {first[-1] - first[-2]}", flush=True)
        st.close()


if __name__ == "__main__":
    main()
