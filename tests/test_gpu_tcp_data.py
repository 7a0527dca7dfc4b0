"""The TCP receive fast path on the device (sccsum_tcp_rx_data), compared with
the per-segment model (tests/tcp_data_model.py).  Every raw call writes into
outputs with guard words on both sides; every field of every run record,
every descriptor and d_total is compared; nothing has a tolerance."""
import copy
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import stack_model as sm
import tcp_data_model as dm
import tcp_data_traffic as tr
import tcp_model as tm
import tcp_traffic
from seastar_amd import batch, native
from test_gpu_eth import Out, _dev

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = tr.TILE
BASE = 0x7000_0000_1000        # d_bytes of the fabricated calls: an address, never read
M32 = 0xFFFFFFFF


def run_data(dev, a: dict, max_bytes: int = M32, shift: int = 0, base: int = BASE) -> dict:
    """sccsum_tcp_rx_data on arrays as tcp_rx leaves them (tcp_data_traffic.arrays) into guarded outputs."""
    lib = native.load()
    n, nconns = a["n"], a["nconns"]
    runs = min(n, nconns) + 1
    seg = _dev(dev, a["seg"].view(np.int64)) if n else None
    rcv = _dev(dev, a["rcv"].view(np.uint8))
    first = _dev(dev, a["first"].view(np.int32))
    run_conn = _dev(dev, np.concatenate([a["run_conn"], [0]]).astype(np.uint32).view(np.int32))
    run_first = _dev(dev, a["run_first"].view(np.int32))
    rx_total = _dev(dev, a["rx_total"].view(np.int64))
    run = Out(dev, 4 * runs, torch.int64, -7, shift)
    desc = Out(dev, 2 * n, torch.int64, -7, shift)
    total = Out(dev, 4, torch.int64, -7, shift)
    ws = Out(dev, int(lib.sccsum_tcp_rx_data_workspace(n, nconns)) // 16, torch.complex128, 3.0, shift)
    assert ws.ptr % 16 == 0 and rcv.data_ptr() % 16 == 0
    rc = lib.sccsum_tcp_rx_data(base, seg.data_ptr() if n else None, first.data_ptr(), run_conn.data_ptr(),
                                run_first.data_ptr(), rx_total.data_ptr(), n, rcv.data_ptr() if nconns else None, nconns,
                                max_bytes, run.ptr, desc.ptr if n else None, total.ptr, ws.ptr,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.host()
    t = total.host().view(np.uint64)
    r = int(a["rx_total"][0])
    assert int(t[0]) <= n
    return dict(run=run.host(4 * r).view(tr.RUN_DTYPE), desc=desc.host(2 * int(t[0])).view(tr.DESC_DTYPE), total=t)


def check(got: dict, want: dict, what="") -> None:
    assert got["total"].tolist() == want["total"].tolist(), what
    for name in tr.RUN_DTYPE.names:
        if name != "pad":
            bad = np.flatnonzero(got["run"][name] != want["run"][name])
            assert bad.size == 0, (what, name, bad[:5], got["run"][bad[:5]], want["run"][bad[:5]])
    assert got["desc"].tobytes() == want["desc"].tobytes(), what


@functools.lru_cache(maxsize=None)
def _mixed(n: int):
    cases = tr.mixed(n % 5, n)
    return cases, tr.arrays(cases), tr.expect(cases, base=BASE)


SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 7]


@pytest.mark.parametrize("n", SIZES)
def test_mixed_runs_against_the_model(dev, n):
    """n segments of bucket 0 (and five of the other buckets behind them): sizes around the wave and the tile."""
    cases, a, want = _mixed(n)
    assert a["n0"] == n
    got = run_data(dev, a)
    check(got, want)
    if n == 2 * TILE + 7:      # the traffic whose coverage tests/test_tcp_data_host.py checks
        assert 0.3 * n <= int(want["total"][0]) <= 0.9 * n
        assert len(set(want["run"]["stop"].tolist())) == 7


def test_bucket_zero_empty_and_no_connections(dev):
    a = tr.arrays([], others=9)
    got = run_data(dev, a)
    assert got["total"].tolist() == [0, 0, 0, 0] and got["run"].size == 0 and got["desc"].size == 0
    a = tr.arrays([], others=0)
    assert a["n"] == 0
    got = run_data(dev, a)
    assert got["total"].tolist() == [0, 0, 0, 0]


LONG = 3 * TILE + 5
SHAPES = {
    # one run over several tiles: never stopped, stopped in tile 0, in the last tile, at its last segment
    "one_straight": ([LONG], [None]),
    "one_stop_tile0": ([LONG], [100]),
    "one_stop_head": ([LONG], [0]),
    "one_stop_last_tile": ([LONG], [3 * TILE + 2]),
    "one_stop_last": ([LONG], [LONG - 1]),
    # runs that end exactly on a wave and on a tile boundary; heads in a tile's first and last lane
    "boundaries": ([64, 64, 896, 1, TILE - 1, TILE, 1, 2 * TILE - 2, 1, 64], [None, 63, None, None, 5, None, 0, None,
                                                                              None, 32]),
    # a stop in the first lane of a tile whose run began in an earlier tile; in the last lane of the tile before
    "first_lane": ([1000, 100, TILE, 900, 200], [None, 24, None, 100, 171]),
    "last_lane": ([1000, 100, 3000], [None, 23, 2 * TILE - 1 - 1100]),
    # a run that stops in one tile and spans three more, then short ones
    "stopped_across": ([10, 4 * TILE, 3, 3], [None, 5, None, 1]),
    "straight_across": ([10, 4 * TILE, 3, 3], [None, None, None, 1]),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_run_shapes_against_the_model(dev, name):
    lengths, stops = SHAPES[name]
    cases = tr.by_lengths(len(name), lengths, stops)
    a = tr.arrays(cases)
    want = tr.expect(cases, base=BASE)
    for r, at, length in zip(want["results"], stops, lengths):
        assert r.taken == (length if at is None else at), name      # the traffic stops where the shape says
    check(run_data(dev, a), want, name)


def test_every_segment_its_own_run(dev):
    """R = n: 1500 runs of one segment, every kind."""
    rng = np.random.default_rng(5)
    cases = [tr.stream(rng, 1, tr.KINDS[k % len(tr.KINDS)] if k % 2 else "none", 0, state=k) for k in range(1500)]
    a = tr.arrays(cases, spare=1, others=0)
    assert a["n"] == 1500 and a["rx_total"][0] == 1500
    want = tr.expect(cases, base=BASE)
    assert 300 < int(want["total"][0]) < 1400
    check(run_data(dev, a), want)


def test_sums_past_32_bits_do_not_wrap(dev):
    """65 537 records of 65 535 bytes (2^32 - 1 in all) against room = 2^30,
    and 65 540 of them: the sum of the run's lengths reaches and passes 2^32,
    where a 32-bit sum compared against room would find room again."""
    _past_32_bits(dev, 65537)
    _past_32_bits(dev, 65540)


def _past_32_bits(dev, count):
    rng = np.random.default_rng(11)
    t, segs = tr.stream(rng, count, lens=[65535] * count)
    assert t.room() == 1 << 30 and count * 65535 >= (1 << 32) - 1
    cases = [(t, segs), tr.stream(rng, 5)]
    a = tr.arrays(cases)
    want = tr.expect(cases, base=BASE)
    taken = -(-(1 << 30) // 65535)
    assert want["run"]["taken"].tolist() == [taken, 5] and want["run"]["stop"][0] == dm.STOP_WINDOW
    assert want["run"]["room"][0] == 0 and taken * 65535 > 1 << 30
    check(run_data(dev, a), want)
    # room above 2^30 is read as 2^30
    a["rcv"]["room"][a["run_conn"][0]] = 0xFFFFFFFF
    check(run_data(dev, a), want)


def test_capacity_cut(dev):
    """max_bytes at the first run, mid-way (in a run that begins in its tile and
    in one that came in from an earlier tile), exactly equal, one short, and 0."""
    cases = tr.by_lengths(3, [40, 3 * TILE, 30, 20, 500, 700, 9], [None, None, 7, 0, None, 450, None])
    a = tr.arrays(cases)
    free = tr.expect(cases, base=BASE)
    b = free["run"]["bytes"].astype(np.int64)
    ends = np.cumsum(b)
    total = int(ends[-1])
    assert (b > 0).sum() == 6
    seen = set()
    for max_bytes in (0, int(b[0]) - 1, int(b[0]), int(ends[1]) - 1, int(ends[1]), int(ends[1]) + 1, int(ends[2]),
                      int(ends[4]) - 1, int(ends[4]), int(ends[5]) - 1, total - 1, total, total + 1, M32):
        want = tr.expect(cases, max_bytes, base=BASE)
        assert int(want["total"][2]) == total
        seen.add(int((want["run"]["stop"] == dm.STOP_CAPACITY).sum()))
        check(run_data(dev, a, max_bytes), want, max_bytes)
    assert seen == {0, 1, 2, 3, 5, 6, 7}
    # mixed traffic: the cut anywhere
    cases, a, free = _mixed(2 * TILE + 7)
    total = int(free["total"][1])
    for max_bytes in (total // 3, total // 2, total - 1):
        check(run_data(dev, a, max_bytes), tr.expect(cases, max_bytes, base=BASE), max_bytes)


def _tcb_after(t: dm.Tcb, run) -> dm.Tcb:
    """The tcb the host has after it applied a run record."""
    t = copy.deepcopy(t)
    t.rcv_next, t.rcv_window = int(run["next"]), int(run["window"])
    t.data_size = t.max_receive_buf_size - int(run["room"])
    t.nr_full_seg_received = 1 if run["flags"] & dm.NR_FULL else 0
    t.armed = bool(run["flags"] & dm.ACK_ARMED)
    return t


def test_hand_off(dev):
    """Per run: the model fed the run record's state and then the segments the
    device left ends where the model fed the whole run ends — also when the
    capacity made the device take less."""
    cases, a, free = _mixed(2 * TILE + 7)
    for max_bytes in (M32, int(free["total"][1]) // 2):
        got = run_data(dev, a, max_bytes)
        for (t, segs), run, whole in zip(cases, got["run"], free["results"]):
            rest = dm.walk(_tcb_after(t, run), segs[int(run["taken"]):])
            assert (rest.next, rest.window, rest.room) == (whole.next, whole.window, whole.room)
            assert rest.flags & (dm.NR_FULL | dm.ACK_ARMED) == whole.flags & (dm.NR_FULL | dm.ACK_ARMED)
            assert int(run["taken"]) + rest.taken == whole.taken and int(run["bytes"]) + rest.bytes == whole.bytes
            assert rest.stop == whole.stop


def test_deterministic(dev):
    """Two runs into outputs at other addresses give identical bytes."""
    _, a, _ = _mixed(2 * TILE + 7)
    for max_bytes in (M32, 200000):
        x, y = run_data(dev, a, max_bytes), run_data(dev, a, max_bytes, shift=3)
        for name in x:
            assert x[name].tobytes() == y[name].tobytes(), name


def test_capturable(dev):
    """The launches replay from a graph: no allocation, no synchronisation inside the call."""
    cases, a, want = _mixed(2 * TILE + 7)
    lib = native.load()
    n, nconns = a["n"], a["nconns"]
    ins = [_dev(dev, x) for x in (a["seg"].view(np.int64), a["first"].view(np.int32),
                                  np.concatenate([a["run_conn"], [0]]).astype(np.uint32).view(np.int32),
                                  a["run_first"].view(np.int32), a["rx_total"].view(np.int64), a["rcv"].view(np.uint8))]
    outs = dict(run=torch.empty(4 * (min(n, nconns) + 1), dtype=torch.int64, device=dev),
                desc=torch.empty(2 * n, dtype=torch.int64, device=dev),
                total=torch.empty(4, dtype=torch.int64, device=dev))
    ws = torch.empty(int(lib.sccsum_tcp_rx_data_workspace(n, nconns)), dtype=torch.uint8, device=dev)

    def launch():
        rc = lib.sccsum_tcp_rx_data(BASE, *[x.data_ptr() for x in ins[:5]], n, ins[5].data_ptr(), nconns, M32,
                                    outs["run"].data_ptr(), outs["desc"].data_ptr(), outs["total"].data_ptr(),
                                    ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    for v in outs.values():
        v.fill_(0x5A)
    launch()
    torch.cuda.synchronize()
    keep = {k: v.clone() for k, v in outs.items()}
    r = len(cases)
    check(dict(run=keep["run"].cpu().numpy()[:4 * r].view(tr.RUN_DTYPE), total=keep["total"].cpu().numpy().view(np.uint64),
               desc=keep["desc"].cpu().numpy()[:2 * int(want["total"][0])].view(tr.DESC_DTYPE)), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for v in outs.values():
        v.fill_(0x5A)
    ws.fill_(0xC3)
    g.replay()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert torch.equal(v, keep[k]), k


# ---------------------------------------------------------------- end to end, from frames

NCONNS = 12


def _wire(seed: int):
    """Frames of NCONNS connections interleaved: in-order streams with payload,
    into which a reordered pair, a FIN, a pure ACK and an advancing ACK are
    spliced; and each connection's tcb."""
    rng = np.random.default_rng(8800 + seed)
    tcbs, streams = [], []
    for c in range(NCONNS):
        una = int(rng.integers(0, 1 << 32))
        t = dm.Tcb(rcv_next=M32 - 40 if c == 2 else int(rng.integers(0, 1 << 32)), mss=100, snd_unacknowledged=una,
                   snd_next=(una + 500) & M32, nr_full_seg_received=c & 1, armed=bool(c & 2),
                   established=c != 7, max_receive_buf_size=700 if c == 8 else 1 << 20)
        t.rcv_window = t.modified_window()
        tcbs.append(t)
        seq, frames = t.rcv_next, []
        for k in range(int(rng.integers(12, 30))):
            length = (100, 99, 101, 1, 100, 100, 250)[int(rng.integers(0, 7))]
            kw = dict(seq=seq, ack=una, flags=tm.ACK | (tm.PSH if k % 3 == 0 else 0),
                      payload=rng.integers(0, 256, length, dtype=np.uint8).tobytes())
            if c % 4 == 1 and k == 6:
                kw["flags"] |= tm.FIN
            if c % 4 == 2 and k == 9:
                kw["payload"] = b""
                length = 0
            if c % 4 == 3 and k == 4:
                kw["ack"] = (una + 7) & M32
            s, d, l4 = tcp_traffic.to_conn(c, **kw)
            frames.append(tcp_traffic.frame(s, d, l4, ident=k))
            seq = (seq + length) & M32
        if c == 4 and len(frames) > 3:
            frames[2], frames[3] = frames[3], frames[2]
        streams.append(frames)
    wire = []
    while any(streams):
        c = int(rng.integers(0, NCONNS))
        if streams[c]:
            wire.append(streams[c].pop(0))
    return tcbs, wire


def test_end_to_end_from_frames(dev):
    """frames -> eth_rx -> ipv4_frames -> tcp_rx -> tcp_rx_data -> pack(): each
    connection's packed bytes are the concatenation of what the model appends
    to _rcv.data; rest(k) is what the model did not take."""
    tcbs, frames = _wire(0)
    length = np.array([len(f) for f in frames], dtype=np.uint32)
    off = (np.cumsum(length + 3, dtype=np.uint64) - length).astype(np.uint64)
    buf = np.zeros(int(off[-1] + length[-1]), dtype=np.uint8)
    for o, f in zip(off.tolist(), frames):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    wire = batch.PacketBatch.from_host(buf, off, length, device=dev)
    ip = batch.eth_rx(wire, (sm.IPV4, sm.ARP)).bucket(0)
    status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(ip, status=status)
    conns = batch.TcpConns(tcp_traffic.conn_array(NCONNS), tcp_traffic.LISTEN, device=dev.index)
    rx = batch.tcp_rx(ip, status, conns, sm.HOST)
    rcv = np.zeros(NCONNS, dtype=batch.TCP_RCV_DTYPE)
    for c, t in enumerate(tcbs):
        for name, v in t.rcv_record().items():
            rcv[c][name] = v
    d = batch.tcp_rx_data(rx, torch.from_numpy(rcv.view(np.uint8).reshape(NCONNS, 32)).to(dev))
    packed = d.pack()
    torch.cuda.synchronize()
    run_conn, _ = rx.runs()
    run_conn = run_conn.cpu().numpy().view(np.uint32)
    assert run_conn.tolist() == list(range(NCONNS)) and rx.bounds()[1] == len(frames)
    data = ip.data.cpu().numpy()
    out = packed.cpu().numpy()
    runs = d.runs_host()
    stops, at, cnt = set(), 0, 0
    for k, c in enumerate(run_conn.tolist()):
        segs = rx.segs(k).cpu().numpy().reshape(-1).view(batch.TCP_SEG_DTYPE)
        want = dm.walk(copy.deepcopy(tcbs[c]), [{n: int(s[n]) for n in segs.dtype.names} for s in segs])
        got = runs[k]
        assert (got["taken"], got["bytes"], got["next"], got["window"], got["room"], got["flags"], got["stop"]) == \
            (want.taken, want.bytes, want.next, want.window, want.room, want.flags, want.stop), (k, got, want)
        assert (got["desc_first"], got["dst_off"]) == (cnt, at)
        text = b"".join(data[o:o + n].tobytes() for o, n in want.data)
        assert len(text) == want.bytes and out[at:at + want.bytes].tobytes() == text, k
        assert d.rest(k).shape[0] == len(segs) - want.taken
        if want.taken < len(segs):
            assert d.rest(k)[0].cpu().numpy().tobytes() == segs[want.taken].tobytes()
        stops.add(want.stop)
        at += want.bytes
        cnt += want.taken
    assert d.totals() == (cnt, at, at) and d.descs.shape[0] == cnt
    assert stops >= {dm.STOP_END, dm.STOP_SEQ, dm.STOP_FLAGS, dm.STOP_EMPTY, dm.STOP_ACK, dm.STOP_INELIGIBLE,
                     dm.STOP_WINDOW}
    # the capacity through the wrapper: half the text
    half = batch.tcp_rx_data(rx, torch.from_numpy(rcv.view(np.uint8).reshape(NCONNS, 32)).to(dev), max_bytes=at // 2)
    t = half.totals()
    assert t[2] == at and 0 < t[1] <= at // 2 and half.runs_host()["stop"][-1] == dm.STOP_CAPACITY
    assert half.pack().cpu().numpy()[:t[1]].tobytes() == out[:t[1]].tobytes()
    conns.close()


def test_cpp_class_on_gpu(tmp_path):
    """Native host program (tests/cpp/tcp_data_gpu.cc): tcp_rx_data against the
    C call it forwards to, on the same inputs into separately poisoned
    outputs; every array byte-equal."""
    exe = str(tmp_path / "tcp_data_gpu")
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "tcp_data_gpu.cc"), "-L", lib_dir, "-lsccsum", "-Wl,-rpath," + lib_dir,
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tcp_data_gpu: OK" in r.stdout
    print(r.stdout)
