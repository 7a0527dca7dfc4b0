"""sccsum_tcp_rx_acks on the GPU against the per-segment model
(tests/tcp_ack_model.py): every field of every run record and d_total, for
runs of every shape around the wave, the block and the entry scan's tile; the
recipe from wire frames; the hand-off to the host's walk; three rounds of the
sender loop; determinism, graph replay and the C++ class."""
import copy
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import stack_model as sm
import tcp_ack_model as am
import tcp_ack_traffic as tr
import tcp_traffic
from seastar_amd import batch, native
from tcp_ack_model import ACK, M32, Entry, Seg, Tcb
from test_gpu_eth import Out, _dev

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, BLOCK = tr.TILE, tr.BLOCK


def _inputs(dev, a: dict) -> list:
    """The device arrays of tcp_ack_traffic.arrays' dict, in the call's order (an empty one has no address)."""
    def ptr_of(x, count):
        return _dev(dev, x) if count else None

    return [ptr_of(a["seg"].view(np.int64), a["n"]), _dev(dev, a["first"].view(np.int32)),
            _dev(dev, np.concatenate([a["run_conn"], [0]]).astype(np.uint32).view(np.int32)),
            _dev(dev, a["run_first"].view(np.int32)), _dev(dev, a["rx_total"].view(np.int64)),
            ptr_of(a["ack"].view(np.uint8), a["nconns"]), _dev(dev, a["q_first"].view(np.int32)),
            ptr_of(a["q_len"].view(np.int32), a["nq"]), ptr_of(a["q_meta"].view(np.int32), a["nq"]),
            ptr_of(a["q_tx"], a["nq"])]


def _call(lib, a: dict, ins: list, run_ptr: int, total_ptr: int, ws_ptr: int) -> int:
    p = [None if x is None else x.data_ptr() for x in ins]
    return lib.sccsum_tcp_rx_acks(p[0], p[1], p[2], p[3], p[4], a["n"], p[5], a["nconns"], p[6], p[7], p[8], p[9], a["nq"],
                                  a["now"], run_ptr, total_ptr, ws_ptr, torch.cuda.current_stream().cuda_stream)


def run_acks(dev, a: dict, shift: int = 0) -> dict:
    """sccsum_tcp_rx_acks on arrays as tcp_rx leaves them (tcp_ack_traffic.arrays) into guarded outputs."""
    lib = native.load()
    n, nconns = a["n"], a["nconns"]
    ins = _inputs(dev, a)
    run = Out(dev, 8 * min(n, nconns), torch.int64, -7, shift)
    total = Out(dev, 4, torch.int64, -7, shift)
    ws = Out(dev, int(lib.sccsum_tcp_rx_acks_workspace(n, nconns, a["nq"])) // 16, torch.complex128, 3.0, shift)
    assert ws.ptr % 16 == 0 and run.ptr % 16 == 0 and (ins[5] is None or ins[5].data_ptr() % 16 == 0)
    rc = _call(lib, a, ins, run.ptr, total.ptr, ws.ptr)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.host()
    r = int(a["rx_total"][0])
    return dict(run=run.host(8 * r).view(tr.RUN_DTYPE), total=total.host().view(np.uint64))


def check(got: dict, want: dict, what="") -> None:
    assert got["total"].tolist() == want["total"].tolist(), what
    for name in tr.RUN_DTYPE.names:
        ne = got["run"][name] != want["run"][name]
        bad = np.flatnonzero(ne if ne.ndim == 1 else ne.any(axis=1))
        assert bad.size == 0, (what, name, bad[:5], got["run"][bad[:5]], want["run"][bad[:5]])
    assert got["run"].tobytes() == want["run"].tobytes(), what


@functools.lru_cache(maxsize=None)
def _mixed(n: int):
    cases = tr.mixed(n % 5 if n != 2 * TILE + 7 else 0, n)
    return cases, tr.arrays(cases), tr.expect(cases)


SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 7]


@pytest.mark.parametrize("n", SIZES)
def test_mixed_runs_against_the_model(dev, n):
    """n segments of bucket 0 (and five of the other buckets behind them): sizes around the wave and the tile."""
    cases, a, want = _mixed(n)
    assert a["n0"] == n
    check(run_acks(dev, a), want)
    if n == 2 * TILE + 7:      # the traffic whose coverage tests/test_tcp_ack_host.py checks
        assert 0.3 * n <= int(want["total"][1]) <= 0.9 * n and len(set(want["run"]["stop"].tolist())) == 9


def test_bucket_zero_empty_and_no_connections(dev):
    a = tr.arrays([], others=9)
    got = run_acks(dev, a)
    assert got["total"].tolist() == [0, 0, 0, 0] and got["run"].size == 0
    a = tr.arrays([], others=0)
    assert a["n"] == 0
    assert run_acks(dev, a)["total"].tolist() == [0, 0, 0, 0]
    # segments, but a table of no connection: nothing is a run
    a = tr.arrays([], others=7)
    a.update(nconns=0, ack=a["ack"][:0], q_first=np.zeros(1, np.uint32), q_len=a["q_len"][:0], q_meta=a["q_meta"][:0],
             q_tx=a["q_tx"][:0], nq=0)
    assert run_acks(dev, a)["total"].tolist() == [0, 0, 0, 0]


LONG = 4 * TILE + 5
SHAPES = {
    # one run over four tiles of 1024 records (sixteen blocks of the record kernel and more)
    "long_straight": ([LONG], None),
    "long_stopped_at_head": ([LONG], [0]),
    "long_stopped_in_tile_0": ([LONG], [700]),
    "long_stopped_in_last_tile": ([LONG], [4 * TILE + 2]),
    "long_stopped_at_last": ([LONG], [LONG - 1]),
    # runs ending on wave and block boundaries, stops in a block's first and last lane
    "boundaries": ([64, 64, 128, 255, 1, 256, 256, 1024, 63, 1, 64], None),
    "stops_in_first_and_last_lane": ([256, 256, 256, 256, 512, 3], [0, 255, None, 128, 256, 2]),
    "stops_behind_a_boundary": ([255, 257, 1023, 1025, 100], [254, 1, 1022, 1024, None]),
    # every segment its own connection: R = n
    "each_its_own_run": ([1] * (TILE + 300), None),
    "runs_of_three": ([3] * 700, None),
}


@functools.lru_cache(maxsize=None)
def _shape(name: str):
    lengths, stops = SHAPES[name]
    cases = tr.by_lengths(sorted(SHAPES).index(name), lengths, stops)
    return cases, tr.arrays(cases), tr.expect(cases)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_run_shapes_against_the_model(dev, name):
    cases, a, want = _shape(name)
    lengths, stops = SHAPES[name]
    taken = want["run"]["taken"].tolist()
    assert taken == [n if s is None else s for n, s in zip(lengths, stops or [None] * len(lengths))]
    if name == "each_its_own_run":
        assert int(a["rx_total"][0]) == a["n0"]
    check(run_acks(dev, a), want, name)


def test_queues_around_the_entry_scans_tiles(dev):
    """Queues whose entries straddle the entry scan's tile boundaries, one
    queue longer than a tile, 1-byte entries, a connection with no entry and
    next == una, and queues that do not add up or hold an entry of no bytes."""
    rng = np.random.default_rng(77)
    cases = tr.by_lengths(40, [300, 900, 40, 700, 5], None, entry_max=40)
    cases += [tr.stream(rng, 1300, "none", 0, 4, entry_max=3)]                      # ~1 300 entries or more
    t = Tcb(una=M32 - 4, wl1=5000, wl2=M32 - 4).queue([1] * 600)                   # 1-byte entries across the wrap
    cases.append((t, [Seg(5000, (t.una + k) & M32) for k in (1, 2, 3, 300, 301, 600)], dict(eligible=None, lens=None)))
    t = Tcb(wl1=5000, wl2=1000).queue([])                                           # nothing in flight
    cases.append((t, [Seg(5000, 1001), Seg(5000, 1000)], dict(eligible=None, lens=None)))
    cases += [tr.stream(rng, 6, "queue_sum", 0, 1), tr.stream(rng, 6, "queue_zero_entry", 0, 3),
              tr.stream(rng, 9, "none", 0, 6)]
    a, want = tr.arrays(cases), tr.expect(cases)
    counts = np.diff(a["q_first"].astype(np.int64))
    assert counts.max() > TILE and a["nq"] > 3 * TILE
    firsts = a["q_first"][:-1][counts > 0]
    assert any(int(f) // TILE != (int(f) + int(c) - 1) // TILE for f, c in zip(firsts, counts[counts > 0]))
    stops = want["run"]["stop"].tolist()
    assert stops[-5:] == [am.STOP_END, am.STOP_ACK, am.STOP_QUEUE, am.STOP_QUEUE, am.STOP_END]
    assert want["run"]["taken"].tolist()[-5] == 6 and int(want["run"]["popped"][-5]) == 600
    check(run_acks(dev, a), want)


def test_hand_off(dev):
    """Per run: the model fed the run record's state and then the segments
    the device left ends where the model fed the whole run ends."""
    cases, a, _ = _mixed(2 * TILE + 7)
    got = run_acks(dev, a)
    names = ("una", "next", "window", "wl1", "wl2", "cwnd", "srtt", "rttvar", "rto", "first_rto_sample", "dupacks",
             "rcv_next", "state", "outputs", "text", "persist", "rtx", "all_acked")
    walked = 0
    for (t, segs, opts), run in zip(cases, got["run"]):
        if opts["lens"] is not None:
            continue                                    # the host's own queue is not what the device was told
        whole = copy.deepcopy(t)
        for s in segs:
            whole.input(s, tr.NOW)
        rec = {name: int(run[name]) for name in tr.RUN_DTYPE.names if name not in ("reserved",)}
        rest = am.apply(t, rec)
        if rec["flags"] & am.POLL:
            rest.outputs += 1                           # clear_delayed_ack(); output()
        for s in segs[rec["taken"]:]:
            rest.input(s, tr.NOW)
        # the walk calls output() once per ACK that could send; the record says whether any could
        both = [(getattr(rest, name), getattr(whole, name)) for name in names if name != "outputs"]
        assert all(x == y for x, y in both), (rec, both)
        assert [e.len for e in rest.data] == [e.len for e in whole.data]
        assert (rest.outputs > 0) == (whole.outputs > 0)
        walked += len(segs) - rec["taken"]
    assert walked > 300


def test_deterministic(dev):
    """Two runs into outputs at other addresses give identical bytes."""
    _, a, _ = _mixed(2 * TILE + 7)
    x, y = run_acks(dev, a), run_acks(dev, a, shift=3)
    for name in x:
        assert x[name].tobytes() == y[name].tobytes(), name


def test_capturable(dev):
    """The launches replay from a graph: no allocation, no synchronisation inside the call."""
    cases, a, want = _mixed(2 * TILE + 7)
    lib = native.load()
    n, nconns = a["n"], a["nconns"]
    ins = _inputs(dev, a)
    outs = dict(run=torch.empty(8 * min(n, nconns), dtype=torch.int64, device=dev),
                total=torch.empty(4, dtype=torch.int64, device=dev))
    ws = torch.empty(int(lib.sccsum_tcp_rx_acks_workspace(n, nconns, a["nq"])), dtype=torch.uint8, device=dev)

    def launch():
        rc = _call(lib, a, ins, outs["run"].data_ptr(), outs["total"].data_ptr(), ws.data_ptr())
        assert rc == 0, rc

    for v in outs.values():
        v.fill_(0x5A)
    launch()
    torch.cuda.synchronize()
    keep = {k: v.clone() for k, v in outs.items()}
    r = len(cases)
    check(dict(run=keep["run"].cpu().numpy()[:8 * r].view(tr.RUN_DTYPE), total=keep["total"].cpu().numpy().view(np.uint64)),
          want)
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


# ---------------------------------------------------------------- from wire frames

def _rx_from_frames(dev, frames: list, nconns: int):
    """frames -> eth_rx -> ipv4_frames -> tcp_rx."""
    length = np.array([len(f) for f in frames], dtype=np.uint32)
    off = (np.cumsum(length + 3, dtype=np.uint64) - length).astype(np.uint64)
    buf = np.zeros(int(off[-1] + length[-1]), dtype=np.uint8)
    for o, f in zip(off.tolist(), frames):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    wire = batch.PacketBatch.from_host(buf, off, length, device=dev)
    ip = batch.eth_rx(wire, (sm.IPV4, sm.ARP)).bucket(0)
    status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(ip, status=status)
    conns = batch.TcpConns(tcp_traffic.conn_array(nconns), tcp_traffic.LISTEN, device=dev.index)
    return batch.tcp_rx(ip, status, conns, sm.HOST), conns


def _interleave(rng, streams: list) -> list:
    streams = [list(s) for s in streams]
    wire = []
    live = [c for c, s in enumerate(streams) if s]
    while live:
        c = live[int(rng.integers(0, len(live)))]
        wire.append(streams[c].pop(0))
        if not streams[c]:
            live.remove(c)
    return wire


def _queues(dev, a: dict) -> batch.TcpAckQueues:
    return batch.TcpAckQueues(first=_dev(dev, a["q_first"].view(np.int32)), length=_dev(dev, a["q_len"].view(np.int32)),
                              meta=_dev(dev, a["q_meta"].view(np.int32)), tx=_dev(dev, a["q_tx"]))


def test_recipe_from_wire_frames(dev):
    """frames -> eth_rx -> ipv4_frames -> tcp_rx -> tcp_rx_acks through the
    wrappers: the mixed traffic of 40 connections interleaved on the wire;
    every run record is the model's, rest(k) is what the model did not take."""
    rng = np.random.default_rng(8900)
    cases = tr.mixed(3, 420)
    a, want = tr.arrays(cases, others=0), tr.expect(cases)
    streams = []
    for k, (t, segs, _) in enumerate(cases):
        c = int(a["run_conn"][k])
        streams.append([tcp_traffic.frame(*tcp_traffic.to_conn(c, seq=s.seq, ack=s.ack, flags=s.flags, window=s.window,
                                                               payload=bytes(s.pay_len)), ident=j)
                        for j, s in enumerate(segs)])
    rx, conns = _rx_from_frames(dev, _interleave(rng, streams), a["nconns"])
    state = _dev(dev, a["ack"].view(np.uint8).reshape(-1, 64))
    d = batch.tcp_rx_acks(rx, state, _queues(dev, a), a["now"])
    torch.cuda.synchronize()
    assert rx.runs()[0].cpu().numpy().view(np.uint32).tolist() == a["run_conn"].tolist()
    assert d.totals() == tuple(int(x) for x in want["total"])
    check(dict(run=d.runs_host(), total=np.array(d.totals(), dtype=np.uint64)), want)
    for k, (t, segs, _) in enumerate(cases):
        taken = int(want["run"]["taken"][k])
        rest = d.rest(k).cpu().numpy().reshape(-1).view(batch.TCP_SEG_DTYPE)
        assert rest.shape[0] == len(segs) - taken
        assert rest["ack"].tolist() == [s.ack for s in segs[taken:]]
    assert d.runs.shape == (len(cases), 64)
    conns.close()


def test_sender_loop(dev):
    """Three rounds of tcp_tx_data -> a model peer that ACKs every second
    segment -> tcp_rx -> tcp_rx_acks -> the next snd records, a model tcb per
    connection compared each round."""
    rng = np.random.default_rng(8950)
    nconns, mtu, scale = 9, 1500, 2
    tcbs = []
    for c in range(nconns):
        t = Tcb(una=(M32 - 3000) if c == 2 else int(rng.integers(0, 1 << 32)), mss=(1460, 536, 1000)[c % 3],
                window=int(rng.integers(8000, 40000)), window_scale=scale, cwnd=int(rng.integers(3000, 20000)),
                ssthresh=(M32, 9000, 2000)[c % 3], unsent_len=int(rng.integers(20000, 90000)),
                rcv_next=int(rng.integers(0, 1 << 32)), first_rto_sample=True,
                state="CLOSE_WAIT" if c == 5 else "ESTABLISHED")
        t.next, t.wl1, t.wl2 = t.una, t.rcv_next, t.una
        tcbs.append(t)
    pool = torch.zeros(1 << 17, dtype=torch.uint8, device=dev)    # every queue's bytes: one buffer each, never read here
    conns = None
    now = 1_000_000_000
    for rnd in range(3):
        # the transmit side: the closed form against the model's own can_send()
        snd = np.zeros(nconns, dtype=batch.TCP_SND_DTYPE)
        for c, t in enumerate(tcbs):
            lip, fip, lp, fp = tcp_traffic.conn_tuple(c)
            snd[c] = (fip, t.next, t.una, t.window, t.cwnd, t.rcv_next, lp, fp, t.mss, 512,
                      (native.TCP_SND_ELIGIBLE if t.dupacks == 0 else 0) | (native.TCP_SND_RTX_ARMED if t.data else 0),
                      (0, 0, 0), (0, 0, 0))
        cut = batch.tcp_tx_data(_dev(dev, snd.view(np.uint8).reshape(nconns, 48)),
                                torch.full((nconns,), pool.data_ptr(), dtype=torch.int64, device=dev),
                                _dev(dev, np.array([t.unsent_len for t in tcbs], dtype=np.uint32).view(np.int32)),
                                torch.arange(nconns + 1, dtype=torch.int32, device=dev), sm.HOST, mtu, max_segs=4096)
        torch.cuda.synchronize()
        sent = cut.runs_host()
        streams = []
        for c, t in enumerate(tcbs):
            used = (t.next - t.una) & M32
            can = 0 if used > t.window or t.dupacks else min(t.window - used, t.unsent_len)
            assert int(sent[c]["bytes"]) == can
            assert int(sent[c]["stop"]) in ((native.TCP_STOP_INELIGIBLE,) if t.dupacks else
                                            (native.TCP_STOP_END, native.TCP_STOP_WINDOW))
            lens = [int(x) for x in cut.segs(c)[1].cpu().numpy().view(np.uint32).tolist() if x]
            assert sum(lens) == can
            for n in lens:
                t.data.append(Entry(n, n, 0, now))
            t.next = (t.next + can) & M32
            assert t.next == int(sent[c]["next"])
            t.unsent_len -= can
            # the peer: an ACK behind every second segment (an even connection's last one too), 30 ms later
            ends = np.cumsum([e.len for e in t.data]).tolist()
            points = sorted(set(ends[1::2] + (ends[-1:] if c % 2 == 0 else [])))
            if c == 4 and rnd == 1 and len(points) > 2:
                points[2] = points[1]                                   # a duplicate ACK mid-run
            segs = [Seg(t.rcv_next, (t.una + p) & M32, window=int(rng.integers(3000, 16000)), flags=ACK) for p in points]
            streams.append(segs)
        now += 30_000_000 + 400_000
        frames = [[tcp_traffic.frame(*tcp_traffic.to_conn(c, seq=s.seq, ack=s.ack, flags=s.flags, window=s.window), ident=j)
                   for j, s in enumerate(segs)] for c, segs in enumerate(streams)]
        if conns is not None:
            conns.close()
        rx, conns = _rx_from_frames(dev, _interleave(rng, frames), nconns)
        cases = [(t, segs, dict(eligible=None, lens=None)) for t, segs in zip(tcbs, streams) if segs]
        live = [c for c, segs in enumerate(streams) if segs]
        state = np.zeros(nconns, dtype=batch.TCP_ACK_DTYPE)
        q_first, q_len, q_meta, q_tx = [0], [], [], []
        for c, t in enumerate(tcbs):
            for name in ("una", "next", "window", "wl1", "wl2", "cwnd", "ssthresh", "unsent_len", "rcv_next", "rto", "srtt",
                         "rttvar", "mss", "window_scale"):
                state[c][name] = getattr(t, name)
            state[c]["flags"] = am.in_flags(t)
            q_len += [e.len for e in t.data]
            q_meta += [e.data_len | (0x10000 if e.nr_transmits else 0) for e in t.data]
            q_tx += [e.tx_time for e in t.data]
            q_first.append(len(q_len))
        q = batch.TcpAckQueues(first=_dev(dev, np.array(q_first, dtype=np.int32)), length=_dev(dev, np.array(q_len, dtype=np.int32)),
                               meta=_dev(dev, np.array(q_meta, dtype=np.int32)), tx=_dev(dev, np.array(q_tx, dtype=np.int64)))
        d = batch.tcp_rx_acks(rx, _dev(dev, state.view(np.uint8).reshape(nconns, 64)), q, now)
        torch.cuda.synchronize()
        assert rx.runs()[0].cpu().numpy().view(np.uint32).tolist() == live
        want = tr.expect(cases, now)
        check(dict(run=d.runs_host(), total=np.array(d.totals(), dtype=np.uint64)), want, rnd)
        # the host: the record into the tcb, then its own walk of the rest; the next snd record follows
        for k, c in enumerate(live):
            rec = {name: int(d.runs_host()[k][name]) for name in tr.RUN_DTYPE.names if name != "reserved"}
            whole = copy.deepcopy(tcbs[c])
            for s in streams[c]:
                whole.input(s, now)
            t = am.apply(tcbs[c], rec)
            for s in streams[c][rec["taken"]:]:
                t.input(s, now)
            assert (t.una, t.window, t.cwnd, t.rto, t.dupacks) == (whole.una, whole.window, whole.cwnd, whole.rto,
                                                                   whole.dupacks), (rnd, c)
            assert [e.len for e in t.data] == [e.len for e in whole.data]
            tcbs[c] = t
        assert int(d.totals()[1]) > nconns
    conns.close()
    # every entry is acknowledged 30, 60 or 90 ms after it was sent; srtt = srtt * 7 / 8 + R / 8 with truncation
    # settles at 24 for samples of 30
    sampled = [t for t in tcbs if not t.first_rto_sample]
    assert len(sampled) > nconns // 2 and all(24 <= t.srtt <= 90 for t in sampled)


def test_cpp_class_on_gpu(tmp_path):
    """Native host program (tests/cpp/tcp_ack_gpu.cc): tcp_rx_acks against the
    C call it forwards to, on the same inputs into separately poisoned
    outputs; every array byte-equal."""
    exe = str(tmp_path / "tcp_ack_gpu")
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "tcp_ack_gpu.cc"), "-L", lib_dir, "-lsccsum", "-Wl,-rpath," + lib_dir,
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tcp_ack_gpu: OK" in r.stdout
    print(r.stdout)
