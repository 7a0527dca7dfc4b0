"""sccsum_tcp_tx_data on the GPU: every field of every run record, segment
array, descriptor and d_total against the model (tests/tcp_tx_model.py through
its numpy restatement, tests/tcp_tx_fast.py, which tests/test_tcp_tx_fast.py
pins to it), the gathered payloads against the queues, the full tx recipe
against stack_model.tx, and a loopback into the receive fast path."""
import copy
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import stack_model as sm
import tcp_model
import tcp_tx_fast as fast
import tcp_tx_model as tm
import tcp_tx_traffic as tr
from seastar_amd import batch, native
from tcp_tx_model import Hw, Tcb
from test_gpu_eth import Out, _dev

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = tr.TILE
M32 = 0xFFFFFFFF
FAKE = 0x7000_0000_1000        # an address for buffers that are never gathered
DESC = np.dtype([("src", "<u8"), ("dst_off", "<u4"), ("len", "<u4")])


def run_tx(dev, a: dict, hw: Hw = Hw(), headroom: int = 20, max_segs: int | None = None, max_bytes: int = M32,
           shift: int = 0, base: int = FAKE) -> dict:
    """sccsum_tcp_tx_data on a's snd / buf_len / buf_first into guarded outputs;
    buffer j lies at base + a["blob_off"][j].  max_segs None: what the batch needs."""
    lib = native.load()
    snd, buf_len, first = a["snd"], a["buf_len"], a["buf_first"]
    nconns, nbuf = snd.size, buf_len.size
    want = fast.expect(snd, buf_len, first, hw.mtu, headroom, hw.tx_tso, hw.max_packet_len)
    room = int(want["total"][0]) if max_segs is None else max_segs
    src = (a["blob_off"].astype(np.uint64) + np.uint64(base)) if nbuf else np.zeros(0, np.uint64)
    d_snd = _dev(dev, snd.view(np.uint8)) if nconns else None
    d_src, d_len = (_dev(dev, src.view(np.int64)), _dev(dev, buf_len.view(np.int32))) if nbuf else (None, None)
    d_first = _dev(dev, first.view(np.int32))
    run = Out(dev, 2 * nconns, torch.complex128, -7.0, shift)
    off = Out(dev, room, torch.int64, -7, shift)
    length = Out(dev, room, torch.int32, -7, shift)
    out = Out(dev, 6 * room, torch.int32, -7, shift)
    seg_first = Out(dev, room + 1, torch.int32, -7, shift)
    desc = Out(dev, 2 * (room + nbuf), torch.int64, -7, shift)
    total = Out(dev, 4, torch.int64, -7, shift)
    ws = Out(dev, int(lib.sccsum_tcp_tx_data_workspace(nconns, nbuf)) // 16, torch.complex128, 3.0, shift)
    assert ws.ptr % 16 == 0 and run.ptr % 16 == 0 and (d_snd is None or d_snd.data_ptr() % 16 == 0)
    import ctypes
    opts = native.TcpTxOpts(sm.HOST, hw.mtu, hw.max_packet_len, headroom, native.TCP_TSO if hw.tx_tso else 0)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = lib.sccsum_tcp_tx_data(ctypes.addressof(opts), p(d_snd), nconns, p(d_src), p(d_len), d_first.data_ptr(), nbuf,
                                room, max_bytes, run.ptr if nconns else None, *(x.ptr if room else None for x in (off, length, out)),
                                seg_first.ptr, desc.ptr if room else None, total.ptr, ws.ptr,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.host()
    t = total.host().view(np.uint64)
    f, pieces = int(t[0]), int(t[2])
    assert f <= room and pieces <= room + nbuf
    return dict(run=run.host().view(fast.RUN_DTYPE), off=off.host(f).view(np.uint64), len=length.host(f).view(np.uint32),
                out=out.host(6 * f).view(fast.OUT_DTYPE), seg_first=seg_first.host(f + 1).view(np.uint32),
                desc=desc.host(2 * pieces).view(DESC), total=t, src=src)


def check(got: dict, want: dict, what="") -> None:
    assert got["total"].tolist() == want["total"].tolist(), what
    for name in ("segs", "bytes", "seg_first", "next", "flags", "stop", "pad", "reserved"):
        bad = np.flatnonzero(np.atleast_2d(got["run"][name].T != want["run"][name].T).any(axis=0))
        assert bad.size == 0, (what, name, bad[:5], got["run"][bad[:5]], want["run"][bad[:5]])
    for name in ("off", "len", "seg_first"):
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, (what, name, bad[:5], got[name][bad[:5]], want[name][bad[:5]])
    assert got["out"].tobytes() == want["out"].tobytes(), what
    assert np.array_equal(got["desc"]["src"], got["src"][want["desc_buf"]] + want["desc_inner"].astype(np.uint64)), what
    assert np.array_equal(got["desc"]["dst_off"], want["desc_dst"]) and np.array_equal(got["desc"]["len"], want["desc_len"])


@functools.lru_cache(maxsize=None)
def _mixed(n: int):
    cases = tr.mixed(n, n)
    return cases, tr.arrays(cases)


SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 7]
SETUPS = [(Hw(1500), 20), (Hw(576), 24), (Hw(1500, True, 65521), 64), (Hw(9000), 20), (Hw(68), 24)]


@pytest.mark.parametrize("n", SIZES)
def test_mixed_connections_against_the_model(dev, n):
    cases, a = _mixed(n)
    hw, headroom = SETUPS[SIZES.index(n) % len(SETUPS)]
    want = fast.expect(a["snd"], a["buf_len"], a["buf_first"], hw.mtu, headroom, hw.tx_tso, hw.max_packet_len)
    check(run_tx(dev, a, hw, headroom), want, n)
    if n == 0:
        assert want["total"].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("headroom", [20, 24, 64])
def test_gathered_payloads_are_the_queues(dev, headroom):
    """pack() through the wrapper, the buffers in device memory: every
    segment's bytes in the staging layout are its connection's stream bytes."""
    cases, a = _mixed(TILE + 1)
    _payloads_through_the_wrapper(dev, cases, a, _dev(dev, a["blob"]), headroom)


def test_buffers_in_pinned_host_memory(dev):
    cases, a = _mixed(65)
    _payloads_through_the_wrapper(dev, cases, a, torch.from_numpy(a["blob"]).pin_memory(), 20)


def _payloads_through_the_wrapper(dev, cases, a, blob, headroom):
    hw = Hw(1500)
    want = fast.expect(a["snd"], a["buf_len"], a["buf_first"], hw.mtu, headroom)
    src = _dev(dev, (a["blob_off"] + np.uint64(blob.data_ptr())).view(np.int64))
    d = batch.tcp_tx_data(_dev(dev, a["snd"].view(np.uint8).reshape(-1, 48)), src, _dev(dev, a["buf_len"].view(np.int32)),
                          _dev(dev, a["buf_first"].view(np.int32)), sm.HOST, hw.mtu, int(want["total"][0]) + 3,
                          headroom=headroom)
    payloads, out = d.pack()
    torch.cuda.synchronize()
    assert d.totals() == tuple(want["total"].tolist()) and payloads.n == out.shape[0] == d.totals()[0]
    assert payloads.bytes_len == d.totals()[1] and payloads.max_len == 1460 and d.descs.shape[0] == d.totals()[2]
    runs = d.runs_host()
    assert runs.tobytes() == want["run"].tobytes()
    staging = payloads.data.cpu().numpy()
    off, length = payloads.off.cpu().numpy(), payloads.length.cpu().numpy()
    assert np.array_equal(off.view(np.uint64), want["off"]) and np.array_equal(length.view(np.uint32), want["len"])
    assert out.cpu().numpy().tobytes() == want["out"].tobytes()
    f = 0
    for c, t in enumerate(cases):
        stream = b"".join(t.unsent)
        o, ln, rec = d.segs(c)
        assert o.shape[0] == ln.shape[0] == rec.shape[0] == runs["segs"][c]
        at = 0
        for k in range(int(runs["segs"][c])):
            n = int(length[f])
            assert staging[int(off[f]):int(off[f]) + n].tobytes() == stream[at:at + n], (c, k)
            at += n
            f += 1
        assert at == runs["bytes"][c]


# ---------------------------------------------------------------- queues and cuts written out

def _one(sizes, **kw) -> Tcb:
    t = Tcb(**dict(dict(snd_window=1 << 30, cwnd=1 << 30, mss=1460), **kw))
    t.unsent_len = sum(sizes)
    t.unsent.extend(sizes)       # lengths alone: these buffers are never read
    return t


def _arrays_of(tcbs) -> dict:
    """tr.arrays for tcbs whose queues hold lengths, not bytes."""
    snd = np.array([tr.snd_record(t) for t in tcbs], dtype=fast.SND_DTYPE)
    buf_len = np.array([n for t in tcbs for n in t.unsent], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(t.unsent) for t in tcbs])]).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(buf_len, dtype=np.uint64)]).astype(np.uint64)[:-1]
    return dict(snd=snd, buf_len=buf_len, buf_first=first, blob_off=off)


def _expect(a, hw=Hw(), headroom=20, max_segs=0x7FFFFFFF, max_bytes=M32):
    return fast.expect(a["snd"], a["buf_len"], a["buf_first"], hw.mtu, headroom, hw.tx_tso, hw.max_packet_len, max_segs,
                       max_bytes)


SHAPES = {
    "no_buffers": [_one([]), _one([]), _one([])],
    "one_buffer_each": [_one([n]) for n in (1, 1459, 1460, 1461, 2920, 2921, 4000)],
    "many_buffers": [_one([700] * 50), _one([1] * 7 + [5000] + [0] * 9 + [3])],
    "one_byte_buffers": [_one([1] * (3 * 1460 + 5)), _one([0, 1] * 1500)],            # 1 460 pieces in a segment
    "one_64k_buffer": [_one([65536]), _one([65536, 65536])],                           # 45 segments out of one buffer
    "cuts_on_boundaries": [_one([1460, 1460, 1460]), _one([1459, 1, 1460, 1461, 1459]), _one([1460, 0, 0, 1460]),
                           _one([2920, 1460]), _one([0, 0, 0])],
    "around_a_multiple": [_one([10000], snd_window=w) for w in (2919, 2920, 2921, 1, 0)],
    "empty_between": [_one([]), _one([100]), _one([]), _one([]), _one([100]), _one([])],
    "tso": [_one([200000]), _one([65481] * 3), _one([65482, 65480])],
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_queue_shapes_against_the_model(dev, name):
    a = _arrays_of(SHAPES[name])
    hw = Hw(1500, True, 65521) if name == "tso" else Hw()
    want = _expect(a, hw)
    got = run_tx(dev, a, hw)
    check(got, want, name)
    pieces = np.diff(want["seg_first"].astype(np.int64))
    if name == "one_byte_buffers":
        assert pieces.max() == 1460
    if name == "one_64k_buffer":
        assert want["run"]["segs"][0] == 45 and pieces[:45].tolist() == [1] * 45
    if name == "tso":
        assert want["len"].max() == 65481


def test_segments_end_on_wave_and_tile_boundaries(dev):
    """cwnd = 1: one byte a segment.  The connections' segments end at 63, 64,
    65, 255, 256, 257, 1023, 1024, 1025 and 2049 of the segment order."""
    ends = [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
    counts = np.diff([0] + ends).tolist()
    a = _arrays_of([_one([5000], cwnd=1, snd_window=n) for n in counts])
    want = _expect(a)
    assert want["run"]["segs"].tolist() == counts and want["len"].tolist() == [1] * 2049
    check(run_tx(dev, a), want)


def test_one_connection_past_the_block_cap(dev):
    """cwnd = 1 and a window that carries the connection's segments past one
    tile of the segment kernel and past its grid's block cap: the second trip
    of the stride.  Small bytes, many segments, the buffers 1 000 bytes each."""
    lib = native.load()
    per_trip = lib.sccsum_tcp_tx_data_seg_tile() * lib.sccsum_tcp_tx_data_max_blocks()
    n = per_trip + 1031
    a = _arrays_of([_one([3]), _one([1000] * (n // 1000 + 2), cwnd=1, snd_window=n, snd_next=M32 - 5,
                                                  snd_unacknowledged=M32 - 5), _one([7])])
    want = _expect(a)
    assert want["total"][0] == n + 2 > per_trip and want["run"]["segs"].tolist() == [1, n, 1]
    check(run_tx(dev, a), want)


def test_sums_past_32_bits(dev):
    """Global buffer sums past 2^32 under small windows (the buffers are never
    gathered), a queue of exactly 2^32 - 1 bytes and one of 2^32."""
    big = 0xF0000000
    tcbs = [_one([big], snd_window=3000 + c) for c in range(6)]
    tcbs += [_one([0x80000000, 0x7FFFFFFF], snd_window=5000), _one([0x80000000, 0x80000000], snd_window=5000),
             _one([M32], snd_window=2000), _one([M32, 1], snd_window=2000), _one([M32, 0], snd_window=2000),
             _one([700, 700], snd_window=5000)]
    a = _arrays_of(tcbs)
    want = _expect(a)
    assert want["run"]["stop"][6:].tolist() == [tm.STOP_WINDOW, tm.STOP_QUEUE, tm.STOP_WINDOW, tm.STOP_QUEUE,
                                                tm.STOP_WINDOW, tm.STOP_END]
    got = run_tx(dev, a)
    check(got, want)
    assert got["desc"]["src"].max() > FAKE + (1 << 34)
    # the whole of a 2^32 - 1 byte queue, in segments of 65 481: the last stream offsets do not wrap
    a = _arrays_of([_one([0x80000000, 0x7FFFFFFF], snd_window=M32, snd_next=5, snd_unacknowledged=5)])
    hw = Hw(1500, True, 65521)
    # with their headroom they fit no layout: the need is reported, nothing is emitted
    c = fast.connections(a["snd"], a["buf_len"], a["buf_first"], hw.mtu, 20, True, hw.max_packet_len)
    assert c["sent"][0] == M32 and c["stop"][0] == tm.STOP_END and c["segs"][0] == 65592
    want = _expect(a, hw)
    assert want["total"].tolist() == [0, 0, 0, M32 + 20 * 65592] and want["run"]["stop"][0] == tm.STOP_CAPACITY
    check(run_tx(dev, a, hw, max_segs=70000), want)
    check(run_tx(dev, a, hw, max_bytes=0), _expect(a, hw, max_bytes=0))
    check(run_tx(dev, a, hw, max_segs=100, max_bytes=M32), _expect(a, hw, max_segs=100))
    # a window 2 MiB short of it: the layout just fits, the last offsets and descriptors stand near 2^32
    a = _arrays_of([_one([0x80000000, 0x7FFFFFFF], snd_window=M32 - (1 << 21), snd_next=5, snd_unacknowledged=5)])
    want = _expect(a, hw)
    assert want["run"]["stop"][0] == tm.STOP_WINDOW and want["run"]["segs"][0] == 65560 and want["total"][1] > 0xFFF00000
    got = run_tx(dev, a, hw)
    check(got, want)
    assert got["desc"]["src"].max() > FAKE + 0xFFD00000 and want["total"][2] == 65561


def test_capacity_cut(dev):
    """The prefix rule on each of the two caps: at the first connection, mid-way,
    exactly equal, one less, and 0."""
    cases, a = _mixed(2 * TILE + 7)
    full = _expect(a)
    segs, lay = int(full["total"][0]), int(full["total"][1])
    seg_at, lay_at = np.cumsum(full["run"]["segs"]), np.cumsum(full["run"]["bytes"] + 20 * full["run"]["segs"].astype(np.int64))
    mid = TILE + 100
    caps = [(segs, lay), (segs - 1, lay), (segs, lay - 1), (int(seg_at[mid]), lay), (int(seg_at[mid]) - 1, lay),
            (segs, int(lay_at[mid])), (segs, int(lay_at[mid]) - 1), (0, lay), (segs, 0), (segs, 19), (1, 20)]
    stops = set()
    for max_segs, max_bytes in caps:
        want = _expect(a, max_segs=max_segs, max_bytes=max_bytes)
        check(run_tx(dev, a, max_segs=max_segs, max_bytes=max_bytes), want, (max_segs, max_bytes))
        assert want["total"][3] == lay
        stops.add(int((want["run"]["stop"] == tm.STOP_CAPACITY).sum()))
    # connections that take nothing anyway, in front of the first that does not fit, keep their own stop
    first = int(np.flatnonzero(full["run"]["segs"])[0])
    assert 0 in stops and len(cases) - first in stops and len(stops) >= 5
    # room for more than is needed changes nothing
    check(run_tx(dev, a, max_segs=segs + 1000), full)


def test_hand_off(dev):
    """The model fed the run record's state continues to where the model fed
    everything ends: for a connection the device took there is nothing left to
    do, for the others the host's own trip starts from the state as given."""
    cases, a = _mixed(TILE + 1)
    hw = Hw()
    full = _expect(a)
    got = run_tx(dev, a, hw, max_segs=int(full["total"][0]) * 2 // 3)
    kinds = set()
    for c, t in enumerate(cases):
        r = got["run"][c]
        lo = int(r["seg_first"])
        rec = tm.Run(int(r["segs"]), int(r["bytes"]), int(r["next"]), int(r["flags"]), int(r["stop"]),
                     got["out"]["seq"][lo:lo + int(r["segs"])].tolist(), got["len"][lo:lo + int(r["segs"])].tolist())
        mine = tm.continue_from(t, rec)
        theirs = copy.deepcopy(t)
        limit = 200 if t.window_probe else 1 << 22   # a window probe's chain does not end by itself
        tm.chain(theirs, hw, limit)
        if rec.segs == 0:
            assert (mine.snd_next, mine.unsent_len, mine.rtx_armed) == (t.snd_next, t.unsent_len, t.rtx_armed)
            tm.chain(mine, hw, limit)        # not taken: the host's own trip, from the state as given
        kinds.add(int(r["stop"]))
        assert (mine.snd_next, mine.unsent_len, mine.rtx_armed, mine.data, b"".join(mine.unsent)) == (
            theirs.snd_next, theirs.unsent_len, theirs.rtx_armed, theirs.data, b"".join(theirs.unsent)), c
    assert kinds == {tm.STOP_END, tm.STOP_WINDOW, tm.STOP_INELIGIBLE, tm.STOP_CAPACITY}


def test_deterministic(dev):
    """Two runs into outputs at other addresses give identical bytes."""
    _, a = _mixed(2 * TILE + 7)
    for max_segs in (None, 3000):
        x, y = run_tx(dev, a, max_segs=max_segs), run_tx(dev, a, max_segs=max_segs, shift=3)
        for name in x:
            assert x[name].tobytes() == y[name].tobytes(), name


def test_capturable(dev):
    """The launches replay from a graph: no allocation, no synchronisation inside the call."""
    import ctypes
    cases, a = _mixed(2 * TILE + 7)
    want = _expect(a)
    lib = native.load()
    nconns, nbuf, room = a["snd"].size, a["buf_len"].size, int(want["total"][0]) + 5
    src = a["blob_off"] + np.uint64(FAKE)
    ins = [_dev(dev, x) for x in (a["snd"].view(np.uint8), src.view(np.int64), a["buf_len"].view(np.int32),
                                  a["buf_first"].view(np.int32))]
    outs = dict(run=torch.empty(4 * nconns, dtype=torch.int64, device=dev), off=torch.empty(room, dtype=torch.int64, device=dev),
                len=torch.empty(room, dtype=torch.int32, device=dev), out=torch.empty(6 * room, dtype=torch.int32, device=dev),
                seg_first=torch.empty(room + 1, dtype=torch.int32, device=dev),
                desc=torch.empty(2 * (room + nbuf), dtype=torch.int64, device=dev),
                total=torch.empty(4, dtype=torch.int64, device=dev))
    ws = torch.empty(int(lib.sccsum_tcp_tx_data_workspace(nconns, nbuf)), dtype=torch.uint8, device=dev)
    opts = native.TcpTxOpts(sm.HOST, 1500, 65535, 20, 0)

    def launch():
        rc = lib.sccsum_tcp_tx_data(ctypes.addressof(opts), ins[0].data_ptr(), nconns, ins[1].data_ptr(), ins[2].data_ptr(),
                                    ins[3].data_ptr(), nbuf, room, M32, *[outs[k].data_ptr() for k in
                                                                          ("run", "off", "len", "out", "seg_first", "desc", "total")],
                                    ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    for v in outs.values():
        v.fill_(0x5A)
    launch()
    torch.cuda.synchronize()
    keep = {k: v.clone() for k, v in outs.items()}
    f, pieces = int(want["total"][0]), int(want["total"][2])
    h = {k: v.cpu().numpy() for k, v in keep.items()}
    check(dict(run=h["run"].view(fast.RUN_DTYPE), off=h["off"][:f].view(np.uint64), len=h["len"][:f].view(np.uint32),
               out=h["out"][:6 * f].view(fast.OUT_DTYPE), seg_first=h["seg_first"][:f + 1].view(np.uint32),
               desc=h["desc"][:2 * pieces].view(DESC), total=h["total"].view(np.uint64), src=src), want)
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


# ---------------------------------------------------------------- the full recipe and the loopback

PEER = sm.ON_LINK[0]


def _recipe_cases(seed: int, n: int) -> list:
    """Connections to one peer, distinct ports, whose segments fit the MTU."""
    cases = tr.mixed(seed, n)
    for c, t in enumerate(cases):
        t.dst, t.sport, t.dport = PEER, 5000 + c, 80 + c % 3
        t.cwnd = max(t.cwnd, 150) if t.cwnd else 0     # not thousands of frames of a few bytes
    return cases


@pytest.mark.parametrize("mtu", [576, 1500])
def test_full_recipe_and_loopback(dev, mtu):
    """tcp_tx_data -> pack() -> tcp_send -> spans -> ipv4_send(SEND_L4) ->
    eth_send(...).pack(): the wire frames byte for byte against the model's
    segments sent through tcp_model.send and stack_model.tx.  Then the frames
    into a peer's eth_rx -> ipv4_frames -> tcp_rx -> tcp_rx_data: the peer's
    packed text is the sender's queue prefix of `bytes` bytes per connection."""
    cases = _recipe_cases(mtu, 90)
    hw = Hw(mtu)
    a = tr.arrays(cases)
    blob = _dev(dev, a["blob"])
    src = _dev(dev, (a["blob_off"] + np.uint64(blob.data_ptr())).view(np.int64))
    d = batch.tcp_tx_data(_dev(dev, a["snd"].view(np.uint8).reshape(-1, 48)), src, _dev(dev, a["buf_len"].view(np.int32)),
                          _dev(dev, a["buf_first"].view(np.int32)), sm.HOST, mtu, max_segs=4096)
    payloads, out = d.pack()
    u = batch.tcp_send(payloads, out, sm.HOST, mtu)
    n = payloads.n
    d_dst = torch.full((n,), PEER, dtype=torch.int32, device=dev)
    ids = [(7 * k + mtu) & 0xFFFF for k in range(n)]
    l4sum = batch.spans(u.sum_batch, seeds=u.seeds)
    r = batch.ipv4_send(u.l4, d_dst, u.proto, mtu, sm.HOST, ids=_dev(dev, np.array(ids, np.uint16).view(np.int16)), l4sum=l4sum,
                        flags=native.SEND_L4)
    arp = {x: sm.peer_mac(x) for x in sm.ON_LINK}
    arp[sm.GW] = sm.GW_MAC
    table = batch.ArpTable(arp)
    wire = batch.eth_send(r, d_dst, table, sm.HW, sm.HOST, sm.NETMASK, sm.GW).pack()
    torch.cuda.synchronize()
    assert u.status.cpu().numpy().tolist() == [native.ST_OK] * n
    # the model: every eligible connection's chain, its segments in order
    model, prefix = [], []
    for t in cases:
        stream = b"".join(t.unsent)
        segs = [] if t.why_not_eligible() else tm.chain(copy.deepcopy(t), hw)[0]
        prefix.append(sum(len(s["payload"]) for s in segs))
        assert b"".join(s["payload"] for s in segs) == stream[:prefix[-1]]
        model += [tcp_model.send(s["payload"], {k: s[k] for k in ("dst", "seq", "ack", "sport", "dport", "window", "flags",
                                                                  "mss")}, sm.HOST) for s in segs]
    assert len(model) == n > 100 and d.runs_host()["bytes"].tolist() == prefix
    cfg = dict(host=sm.HOST, netmask=sm.NETMASK, gw=sm.GW, hw=sm.HW, mtu=mtu, arp=arp)
    t = sm.tx([(m["zero"], sm.TCP, PEER, i) for m, i in zip(model, ids)], cfg)
    data, w_off, w_len = wire.data.cpu().numpy(), wire.off.cpu().numpy(), wire.length.cpu().numpy()
    assert wire.n == len(t["frames"]) == n
    for k, want_f in enumerate(t["frames"]):
        assert data[int(w_off[k]):int(w_off[k]) + int(w_len[k])].tobytes() == want_f, ("wire frame", k)
    table.close()

    # the peer
    ip = batch.eth_rx(wire, (sm.IPV4, sm.ARP)).bucket(0)
    status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(ip, status=status)
    conns = batch.TcpConns([(PEER, sm.HOST, tc.dport, tc.sport) for tc in cases], device=dev.index)
    rx = batch.tcp_rx(ip, status, conns, PEER)
    rcv = np.zeros(len(cases), dtype=batch.TCP_RCV_DTYPE)
    for c, tc in enumerate(cases):
        rcv[c] = (tc.snd_next, 1 << 20, 1 << 20, 1 << 20, tc.rcv_next, tc.mss, native.TCP_RCV_ELIGIBLE, 0, (0, 0))
    back = batch.tcp_rx_data(rx, torch.from_numpy(rcv.view(np.uint8).reshape(-1, 32)).to(dev))
    text = back.pack().cpu().numpy()
    torch.cuda.synchronize()
    assert rx.bounds()[1] == n
    run_conn = rx.runs()[0].cpu().numpy().view(np.uint32).tolist()
    assert run_conn == [c for c, tc in enumerate(cases) if not tc.why_not_eligible()]
    for k, run in enumerate(back.runs_host()):
        c = run_conn[k]
        stream = b"".join(cases[c].unsent)
        assert run["bytes"] == prefix[c] and run["next"] == (cases[c].snd_next + prefix[c]) & M32, c
        assert text[int(run["dst_off"]):int(run["dst_off"]) + prefix[c]].tobytes() == stream[:prefix[c]], c
        assert run["stop"] == (native.TCP_STOP_END if prefix[c] else native.TCP_STOP_EMPTY)
    conns.close()


def test_cpp_class_on_gpu(tmp_path):
    """Native host program (tests/cpp/tcp_tx_data_gpu.cc): tcp_tx_data against
    the C call it forwards to, on the same inputs into separately poisoned
    outputs; every array byte-equal, and the gathered bytes are the queues'."""
    exe = str(tmp_path / "tcp_tx_data_gpu")
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "tcp_tx_data_gpu.cc"), "-L", lib_dir, "-lsccsum", "-Wl,-rpath," + lib_dir,
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tcp_tx_data_gpu: OK" in r.stdout
    print(r.stdout)
