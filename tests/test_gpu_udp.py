"""The UDP layer on the device (sccsum_udp_rx, sccsum_udp_rx_reasm,
sccsum_udp_send), compared with the per-datagram models (tests/udp_model.py on
top of tests/stack_model.py).  Every raw call writes into outputs with guard
words on both sides; every comparison is exact, nothing has a tolerance."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import stack_model as sm
import udp_model
import udp_traffic
from seastar_amd import batch, native
from test_gpu_eth import Out, _dev, _u32_dev, _u64_dev

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = sm.HOST
NEED, REJECT = batch.UDP_NEED, batch.UDP_REJECT
SKIP, SHORT, NOPORT = native.UDP_SKIP, native.UDP_SHORT, native.UDP_NOPORT
DROPPED = dict(cls=SKIP, payload=b"", src=0, sport=0, at=0)
FULL = 2 * 1024 + 7


def _i16_dev(dev, a) -> torch.Tensor:
    return _dev(dev, np.asarray(a, dtype=np.uint16).view(np.int16))


@functools.lru_cache(maxsize=None)
def _ports(dev_index: int, nch: int) -> batch.UdpPorts:
    return batch.UdpPorts(udp_traffic.PORTS[:nch], device=dev_index)


def _port_map(nch: int) -> dict:
    return {p: k for k, p in enumerate(udp_traffic.PORTS[:nch])}


# ---------------------------------------------------------------- udp_rx: one raw call

def run_udp_rx(dev, b: batch.PacketBatch, nbatch: int, status, ports, index=None, n=None, need=NEED, reject=REJECT,
               host=HOST, with_class=True, shift=0) -> dict:
    """sccsum_udp_rx on the first nbatch frames of b into guarded outputs; returns their host copies."""
    lib = native.load()
    n = (nbatch if index is None else int(index.numel())) if n is None else n
    nch = len(ports.ports)
    cls = Out(dev, n, torch.uint8, 0xA5, shift)
    first = Out(dev, nch + 2, torch.int32, -7, shift)
    order = Out(dev, n, torch.int32, -7, shift)
    pay_off = Out(dev, n, torch.int64, -7, shift)
    pay_len = Out(dev, n, torch.int32, -7, shift)
    src = Out(dev, n, torch.int32, -7, shift)
    sport = Out(dev, n, torch.int16, -7, shift)
    ws = Out(dev, int(lib.sccsum_udp_rx_workspace(n)) // 16, torch.complex128, 3.0, shift)
    assert ws.ptr % 16 == 0
    some = nbatch > 0
    rc = lib.sccsum_udp_rx(b.data.data_ptr(), b.bytes_len, b.off.data_ptr() if some else None,
                           b.length.data_ptr() if some else None, nbatch, status.data_ptr() if some else None, need,
                           reject, host, ports.handle, None if index is None or n == 0 else index.data_ptr(), n,
                           cls.ptr if with_class else None, first.ptr, order.ptr if n else None,
                           pay_off.ptr if n else None, pay_len.ptr if n else None, src.ptr if n else None,
                           sport.ptr if n else None, ws.ptr, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.host()
    return dict(cls=cls.host() if with_class else cls.host(0), first=first.host().view(np.uint32),
                order=order.host().view(np.uint32), pay_off=pay_off.host().view(np.uint64),
                pay_len=pay_len.host().view(np.uint32), src=src.host().view(np.uint32),
                sport=sport.host().view(np.uint16))


def check_rx(got: dict, items: list, nch: int, off=None, index=None, with_class=True):
    """Every output array against the per-datagram results `items` (the call's order)."""
    want = udp_traffic.expect_rx(items, nch, index)
    names = ["first", "order", "pay_len", "src", "sport"] + (["cls"] if with_class else [])
    for name in names:
        assert np.array_equal(got[name], want[name]), name
    if off is not None:
        idx = list(range(len(items))) if index is None else [int(x) for x in index]
        pay_off = [(int(off[idx[j]]) + items[j]["at"]) if idx[j] < len(off) else 0 for j in want["pos"]]
        assert got["pay_off"].tolist() == pay_off, "pay_off"
    return want


@functools.lru_cache(maxsize=None)
def _bucket(dev_index: int, seed: int):
    """A seed's IPv4 bucket on the device as the recipe makes it (eth_rx, the
    frames call's status), and the model's view of the same frames."""
    dev = torch.device("cuda", dev_index)
    c = udp_traffic.case(seed)
    length = np.array([len(f) for f in c["frames"]], dtype=np.uint32)
    gaps = np.arange(length.size) % 5
    off = (np.cumsum(length + gaps, dtype=np.uint64) - length).astype(np.uint64)
    buf = np.zeros(int(off[-1] + length[-1]), dtype=np.uint8)
    for o, f in zip(off.tolist(), c["frames"]):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    wire = batch.PacketBatch.from_host(buf, off, length, device=dev)
    rx = batch.eth_rx(wire, (sm.IPV4, sm.ARP))
    ip = rx.bucket(0)
    status = torch.empty(max(ip.n, 1), dtype=torch.uint8, device=dev)[:ip.n]
    batch.ipv4_frames(ip, status=status)
    torch.cuda.synchronize()
    assert ip.n == len(c["ip"])
    assert status.cpu().numpy().tolist() == [i["status"] for i in c["info"]]
    return c, ip, status, ip.off.cpu().numpy().view(np.uint64)


def _atomic(c, nch: int) -> list:
    pm = _port_map(nch)
    return [udp_model.atomic(p, info["delivered"], pm) for p, info in zip(c["ip"], c["info"])]


SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, FULL]
CHANNELS = [0, 1, 2, 64, 65, 252]
RX_CASES = ([(n, 252, True) for n in SIZES] + [(n, 2, k % 2 == 0) for k, n in enumerate(SIZES)]
            + [(FULL, c, c % 2 == 0) for c in CHANNELS] + [(1025, 65, False), (64, 64, True)])


@pytest.mark.parametrize("n,nch,with_class", RX_CASES)
def test_udp_rx_against_the_model(dev, n, nch, with_class):
    """The first n frames of a seed's IPv4 bucket through C channels: sizes
    around the wave and the tile, channel counts on both scan paths."""
    c, ip, status, off = _bucket(dev.index, 0)
    assert ip.n >= FULL
    got = run_udp_rx(dev, ip, n, status, _ports(dev.index, nch), with_class=with_class)
    want = check_rx(got, _atomic(c, nch)[:n], nch, off, with_class=with_class)
    if n == FULL and nch == 252:
        counts = np.diff(want["first"].astype(np.int64))
        assert counts[0] > 1024 and counts[251] == 0 and counts[252] > 50


@pytest.mark.parametrize("seed", udp_traffic.SEEDS)
def test_udp_rx_wrapper_channels_and_queue_room(dev, seed):
    """batch.udp_rx on every seed: channel(k) is a spans batch of the model's
    payloads, and taken(k, room) the datagrams the channel's queue accepts."""
    c, ip, status, off = _bucket(dev.index, seed)
    ports = _ports(dev.index, 252)
    r = batch.udp_rx(ip, status, ports, HOST)
    torch.cuda.synchronize()
    items = _atomic(c, 252)
    got = dict(cls=r.cls.cpu().numpy(), first=r.first.cpu().numpy().view(np.uint32),
               order=r.order.cpu().numpy().view(np.uint32), pay_off=r.pay_off.cpu().numpy().view(np.uint64),
               pay_len=r.pay_len.cpu().numpy().view(np.uint32), src=r.src_all.cpu().numpy().view(np.uint32),
               sport=r.sport_all.cpu().numpy().view(np.uint16))
    want = check_rx(got, items, 252, off)
    data = ip.data.cpu().numpy()
    accepted = udp_model.queue([it["cls"] for it in items], 252, [udp_traffic.room_for(k) for k in range(252)])
    overflowed = 0
    for k in range(252):
        ch = r.channel(k)
        mine = [j for j in want["pos"] if items[j]["cls"] == k]
        assert ch.n == r.count(k) == len(mine)
        o, ln = ch.off.cpu().numpy(), ch.length.cpu().numpy()
        for j, a, m in zip(mine, o.tolist(), ln.tolist()):
            assert data[a:a + m].tobytes() == items[j]["payload"], (k, j)
        took = r.taken(k, udp_traffic.room_for(k))
        assert mine[:took] == accepted[k]
        overflowed += took < len(mine)
        assert r.src(k).cpu().numpy().view(np.uint32).tolist() == [items[j]["src"] for j in mine]
        assert r.sport(k).cpu().numpy().view(np.uint16).tolist() == [items[j]["sport"] for j in mine]
        assert r.indices(k).cpu().numpy().tolist() == mine
    assert overflowed >= 2 and r.taken(0) == 1024 and r.count(251) == 0
    if seed == 0:
        sums = batch.spans(r.channel(0))     # a bucket's slices are a spans batch as they stand
        torch.cuda.synchronize()
        mine = [j for j in want["pos"] if items[j]["cls"] == 0]
        assert batch.as_u16(sums).view(np.uint8).reshape(-1, 2).tolist() == \
            [list(sm.csum(items[j]["payload"]).to_bytes(2, "big")) for j in mine]


def test_udp_rx_one_channel_and_all_dropped(dev):
    """Through d_index: only the hot channel's frames with that one channel
    bound, and only frames the layer drops."""
    c, ip, status, off = _bucket(dev.index, 1)
    items = _atomic(c, 1)
    hot = np.array([j for j, it in enumerate(items) if it["cls"] == 0], dtype=np.uint32)
    rest = np.array([j for j, it in enumerate(items) if it["cls"] != 0], dtype=np.uint32)
    assert hot.size > 1024 and rest.size > 700
    for index in (hot, rest):
        got = run_udp_rx(dev, ip, ip.n, status, _ports(dev.index, 1), index=_u32_dev(dev, index))
        want = check_rx(got, [items[int(j)] for j in index], 1, off, index)
        assert want["first"].tolist() in ([0, hot.size, hot.size], [0, 0, rest.size])
    got = run_udp_rx(dev, ip, ip.n, status, _ports(dev.index, 0), index=_u32_dev(dev, hot))
    check_rx(got, [dict(DROPPED, cls=NOPORT)] * hot.size, 0, off, hot)   # no channel at all: nothing has a port
    assert got["first"].tolist() == [0, hot.size]


@pytest.mark.parametrize("nch", [2, 252])
def test_udp_rx_index_slices(dev, nch):
    """A permuted and a strided slice of the batch as d_index, indices out of
    range among them, and a list longer than the batch."""
    c, ip, status, off = _bucket(dev.index, 2)
    items = _atomic(c, nch)
    rng = np.random.default_rng(nch)
    away = np.array([ip.n, ip.n + 1, 1 << 31, 0xFFFFFFFF], dtype=np.uint32)
    perm = rng.permutation(ip.n).astype(np.uint32)
    perm[[3, 64, 1023, 1024, -1]] = away[[0, 1, 2, 3, 0]]
    strided = np.concatenate([np.arange(5, ip.n, 3, dtype=np.uint32), away])
    twice = np.concatenate([perm, perm[::-1], away]).astype(np.uint32)
    for k, index in enumerate((perm, strided, twice, away)):
        got = run_udp_rx(dev, ip, ip.n, status, _ports(dev.index, nch), index=_u32_dev(dev, index), with_class=k != 1)
        call = [items[int(j)] if j < ip.n else DROPPED for j in index]
        check_rx(got, call, nch, off, index, with_class=k != 1)
    # the wrapper: a shard's slice of a grouped list
    r = batch.udp_rx(ip, status, _ports(dev.index, nch), HOST, index=_u32_dev(dev, strided))
    torch.cuda.synchronize()
    want = udp_traffic.expect_rx([items[int(j)] if j < ip.n else DROPPED for j in strided], nch, strided)
    assert np.array_equal(r.order.cpu().numpy().view(np.uint32), want["order"])
    assert np.array_equal(r.first.cpu().numpy().view(np.uint32), want["first"])


def _hand_batch(dev):
    """Frames at all 16 start alignments with ihl 5-15, to bound and unbound
    ports, some for another host, some with a wrong UDP checksum, frames
    outside the buffer in every way and one ending at the buffer's last byte."""
    rng = np.random.default_rng(5)
    packets, slot = [], 128
    for k in range(16 * 11 * 2):
        ihl = 5 + (k // 16) % 11
        dport = udp_traffic.PORTS[k % 7] if k % 5 else udp_traffic.UNBOUND[k % 3]
        dst = sm.OTHER_HOST if k % 13 == 4 else HOST
        s = udp_model.send(rng.integers(0, 256, k % 30, dtype=np.uint8).tobytes(), 4000 + k, dport, sm.ON_LINK[k % 5],
                           dst, 1500)
        l4 = s["zero"] if k % 9 == 2 else s["l4"]              # a zero field: "no checksum", L4_OK clear
        ip = sm.ip_header(4 * ihl + len(l4), k, 0, sm.UDP, sm.ON_LINK[k % 5], dst, ihl, bytes([1] * (4 * (ihl - 5))))
        packets.append(ip + l4)
    n = len(packets)
    off = np.arange(n, dtype=np.uint64) * np.uint64(slot) + (np.arange(n, dtype=np.uint64) % np.uint64(16))
    length = np.array([len(p) for p in packets], dtype=np.uint32)
    last = packets[7]
    bytes_len = int(off[-1]) + slot + len(last)
    buf = rng.integers(0, 256, bytes_len, dtype=np.uint8)
    for o, p in zip(off.tolist(), packets):
        buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
    buf[bytes_len - len(last):] = np.frombuffer(last, np.uint8)
    extra_off = [bytes_len - len(last), bytes_len - len(last) + 1, bytes_len + 1, 1 << 63, (1 << 64) - 8, bytes_len, 0]
    extra_len = [len(last), len(last), 40, 40, 40, 0, 0xFFFFFFFF]
    inside = [True] * n + [True, False, False, False, False, True, False]   # an empty frame at the end is inside
    packets += [last] + [None] * 6
    off = np.concatenate([off, np.array(extra_off, dtype=np.uint64)])
    length = np.concatenate([length, np.array(extra_len, dtype=np.uint32)])
    return packets, inside, batch.PacketBatch.from_host(buf, off, length, device=dev), off


def test_udp_rx_alignments_options_and_the_buffer_edge(dev):
    packets, inside, b, off = _hand_batch(dev)
    status = torch.empty(b.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(b, status=status)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert all(bool(s & native.ST_RANGE) != ok for s, ok in zip(st.tolist(), inside))
    pm = _port_map(7)
    ports = _ports(dev.index, 7)

    def items(host, need):
        out = []
        for p, s in zip(packets, st.tolist()):
            good = p is not None and (s & need) == need and not s & REJECT
            out.append(udp_model.atomic(p, good and (host == 0 or sm.be32(p, 16) == host), pm) if p is not None
                       else DROPPED)
        return out

    for host, need in ((HOST, NEED), (0, NEED), (HOST, NEED | native.ST_L4_OK), (sm.OTHER_HOST, NEED)):
        got = run_udp_rx(dev, b, b.n, status, ports, host=host, need=need)
        want = items(host, need)
        check_rx(got, want, 7, off)
        cls = [it["cls"] for it in want]
        assert {SKIP, NOPORT, 0, 6} <= set(cls) or host == sm.OTHER_HOST
    # with the L4 verify required the zero-field datagrams are skipped; with host 0 the other host's are taken
    assert sum(it["cls"] < 7 for it in items(0, NEED)) > sum(it["cls"] < 7 for it in items(HOST, NEED)) > \
        sum(it["cls"] < 7 for it in items(HOST, NEED | native.ST_L4_OK)) > 100
    assert items(HOST, NEED)[len(packets) - 7]["cls"] < 7       # the frame at the buffer's last byte is read
    # the array form of the model agrees on this batch too
    fast = udp_model.fast_rx(b.data.cpu().numpy(), b.bytes_len, off, b.length.cpu().numpy().view(np.uint32), st, NEED,
                             REJECT, HOST, udp_traffic.PORTS[:7])
    got = run_udp_rx(dev, b, b.n, status, ports)
    for name in ("cls", "first", "order", "pay_off", "pay_len", "src", "sport"):
        assert np.array_equal(got[name], fast[name]), name


def test_udp_rx_is_deterministic(dev):
    """Two runs into outputs at other addresses give identical bytes."""
    c, ip, status, _ = _bucket(dev.index, 3)
    a = run_udp_rx(dev, ip, ip.n, status, _ports(dev.index, 252))
    b = run_udp_rx(dev, ip, ip.n, status, _ports(dev.index, 252), shift=3)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def test_udp_rx_is_capturable(dev):
    """The three (four) launches replay from a graph: no allocation, no
    synchronisation inside the call."""
    c, ip, status, off = _bucket(dev.index, 3)
    ports = _ports(dev.index, 252)
    lib = native.load()
    n = ip.n
    outs = dict(cls=torch.empty(n, dtype=torch.uint8, device=dev), first=torch.empty(254, dtype=torch.int32, device=dev),
                order=torch.empty(n, dtype=torch.int32, device=dev), pay_off=torch.empty(n, dtype=torch.int64, device=dev),
                pay_len=torch.empty(n, dtype=torch.int32, device=dev), src=torch.empty(n, dtype=torch.int32, device=dev),
                sport=torch.empty(n, dtype=torch.int16, device=dev))
    ws = torch.empty(int(lib.sccsum_udp_rx_workspace(n)), dtype=torch.uint8, device=dev)

    def launch():
        rc = lib.sccsum_udp_rx(ip.data.data_ptr(), ip.bytes_len, ip.off.data_ptr(), ip.length.data_ptr(), n,
                               status.data_ptr(), NEED, REJECT, HOST, ports.handle, None, n, outs["cls"].data_ptr(),
                               outs["first"].data_ptr(), outs["order"].data_ptr(), outs["pay_off"].data_ptr(),
                               outs["pay_len"].data_ptr(), outs["src"].data_ptr(), outs["sport"].data_ptr(),
                               ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    launch()
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in outs.items()}
    assert np.array_equal(want["order"].cpu().numpy().view(np.uint32), udp_traffic.expect_rx(_atomic(c, 252), 252)["order"])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for v in outs.values():
        v.fill_(0x5A)
    ws.fill_(0xC3)
    g.replay()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert torch.equal(v, want[k]), k


# ---------------------------------------------------------------- udp_rx_reasm

def _reasm_outputs(r) -> dict:
    return dict(cls=r.cls.cpu().numpy(), first=r.first.cpu().numpy().view(np.uint32),
                order=r.order.cpu().numpy().view(np.uint32), pay_len=r.pay_len.cpu().numpy().view(np.uint32),
                src=r.src_all.cpu().numpy().view(np.uint32), sport=r.sport_all.cpu().numpy().view(np.uint16))


@pytest.mark.parametrize("seed", udp_traffic.SEEDS)
def test_udp_rx_reassembled_against_the_model(dev, seed):
    """The lists batch.reassemble builds from the seed's fragments (cut by the
    model's tx at MTU 68 and 576; the 576 keys overlap and are the host's):
    classes, order, lengths, sources, and the payload bytes behind +8."""
    c, ip, status, _ = _bucket(dev.index, seed)
    recs = batch.frag_records(ip, status, host_address=HOST, tag=seed)
    rr = batch.reassemble(recs)
    desc, first, off, length, seeds, max_len = rr.lists()
    l4_status = torch.empty(max(int(off.numel()), 1), dtype=torch.uint8, device=dev)
    batch.spans_desc(desc, first, off, length, max_len, seeds=seeds, status=l4_status)
    packed = rr.pack()
    torch.cuda.synchronize()
    d, _, pending, host_recs = rr.totals()
    assert d == len(c["delivered"]) >= 40 and host_recs > 0
    data, p_off, p_len = packed.data.cpu().numpy(), off.cpu().numpy(), length.cpu().numpy()
    for k, m in enumerate(c["delivered"]):
        assert data[int(p_off[k]):int(p_off[k]) + int(p_len[k])].tobytes() == m["data"], k
    for nch in (252, 3, 0):
        pm = _port_map(nch)
        items = [udp_model.reassembled(m, pm) for m in c["delivered"]]
        r = batch.udp_rx_reassembled(rr, recs, _ports(dev.index, nch), HOST)
        torch.cuda.synchronize()
        want = check_rx(_reasm_outputs(r), items, nch)
        for j, n in zip(want["pos"], want["pay_len"].tolist()):
            if items[j]["cls"] < nch:                       # the payload is the datagram's layout bytes from +8
                a = int(p_off[j]) + 8
                assert data[a:a + n].tobytes() == items[j]["payload"], j
        assert r.pay_off is None
        with pytest.raises(ValueError, match="fragment lists"):
            r.channel(0)
    # with the L4 verify required: the datagrams whose checksum fails are skipped
    st = l4_status.cpu().numpy()[:d]
    assert [bool(s & native.ST_OK) for s in st.tolist()] == [m["l4_ok"] for m in c["delivered"]]
    pm = _port_map(252)
    items = [udp_model.reassembled(m, pm) if m["l4_ok"] else DROPPED for m in c["delivered"]]
    r = batch.udp_rx_reassembled(rr, recs, _ports(dev.index, 252), HOST, l4_status=l4_status[:d], need=native.ST_OK,
                                 reject=native.ST_RANGE)
    torch.cuda.synchronize()
    check_rx(_reasm_outputs(r), items, 252)
    # for another host nothing is ours
    r = batch.udp_rx_reassembled(rr, recs, _ports(dev.index, 252), sm.OTHER_HOST)
    torch.cuda.synchronize()
    assert set(r.cls.cpu().numpy().tolist()) == {SKIP}


def _cuts():
    """(E, piece lengths): the header cut at every position 1-7, over 2-8
    descriptors, E = 7, 8 and 9 and longer ones."""
    out = []
    for e in (8, 9, 40):
        for c in range(1, 8):
            out.append((e, [c, e - c]))                       # the cut at c
        for k in range(2, 9):
            head = [1] * (k - 1)
            if e - (k - 1) > 0:
                out.append((e, head + [e - (k - 1)]))         # k descriptors: k - 1 single bytes, then the rest
    out += [(40, [1, 2, 1, 3, 1, 20, 12]), (40, [7, 1, 32]), (9, [1] * 9), (7, [7]), (7, [3, 4]), (0, []), (1, [1]),
            (8, [8]), (9, [9]), (200, [200])]
    return out


def test_udp_rx_reasm_hand_built_lists(dev):
    """Lists written by hand: every cut of the 8 header bytes, datagrams
    shorter than the header, other hosts and protocols, a head index past the
    records, and lists that do not hold the header (never read past their own
    end)."""
    lib = native.load()
    rng = np.random.default_rng(11)
    pm = _port_map(5)
    ports = _ports(dev.index, 5)
    pool = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    base = pool.data_ptr()
    pool_h = np.zeros(1 << 16, dtype=np.uint8)
    src_a, dst_o, ln, dfirst, doff, dlen, dhead, items, recs = [], [], [], [0], [], [], [], [], []
    at, layout = 0, 5000

    def add(e, pieces, dport=None, proto=sm.UDP, dst=HOST, head_ok=True, want=None, claim=None, advance=True):
        nonlocal at, layout
        dport = udp_traffic.PORTS[len(items) % 5] if dport is None else dport
        body = (udp_model.send(rng.integers(0, 256, max(e - 8, 0), dtype=np.uint8).tobytes(), 3000 + len(items), dport,
                               sm.ON_LINK[0], dst, 1500)["l4"] + bytes(8))[:e]
        pos = 0
        for p in pieces:
            at += int(rng.integers(0, 9))                      # the pieces lie apart, at any alignment
            pool_h[at:at + p] = np.frombuffer(body[pos:pos + p], np.uint8)
            src_a.append(base + at)
            dst_o.append((layout + pos) & 0xFFFFFFFF)
            ln.append(p)
            at += p
            pos += p
        dfirst.append(len(src_a))
        doff.append(layout)
        dlen.append(e if claim is None else claim)
        dhead.append(len(recs) if head_ok else 1 << 20)
        recs.append((sm.ON_LINK[0] + len(items), dst, proto))
        layout += pos + 3 if advance else 0
        m = dict(proto=proto, src=recs[-1][0], dst=dst, data=body)
        items.append(udp_model.reassembled(m, pm) if want is None and dst == HOST else dict(DROPPED, cls=want or SKIP))

    for e, pieces in _cuts():
        add(e, pieces)
    add(30, [2, 28], dport=udp_traffic.UNBOUND[0])
    add(30, [5, 25], proto=sm.TCP)
    add(30, [5, 25], dst=sm.OTHER_HOST)
    add(30, [4, 26], head_ok=False, want=SKIP)
    add(5, [2, 3], claim=30, want=SKIP)                       # the list ends before the header does
    add(30, [1, 1, 1, 1, 1, 1, 1, 0, 23], want=SKIP)          # an empty descriptor: the header is past the eighth
    # no descriptor at all; the next list starts at the same layout position, and is not read for this one
    add(0, [], claim=12, want=SKIP, advance=False)
    add(30, [8, 22])
    layout = (1 << 32) + 77                                   # a layout position past 2^32: dst_off is its low half
    add(20, [3, 17])
    assert {SKIP, SHORT, NOPORT, 0, 4} <= {it["cls"] for it in items}
    m = len(items)
    pool.copy_(torch.from_numpy(pool_h))
    rec = np.zeros(m, dtype=batch.REC_DTYPE)
    rec["src"], rec["dst"], rec["proto"] = [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]
    d_rec = _dev(dev, rec.view(np.uint8))
    d_desc = _dev(dev, batch.make_desc(src_a, dst_o, ln).view(np.uint8))
    d_first, d_off = _u32_dev(dev, dfirst), _u64_dev(dev, doff)
    d_len, d_head = _u32_dev(dev, dlen), _u32_dev(dev, dhead)
    outs = []
    for shift in (0, 2):
        cls = Out(dev, m, torch.uint8, 0xA5, shift)
        first = Out(dev, 7, torch.int32, -7, shift)
        order = Out(dev, m, torch.int32, -7, shift)
        pay_len = Out(dev, m, torch.int32, -7, shift)
        src = Out(dev, m, torch.int32, -7, shift)
        sport = Out(dev, m, torch.int16, -7, shift)
        ws = Out(dev, int(lib.sccsum_udp_rx_reasm_workspace(m)) // 16, torch.complex128, 3.0, shift)
        rc = lib.sccsum_udp_rx_reasm(d_desc.data_ptr(), d_first.data_ptr(), d_off.data_ptr(), d_len.data_ptr(),
                                     d_head.data_ptr(), m, d_rec.data_ptr(), m, None, 0, 0, HOST, ports.handle, cls.ptr,
                                     first.ptr, order.ptr, pay_len.ptr, src.ptr, sport.ptr, ws.ptr,
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        ws.host()
        outs.append(dict(cls=cls.host(), first=first.host().view(np.uint32), order=order.host().view(np.uint32),
                         pay_len=pay_len.host().view(np.uint32), src=src.host().view(np.uint32),
                         sport=sport.host().view(np.uint16)))
    check_rx(outs[0], items, 5)
    for name in outs[0]:
        assert outs[0][name].tobytes() == outs[1][name].tobytes(), name       # two runs, identical bytes
    # m == 0 writes the closing entries
    first = Out(dev, 7, torch.int32, -7)
    ws = Out(dev, int(lib.sccsum_udp_rx_reasm_workspace(0)) // 16, torch.complex128, 3.0)
    assert lib.sccsum_udp_rx_reasm(None, None, None, None, None, 0, None, 0, None, 0, 0, HOST, ports.handle, None,
                                   first.ptr, None, None, None, None, ws.ptr,
                                   torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert first.host().tolist() == [0] * 7


# ---------------------------------------------------------------- udp_send

SEND_LENGTHS = list(range(65)) + [1472, 1473, 65507, 65508]


def _send_case(dev, seed: int):
    """Payloads of every length 0-64 and around the limits, each behind 8 bytes
    of headroom at any alignment; one at offset 8, one at offset 7, the last
    ending at the buffer's end, one past it."""
    rng = np.random.default_rng(300 + seed)
    lens = SEND_LENGTHS + [33, 20, 12]
    parts, off, at = [], [], 0
    for k, n in enumerate(lens[:-2]):
        gap = 8 + (k % 5 if k else 0)                  # payload 0 at offset 8: its headroom is the buffer's start
        parts.append(rng.integers(0, 256, gap + n, dtype=np.uint8))
        off.append(at + gap)
        at += gap + n
    buf = np.concatenate(parts)
    off.append(7)                                       # no room for the header
    off.append(buf.size - 5)                            # ends past the buffer
    assert off[0] == 8 and off[-3] + lens[-3] == buf.size   # the headroom at the buffer's start; ends at its last byte
    n = len(lens)
    dst = [(sm.ON_LINK + sm.OFF_LINK)[k % 8] for k in range(n)]
    dport = rng.integers(0, 65536, n).tolist()
    sport = rng.integers(0, 65536, n).tolist()
    ids = [(17 * k + seed) & 0xFFFF for k in range(n)]
    pay = batch.PacketBatch.from_host(buf, np.array(off, np.uint64), np.array(lens, np.uint32), device=dev)
    return buf, off, lens, dst, dport, sport, ids, pay


@pytest.mark.parametrize("mtu", [68, 576, 1500])
@pytest.mark.parametrize("flags", [0, native.UDP_CSUM_OFFLOAD, native.UDP_UFO, native.UDP_CSUM_OFFLOAD | native.UDP_UFO])
def test_udp_send_recipe_against_the_models(dev, flags, mtu):
    """udp_send -> spans -> ipv4_send(SEND_L4) -> eth_send -> pack(): the wire
    frames byte for byte against stack_model.tx fed by udp_model.send."""
    buf, off, lens, dst, dport, sport, ids, pay = _send_case(dev, mtu + flags)
    n = len(lens)
    offload, ufo = bool(flags & native.UDP_CSUM_OFFLOAD), bool(flags & native.UDP_UFO)
    d_dst = _u32_dev(dev, dst)
    u = batch.udp_send(pay, d_dst, _i16_dev(dev, dport), _i16_dev(dev, sport), HOST, mtu, flags)
    torch.cuda.synchronize()
    # what the call itself wrote: status, the headers in the headroom and nothing else
    status = [(native.ST_RANGE if o < 8 or o + ln > buf.size else 0) | (native.ST_MALFORMED if ln > 65507 else 0)
              for o, ln in zip(off, lens)]
    status = [s or native.ST_OK for s in status]
    assert status.count(native.ST_OK) == n - 3 and native.ST_MALFORMED in status
    assert u.status.cpu().numpy().tolist() == status
    model = [udp_model.send(buf[o:o + ln].tobytes(), sp, dp, HOST, d, mtu, offload, ufo) if s == native.ST_OK else None
             for o, ln, sp, dp, d, s in zip(off, lens, sport, dport, dst, status)]
    want = buf.copy()
    for o, m in zip(off, model):
        if m is not None:
            want[o - 8:o] = np.frombuffer(m["zero"][:8], np.uint8)
    assert np.array_equal(pay.data.cpu().numpy()[:buf.size], want), "the buffer after udp_send"
    ok = np.array([m is not None for m in model])
    assert u.l4.off.cpu().numpy().view(np.uint64).tolist() == [o - 8 if k else (1 << 64) - 1 for o, k in zip(off, ok)]
    assert u.l4.length.cpu().numpy().tolist() == [ln + 8 if k else 0 for ln, k in zip(lens, ok)]
    assert u.proto.cpu().numpy().tolist() == [17] * n
    needs = [bool(m and m["needs_csum"]) for m in model]
    assert u.needs_csum.cpu().numpy().astype(bool).tolist() == needs
    assert needs == [bool(k) and offload and (ufo or ln + 28 <= mtu) for ln, k in zip(lens, ok)]
    assert u.sum_batch.length.cpu().numpy().tolist() == [0 if (nc or not k) else ln + 8
                                                         for ln, k, nc in zip(lens, ok, needs)]
    seeds = [0 if not k else (0xFFFF ^ udp_model.pseudo_sum(HOST, d, ln + 8)) if nc else udp_model.pseudo_sum(HOST, d, ln + 8)
             for ln, d, k, nc in zip(lens, dst, ok, needs)]
    assert u.seeds.cpu().numpy().view(np.uint32).tolist() == seeds
    # the chain
    l4sum = batch.spans(u.sum_batch, seeds=u.seeds)
    r = batch.ipv4_send(u.l4, d_dst, u.proto, mtu, HOST, ids=_i16_dev(dev, ids), l4sum=l4sum,
                        flags=native.SEND_L4 | (native.SEND_UFO if ufo else 0))
    arp = {d: sm.peer_mac(d) for d in sm.ON_LINK}
    arp[sm.GW] = sm.GW_MAC
    table = batch.ArpTable(arp)
    e = batch.eth_send(r, d_dst, table, sm.HW, HOST, sm.NETMASK, sm.GW)
    wire = e.pack()
    torch.cuda.synchronize()
    assert r.status.cpu().numpy().tolist() == [native.ST_OK if k else native.ST_RANGE for k in ok]
    sent = pay.data.cpu().numpy()
    for o, m in zip(off, model):
        if m is not None:
            assert sent[o - 8:o - 8 + len(m["l4"])].tobytes() == m["l4"], "the datagram as sent"
    cfg = dict(host=HOST, netmask=sm.NETMASK, gw=sm.GW, hw=sm.HW, mtu=65535 if ufo else mtu, arp=arp)
    t = sm.tx([(m["zero"] if m else None, sm.UDP, d, i) for m, d, i in zip(model, dst, ids)], cfg)
    frames = list(t["frames"])
    for k, owner in enumerate(t["owner"]):
        if needs[owner]:                                   # never cut: the one frame carries the bare pseudo sum
            f = frames[k]
            frames[k] = f[:14 + 20 + 6] + model[owner]["l4"][6:8] + f[14 + 20 + 8:]
    data, w_off, w_len = wire.data.cpu().numpy(), wire.off.cpu().numpy(), wire.length.cpu().numpy()
    assert wire.n == len(frames) > n - 3 - 1
    for k, want_f in enumerate(frames):
        assert data[int(w_off[k]):int(w_off[k]) + int(w_len[k])].tobytes() == want_f, ("wire frame", k, t["owner"][k])
    if not ufo and mtu == 68:
        assert wire.n > 65507 // 48
    table.close()


def test_udp_send_is_deterministic_and_empty(dev):
    buf, off, lens, dst, dport, sport, ids, pay = _send_case(dev, 1)
    pay2 = batch.PacketBatch(data=pay.data.clone(), off=pay.off, length=pay.length, bytes_len=pay.bytes_len,
                             max_len=pay.max_len)
    args = (_u32_dev(dev, dst), _i16_dev(dev, dport), _i16_dev(dev, sport), HOST, 576, native.UDP_CSUM_OFFLOAD)
    a, b = batch.udp_send(pay, *args), batch.udp_send(pay2, *args)
    torch.cuda.synchronize()
    assert torch.equal(pay.data, pay2.data)
    for x, y in ((a.l4.off, b.l4.off), (a.l4.length, b.l4.length), (a.sum_batch.length, b.sum_batch.length),
                 (a.seeds, b.seeds), (a.needs_csum, b.needs_csum), (a.status, b.status), (a.proto, b.proto)):
        assert torch.equal(x, y)
    none = batch.PacketBatch(data=pay.data, off=pay.off[:0], length=pay.length[:0], bytes_len=pay.bytes_len, max_len=0)
    z = torch.zeros(0, dtype=torch.int16, device=dev)
    r = batch.udp_send(none, torch.zeros(0, dtype=torch.int32, device=dev), z, z, HOST, 1500)
    assert r.l4.n == 0 and r.status.numel() == 0


# ---------------------------------------------------------------- loopback

@pytest.mark.parametrize("seed,mtu", [(0, 68), (1, 1500), (2, 108), (3, 68)])
def test_loopback_device_tx_into_device_rx(dev, seed, mtu):
    """udp_send ... eth_send ... pack() into eth_rx, the frames call,
    reassembly and both udp_rx forms: every payload comes back with its
    channel, source address and source port."""
    rng = np.random.default_rng(900 + seed)
    n = 300
    lens = rng.integers(0, 600, n).tolist()
    parts, off, at = [], [], 0
    for ln in lens:
        parts.append(rng.integers(0, 256, 8 + ln, dtype=np.uint8))
        off.append(at + 8)
        at += 8 + ln
    buf = np.concatenate(parts)
    dsts = [sm.ON_LINK[k % 4] for k in range(n)]           # the device plays every receiving host: host_address 0
    chans = rng.integers(0, 40, n).tolist()
    dport = [udp_traffic.PORTS[k] for k in chans]
    sport = rng.integers(0, 65536, n).tolist()
    pay = batch.PacketBatch.from_host(buf, np.array(off, np.uint64), np.array(lens, np.uint32), device=dev)
    d_dst = _u32_dev(dev, dsts)
    u = batch.udp_send(pay, d_dst, _i16_dev(dev, dport), _i16_dev(dev, sport), HOST, mtu)
    l4sum = batch.spans(u.sum_batch, seeds=u.seeds)
    ids = _i16_dev(dev, [(seed * 1000 + k) & 0xFFFF for k in range(n)])
    r = batch.ipv4_send(u.l4, d_dst, u.proto, mtu, HOST, ids=ids, l4sum=l4sum, flags=native.SEND_L4)
    table = batch.ArpTable({d: sm.peer_mac(d) for d in sm.ON_LINK})
    wire = batch.eth_send(r, d_dst, table, sm.HW, HOST, sm.NETMASK, sm.GW).pack()
    want = sorted((c, sp, HOST, buf[o:o + ln].tobytes()) for c, sp, o, ln in zip(chans, sport, off, lens))
    # rx
    rx = batch.eth_rx(wire, (sm.IPV4, sm.ARP))
    ip = rx.bucket(0)
    status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(ip, status=status)
    ports = _ports(dev.index, 40)
    got = []
    ra = batch.udp_rx(ip, status, ports, 0, need=NEED | native.ST_L4_OK)
    recs = batch.frag_records(ip, status, host_address=0, tag=1)
    rr = batch.reassemble(recs)
    desc, first, d_off, d_len, seeds, max_len = rr.lists()
    if int(d_off.numel()):
        l4_status = torch.empty(int(d_off.numel()), dtype=torch.uint8, device=dev)
        batch.spans_desc(desc, first, d_off, d_len, max_len, seeds=seeds, status=l4_status)
        rb = batch.udp_rx_reassembled(rr, recs, ports, 0, l4_status=l4_status, need=native.ST_OK)
    else:
        rb = batch.udp_rx_reassembled(rr, recs, ports, 0)     # nothing was cut: the closing entries alone
    packed = rr.pack()
    torch.cuda.synchronize()
    assert rr.totals()[2:] == (0, 0)
    data = ip.data.cpu().numpy()
    for k in range(40):
        ch = ra.channel(k)
        for a, m, s, p in zip(ch.off.cpu().tolist(), ch.length.cpu().tolist(),
                              ra.src(k).cpu().numpy().view(np.uint32).tolist(),
                              ra.sport(k).cpu().numpy().view(np.uint16).tolist()):
            got.append((k, p, s, data[a:a + m].tobytes()))
    pdata, p_off = packed.data.cpu().numpy(), d_off.cpu().numpy()
    for k in range(40):
        for d, m, s, p in zip(rb.indices(k).cpu().tolist(), rb.payload_len(k).cpu().tolist(),
                              rb.src(k).cpu().numpy().view(np.uint32).tolist(),
                              rb.sport(k).cpu().numpy().view(np.uint16).tolist()):
            a = int(p_off[d]) + 8
            got.append((k, p, s, pdata[a:a + m].tobytes()))
    assert ra.count(40) == ip.n - ra.bounds()[40] and rb.count(40) == 0
    cut = sum(1 for ln in lens if ln + 8 + 20 > mtu)
    assert int(rb.bounds()[40]) == cut and (cut > 100 or mtu == 1500)
    assert sorted(got) == want
    table.close()


def test_cpp_classes_on_gpu(tmp_path):
    """Native host program (tests/cpp/udp_gpu.cc): udp_ports, udp_rx and udp_tx
    each against the C call it forwards to, on the same inputs into separately
    poisoned outputs; every array byte-equal."""
    exe = str(tmp_path / "udp_gpu")
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "udp_gpu.cc"), "-L", lib_dir, "-lsccsum", "-Wl,-rpath," + lib_dir,
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
    print(r.stdout)
