"""The TCP layer on the device (sccsum_tcp_rx, sccsum_tcp_send), compared with
the per-segment model (tests/tcp_model.py on top of tests/stack_model.py).
Every raw call writes into outputs with guard words on both sides; every
comparison is exact, nothing has a tolerance.

The sort key built is the suggested one (the connection index, then nconns + 0
/ 1 / 2 for the other buckets), so the table sizes 253 / 254 and 65 533 /
65 534 lie on both sides of the one / two and two / three pass boundaries."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import stack_model as sm
import tcp_model as tm
import tcp_traffic
from seastar_amd import batch, native
from test_gpu_eth import Out, _dev, _u32_dev

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = sm.HOST
NEED, REJECT = batch.TCP_NEED, batch.TCP_REJECT
FULL = tcp_traffic.FULL
SKIPPED = dict(cls=tm.SKIP, conn=tm.NO_CONN, hdr=None, H=0, pay_len=0, src=0, dst=0, at=0)
NAMES = ("cls", "first", "order", "seg", "src", "run_conn", "run_first", "rst", "rst_dst", "total")


def _i16_dev(dev, a) -> torch.Tensor:
    return _dev(dev, np.asarray(a, dtype=np.uint16).view(np.int16))


@functools.lru_cache(maxsize=None)
def _conns(dev_index: int, nconns: int, listen=tcp_traffic.LISTEN) -> batch.TcpConns:
    return batch.TcpConns(tcp_traffic.conn_array(nconns), listen, device=dev_index)


@functools.lru_cache(maxsize=None)
def _items(name, nconns: int, need: int = NEED) -> list:
    return tcp_traffic.items(tcp_traffic.case(name), nconns, need)


# ---------------------------------------------------------------- tcp_rx: one raw call

def run_tcp_rx(dev, b: batch.PacketBatch, nbatch: int, status, conns, index=None, n=None, need=NEED, reject=REJECT,
               host=HOST, flags=0, with_class=True, shift=0) -> dict:
    """sccsum_tcp_rx on the first nbatch frames of b into guarded outputs; returns their host copies."""
    lib = native.load()
    n = (nbatch if index is None else int(index.numel())) if n is None else n
    runs = min(n, conns.nconns) + 1
    cls = Out(dev, n, torch.uint8, 0xA5, shift)
    first = Out(dev, 5, torch.int32, -7, shift)
    order = Out(dev, n, torch.int32, -7, shift)
    seg = Out(dev, 4 * n, torch.int64, -7, shift)
    src = Out(dev, n, torch.int32, -7, shift)
    run_conn = Out(dev, runs, torch.int32, -7, shift)
    run_first = Out(dev, runs, torch.int32, -7, shift)
    rst = Out(dev, 5 * n, torch.int32, -7, shift)
    rst_dst = Out(dev, n, torch.int32, -7, shift)
    total = Out(dev, 4, torch.int64, -7, shift)
    ws = Out(dev, int(lib.sccsum_tcp_rx_workspace(n, conns.nconns)) // 16, torch.complex128, 3.0, shift)
    assert ws.ptr % 16 == 0
    some = nbatch > 0
    rc = lib.sccsum_tcp_rx(b.data.data_ptr(), b.bytes_len, b.off.data_ptr() if some else None,
                           b.length.data_ptr() if some else None, nbatch, status.data_ptr() if some else None, need,
                           reject, host, conns.handle, None if index is None or n == 0 else index.data_ptr(), n, flags,
                           cls.ptr if with_class else None, first.ptr, order.ptr if n else None, seg.ptr if n else None,
                           src.ptr if n else None, run_conn.ptr if n else None, run_first.ptr,
                           rst.ptr if n else None, rst_dst.ptr if n else None, total.ptr, ws.ptr,
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.host()
    t = total.host().view(np.uint64)
    r, k = int(t[0]), int(t[1])
    assert r <= runs - 1 and k <= n
    return dict(cls=cls.host() if with_class else cls.host(0), first=first.host().view(np.uint32),
                order=order.host().view(np.uint32), seg=seg.host().view(tm.SEG_DTYPE), src=src.host().view(np.uint32),
                run_conn=run_conn.host(r).view(np.uint32), run_first=run_first.host(r + 1).view(np.uint32),
                rst=rst.host(5 * k).view(np.uint8), rst_dst=rst_dst.host(k).view(np.uint32), total=t)


def check_rx(got: dict, items: list, off, index=None, with_class=True, offload=False) -> dict:
    """Every output array against the per-segment results `items` (the call's order)."""
    want = tm.expect_rx(items, off, index, offload)
    for name in NAMES:
        if name != "cls" or with_class:
            assert np.array_equal(got[name], want[name]), name
    return want


@functools.lru_cache(maxsize=None)
def _bucket(dev_index: int, name, kind=None, n=0, nconns=0):
    """A wire batch's IPv4 bucket on the device as the recipe makes it (eth_rx,
    the frames call's status), and the model's view of the same frames."""
    dev = torch.device("cuda", dev_index)
    c = tcp_traffic.case(name, None if kind is None else tcp_traffic.pattern(kind, n, nconns))
    length = np.array([len(f) for f in c["frames"]], dtype=np.uint32)
    gaps = np.arange(length.size) % 5
    off = (np.cumsum(length + gaps, dtype=np.uint64) - length).astype(np.uint64)
    buf = np.zeros(int(off[-1] + length[-1]), dtype=np.uint8)
    for o, f in zip(off.tolist(), c["frames"]):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    wire = batch.PacketBatch.from_host(buf, off, length, device=dev)
    ip = batch.eth_rx(wire, (sm.IPV4, sm.ARP)).bucket(0)
    status = torch.empty(max(ip.n, 1), dtype=torch.uint8, device=dev)[:ip.n]
    batch.ipv4_frames(ip, status=status)
    torch.cuda.synchronize()
    assert ip.n == len(c["ip"])
    assert status.cpu().numpy().tolist() == [i["status"] for i in c["info"]]
    return c, ip, status, ip.off.cpu().numpy().view(np.uint64)


SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, FULL]
NCONNS = [0, 1, 253, 254, 65533, 65534]
RX_CASES = [(n, 254, True) for n in SIZES] + [(FULL, c, c % 2 == 0) for c in NCONNS] + \
    [(n, NCONNS[k % 6], k % 2 == 1) for k, n in enumerate(SIZES)]


@pytest.mark.parametrize("n,nconns,with_class", RX_CASES)
def test_tcp_rx_against_the_model(dev, n, nconns, with_class):
    """The first n frames of the mixed batch through tables of nconns
    connections: sizes around the wave and the tile, tables on both sides of
    the sort's pass boundaries; both reset forms."""
    c, ip, status, off = _bucket(dev.index, 0)
    assert ip.n >= FULL
    offload = nconns % 2 == 1
    got = run_tcp_rx(dev, ip, n, status, _conns(dev.index, nconns), with_class=with_class,
                     flags=native.TCP_CSUM_OFFLOAD if offload else 0)
    want = check_rx(got, _items(0, nconns)[:n], off, with_class=with_class, offload=offload)
    if n == FULL:
        counts = np.diff(want["first"].astype(np.int64))
        assert (counts[1:] > 50).all() and (counts[0] > 300 or nconns < 2)
        assert want["total"][1] > 100 and (want["total"][0] >= min(nconns, 6))


def test_tcp_rx_without_the_l4_verify_and_for_another_host(dev):
    """rx_csum_offload: need without ST_L4_OK takes the segment whose checksum
    fails; another host_address takes nothing of ours."""
    c, ip, status, off = _bucket(dev.index, 0)
    got = run_tcp_rx(dev, ip, ip.n, status, _conns(dev.index, 254), need=native.ST_OK)
    check_rx(got, _items(0, 254, native.ST_OK), off)
    assert (got["cls"] != np.array([it["cls"] for it in _items(0, 254)], dtype=np.uint8)).sum() >= 1
    got = run_tcp_rx(dev, ip, ip.n, status, _conns(dev.index, 254), host=sm.OTHER_HOST)
    assert sorted(x for x in got["cls"].tolist() if x != tm.SKIP) == [tm.LISTEN]     # the one frame sent to that host


PATTERNS = [("one", 1025, 254), ("one", 64, 1), ("each", 1025, 65534), ("each", 253, 253), ("descending", 1025, 65534),
            ("descending", 254, 254), ("interleaved", 1025, 65534), ("interleaved", 130, 254), ("twins", 1025, 253)]


@pytest.mark.parametrize("kind,n,nconns", PATTERNS)
def test_tcp_rx_traffic_patterns(dev, kind, n, nconns):
    """One connection taking the whole batch (a single run), every segment on
    its own connection (R = n; every connection of a small table hit),
    connections hit in descending order, interleaved arrivals whose order
    inside a connection shows in seq, and pairs of identical headers with
    payloads elsewhere, which must keep the call's order."""
    name = (kind, n, nconns)
    c, ip, status, off = _bucket(dev.index, name, kind, n, nconns)
    got = run_tcp_rx(dev, ip, n, status, _conns(dev.index, nconns))
    items = _items(name, nconns)
    assert all(it["cls"] == tm.CONN for it in items)
    want = check_rx(got, items, off)
    r = int(got["total"][0])
    assert got["first"].tolist() == [0, n, n, n, n]
    if kind == "one":
        assert r == 1 and got["order"].tolist() == list(range(n))
    if kind == "each":
        assert r == n and got["run_first"].tolist() == list(range(n + 1))
        assert nconns != 253 or got["run_conn"].tolist() == list(range(253))
    if kind == "descending":
        assert got["order"].tolist() == list(range(n - 1, -1, -1))
    if kind == "interleaved":
        assert r == 4
        for k in range(4):
            a, e = got["run_first"][k], got["run_first"][k + 1]
            assert (np.diff(got["seg"]["seq"][a:e].astype(np.int64)) == 1).all()
    if kind == "twins":
        assert r == 3
        for k in range(3):
            a, e = got["run_first"][k], got["run_first"][k + 1]
            assert (np.diff(got["order"][a:e].astype(np.int64)) > 0).all()
            assert len(set(got["seg"]["seq"][a:e].tolist())) == 1
            assert (np.diff(got["seg"]["pay_off"][a:e].astype(np.int64)) > 0).all()
    assert want["pos"] == [int(x) for x in got["order"]]


@pytest.mark.parametrize("nconns", [254, 65534])
def test_tcp_rx_index_slices(dev, nconns):
    """A permuted, a strided and a repeated slice of the batch as d_index,
    indices out of range among them, and a list longer than the batch."""
    c, ip, status, off = _bucket(dev.index, 0)
    items = _items(0, nconns)
    rng = np.random.default_rng(nconns)
    away = np.array([ip.n, ip.n + 1, 1 << 31, 0xFFFFFFFF], dtype=np.uint32)
    perm = rng.permutation(ip.n).astype(np.uint32)
    perm[[3, 64, 1023, 1024, -1]] = away[[0, 1, 2, 3, 0]]
    strided = np.concatenate([np.arange(5, ip.n, 3, dtype=np.uint32), away])
    twice = np.concatenate([perm, perm[::-1], away]).astype(np.uint32)
    for k, index in enumerate((perm, strided, twice, away)):
        got = run_tcp_rx(dev, ip, ip.n, status, _conns(dev.index, nconns), index=_u32_dev(dev, index), with_class=k != 1)
        call = [items[int(j)] if j < ip.n else SKIPPED for j in index]
        check_rx(got, call, off, index, with_class=k != 1)
    # the wrapper: a shard's slice of a grouped list
    r = batch.tcp_rx(ip, status, _conns(dev.index, nconns), HOST, index=_u32_dev(dev, strided))
    torch.cuda.synchronize()
    want = tm.expect_rx([items[int(j)] if j < ip.n else SKIPPED for j in strided], off, strided)
    assert np.array_equal(r.order.cpu().numpy().view(np.uint32), want["order"])
    assert np.array_equal(r.first.cpu().numpy().view(np.uint32), want["first"])
    assert np.array_equal(r.seg.cpu().numpy().reshape(-1).view(tm.SEG_DTYPE), want["seg"])
    run_conn, run_first = r.runs()
    assert np.array_equal(run_conn.cpu().numpy().view(np.uint32), want["run_conn"])
    assert np.array_equal(run_first.cpu().numpy().view(np.uint32), want["run_first"])
    for k in (0, len(want["run_conn"]) - 1):
        a, e = want["run_first"][k], want["run_first"][k + 1]
        assert np.array_equal(r.segs(k).cpu().numpy().reshape(-1).view(tm.SEG_DTYPE), want["seg"][a:e])
    l4, dst = r.resets
    k = int(want["total"][1])
    assert l4.n == k > 10 and np.array_equal(dst.cpu().numpy().view(np.uint32), want["rst_dst"])
    assert np.array_equal(l4.data.cpu().numpy()[:20 * k], want["rst"])
    assert l4.off.cpu().tolist() == [20 * j for j in range(k)] and set(l4.length.cpu().tolist()) == {20}
    assert r.taken(0) == 0 and r.taken(59) == 2 and r.taken(60) == 3 and r.taken(1 << 30) == k
    with pytest.raises(ValueError, match="conn_run"):
        r.segs(len(want["run_conn"]))


def _hand_batch(dev):
    """Packets (no Ethernet header) at all 16 start alignments with ihl 5-15
    and H 20-60, to connections, listeners and closed ports, frames outside the
    buffer in every way and one ending at the buffer's last byte."""
    rng = np.random.default_rng(5)
    packets, slot = [], 192
    for k in range(16 * 11 * 2):
        ihl = 5 + (k // 16) % 11
        optlen = 4 * ((k // 3) % 11)
        opts = rng.integers(0, 256, optlen, dtype=np.uint8).tobytes()
        pay = rng.integers(0, 256, k % 23, dtype=np.uint8).tobytes()
        if k % 5 == 3:
            s, d, l4 = sm.ON_LINK[k % 5], HOST, tcp_traffic.segment(sm.ON_LINK[k % 5], HOST, 4000 + k, (80, 443)[k % 8 == 3],
                                                                  seq=k, ack=3 * k, flags=(tm.SYN, tm.ACK, tm.RST)[k % 3],
                                                                  options=opts, payload=pay)
        else:
            s, d, l4 = tcp_traffic.to_conn(k % 40, seq=k, ack=7 * k, flags=k % 64, options=opts, payload=pay, window=k)
        if k % 13 == 4:
            d = sm.OTHER_HOST
        packets.append(sm.ip_header(4 * ihl + len(l4), k, 0, sm.TCP, s, d, ihl, bytes([1] * (4 * (ihl - 5)))) + l4)
    n = len(packets)
    off = np.arange(n, dtype=np.uint64) * np.uint64(slot) + (np.arange(n, dtype=np.uint64) % np.uint64(16))
    length = np.array([len(p) for p in packets], dtype=np.uint32)
    last = packets[6]
    bytes_len = int(off[-1]) + slot + len(last)
    buf = rng.integers(0, 256, bytes_len, dtype=np.uint8)
    for o, p in zip(off.tolist(), packets):
        buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
    buf[bytes_len - len(last):] = np.frombuffer(last, np.uint8)
    extra_off = [bytes_len - len(last), bytes_len - len(last) + 1, bytes_len + 1, 1 << 63, (1 << 64) - 8, bytes_len, 0]
    extra_len = [len(last), len(last), 40, 40, 40, 0, 0xFFFFFFFF]
    packets += [last] + [None] * 6
    off = np.concatenate([off, np.array(extra_off, dtype=np.uint64)])
    length = np.concatenate([length, np.array(extra_len, dtype=np.uint32)])
    return packets, batch.PacketBatch.from_host(buf, off, length, device=dev), off


def test_tcp_rx_alignments_options_and_the_buffer_edge(dev):
    packets, b, off = _hand_batch(dev)
    status = torch.empty(b.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(b, status=status)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    table = tcp_traffic.tcbs(40)

    def items(host):
        out = []
        for p, s in zip(packets, st.tolist()):
            info = dict(status=s, delivered=p is not None and (host == 0 or sm.be32(p, 16) == host))
            out.append(SKIPPED if p is None else tm.atomic(p, info, table, tcp_traffic.LISTEN))
        return out

    for host in (HOST, 0, sm.OTHER_HOST):
        got = run_tcp_rx(dev, b, b.n, status, _conns(dev.index, 40), host=host)
        want = items(host)
        check_rx(got, want, off)
        if host != sm.OTHER_HOST:
            conn = [(p[0] & 0xF, it["H"], int(o) % 16) for p, it, o in zip(packets, want, off) if it["cls"] == tm.CONN]
            assert {c[0] for c in conn} == set(range(5, 16)) and {c[1] for c in conn} == set(range(20, 61, 4))
            assert {c[2] for c in conn} == set(range(16))
            assert len({it["hdr"]["flags"] for it in want if it["cls"] == tm.CONN}) >= 60
            assert {tm.CONN, tm.LISTEN, tm.RESET, tm.NOCONN, tm.SKIP} <= {it["cls"] for it in want}
    assert items(HOST)[len(packets) - 7]["cls"] == tm.CONN       # the frame at the buffer's last byte is read
    # the array form of the model agrees on this batch too
    fast = tm.fast_rx(b.data.cpu().numpy(), b.bytes_len, off, b.length.cpu().numpy().view(np.uint32), st, NEED, REJECT,
                      HOST, tcp_traffic.conn_array(40), tcp_traffic.LISTEN)
    got = run_tcp_rx(dev, b, b.n, status, _conns(dev.index, 40))
    for name in ("cls", "first", "order", "seg", "src", "run_conn", "run_first"):
        assert np.array_equal(got[name], fast[name]), name


def test_tcp_rx_colliding_table_and_listeners_only(dev):
    """A 2^17-slot table (65 536 connections) with a run of colliding keys that
    wraps past the last slot, and an empty table with listeners only."""
    lib = native.load()
    bits, nconns = 17, 1 << 16
    last = (1 << bits) - 1
    conns = tcp_traffic.conn_array(nconns)
    keys, b = [], 1
    while len(keys) < 12:                                  # twelve keys homed at the last two slots
        if lib.sccsum_tcp_conns_slot(HOST, 0x0C000000 + b, 8080, 5000, bits) >= last - 1:
            keys.append((HOST, 0x0C000000 + b, 8080, 5000))
        b += 1
    conns[:12] = keys
    variants = []                                          # not in the table: a key's foreign port changed, homed inside the run
    for lip, fip, lp, fp in keys:
        for q in range(1, 65536):
            if len(variants) < 6 and q != fp and lib.sccsum_tcp_conns_slot(lip, fip, lp, q, bits) >= last - 1:
                variants.append((lip, fip, lp, q))
    assert len(variants) >= 3
    t = batch.TcpConns(conns, tcp_traffic.LISTEN, device=dev.index)
    assert t.bits == bits and [t.lookup(*k) for k in keys] == list(range(12))
    table = {tuple(r): c for c, r in enumerate(conns.tolist())}
    frames = []
    for j in range(300):
        lip, fip, lp, fp = keys[j % 12] if j % 3 else tuple(conns[(j * 977) % nconns])
        if j % 10 == 9:
            fip += 0x01000000                              # a neighbour of the colliding keys: a miss, its port listens
        if j % 10 == 8:
            lip, fip, lp, fp = variants[j % len(variants)]
        frames.append(tcp_traffic.frame(fip, lip, tcp_traffic.segment(fip, lip, fp, lp, seq=j), ident=j))
    c = tcp_traffic.case("colliding", frames)
    c, ip, status, off = _bucket_of(dev, c)
    items = tcp_traffic.items(c, nconns, table=table)
    got = run_tcp_rx(dev, ip, ip.n, status, t)
    check_rx(got, items, off)
    assert sum(it["cls"] == tm.CONN and it["conn"] < 12 for it in items) > 150
    assert sum(it["cls"] == tm.LISTEN for it in items) >= 50
    t.close()
    # no connection at all: everything is the listeners' or answered
    c, ip, status, off = _bucket(dev.index, 0)
    got = run_tcp_rx(dev, ip, FULL, status, _conns(dev.index, 0))
    want = check_rx(got, _items(0, 0)[:FULL], off)
    assert want["first"][1] == 0 and want["total"][0] == 0 and got["run_first"].tolist() == [0]
    got = run_tcp_rx(dev, ip, FULL, status, _conns(dev.index, 0, ()))
    assert got["first"].tolist()[:3] == [0, 0, 0] and tm.LISTEN not in got["cls"].tolist()


def _bucket_of(dev, c):
    length = np.array([len(f) for f in c["frames"]], dtype=np.uint32)
    off = (np.cumsum(length + 3, dtype=np.uint64) - length).astype(np.uint64)
    buf = np.zeros(int(off[-1] + length[-1]), dtype=np.uint8)
    for o, f in zip(off.tolist(), c["frames"]):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    ip = batch.eth_rx(batch.PacketBatch.from_host(buf, off, length, device=dev), (sm.IPV4, sm.ARP)).bucket(0)
    status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(ip, status=status)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [i["status"] for i in c["info"]]
    return c, ip, status, ip.off.cpu().numpy().view(np.uint64)


def test_tcp_rx_is_deterministic(dev):
    """Two runs into outputs at other addresses give identical bytes."""
    c, ip, status, _ = _bucket(dev.index, 0)
    for nconns in (254, 65534):
        a = run_tcp_rx(dev, ip, ip.n, status, _conns(dev.index, nconns))
        b = run_tcp_rx(dev, ip, ip.n, status, _conns(dev.index, nconns), shift=3)
        for name in a:
            assert a[name].tobytes() == b[name].tobytes(), name


def test_tcp_rx_is_capturable(dev):
    """The launches replay from a graph: no allocation, no synchronisation inside the call."""
    c, ip, status, off = _bucket(dev.index, 0)
    conns = _conns(dev.index, 65534)
    lib = native.load()
    n = ip.n
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)  # noqa: E731
    outs = dict(cls=torch.empty(n, dtype=torch.uint8, device=dev), first=i32(5), order=i32(n),
                seg=torch.empty(4 * n, dtype=torch.int64, device=dev), src=i32(n), run_conn=i32(n + 1),
                run_first=i32(n + 1), rst=i32(5 * n), rst_dst=i32(n), total=torch.empty(4, dtype=torch.int64, device=dev))
    ws = torch.empty(int(lib.sccsum_tcp_rx_workspace(n, 65534)), dtype=torch.uint8, device=dev)

    def launch():
        rc = lib.sccsum_tcp_rx(ip.data.data_ptr(), ip.bytes_len, ip.off.data_ptr(), ip.length.data_ptr(), n,
                               status.data_ptr(), NEED, REJECT, HOST, conns.handle, None, n, 0,
                               *[outs[k].data_ptr() for k in ("cls", "first", "order", "seg", "src", "run_conn",
                                                              "run_first", "rst", "rst_dst", "total")],
                               ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    for v in outs.values():
        v.fill_(0x5A)
    launch()
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in outs.items()}
    exp = tm.expect_rx(_items(0, 65534), off)
    assert np.array_equal(want["order"].cpu().numpy().view(np.uint32), exp["order"])
    assert np.array_equal(want["seg"].cpu().numpy().view(tm.SEG_DTYPE), exp["seg"])
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


# ---------------------------------------------------------------- tcp_send

SEND_LENGTHS = list(range(65)) + [1459, 1460, 1461]


def _send_case(dev, seed: int, tso_flag: bool):
    """Payloads of every length 0-64, around 1 460 and around 65 515 - hdr_len,
    each behind hdr_len bytes of headroom (20-60, the options already there) at
    any alignment, mss below, at and above the length; one whose headroom is
    the buffer's start, the refusals, one ending at the buffer's last byte."""
    rng = np.random.default_rng(300 + seed)
    lens = SEND_LENGTHS + [65515 - 24 - 1, 65515 - 24, 65515 - 24 + 1, 5, 5, 5, 5, 5, 33, 20, 12]
    hdrs = [20 + 4 * (k % 11) for k in range(len(SEND_LENGTHS))] + [24, 24, 24, 22, 16, 64, 0, 20, 28, 20, 20]
    parts, off, at = [], [], 0
    for k, (n, h) in enumerate(zip(lens[:-2], hdrs[:-2])):
        gap = max(h, 20) + (k % 5 if k else 0)
        parts.append(rng.integers(0, 256, gap + n, dtype=np.uint8))
        off.append(at + gap)
        at += gap + n
    buf = np.concatenate(parts)
    off.append(19)                                      # no room for the header
    off.append(buf.size - 5)                            # ends past the buffer
    assert off[0] == hdrs[0] == 20 and off[-3] + lens[-3] == buf.size
    n = len(lens)
    mss = [(max(ln - 1, 1), max(ln, 1), ln + 1, 1460)[k % 4] for k, ln in enumerate(lens)]
    mss[len(SEND_LENGTHS) + 7] = 0                      # refused with TSO
    out = np.zeros(n, dtype=batch.TCP_OUT_DTYPE)
    out["dst"] = [(sm.ON_LINK + sm.OFF_LINK)[k % 8] for k in range(n)]
    out["seq"], out["ack"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n)
    out["sport"], out["dport"], out["window"] = (rng.integers(0, 65536, n) for _ in range(3))
    out["flags"], out["hdr_len"], out["mss"] = np.arange(n) * 5 % 256, hdrs, mss
    ids = [(17 * k + seed) & 0xFFFF for k in range(n)]
    pay = batch.PacketBatch.from_host(buf, np.array(off, np.uint64), np.array(lens, np.uint32), device=dev)
    status = [tm.send_status(o, ln, h, buf.size, tso_flag, m) or native.ST_OK for o, ln, h, m in zip(off, lens, hdrs, mss)]
    return buf, off, lens, out, ids, pay, status


@pytest.mark.parametrize("mtu", [68, 576, 1500])
@pytest.mark.parametrize("flags", [0, native.TCP_CSUM_OFFLOAD, native.TCP_TSO, native.TCP_CSUM_OFFLOAD | native.TCP_TSO])
def test_tcp_send_recipe_against_the_models(dev, flags, mtu):
    """tcp_send -> spans -> ipv4_send(SEND_L4) -> eth_send -> pack(): the wire
    frames byte for byte against stack_model.tx fed by tcp_model.send."""
    offload, tso = bool(flags & native.TCP_CSUM_OFFLOAD), bool(flags & native.TCP_TSO)
    buf, off, lens, out, ids, pay, status = _send_case(dev, mtu + flags, tso)
    n = len(lens)
    d_out = _dev(dev, out.view(np.uint8).reshape(n, 24))
    u = batch.tcp_send(pay, d_out, HOST, mtu, flags)
    torch.cuda.synchronize()
    bad = status.count(native.ST_MALFORMED) + status.count(native.ST_RANGE) + status.count(native.ST_RANGE | native.ST_MALFORMED)
    assert bad == (8 if tso else 7) and status.count(native.ST_OK) == n - bad
    assert u.status.cpu().numpy().tolist() == status
    model = []
    for k, (o, ln, s) in enumerate(zip(off, lens, status)):
        h = int(out["hdr_len"][k])
        rec = {f: int(out[f][k]) for f in ("dst", "seq", "ack", "sport", "dport", "window", "flags", "mss")}
        model.append(tm.send(buf[o:o + ln].tobytes(), rec, HOST, buf[o - h + 20:o].tobytes(), offload, tso)
                     if s == native.ST_OK else None)
    want = buf.copy()
    for k, (o, m) in enumerate(zip(off, model)):
        if m is not None:
            h = int(out["hdr_len"][k])
            want[o - h:o - h + 20] = np.frombuffer(m["zero"][:20], np.uint8)
            assert m["zero"][20:h] == buf[o - h + 20:o].tobytes()
    assert np.array_equal(pay.data.cpu().numpy()[:buf.size], want), "the buffer after tcp_send"
    ok = [m is not None for m in model]
    hl = out["hdr_len"].tolist()
    assert u.l4.off.cpu().numpy().view(np.uint64).tolist() == [o - h if k else (1 << 64) - 1 for o, h, k in zip(off, hl, ok)]
    assert u.l4.length.cpu().numpy().tolist() == [ln + h if k else 0 for ln, h, k in zip(lens, hl, ok)]
    assert u.proto.cpu().numpy().tolist() == [6] * n
    assert u.needs_csum.cpu().numpy().astype(bool).tolist() == [k and offload for k in ok]
    big = [bool(k) and offload and tso and ln > int(m) for ln, m, k in zip(lens, out["mss"].tolist(), ok)]
    assert u.tso_seg.cpu().numpy().view(np.uint16).tolist() == [int(m) & 0xFFFF if g else 0 for m, g in zip(out["mss"].tolist(), big)]
    assert [m["tso_seg"] if m else 0 for m in model] == [int(m) if g else 0 for m, g in zip(out["mss"].tolist(), big)]
    assert not (offload and tso) or (sum(big) > 15 and sum(ok) - sum(big) > 15)
    assert u.sum_batch.length.cpu().numpy().tolist() == [0 if (offload or not k) else ln + h for ln, h, k in zip(lens, hl, ok)]
    pseudo = [tm.pseudo_sum(HOST, int(d), 0 if g else ln + h) for d, ln, h, g in zip(out["dst"].tolist(), lens, hl, big)]
    assert u.seeds.cpu().numpy().view(np.uint32).tolist() == [0 if not k else (0xFFFF ^ p) if offload else p
                                                              for p, k in zip(pseudo, ok)]
    # the chain
    d_dst = _u32_dev(dev, out["dst"])
    l4sum = batch.spans(u.sum_batch, seeds=u.seeds)
    r = batch.ipv4_send(u.l4, d_dst, u.proto, mtu, HOST, ids=_i16_dev(dev, ids), l4sum=l4sum, flags=native.SEND_L4)
    arp = {d: sm.peer_mac(d) for d in sm.ON_LINK}
    arp[sm.GW] = sm.GW_MAC
    table = batch.ArpTable(arp)
    wire = batch.eth_send(r, d_dst, table, sm.HW, HOST, sm.NETMASK, sm.GW).pack()
    torch.cuda.synchronize()
    assert r.status.cpu().numpy().tolist() == [native.ST_OK if k else native.ST_RANGE for k in ok]
    sent = pay.data.cpu().numpy()
    for k, (o, m) in enumerate(zip(off, model)):
        if m is not None:
            assert sent[o - hl[k]:o - hl[k] + len(m["l4"])].tobytes() == m["l4"], "the segment as sent"
    cfg = dict(host=HOST, netmask=sm.NETMASK, gw=sm.GW, hw=sm.HW, mtu=mtu, arp=arp)
    t = sm.tx([(m["zero"] if m else None, sm.TCP, int(d), i) for m, d, i in zip(model, out["dst"].tolist(), ids)], cfg)
    frames = list(t["frames"])
    seen = set()
    for k, owner in enumerate(t["owner"]):
        if offload and owner not in seen:                  # the first piece carries the bare pseudo sum
            f = frames[k]
            frames[k] = f[:14 + 20 + 16] + model[owner]["l4"][16:18] + f[14 + 20 + 18:]
        seen.add(owner)
    data, w_off, w_len = wire.data.cpu().numpy(), wire.off.cpu().numpy(), wire.length.cpu().numpy()
    assert wire.n == len(frames) >= sum(ok)
    for k, want_f in enumerate(frames):
        assert data[int(w_off[k]):int(w_off[k]) + int(w_len[k])].tobytes() == want_f, ("wire frame", k, t["owner"][k])
    table.close()


def test_tcp_send_is_deterministic_and_empty(dev):
    buf, off, lens, out, ids, pay, status = _send_case(dev, 1, True)
    pay2 = batch.PacketBatch(data=pay.data.clone(), off=pay.off, length=pay.length, bytes_len=pay.bytes_len,
                             max_len=pay.max_len)
    d_out = _dev(dev, out.view(np.uint8).reshape(len(lens), 24))
    a, b = batch.tcp_send(pay, d_out, HOST, 576, 3), batch.tcp_send(pay2, d_out, HOST, 576, 3)
    torch.cuda.synchronize()
    assert torch.equal(pay.data, pay2.data)
    for x, y in ((a.l4.off, b.l4.off), (a.l4.length, b.l4.length), (a.sum_batch.length, b.sum_batch.length),
                 (a.seeds, b.seeds), (a.needs_csum, b.needs_csum), (a.status, b.status), (a.proto, b.proto),
                 (a.tso_seg, b.tso_seg)):
        assert torch.equal(x, y)
    none = batch.PacketBatch(data=pay.data, off=pay.off[:0], length=pay.length[:0], bytes_len=pay.bytes_len, max_len=0)
    r = batch.tcp_send(none, torch.zeros((0, 24), dtype=torch.uint8, device=dev), HOST, 1500)
    assert r.l4.n == 0 and r.status.numel() == 0


# ---------------------------------------------------------------- loopback

def _wire_to_rx(dev, wire):
    ip = batch.eth_rx(wire, (sm.IPV4, sm.ARP)).bucket(0)
    status = torch.empty(max(ip.n, 1), dtype=torch.uint8, device=dev)[:ip.n]
    batch.ipv4_frames(ip, status=status)
    return ip, status


def test_loopback_device_tx_into_device_rx(dev):
    """tcp_send ... eth_send ... pack() into eth_rx, the frames call and
    tcp_rx: every segment comes back on its connection, verified, with what
    was sent; and the device's resets, sent to a peer, class as NOCONN there."""
    rng = np.random.default_rng(77)
    n, nconns = 300, 40
    lens = rng.integers(0, 600, n).tolist()
    hdrs = [20 + 4 * (k % 11) for k in range(n)]
    parts, off, at = [], [], 0
    for ln, h in zip(lens, hdrs):
        parts.append(rng.integers(0, 256, h + ln, dtype=np.uint8))
        off.append(at + h)
        at += h + ln
    buf = np.concatenate(parts)
    conn = rng.integers(0, nconns, n)
    peers = [(sm.ON_LINK[c % 4], HOST, 2000 + c, 30000 + 7 * c) for c in range(nconns)]   # the peers' connids
    out = np.zeros(n, dtype=batch.TCP_OUT_DTYPE)
    out["dst"] = [peers[c][0] for c in conn]
    out["dport"], out["sport"] = [peers[c][2] for c in conn], [peers[c][3] for c in conn]
    out["seq"], out["ack"], out["window"] = np.arange(n), rng.integers(0, 1 << 32, n), rng.integers(0, 65536, n)
    out["flags"], out["hdr_len"], out["mss"] = rng.integers(0, 64, n), hdrs, 1460
    pay = batch.PacketBatch.from_host(buf, np.array(off, np.uint64), np.array(lens, np.uint32), device=dev)
    d_dst = _u32_dev(dev, out["dst"])
    u = batch.tcp_send(pay, _dev(dev, out.view(np.uint8).reshape(n, 24)), HOST, 1500)
    l4sum = batch.spans(u.sum_batch, seeds=u.seeds)
    r = batch.ipv4_send(u.l4, d_dst, u.proto, 1500, HOST, ids=_i16_dev(dev, np.arange(n)), l4sum=l4sum, flags=native.SEND_L4)
    table = batch.ArpTable({d: sm.peer_mac(d) for d in sm.ON_LINK})
    wire = batch.eth_send(r, d_dst, table, sm.HW, HOST, sm.NETMASK, sm.GW).pack()
    ip, status = _wire_to_rx(dev, wire)
    t = batch.TcpConns(peers, device=dev.index)
    rx = batch.tcp_rx(ip, status, t, 0)                       # the device plays every receiving host
    torch.cuda.synchronize()
    assert rx.bounds().tolist() == [0, n, n, n, n] and rx.totals() == (len(set(conn.tolist())), 0)
    seg = rx.seg.cpu().numpy().reshape(-1).view(tm.SEG_DTYPE)
    data = ip.data.cpu().numpy()
    assert set(rx.src_all.cpu().numpy().view(np.uint32).tolist()) == {HOST}
    order = rx.order.cpu().numpy()
    assert sorted(order.tolist()) == list(range(n))
    for p, j in enumerate(order.tolist()):                    # frame j is segment j: nothing was cut or dropped
        s = seg[p]
        assert (s["conn"], s["seq"], s["ack"], s["window"], s["flags"], s["hdr_len"], s["pay_len"]) == \
            (conn[j], j, out["ack"][j], out["window"][j], out["flags"][j], hdrs[j], lens[j])
        a = int(s["pay_off"])
        assert data[a:a + lens[j]].tobytes() == buf[off[j]:off[j] + lens[j]].tobytes()
        assert data[a - hdrs[j] + 20:a].tobytes() == buf[off[j] - hdrs[j] + 20:off[j]].tobytes()
    assert (np.diff(seg["conn"].astype(np.int64)) >= 0).all()
    t.close()
    # the resets of the mixed batch, on the wire and into a peer's tcp_rx
    c, mixed, mstatus, _ = _bucket(dev.index, 0)
    ans = batch.tcp_rx(mixed, mstatus, _conns(dev.index, 254), HOST)
    l4, dst = ans.resets
    k = l4.n
    assert k > 100
    proto = torch.full((k,), 6, dtype=torch.uint8, device=dev)
    r = batch.ipv4_send(l4, dst, proto, 1500, HOST, ids=_i16_dev(dev, np.arange(k)))
    wire = batch.eth_send(r, dst, table_for_resets(dev), sm.HW, HOST, sm.NETMASK, sm.GW).pack()
    ip, status = _wire_to_rx(dev, wire)
    peer = batch.TcpConns(device=dev.index)
    back = batch.tcp_rx(ip, status, peer, 0)
    torch.cuda.synchronize()
    assert ip.n == k and set(back.cls.cpu().tolist()) == {tm.NOCONN}         # verified (L4_OK), RST set: discarded
    assert back.bounds().tolist() == [0, 0, 0, 0, k] and back.totals() == (0, 0)
    peer.close()
    table.close()


def table_for_resets(dev):
    arp = {d: sm.peer_mac(d) for d in sm.ON_LINK}
    arp[sm.GW] = sm.GW_MAC
    return batch.ArpTable(arp)


def test_cpp_classes_on_gpu(tmp_path):
    """Native host program (tests/cpp/tcp_gpu.cc): tcp_conns, tcp_rx and tcp_tx
    each against the C call it forwards to, on the same inputs into separately
    poisoned outputs; every array byte-equal."""
    exe = str(tmp_path / "tcp_gpu")
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "tcp_gpu.cc"), "-L", lib_dir, "-lsccsum", "-Wl,-rpath," + lib_dir,
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tcp_gpu: OK" in r.stdout
    print(r.stdout)
