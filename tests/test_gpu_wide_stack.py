"""Every stack layer on frames that really lie at offsets past 2^31 / 2^32:
the traffic and the assertions of the layer tests (tests/test_gpu_stack.py,
test_gpu_udp.py, test_gpu_tcp.py, test_gpu_tcp_data.py, test_gpu_tcp_tx_data.py)
with the frames placed by tests/wide_layout.py in one device buffer of
W = 2^32 + 2^26 bytes.  The models do not depend on position, so the expected
values are theirs; every comparison is exact.

One byte belongs to one frame, so one layout holds one frame across each of
the three lines (offset 2^31, offset 2^32, the absolute 2^32 line); the tests
run every *variant* of the layout, which together put every header boundary of
a frame on every line (tests/test_wide_layout.py asserts that on the plans
below, without a device).  There is no host copy of the W bytes: what a test
reads back are the clusters it wrote, and small windows.

Not covered: a buffer crossing a 64 GiB-aligned address (a test cannot choose
where an allocation lands), and a packed output of more than 4 GiB (dst_off
is 32-bit by contract; the capacity cases at the end check the refusal)."""
import copy
import functools
import types

import numpy as np
import pytest
import torch

import stack_model as sm
import tcp_data_model as dm
import tcp_data_traffic as dtr
import tcp_model as tm
import tcp_traffic
import tcp_tx_fast as fast
import tcp_tx_traffic as ttr
import udp_model
import udp_traffic
import wide_layout as wl
from seastar_amd import batch, devsynth, native
from tcp_tx_model import Hw
from test_stack_model import modelled
from wide_layout import P31, P32, W

pytestmark = pytest.mark.gpu

HOST = sm.HOST
M32 = 0xFFFFFFFF
STACK_SEED = 2                      # the smallest case of stack_model.BATCH_SIZES: 1, one tile, 0 frames
RX_SLOTS = wl.slots()               # Ethernet frames: every boundary of FRAME_BYTES
UDP_TX_SLOTS = wl.slots(42, 8, extra=(-4,))     # payloads behind 8 bytes of headroom
TCP_TX_SLOTS = wl.slots(54, 60, extra=(-4,))    # payloads behind up to 60
BUF_SLOTS = wl.slots(54)            # tcp_tx_data's buffers: plain bytes


# ---------------------------------------------------------------- the plans: what is placed, host only

def _kind(f):
    if f is None or len(f) < 14:
        return "short"
    return (f[12:14], f[23] if f[12:14] == b"\x08\x00" and len(f) >= 34 else -1)


def _plan(frames, sub=()):
    return types.SimpleNamespace(frames=frames, lengths=[None if f is None else len(f) for f in frames],
                                 kinds=[_kind(f) for f in frames],
                                 prefer=[f is not None and len(f) >= 60 and f[12:14] == b"\x08\x00" for f in frames],
                                 sub=[np.asarray(s, np.int64) for s in sub])


@functools.lru_cache(maxsize=None)
def stack_plan():
    """The three wire batches of STACK_SEED in one layout; sub-batches: each wire batch and its IPv4 bucket."""
    batches, outs, _ = modelled(STACK_SEED)
    starts = np.concatenate([[0], np.cumsum([len(b) for b in batches])]).astype(np.int64)
    sub = [np.arange(starts[b], starts[b + 1]) for b in range(len(batches))]
    sub += [starts[b] + np.array(o["buckets"][0], np.int64) for b, o in enumerate(outs)]
    p = _plan([f for b in batches for f in b], sub)
    p.starts = starts
    return p


@functools.lru_cache(maxsize=None)
def udp_plan():
    frames = udp_traffic.case(0)["frames"]
    return _plan(frames, [np.arange(len(frames))])


@functools.lru_cache(maxsize=None)
def tcp_plan():
    frames = tcp_traffic.case(0)["frames"]
    return _plan(frames, [np.arange(len(frames))])


@functools.lru_cache(maxsize=None)
def tcp_data_plan():
    from test_gpu_tcp_data import _wire
    tcbs, frames = _wire(0)
    p = _plan(frames, [np.arange(len(frames))])
    p.tcbs = tcbs
    return p


def lay_of(plan, base, variant, slot_list=RX_SLOTS, **kw):
    return wl.place(plan.lengths, base, variant, slot_list, kinds=plan.kinds, prefer=plan.prefer, **kw)


# ---------------------------------------------------------------- the buffer

@pytest.fixture(scope="module")
def wide(dev):
    """W random bytes in HBM (generated there), shifted inside their allocation
    so that the absolute 2^32 line keeps apart from the offset lines."""
    g = torch.Generator(device=dev)
    g.manual_seed(0x57AC)
    raw = devsynth.random_bytes(W + wl.SLACK, g, dev)      # torch.empty inside: no room is an error, never a skip
    s = wl.base_shift(raw.data_ptr())
    data = raw[s:s + W]
    torch.cuda.synchronize()
    return types.SimpleNamespace(raw=raw, data=data, base=data.data_ptr(), dev=dev)


def _write(w, lay, frames, seed=0) -> list:
    """The layout's clusters into the buffer, one copy each; returns the images."""
    imgs = wl.images(lay, frames, seed)
    for a, img in imgs:
        w.data[a:a + img.size].copy_(torch.from_numpy(img))
    return imgs


def _t64(dev, a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(dev)


def _t32(dev, a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)


def _t16(dev, a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16).copy()).to(dev)


def _pb(w, off, length) -> batch.PacketBatch:
    length = np.asarray(length, np.uint32)
    return batch.PacketBatch(data=w.data, off=_t64(w.dev, off), length=_t32(w.dev, length), bytes_len=W,
                             max_len=int(length.max()) if length.size else 0)


class Reader:
    """A frame's bytes by their offset in the wide buffer, from the frames themselves."""

    def __init__(self, lay, frames):
        self.real = lay.real[np.argsort(lay.off[lay.real], kind="stable")]
        self.off, self.frames = lay.off[self.real].astype(np.int64), frames

    def __call__(self, o: int, n: int) -> bytes:
        k = int(np.searchsorted(self.off, o, side="right")) - 1
        f, at = self.frames[int(self.real[k])], o - int(self.off[k])
        assert 0 <= at and at + n <= len(f), (o, n)
        return f[at:at + n]


def _sides(addrs, lines) -> bool:
    """Do the offsets lie on both sides of one of the lines?"""
    return any(min(addrs) < X <= max(addrs) for X in lines)


def _laid(w, plan, variant, slot_list=RX_SLOTS, **kw):
    lay = lay_of(plan, w.base, variant, slot_list, **kw)
    wl.check(lay, plan.sub)
    return lay, _write(w, lay, plan.frames, variant)


def _ip_bucket(w, lay, info):
    """eth_rx and the frames call on the whole layout, as the layer tests' _bucket makes them."""
    wire = _pb(w, lay.off, lay.length)
    rx = batch.eth_rx(wire, (sm.IPV4, sm.ARP))
    ip = rx.bucket(0)
    status = torch.empty(max(ip.n, 1), dtype=torch.uint8, device=w.dev)[:ip.n]
    batch.ipv4_frames(ip, status=status)
    torch.cuda.synchronize()
    assert ip.n == len(info) and status.cpu().numpy().tolist() == [i["status"] for i in info]
    off = ip.off.cpu().numpy().view(np.uint64)
    idx = rx.indices(0).cpu().numpy().view(np.uint32)
    assert np.array_equal(off, lay.off[idx] + np.uint64(14))
    assert wl.mixed(off)
    return ip, status, off


# ---------------------------------------------------------------- rx

class WideWires:
    """test_gpu_stack.Wires for wire batches that share the wide buffer."""

    def __init__(self, w, lay, starts):
        self.w, self.lay, self.starts, self.batches, self.where = w, lay, starts, [], {}

    def add(self, frames) -> batch.PacketBatch:
        b = len(self.batches)
        lo, hi = int(self.starts[b]), int(self.starts[b + 1])
        assert hi - lo == len(frames)
        wire = _pb(self.w, self.lay.off[lo:hi], self.lay.length[lo:hi])
        self.batches.append(wire)
        # an IPv4 packet's address names its frame; an empty frame may start where its neighbour does
        self.where.update({int(o) + native.ETH_HDR: (b, k) for k, o in enumerate(self.lay.off[lo:hi].tolist())
                           if frames[k] is not None and len(frames[k]) > native.ETH_HDR})
        return wire

    def frame_of(self, addr: int) -> tuple:
        return self.where[addr - self.w.base]


@pytest.mark.parametrize("variant", wl.variants(RX_SLOTS))
def test_stack_rx(dev, wide, variant):
    """run_rx / check_rx of tests/test_gpu_stack.py: eth_rx, ipv4_frames_rss,
    arp_learn_records, frag_records, reassemble, spans_desc, pack() and both
    steer runs, the three wire batches in one layout."""
    from test_gpu_stack import check_rx, run_rx
    plan = stack_plan()
    batches, model_outs, tables = modelled(STACK_SEED)
    lay, _ = _laid(wide, plan, variant)
    cfg = sm.rx_cfg()
    steer = batch.Steer(cfg["ncpu"], np.array(cfg["reta"], dtype=np.uint8))
    outs, wires = run_rx(dev, steer, batches, tables, wires=WideWires(wide, lay, plan.starts))
    steer.close()
    nframes, ndgrams = check_rx(outs, wires, model_outs, cfg["ncpu"])
    assert nframes == len(plan.frames) and ndgrams > 20
    across = 0
    for b, g in enumerate(outs):
        lo = int(plan.starts[b])
        assert np.array_equal(g["ip_off"], lay.off[lo + g["idx"][0].astype(np.int64)] + np.uint64(14)), b
        for r in g["records"]:
            wires.frame_of(int(r["frame"]))               # the buffer's address + off + 14 of one of the frames
        src = g["desc"]["src"].astype(np.int64) - wide.base
        for k in range(g["totals"][0]):
            piece = src[int(g["dgram_first"][k]):int(g["dgram_first"][k + 1])]
            across += bool(piece.min() < P32 <= piece.max())
    assert across >= 8, across


@pytest.mark.parametrize("variant", wl.variants(RX_SLOTS))
def test_udp_rx(dev, wide, variant):
    """sccsum_udp_rx (the raw call and the wrapper) and udp_rx_reassembled against udp_model."""
    from test_gpu_udp import _atomic, _port_map, _ports, _reasm_outputs, check_rx, run_udp_rx
    plan, c = udp_plan(), udp_traffic.case(0)
    lay, _ = _laid(wide, plan, variant)
    ip, status, off = _ip_bucket(wide, lay, c["info"])
    ports, items = _ports(dev.index, 252), _atomic(c, 252)
    want = check_rx(run_udp_rx(dev, ip, ip.n, status, ports), items, 252, off)
    r = batch.udp_rx(ip, status, ports, HOST)
    torch.cuda.synchronize()
    got = dict(cls=r.cls.cpu().numpy(), first=r.first.cpu().numpy().view(np.uint32),
               order=r.order.cpu().numpy().view(np.uint32), pay_off=r.pay_off.cpu().numpy().view(np.uint64),
               pay_len=r.pay_len.cpu().numpy().view(np.uint32), src=r.src_all.cpu().numpy().view(np.uint32),
               sport=r.sport_all.cpu().numpy().view(np.uint16))
    check_rx(got, items, 252, off)
    assert int((got["pay_off"] >= P32).sum()) > 100
    for k in (0, 1, 7):                                      # a channel's slices are a spans batch as they stand
        sums = batch.spans(r.channel(k))
        torch.cuda.synchronize()
        mine = [j for j in want["pos"] if items[j]["cls"] == k]
        assert batch.as_u16(sums).view(np.uint8).reshape(-1, 2).tolist() == \
            [list(sm.csum(items[j]["payload"]).to_bytes(2, "big")) for j in mine]
    # the fragments: reassembled, packed, demultiplexed
    recs = batch.frag_records(ip, status, host_address=HOST, tag=0)
    rr = batch.reassemble(recs)
    desc, first, d_off, length, seeds, max_len = rr.lists()
    packed = rr.pack()
    torch.cuda.synchronize()
    d = rr.totals()[0]
    assert d == len(c["delivered"]) >= 40
    data, p_off, p_len = packed.data.cpu().numpy(), d_off.cpu().numpy(), length.cpu().numpy()
    dh, fh = desc.cpu().numpy().view(batch.DESC_DTYPE), first.cpu().numpy().view(np.uint32)
    across = 0
    for k, m in enumerate(c["delivered"]):
        assert data[int(p_off[k]):int(p_off[k]) + int(p_len[k])].tobytes() == m["data"], k
        across += _sides((dh["src"][int(fh[k]):int(fh[k + 1])].astype(np.int64) - wide.base).tolist(), lay.lines)
    assert across >= 8, across
    for nch in (252, 3):
        pm = _port_map(nch)
        items_r = [udp_model.reassembled(m, pm) for m in c["delivered"]]
        rr_u = batch.udp_rx_reassembled(rr, recs, _ports(dev.index, nch), HOST)
        torch.cuda.synchronize()
        want_r = check_rx(_reasm_outputs(rr_u), items_r, nch)
        for j, n in zip(want_r["pos"], want_r["pay_len"].tolist()):
            if items_r[j]["cls"] < nch:
                a = int(p_off[j]) + 8
                assert data[a:a + n].tobytes() == items_r[j]["payload"], j


@pytest.mark.parametrize("variant", wl.variants(RX_SLOTS))
def test_tcp_rx(dev, wide, variant):
    """sccsum_tcp_rx against tcp_model: classes, segment records (pay_off as u64), runs, reset records."""
    from test_gpu_tcp import _conns, _items, check_rx, run_tcp_rx
    plan, c = tcp_plan(), tcp_traffic.case(0)
    lay, _ = _laid(wide, plan, variant)
    ip, status, off = _ip_bucket(wide, lay, c["info"])
    for nconns, offload in ((254, False), (65533, True)):
        got = run_tcp_rx(dev, ip, ip.n, status, _conns(dev.index, nconns),
                         flags=native.TCP_CSUM_OFFLOAD if offload else 0)
        want = check_rx(got, _items(0, nconns), off, offload=offload)
        assert int(want["total"][1]) > 100 and int((want["seg"]["pay_off"] >= P32).sum()) > 100


@pytest.mark.parametrize("variant", wl.variants(RX_SLOTS))
def test_tcp_rx_data_from_frames(dev, wide, variant):
    """frames -> eth_rx -> ipv4_frames -> tcp_rx -> tcp_rx_data -> pack(): every
    descriptor's src is the buffer's address + pay_off, every connection's
    packed stream the model's bytes."""
    from test_gpu_tcp_data import NCONNS
    plan = tcp_data_plan()
    lay, _ = _laid(wide, plan, variant)
    read = Reader(lay, plan.frames)
    wire = _pb(wide, lay.off, lay.length)
    ip = batch.eth_rx(wire, (sm.IPV4, sm.ARP)).bucket(0)
    status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(ip, status=status)
    conns = batch.TcpConns(tcp_traffic.conn_array(NCONNS), tcp_traffic.LISTEN, device=dev.index)
    rx = batch.tcp_rx(ip, status, conns, HOST)
    rcv = np.zeros(NCONNS, dtype=batch.TCP_RCV_DTYPE)
    for cc, t in enumerate(plan.tcbs):
        for name, v in t.rcv_record().items():
            rcv[cc][name] = v
    d = batch.tcp_rx_data(rx, torch.from_numpy(rcv.view(np.uint8).reshape(NCONNS, 32)).to(dev))
    packed = d.pack()
    torch.cuda.synchronize()
    assert np.array_equal(ip.off.cpu().numpy().view(np.uint64), lay.off + np.uint64(14))
    run_conn = rx.runs()[0].cpu().numpy().view(np.uint32)
    assert run_conn.tolist() == list(range(NCONNS)) and rx.bounds()[1] == len(plan.frames)
    out, runs = packed.cpu().numpy(), d.runs_host()
    descs = d.descs.cpu().numpy().reshape(-1).view(batch.DESC_DTYPE)
    at, cnt, above = 0, 0, 0
    for k, cc in enumerate(run_conn.tolist()):
        segs = rx.segs(k).cpu().numpy().reshape(-1).view(batch.TCP_SEG_DTYPE)
        want = dm.walk(copy.deepcopy(plan.tcbs[cc]), [{n: int(s[n]) for n in segs.dtype.names} for s in segs])
        got = runs[k]
        assert (got["taken"], got["bytes"], got["next"], got["window"], got["room"], got["flags"], got["stop"]) == \
            (want.taken, want.bytes, want.next, want.window, want.room, want.flags, want.stop), (k, got, want)
        assert (got["desc_first"], got["dst_off"]) == (cnt, at)
        mine = descs[cnt:cnt + want.taken]
        assert mine["src"].tolist() == [wide.base + o for o, _ in want.data], k
        assert mine["len"].tolist() == [n for _, n in want.data], k
        above += sum(o >= P32 for o, _ in want.data)
        text = b"".join(read(o, n) for o, n in want.data)
        assert len(text) == want.bytes and out[at:at + want.bytes].tobytes() == text, k
        at += want.bytes
        cnt += want.taken
    assert d.totals() == (cnt, at, at) and descs.size == cnt and above >= 20
    conns.close()


def _wide_pay_offs(n: int) -> list:
    """k, 2^31 + k, 2^32 - 1, 2^32, 2^32 + k, 2^33 + k, turn by turn: six kinds in every wave."""
    return [(37 * k, P31 + 37 * k, P32 - 1, P32, P32 + 37 * k, (1 << 33) + 37 * k)[k % 6] for k in range(n)]


@pytest.mark.parametrize("n", [65, dtr.TILE + 1])
def test_tcp_rx_data_fabricated(dev, n):
    """sccsum_tcp_rx_data reads no frame byte: segment records whose pay_off has
    a high half, against BASE, the descriptors' src compared as u64."""
    from test_gpu_tcp_data import BASE, check, run_data
    cases = dtr.mixed(n % 5, n)
    a = dtr.arrays(cases)
    offs = _wide_pay_offs(a["n0"])
    p = 0
    for _, segs in cases:
        for s in segs:
            s["pay_off"] = offs[p]
            a["seg"][p]["pay_off"] = offs[p]
            p += 1
    want = dtr.expect(cases, base=BASE)
    assert p == n and int((want["desc"]["src"] >= BASE + P32).sum()) >= n // 8
    assert len({int(x - BASE) >> 31 for x in want["desc"]["src"][:64]}) >= 4
    check(run_data(dev, a), want)


# ---------------------------------------------------------------- tx: headers into the headroom

def _raw_plan(payloads):
    p = _plan(payloads, [np.arange(len(payloads))])
    p.kinds = [0] * len(payloads)
    p.prefer = [f is not None and len(f) >= 16 for f in payloads]
    return p


def _payloads(seed: int, lens) -> list:
    """Random payloads of the given lengths; two entries lie past the buffer (None)."""
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    out[50] = out[200] = None
    return out


@functools.lru_cache(maxsize=None)
def udp_send_plan():
    """Every length 0-64 four times over (all 16 alignments of each zone), the limits of one frame and of UDP."""
    return _raw_plan(_payloads(0x0D9, list(range(65)) * 4 + [1472, 1473, 300, 65507, 65508, 301]))


@functools.lru_cache(maxsize=None)
def tcp_send_plan():
    p = _raw_plan(_payloads(0x7C9, list(range(65)) * 4 + [1459, 1460, 1461, 300, 65515 - 24, 65515 - 24 + 1, 301]))
    n = len(p.frames)
    rng = np.random.default_rng(0x7CA)
    p.hdrs = [20 + 4 * (k % 11) for k in range(n)]
    p.hdrs[n - 3] = p.hdrs[n - 2] = 24
    out = np.zeros(n, dtype=batch.TCP_OUT_DTYPE)
    lens = [0 if f is None else len(f) for f in p.frames]
    out["dst"] = [(sm.ON_LINK + sm.OFF_LINK)[k % 8] for k in range(n)]
    out["seq"], out["ack"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n)
    out["sport"], out["dport"], out["window"] = (rng.integers(0, 65536, n) for _ in range(3))
    out["flags"], out["hdr_len"] = np.arange(n) * 5 % 256, p.hdrs
    out["mss"] = [(max(ln - 1, 1), max(ln, 1), ln + 1, 1460)[k % 4] for k, ln in enumerate(lens)]
    p.out = out
    return p


def _img_read(imgs, o: int, n: int) -> bytes:
    for a, img in imgs:
        if a <= o and o + n <= a + img.size:
            return img[o - a:o - a + n].tobytes()
    raise AssertionError((o, n))


def _img_write(imgs, o: int, data: bytes) -> None:
    for a, img in imgs:
        if a <= o and o + len(data) <= a + img.size:
            img[o - a:o - a + len(data)] = np.frombuffer(data, np.uint8)
            return
    raise AssertionError((o, len(data)))


class Aliases:
    """The header bytes' low aliases, (off - hdr) mod 2^32, where they lie in no
    cluster: gathered before the run, compared after it.  (Inside a cluster
    the comparison of the cluster's bytes covers them.)"""

    def __init__(self, w, lay, hdrs):
        at = []
        for i in lay.real.tolist():
            o = int(lay.off[i]) - hdrs[i]
            if o >= P32 and not any(a < o - P32 + hdrs[i] and o - P32 < b for a, b in lay.clusters):
                at.append(np.arange(o - P32, o - P32 + hdrs[i]))
        assert len(at) >= 16
        self.w, self.idx = w, torch.from_numpy(np.concatenate(at)).to(w.dev)
        self.before = w.data[self.idx].clone()

    def untouched(self) -> None:
        assert torch.equal(self.w.data[self.idx], self.before), "bytes at (off - hdr) mod 2^32 changed"


def _assert_clusters(w, imgs, what) -> None:
    """Every cluster byte for byte (its margins of 64 bytes and more included):
    the headers where the model puts them, everything else as it was written."""
    for a, img in imgs:
        got = w.data[a:a + img.size].cpu().numpy()
        bad = np.flatnonzero(got != img)
        assert bad.size == 0, f"{what}: cluster at {a}: {bad.size} bytes differ, first at {a + int(bad[0])}"


def _chain(w, u, dst, ids, mtu, flags=native.SEND_L4):
    """spans(seeds) -> ipv4_send(SEND_L4) -> ipv4_fill_desc(FILL_IP) -> eth_send -> pack(), every peer resolved."""
    d_dst = _t32(w.dev, dst)
    ids16 = _t16(w.dev, ids)
    l4sum = batch.spans(u.sum_batch, seeds=u.seeds)
    r = batch.ipv4_send(u.l4, d_dst, u.proto, mtu, HOST, ids=ids16, l4sum=l4sum, flags=flags)
    desc, first, off, length, max_len = r.lists()
    batch.ipv4_fill_desc(desc, first, off, length, max_len, mode=native.FILL_IP)
    arp = {d: sm.peer_mac(d) for d in sm.ON_LINK}
    arp[sm.GW] = sm.GW_MAC
    table = batch.ArpTable(arp)
    wire = batch.eth_send(r, d_dst, table, sm.HW, HOST, sm.NETMASK, sm.GW).pack()
    torch.cuda.synchronize()
    table.close()
    return r, wire, arp


def _assert_wire(w, r, wire, frames, owner, l4_off) -> None:
    """The packed frames byte for byte, and ipv4_send's payload descriptors:
    src = address + l4.off + the piece's offset."""
    data, w_off, w_len = wire.data.cpu().numpy(), wire.off.cpu().numpy(), wire.length.cpu().numpy()
    assert wire.n == len(frames) == r.frames_emitted()
    at, src = {}, []
    for k, want_f in enumerate(frames):
        assert data[int(w_off[k]):int(w_off[k]) + int(w_len[k])].tobytes() == want_f, ("wire frame", k, owner[k])
        src.append(w.base + l4_off[owner[k]] + at.get(owner[k], 0))
        at[owner[k]] = at.get(owner[k], 0) + len(want_f) - 34
    d = r.desc[: 32 * len(frames)].cpu().numpy().view(batch.DESC_DTYPE)
    assert d["src"][1::2].tolist() == src
    assert len({o for o, a in zip(owner, src) if a >= w.base + P32}) >= 30


ALL_UDP = native.UDP_CSUM_OFFLOAD | native.UDP_UFO
ALL_TCP = native.TCP_CSUM_OFFLOAD | native.TCP_TSO


@pytest.mark.parametrize("flags", [0, ALL_UDP], ids=["plain", "offload_ufo"])
@pytest.mark.parametrize("variant", wl.variants(UDP_TX_SLOTS))
def test_udp_send(dev, wide, variant, flags):
    """udp_send's headers at off - 8 and nothing else, then the tx recipe at MTU 68 and 1500 against stack_model.tx."""
    plan = udp_send_plan()
    n = len(plan.frames)
    offload, ufo = bool(flags & native.UDP_CSUM_OFFLOAD), bool(flags & native.UDP_UFO)
    rng = np.random.default_rng(500 + variant)
    dst = [(sm.ON_LINK + sm.OFF_LINK)[k % 8] for k in range(n)]
    dport, sport = rng.integers(0, 65536, n).tolist(), rng.integers(0, 65536, n).tolist()
    ids = [(17 * k + variant) & 0xFFFF for k in range(n)]
    for mtu in (68, 1500):
        lay, imgs = _laid(wide, plan, variant, UDP_TX_SLOTS, strip=42, head=8)
        off, lens = [int(x) for x in lay.off], [int(x) for x in lay.length]
        alias = Aliases(wide, lay, [8] * n)
        pay = _pb(wide, lay.off, lay.length)
        u = batch.udp_send(pay, _t32(dev, dst), _t16(dev, dport), _t16(dev, sport),
                           HOST, mtu, flags)
        torch.cuda.synchronize()
        status = [native.ST_RANGE if f is None else native.ST_MALFORMED if len(f) > 65507 else native.ST_OK
                  for f in plan.frames]
        assert status.count(native.ST_OK) == n - 3 and u.status.cpu().numpy().tolist() == status
        model = [udp_model.send(f, sp, dp, HOST, d, mtu, offload, ufo) if s == native.ST_OK else None
                 for f, sp, dp, d, s in zip(plan.frames, sport, dport, dst, status)]
        for o, m in zip(off, model):
            if m is not None:
                _img_write(imgs, o - 8, m["zero"][:8])
        _assert_clusters(wide, imgs, "after udp_send")
        alias.untouched()
        ok = [m is not None for m in model]
        assert u.l4.off.cpu().numpy().view(np.uint64).tolist() == [o - 8 if k else (1 << 64) - 1
                                                                   for o, k in zip(off, ok)]
        assert u.l4.length.cpu().numpy().tolist() == [ln + 8 if k else 0 for ln, k in zip(lens, ok)]
        needs = [bool(m and m["needs_csum"]) for m in model]
        assert u.needs_csum.cpu().numpy().astype(bool).tolist() == needs
        seeds = [0 if not k else (0xFFFF ^ udp_model.pseudo_sum(HOST, d, ln + 8)) if nc
                 else udp_model.pseudo_sum(HOST, d, ln + 8) for ln, d, k, nc in zip(lens, dst, ok, needs)]
        assert u.seeds.cpu().numpy().view(np.uint32).tolist() == seeds
        r, wire, arp = _chain(wide, u, dst, ids, mtu, native.SEND_L4 | (native.SEND_UFO if ufo else 0))
        assert r.status.cpu().numpy().tolist() == [native.ST_OK if k else native.ST_RANGE for k in ok]
        for o, m in zip(off, model):
            if m is not None:
                _img_write(imgs, o - 8, m["l4"][:8])
        _assert_clusters(wide, imgs, "the datagrams as sent")
        alias.untouched()
        cfg = dict(host=HOST, netmask=sm.NETMASK, gw=sm.GW, hw=sm.HW, mtu=65535 if ufo else mtu, arp=arp)
        t = sm.tx([(m["zero"] if m else None, sm.UDP, d, i) for m, d, i in zip(model, dst, ids)], cfg)
        frames = list(t["frames"])
        for k, owner in enumerate(t["owner"]):
            if needs[owner]:                                   # never cut: the one frame carries the bare pseudo sum
                f = frames[k]
                frames[k] = f[:14 + 20 + 6] + model[owner]["l4"][6:8] + f[14 + 20 + 8:]
        _assert_wire(wide, r, wire, frames, t["owner"], [o - 8 for o in off])


@pytest.mark.parametrize("flags", [0, ALL_TCP], ids=["plain", "offload_tso"])
@pytest.mark.parametrize("variant", wl.variants(TCP_TX_SLOTS))
def test_tcp_send(dev, wide, variant, flags):
    """tcp_send's 20 header bytes at off - hdr_len (the options behind them stay), then the tx recipe."""
    plan = tcp_send_plan()
    n, out, hl = len(plan.frames), plan.out, plan.hdrs
    offload, tso = bool(flags & native.TCP_CSUM_OFFLOAD), bool(flags & native.TCP_TSO)
    ids = [(17 * k + variant) & 0xFFFF for k in range(n)]
    d_out = torch.from_numpy(out.view(np.uint8).reshape(n, 24).copy()).to(dev)
    for mtu in (68, 1500):
        lay, imgs = _laid(wide, plan, variant, TCP_TX_SLOTS, strip=54, head=60)
        off, lens = [int(x) for x in lay.off], [int(x) for x in lay.length]
        alias = Aliases(wide, lay, hl)
        pay = _pb(wide, lay.off, lay.length)
        u = batch.tcp_send(pay, d_out, HOST, mtu, flags)
        torch.cuda.synchronize()
        status = [tm.send_status(o, ln, h, W, tso, int(m)) or native.ST_OK
                  for o, ln, h, m in zip(off, lens, hl, out["mss"].tolist())]
        assert status.count(native.ST_RANGE) == 2 and status.count(native.ST_MALFORMED) == 1
        assert u.status.cpu().numpy().tolist() == status
        model = []
        for k, (o, f, s) in enumerate(zip(off, plan.frames, status)):
            rec = {x: int(out[x][k]) for x in ("dst", "seq", "ack", "sport", "dport", "window", "flags", "mss")}
            model.append(tm.send(f, rec, HOST, _img_read(imgs, o - hl[k] + 20, hl[k] - 20), offload, tso)
                         if s == native.ST_OK else None)
        for k, (o, m) in enumerate(zip(off, model)):
            if m is not None:
                _img_write(imgs, o - hl[k], m["zero"][:20])
        _assert_clusters(wide, imgs, "after tcp_send")
        alias.untouched()
        ok = [m is not None for m in model]
        assert u.l4.off.cpu().numpy().view(np.uint64).tolist() == [o - h if k else (1 << 64) - 1
                                                                   for o, h, k in zip(off, hl, ok)]
        assert u.l4.length.cpu().numpy().tolist() == [ln + h if k else 0 for ln, h, k in zip(lens, hl, ok)]
        assert u.needs_csum.cpu().numpy().astype(bool).tolist() == [k and offload for k in ok]
        big = [bool(k) and offload and tso and ln > int(m) for ln, m, k in zip(lens, out["mss"].tolist(), ok)]
        assert u.tso_seg.cpu().numpy().view(np.uint16).tolist() == [int(m) & 0xFFFF if g else 0
                                                                    for m, g in zip(out["mss"].tolist(), big)]
        pseudo = [tm.pseudo_sum(HOST, int(d), 0 if g else ln + h)
                  for d, ln, h, g in zip(out["dst"].tolist(), lens, hl, big)]
        assert u.seeds.cpu().numpy().view(np.uint32).tolist() == [0 if not k else (0xFFFF ^ p) if offload else p
                                                                  for p, k in zip(pseudo, ok)]
        r, wire, arp = _chain(wide, u, out["dst"].tolist(), ids, mtu)
        assert r.status.cpu().numpy().tolist() == [native.ST_OK if k else native.ST_RANGE for k in ok]
        for k, (o, m) in enumerate(zip(off, model)):
            if m is not None:
                _img_write(imgs, o - hl[k], m["l4"][:20])
        _assert_clusters(wide, imgs, "the segments as sent")
        alias.untouched()
        cfg = dict(host=HOST, netmask=sm.NETMASK, gw=sm.GW, hw=sm.HW, mtu=mtu, arp=arp)
        t = sm.tx([(m["zero"] if m else None, sm.TCP, int(d), i)
                   for m, d, i in zip(model, out["dst"].tolist(), ids)], cfg)
        frames, seen = list(t["frames"]), set()
        for k, owner in enumerate(t["owner"]):
            if offload and owner not in seen:                  # the first piece carries the bare pseudo sum
                f = frames[k]
                frames[k] = f[:14 + 20 + 16] + model[owner]["l4"][16:18] + f[14 + 20 + 18:]
            seen.add(owner)
        _assert_wire(wide, r, wire, frames, t["owner"], [o - h for o, h in zip(off, hl)])


# ---------------------------------------------------------------- tcp_tx_data

@functools.lru_cache(maxsize=None)
def tx_data_plan():
    """The unsent buffers of 120 mixed connections, each a 'frame' of its own."""
    cases = ttr.mixed(0x7D, 120)
    a = ttr.arrays(cases)
    p = _raw_plan([bytes(b) for t in cases for b in t.unsent])
    p.prefer = [len(f) >= 600 for f in p.frames]            # longer than an MSS of 536: a cut inside it
    p.cases, p.a = cases, a
    return p


@pytest.mark.parametrize("headroom,variant", [(20, 0), (24, 1), (64, 2), (20, 3)])
def test_tcp_tx_data_gathers_across_the_lines(dev, wide, headroom, variant):
    """pack() through the wrapper, the buffers where the layout puts them:
    every segment's staged bytes are its stream's."""
    from test_gpu_tcp_tx_data import _payloads_through_the_wrapper
    plan = tx_data_plan()
    lay, _ = _laid(wide, plan, variant, BUF_SLOTS, strip=54)
    a = dict(plan.a, blob_off=lay.off.copy())
    for X in lay.lines:
        assert any(0 < p < L for p, L in wl.line_byte(lay, X)) or lay.special[X][0] == "edge"
    _payloads_through_the_wrapper(dev, plan.cases, a, wide.data, headroom)


@pytest.mark.parametrize("n", [65, ttr.TILE + 1])
def test_tcp_tx_data_fabricated_carry(dev, n):
    """No gather, fake addresses: every third buffer starts within its own
    length below a multiple of 2^32, so src + consumed carries into the high
    word, in buffers a segment boundary cuts too."""
    from test_gpu_tcp_tx_data import FAKE, check, run_tx
    cases = ttr.mixed(n, n)
    a = ttr.arrays(cases)
    rng = np.random.default_rng(n)
    src = a["blob_off"].astype(np.uint64) + np.uint64(FAKE)
    for j, ln in enumerate(a["buf_len"].tolist()):
        if j % 3 == 0 and ln >= 2:
            src[j] = ((j % 7 + 0x7001) << 32) - int(rng.integers(1, ln))
    a = dict(a, blob_off=src - np.uint64(FAKE))
    hw, headroom = Hw(576), 24
    want = fast.expect(a["snd"], a["buf_len"], a["buf_first"], hw.mtu, headroom, hw.tx_tso, hw.max_packet_len)
    lo = (src[want["desc_buf"]] & np.uint64(M32)).astype(np.int64)
    inner = want["desc_inner"].astype(np.int64)
    carried = (inner > 0) & (lo + inner >= P32)                      # a piece behind a cut, past the carry
    straddle = (lo < P32) & (lo + inner + want["desc_len"].astype(np.int64) > P32) & (lo + inner < P32)
    assert int(carried.sum()) >= n // 16 and int(straddle.sum()) >= n // 16
    got = run_tx(dev, a, hw, headroom)
    assert np.array_equal(got["src"], src)
    check(got, want, n)


# ---------------------------------------------------------------- layouts whose totals pass 2^32: lists only
#
# The calls below read no frame byte, so their inputs are lengths alone and
# nothing is packed.  Under the default max_out_bytes (2^32 - 1) the layout of
# the whole batch would pass 2^32: the prefix rule cuts it, the running sum
# goes on past 2^32 without wrapping (a wrapped sum would find room again for
# the datagrams behind the cut), and the 64-bit offsets below the cut are
# exact.  sccsum_tcp_rx_data and sccsum_tcp_tx_data have this already:
# test_gpu_tcp_data.py::test_sums_past_32_bits_do_not_wrap and
# test_gpu_tcp_tx_data.py::test_sums_past_32_bits.

DGRAMS = 65600                       # x 65 528 .. 65 549 bytes: more than 2^32 in all


def test_reassemble_total_past_2_32(dev):
    """65 600 datagrams of 65 528 bytes in two records each; no key, so no frame byte is read."""
    from test_gpu_reasm import PENDING, Raw, _check, _expect
    recs = np.zeros(2 * DGRAMS, batch.REC_DTYPE)
    k = np.arange(DGRAMS)
    for j, (o, ln, mf) in enumerate(((0, 32768, 1), (32768, 32760, 0))):
        recs["src"][j::2], recs["dst"][j::2], recs["id"][j::2] = 0x0A010000 + k, HOST, k & 0xFFFF
        recs["proto"][j::2] = 17
        recs["offset"][j::2], recs["len"][j::2], recs["mf"][j::2], recs["hdr_len"][j::2] = o, ln, mf, 20
        recs["frame"][j::2] = 0x7000_0000_1000 + k * (1 << 17) + j * 40000       # addresses, never read
    st, emitted = _expect(recs, collisions=True)
    total = sum(d.length for d in emitted)
    assert total <= M32 < total + 65528 and DGRAMS * 65528 > P32
    assert 100 <= int((st == PENDING).sum()) and len(emitted) > 65500
    h = Raw(dev, recs.size).run(torch.from_numpy(recs.view(np.uint8).copy()).to(dev), key=None)
    _check(h, recs, st, emitted, key=None)
    assert int(h["dgram_off"][: 8 * len(emitted)].view(np.uint64)[-1]) == total - 65528 > P32 - (1 << 17)


@pytest.fixture(scope="module")
def sent_past(dev):
    """ipv4_send on 65 600 UDP datagrams of 65 515 bytes under SEND_UFO: one
    frame of 65 535 bytes each, all of them the same 65 536 bytes of a small buffer."""
    data = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    n = DGRAMS
    l4 = batch.PacketBatch(data=data, off=_t64(dev, np.zeros(n, np.uint64)),
                           length=_t32(dev, np.full(n, sm.L4_MAX, np.uint32)), bytes_len=1 << 16, max_len=sm.L4_MAX)
    dst = _t32(dev, np.full(n, sm.ON_LINK[0], np.uint32))
    proto = torch.full((n,), 17, dtype=torch.uint8, device=dev)
    r = batch.ipv4_send(l4, dst, proto, 1500, HOST, ids=_t16(dev, np.arange(n) & 0xFFFF), flags=native.SEND_UFO,
                        max_frames=n, max_out_bytes=M32)
    torch.cuda.synchronize()
    return r, dst, l4


def test_ipv4_send_total_past_2_32(dev, sent_past):
    r, _, l4 = sent_past
    n, frame = DGRAMS, 65535
    prefix = M32 // frame
    assert prefix * frame == M32 and n * frame > P32           # the last datagram that fits ends exactly on the cap
    assert r.totals() == (n, n * frame, prefix) and r.frames_emitted() == prefix
    assert r.status.cpu().numpy().tolist() == [native.ST_OK] * prefix + [0] * (n - prefix)
    f = np.arange(prefix, dtype=np.uint64)
    assert np.array_equal(r.out_off[:prefix].cpu().numpy().view(np.uint64), f * np.uint64(frame))
    assert np.all(r.out_len[:prefix].cpu().numpy() == frame)
    assert np.array_equal(r.dgram_first.cpu().numpy().view(np.uint32), np.minimum(np.arange(n + 1), prefix))
    d = r.desc[: 32 * prefix].cpu().numpy().view(batch.DESC_DTYPE)
    assert np.array_equal(d["dst_off"][0::2], (f * np.uint64(frame)).astype(np.uint32))
    assert np.array_equal(d["dst_off"][1::2], (f * np.uint64(frame) + np.uint64(20)).astype(np.uint32))
    assert np.all(d["src"][1::2] == l4.data.data_ptr()) and np.all(d["len"][1::2] == frame - 20)
    assert int(d["dst_off"][-1]) == M32 - frame + 20


def test_eth_send_total_past_2_32(dev, sent_past):
    """The 65 537 frames ipv4_send emitted, 14 bytes longer each: past 2^32 again."""
    r, dst, _ = sent_past
    frames, frame = M32 // 65535, 65535 + 14
    table = batch.ArpTable({sm.ON_LINK[0]: sm.peer_mac(sm.ON_LINK[0])})
    e = batch.eth_send(r, dst, table, sm.HW, HOST, sm.NETMASK, sm.GW)
    torch.cuda.synchronize()
    prefix = M32 // frame
    assert frames * frame > P32 and prefix < frames
    need_f, need_b, taken, unresolved = e.totals()
    assert (need_f, need_b, unresolved) == (frames, frames * frame, 0)
    assert e.emitted() == (prefix, 3 * prefix)
    st = e.status.cpu().numpy()
    assert st[:prefix].tolist() == [native.ST_OK] * prefix and not st[prefix:].any() and taken == prefix
    f = np.arange(prefix, dtype=np.uint64)
    assert np.array_equal(e.out_off[:prefix].cpu().numpy().view(np.uint64), f * np.uint64(frame))
    assert np.all(e.out_len[:prefix].cpu().numpy() == frame)
    assert np.array_equal(e.frame_src[:prefix].cpu().numpy(), np.arange(prefix))
    assert int(e.out_off[prefix - 1].item()) == (prefix - 1) * frame > P32 - (1 << 17)
    table.close()
