"""The rx and tx recipes of INTEGRATION.md ("Link layer", "Fragments",
"Steering", "Send") run end to end through the batch.py wrappers, every output
compared with tests/stack_model.py: one per-packet restatement of the reference
stack from NIC to shard, which shares no convention with the per-call models.
The rx wire batches are the MODEL's tx frames (several peers, MTU 68 / 576 /
1500), so the rx side does not lean on the device's tx side; tests/
test_stack_model.py asserts what every seed's traffic holds.  All comparisons
are exact."""
import numpy as np
import pytest
import torch

import stack_model as sm
from seastar_amd import batch, native
from test_stack_model import laid_out, modelled

pytestmark = pytest.mark.gpu

HOST, MASK, GW, HW = sm.HOST, sm.NETMASK, sm.GW, sm.HW
NEED, REJECT = native.ST_OK, native.ST_MALFORMED | native.ST_RANGE


def _i32(dev, a) -> torch.Tensor:
    return torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def _swap(v: int) -> int:
    """A checksum as the device returns it (the field's two wire bytes read little-endian) as a number."""
    return ((v & 0xFF) << 8) | (v >> 8)


@pytest.fixture(scope="module")
def steer(dev):
    cfg = sm.rx_cfg()
    st = batch.Steer(cfg["ncpu"], np.array(cfg["reta"], dtype=np.uint8))
    yield st
    st.close()


# ---------------------------------------------------------------- rx

class Wires:
    """The wire batches of a case in their device buffers, all kept alive, and
    the way back from an address inside one of them to (batch, frame)."""

    def __init__(self, dev):
        self.dev, self.batches, self.where = dev, [], []

    def add(self, frames) -> batch.PacketBatch:
        buf, _, off, length = laid_out(frames)
        w = batch.PacketBatch.from_host(buf, off, length, device=self.dev)
        self.batches.append(w)
        self.where.append({int(o) + native.ETH_HDR: k for k, o in enumerate(off.tolist())})
        return w

    def frame_of(self, addr: int) -> tuple:
        for b, w in enumerate(self.batches):
            base = w.data.data_ptr()
            if base <= addr < base + w.bytes_len:
                return b, self.where[b][addr - base]
        raise AssertionError(f"address {addr:#x} lies in no wire buffer")


def run_rx(dev, steer, batches, tables, host_address=HOST, wires=None) -> tuple:
    """The rx recipe, batch after batch, exactly as INTEGRATION.md writes it.
    Returns (per batch a dict of host arrays, the Wires).  wires: a Wires whose
    add() lays the frames out elsewhere (tests/test_gpu_wide_stack.py)."""
    wires = Wires(dev) if wires is None else wires
    carry = torch.zeros(0, dtype=torch.uint8, device=dev)
    outs = []
    for b, frames in enumerate(batches):
        wire = wires.add(frames)
        table = batch.ArpTable(tables[b])
        rx = batch.eth_rx(wire, (sm.IPV4, sm.ARP))
        ip = rx.bucket(0)
        status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
        _, hashes = batch.ipv4_frames_rss(ip, sm.RSS_KEY, status=status)
        learn = batch.arp_learn_records(ip, status, rx.src_mac(0), HOST, MASK, table)
        recs = batch.frag_records(ip, status, host_address=host_address, tag=b)
        records = torch.cat([carry, recs])
        r = batch.reassemble(records, key=sm.RSS_KEY)
        desc, first, off, length, seeds, max_len = r.lists()
        l4 = batch.spans_desc(desc, first, off, length, max_len, seeds=seeds)
        cpu, order, sfirst = steer.run(r.hashes)
        cpu2, order2, sfirst2 = steer.run(hashes, status, need=NEED, reject=REJECT)
        carry = r.pending.clone()
        packed = r.pack()
        torch.cuda.synchronize()
        d, k, npend, nhost = r.totals()
        outs.append(dict(
            bounds=rx.bounds(), idx=[rx.indices(j).cpu().numpy().view(np.uint32) for j in range(3)],
            cls=rx.cls.cpu().numpy(), mac=[rx.src_mac(j).cpu().numpy().view(np.uint64) for j in range(3)],
            ip_off=ip.off.cpu().numpy().view(np.uint64),
            status=status.cpu().numpy(), hashes=_u32(hashes), learn=learn.cpu().numpy().view(batch.ARP_REC_DTYPE),
            records=records.cpu().numpy().view(batch.REC_DTYPE), totals=(d, k, npend, nhost),
            dgram_first=_u32(first), dgram_off=off.cpu().numpy().view(np.uint64), dgram_len=_u32(length),
            dgram_seed=_u32(seeds), dgram_head=_u32(r.dgram_head[:d]), dgram_last=_u32(r.dgram_last[:d]),
            dgram_hash=_u32(r.hashes), rec_state=r.rec_state.cpu().numpy(),
            desc=desc.cpu().numpy().view(batch.DESC_DTYPE), l4=l4.cpu().numpy().view(np.uint16),
            packed=packed.data.cpu().numpy()[:packed.bytes_len], pending=carry.cpu().numpy().view(batch.REC_DTYPE),
            host=r.host.cpu().numpy().view(batch.REC_DTYPE), cpu=cpu.cpu().numpy(), order=_u32(order),
            first=_u32(sfirst), cpu2=cpu2.cpu().numpy(), order2=_u32(order2), first2=_u32(sfirst2)))
        table.close()
    return outs, wires


def _rec_key(r) -> tuple:
    return int(r["src"]), int(r["dst"]), int(r["id"]), int(r["proto"])


def check_rx(outs, wires, model_outs, ncpu) -> tuple:
    """Every array of every batch against the model; returns (frames, datagrams) compared."""
    nframes = ndgrams = 0
    for b, (g, o) in enumerate(zip(outs, model_outs)):
        msg = f"batch {b}"
        # dispatch_packet
        assert g["bounds"].tolist() == np.cumsum([0] + [len(x) for x in o["buckets"]]).tolist(), (msg, "bounds")
        for j in range(3):
            assert g["idx"][j].tolist() == o["buckets"][j], (msg, "indices", j)
        assert g["cls"].tolist() == o["cls"], (msg, "cls")
        for j in range(2):
            assert g["mac"][j].tolist() == o["src_mac"][j], (msg, "src_mac", j)
        assert not g["mac"][2].any(), (msg, "src_mac of the dropped frames")
        nframes += len(o["cls"])
        # handle_received_packet: the status bytes, the dispatch hash, the learn records
        assert g["status"].tolist() == [i["status"] for i in o["ip"]], (msg, "status")
        assert g["hashes"].tolist() == [i["hash"] for i in o["ip"]], (msg, "dispatch hashes")
        idx0 = g["idx"][0]
        assert [(int(r["ip"]), int(idx0[int(r["index"])]), int(r["mac"])) for r in g["learn"]] == o["learn"], (msg, "learn records")
        # the delivered datagrams, in delivery order
        want = [d for d in o["delivered"] if d["plain"]]
        d_n, k_n, _, _ = g["totals"]
        assert d_n == len(want), (msg, "datagrams delivered")
        recs = g["records"]
        for k, d in enumerate(want):
            at, ln = int(g["dgram_off"][k]), int(g["dgram_len"][k])
            m = (msg, "datagram", k, hex(d["src"]), d["id"])
            assert ln == len(d["data"]), m
            assert g["packed"][at:at + ln].tobytes() == d["data"], m
            assert int(g["dgram_seed"][k]) == d["seed"], m
            assert _swap(int(g["l4"][k])) == d["l4"] and (int(g["l4"][k]) == 0) == d["l4_ok"], m
            assert int(g["dgram_hash"][k]) == d["hash"], m
            assert int(g["cpu"][k]) == d["shard"], m
            assert wires.frame_of(int(recs[int(g["dgram_last"][k])]["frame"])) == d["last"], (m, "completing frame")
            assert wires.frame_of(int(recs[int(g["dgram_head"][k])]["frame"])) == d["head"], (m, "kept header")
            assert _rec_key(recs[int(g["dgram_head"][k])]) == (d["src"], d["dst"], d["id"], d["proto"]), m
            assert int(g["dgram_first"][k + 1] - g["dgram_first"][k]) == d["nrecs"], m
        ndgrams += len(want)
        # what stays, and what the host takes over
        assert {_rec_key(r) for r in g["pending"]} == o["pending"], (msg, "pending keys")
        want_host = sorted((w, key, a, n, mf) for key, rs in o["host"].items() for w, a, n, mf in rs)
        got_host = [(wires.frame_of(int(r["frame"])), _rec_key(r), int(r["offset"]), int(r["len"]), int(r["mf"]))
                    for r in g["host"]]
        assert got_host == want_host, (msg, "host records")
        assert len(recs) == k_n + len(g["pending"]) + len(g["host"]), (msg, "every record in one bucket")
        # hash2cpu on the datagram hashes, then on the IPv4 bucket with the drop masks
        order, first = sm.partition([d["shard"] for d in want], ncpu + 1)
        assert g["order"].tolist() == order and g["first"].tolist() == first, (msg, "steer on the datagram hashes")
        dest = [i["shard"] if (i["status"] & NEED) == NEED and not i["status"] & REJECT else ncpu for i in o["ip"]]
        order, first = sm.partition(dest, ncpu + 1)
        assert g["cpu2"].tolist() == [native.STEER_DROPPED if x == ncpu else x for x in dest], (msg, "steer cpu")
        assert g["order2"].tolist() == order and g["first2"].tolist() == first, (msg, "steer on the IPv4 bucket")
    return nframes, ndgrams


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_rx_recipe_against_the_stack_model(dev, steer, seed):
    assert native.load().sccsum_eth_tile_packets() == sm.TILE
    batches, model_outs, tables = modelled(seed)
    outs, wires = run_rx(dev, steer, batches, tables)
    nframes, ndgrams = check_rx(outs, wires, model_outs, sm.rx_cfg()["ncpu"])
    print(f"seed {seed}: {nframes} frames, {ndgrams} reassembled datagrams compared")
    # the device's learn records, applied in order, leave the table the reference's _arp.learn calls leave
    table = dict(tables[0])
    for g in outs:
        for r in g["learn"]:
            table[int(r["ip"])] = int(r["mac"])
    want = dict(tables[-1])
    want.update({ip: mac for ip, _, mac in model_outs[-1]["learn"]})
    assert table == want


def test_rx_recipe_is_deterministic(dev, steer):
    """Twice into separately allocated wire buffers and outputs: every array is
    byte-identical once the addresses (a record's frame, a descriptor's src)
    are taken back to (batch, frame)."""
    batches, _, tables = modelled(0)
    a, wa = run_rx(dev, steer, batches, tables)
    b, wb = run_rx(dev, steer, batches, tables)
    assert all(x.data.data_ptr() != y.data.data_ptr() for x, y in zip(wa.batches, wb.batches))

    def rebased(arr, field, wires):
        out = arr.copy()
        for k in range(out.size):
            addr = int(out[field][k])
            for bi, w in enumerate(wires.batches):
                if w.data.data_ptr() <= addr < w.data.data_ptr() + w.bytes_len:
                    out[field][k] = (bi << 40) | (addr - w.data.data_ptr())
                    break
            else:
                raise AssertionError("an address outside the wire buffers")
        return out
    for ga, gb in zip(a, b):
        for name in ga:
            if name in ("records", "pending", "host"):
                assert rebased(ga[name], "frame", wa).tobytes() == rebased(gb[name], "frame", wb).tobytes(), name
            elif name == "desc":
                assert rebased(ga[name], "src", wa).tobytes() == rebased(gb[name], "src", wb).tobytes(), name
            elif name in ("idx", "mac"):
                assert all(x.tobytes() == y.tobytes() for x, y in zip(ga[name], gb[name])), name
            elif name == "totals":
                assert ga[name] == gb[name]
            else:
                assert ga[name].tobytes() == gb[name].tobytes(), name


# ---------------------------------------------------------------- tx

def l4_batch(dev, dgrams):
    """The datagrams in one device buffer with gaps between them; None: past the buffer."""
    parts, off, length, at = [], [], [], 5
    for k, (data, _, _, _) in enumerate(dgrams):
        if data is None:
            off.append(None)
            length.append(10)
            continue
        pad = k % 7
        parts.append(bytes(pad) + data)
        off.append(at + pad)
        length.append(len(data))
        at += pad + len(data)
    buf = np.frombuffer(bytes(5) + b"".join(parts), np.uint8)
    off = np.array([buf.size + 3 + k if o is None else o for k, o in enumerate(off)], np.uint64)
    return batch.PacketBatch.from_host(buf, off, np.array(length, np.uint32), device=dev)


def run_tx(dev, dgrams, mtu: int, arp: dict):
    """The tx recipe: spans(seeds) -> ipv4_send(SEND_L4) -> ipv4_fill_desc(FILL_IP) -> eth_send -> pack()."""
    l4 = l4_batch(dev, dgrams)
    lens = l4.length.cpu().numpy().view(np.uint32)
    dst = _i32(dev, [d[2] for d in dgrams])
    proto = torch.tensor([d[1] for d in dgrams], dtype=torch.uint8, device=dev)
    ids = torch.from_numpy(np.array([d[3] for d in dgrams], np.uint16).view(np.int16).copy()).to(dev)
    seeds = _i32(dev, [batch.pseudo_seed(HOST, d[2], d[1], int(n)) for d, n in zip(dgrams, lens)])
    l4sum = batch.spans(l4, seeds=seeds)
    r = batch.ipv4_send(l4, dst, proto, mtu, HOST, ids=ids, l4sum=l4sum, flags=native.SEND_L4)
    desc, first, off, length, max_len = r.lists()
    batch.ipv4_fill_desc(desc, first, off, length, max_len, mode=native.FILL_IP)
    table = batch.ArpTable(arp)
    e = batch.eth_send(r, dst, table, HW, HOST, MASK, GW)
    wire = e.pack()
    torch.cuda.synchronize()
    return l4, r, e, wire, dst, table


def wire_frames(wire) -> list:
    data, off, ln = wire.data.cpu().numpy(), wire.off.cpu().numpy(), wire.length.cpu().numpy().view(np.uint32)
    return [data[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, ln)]


def check_tx(r, e, wire, t, n):
    frames = wire_frames(wire)
    assert len(frames) == len(t["frames"])
    for k, (got, want) in enumerate(zip(frames, t["frames"])):
        assert got == want, ("wire frame", k, "of datagram", t["owner"][k])
    assert e.status.cpu().numpy().tolist() == t["status"]
    assert r.status.cpu().numpy().tolist() == t["send_status"]
    assert [(int(u["dgram"]), int(u["next_hop"])) for u in e.unresolved()] == t["unresolved"]
    nbytes = sum(len(f) for f in t["frames"])
    assert e.totals() == (len(t["frames"]), nbytes, n, len(t["unresolved"]))
    assert e.emitted() == (len(t["frames"]), 3 * len(t["frames"]))   # send's two descriptors and the Ethernet one
    return frames


@pytest.mark.parametrize("mtu", [68, 576, 1500])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_tx_recipe_against_the_stack_model(dev, seed, mtu):
    dgrams = sm.tx_traffic(seed)
    n = len(dgrams)
    cfg = sm.tx_cfg(mtu)
    if seed % 2:
        del cfg["arp"][GW]       # the gateway itself is unknown: everything off the link waits for it
    t = sm.tx(dgrams, cfg)
    assert {sm.ST_OK, sm.ST_NOARP, 0} == set(t["status"]) and {sm.ST_RANGE, sm.ST_MALFORMED} < set(t["send_status"])
    hops = {hop for _, hop in t["unresolved"]}
    assert (GW in hops) == bool(seed % 2) and hops - {GW}    # unknown on the link, and behind an unknown gateway
    l4, r, e, wire, dst, table = run_tx(dev, dgrams, mtu, cfg["arp"])
    frames = check_tx(r, e, wire, t, n)
    # the datagrams as sent: the only write into the L4 buffer is the checksum field
    data, off = l4.data.cpu().numpy(), l4.off.cpu().numpy()
    for i, want in enumerate(t["l4"]):
        if want is not None and len(want) <= sm.L4_MAX:
            assert data[int(off[i]):int(off[i]) + len(want)].tobytes() == want, ("L4 datagram", i)
    # resubmit with a table that has learnt the unresolved hops: both calls together are the full table's frames
    learnt = dict(cfg["arp"])
    learnt.update({hop: sm.peer_mac(hop) for _, hop in t["unresolved"]})
    full = sm.tx(dgrams, dict(cfg, arp=learnt))
    assert not full["unresolved"] and len(full["frames"]) > len(t["frames"])
    table2 = batch.ArpTable(learnt)
    e2 = batch.eth_send(r, dst, table2, HW, HOST, MASK, GW)
    frames2 = check_tx(r, e2, e2.pack(), full, n)
    late = {i for i, _ in t["unresolved"]}
    union = sorted([(o, k, f) for k, (o, f) in enumerate(zip(t["owner"], frames))]
                   + [(o, k, f) for k, (o, f) in enumerate(zip(full["owner"], frames2)) if o in late])
    assert [f for _, _, f in union] == full["frames"]
    print(f"seed {seed} mtu {mtu}: {len(frames) + len(frames2)} wire frames of {n} datagrams compared")
    table.close()
    table2.close()


# ---------------------------------------------------------------- loopback

def test_loopback_device_tx_into_device_rx(dev, steer):
    """The device's packed wire frames at MTU 68 into the device's rx chain:
    every L4 datagram's bytes come back, the cut ones through reassembly."""
    dgrams = [d for d in sm.tx_traffic(7, n=150) if d[0] is not None and len(d[0]) <= sm.L4_MAX]
    arp = {d[2]: sm.peer_mac(d[2]) for d in dgrams}
    arp[GW] = sm.GW_MAC
    l4, r, e, wire, dst, table = run_tx(dev, dgrams, 68, arp)
    assert e.unresolved().size == 0 and e.emitted()[0] == r.frames_emitted() > 5000
    sent = l4.data.cpu().numpy()
    l4_off = l4.off.cpu().numpy()
    want = {}
    for i, (data, proto, to, ident) in enumerate(dgrams):
        want[(HOST, to, ident, proto)] = sent[int(l4_off[i]):int(l4_off[i]) + len(data)].tobytes()
    assert len(want) == len(dgrams)
    rx = batch.eth_rx(wire, (sm.IPV4, sm.ARP))
    assert rx.bounds().tolist() == [0, wire.n, wire.n, wire.n]
    ip = rx.bucket(0)
    status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
    _, hashes = batch.ipv4_frames_rss(ip, sm.RSS_KEY, status=status)
    recs = batch.frag_records(ip, status, host_address=0, tag=1)
    rr = batch.reassemble(recs, key=sm.RSS_KEY)
    desc, first, off, length, seeds, max_len = rr.lists()
    l4v = batch.spans_desc(desc, first, off, length, max_len, seeds=seeds)
    packed = rr.pack()
    torch.cuda.synchronize()
    assert np.all(rx.src_mac(0).cpu().numpy().view(np.uint64) == HW)
    st = status.cpu().numpy()
    assert np.all((st & NEED) == NEED) and not np.any(st & REJECT)
    got = {}
    w_data, i_off, i_len = wire.data.cpu().numpy(), ip.off.cpu().numpy(), ip.length.cpu().numpy()
    for k in np.flatnonzero((st & native.ST_IPFRAG) == 0).tolist():     # the uncut frames
        f = w_data[int(i_off[k]):int(i_off[k]) + int(i_len[k])].tobytes()
        key = (sm.be32(f, 12), sm.be32(f, 16), sm.be16(f, 4), f[9])
        got[key] = f[20:]
        if sm.l4_field(f[9], len(f) - 20) is not None:
            assert st[k] & native.ST_L4_OK, key
    d, _, npend, nhost = rr.totals()
    assert npend == 0 and nhost == 0
    rec = recs.cpu().numpy().view(batch.REC_DTYPE)
    p_data, p_off, p_len = packed.data.cpu().numpy(), off.cpu().numpy(), length.cpu().numpy()
    head, l4v = rr.dgram_head[:d].cpu().numpy(), l4v.cpu().numpy()
    for k in range(d):
        key = _rec_key(rec[int(head[k])])
        assert key not in got
        got[key] = p_data[int(p_off[k]):int(p_off[k]) + int(p_len[k])].tobytes()
        if sm.l4_field(key[3], int(p_len[k])) is not None:
            assert int(l4v[k]) == 0, key
    assert d > 50 and got == want
    table.close()
