"""Pins tests/stack_model.py without a device: frames written out byte by byte,
agreement layer by layer with the per-call restatements and the oracle on the
seeded traffic, and the coverage every seed of tests/test_gpu_stack.py must
have — asserted on the model's output alone, so it holds before any GPU run."""
import functools

import numpy as np
import pytest

import oracle
import reasm_model
import stack_model as sm
from seastar_amd import batch, native
from test_eth_host import ref_eth_rx, ref_eth_send, ref_learn
from test_send_host import expected_send

HOST, PEER, PEER_MAC = sm.HOST, 0x0A000110, 0x0C001F100330

# 10.0.0.1 sends a 60-byte UDP datagram (1234 -> 5678, payload 0..51) to 10.0.1.16 at MTU 68: pieces of 48 and 12.
UDP_DATAGRAM = bytes([0x04, 0xD2, 0x16, 0x2E, 0x00, 0x3C, 0x00, 0x00]) + bytes(range(52))
UDP_FRAME_0 = bytes([
    0x0C, 0x00, 0x1F, 0x10, 0x03, 0x30,              # dst_mac: 10.0.1.16's
    0x02, 0xAB, 0x12, 0xCD, 0x34, 0xEF,              # src_mac: hw_address
    0x08, 0x00,                                      # IPv4
    0x45, 0x00, 0x00, 0x44, 0x12, 0x34, 0x20, 0x00,  # ihl 5, len 68, id 0x1234, MF, offset 0
    0x40, 0x11, 0x33, 0x65,                          # ttl 64, UDP, header checksum
    0x0A, 0x00, 0x00, 0x01, 0x0A, 0x00, 0x01, 0x10,  # 10.0.0.1 -> 10.0.1.16
    0x04, 0xD2, 0x16, 0x2E, 0x00, 0x3C, 0x42, 0xBF,  # the UDP header, its checksum over the whole datagram
]) + bytes(range(40))
UDP_FRAME_1 = bytes([
    0x0C, 0x00, 0x1F, 0x10, 0x03, 0x30, 0x02, 0xAB, 0x12, 0xCD, 0x34, 0xEF, 0x08, 0x00,
    0x45, 0x00, 0x00, 0x20, 0x12, 0x34, 0x00, 0x06,  # len 32, no MF, offset 48 / 8
    0x40, 0x11, 0x53, 0x83,
    0x0A, 0x00, 0x00, 0x01, 0x0A, 0x00, 0x01, 0x10,
]) + bytes(range(40, 52))
# a 24-byte TCP segment to 192.168.1.5, which is behind the gateway 10.0.0.254
TCP_SEGMENT = bytes([0x1F, 0x90, 0xC0, 0x01, 0x00, 0x00, 0x00, 0x01, 0x00, 0x00, 0x00, 0x02, 0x50, 0x18, 0x20, 0x00,
                     0x00, 0x00, 0x00, 0x00, 0x68, 0x69, 0x21, 0x0A])
TCP_FRAME = bytes([
    0x02, 0x00, 0x00, 0x00, 0xFF, 0xFE,              # dst_mac: the gateway's
    0x02, 0xAB, 0x12, 0xCD, 0x34, 0xEF, 0x08, 0x00,
    0x45, 0x00, 0x00, 0x2C, 0xBE, 0xEF, 0x00, 0x00,  # len 44, id 0xBEEF, not a fragment
    0x40, 0x06, 0xF0, 0x2E,
    0x0A, 0x00, 0x00, 0x01, 0xC0, 0xA8, 0x01, 0x05,
    0x1F, 0x90, 0xC0, 0x01, 0x00, 0x00, 0x00, 0x01, 0x00, 0x00, 0x00, 0x02, 0x50, 0x18, 0x20, 0x00,
    0x5B, 0x12, 0x00, 0x00, 0x68, 0x69, 0x21, 0x0A,  # checksum at TCP + 16
])
ARP_FRAME = bytes([
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x00, 0x11, 0x22, 0x33, 0x44, 0x55, 0x08, 0x06,
    0x00, 0x01, 0x08, 0x00, 0x06, 0x04, 0x00, 0x01,
    0x00, 0x11, 0x22, 0x33, 0x44, 0x55, 0x0A, 0x00, 0x00, 0x09,
    0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x0A, 0x00, 0x00, 0x01,
])
# 10.0.1.19 -> 10.0.0.1, ihl 6 (four NOP option bytes), a 12-byte UDP datagram 53 -> 32768
OPTIONS_FRAME = bytes([
    0x02, 0xAB, 0x12, 0xCD, 0x34, 0xEF, 0x0C, 0x00, 0x1F, 0x13, 0x03, 0x39, 0x08, 0x00,
    0x46, 0x00, 0x00, 0x24, 0x00, 0x42, 0x00, 0x00,  # ihl 6, len 36
    0x40, 0x11, 0x64, 0x74,                          # the checksum covers the first 20 bytes only (ip.cc:123)
    0x0A, 0x00, 0x01, 0x13, 0x0A, 0x00, 0x00, 0x01,
    0x01, 0x01, 0x01, 0x01,                          # options
    0x00, 0x35, 0x80, 0x00, 0x00, 0x0C, 0xCC, 0xEF, 0xDE, 0xAD, 0xBE, 0xEF,
])


def test_tx_frames_byte_by_byte():
    t = sm.tx([(UDP_DATAGRAM, sm.UDP, PEER, 0x1234), (TCP_SEGMENT, sm.TCP, 0xC0A80105, 0xBEEF),
               (UDP_DATAGRAM, sm.UDP, 0x0A000177, 1), (None, sm.UDP, PEER, 2), (bytes(65516), sm.ICMP, PEER, 3)],
              sm.tx_cfg(68))
    assert t["frames"] == [UDP_FRAME_0, UDP_FRAME_1, TCP_FRAME]
    assert t["owner"] == [0, 0, 1]
    assert t["status"] == [sm.ST_OK, sm.ST_OK, sm.ST_NOARP, 0, 0]
    assert t["send_status"] == [sm.ST_OK, sm.ST_OK, sm.ST_OK, sm.ST_RANGE, sm.ST_MALFORMED]
    assert t["unresolved"] == [(2, 0x0A000177)]
    # behind a gateway the table does not know: the next hop asked for is the gateway
    t = sm.tx([(TCP_SEGMENT, sm.TCP, 0xC0A80105, 0xBEEF)], dict(sm.tx_cfg(1500), gw=sm.TX_OTHER_GW))
    assert t["frames"] == [] and t["unresolved"] == [(0, sm.TX_OTHER_GW)]
    # every literal verifies under the oracle: the header checksum, and L4 on the uncut frame
    for f, want in ((UDP_FRAME_0, native.ST_OK | native.ST_IPFRAG), (UDP_FRAME_1, native.ST_OK | native.ST_IPFRAG),
                    (TCP_FRAME, native.ST_OK | native.ST_L4_OK), (OPTIONS_FRAME, native.ST_OK | native.ST_L4_OK)):
        ip = np.frombuffer(f[14:], np.uint8)
        _, st = oracle.batch_ipv4(ip, np.zeros(1, np.uint64), np.array([ip.size], np.uint32))
        assert int(st[0]) == want


def test_rx_frames_byte_by_byte():
    cfg = sm.rx_cfg()
    # the two UDP fragments as 10.0.1.16 sends them to 10.0.0.1, the later one first
    peer = dict(host=PEER, netmask=sm.NETMASK, gw=sm.GW, hw=PEER_MAC, mtu=68, arp={HOST: sm.HW})
    sent = sm.tx([(UDP_DATAGRAM, sm.UDP, HOST, 0x1234)], peer)["frames"]
    assert sent[0][:14] == bytes([0x02, 0xAB, 0x12, 0xCD, 0x34, 0xEF, 0x0C, 0x00, 0x1F, 0x10, 0x03, 0x30, 0x08, 0x00])
    assert sent[0][14 + 12:14 + 20] == bytes([0x0A, 0x00, 0x01, 0x10, 0x0A, 0x00, 0x00, 0x01])
    rx = sm.Rx(cfg)
    o = rx.batch([sent[1], ARP_FRAME, OPTIONS_FRAME, bytes(13), None, sent[0], bytes(12) + b"\x86\xdd" + bytes(40)])
    assert o["cls"] == [0, 1, 0, sm.CLS_SHORT, sm.CLS_RANGE, 0, sm.CLS_UNKNOWN]
    assert o["buckets"] == [[0, 2, 5], [1], [3, 4, 6]]
    assert o["src_mac"] == [[PEER_MAC, 0x0C001F130339, PEER_MAC], [0x001122334455]]
    assert [i["status"] for i in o["ip"]] == [sm.ST_OK | sm.ST_IPFRAG, sm.ST_OK | sm.ST_L4_OK, sm.ST_OK | sm.ST_IPFRAG]
    # 10.0.1.16 is in the table under this MAC; 10.0.1.19 is not: one learn record, index into the wire batch
    assert o["learn"] == [(0x0A000113, 2, 0x0C001F130339)] and rx.arp[0x0A000113] == 0x0C001F130339
    # the dispatch hash of ipv4::forward: addresses alone for a fragment, with the four bytes at IP + 20 for an
    # atomic datagram, which are the options here, not the ports (ip.cc:89: off + sizeof(ip_hdr))
    addr = bytes([0x0A, 0x00, 0x01, 0x10, 0x0A, 0x00, 0x00, 0x01])
    assert o["ip"][0]["hash"] == o["ip"][2]["hash"] == oracle.toeplitz(sm.RSS_KEY, addr)
    assert o["ip"][1]["hash"] == oracle.toeplitz(sm.RSS_KEY, bytes([0x0A, 0, 1, 0x13, 0x0A, 0, 0, 1, 1, 1, 1, 1]))
    assert o["ip"][1]["ihl"] == 6 and o["ip"][1]["delivered"]
    (d,) = o["delivered"]
    assert d["data"] == UDP_DATAGRAM[:6] + bytes([0x42, 0xBF]) + UDP_DATAGRAM[8:]
    assert (d["src"], d["dst"], d["id"], d["proto"]) == (PEER, HOST, 0x1234, sm.UDP)
    assert d["l4_ok"] and d["l4"] == 0 and d["plain"] and d["last"] == (0, 5) and d["head"] == (0, 5)
    # ip.cc:186-197: the addresses, then the ports of the reassembled datagram
    assert d["hash"] == oracle.toeplitz(sm.RSS_KEY, addr + bytes([0x04, 0xD2, 0x16, 0x2E]))
    assert d["shard"] == cfg["reta"][d["hash"] % 128] == batch.steer_dest(d["hash"], cfg["ncpu"], cfg["reta"])
    assert o["pending"] == set() and o["host"] == {}
    # state between batches: the first piece in one batch, the second in the next
    rx = sm.Rx(cfg)
    o = rx.batch([sent[0]])
    assert o["delivered"] == [] and o["pending"] == {(PEER, HOST, 0x1234, sm.UDP)}
    o = rx.batch([sent[1]])
    assert [x["data"] for x in o["delivered"]] == [d["data"]] and o["delivered"][0]["last"] == (1, 0)
    assert o["delivered"][0]["head"] == (0, 0) and o["pending"] == set()


def test_checksums_against_the_oracle():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 19, 20, 1499, 1500, 65515):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        got = int(oracle.ip_checksum(np.frombuffer(data, np.uint8)))  # the field as a little-endian host reads it
        assert got.to_bytes(2, "little") == sm.csum(data).to_bytes(2, "big")
    for src, dst, proto, ln in ((HOST, PEER, 17, 60), (0xFFFFFFFF, 0xFFFFFFFF, 6, 65535), (0, 0, 6, 0), (1, 2, 17, 65536),
                                (HOST, PEER, 1, 99)):
        want = oracle.pseudo_seed(src, dst, proto, ln) if proto in (6, 17) else 0
        assert sm.pseudo(src, dst, proto, ln) == want


# ---------------------------------------------------------------- the seeded traffic, layer by layer

@functools.lru_cache(maxsize=None)
def modelled(seed: int):
    """(the three wire batches, the model's output per batch, the ARP dict before each batch)."""
    batches = sm.rx_traffic(seed)
    rx = sm.Rx(sm.rx_cfg())
    outs, tables = [], []
    for frames in batches:
        tables.append(dict(rx.arp))
        outs.append(rx.batch(frames))
    return batches, outs, tables


def laid_out(frames):
    """(buffer, bytes_len, off, length) with a gap between frames; None: past the buffer."""
    parts, off, length, at = [], [], [], 3
    for k, f in enumerate(frames):
        if f is None:
            off.append(None)
            length.append(40)
            continue
        pad = k % 5
        parts.append(bytes(pad) + f)
        off.append(at + pad)
        length.append(len(f))
        at += pad + len(f)
    buf = np.frombuffer(bytes(3) + b"".join(parts), np.uint8)
    off = np.array([buf.size + 1 + k if o is None else o for k, o in enumerate(off)], np.uint64)
    return buf, int(buf.size), off, np.array(length, np.uint32)


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_rx_model_agrees_with_the_per_layer_restatements(seed):
    batches, outs, tables = modelled(seed)
    cfg = sm.rx_cfg()
    assert [len(b) for b in batches] == list(sm.BATCH_SIZES[seed])
    carry = []
    for b, (frames, o, table) in enumerate(zip(batches, outs, tables)):
        buf, bytes_len, off, length = laid_out(frames)
        # the link layer: tests/test_eth_host.py
        want = ref_eth_rx(buf, bytes_len, off, length, (sm.IPV4, sm.ARP))
        assert want["cls"].tolist() == o["cls"]
        assert want["order"].tolist() == [i for bk in o["buckets"] for i in bk]
        assert want["first"].tolist() == np.cumsum([0] + [len(bk) for bk in o["buckets"]]).tolist()
        nip, narp = len(o["buckets"][0]), len(o["buckets"][1])
        assert want["src_mac"][:nip].tolist() == o["src_mac"][0]
        assert want["src_mac"][nip:nip + narp].tolist() == o["src_mac"][1]
        # the frames call and the dispatch hash: the oracle
        ip_off, ip_len = want["l3_off"][:nip], want["l3_len"][:nip]
        _, st = oracle.batch_ipv4(buf, ip_off, ip_len)
        h, _ = oracle.batch_ipv4_rss(buf, ip_off, ip_len, sm.RSS_KEY, native.RSS_DISPATCH)
        assert st.tolist() == [i["status"] for i in o["ip"]]
        assert h.tolist() == [i["hash"] for i in o["ip"]]
        for i in o["ip"][:50]:
            assert i["shard"] == batch.steer_dest(i["hash"], cfg["ncpu"], cfg["reta"])
        # the learn records
        mac = np.array(o["src_mac"][0], np.uint64)
        rec = ref_learn(buf, bytes_len, ip_off, ip_len, st, batch.LEARN_NEED, batch.LEARN_REJECT, mac, HOST, sm.NETMASK,
                        table)
        ipi = o["buckets"][0]
        assert [(int(r["ip"]), ipi[int(r["index"])], int(r["mac"])) for r in rec] == o["learn"]
        # reassembly: tests/reasm_model.py over the carried and the new records
        recs = carry + [dict(src=k[0], dst=k[1], id=k[2], proto=k[3], offset=a, len=n, mf=mf, frame=w)
                        for w, k, a, n, mf, _ in o["frags"]]
        done, held = reasm_model.run(recs)
        state = reasm_model.buckets(recs)
        key_of = lambda r: (r["src"], r["dst"], r["id"], r["proto"])   # noqa: E731
        assert [d.key for d in done] == [(d["src"], d["dst"], d["id"], d["proto"]) for d in o["delivered"]]
        for d, m in zip(done, o["delivered"]):
            assert recs[d.last]["frame"] == m["last"] and recs[d.head]["frame"] == m["head"] and d.length == len(m["data"])
            assert m["plain"] == (state[d.last] == 1)
            assert m["shard"] == batch.steer_dest(m["hash"], cfg["ncpu"], cfg["reta"])
            assert m["seed"] == (oracle.pseudo_seed(m["src"], m["dst"], m["proto"], len(m["data"]))
                                 if m["proto"] in (6, 17) else 0)
            want_l4 = oracle.batch_spans(np.frombuffer(m["data"], np.uint8), np.zeros(1, np.uint64),
                                         np.array([len(m["data"])], np.uint32), np.array([m["seed"]], np.uint32))
            assert int(want_l4[0]).to_bytes(2, "little") == m["l4"].to_bytes(2, "big")
        assert {key_of(r) for r, s in zip(recs, state) if s == 3} == set(o["host"])
        assert {key_of(r) for r, s in zip(recs, state) if s == 2} == o["pending"]
        assert o["late_host"] == []
        carry = [r for r, s in zip(recs, state) if s == 2]


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_rx_traffic_covers_the_mix(seed):
    """Conditions on the generator, not measurements: a seed that misses one is a generator to change."""
    batches, outs, _ = modelled(seed)
    assert sorted(sm.BATCH_SIZES[seed]) == sorted(len(b) for b in batches)
    cls = [c for o in outs for c in o["cls"]]
    assert {0, 1, sm.CLS_UNKNOWN, sm.CLS_SHORT, sm.CLS_RANGE} <= set(cls)
    short = {len(f) for b in batches for f in b if f is not None and len(f) < 14}
    assert {0, 13} <= short
    ip = [i for o in outs for i in o["ip"]]
    ok = sm.ST_OK
    assert any(not i["status"] & ok for i in ip)                                       # a corrupted header checksum
    assert any(not i["status"] & ok and i["frag"] for i in ip)                         # ... on a fragment too
    assert any(i["status"] & sm.ST_MALFORMED for i in ip)                              # shorter than its IP length
    assert any(i["ihl"] > 5 and i["delivered"] for i in ip)                            # IP options, atomic
    assert any(i["ihl"] > 5 and i["frag"] and i["to_host"] for i in ip)                # ... and on fragments
    good = lambda i: i["status"] & ok and not i["status"] & sm.ST_MALFORMED           # noqa: E731
    assert any(good(i) and not i["to_host"] and not i["frag"] for i in ip)             # for another host
    assert any(good(i) and not i["to_host"] and i["frag"] for i in ip)
    assert any(i["delivered"] and not i["status"] & sm.ST_L4_OK for i in ip)           # L4 corrupted, atomic
    assert any(i["delivered"] and i["status"] & sm.ST_L4_OK for i in ip)
    done = [d for o in outs for d in o["delivered"]]
    assert any(d["plain"] and not d["l4_ok"] and d["proto"] == sm.UDP for d in done)   # L4 corrupted, reassembled
    assert sum(1 for d in done if d["plain"] and d["l4_ok"]) >= 50
    assert any(d["plain"] and d["nrecs"] >= 8 for d in done)
    assert {d["proto"] for d in done if d["plain"]} >= {sm.TCP, sm.UDP, sm.ICMP}
    if sum(sm.BATCH_SIZES[seed]) > 1100:
        assert any(len(d["data"]) == sm.L4_MAX and d["plain"] for d in done)
    assert outs[-1]["pending"]                                                         # a fragment never arrives
    hosts = {k: v for o in outs for k, v in o["host"].items()}
    kinds = set()
    for recs in hosts.values():
        spans = sorted((a, a + n) for _, a, n, _ in recs)
        kinds.add("duplicate" if len(set(spans)) < len(spans) else "overlap")
    assert kinds == {"duplicate", "overlap"}
    assert any(o["learn"] for o in outs)
    # a batch boundary inside a datagram's fragments; a completing fragment in a later batch than the first
    later = [d for d in done if d["plain"] and d["head"][0] < d["last"][0]]
    assert later
    for o in outs[:-1]:
        if o["cls"]:
            assert o["pending"]
    # no two keys of one case share the 32-bit mix the device groups by (they would go to the host whole)
    keys = {k for o in outs for _, k, *_ in o["frags"]}
    lib = native.load()
    assert len({int(lib.sccsum_reasm_key_mix(*k)) for k in keys}) == len(keys)
    # a key the host was handed stays inside its batch
    assert all(len({w[0] for w, *_ in recs}) == 1 for recs in hosts.values())


@pytest.mark.parametrize("with_gw", [True, False])
@pytest.mark.parametrize("mtu", [68, 576, 1500])
def test_tx_model_agrees_with_the_per_layer_restatements(mtu, with_gw):
    dgrams = sm.tx_traffic(mtu)
    cfg = sm.tx_cfg(mtu)
    if not with_gw:
        del cfg["arp"][sm.GW]
    t = sm.tx(dgrams, cfg)
    assert (sm.GW in {h for _, h in t["unresolved"]}) == (not with_gw)
    lens = [len(d[0]) if d[0] is not None else 10 for d in dgrams]
    assert max(lens) > sm.L4_MAX and lens.count(sm.L4_MAX) >= 2 and any(d[0] is None for d in dgrams)
    assert {sm.ST_OK, sm.ST_NOARP, 0} == set(t["status"]) and t["unresolved"]
    # ipv4::send: tests/test_send_host.py on the datagrams with their checksum stored
    stored = [x if x is not None else b"" for x in t["l4"]]
    buf = np.frombuffer(b"".join(stored), np.uint8)
    length = np.array([len(x) for x in stored], np.uint32)
    off = (np.cumsum(length) - length).astype(np.uint64)
    for i, d in enumerate(dgrams):
        if d[0] is None:
            off[i], length[i] = buf.size + 1, 10
    dst = np.array([d[2] for d in dgrams], np.uint32)
    proto = np.array([d[1] for d in dgrams], np.uint8)
    ids = np.array([d[3] for d in dgrams], np.uint16)
    want = expected_send(buf, off, length, dst, proto, mtu, HOST, ids=ids)
    assert want["status"].tolist() == t["send_status"]
    resolved = [i for i, s in enumerate(t["status"]) if s == sm.ST_OK]
    ip_frames = [bytes(f) for f, (i, _) in zip(want["frames"], want["owner"]) if i in set(resolved)]
    assert ip_frames == [f[14:] for f in t["frames"]]
    # the L4 checksum: every uncut frame verifies under the oracle
    for f in t["frames"][:200]:
        ip = np.frombuffer(f[14:], np.uint8)
        _, st = oracle.batch_ipv4(ip, np.zeros(1, np.uint64), np.array([ip.size], np.uint32))
        l4 = sm.l4_field(ip[9], ip.size - 20)
        assert st[0] & native.ST_OK and (st[0] & native.ST_IPFRAG or st[0] & native.ST_L4_OK or l4 is None)
    # the link layer: tests/test_eth_host.py on send's lists
    desc = batch.make_desc(np.arange(int(want["first"][-1])), np.zeros(int(want["first"][-1])),
                           np.zeros(int(want["first"][-1])))
    e = ref_eth_send(dict(hw_address=sm.HW, host=HOST, netmask=sm.NETMASK, gw=sm.GW, eth_proto=sm.IPV4), cfg["arp"], dst,
                     want["dgram_first"], desc, want["first"], want["out_off"], want["out_len"], 0xFFFFFFFF, 0)
    assert e["status"].tolist() == t["status"]
    assert [(int(u["dgram"]), int(u["next_hop"])) for u in e["unresolved"]] == t["unresolved"]
    assert bytes(e["eth"]) == b"".join(f[:14] for f in t["frames"])
    assert [int(want["owner"][int(f)][0]) for f in e["frame_src"]] == t["owner"]
