"""The link layer, the host side (no device needed): the new C-ABI symbols,
the ARP table's lookup against a dict, every argument error (reported before
any device work), the C++ classes, and the numpy restatement of the
reference that tests/test_gpu_eth.py compares the device results with, pinned
here by three frames written out byte by byte.

The restatement (paths relative to the reference tree):
  dispatch_packet     eth_hdr = get_header<eth_hdr>(0), null for < 14 bytes;
                      ntoh; _proto_map.find(eth_proto), unknown: dropped;
                      from = src_mac; trim_front(14)           src/net/net.cc:324-357
  eth_hdr             dst_mac[6], src_mac[6], eth_proto (be16)  include/seastar/net/net.hh (eth_hdr)
  learn               if (in_my_netmask(h.src_ip) && h.src_ip != _host_address)
                          _arp.learn(from, h.src_ip)             src/net/ip.cc:147-149
  get_l2_dst_address  dst = in_my_netmask(to) ? to : _gw_address;
                      _arp.lookup(dst)                           ip.cc:231-242
  in_my_netmask       !((a.ip ^ _host_address.ip) & _netmask.ip) ip.cc:116-119
  packet provider     eh->dst_mac = to; eh->src_mac = _hw_address;
                      eh->eth_proto = proto_num; hton            net.cc:266-284
A MAC is the six wire bytes as a big-endian number."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import cpp_host
from seastar_amd import batch, native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = native.SCCSUM_EINVAL
ETH = native.ETH_HDR
IPV4, ARP = 0x0800, 0x0806
DESC_DTYPE = batch.DESC_DTYPE


# ---------------------------------------------------------------- the restatement

def _u64(a) -> np.ndarray:
    return np.asarray(a).astype(np.uint64)


def _byte_at(data: np.ndarray, idx: np.ndarray) -> np.ndarray:
    return data[idx.astype(np.int64)].astype(np.uint64)


def ref_in_buffer(bytes_len: int, off, length) -> np.ndarray:
    """The 64-bit range test of sccsum_spans: [off, off + len) inside [0, bytes_len)."""
    off, length = _u64(off), _u64(length)
    blen = np.uint64(bytes_len)
    inside = off <= blen
    return inside & (length <= blen - np.where(inside, off, blen))


def ref_eth_rx(data: np.ndarray, bytes_len: int, off, length, protos) -> dict:
    """dispatch_packet for a batch.  cls [n] in arrival order; first [K + 2];
    order, l3_off, l3_len, src_mac [n] in grouped order (a stable partition)."""
    off, length = _u64(off), _u64(length)
    n, k_protos = int(off.size), len(protos)
    inside = ref_in_buffer(bytes_len, off, length)
    readable = inside & (length >= ETH)
    at = np.where(readable, off, 0)
    proto = np.zeros(n, dtype=np.uint64)
    mac = np.zeros(n, dtype=np.uint64)
    if data.size >= ETH:
        proto = (_byte_at(data, at + 12) << 8) | _byte_at(data, at + 13)
        for k in range(6):
            mac = (mac << np.uint64(8)) | _byte_at(data, at + 6 + k)
    cls = np.full(n, native.ETH_UNKNOWN, dtype=np.uint8)
    for k, p in enumerate(protos):
        cls[readable & (proto == p)] = k
    cls[inside & ~readable] = native.ETH_SHORT
    cls[~inside] = native.ETH_RANGE
    classified = cls < k_protos
    bucket = np.where(classified, cls, k_protos).astype(np.int64)
    order = np.argsort(bucket, kind="stable")
    first = np.concatenate([[0], np.cumsum(np.bincount(bucket, minlength=k_protos + 1))]).astype(np.uint32)
    return dict(cls=cls, first=first, order=order.astype(np.uint32),
                l3_off=np.where(classified, off + np.uint64(ETH), off)[order],
                l3_len=np.where(classified, length - np.uint64(ETH), 0).astype(np.uint32)[order],
                src_mac=np.where(classified, mac, 0).astype(np.uint64)[order])


def _table_arrays(table):
    """A dict {ip: mac} as sorted key / value arrays."""
    keys = np.array(sorted(table or {}), dtype=np.uint64)
    vals = np.array([table[int(k)] for k in keys], dtype=np.uint64)
    return keys, vals


def _table_find(table, ips: np.ndarray):
    """(hit [n], mac [n]) of every ip through a dict table."""
    keys, vals = _table_arrays(table)
    ips = _u64(ips)
    if not keys.size:
        return np.zeros(ips.size, dtype=bool), np.zeros(ips.size, dtype=np.uint64)
    pos = np.minimum(np.searchsorted(keys, ips), keys.size - 1)
    hit = keys[pos] == ips
    return hit, np.where(hit, vals[pos], 0).astype(np.uint64)


def ref_learn(data: np.ndarray, bytes_len: int, off, length, status, need: int, reject: int, src_mac, host: int,
              netmask: int, table) -> np.ndarray:
    """The learn candidates of ip.cc:147-149 among an IPv4 bucket, as
    batch.ARP_REC_DTYPE records in arrival order.  A frame outside the buffer
    or shorter than an IP header is never read."""
    off, length = _u64(off), _u64(length)
    st = np.asarray(status).astype(np.int64)
    passes = ((st & need) == need) & ((st & reject) == 0)
    ok = passes & ref_in_buffer(bytes_len, off, length) & (length >= 20)
    at = np.where(ok, off, 0)
    src = np.zeros(off.size, dtype=np.uint64)
    if data.size >= 20:
        for k in range(4):
            src = (src << np.uint64(8)) | _byte_at(data, at + 12 + k)
    mac = _u64(src_mac)
    hit, known = _table_find(table, src)
    keep = ok & (((src ^ np.uint64(host)) & np.uint64(netmask)) == 0) & (src != host) & ~(hit & (known == mac))
    rec = np.zeros(int(keep.sum()), dtype=batch.ARP_REC_DTYPE)
    rec["ip"] = src[keep]
    rec["index"] = np.flatnonzero(keep)
    rec["mac"] = mac[keep]
    return rec


def ref_eth_header(dst_mac: int, src_mac: int, eth_proto: int) -> bytes:
    return int(dst_mac).to_bytes(6, "big") + int(src_mac).to_bytes(6, "big") + int(eth_proto).to_bytes(2, "big")


def _ranges(lo: np.ndarray, count: np.ndarray) -> np.ndarray:
    """Concatenation of [lo_i, lo_i + count_i)."""
    total = int(count.sum())
    starts = np.cumsum(count) - count
    return np.repeat(lo - starts, count) + np.arange(total, dtype=np.int64)


def ref_eth_send(opts: dict, table: dict, dst, dgram_first, desc: np.ndarray, first, off, length, max_out_bytes: int,
                 eth_addr: int) -> dict:
    """get_l2_dst_address + the packet provider's eth_hdr for frames given as
    fragment lists (desc: DESC_DTYPE records); eth_addr is where the call's
    Ethernet headers lie.  Capacity is the prefix rule of send."""
    dst = _u64(dst)
    n, nframes = int(dst.size), int(np.asarray(off).size)
    first = np.asarray(first).astype(np.int64)
    off, length = _u64(off), np.asarray(length).astype(np.int64)
    df = np.arange(n + 1, dtype=np.int64) if dgram_first is None else np.asarray(dgram_first).astype(np.int64)
    hi = np.minimum(df[1:], nframes)
    lo = np.minimum(df[:-1], hi)
    has = hi > lo
    hop = np.where(((dst ^ np.uint64(opts["host"])) & np.uint64(opts["netmask"])) == 0, dst, np.uint64(opts["gw"]))
    hit, mac = _table_find(table, hop)
    resolved = has & hit
    unres = has & ~hit
    wire_len = length + ETH
    psum = np.concatenate([[0], np.cumsum(wire_len)])
    nbytes = np.where(resolved, psum[hi] - psum[lo], 0)
    over = np.cumsum(nbytes) > max_out_bytes
    prefix = int(np.argmax(over)) if over.any() else n
    taken = np.arange(n) < prefix
    status = np.where(taken & resolved, native.ST_OK, np.where(taken & unres, native.ST_NOARP, 0)).astype(np.uint8)
    listed = np.flatnonzero(taken & unres)
    unresolved = np.zeros(listed.size, dtype=batch.UNRESOLVED_DTYPE)
    unresolved["dgram"] = listed
    unresolved["next_hop"] = hop[listed]
    emit = taken & resolved
    count = np.where(emit, hi - lo, 0)
    frame_src = _ranges(lo, count)
    e = int(frame_src.size)
    out_len = wire_len[frame_src]
    out_off = np.cumsum(out_len) - out_len
    ndesc = first[frame_src + 1] - first[frame_src]
    first_out = np.concatenate([[0], np.cumsum(ndesc + 1)])
    frame_mac = np.repeat(mac, count)
    eth = np.zeros((e, ETH), dtype=np.uint8)
    for k in range(6):
        eth[:, k] = (frame_mac >> np.uint64(40 - 8 * k)) & np.uint64(0xFF)
        eth[:, 6 + k] = (opts["hw_address"] >> (40 - 8 * k)) & 0xFF
    eth[:, 12] = opts["eth_proto"] >> 8
    eth[:, 13] = opts["eth_proto"] & 0xFF
    out_desc = np.zeros(int(first_out[-1]), dtype=DESC_DTYPE)
    head = first_out[:-1]
    out_desc["src"][head] = eth_addr + ETH * np.arange(e, dtype=np.uint64)
    out_desc["dst_off"][head] = out_off.astype(np.uint64) & np.uint64(0xFFFFFFFF)
    out_desc["len"][head] = ETH
    old = _ranges(first[frame_src], ndesc)                 # the input descriptors, frame by frame
    owner = np.repeat(np.arange(e), ndesc)                 # the emitted frame of each
    where = _ranges(head + 1, ndesc)
    shift = (out_off[owner].astype(np.uint64) + np.uint64(ETH) - off[frame_src][owner]) & np.uint64(0xFFFFFFFF)
    out_desc["src"][where] = desc["src"][old]
    out_desc["dst_off"][where] = (desc["dst_off"][old].astype(np.uint64) + shift) & np.uint64(0xFFFFFFFF)
    out_desc["len"][where] = desc["len"][old]
    total = np.array([int(np.where(resolved, hi - lo, 0).sum()), int(nbytes.sum()), prefix, listed.size, e,
                      int(first_out[-1])], dtype=np.uint64)
    return dict(status=status, unresolved=unresolved, frame_src=frame_src.astype(np.uint32), eth=eth.ravel(),
                out_off=out_off.astype(np.uint64), out_len=out_len.astype(np.uint32),
                first=first_out.astype(np.uint32), desc=out_desc, total=total)


# ---------------------------------------------------------------- tests

ETH_SYMBOLS = ["sccsum_arp_table_create", "sccsum_arp_table_create_host", "sccsum_arp_table_destroy",
               "sccsum_arp_table_lookup", "sccsum_arp_table_slot", "sccsum_arp_table_bits", "sccsum_eth_tile_packets",
               "sccsum_eth_rx_workspace", "sccsum_eth_rx", "sccsum_arp_learn_workspace", "sccsum_arp_learn_records",
               "sccsum_eth_send_workspace", "sccsum_eth_send"]


def test_symbols_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    declared = native.header_symbols()
    lib = native.load()
    for s in ETH_SYMBOLS:
        assert s in declared and s in exported and s in native._PROTOS, s
        assert getattr(lib, s).argtypes is not None
    assert lib.sccsum_abi_version() == native.ABI_VERSION == 4
    t = lib.sccsum_eth_tile_packets()
    assert t >= 64 and t % 64 == 0
    header = open(native.HEADER_PATH).read()
    for name, value in (("SCCSUM_ST_NOARP", native.ST_NOARP), ("SCCSUM_ETH_UNKNOWN", native.ETH_UNKNOWN),
                        ("SCCSUM_ETH_SHORT", native.ETH_SHORT), ("SCCSUM_ETH_RANGE", native.ETH_RANGE)):
        assert f"#define {name}" in header and f"0x{value:02X}u" in header.split(f"#define {name}")[1].split("\n")[0]
    assert native.ST_NOARP == 0x20 and (native.ETH_UNKNOWN, native.ETH_SHORT, native.ETH_RANGE) == (0xFF, 0xFE, 0xFD)


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"sccsum_arp_entry": native.ArpEntry, "sccsum_eth_opts": native.EthOpts}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'    printf("{cname} size %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    for cname, dtype in (("sccsum_arp_rec", batch.ARP_REC_DTYPE), ("sccsum_eth_unresolved", batch.UNRESOLVED_DTYPE)):
        lines.append(f'    printf("{cname} size %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f in dtype.names]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <sccsum.h>\nint main(void) {\n"
                   + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", exe], check=True)
    got = {tuple(line.split()[:2]): int(line.split()[2])
           for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()}
    for cname, cls in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls)
        for f, _ in cls._fields_:
            assert got[(cname, f)] == getattr(cls, f).offset, (cname, f)
    for cname, dtype in (("sccsum_arp_rec", batch.ARP_REC_DTYPE), ("sccsum_eth_unresolved", batch.UNRESOLVED_DTYPE)):
        assert got[(cname, "size")] == dtype.itemsize
        for f in dtype.names:
            assert got[(cname, f)] == dtype.fields[f][1], (cname, f)


def _bits_for(n: int) -> int:
    bits = 4
    while (1 << bits) < 2 * n:
        bits += 1
    return bits


def _check_table(pairs):
    want = {}
    for ip, mac in pairs:
        want[ip] = mac
    t = batch.ArpTable(pairs, device=None)
    assert t.bits == _bits_for(len(pairs))
    for ip, mac in want.items():
        assert t.lookup(ip) == mac, hex(ip)
    rng = np.random.default_rng(len(pairs))
    for ip in [0, 1, 0xFFFFFFFF, 0xFFFFFFFE] + rng.integers(0, 1 << 32, 300).tolist():
        assert t.lookup(ip) == want.get(ip), hex(ip)
    t.close()
    return want


def test_table_lookup_against_a_dict():
    rng = np.random.default_rng(2)
    _check_table([])                                         # n = 0: every lookup misses
    _check_table([(0x0A000001, 0x0200DEADBEEF)])             # n = 1
    assert _check_table([(0, 0x111111111111), (0xFFFFFFFF, 0xFFFFFFFFFFFF)]) == {0: 0x111111111111,
                                                                               0xFFFFFFFF: 0xFFFFFFFFFFFF}
    # the later duplicate wins, as successive learn calls do
    want = _check_table([(7, 1), (9, 2), (7, 3), (0, 4), (7, 5), (0, 6)])
    assert want == {7: 5, 9: 2, 0: 6}
    for n in (15, 16, 17, 1000, 20000):
        ips = rng.integers(0, 1 << 32, n, dtype=np.uint64) >> np.uint64(int(rng.integers(0, 24)))
        macs = rng.integers(0, 1 << 48, n, dtype=np.uint64)
        _check_table(list(zip(ips.tolist(), macs.tolist())))
    t = batch.ArpTable({0xC0A80001: "02:00:00:00:00:01", 0xC0A80002: bytes([2, 0, 0, 0, 0, 2])}, device=None)
    assert t.lookup(0xC0A80001) == 0x020000000001 and t.lookup(0xC0A80002) == 0x020000000002
    assert t.lookup(0xC0A80003) is None


def colliding_keys(bits: int, slot: int, count: int, start: int = 1) -> list:
    """`count` ips whose home slot in a table of 2^bits slots is `slot`."""
    lib = native.load()
    out, ip = [], start
    while len(out) < count:
        if lib.sccsum_arp_table_slot(ip, bits) == slot:
            out.append(ip)
        ip += 1
    return out


def test_table_colliding_keys_wrap_past_the_last_slot():
    lib = native.load()
    bits = 5
    last = (1 << bits) - 1
    # ten keys at home in the last slot but one: the third and later probes wrap to slot 0, 1, ...
    keys = colliding_keys(bits, last - 1, 10)
    others = colliding_keys(bits, 0, 3, start=1000)  # pushed along by the wrapped run
    pairs = [(ip, 0x020000000000 + ip) for ip in keys + others]
    assert _bits_for(len(pairs)) == bits
    want = _check_table(pairs)
    assert len(want) == 13
    t = batch.ArpTable(pairs, device=None)
    absent = colliding_keys(bits, last - 1, 11)[-1]     # the same home slot, not in the table: a miss after the run
    assert t.lookup(absent) is None
    assert lib.sccsum_arp_table_slot(5, 32) == 0xFFFFFFFF and lib.sccsum_arp_table_slot(5, 0) == 0
    for b in (4, 5, 21, 31):
        assert all(lib.sccsum_arp_table_slot(ip, b) < (1 << b) for ip in (0, 1, 0xFFFFFFFF, 0x0A000001))


def test_table_create_argument_errors():
    lib = native.load()
    h = ctypes.c_void_p()
    one = (native.ArpEntry * 1)(native.ArpEntry(1, 0, 2))
    wide = (native.ArpEntry * 2)(native.ArpEntry(1, 0, 2), native.ArpEntry(3, 0, 1 << 48))
    for create in (lambda *a: lib.sccsum_arp_table_create(0, *a), lib.sccsum_arp_table_create_host):
        assert create(ctypes.addressof(one), 1, None) == EINVAL
        assert create(None, 1, ctypes.byref(h)) == EINVAL and not h.value
        assert create(ctypes.addressof(wide), 2, ctypes.byref(h)) == EINVAL and not h.value
        assert create(ctypes.addressof(one), native.ARP_MAX_ENTRIES + 1, ctypes.byref(h)) == EINVAL
    rc = lib.sccsum_arp_table_create(-1, ctypes.addressof(one), 1, ctypes.byref(h))
    assert rc != 0 and not h.value                          # device -1 is refused
    assert lib.sccsum_arp_table_destroy(None) == 0 and lib.sccsum_arp_table_bits(None) == 0
    mac = ctypes.c_uint64(5)
    assert lib.sccsum_arp_table_lookup(None, 1, ctypes.byref(mac)) == 0 and mac.value == 5
    with pytest.raises(ValueError, match="mac"):
        batch.ArpTable({1: 1 << 48}, device=None)
    with pytest.raises(ValueError, match="mac"):
        batch.ArpTable({1: "02:00:00:00:01"}, device=None)
    with pytest.raises(ValueError, match="ip"):
        batch.ArpTable({1 << 32: 1}, device=None)


def test_device_calls_argument_errors_without_device():
    """A sample of each device call's argument errors through the Python
    binding (tests/cpp/eth_host.cc lists every one): all are SCCSUM_EINVAL
    before any device work, and n == 0 still needs the arrays it writes."""
    lib = native.load()
    p = 0x10000
    protos = (ctypes.c_uint16 * 9)(IPV4, ARP, 1, 2, 3, 4, 5, 6, 7)
    twice = (ctypes.c_uint16 * 2)(IPV4, IPV4)
    pa, ta = ctypes.addressof(protos), ctypes.addressof(twice)

    def rx(pr=pa, k=2, n=8, off=p, first=p, order=p, l3_off=p, l3_len=p, mac=p, ws=p):
        return lib.sccsum_eth_rx(p, 1 << 20, off, p, n, pr, k, None, first, order, l3_off, l3_len, mac, ws, None)

    for bad in (dict(pr=None), dict(k=0), dict(k=9), dict(pr=ta), dict(n=1 << 32), dict(off=None), dict(off=p + 4),
                dict(first=None), dict(first=p + 2), dict(order=None), dict(l3_off=p + 4), dict(l3_len=p + 2),
                dict(mac=None), dict(mac=p + 4), dict(ws=None), dict(ws=p + 8), dict(n=0, first=None)):
        assert rx(**bad) == EINVAL, bad

    def learn(n=8, need=1, reject=12, off=p, st=p, mac=p, rec=p, count=p, ws=p):
        return lib.sccsum_arp_learn_records(p, 1 << 20, off, p, st, need, reject, mac, n, 1, 2, None, rec, count, ws,
                                            None)

    for bad in (dict(n=1 << 31), dict(need=0x100), dict(reject=0x100), dict(off=None), dict(off=p + 4), dict(st=None),
                dict(mac=None), dict(mac=p + 4), dict(rec=None), dict(rec=p + 4), dict(count=None), dict(count=p + 2),
                dict(ws=None), dict(ws=p + 8), dict(n=0, count=None)):
        assert learn(**bad) == EINVAL, bad

    table = batch.ArpTable({1: 2}, device=None)
    good = native.EthOpts(0x020000000001, 0x0A000001, 0xFFFFFF00, 0x0A0000FE, IPV4)
    wide = native.EthOpts(1 << 48, 0x0A000001, 0xFFFFFF00, 0x0A0000FE, IPV4)

    def send(opts=good, tab=table.handle, n=8, frames=9, cap=1 << 20, dst=p, dgf=p, desc=p, first=p, off=p, ln=p, eth=p,
             desc_out=p, first_out=p, off_out=p, len_out=p, src=p, status=p, unres=p, total=p, ws=p):
        return lib.sccsum_eth_send(None if opts is None else ctypes.addressof(opts), tab, dst, dgf, n, desc, first, off,
                                   ln, frames, cap, eth, desc_out, first_out, off_out, len_out, src, status, unres,
                                   total, ws, None)

    assert send() == native.SCCSUM_ENODEV  # valid: only the host-only table's missing device copy stops it
    for bad in (dict(opts=None), dict(opts=wide), dict(tab=None), dict(n=1 << 32), dict(frames=1 << 31),
                dict(cap=1 << 32), dict(dgf=None), dict(dst=None), dict(dst=p + 2), dict(desc=p + 4), dict(first=None),
                dict(off=p + 4), dict(ln=p + 2), dict(eth=None), dict(desc_out=None), dict(desc_out=p + 4),
                dict(first_out=None), dict(off_out=p + 4), dict(len_out=None), dict(src=p + 2), dict(status=None),
                dict(unres=None), dict(unres=p + 4), dict(total=None), dict(total=p + 4), dict(ws=None),
                dict(ws=p + 8), dict(n=0, frames=0, total=None)):
        assert send(**bad) == EINVAL, bad
    for fn in (lib.sccsum_eth_rx_workspace, lib.sccsum_arp_learn_workspace, lib.sccsum_eth_send_workspace):
        for n in (0, 1, 1024, 1025, 1 << 20):
            assert fn(n) >= 16 and fn(n) % 16 == 0


def test_python_wrapper_validation():
    """eth_rx_check / arp_learn_check / eth_send_check refuse wrong dtypes,
    devices, strides and sizes before any launch."""
    n = 40
    b = batch.PacketBatch(data=torch.zeros(4096, dtype=torch.uint8), off=torch.zeros(n, dtype=torch.int64),
                          length=torch.zeros(n, dtype=torch.int32), bytes_len=4096, max_len=0)
    assert batch.eth_rx_check(b, (IPV4, ARP)) == (n, (IPV4, ARP))
    for protos in ((), tuple(range(9)), (IPV4, IPV4), (0x10000,), (-1,)):
        with pytest.raises(ValueError, match="protos"):
            batch.eth_rx_check(b, protos)
    for cls in (torch.zeros(n - 1, dtype=torch.uint8), torch.zeros(n, dtype=torch.int8),
                torch.zeros(2 * n, dtype=torch.uint8)[::2], np.zeros(n, np.uint8)):
        with pytest.raises(ValueError, match="cls"):
            batch.eth_rx_check(b, (IPV4,), cls)
    with pytest.raises(ValueError, match="PacketBatch"):
        batch.eth_rx_check(None, (IPV4,))

    ok = dict(status=torch.zeros(n, dtype=torch.uint8), src_mac=torch.zeros(n, dtype=torch.int64), host=1, netmask=2,
              table=None, need=1, reject=12)
    assert batch.arp_learn_check(b, **ok) == n
    for name, value in (("status", torch.zeros(n - 1, dtype=torch.uint8)), ("status", torch.zeros(n, dtype=torch.int8)),
                        ("src_mac", torch.zeros(n, dtype=torch.int32)), ("src_mac", torch.zeros(n - 1, dtype=torch.int64)),
                        ("src_mac", torch.zeros(2 * n, dtype=torch.int64)[::2]), ("need", 0x100), ("reject", -1),
                        ("host", 1 << 32), ("netmask", -1), ("table", object())):
        with pytest.raises(ValueError, match=name):
            batch.arp_learn_check(b, **dict(ok, **{name: value}))
    with pytest.raises(ValueError, match="^table: need an ArpTable$"):
        batch.arp_learn_check(b, **dict(ok, table=object()))
    host_table = batch.ArpTable({1: 2}, device=None)
    with pytest.raises(ValueError, match="table"):
        batch.arp_learn_check(b, **dict(ok, table=host_table))  # a host-only table is on no device

    f = 12
    lists = (torch.zeros(16 * 24, dtype=torch.uint8), torch.zeros(f + 1, dtype=torch.int32),
             torch.zeros(f, dtype=torch.int64), torch.zeros(f, dtype=torch.int32))
    sk = dict(dst=torch.zeros(f, dtype=torch.int32), dgram_first=None, table=host_table, hw_address=1, host=1,
              netmask=2, gw=3, eth_proto=IPV4, max_out_bytes=None)
    with pytest.raises(ValueError, match="table"):
        batch.eth_send_check(lists, **sk)  # every list is fine: the table's device is what is left to refuse
    for name, value in (("dst", torch.zeros(f, dtype=torch.int64)), ("dst", torch.zeros(f - 1, dtype=torch.int32)),
                        ("dgram_first", torch.zeros(f, dtype=torch.int32)),
                        ("dgram_first", torch.zeros(f + 1, dtype=torch.int64)), ("hw_address", 1 << 48),
                        ("host", 1 << 32), ("gw", -1), ("eth_proto", 1 << 16), ("max_out_bytes", 1 << 32)):
        with pytest.raises(ValueError, match="mac" if name == "hw_address" else name):
            batch.eth_send_check(lists, **dict(sk, table=_FakeDeviceTable(), **{name: value}))
    for k, value, what in ((0, torch.zeros(16 * 24 + 8, dtype=torch.uint8), "lists"),
                           (1, torch.zeros(f, dtype=torch.int32), "first"),
                           (2, torch.zeros(f, dtype=torch.int32), "off"),
                           (3, torch.zeros(f, dtype=torch.int64), "length"),
                           (3, torch.zeros(f + 1, dtype=torch.int32), "lists")):
        bad = list(lists)
        bad[k] = value
        with pytest.raises(ValueError, match=what):
            batch.eth_send_check(tuple(bad), **dict(sk, table=_FakeDeviceTable()))
    with pytest.raises(ValueError, match="lists"):
        batch.eth_send_check(lists[:3], **sk)


class _FakeDeviceTable(batch.ArpTable):
    """An ArpTable that claims the CPU tensors' device, so that eth_send_check's
    later checks are reached without a GPU."""

    def __init__(self):
        super().__init__({1: 2}, device=None)
        self.device = torch.device("cpu")


# Three frames written out byte by byte: the field offsets and the MAC encoding of the restatement.
KAT_IPV4 = bytes([
    0x02, 0x00, 0x00, 0x00, 0x00, 0x01,              # dst_mac 02:00:00:00:00:01
    0x02, 0x1A, 0x2B, 0x3C, 0x4D, 0x5E,              # src_mac 02:1a:2b:3c:4d:5e
    0x08, 0x00,                                      # eth_proto IPv4
    0x45, 0x00, 0x00, 0x1C, 0x12, 0x34, 0x00, 0x00,  # ver/ihl, tos, len 28, id, frag
    0x40, 0x11, 0x00, 0x00,                          # ttl 64, UDP, csum (not looked at here)
    0x0A, 0x00, 0x00, 0x07,                          # src 10.0.0.7
    0x0A, 0x00, 0x00, 0x01,                          # dst 10.0.0.1
    0x04, 0xD2, 0x16, 0x2E, 0x00, 0x08, 0x00, 0x00,  # UDP 1234 -> 5678, len 8
])
KAT_ARP = bytes([
    0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,              # broadcast
    0x00, 0x11, 0x22, 0x33, 0x44, 0x55,              # src_mac 00:11:22:33:44:55
    0x08, 0x06,                                      # eth_proto ARP
    0x00, 0x01, 0x08, 0x00, 0x06, 0x04, 0x00, 0x01,  # ethernet, IPv4, 6, 4, request
    0x00, 0x11, 0x22, 0x33, 0x44, 0x55, 0x0A, 0x00, 0x00, 0x09,
    0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x0A, 0x00, 0x00, 0x01,
])
KAT_IPV6 = bytes([
    0x33, 0x33, 0x00, 0x00, 0x00, 0x01,
    0xFE, 0xDC, 0xBA, 0x98, 0x76, 0x54,              # src_mac fe:dc:ba:98:76:54
    0x86, 0xDD,                                      # eth_proto IPv6: not registered
    0x60, 0x00, 0x00, 0x00, 0x00, 0x00, 0x3B, 0x40,
])


def test_known_answer_frames():
    frames = [KAT_IPV4, KAT_ARP, KAT_IPV6]
    data = np.frombuffer(b"".join(frames), dtype=np.uint8)
    length = np.array([len(f) for f in frames], dtype=np.uint32)
    off = (np.cumsum(length) - length).astype(np.uint64)
    assert list(length) == [42, 42, 22]
    r = ref_eth_rx(data, data.size, off, length, (IPV4, ARP))
    assert r["cls"].tolist() == [0, 1, 0xFF]
    assert r["first"].tolist() == [0, 1, 2, 3]            # K + 2 entries: IPv4, ARP, dropped, n
    assert r["order"].tolist() == [0, 1, 2]
    assert r["l3_off"].tolist() == [14, 42 + 14, 84]       # the dropped frame keeps its offset
    assert r["l3_len"].tolist() == [28, 28, 0]
    assert r["src_mac"].tolist() == [0x021A2B3C4D5E, 0x001122334455, 0]
    # registered the other way round, and IPv6 registered too: the class is the index into protos
    r = ref_eth_rx(data, data.size, off, length, (0x86DD, ARP, IPV4))
    assert r["cls"].tolist() == [2, 1, 0] and r["order"].tolist() == [2, 1, 0]
    assert r["src_mac"].tolist() == [0xFEDCBA987654, 0x001122334455, 0x021A2B3C4D5E]
    # cut short / outside the buffer
    r = ref_eth_rx(data, data.size, [0, 42, 84, 100], [13, 14, 23, 7], (IPV4, ARP))
    assert r["cls"].tolist() == [0xFE, 1, 0xFD, 0xFD] and r["l3_len"].tolist() == [0, 0, 0, 0]
    assert r["order"].tolist() == [1, 0, 2, 3] and r["l3_off"].tolist() == [56, 0, 84, 100]

    # the IPv4 frame behind its Ethernet header is a learn candidate of 10.0.0.1/24 ...
    args = dict(data=data, bytes_len=int(data.size), off=[14], length=[28], status=[native.ST_OK], need=native.ST_OK,
                reject=native.ST_MALFORMED | native.ST_RANGE, src_mac=[0x021A2B3C4D5E], host=0x0A000001,
                netmask=0xFFFFFF00, table=None)
    rec = ref_learn(**args)
    assert rec.tolist() == [(0x0A000007, 0, 0x021A2B3C4D5E)]
    # ... unless the table knows it with this MAC, the source is off the subnet or the host itself
    assert ref_learn(**dict(args, table={0x0A000007: 0x021A2B3C4D5E})).size == 0
    assert ref_learn(**dict(args, table={0x0A000007: 0x021A2B3C4D5F})).size == 1
    assert ref_learn(**dict(args, netmask=0xFFFFFFFF)).size == 0
    assert ref_learn(**dict(args, host=0x0A000007)).size == 0
    assert ref_learn(**dict(args, host=0x0B000001, netmask=0)).size == 1
    assert ref_learn(**dict(args, status=[0])).size == 0
    assert ref_learn(**dict(args, length=[19], need=0, reject=0)).size == 0

    assert ref_eth_header(0x020000000001, 0x021A2B3C4D5E, IPV4) == KAT_IPV4[:14]
    assert ref_eth_header(0xFFFFFFFFFFFF, 0x001122334455, ARP) == KAT_ARP[:14]
    assert batch.mac_int("02:1a:2b:3c:4d:5e") == batch.mac_int(KAT_IPV4[6:12]) == 0x021A2B3C4D5E

    # tx: the IP packet of the first frame as one descriptor, sent to 10.0.0.7 (on the link) and to
    # 192.168.1.1 (through the gateway 10.0.0.254, which the table does not know)
    opts = dict(hw_address=0x021A2B3C4D5E, host=0x0A000001, netmask=0xFFFFFF00, gw=0x0A0000FE, eth_proto=IPV4)
    desc = batch.make_desc([0x7000, 0x8000], [0, 28], [28, 28])
    s = ref_eth_send(opts, {0x0A000007: 0x020000000001}, [0x0A000007, 0xC0A80101], None, desc, [0, 1, 2], [0, 28],
                     [28, 28], 1 << 20, eth_addr=0x9000)
    assert s["status"].tolist() == [native.ST_OK, native.ST_NOARP]
    assert s["unresolved"].tolist() == [(1, 0x0A0000FE)]
    assert bytes(s["eth"]) == KAT_IPV4[:14]
    assert s["desc"].tolist() == [(0x9000, 0, 14), (0x7000, 14, 28)]
    assert s["first"].tolist() == [0, 2] and s["out_off"].tolist() == [0] and s["out_len"].tolist() == [42]
    assert s["frame_src"].tolist() == [0] and s["total"].tolist() == [1, 42, 2, 1, 1, 2]
    # a cap one byte short: nothing is emitted or listed from the first resolved datagram on
    s = ref_eth_send(opts, {0x0A000007: 0x020000000001}, [0xC0A80101, 0x0A000007, 0xC0A80101], None,
                     batch.make_desc([1, 2, 3], [0, 28, 56], [28, 28, 28]), [0, 1, 2, 3], [0, 28, 56], [28, 28, 28], 41,
                     eth_addr=0x9000)
    assert s["status"].tolist() == [native.ST_NOARP, 0, 0] and s["total"].tolist() == [1, 42, 1, 1, 0, 0]


def test_cpp_classes_on_the_host(tmp_path):
    """seastar::net::arp_table, eth_rx and eth_tx (tests/cpp/eth_host.cc): the
    table against a std::map, workspace() against the C calls, and every
    argument error of the three device calls."""
    cpp_host.build_and_run(tmp_path, "eth_host", "eth_host: OK")


def test_cpp_classes_on_the_host_sanitized(tmp_path):
    """The same stand-alone program with eth.hip itself compiled in, its host
    side under AddressSanitizer + UndefinedBehaviorSanitizer (device code is
    not instrumented): the table's build and lookup and the argument checks."""
    cpp_host.build_and_run_sanitized(tmp_path, "eth_host", "eth.hip", "eth_host: OK")
