"""The link layer on the device (sccsum_eth_rx, sccsum_arp_learn_records,
sccsum_eth_send), compared byte for byte with the numpy restatement of the
reference in tests/test_eth_host.py.  Every output is allocated with guard
words on both sides; every comparison is exact, nothing has a tolerance."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from seastar_amd import batch, native
from test_eth_host import (ARP, ETH, IPV4, colliding_keys, ref_eth_header, ref_eth_rx, ref_eth_send, ref_learn)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16  # guard elements on either side of every output
REGISTERED = (IPV4, ARP, 0x88CC, 0x8847, 0x8863, 0x8864, 0x0842, 0x22F0)
UNKNOWN = (0x86DD, 0x8100, 0x0801, 0x0008, 0x0000, 0xFFFF)
HOST, MASK16, GW = 0x0A000001, 0xFFFF0000, 0x0A0000FE
HW = 0x02AB12CD34EF
NEED, REJECT = native.ST_OK, native.ST_MALFORMED | native.ST_RANGE


@functools.lru_cache(maxsize=None)
def _tile() -> int:
    return int(native.load().sccsum_eth_tile_packets())


def _sizes():
    t = _tile()
    return [0, 1, t - 1, t, t + 1, 2 * t + 7]


def _scale_n() -> int:
    """1 024 tiles + 1 tile + 7: the one-block carry goes into its second chunk."""
    return 1025 * _tile() + 7


class Out:
    """A guarded output: `numel` elements between GUARD poisoned ones on either side."""

    def __init__(self, dev, numel: int, dtype, fill: int, shift: int = 0):
        # shift moves the payload by whole guard blocks: other addresses for the determinism runs
        self.lead = GUARD * (1 + shift)
        self.numel, self.fill = numel, fill
        self.all = torch.full((numel + self.lead + GUARD,), fill, dtype=dtype, device=dev)
        self.t = self.all[self.lead:self.lead + numel]

    @property
    def ptr(self) -> int:
        return self.all.data_ptr() + self.lead * self.all.element_size()

    def host(self, count: int | None = None) -> np.ndarray:
        """The first `count` elements; asserts that nothing outside them was written."""
        count = self.numel if count is None else count
        h = self.all.cpu().numpy()
        assert np.all(h[:self.lead] == self.fill) and np.all(h[self.lead + count:] == self.fill), "written out of bounds"
        return h[self.lead:self.lead + count]


def _dev(dev, a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _u64_dev(dev, a) -> torch.Tensor:
    return _dev(dev, np.asarray(a, dtype=np.uint64).view(np.int64))


def _u32_dev(dev, a) -> torch.Tensor:
    return _dev(dev, np.asarray(a, dtype=np.uint32).view(np.int32))


# ---------------------------------------------------------------- eth_rx

SLOT = 80  # bytes between frame starts: room for a 60-byte frame at any of the 16 alignments


def wire_frames(rng, n: int, mix: str = "mixed", protos=REGISTERED):
    """(data, bytes_len, off, length): frames of 14-60 bytes at all 16
    alignments with their eth_proto drawn from the registered values and, for
    "mixed", unknown ones, short frames (0..13 bytes) and frames outside the
    buffer; "one" = every frame of protos[0], "dropped" = none registered."""
    bytes_len = max(n, 1) * SLOT + 5
    data = rng.integers(0, 256, size=bytes_len + 11, dtype=np.uint8)  # the buffer's padding is random too
    idx = np.arange(n, dtype=np.uint64)
    off = idx * np.uint64(SLOT) + (idx % np.uint64(16))
    length = rng.integers(ETH, 61, size=n).astype(np.uint32)
    kind = rng.random(n)
    if mix == "one":
        proto = np.full(n, protos[0])
    elif mix == "dropped":
        proto = rng.choice(UNKNOWN, size=n)
    else:
        proto = np.where(kind < 0.7, rng.choice(protos, size=n), rng.choice(UNKNOWN, size=n))
    at = off.astype(np.int64)
    data[at + 12] = proto >> 8
    data[at + 13] = proto & 0xFF
    if mix != "one":
        short = (kind >= 0.8) & (kind < 0.9) if mix == "mixed" else kind < 0.3
        length[short] = (np.arange(n) % ETH).astype(np.uint32)[short]  # 0..13
        away = kind >= 0.9 if mix == "mixed" else (kind >= 0.3) & (kind < 0.5)
        ways = np.arange(n) % 5
        off = np.where(away & (ways == 0), np.uint64(bytes_len - 5), off)               # ends past the buffer
        off = np.where(away & (ways == 1), np.uint64(bytes_len + 1), off)               # starts past it
        off = np.where(away & (ways == 2), np.uint64(1 << 63), off)
        off = np.where(away & (ways == 3), np.uint64((1 << 64) - 8), off)               # off + len wraps
        length = np.where(away & (ways == 4), np.uint32(0xFFFFFFFF), length).astype(np.uint32)
        length = np.where(away & (ways != 4), np.maximum(length, 20), length).astype(np.uint32)
    if n > 3 and mix == "mixed":
        off[1], length[1] = bytes_len, 0        # an empty frame at the very end: inside, short
        off[2], length[2] = bytes_len - 14, 14  # the last 14 bytes: inside, read
    return data, bytes_len, off.astype(np.uint64), length


def run_eth_rx(dev, d_data, bytes_len, d_off, d_len, n, protos, with_class=True, shift=0):
    """One raw call into guarded outputs; returns their host copies."""
    lib = native.load()
    k = len(protos)
    cls = Out(dev, n, torch.uint8, 0xA5, shift)
    first = Out(dev, k + 2, torch.int32, -7, shift)
    order = Out(dev, n, torch.int32, -7, shift)
    l3_off = Out(dev, n, torch.int64, -7, shift)
    l3_len = Out(dev, n, torch.int32, -7, shift)
    mac = Out(dev, n, torch.int64, -7, shift)
    wsb = int(lib.sccsum_eth_rx_workspace(n))
    ws = Out(dev, wsb // 16, torch.complex128, 3.0, shift)  # 16-byte elements: the payload stays 16-byte aligned
    assert ws.ptr % 16 == 0
    arr = (ctypes.c_uint16 * k)(*protos)
    rc = lib.sccsum_eth_rx(d_data.data_ptr(), bytes_len, d_off.data_ptr() if n else None,
                           d_len.data_ptr() if n else None, n, ctypes.addressof(arr), k,
                           cls.ptr if with_class else None, first.ptr, order.ptr if n else None,
                           l3_off.ptr if n else None, l3_len.ptr if n else None, mac.ptr if n else None, ws.ptr,
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.host()
    return dict(cls=cls.host() if with_class else cls.host(0), first=first.host().view(np.uint32),
                order=order.host().view(np.uint32), l3_off=l3_off.host().view(np.uint64),
                l3_len=l3_len.host().view(np.uint32), src_mac=mac.host().view(np.uint64))


def check_eth_rx(got, want, with_class, msg):
    for name in ("first", "order", "l3_off", "l3_len", "src_mac") + (("cls",) if with_class else ()):
        assert np.array_equal(got[name], want[name]), (msg, name)
    if not with_class:
        assert got["cls"].size == 0


@pytest.mark.parametrize("n", _sizes())
def test_eth_rx_matches_the_restatement(dev, n):
    rng = np.random.default_rng(100 + n)
    for mix in ("mixed", "one", "dropped"):
        data, bytes_len, off, length = wire_frames(rng, n, mix)
        d_data, d_off, d_len = _dev(dev, data), _u64_dev(dev, off), _u32_dev(dev, length)
        for k in (1, 2, 8):
            protos = REGISTERED[:k]
            want = ref_eth_rx(data, bytes_len, off, length, protos)
            assert int(want["first"][-1]) == n
            if n >= 1000 and mix == "mixed":
                cls = set(want["cls"].tolist())
                assert set(range(k)) | {native.ETH_UNKNOWN, native.ETH_SHORT, native.ETH_RANGE} <= cls
                if k == 8:
                    assert {int(o) % 16 for o in off[want["cls"] < k]} == set(range(16))
            if mix == "one" and n:
                assert want["first"].tolist() == [0] + [n] * (k + 1)
            if mix == "dropped":
                assert want["first"].tolist() == [0] * (k + 1) + [n]
            for with_class in (True, False):
                got = run_eth_rx(dev, d_data, bytes_len, d_off, d_len, n, protos, with_class)
                check_eth_rx(got, want, with_class, (n, mix, k, with_class))


def test_eth_rx_scale(dev):
    """More tiles than the one-block scan takes at once (tests/test_gpu_scale.py's reason)."""
    n = _scale_n()
    rng = np.random.default_rng(7)
    data, bytes_len, off, length = wire_frames(rng, n)
    want = ref_eth_rx(data, bytes_len, off, length, REGISTERED[:2])
    got = run_eth_rx(dev, _dev(dev, data), bytes_len, _u64_dev(dev, off), _u32_dev(dev, length), n, REGISTERED[:2])
    check_eth_rx(got, want, True, "scale")


def test_eth_rx_is_deterministic(dev):
    n = 2 * _tile() + 7
    data, bytes_len, off, length = wire_frames(np.random.default_rng(3), n)
    d_data, d_off, d_len = _dev(dev, data), _u64_dev(dev, off), _u32_dev(dev, length)
    a = run_eth_rx(dev, d_data, bytes_len, d_off, d_len, n, REGISTERED[:3])
    b = run_eth_rx(dev, d_data, bytes_len, d_off, d_len, n, REGISTERED[:3])
    c = run_eth_rx(dev, d_data.clone(), bytes_len, d_off.clone(), d_len.clone(), n, REGISTERED[:3], shift=3)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes() == c[name].tobytes(), name


# ---------------------------------------------------------------- learn records

def mac_of(ip) -> np.ndarray:
    """The MAC a peer sends from in these tests."""
    return (np.asarray(ip).astype(np.uint64) * np.uint64(0x10003) + np.uint64(0x020000000000)) & np.uint64((1 << 48) - 1)


@functools.lru_cache(maxsize=None)
def peers():
    """(on-subnet peers, the ten of them that share a home slot in the tables
    below and wrap past the last slot, off-subnet sources).  The subnet is
    10.0.0.0/16, the host 10.0.0.1."""
    rng = np.random.default_rng(44)
    plain = (0x0A000000 + rng.choice(np.arange(2, 60000), size=30, replace=False)).tolist()
    bits = 7  # 40 entries: 128 slots
    collide = colliding_keys(bits, (1 << bits) - 2, 10, start=0x0A000100)
    assert all((ip ^ HOST) & MASK16 == 0 for ip in collide)
    off_net = [0x0B000005, 0xC0A80101, 0x0A010001, 0, 0xFFFFFFFF]
    return plain, collide, off_net


def learn_tables():
    """name -> dict: what the table holds of the on-subnet peers."""
    plain, collide, _ = peers()
    on = plain + collide
    same = {ip: int(mac_of(ip)) for ip in on}
    mixed = {}
    for k, ip in enumerate(on):
        if k % 4 in (0, 1):
            mixed[ip] = int(mac_of(ip))            # known, this MAC
        elif k % 4 == 2:
            mixed[ip] = int(mac_of(ip)) ^ 0x100    # known, another MAC
    assert len(same) == 40 and batch.ArpTable(same, device=None).bits == 7
    return {"none": None, "same": same, "mixed": mixed}


def ip_frames(rng, n: int):
    """An IPv4 bucket: (data, bytes_len, off, length, status, src_mac) with
    every combination of the five status bits, sources on and off the subnet
    and the host itself, frames shorter than 20 bytes and outside the buffer."""
    plain, collide, off_net = peers()
    pool = np.array(plain + collide + off_net + [HOST], dtype=np.uint64)
    bytes_len = max(n, 1) * SLOT + 3
    data = rng.integers(0, 256, size=bytes_len + 13, dtype=np.uint8)
    idx = np.arange(n, dtype=np.uint64)
    off = idx * np.uint64(SLOT) + (idx % np.uint64(16))
    length = rng.integers(20, 61, size=n).astype(np.uint32)
    src = pool[rng.integers(0, pool.size, size=n)]
    at = off.astype(np.int64)
    for k in range(4):
        data[at + 12 + k] = (src >> np.uint64(24 - 8 * k)) & np.uint64(0xFF)
    kind = rng.random(n)
    length[kind < 0.1] = (np.arange(n) % 20).astype(np.uint32)[kind < 0.1]               # 0..19: no IP header
    away = (kind >= 0.1) & (kind < 0.2)
    ways = np.arange(n) % 3
    off = np.where(away & (ways == 0), np.uint64(bytes_len - 10), off)
    off = np.where(away & (ways == 1), np.uint64(bytes_len + 1), off)
    length = np.where(away & (ways == 2), np.uint32(0xFFFFFFF0), length).astype(np.uint32)
    status = (np.arange(n) % 32).astype(np.uint8)                                         # every combination of 5 bits
    rng.shuffle(status)
    src_mac = mac_of(src)
    return data, bytes_len, off.astype(np.uint64), length, status, src_mac


def run_learn(dev, d, n, need, reject, host, netmask, table, shift=0):
    lib = native.load()
    rec = Out(dev, 2 * n, torch.int64, -7, shift)
    count = Out(dev, 1, torch.int32, -7, shift)
    wsb = int(lib.sccsum_arp_learn_workspace(n))
    ws = Out(dev, wsb // 16, torch.complex128, 3.0, shift)
    d_data, d_off, d_len, d_st, d_mac = d
    rc = lib.sccsum_arp_learn_records(d_data.data_ptr(), d_data.bytes_len, d_off.data_ptr() if n else None, d_len.data_ptr() if n else None,
                                      d_st.data_ptr() if n else None, need, reject, d_mac.data_ptr() if n else None, n,
                                      host, netmask, None if table is None else table.handle, rec.ptr if n else None,
                                      count.ptr, ws.ptr, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.host()
    m = int(count.host().view(np.uint32)[0])
    assert m <= n
    return rec.host(2 * m).view(batch.ARP_REC_DTYPE)


class _Data:
    """A device byte buffer that remembers how many bytes are valid."""

    def __init__(self, t, bytes_len):
        self.t, self.bytes_len = t, bytes_len

    def data_ptr(self):
        return self.t.data_ptr()


def _learn_inputs(dev, data, bytes_len, off, length, status, src_mac):
    return (_Data(_dev(dev, data), bytes_len), _u64_dev(dev, off), _u32_dev(dev, length), _dev(dev, status),
            _u64_dev(dev, src_mac))


@pytest.fixture(scope="module")
def device_tables(dev):
    tabs = {name: (None if t is None else batch.ArpTable(t)) for name, t in learn_tables().items()}
    yield tabs
    for t in tabs.values():
        if t is not None:
            t.close()


@pytest.mark.parametrize("n", _sizes())
def test_learn_records_match_the_restatement(dev, device_tables, n):
    rng = np.random.default_rng(200 + n)
    data, bytes_len, off, length, status, src_mac = ip_frames(rng, n)
    d = _learn_inputs(dev, data, bytes_len, off, length, status, src_mac)
    tables = learn_tables()
    kept = {}
    for name, table in tables.items():
        for need, reject in ((NEED, REJECT), (0, 0), (native.ST_OK | native.ST_L4_OK, native.ST_IPFRAG)):
            for host, netmask in ((HOST, MASK16), (HOST, 0), (HOST, 0xFFFFFFFF), (0x0B000005, 0xFF000000)):
                want = ref_learn(data, bytes_len, off, length, status, need, reject, src_mac, host, netmask, table)
                got = run_learn(dev, d, n, need, reject, host, netmask, device_tables[name])
                assert got.tobytes() == want.tobytes(), (n, name, need, reject, hex(netmask))
                kept[(name, need, netmask)] = want
    if n >= 1000:
        # the cases bite: new pairs without a table, none in the steady state, the changed MACs in between
        assert kept[("none", NEED, MASK16)].size > kept[("mixed", NEED, MASK16)].size > 0
        assert kept[("same", NEED, MASK16)].size == 0 and kept[("same", 0, MASK16)].size == 0
        assert kept[("none", 0, 0)].size > kept[("none", 0, MASK16)].size  # netmask 0: every source is on the link
        assert kept[("none", 0, 0xFFFFFFFF)].size == 0                     # /32: only the host itself, which is skipped
        _, collide, _ = peers()
        assert set(collide) <= set(kept[("none", 0, MASK16)]["ip"].tolist())
        assert set(kept[("mixed", 0, MASK16)]["ip"].tolist()) & set(collide)
        # frames without an IP header or outside the buffer pass need = reject = 0 and are still skipped
        idx = kept[("none", 0, 0)]["index"]
        assert np.all(length[idx] >= 20) and np.all(off[idx] + length[idx] <= bytes_len)
        assert np.any(length < 20) and np.any(off > bytes_len)


def test_learn_records_scale_and_determinism(dev, device_tables):
    n = _scale_n()
    rng = np.random.default_rng(9)
    data, bytes_len, off, length, status, src_mac = ip_frames(rng, n)
    length = np.where(np.arange(n) % 7 == 0, np.uint32(14), length).astype(np.uint32)  # frames of 14-60 bytes
    d = _learn_inputs(dev, data, bytes_len, off, length, status, src_mac)
    want = ref_learn(data, bytes_len, off, length, status, 0, 0, src_mac, HOST, MASK16, learn_tables()["mixed"])
    assert want.size > _tile() * 100
    a = run_learn(dev, d, n, 0, 0, HOST, MASK16, device_tables["mixed"])
    assert a.tobytes() == want.tobytes()
    b = run_learn(dev, d, n, 0, 0, HOST, MASK16, device_tables["mixed"], shift=2)
    assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- eth_send

def send_opts(**kw) -> dict:
    return dict(dict(hw_address=HW, host=HOST, netmask=MASK16, gw=GW, eth_proto=IPV4), **kw)


def run_eth_send(dev, table, opts, d_dst, d_dgram_first, n, lists, cap, shift=0):
    """One raw call into guarded outputs; returns (host copies trimmed to what
    d_total says was emitted, the device outputs)."""
    lib = native.load()
    d_desc, d_first, d_off, d_len = lists
    nframes = int(d_off.numel())
    ndesc = int(d_desc.numel()) // 16
    eth = Out(dev, ETH * nframes, torch.uint8, 0xA5, shift)
    desc = Out(dev, 2 * (ndesc + nframes), torch.int64, -7, shift)
    first = Out(dev, nframes + 1, torch.int32, -7, shift)
    out_off = Out(dev, nframes, torch.int64, -7, shift)
    out_len = Out(dev, nframes, torch.int32, -7, shift)
    src = Out(dev, nframes, torch.int32, -7, shift)
    status = Out(dev, n, torch.uint8, 0xA5, shift)
    unres = Out(dev, n, torch.int64, -7, shift)
    total = Out(dev, 6, torch.int64, -7, shift)
    wsb = int(lib.sccsum_eth_send_workspace(n))
    ws = Out(dev, wsb // 16, torch.complex128, 3.0, shift)
    o = native.EthOpts(opts["hw_address"], opts["host"], opts["netmask"], opts["gw"], opts["eth_proto"])
    rc = lib.sccsum_eth_send(ctypes.addressof(o), table.handle, d_dst.data_ptr() if n else None,
                             None if d_dgram_first is None else d_dgram_first.data_ptr(), n,
                             d_desc.data_ptr() if ndesc else None, d_first.data_ptr() if nframes else None,
                             d_off.data_ptr() if nframes else None, d_len.data_ptr() if nframes else None, nframes, cap,
                             eth.ptr, desc.ptr, first.ptr, out_off.ptr, out_len.ptr, src.ptr, status.ptr, unres.ptr,
                             total.ptr, ws.ptr, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.host()
    t = total.host().view(np.uint64)
    e, d, u = int(t[4]), int(t[5]), int(t[3])
    assert e <= nframes and d <= ndesc + nframes and u <= n
    got = dict(total=t, status=status.host(), unresolved=unres.host(u).view(batch.UNRESOLVED_DTYPE),
               eth=eth.host(ETH * e), desc=desc.host(2 * d).view(batch.DESC_DTYPE),
               first=first.host(e + 1).view(np.uint32), out_off=out_off.host(e).view(np.uint64),
               out_len=out_len.host(e).view(np.uint32), frame_src=src.host(e).view(np.uint32))
    return got, dict(eth=eth, desc=desc)


def check_eth_send(got, want, msg):
    for name in ("total", "status", "unresolved", "frame_src", "eth", "out_off", "out_len", "first", "desc"):
        assert got[name].tobytes() == want[name].tobytes(), (msg, name)


def gathered(dev, outs, got) -> np.ndarray:
    """sccsum_gather over the emitted descriptors: the packed wire bytes."""
    nbytes = int(got["out_off"][-1] + got["out_len"][-1]) if got["out_len"].size else 0
    dst = torch.full((nbytes + 32,), 0x5A, dtype=torch.uint8, device=dev)
    nd = int(got["desc"].size)
    if nd:
        rc = native.load().sccsum_gather(outs["desc"].ptr, nd, dst.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    h = dst.cpu().numpy()
    assert np.all(h[nbytes:] == 0x5A)
    return h[:nbytes]


def wire_bytes(want, frame_bytes) -> np.ndarray:
    """The restatement's wire frames: the Ethernet header, then the input frame."""
    eth = want["eth"].reshape(-1, ETH)
    parts = []
    for k, f in enumerate(want["frame_src"].tolist()):
        parts += [eth[k], frame_bytes(f)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def destinations(rng, n: int, how: str = "mixed") -> np.ndarray:
    """Destinations on the subnet (known and unknown to send_table), behind the gateway, unresolved."""
    plain, collide, off_net = peers()
    known = np.array(plain[:20] + collide, dtype=np.uint32)
    unknown_on_link = np.array(plain[20:], dtype=np.uint32)
    behind_gw = np.array([0xC0A80101, 0x08080808, 0x0B000005, 0xFFFFFFFF, 0], dtype=np.uint32)
    if how == "resolved":
        return known[rng.integers(0, known.size, n)]
    if how == "unresolved":
        return unknown_on_link[rng.integers(0, unknown_on_link.size, n)]
    r = rng.random(n)
    return np.where(r < 0.6, known[rng.integers(0, known.size, n)],
                    np.where(r < 0.8, behind_gw[rng.integers(0, behind_gw.size, n)],
                             unknown_on_link[rng.integers(0, unknown_on_link.size, n)])).astype(np.uint32)


def send_table(with_gw: bool) -> dict:
    plain, collide, _ = peers()
    t = {ip: int(mac_of(ip)) for ip in plain[:20] + collide}
    if with_gw:
        t[GW] = 0x02000000FFFE
    return t


@pytest.fixture(scope="module")
def send_tables(dev):
    tabs = {w: (send_table(w), batch.ArpTable(send_table(w))) for w in (True, False)}
    yield tabs
    for _, t in tabs.values():
        t.close()


def l4_datagrams(dev, rng, n: int):
    """n L4 datagrams of 1..3 000 bytes, every 37th outside the buffer (refused by send: no frame)."""
    lens = rng.integers(1, 3001, size=n).astype(np.uint32)
    off = (np.cumsum(lens) - lens).astype(np.uint64)
    nbytes = int(lens.sum())
    off[np.arange(n) % 37 == 5] = nbytes + 1
    buf = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
    proto = np.where(rng.random(n) < 0.5, 17, 6).astype(np.uint8)
    return batch.PacketBatch.from_host(buf, off, lens, device=dev), _dev(dev, proto)


@functools.lru_cache(maxsize=None)
def _sent(mtu: int):
    """ipv4_send's lists for 2 tiles + 7 datagrams at `mtu`, with the host copies the restatement takes."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(mtu)
    n = 2 * _tile() + 7
    l4, proto = l4_datagrams(dev, rng, n)
    dst = destinations(rng, n)
    r = batch.ipv4_send(l4, _u32_dev(dev, dst), proto, mtu, HOST)
    desc, first, off, length, max_len = r.lists()
    batch.ipv4_fill_desc(desc, first, off, length, max_len, mode=native.FILL_IP)
    packed = r.pack()
    torch.cuda.synchronize()
    host = dict(dst=dst, dgram_first=r.dgram_first.cpu().numpy().view(np.uint32),
                desc=desc.cpu().numpy().view(batch.DESC_DTYPE), first=first.cpu().numpy().view(np.uint32),
                off=off.cpu().numpy().view(np.uint64), length=length.cpu().numpy().view(np.uint32),
                packed=packed.data.cpu().numpy(), status=r.status.cpu().numpy())
    assert np.any(host["status"] != native.ST_OK) and np.any(np.diff(host["dgram_first"].astype(np.int64)) == 0)
    return r, (desc, first, off, length), host


def _frame_bytes(host):
    return lambda f: host["packed"][int(host["off"][f]):int(host["off"][f]) + int(host["length"][f])]


@pytest.mark.parametrize("mtu", [68, 576, 1500])
def test_eth_send_on_ipv4_send_lists(dev, send_tables, mtu):
    r, lists, host = _sent(mtu)
    n = int(host["dst"].size)
    d_dst = _u32_dev(dev, host["dst"])
    for with_gw in (True, False):  # False: the gateway itself is unresolved
        table, d_table = send_tables[with_gw]
        got, outs = run_eth_send(dev, d_table, send_opts(), d_dst, r.dgram_first, n, lists, 0xFFFFFFFF)
        want = ref_eth_send(send_opts(), table, host["dst"], host["dgram_first"], host["desc"], host["first"],
                            host["off"], host["length"], 0xFFFFFFFF, outs["eth"].ptr)
        check_eth_send(got, want, (mtu, with_gw))
        st = want["status"]
        assert np.any(st == native.ST_OK) and np.any(st == native.ST_NOARP) and np.any(st == 0)
        assert int(want["total"][2]) == n and int(want["total"][0]) == int(want["total"][4])
        assert bool(np.any(want["unresolved"]["next_hop"] == GW)) == (not with_gw)
        assert np.array_equal(gathered(dev, outs, got), wire_bytes(want, _frame_bytes(host))), (mtu, with_gw)
    # netmask 0, the reference's initial value: every destination is on the link, the gateway is never asked
    table, d_table = send_tables[True]
    opts = send_opts(netmask=0)
    got, outs = run_eth_send(dev, d_table, opts, d_dst, r.dgram_first, n, lists, 0xFFFFFFFF)
    want = ref_eth_send(opts, table, host["dst"], host["dgram_first"], host["desc"], host["first"], host["off"],
                        host["length"], 0xFFFFFFFF, outs["eth"].ptr)
    check_eth_send(got, want, (mtu, "netmask 0"))
    assert not np.any(want["unresolved"]["next_hop"] == GW) and want["unresolved"].size


def test_eth_send_caps(dev, send_tables):
    """The prefix rule: a cap in the first tile, in a later tile, exactly on a
    datagram's end, one byte short of it, and 0; d_total reports the full need
    for every cap, and a rerun with it emits everything."""
    r, lists, host = _sent(576)
    n, t = int(host["dst"].size), _tile()
    table, d_table = send_tables[True]
    d_dst = _u32_dev(dev, host["dst"])
    args = (host["dst"], host["dgram_first"], host["desc"], host["first"], host["off"], host["length"])
    full = ref_eth_send(send_opts(), table, *args, 0xFFFFFFFF, 0)
    need_frames, need_bytes = int(full["total"][0]), int(full["total"][1])
    ends = full["out_off"] + full["out_len"]                      # where every emitted frame ends in the layout
    dgram_of_frame = np.searchsorted(host["dgram_first"], full["frame_src"], side="right") - 1
    last_of_dgram = np.flatnonzero(np.append(np.diff(dgram_of_frame) != 0, True))
    dgram_ends = ends[last_of_dgram]                              # layout bytes through each emitted datagram
    owners = dgram_of_frame[last_of_dgram]
    in_first = int(dgram_ends[np.searchsorted(owners, t // 3)])
    in_later = int(dgram_ends[np.searchsorted(owners, t + t // 2)])
    on_tile = int(dgram_ends[np.searchsorted(owners, t) - 1])     # everything the first tile's datagrams need
    for cap in (0, 13, in_first, in_first - 1, in_first + 5, in_later, in_later - 1, on_tile, on_tile - 1,
                need_bytes - 1, need_bytes):
        got, outs = run_eth_send(dev, d_table, send_opts(), d_dst, r.dgram_first, n, lists, cap)
        want = ref_eth_send(send_opts(), table, *args, cap, outs["eth"].ptr)
        check_eth_send(got, want, cap)
        assert int(got["total"][0]) == need_frames and int(got["total"][1]) == need_bytes
        prefix = int(got["total"][2])
        assert (prefix == n) == (cap >= need_bytes)
        assert np.all(got["status"][prefix:] == 0)
        assert int((got["out_off"] + got["out_len"]).max(initial=0)) <= cap
        assert np.array_equal(gathered(dev, outs, got), wire_bytes(want, _frame_bytes(host))), cap
    assert int(ref_eth_send(send_opts(), table, *args, in_first, 0)["total"][2]) < t < \
        int(ref_eth_send(send_opts(), table, *args, in_later, 0)["total"][2]) < n
    got, _ = run_eth_send(dev, d_table, send_opts(), d_dst, r.dgram_first, n, lists, int(got["total"][1]))
    assert int(got["total"][4]) == need_frames and int(got["total"][2]) == n


def hand_built(dev, rng, n: int, lo: int = 20, hi: int = 200):
    """n frames, one per datagram, each 1-5 descriptors over a device buffer of
    random bytes, at layout positions that are not packed from 0."""
    lens = rng.integers(lo, hi + 1, size=n).astype(np.uint32)
    pieces = 1 + (np.arange(n) % 5)
    pieces = np.minimum(pieces, lens).astype(np.int64)
    nbytes = int(lens.sum())
    src_buf = rng.integers(0, 256, size=nbytes + 16, dtype=np.uint8)
    d_src = _dev(dev, src_buf)
    start = (np.cumsum(lens) - lens).astype(np.int64)     # where the frame's bytes lie in src_buf
    off = (start + 1000).astype(np.uint64)                # its position in the caller's layout
    first = np.concatenate([[0], np.cumsum(pieces)]).astype(np.uint32)
    owner = np.repeat(np.arange(n), pieces)
    j = np.arange(owner.size) - first[:-1].astype(np.int64)[owner]
    base = (lens[owner] // pieces[owner]).astype(np.int64)
    p_off = j * base                                       # equal pieces, the last takes the rest
    p_len = np.where(j == pieces[owner] - 1, lens[owner] - p_off, base)
    desc = batch.make_desc(d_src.data_ptr() + start[owner] + p_off, off[owner].astype(np.int64) + p_off, p_len)
    lists = (_dev(dev, desc.view(np.uint8)), _u32_dev(dev, first), _u64_dev(dev, off), _u32_dev(dev, lens))
    host = dict(desc=desc, first=first, off=off, length=lens)
    return lists, host, (lambda f: src_buf[int(start[f]):int(start[f]) + int(lens[f])]), d_src


@pytest.mark.parametrize("how", ["mixed", "resolved", "unresolved"])
def test_eth_send_hand_built_lists_without_dgram_first(dev, send_tables, how):
    rng = np.random.default_rng(5)
    n = 2 * _tile() + 7
    lists, host, frame_bytes, keep = hand_built(dev, rng, n)
    dst = destinations(rng, n, how)
    table, d_table = send_tables[False]
    opts = send_opts(eth_proto=0x88CC)
    got, outs = run_eth_send(dev, d_table, opts, _u32_dev(dev, dst), None, n, lists, 0xFFFFFFFF)
    want = ref_eth_send(opts, table, dst, None, host["desc"], host["first"], host["off"], host["length"], 0xFFFFFFFF,
                        outs["eth"].ptr)
    check_eth_send(got, want, how)
    e, u = int(want["total"][4]), int(want["total"][3])
    assert e + u == n and {"mixed": 0 < e < n, "resolved": e == n, "unresolved": e == 0}[how]
    assert np.array_equal(gathered(dev, outs, got), wire_bytes(want, frame_bytes))
    del keep


def test_eth_send_no_datagrams(dev, send_tables):
    table, d_table = send_tables[True]
    empty = (torch.zeros(0, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
             torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev))
    got, _ = run_eth_send(dev, d_table, send_opts(), torch.zeros(0, dtype=torch.int32, device=dev), None, 0, empty, 100)
    assert got["total"].tolist() == [0] * 6 and got["first"].tolist() == [0]


def test_eth_send_scale_and_determinism(dev, send_tables):
    n = _scale_n()
    rng = np.random.default_rng(12)
    lists, host, frame_bytes, keep = hand_built(dev, rng, n, lo=14, hi=60)
    dst = destinations(rng, n)
    table, d_table = send_tables[True]
    d_dst = _u32_dev(dev, dst)
    need = ref_eth_send(send_opts(), table, dst, None, host["desc"], host["first"], host["off"], host["length"],
                        0xFFFFFFFF, 0)["total"]
    cap = int(need[1]) - 40  # falls in the last tiles, past the scan's first chunk of 1 024 tiles
    a, outs_a = run_eth_send(dev, d_table, send_opts(), d_dst, None, n, lists, cap)
    want = ref_eth_send(send_opts(), table, dst, None, host["desc"], host["first"], host["off"], host["length"], cap,
                        outs_a["eth"].ptr)
    check_eth_send(a, want, "scale")
    assert 1024 * _tile() < int(want["total"][2]) < n
    b, outs_b = run_eth_send(dev, d_table, send_opts(), d_dst, None, n, lists, cap, shift=2)
    moved = outs_b["eth"].ptr - outs_a["eth"].ptr
    assert moved != 0
    heads = a["first"][:-1].astype(np.int64)
    for name in a:
        if name == "desc":  # the Ethernet descriptors hold d_eth's address: equal once the move is taken out
            fixed = b["desc"].copy()
            fixed["src"][heads] = (fixed["src"][heads].astype(np.int64) - moved).astype(np.uint64)
            assert a["desc"].tobytes() == fixed.tobytes()
        else:
            assert a[name].tobytes() == b[name].tobytes(), name
    del keep


def single_desc_frames(dev, rng, n: int, lo: int = 20, hi: int = 60):
    """n frames of one descriptor each whose bytes lie anywhere in one 1 MiB
    device buffer of random bytes (sources may overlap: nothing is written
    through them), packed back to back in the caller's layout."""
    pool = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)
    d_pool = _dev(dev, pool)
    lens = rng.integers(lo, hi + 1, size=n).astype(np.uint32)
    start = rng.integers(0, pool.size - hi, size=n)
    off = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    first = np.arange(n + 1, dtype=np.uint32)
    desc = batch.make_desc(d_pool.data_ptr() + start, off & np.uint64(0xFFFFFFFF), lens)
    lists = (_dev(dev, desc.view(np.uint8)), _u32_dev(dev, first), _u64_dev(dev, off), _u32_dev(dev, lens))
    host = dict(desc=desc, first=first, off=off, length=lens)
    return lists, host, (lambda f: pool[int(start[f]):int(start[f]) + int(lens[f])]), d_pool


def test_eth_send_emits_more_frames_than_the_emit_grid_has_slots(dev, send_tables):
    """eth_send_emit_kernel runs at most kEmitMaxBlocks * kEmitBlock = 16 384 *
    256 threads and strides over the frames past that: 4 194 304 + one tile + 7
    frames take the loop's second trip (send.hip's twin:
    test_send_emits_more_frames_than_the_emit_grid_has_slots).  The build
    exposes no getter for the two constants; the product is stated here."""
    grid = 16384 * 256
    n = grid + _tile() + 7
    rng = np.random.default_rng(14)
    lists, host, frame_bytes, keep = single_desc_frames(dev, rng, n)
    dst = destinations(rng, n, "resolved")
    table, d_table = send_tables[True]
    got, outs = run_eth_send(dev, d_table, send_opts(), _u32_dev(dev, dst), None, n, lists, 0xFFFFFFFF)
    want = ref_eth_send(send_opts(), table, dst, None, host["desc"], host["first"], host["off"], host["length"],
                        0xFFFFFFFF, outs["eth"].ptr)
    assert int(want["total"][4]) == n == int(want["total"][2]) and int(want["total"][1]) < 0xFFFFFFFF
    check_eth_send(got, want, "past the emit grid")
    packed = gathered(dev, outs, got)
    sample = np.unique(np.concatenate([np.arange(0, 64), np.arange(grid - 300, grid + 300), np.arange(n - 64, n),
                                       rng.integers(0, grid, 1500), rng.integers(grid, n, 800)]))
    eth = want["eth"].reshape(-1, ETH)
    for f in sample.tolist():
        at, ln = int(want["out_off"][f]), int(want["out_len"][f])
        assert packed[at:at + ETH].tobytes() == eth[f].tobytes(), f
        assert np.array_equal(packed[at + ETH:at + ln], frame_bytes(f)), f
    del keep


def test_device_lookup_in_a_large_table(dev):
    """table_lookup on the device in a table of 2^17 slots (about 50 000
    entries), a run of colliding keys that wraps past the last slot included,
    and in a table created with n = 0, through both eth_send and
    arp_learn_records; destinations and sources half from the table, half not.
    netmask 0: every address is on the link, so every one of them is looked up."""
    rng = np.random.default_rng(17)
    bits = 17
    run = colliding_keys(bits, (1 << bits) - 2, 14, start=0x0A000100)
    collide, absent_run = run[:12], run[12:]                         # the same home slot: held, and not held
    others = colliding_keys(bits, 0, 2, start=0x0B000000)           # pushed along by the wrapped run
    plain = np.unique(rng.integers(1, 1 << 32, 50000, dtype=np.uint64)).tolist()
    held = [ip for ip in dict.fromkeys(collide + others + plain) if ip not in absent_run]
    table = {int(ip): int(mac_of(ip)) for ip in held}
    d_table, d_empty = batch.ArpTable(table), batch.ArpTable({})
    assert d_table.bits == bits and d_empty.bits == 4
    held_a = np.array(held, dtype=np.uint64)
    n = 2 * _tile() + 7
    miss = rng.integers(1, 1 << 32, n, dtype=np.uint64)
    miss = np.where(np.isin(miss, held_a), np.uint64(0), miss)      # 0 is not held
    pick = np.where(rng.random(n) < 0.5, held_a[rng.integers(0, held_a.size, n)], miss)
    pick[:2] = absent_run
    pick[4:4 + len(collide)] = collide
    pick[20:22] = others
    assert 0.3 * n < int(np.isin(pick, held_a).sum()) < 0.7 * n
    opts = send_opts(netmask=0)

    # eth_send: the destinations
    lists, host, frame_bytes, keep = hand_built(dev, rng, n)
    dst = pick.astype(np.uint32)
    for tab, d_tab in ((table, d_table), ({}, d_empty)):
        got, outs = run_eth_send(dev, d_tab, opts, _u32_dev(dev, dst), None, n, lists, 0xFFFFFFFF)
        want = ref_eth_send(opts, tab, dst, None, host["desc"], host["first"], host["off"], host["length"], 0xFFFFFFFF,
                            outs["eth"].ptr)
        check_eth_send(got, want, ("large table", len(tab)))
        assert np.array_equal(gathered(dev, outs, got), wire_bytes(want, frame_bytes))
        e, u = int(want["total"][4]), int(want["total"][3])
        assert e + u == n and (e == 0 if not tab else 0.3 * n < e < 0.7 * n)
        if tab:
            assert np.all(want["status"][4:4 + len(collide)] == native.ST_OK) and np.all(want["status"][:2] == native.ST_NOARP)

    # arp_learn_records: the sources; a held source comes with the held MAC or, every third, with another
    data, bytes_len, off, length, _, _ = ip_frames(rng, n)
    length = np.clip(length, 20, 60).astype(np.uint32)               # every frame inside the buffer, with a header
    off = np.arange(n, dtype=np.uint64) * np.uint64(SLOT)
    for k in range(4):
        data[off.astype(np.int64) + 12 + k] = (pick >> np.uint64(24 - 8 * k)) & np.uint64(0xFF)
    status = np.full(n, native.ST_OK, dtype=np.uint8)
    src_mac = mac_of(pick) ^ np.where(np.arange(n) % 3 == 0, np.uint64(0x100), np.uint64(0))
    d = _learn_inputs(dev, data, bytes_len, off, length, status, src_mac)
    for tab, d_tab in ((table, d_table), ({}, d_empty)):
        want = ref_learn(data, bytes_len, off, length, status, NEED, REJECT, src_mac, HOST, 0, tab)
        got = run_learn(dev, d, n, NEED, REJECT, HOST, 0, d_tab)
        assert got.tobytes() == want.tobytes(), ("large table", len(tab))
        if tab:
            assert 0.5 * n < want.size < 0.8 * n     # the misses, and a third of the hits
            assert not set(collide[1:]) & set(want["ip"][want["index"] % 3 != 0].tolist())
        else:
            assert want.size == n
    d_table.close()
    d_empty.close()
    del keep


def test_eth_send_with_an_inconsistent_dgram_first(dev, send_tables):
    """need_of clamps a datagram's frames [dgram_first[i], dgram_first[i + 1])
    into the frame arrays: entries beyond nframes, and a decreasing pair, which
    makes one datagram empty and lets the next take ten frames a second time.
    The first 32 frames belong to no datagram, so the frames asked for still
    fit the outputs; the result is the restatement's, which clamps the same
    way, and run_eth_send's guards see nothing written outside."""
    rng = np.random.default_rng(19)
    nframes = 2 * _tile() + 7
    lists, host, frame_bytes, keep = hand_built(dev, rng, nframes)
    n = 600
    cuts = np.sort(rng.choice(np.arange(40, nframes - 40), size=n - 4, replace=False))
    df = np.concatenate([[32], cuts, [nframes + 5, nframes + 1000, 0xFFFFFFFF, 7]]).astype(np.uint32)
    assert df.size == n + 1
    df[200] = df[199] - 10                                   # a decreasing pair
    assert df[201] > df[199] >= 42
    dst = destinations(rng, n)
    dst[195:205] = destinations(rng, 10, "resolved")
    table, d_table = send_tables[True]
    args = (dst, df, host["desc"], host["first"], host["off"], host["length"])
    need = ref_eth_send(send_opts(), table, *args, 0xFFFFFFFF, 0)["total"]
    assert int(need[0]) <= nframes - 16                      # room in every per-frame output
    for cap in (0xFFFFFFFF, int(need[1]) // 2):
        got, outs = run_eth_send(dev, d_table, send_opts(), _u32_dev(dev, dst), _u32_dev(dev, df), n, lists, cap)
        want = ref_eth_send(send_opts(), table, *args, cap, outs["eth"].ptr)
        check_eth_send(got, want, ("inconsistent dgram_first", cap))
        assert np.array_equal(gathered(dev, outs, got), wire_bytes(want, frame_bytes))
    full = ref_eth_send(send_opts(), table, *args, 0xFFFFFFFF, 0)
    assert full["status"][199] == 0 and full["status"][200] != 0       # the emptied datagram is not looked up
    assert np.all(full["status"][n - 3:] == 0)                         # nor are those wholly beyond nframes
    src = full["frame_src"].astype(np.int64)
    assert int(src.min()) >= 32 and np.any(np.diff(src) < 0)          # ten frames are emitted twice
    del keep


# ---------------------------------------------------------------- the wrappers, end to end

def test_round_trip_through_the_wrappers(dev):
    """datagrams -> ipv4_send -> ipv4_fill_desc -> eth_send -> pack() -> eth_rx
    -> ipv4_frames: every frame comes back in the IPv4 bucket with ST_OK, from
    hw_address, its L3 bytes send's own; spliced ARP and garbage frames land in
    their own buckets and leave the order of the rest intact."""
    rng = np.random.default_rng(21)
    n = _tile() + 300
    lens = rng.integers(1, 3001, size=n).astype(np.uint32)
    off = (np.cumsum(lens) - lens).astype(np.uint64)
    l4 = batch.PacketBatch.from_host(rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8), off, lens, device=dev)
    dst = destinations(rng, n, "resolved")
    proto = _dev(dev, np.full(n, 17, dtype=np.uint8))
    table = batch.ArpTable(send_table(True))
    r = batch.ipv4_send(l4, _u32_dev(dev, dst), proto, 576, HOST)
    desc, first, foff, flen, max_len = r.lists()
    batch.ipv4_fill_desc(desc, first, foff, flen, max_len, mode=native.FILL_IP)
    e = batch.eth_send(r, _u32_dev(dev, dst), table, HW, HOST, MASK16, GW)
    nframes = r.frames_emitted()
    assert e.totals() == (nframes, int(flen.sum().item()) + ETH * nframes, n, 0) and e.emitted()[0] == nframes
    assert e.unresolved().size == 0 and bool(torch.all(e.status == native.ST_OK))
    wire = e.pack()
    sent = r.pack()
    torch.cuda.synchronize()
    w_data, w_off, w_len = wire.data.cpu().numpy(), wire.off.cpu().numpy(), wire.length.cpu().numpy()
    s_data, s_off, s_len = sent.data.cpu().numpy(), sent.off.cpu().numpy(), sent.length.cpu().numpy()
    assert np.array_equal(w_len, s_len + ETH)

    # splice a few ARP and garbage frames in between
    arp = np.frombuffer(ref_eth_header(0xFFFFFFFFFFFF, 0x001122334455, ARP) + bytes(28), dtype=np.uint8)
    junk = [np.frombuffer(ref_eth_header(HW, 0x00AA00AA00AA, 0x86DD) + bytes(range(40)), dtype=np.uint8),
            np.arange(9, dtype=np.uint8)]
    extra = {0: arp, 7: junk[0], nframes // 2: arp, nframes // 2 + 1: junk[1], nframes - 1: arp}
    frames, kinds = [], []
    for f in range(nframes):
        if f in extra:
            frames.append(extra[f])
            kinds.append(1 if extra[f] is arp else 2)
        frames.append(w_data[int(w_off[f]):int(w_off[f]) + int(w_len[f])])
        kinds.append(0)
    kinds = np.array(kinds)
    m_len = np.array([f.size for f in frames], dtype=np.uint32)
    mixed = batch.PacketBatch.from_host(np.concatenate(frames), (np.cumsum(m_len) - m_len).astype(np.uint64), m_len,
                                        device=dev)
    rx = batch.eth_rx(mixed, (IPV4, ARP))
    assert rx.bounds().tolist() == [0, nframes, nframes + 3, nframes + 5]
    assert rx.indices(0).cpu().numpy().tolist() == np.flatnonzero(kinds == 0).tolist()
    assert rx.indices(1).cpu().numpy().tolist() == np.flatnonzero(kinds == 1).tolist()
    assert rx.indices(2).cpu().numpy().tolist() == np.flatnonzero(kinds == 2).tolist()
    cls = rx.cls.cpu().numpy()
    assert np.all(cls[kinds == 0] == 0) and np.all(cls[kinds == 1] == 1)
    assert sorted(cls[kinds == 2].tolist()) == [native.ETH_SHORT, native.ETH_UNKNOWN]
    ip = rx.bucket(0)
    assert ip.n == nframes
    status = torch.zeros(ip.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(ip, status=status)
    torch.cuda.synchronize()
    assert bool(torch.all((status & native.ST_OK) != 0)) and not bool(torch.any((status & REJECT) != 0))
    assert np.all(rx.src_mac(0).cpu().numpy().view(np.uint64) == HW)
    assert rx.src_mac(1).cpu().numpy().view(np.uint64).tolist() == [0x001122334455] * 3
    assert rx.src_mac(2).cpu().numpy().tolist() == [0, 0]
    m_data, i_off, i_len = mixed.data.cpu().numpy(), ip.off.cpu().numpy(), ip.length.cpu().numpy()
    assert np.array_equal(i_len, s_len)
    for f in range(nframes):
        a = m_data[int(i_off[f]):int(i_off[f]) + int(i_len[f])]
        assert np.array_equal(a, s_data[int(s_off[f]):int(s_off[f]) + int(s_len[f])]), f
    # every sender is the host itself: nothing to learn; seen from a peer, the host is one new pair per frame
    assert batch.arp_learn_records(ip, status, rx.src_mac(0), HOST, MASK16, table).numel() == 0
    recs = batch.arp_learn_records(ip, status, rx.src_mac(0), HOST + 1, MASK16, table)
    recs = recs.cpu().numpy().view(batch.ARP_REC_DTYPE)
    assert recs.size == nframes and np.all(recs["ip"] == HOST) and np.all(recs["mac"] == HW)
    assert np.array_equal(recs["index"], np.arange(nframes))
    table.close()


def test_wrapper_unresolved_and_resubmit(dev):
    """eth_send on hand-built lists: the unresolved datagrams come back as
    {datagram, next hop}; a table that has learnt them emits the rest."""
    rng = np.random.default_rng(31)
    n = 500
    lists, host, frame_bytes, keep = hand_built(dev, rng, n)
    dst = destinations(rng, n)
    table = batch.ArpTable(send_table(False))
    e = batch.eth_send(lists, _u32_dev(dev, dst), table, HW, HOST, MASK16, GW)
    want = ref_eth_send(send_opts(), send_table(False), dst, None, host["desc"], host["first"], host["off"],
                        host["length"], 0xFFFFFFFF, e.eth.data_ptr())
    assert e.unresolved().tobytes() == want["unresolved"].tobytes() and want["unresolved"].size
    assert e.totals() == tuple(int(x) for x in want["total"][:4])
    assert np.array_equal(e.pack().data.cpu().numpy()[:int(want["total"][1])], wire_bytes(want, frame_bytes))
    learnt = send_table(False)
    learnt.update({int(h): 0x02000000AAAA for h in e.unresolved()["next_hop"]})
    table2 = batch.ArpTable(learnt)
    e2 = batch.eth_send(lists, _u32_dev(dev, dst), table2, HW, HOST, MASK16, GW)
    assert e2.unresolved().size == 0 and e2.emitted()[0] == n
    with pytest.raises(ValueError, match="table"):
        batch.eth_send(lists, _u32_dev(dev, dst), batch.ArpTable(learnt, device=None), HW, HOST, MASK16, GW)
    table.close()
    table2.close()
    del keep


def test_cpp_classes_on_gpu(tmp_path):
    """Native host program (tests/cpp/eth_gpu.cc): arp_table, eth_rx and eth_tx
    each against the C call it forwards to, on the same inputs into separately
    poisoned outputs; every array byte-equal."""
    exe = str(tmp_path / "eth_gpu")
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "eth_gpu.cc"), "-L", lib_dir, "-lsccsum", "-Wl,-rpath," + lib_dir,
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
    print(r.stdout)
