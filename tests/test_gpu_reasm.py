"""Rx reassembly on the device (sccsum_ipv4_frag_records, sccsum_ipv4_reasm):
every output compared byte for byte with tests/reasm_model.py, the Python
restatement of the reference's reassembly that tests/test_reasm_ref.py and
tests/golden/reasm.json pin to the reference's own packet_merger.  Nothing has
a tolerance; every output array has poisoned guard bytes that must stay
untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
import reasm_model
from fast_models import key_mix as np_key_mix
from seastar_amd import batch, native, synth
from test_gpu_send import SRC, _datagrams, _dev_inputs
from test_reasm_host import key_mix

pytestmark = pytest.mark.gpu

HOST = 0xC0A80A63
KEY = oracle.RSS_KEY_40
GUARD = 64
POISON = 0xA5
REC = batch.REC_DTYPE
COMPLETE, PENDING, HOSTB = native.REASM_COMPLETE, native.REASM_PENDING, native.REASM_HOST
# bytes per entry of every output; dgram_first has one closing entry more
ELEM = dict(desc=16, dgram_first=4, dgram_off=8, dgram_len=4, dgram_seed=4, dgram_head=4, dgram_last=4, dgram_hash=4,
            pending=32, host=32, rec_state=1)
FIELD = dict(desc="d_desc", dgram_first="d_dgram_first", dgram_off="d_dgram_off", dgram_len="d_dgram_len",
             dgram_seed="d_dgram_seed", dgram_head="d_dgram_head", dgram_last="d_dgram_last",
             dgram_hash="d_dgram_hash", pending="d_pending", host="d_host", rec_state="d_rec_state", total="d_total")


@functools.lru_cache(maxsize=None)
def _tiles() -> tuple:
    lib = native.load()
    return int(lib.sccsum_reasm_sort_tile_records()), int(lib.sccsum_reasm_scan_tile_records())


def _mix(key) -> int:
    return key_mix(*key)


class Mem:
    """Host copies of the device buffers records point into: bytes by address."""

    def __init__(self):
        self.blocks = []

    def add(self, t: torch.Tensor, host: np.ndarray | None = None):
        self.blocks.append((t.data_ptr(), t.cpu().numpy().copy() if host is None else host, t))
        return self

    def read(self, addr: int, n: int) -> np.ndarray:
        for base, buf, _ in self.blocks:
            if base <= addr and addr + n <= base + buf.size:
                return buf[addr - base: addr - base + n]
        raise AssertionError(f"address {addr:#x} + {n} is in no buffer")


class Raw:
    """sccsum_ipv4_reasm through the C-ABI into outputs this test owns: every
    array has room for m entries plus GUARD bytes, all poisoned before a run."""

    def __init__(self, dev, m: int):
        self.dev, self.m = dev, int(m)
        self.size = {k: e * (self.m + (1 if k == "dgram_first" else 0)) for k, e in ELEM.items()}
        self.size["total"] = 32
        self.buf = {k: torch.empty(v + GUARD, dtype=torch.uint8, device=dev) for k, v in self.size.items()}
        self.ws = torch.empty(int(native.load().sccsum_ipv4_reasm_workspace(self.m)) or 16, dtype=torch.uint8,
                              device=dev)

    def poison(self) -> None:
        for t in self.buf.values():
            t.fill_(POISON)
        self.ws.fill_(0x5A)  # whatever the workspace held must not matter

    def read(self) -> dict:
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in self.buf.items()}

    def run(self, rec_t, max_out_bytes=0xFFFFFFFF, key=KEY) -> dict:
        self.poison()
        self.launch(rec_t, max_out_bytes, key)
        return self.read()

    def launch(self, rec_t, max_out_bytes=0xFFFFFFFF, key=KEY) -> None:
        """The call alone, on torch's current stream."""
        f = {FIELD[k]: v.data_ptr() for k, v in self.buf.items()}
        if key is None:
            f["d_dgram_hash"] = None
        out = native.ReasmOut(**f)
        kb = None if key is None else (ctypes.c_uint8 * len(key)).from_buffer_copy(key)
        assert rec_t is None or rec_t.numel() == 32 * self.m
        code = native.load().sccsum_ipv4_reasm(
            rec_t.data_ptr() if self.m else None, self.m, int(max_out_bytes),
            None if kb is None else ctypes.addressof(kb), 0 if key is None else len(key), ctypes.addressof(out),
            self.ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        native.check(code, "sccsum_ipv4_reasm")


def _expect(recs: np.ndarray, cap: int = 0xFFFFFFFF, collisions: bool = False):
    """(state uint8 [m], datagrams emitted in order) from the model and the
    interface's definition of the buckets; asserts the two agree on plain keys
    and that no two keys of the input share a mix by chance."""
    keys = [(int(r["src"]), int(r["dst"]), int(r["id"]), int(r["proto"])) for r in recs]
    if not collisions:
        assert len({_mix(k) for k in set(keys)}) == len(set(keys)), "seeded keys collide: choose another seed"
    st = reasm_model.buckets(recs, mix=_mix)
    of_key = dict(zip(keys, st.tolist()))
    delivered, _ = reasm_model.run(recs)
    dg = [d for d in delivered if of_key[d.key] == COMPLETE]
    assert sorted(d.key for d in dg) == sorted(k for k, s in of_key.items() if s == COMPLETE)
    assert not any(of_key[d.key] == PENDING for d in delivered)
    emitted, total = [], 0
    for d in dg:
        if total + d.length > cap:
            break
        emitted.append(d)
        total += d.length
    late = {d.key for d in dg[len(emitted):]}
    for i, k in enumerate(keys):
        if k in late:
            st[i] = PENDING
    return st, emitted


def _check(h: dict, recs: np.ndarray, st: np.ndarray, emitted: list, mem: Mem | None = None, key=KEY, msg=""):
    """Every output of a run (host copies, guards included) against the expectation."""
    m = recs.size
    D = len(emitted)
    K = sum(len(d.pieces) for d in emitted)
    pend, host = recs[st == PENDING], recs[st == HOSTB]
    total = h["total"][:32].view(np.uint64)
    assert total.tolist() == [D, K, pend.size, host.size], msg
    assert np.array_equal(h["rec_state"][:m], st), msg
    assert pend.tobytes() == h["pending"][: 32 * pend.size].tobytes(), msg
    assert host.tobytes() == h["host"][: 32 * host.size].tobytes(), msg
    first = h["dgram_first"][: 4 * (D + 1)].view(np.uint32)
    off = h["dgram_off"][: 8 * D].view(np.uint64)
    want_first = np.concatenate([[0], np.cumsum([len(d.pieces) for d in emitted])]).astype(np.uint32)
    want_off = np.concatenate([[0], np.cumsum([d.length for d in emitted])]).astype(np.uint64)[:D]
    assert np.array_equal(first, want_first), msg
    assert np.array_equal(off, want_off), msg
    assert np.array_equal(h["dgram_len"][: 4 * D].view(np.uint32), np.array([d.length for d in emitted], np.uint32)), msg
    assert np.array_equal(h["dgram_head"][: 4 * D].view(np.uint32), np.array([d.head for d in emitted], np.uint32)), msg
    assert np.array_equal(h["dgram_last"][: 4 * D].view(np.uint32), np.array([d.last for d in emitted], np.uint32)), msg
    # delivery order is completion order
    assert all(a.last < b.last for a, b in zip(emitted, emitted[1:])), msg
    seeds = [oracle.pseudo_seed(d.key[0], d.key[1], d.key[3], d.length) if d.key[3] in (6, 17) else 0 for d in emitted]
    assert np.array_equal(h["dgram_seed"][: 4 * D].view(np.uint32), np.array(seeds, np.uint32)), msg
    desc = h["desc"][: 16 * K].view(batch.DESC_DTYPE)
    want = np.zeros(K, batch.DESC_DTYPE)
    k = 0
    for d, o in zip(emitted, want_off):
        pos = 0
        for r, frm, ln in d.pieces:
            want[k] = (int(recs[r]["frame"]) + int(recs[r]["hdr_len"]) + frm, (int(o) + pos) & 0xFFFFFFFF, ln)
            pos += ln
            k += 1
    assert desc.tobytes() == want.tobytes(), msg
    # nothing past what was emitted, nothing past the end of the others
    written = dict(desc=16 * K, dgram_first=4 * (D + 1), dgram_off=8 * D, dgram_len=4 * D, dgram_seed=4 * D,
                   dgram_head=4 * D, dgram_last=4 * D, dgram_hash=4 * D if key is not None else 0,
                   pending=32 * pend.size, host=32 * host.size, rec_state=m, total=32)
    for name, w in written.items():
        assert np.all(h[name][w:] == POISON), (name, msg)
    if mem is not None and key is not None and D:
        # the hash of ip.cc:186-197 = the oracle's REASSEMBLED hash of the frame the host would assemble
        frames = []
        for d in emitted:
            hr = recs[d.head]   # the header frag::merge keeps, with the datagram's length (ip.cc:439-455)
            hdr = np.zeros((1, int(hr["hdr_len"])), np.uint8)
            synth.write_ipv4_header(hdr, [hdr.size + d.length], d.key[3], [d.key[0]], [d.key[1]])
            hdr[0, 0] = 0x40 | (hdr.size // 4)
            frames.append(np.concatenate([hdr.reshape(-1), _bytes_of(d, recs, mem)]))
        lens = np.array([f.size for f in frames], np.uint32)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)[:D]
        want_hash, _ = oracle.batch_ipv4_rss(np.concatenate(frames), offs, lens, KEY, native.RSS_REASSEMBLED)
        for k, (d, f) in enumerate(zip(emitted, frames)):
            if f.size > 65535:
                # records built by hand past what a frame's 16-bit total length can say: the forward_hash
                # itself (src, dst, the UDP ports: ip.cc:192-195, udp.cc:153-161)
                assert d.key[3] == 17
                hl = int(recs[d.head]["hdr_len"])
                data = d.key[0].to_bytes(4, "big") + d.key[1].to_bytes(4, "big") + f[hl: hl + 4].tobytes()
                want_hash[k] = oracle.toeplitz(KEY, data)
        assert np.array_equal(h["dgram_hash"][: 4 * D].view(np.uint32), want_hash), msg


def _bytes_of(d, recs, mem: Mem) -> np.ndarray:
    parts = [mem.read(int(recs[r]["frame"]) + int(recs[r]["hdr_len"]) + frm, ln) for r, frm, ln in d.pieces]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def _wrapper_checks(rec_t, recs, emitted, mem: Mem, corrupt: bool = True):
    """batch.reassemble: .lists() through spans_desc with the returned seeds
    verifies every TCP / UDP datagram, .pack() equals the model's bytes, and one
    corrupted payload byte does not verify."""
    r = batch.reassemble(rec_t, key=KEY)
    D = len(emitted)
    assert r.totals()[0] == D
    desc, first, off, length, seeds, max_len = r.lists()
    assert max_len == max((d.length for d in emitted), default=0)
    if not D:
        return
    packed = r.pack()
    torch.cuda.synchronize()
    want = np.concatenate([_bytes_of(d, recs, mem) for d in emitted])
    assert packed.bytes_len == want.size
    assert np.array_equal(packed.data.cpu().numpy()[: want.size], want)
    l4 = [i for i, d in enumerate(emitted) if (d.key[3] == 17 and d.length >= 8) or (d.key[3] == 6 and d.length >= 20)]
    assert l4
    out = batch.spans_desc(desc, first, off, length, max_len, seeds=seeds)
    torch.cuda.synchronize()
    got = batch.as_u16(out)
    assert np.all(got[l4] == 0), "a reassembled datagram's L4 checksum does not verify"
    assert np.array_equal(r.hashes.cpu().numpy(), r.dgram_hash[:D].cpu().numpy())
    if corrupt:
        # the steering call takes the datagram hashes as they stand (ip.cc:197)
        reta = batch.build_reta({c: 1.0 for c in range(4)})
        steer = batch.Steer(4, reta)
        cpu, _, _ = steer.run(r.hashes)
        torch.cuda.synchronize()
        steer.close()
        assert cpu.cpu().numpy().tolist() == [batch.steer_dest(int(x), 4, reta)
                                              for x in r.hashes.cpu().numpy().view(np.uint32)]
        d = emitted[l4[len(l4) // 2]]
        rr, frm, ln = d.pieces[len(d.pieces) // 2]
        addr = int(recs[rr]["frame"]) + int(recs[rr]["hdr_len"]) + frm + ln // 2
        base, _, t = next(b for b in mem.blocks if b[0] <= addr < b[0] + b[1].size)
        t[addr - base] ^= 0x40
        out = batch.spans_desc(desc, first, off, length, max_len, seeds=seeds)
        torch.cuda.synchronize()
        got = batch.as_u16(out)
        t[addr - base] ^= 0x40
        bad = l4[len(l4) // 2]
        assert got[bad] != 0 and np.all(got[[i for i in l4 if i != bad]] == 0)


# ---------------------------------------------------------------- records

def _frame(src, dst, ident, proto, mf, off8, payload, ihl=5, good=True, pad=0):
    """One IPv4 frame: a 4 * ihl byte header (options zero), the header checksum
    over its first 20 bytes (what ip.cc:121-127 verifies), payload, `pad`
    trailing bytes past the IP total length."""
    payload = np.asarray(payload, np.uint8)
    f = np.zeros((1, 4 * ihl + payload.size + pad), np.uint8)
    synth.write_ipv4_header(f, [4 * ihl + payload.size], proto, [src], [dst])
    f[0, 0] = 0x40 | ihl
    f[0, 4], f[0, 5] = ident >> 8, ident & 0xFF
    w = (0x2000 if mf else 0) | off8
    f[0, 6], f[0, 7] = w >> 8, w & 0xFF
    f = f.reshape(-1)
    f[4 * ihl: 4 * ihl + payload.size] = payload
    f[10:12] = np.frombuffer(np.uint16(oracle.ip_checksum(f[:20])).tobytes(), np.uint8)
    if not good:
        f[10] ^= 0x55
    return f


def _with_checksum(f):
    f[10:12] = 0
    f[10:12] = np.frombuffer(np.uint16(oracle.ip_checksum(f[:20])).tobytes(), np.uint8)
    return f


def _rx_frames(rng, n):
    """n frames of every kind the rx path meets, in random order."""
    frames = []
    while len(frames) < n:
        kind = int(rng.integers(0, 10))
        dst = HOST
        ident = int(rng.integers(0, 65536))
        src = int(rng.integers(1, 2**32))
        proto = int(rng.choice([6, 17, 1]))
        pay = rng.integers(0, 256, int(rng.integers(8, 200)), dtype=np.uint8)
        if kind <= 2:    # a datagram cut as ipv4::send cuts it, its fragments
            data = rng.integers(0, 256, int(rng.integers(60, 400)), dtype=np.uint8)
            frames += [_with_checksum(f) for f in synth.ipv4_fragment(data, proto, src, dst, mtu=68, ident=ident)]
        elif kind == 3:  # a whole datagram: not a fragment
            frames.append(_frame(src, dst, ident, proto, 0, 0, pay))
        elif kind == 4:  # a fragment whose header checksum is wrong
            frames.append(_frame(src, dst, ident, proto, 1, 3, pay, good=False))
        elif kind == 5:  # short: fewer bytes than a header / than the IP total length
            f = _frame(src, dst, ident, proto, 1, 0, pay)
            frames.append(f[: int(rng.choice([12, 19, f.size - 1]))])
        elif kind == 6:  # options, and bytes past the IP total length (trimmed, ip.cc:134-136)
            frames.append(_frame(src, dst, ident, proto, int(rng.integers(0, 2)), int(rng.integers(1, 100)), pay,
                                 ihl=int(rng.integers(6, 16)), pad=int(rng.integers(0, 7))))
        elif kind == 7:  # another host's
            frames.append(_frame(src, HOST ^ 0x100, ident, proto, 1, 2, pay))
        elif kind == 8:  # offset + length past 65535 (ip.cc:141-144)
            frames.append(_frame(src, dst, ident, proto, 0, 0x1FFF, pay[:8] if pay.size < 40 else pay))
        else:            # a last fragment on its own
            frames.append(_frame(src, dst, ident, proto, 0, int(rng.integers(1, 0x1000)), pay))
    frames = frames[:n]
    return [frames[int(i)] for i in rng.permutation(n)]


def _expected_records(frames, offs, base, tag):
    """The frames ip.cc:121-166 lets reach line 164 and sends into the branch
    at 166, as records, decoded here from the bytes."""
    out = []
    for f, o in zip(frames, offs):
        if f.size < 20 or oracle.ip_checksum(f[:20]) != 0:
            continue
        ihl, ip_len = int(f[0]) & 0xF, (int(f[2]) << 8) | int(f[3])
        w = (int(f[6]) << 8) | int(f[7])
        mf, offset = (w >> 13) & 1, (w & 0x1FFF) << 3
        dst = int.from_bytes(f[16:20].tobytes(), "big")
        if f.size < ip_len or 4 * ihl > ip_len or offset + ip_len > 65535 or dst != HOST or not (mf or offset):
            continue
        out.append((base + int(o), int.from_bytes(f[12:16].tobytes(), "big"), dst, (int(f[4]) << 8) | int(f[5]),
                    int(f[9]), mf, offset, 4 * ihl, ip_len - 4 * ihl, 0, tag))
    return np.array(out, dtype=REC) if out else np.zeros(0, REC)


def _pack_frames(rng, frames):
    lens = np.array([f.size for f in frames], np.uint32)
    gaps = rng.integers(0, 4, len(frames))
    offs = (np.cumsum(gaps) + np.concatenate([[0], np.cumsum(lens)[:-1]]) + 1).astype(np.uint64) if frames else \
        np.zeros(0, np.uint64)
    buf = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 5 if frames else 16, dtype=np.uint8)
    for f, o in zip(frames, offs):
        buf[int(o): int(o) + f.size] = f
    return buf, offs, lens


def _records_raw(dev, b, status, n, host_address, tag, need=batch.FRAG_NEED, reject=batch.FRAG_REJECT):
    lib = native.load()
    rec = torch.full((32 * n + GUARD,), POISON, dtype=torch.uint8, device=dev)
    count = torch.full((4 + GUARD,), POISON, dtype=torch.uint8, device=dev)
    ws = torch.full((int(lib.sccsum_ipv4_reasm_workspace(n)),), 0x5A, dtype=torch.uint8, device=dev)
    code = lib.sccsum_ipv4_frag_records(
        b.data.data_ptr(), b.bytes_len, b.off.data_ptr() if n else None, b.length.data_ptr() if n else None,
        status.data_ptr() if n else None, need, reject, n, host_address, tag, rec.data_ptr(), count.data_ptr(),
        ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    native.check(code, "sccsum_ipv4_frag_records")
    torch.cuda.synchronize()
    return rec.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("where", ["zero", "tile-1", "tile", "tile+1", "3 tiles+7"])
def test_records_are_the_fragments_the_rx_path_accepts(dev, where):
    tile = _tiles()[1]
    n = {"zero": 0, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "3 tiles+7": 3 * tile + 7}[where]
    rng = np.random.Generator(np.random.PCG64(1000 + n))
    frames = _rx_frames(rng, n)
    buf, offs, lens = _pack_frames(rng, frames)
    b = batch.PacketBatch.from_host(buf, offs, lens, device=dev)
    status = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    if n:
        batch.ipv4_frames(b, status=status)
    want = _expected_records(frames, offs, b.data.data_ptr(), 0xBEEF0000 + n)
    rec, count = _records_raw(dev, b, status, n, HOST, 0xBEEF0000 + n)
    assert int(count[:4].view(np.uint32)[0]) == want.size
    assert np.all(count[4:] == POISON)
    assert n == 0 or 0 < want.size < n                      # the batch has both kinds
    assert rec[: 32 * want.size].tobytes() == want.tobytes()
    assert np.all(rec[32 * want.size:] == POISON)
    if n:
        # host_address 0 accepts every destination; the wrapper returns the same records
        any_dst = batch.frag_records(b, status, host_address=0, tag=1).cpu().numpy().view(REC)
        assert any_dst.size > want.size and set(any_dst["dst"].tolist()) == {HOST, HOST ^ 0x100}
        mine = batch.frag_records(b, status, host_address=HOST, tag=0xBEEF0000 + n).cpu().numpy()
        assert mine.tobytes() == want.tobytes()
        # need without SCCSUM_ST_IPFRAG lets the whole datagrams through too
        more, cnt = _records_raw(dev, b, status, n, HOST, 0, need=native.ST_OK)
        whole = more[: 32 * int(cnt[:4].view(np.uint32)[0])].view(REC)
        assert whole.size > want.size and np.any((whole["mf"] == 0) & (whole["offset"] == 0))


# ---------------------------------------------------------------- plain datagrams, cut by the send path

def _sent_fragments(dev, rng, lens, protos, mtu):
    """Datagrams with valid L4 checksums cut by sccsum_ipv4_send, the packed
    wire frames shuffled: (frames batch, status, its host bytes)."""
    buf, off, lens, dst, proto, ids = _datagrams(rng, lens, protos, valid_l4=True)
    ids = rng.permutation(65536)[: lens.size].astype(np.uint16)     # one key per datagram
    l4, d_dst, d_proto, d_ids = _dev_inputs(dev, buf, off, lens, dst, proto, ids)
    frames = batch.ipv4_send(l4, d_dst, d_proto, mtu, SRC, ids=d_ids).pack()
    torch.cuda.synchronize()
    perm = torch.from_numpy(rng.permutation(frames.n)).to(dev)
    fb = batch.PacketBatch(data=frames.data, off=frames.off[perm].contiguous(),
                           length=frames.length[perm].contiguous(), bytes_len=frames.bytes_len,
                           max_len=frames.max_len)
    status = torch.zeros(fb.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(fb, status=status)
    return fb, status


@pytest.mark.parametrize("mtu", [68, 576, 1500, 1490])
def test_datagrams_cut_by_ipv4_send_come_back(dev, mtu):
    """ipv4_send -> frames -> frag_records -> reassemble.  mtu - 20 is a
    multiple of 8 for 68 and 1500: every cut datagram is delivered and its L4
    checksum verifies.  For 576 and 1490 the reference's truncated offsets make
    the pieces overlap: host bucket, as the model says."""
    rng = np.random.Generator(np.random.PCG64(mtu))
    room = mtu - 20
    lens = [room + 1, 2 * room, 2 * room + 1, 63 * room, 64 * room - 3, 65 * room, 20, 8, room, 5 * room + 9,
            17 * room + 1] + [int(x) for x in rng.integers(room + 1, min(65515, 40 * room), 12)]
    lens = [min(x, 65515) for x in lens]
    protos = [17, 6, 17, 6, 17, 17, 6, 17, 1, 47, 6] + [int(x) for x in rng.choice([6, 17], 12)]
    fb, status = _sent_fragments(dev, rng, lens, protos, mtu)
    rec_t = batch.frag_records(fb, status)
    recs = rec_t.cpu().numpy().view(REC)
    assert recs.size == sum(-(-x // room) for x in lens if x > room)   # every fragment, no whole datagram
    st, emitted = _expect(recs)
    if room % 8 == 0:
        assert len(emitted) == sum(1 for x in lens if x > room) and np.all(st == COMPLETE)
    else:
        assert np.any(st == HOSTB)
    mem = Mem().add(fb.data)
    h = Raw(dev, recs.size).run(rec_t)
    _check(h, recs, st, emitted, mem, msg=f"mtu {mtu}")
    _wrapper_checks(rec_t, recs, emitted, mem, corrupt=room % 8 == 0)


# ---------------------------------------------------------------- records built directly

def _udp_datagram(rng, src, dst, length):
    d = rng.integers(0, 256, length, dtype=np.uint8)
    if length >= 8:
        d[4], d[5] = length >> 8, length & 0xFF
        d[6:8] = 0
        c = oracle.batch_spans(d, np.zeros(1, np.uint64), np.array([length], np.uint32),
                               np.array([oracle.pseudo_seed(src, dst, 17, length)], np.uint32))
        d[6:8] = np.frombuffer(np.uint16(c[0]).tobytes(), np.uint8)
    return d


def _interleave(rng, streams):
    """One arrival order of several record streams, each stream's own order kept."""
    who = np.concatenate([np.full(len(s), k) for k, s in enumerate(streams)])
    rng.shuffle(who)
    at = [0] * len(streams)
    out = []
    for k in who:
        out.append(streams[k][at[k]])
        at[k] += 1
    return out


def _direct(dev, rng, specs, m=None):
    """Records of UDP datagrams whose pieces lie in one device buffer.  specs:
    (pieces, piece bytes, drop) — `drop` leaves one piece out (a pending key).
    Padded with one-record datagrams up to m records.  A datagram's pieces
    arrive in shuffled blocks of 96, the datagrams interleaved."""
    specs = list(specs)
    have = sum(p - (1 if drop else 0) for p, _, drop in specs)
    if m is not None:
        assert m >= have
        specs += [(1, int(rng.integers(8, 64)), False) for _ in range(m - have)]
    ids = rng.permutation(65536)[: len(specs)]
    data, at, streams = [], 33, []   # past 20: a record's frame is its piece's address - hdr_len
    for k, (pieces, piece, drop) in enumerate(specs):
        src, dst = int(rng.integers(1, 2**32)), int(rng.integers(1, 2**32))
        length = pieces * piece - (int(rng.integers(0, min(piece, 8))) if pieces > 1 else 0)
        d = _udp_datagram(rng, src, dst, length)
        recs = []
        for j in range(pieces):
            o = j * piece
            ln = min(piece, length - o)
            recs.append((at + o - 20, src, dst, int(ids[k]), 17, 1 if j + 1 < pieces else 0, o, 20, ln, 0, k))
        if drop:
            del recs[int(rng.integers(0, len(recs)))]
        blocks = [recs[i: i + 96] for i in range(0, len(recs), 96)]
        streams.append([r for i in rng.permutation(len(blocks)) for r in
                        (blocks[i] if len(blocks) > 1 else [blocks[0][int(q)] for q in rng.permutation(len(blocks[0]))])])
        data.append((at, d))
        at += length + int(rng.integers(0, 4))
    buf = rng.integers(0, 256, at + 9, dtype=np.uint8)
    for o, d in data:
        buf[o: o + d.size] = d
    t = torch.from_numpy(buf).to(dev)
    recs = np.array(_interleave(rng, streams), dtype=REC)
    recs["frame"] += np.uint64(t.data_ptr())
    return recs, torch.from_numpy(recs.view(np.uint8).copy()).to(dev), Mem().add(t, buf)


def _small_specs():
    # datagrams of 1, 2, 63, 64 and 65 fragments, and keys with a piece missing
    return [(1, 40, False), (2, 24, False), (63, 8, False), (64, 16, False), (65, 8, False), (2, 8, True), (30, 8, True),
            (64, 8, True), (3, 1480, False)]


@pytest.mark.parametrize("where", ["small", "scan-1", "scan", "scan+1", "sort-1", "sort", "sort+1", "2 sort+1"])
def test_plain_datagrams_at_the_tile_boundaries(dev, where):
    sort, scan = _tiles()
    m = {"small": None, "scan-1": scan - 1, "scan": scan, "scan+1": scan + 1, "sort-1": sort - 1, "sort": sort,
         "sort+1": sort + 1, "2 sort+1": 2 * sort + 1}[where]
    rng = np.random.Generator(np.random.PCG64(sum(map(ord, where))))
    recs, rec_t, mem = _direct(dev, rng, _small_specs(), m)
    assert m is None or recs.size == m
    st, emitted = _expect(recs)
    assert np.any(st == PENDING) and np.any(st == COMPLETE) and not np.any(st == HOSTB)
    h = Raw(dev, recs.size).run(rec_t)
    _check(h, recs, st, emitted, mem, msg=where)
    _wrapper_checks(rec_t, recs, emitted, mem, corrupt=where in ("small", "sort+1"))


def test_a_datagram_of_8191_fragments(dev):
    """65 528 bytes in 8-byte pieces, among other keys; the run spans several
    tiles of every kernel."""
    rng = np.random.Generator(np.random.PCG64(8191))
    sort, _ = _tiles()
    m = 8191 + 195 + 3 * 4 + 1000
    m += (-m) % sort + 1                      # a tile boundary + 1
    recs, rec_t, mem = _direct(dev, rng, [(8191, 8, False), (8191 // 64, 8, True)] + _small_specs()[:5], m)
    st, emitted = _expect(recs)
    assert max(len(d.pieces) for d in emitted) == 8191
    h = Raw(dev, recs.size).run(rec_t)
    _check(h, recs, st, emitted, mem)
    _wrapper_checks(rec_t, recs, emitted, mem, corrupt=False)


def test_two_runs_give_identical_bytes(dev):
    rng = np.random.Generator(np.random.PCG64(22))
    sort, _ = _tiles()
    recs, rec_t, _ = _direct(dev, rng, _small_specs() * 3, 3 * sort + 5)
    raw = Raw(dev, recs.size)
    a = raw.run(rec_t)
    b = raw.run(rec_t)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    other = Raw(dev, recs.size).run(rec_t)      # other addresses, another workspace
    for name in a:
        assert a[name].tobytes() == other[name].tobytes(), name


def test_capture_and_replay(dev):
    """One call under torch.cuda.graph (a single chain of kernels, no allocation,
    no synchronisation), replayed into poisoned outputs."""
    rng = np.random.Generator(np.random.PCG64(23))
    recs, rec_t, mem = _direct(dev, rng, _small_specs(), _tiles()[0] + 1)
    st, emitted = _expect(recs)
    raw = Raw(dev, recs.size)
    want = raw.run(rec_t)
    _check(want, recs, st, emitted, mem)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        raw.launch(rec_t)
    raw.poison()
    g.replay()
    got = raw.read()
    for name in want:
        assert want[name].tobytes() == got[name].tobytes(), name


def test_no_key_no_hash_array(dev):
    rng = np.random.Generator(np.random.PCG64(5))
    recs, rec_t, mem = _direct(dev, rng, _small_specs())
    st, emitted = _expect(recs)
    h = Raw(dev, recs.size).run(rec_t, key=None)
    _check(h, recs, st, emitted, mem, key=None)
    assert np.all(h["dgram_hash"] == POISON)


def test_no_records(dev):
    """m == 0 writes the totals and the closing CSR entry, with every other array NULL too."""
    h = Raw(dev, 0).run(None)
    _check(h, np.zeros(0, REC), np.zeros(0, np.uint8), [])
    total = torch.full((32 + GUARD,), POISON, dtype=torch.uint8, device=dev)
    first = torch.full((4 + GUARD,), POISON, dtype=torch.uint8, device=dev)
    out = native.ReasmOut(d_total=total.data_ptr(), d_dgram_first=first.data_ptr())
    native.check(native.load().sccsum_ipv4_reasm(None, 0, 0, None, 0, ctypes.addressof(out), None,
                                                 torch.cuda.current_stream().cuda_stream), "sccsum_ipv4_reasm")
    torch.cuda.synchronize()
    assert np.all(total.cpu().numpy()[:32] == 0) and np.all(total.cpu().numpy()[32:] == POISON)
    assert np.all(first.cpu().numpy()[:4] == 0) and np.all(first.cpu().numpy()[4:] == POISON)
    r = batch.reassemble(torch.zeros(0, dtype=torch.uint8, device=dev))
    assert r.totals() == (0, 0, 0, 0) and r.pending.numel() == 0 and r.pack().n == 0


# ---------------------------------------------------------------- carry, capacity

def test_a_datagram_split_over_three_calls(dev):
    """The pending records of a call go in front of the next call's: a
    datagram whose pieces arrive in three batches is delivered in the third,
    exactly as if every record had come at once, tags kept."""
    rng = np.random.Generator(np.random.PCG64(33))
    src = 0x0A000009
    data = _udp_datagram(rng, src, HOST, 3 * 48 + 11)
    other = rng.integers(0, 256, 100, dtype=np.uint8)
    fa = [_with_checksum(f) for f in synth.ipv4_fragment(data, 17, src, HOST, mtu=68, ident=77)]
    fo = [_with_checksum(f) for f in synth.ipv4_fragment(other, 17, src, HOST, mtu=68, ident=78)]
    assert len(fa) == 4 and len(fo) == 3
    calls = [[fa[1], fo[0]], [fa[3], fo[2], fa[0]], [fa[2]]]
    mem, carry, every = Mem(), torch.zeros(0, dtype=torch.uint8, device=dev), []
    for k, frames in enumerate(calls):
        buf, offs, lens = _pack_frames(rng, frames)
        b = batch.PacketBatch.from_host(buf, offs, lens, device=dev)
        status = torch.zeros(b.n, dtype=torch.uint8, device=dev)
        batch.ipv4_frames(b, status=status)
        new = batch.frag_records(b, status, host_address=HOST, tag=100 + k)
        assert new.numel() == 32 * len(frames)
        mem.add(b.data)
        every.append(new)
        rec_t = torch.cat([carry, new])
        recs = rec_t.cpu().numpy().view(REC)
        st, emitted = _expect(recs)
        h = Raw(dev, recs.size).run(rec_t)
        _check(h, recs, st, emitted, mem, msg=f"call {k}")
        assert len(emitted) == (1 if k == 2 else 0)
        r = batch.reassemble(rec_t, key=KEY)
        carry = r.pending.clone()
        assert carry.cpu().numpy().tobytes() == recs[st == PENDING].tobytes()
    # all at once
    rec_t = torch.cat(every)
    recs = rec_t.cpu().numpy().view(REC)
    assert recs["tag"].tolist() == [100, 100, 101, 101, 101, 102]
    st, emitted = _expect(recs)
    once = Raw(dev, recs.size).run(rec_t)
    _check(once, recs, st, emitted, mem, msg="at once")
    for name in once:                       # the third call saw the same six records in the same order
        assert once[name].tobytes() == h[name].tobytes(), name
    assert _bytes_of(emitted[0], recs, mem).tobytes() == data.tobytes()
    _wrapper_checks(rec_t, recs, emitted, mem)


def test_capacity_is_a_prefix_rule(dev):
    rng = np.random.Generator(np.random.PCG64(44))
    specs = [(3, 16, False), (5, 8, False), (2, 64, False), (4, 8, True)]
    recs, rec_t, mem = _direct(dev, rng, specs)
    st_all, all_dg = _expect(recs)
    assert len(all_dg) == 3
    raw = Raw(dev, recs.size)
    for cap, want in ((all_dg[0].length + all_dg[1].length - 1, 1), (all_dg[0].length + all_dg[1].length, 2),
                      (all_dg[0].length - 1, 0), (0, 0), (0xFFFFFFFF, 3)):
        st, emitted = _expect(recs, cap=cap)
        assert len(emitted) == want
        assert np.count_nonzero(st == PENDING) == recs.size - sum(len(d.pieces) for d in emitted)
        h = raw.run(rec_t, max_out_bytes=cap)
        _check(h, recs, st, emitted, mem, msg=f"cap {cap}")
    # what did not fit is pending: the next call delivers it
    h = raw.run(rec_t, max_out_bytes=all_dg[0].length)
    pend = h["pending"][: 32 * int(h["total"][:32].view(np.uint64)[2])]
    rec2 = torch.from_numpy(pend.copy()).to(dev)
    recs2 = pend.view(REC)
    st2, emitted2 = _expect(recs2)
    assert len(emitted2) == 2
    _check(Raw(dev, recs2.size).run(rec2), recs2, st2, emitted2, mem, msg="the rest")


# ---------------------------------------------------------------- the host bucket

def _seeded_keys(dev, rng, seqs, keys=None):
    """One key per fragment sequence (reasm_model.seeded_sequences), every
    record's payload its own slice of a random buffer, the keys interleaved
    with each key's arrival order kept."""
    total = sum(ln for _, s in seqs for _, ln, _ in s) + 64
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    t = torch.from_numpy(buf).to(dev)
    at, streams = 20, []
    ids = rng.permutation(65536)[: len(seqs)]
    for k, (_, seq) in enumerate(seqs):
        src, dst, ident, proto = keys[k] if keys else (int(rng.integers(1, 2**32)), HOST, int(ids[k]), 17)
        s = []
        for o, ln, mf in seq:
            s.append((t.data_ptr() + at - 20, src, dst, ident, proto, mf, o, 20, ln, 0, k))
            at += ln
        streams.append(s)
    recs = np.array(_interleave(rng, streams), dtype=REC)
    return recs, torch.from_numpy(recs.view(np.uint8).copy()).to(dev), Mem().add(t, buf)


def test_host_bucket_holds_exactly_the_non_plain_keys(dev):
    rng = np.random.Generator(np.random.PCG64(55))
    seqs = reasm_model.seeded_sequences(0xB0C4E7, 600)
    recs, rec_t, mem = _seeded_keys(dev, rng, seqs)
    st, emitted = _expect(recs)
    # by construction: every plain sequence is complete or pending, every other kind is host
    for k, (kind, _) in enumerate(seqs):
        mine = st[recs["tag"] == k]
        assert np.all(mine == mine[0])
        assert (mine[0] == HOSTB) == (kind not in ("plain", "plain_hole")), (kind, seqs[k])
    assert {int(x) for x in st} == {COMPLETE, PENDING, HOSTB}
    h = Raw(dev, recs.size).run(rec_t)
    _check(h, recs, st, emitted, mem)
    # the host replays its bucket through the reference's merger: the same deliveries, the same
    # held state, as the whole stream gives for those keys
    host = h["host"][: 32 * int(np.count_nonzero(st == HOSTB))].view(REC)
    index = np.flatnonzero(st == HOSTB)
    got, got_held = reasm_model.run(host)
    want, want_held = reasm_model.run(recs)
    host_keys = {(int(r["src"]), int(r["dst"]), int(r["id"]), int(r["proto"])) for r in host}
    want = [d for d in want if d.key in host_keys]
    assert [(d.key, [(int(index[r]), f, n) for r, f, n in d.pieces], int(index[d.head]), int(index[d.last]))
            for d in got] == [(d.key, d.pieces, d.head, d.last) for d in want]
    assert any(d.key in host_keys for d in want)
    for k, f in got_held.items():
        assert [(o, [(int(index[r]), a, n) for r, a, n in p]) for o, p in f.data.segments()] == \
            want_held[k].data.segments()
    assert set(got_held) == {k for k in want_held if k in host_keys}


def test_two_keys_of_one_mix_go_to_the_host_whole(dev):
    """The sort groups by sccsum_reasm_key_mix: two distinct keys that share
    it (found among 2^18 random keys) are both host, whole; their neighbours
    are unaffected."""
    rng = np.random.Generator(np.random.PCG64(66))
    n = 1 << 18
    src = rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    dst = rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    ident = rng.integers(0, 65536, n).astype(np.uint32)
    proto = np.full(n, 17, np.uint32)
    mix = np_key_mix(src, dst, ident, proto)
    order = np.argsort(mix, kind="stable")
    same = np.flatnonzero(mix[order][1:] == mix[order][:-1])
    assert same.size, "no colliding pair among the random keys"
    a, b = int(order[same[0]]), int(order[same[0] + 1])
    ka, kb = [(int(src[i]), int(dst[i]), int(ident[i]), 17) for i in (a, b)]
    lib = native.load()
    assert ka != kb and lib.sccsum_reasm_key_mix(*ka) == lib.sccsum_reasm_key_mix(*kb) == _mix(ka)
    plain = [("plain", [(0, 16, 1), (16, 9, 0)]), ("plain", [(8, 8, 0), (0, 8, 1)])]
    around = reasm_model.seeded_sequences(0xC0111DE, 64)
    seqs = around[:32] + plain + around[32:]
    keys = [(int(rng.integers(1, 2**32)), HOST, 1000 + k, 17) for k in range(len(seqs))]
    keys[32], keys[33] = ka, kb
    recs, rec_t, mem = _seeded_keys(dev, rng, seqs, keys)
    st, emitted = _expect(recs, collisions=True)
    for k in (32, 33):
        assert np.all(st[recs["tag"] == k] == HOSTB)
    # grouped by the full key the same two keys would be delivered, and nobody else changes
    alone = reasm_model.buckets(recs, mix=None)
    others = ~np.isin(recs["tag"], [32, 33])
    assert np.array_equal(alone[others], st[others]) and np.all(alone[~others] == COMPLETE)
    h = Raw(dev, recs.size).run(rec_t)
    _check(h, recs, st, emitted, mem)


# ---------------------------------------------------------------- the capacity cut outside tile 0

def test_capacity_cut_in_a_later_scan_tile(dev):
    """The first datagram that does not fit is completed by the record at slot 0
    of scan tile 1, at that tile's last slot, and inside tile 2: dg_carry scans
    the cut tile again on top of the tiles before it.  Also the exact byte
    total up to a tile's last datagram (it fits: the cut is the next tile's
    first datagram) and that total minus one."""
    rng = np.random.Generator(np.random.PCG64(45))
    _, scan = _tiles()
    m = 3 * scan + 5
    recs, _, mem = _direct(dev, rng, _small_specs(), m)
    # a record that is a whole datagram at both edges of tile 1 (swapped there from tile 0 if need be)
    alone = np.flatnonzero((recs["mf"] == 0) & (recs["offset"] == 0))
    spare = [int(i) for i in alone if 8 <= i < scan - 8]
    for slot in (scan, 2 * scan - 1):
        if slot not in alone:
            other = spare.pop()
            recs[[slot, other]] = recs[[other, slot]]
    rec_t = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
    st_all, all_dg = _expect(recs)
    assert np.any(st_all == PENDING) and len(all_dg) > 2 * scan
    last = np.array([d.last for d in all_dg])
    sums = np.cumsum([d.length for d in all_dg])
    at = {name: int(np.flatnonzero(last == i)[0]) for name, i in (("slot 0 of tile 1", scan),
                                                                  ("the last slot of tile 1", 2 * scan - 1))}
    at["inside tile 2"] = int(np.flatnonzero((last > 2 * scan + 10) & (last < 3 * scan - 10))[3])
    end_of_tile = {t: int(np.flatnonzero(last < (t + 1) * scan)[-1]) for t in (0, 1)}   # a tile's last datagram
    assert end_of_tile[0] + 1 == at["slot 0 of tile 1"] and end_of_tile[1] == at["the last slot of tile 1"]
    raw = Raw(dev, recs.size)
    cases = [(name, int(sums[d]) - 1, d) for name, d in at.items()]
    cases += [(f"tile {t} fits", int(sums[d]), d + 1) for t, d in end_of_tile.items()]
    cases += [("tile 0 less one byte", int(sums[end_of_tile[0]]) - 1, end_of_tile[0])]
    for name, cap, want in cases:
        st, emitted = _expect(recs, cap=cap)
        assert len(emitted) == want, name
        cut_tile = all_dg[want].last // scan       # the tile of the first datagram that does not fit
        assert cut_tile >= 1 or name == "tile 0 less one byte", name
        assert np.count_nonzero(st == PENDING) == recs.size - sum(len(d.pieces) for d in emitted)
        h = raw.run(rec_t, max_out_bytes=cap)
        _check(h, recs, st, emitted, mem, msg=f"{name}: cap {cap}")
    assert {all_dg[want].last // scan for _, _, want in cases} == {0, 1, 2}
    assert {all_dg[want].last % scan for _, _, want in cases} >= {0, scan - 1}


# ---------------------------------------------------------------- hdr_len

def _direct_hdr(dev, rng, specs):
    """Records of complete UDP datagrams as _direct builds them, with a header
    length per piece: specs = (piece bytes, [hdr_len of piece 0, 1, ...]).
    frame = the piece's address - hdr_len."""
    ids = rng.permutation(65536)[: len(specs)]
    data, at, streams = [], 64, []
    for k, (piece, hdr_lens) in enumerate(specs):
        src, dst = int(rng.integers(1, 2**32)), int(rng.integers(1, 2**32))
        pieces = len(hdr_lens)
        length = pieces * piece - (int(rng.integers(0, min(piece, 8))) if pieces > 1 else 0)
        d = _udp_datagram(rng, src, dst, length)
        recs = [(at + j * piece - hl, src, dst, int(ids[k]), 17, 1 if j + 1 < pieces else 0, j * piece, hl,
                 min(piece, length - j * piece), 0, k) for j, hl in enumerate(hdr_lens)]
        streams.append([recs[int(q)] for q in rng.permutation(pieces)])
        data.append((at, d))
        at += length + int(rng.integers(0, 4))
    buf = rng.integers(0, 256, at + 9, dtype=np.uint8)
    for o, d in data:
        buf[o: o + d.size] = d
    t = torch.from_numpy(buf).to(dev)
    recs = np.array(_interleave(rng, streams), dtype=REC)
    recs["frame"] += np.uint64(t.data_ptr())
    return recs, torch.from_numpy(recs.view(np.uint8).copy()).to(dev), Mem().add(t, buf)


def test_header_lengths_other_than_20(dev):
    """The descriptors and the ports lie at frame + hdr_len: header lengths of
    20, 24 and 60 within one datagram, the head record's 24 and 60."""
    rng = np.random.Generator(np.random.PCG64(46))
    specs = [(16, [24, 20, 60]), (8, [60, 24, 20, 20, 60]), (40, [20, 60]), (24, [24]), (32, [60]), (8, [20, 24]),
             (1480, [60, 24, 20]), (8, [28, 32, 36, 40, 44, 48, 52, 56] * 9)]
    recs, rec_t, mem = _direct_hdr(dev, rng, specs)
    st, emitted = _expect(recs)
    assert len(emitted) == len(specs) and np.all(st == COMPLETE)
    assert {int(recs[d.head]["hdr_len"]) for d in emitted} >= {20, 24, 60}
    assert any({int(recs[r]["hdr_len"]) for r, _, _ in d.pieces} == {20, 24, 60} for d in emitted)
    h = Raw(dev, recs.size).run(rec_t)
    _check(h, recs, st, emitted, mem)                   # the descriptor sources, and the hashes: ports at frame + hdr_len
    _wrapper_checks(rec_t, recs, emitted, mem)          # pack() bytes, the L4 verify through spans_desc


def test_frames_with_ip_options_end_to_end(dev):
    """Frames with ihl 6-15 cut by hand into complete datagrams -> ipv4_frames ->
    frag_records -> reassemble: every emitted record has hdr_len != 20."""
    rng = np.random.Generator(np.random.PCG64(47))
    frames, want_bytes = [], {}
    for k in range(40):
        src = int(rng.integers(1, 2**32))
        pieces = int(rng.choice([2, 3, 5, 9]))
        piece = 8 * int(rng.integers(1, 12))
        length = pieces * piece - int(rng.integers(0, 8))
        d = _udp_datagram(rng, src, HOST, length)
        want_bytes[(src, HOST, 1000 + k, 17)] = d
        for j in range(pieces):
            frames.append(_frame(src, HOST, 1000 + k, 17, 1 if j + 1 < pieces else 0, j * piece // 8,
                                 d[j * piece: (j + 1) * piece], ihl=int(rng.integers(6, 16)), pad=int(rng.integers(0, 5))))
    frames = [frames[int(i)] for i in rng.permutation(len(frames))]
    buf, offs, lens = _pack_frames(rng, frames)
    b = batch.PacketBatch.from_host(buf, offs, lens, device=dev)
    status = torch.zeros(b.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(b, status=status)
    rec_t = batch.frag_records(b, status, host_address=HOST, tag=9)
    recs = rec_t.cpu().numpy().view(REC)
    assert recs.size == len(frames) and np.all(recs["hdr_len"] > 20) and len(set(recs["hdr_len"].tolist())) == 10
    assert np.array_equal(recs["frame"], np.uint64(b.data.data_ptr()) + offs)
    st, emitted = _expect(recs)
    assert len(emitted) == 40 and np.all(st == COMPLETE)
    mem = Mem().add(b.data)
    h = Raw(dev, recs.size).run(rec_t)
    _check(h, recs, st, emitted, mem)
    for d in emitted:
        assert _bytes_of(d, recs, mem).tobytes() == want_bytes[d.key].tobytes()
    _wrapper_checks(rec_t, recs, emitted, mem)


# ---------------------------------------------------------------- key lengths

KEY_52 = KEY + bytes.fromhex("6d5a56da255b0ec24167253d")


@pytest.mark.parametrize("key_len", [4, 5, 13, 16, 39, 52])
def test_hash_keys_of_other_lengths(dev, key_len):
    """The key's bits past key_len are zero (toeplitz.hh:78-98 with a short
    key): dgram_hash against the oracle's toeplitz over src | dst | ports."""
    rng = np.random.Generator(np.random.PCG64(48))
    key = KEY_52[:key_len]
    recs, rec_t, mem = _direct(dev, rng, _small_specs())
    st, emitted = _expect(recs)
    h = Raw(dev, recs.size).run(rec_t, key=key)
    _check(h, recs, st, emitted, key=key, msg=f"key of {key_len} bytes")
    want = []
    for d in emitted:
        hr = recs[d.head]
        ports = mem.read(int(hr["frame"]) + int(hr["hdr_len"]), 4).tobytes() if d.length >= 8 else b""
        want.append(oracle.toeplitz(key, d.key[0].to_bytes(4, "big") + d.key[1].to_bytes(4, "big") + ports))
    assert len(emitted) >= 5 and len(set(want)) > 1
    assert np.array_equal(h["dgram_hash"][: 4 * len(emitted)].view(np.uint32), np.array(want, np.uint32))
