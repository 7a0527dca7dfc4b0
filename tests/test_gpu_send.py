"""Tx send on the device (sccsum_ipv4_send): the headers, fragment lists and
layout of every wire frame, compared byte for byte with the expectation
tests/test_send_host.py builds from synth.ipv4_fragment per datagram and
oracle.ip_checksum per header.  Nothing has a tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from seastar_amd import batch, native
from test_send_host import L4_LENS, NO_IP_CSUM, SEND_L4, TSO, UFO, expected_send

pytestmark = pytest.mark.gpu

SRC = 0xC0A80A01
GUARD = 64   # poisoned bytes behind every output
POISON = 0xA5
OUT_ELEM = dict(hdr=20, desc=32, first=4, out_off=8, out_len=4)  # bytes per frame of the per-frame outputs


@functools.lru_cache(maxsize=None)
def _tiles() -> tuple:
    lib = native.load()
    return int(lib.sccsum_send_tile_datagrams()), int(lib.sccsum_send_emit_tile_frames())


def _datagrams(rng, lens, protos=None, valid_l4=False, tail=5):
    """L4 datagrams of the given lengths packed at odd offsets with 0-3 byte
    gaps: (buf, off, lens, dst, proto, ids).  With valid_l4, UDP (>= 8 bytes)
    and TCP (>= 20) datagrams carry the checksum the L4 writers store before
    ipv4::send (udp.cc:184-195, tcp.hh:1656-1694), from the oracle."""
    lens = np.asarray(lens, dtype=np.uint32)
    n = lens.size
    off = np.empty(n, np.uint64)
    pos = 3
    for i in range(n):
        pos += int(rng.integers(0, 4))
        off[i] = pos
        pos += int(lens[i])
    buf = rng.integers(0, 256, size=pos + tail, dtype=np.uint8)
    proto = (rng.choice([6, 17, 1, 47], size=n) if protos is None else np.asarray(protos)).astype(np.uint8)
    dst = rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    ids = rng.integers(0, 65536, size=n).astype(np.uint16)
    if valid_l4:
        for i in range(n):
            o, ln, p = int(off[i]), int(lens[i]), int(proto[i])
            fo = 6 if p == 17 else 16
            if (p == 17 and ln >= 8) or (p == 6 and ln >= 20):
                l4 = buf[o:o + ln]
                if p == 17:
                    l4[4], l4[5] = ln >> 8, ln & 0xFF
                else:
                    l4[12] = 0x50
                l4[fo:fo + 2] = 0
                seed = oracle.pseudo_seed(SRC, int(dst[i]), p, ln)
                c = oracle.batch_spans(l4, np.zeros(1, np.uint64), np.array([ln], np.uint32), np.array([seed], np.uint32))
                l4[fo:fo + 2] = np.frombuffer(np.uint16(c[0]).tobytes(), np.uint8)
    return buf, off, lens, dst, proto, ids


def _dev_inputs(dev, buf, off, lens, dst, proto, ids):
    l4 = batch.PacketBatch.from_host(buf, off, lens, device=dev)
    return (l4, torch.from_numpy(dst.view(np.int32).copy()).to(dev), torch.from_numpy(proto.copy()).to(dev),
            None if ids is None else torch.from_numpy(ids.view(np.int16).copy()).to(dev))


class Raw:
    """sccsum_ipv4_send through the C-ABI into outputs this test owns: every
    array has room for `room` frames (n + 1 / n / 3 entries for the per-datagram
    ones) plus GUARD bytes, all poisoned with 0xA5 before each run."""

    def __init__(self, dev, l4, d_dst, d_proto, d_ids, room, hdr_shift=0):
        self.dev, self.l4, self.dst, self.proto, self.ids, self.room = dev, l4, d_dst, d_proto, d_ids, int(room)
        self.hdr_shift = hdr_shift  # d_hdr starts this many bytes into its (aligned) buffer
        n = l4.n
        self.size = dict(hdr=20 * self.room, desc=32 * self.room, first=4 * (self.room + 1), out_off=8 * self.room,
                         out_len=4 * self.room, dgram_first=4 * (n + 1), status=n, total=24)
        self.buf = {k: torch.empty(v + GUARD + (hdr_shift if k == "hdr" else 0), dtype=torch.uint8, device=dev)
                    for k, v in self.size.items()}
        self.ws = torch.empty(int(native.load().sccsum_ipv4_send_workspace(n)), dtype=torch.uint8, device=dev)

    def run(self, mtu, flags=0, max_frames=None, max_out_bytes=0xFFFFFFFF, l4sum=None, use_ids=True):
        max_frames = self.room if max_frames is None else int(max_frames)
        assert max_frames <= self.room
        for t in self.buf.values():
            t.fill_(POISON)
        n = self.l4.n
        opts = native.SendOpts(SRC, mtu, flags)
        p = {k: v.data_ptr() + (self.hdr_shift if k == "hdr" else 0) for k, v in self.buf.items()}
        ids = self.ids if use_ids else None
        code = native.load().sccsum_ipv4_send(
            ctypes.addressof(opts), self.l4.data.data_ptr(), self.l4.bytes_len, self.l4.off.data_ptr() if n else None,
            self.l4.length.data_ptr() if n else None, self.dst.data_ptr() if n else None,
            self.proto.data_ptr() if n else None, None if ids is None or not n else ids.data_ptr(),
            None if l4sum is None else l4sum.data_ptr(), n, max_frames, int(max_out_bytes), p["hdr"], p["desc"],
            p["first"], p["out_off"], p["out_len"], p["dgram_first"], p["status"], p["total"], self.ws.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
        native.check(code, "sccsum_ipv4_send")
        torch.cuda.synchronize()
        b, s = self.buf, self.size
        return batch.SendResult(
            l4=self.l4, hdr=b["hdr"][self.hdr_shift: self.hdr_shift + s["hdr"]], desc=b["desc"][: s["desc"]],
            first=b["first"][: s["first"]].view(torch.int32), out_off=b["out_off"][: s["out_off"]].view(torch.int64),
            out_len=b["out_len"][: s["out_len"]].view(torch.int32),
            dgram_first=b["dgram_first"][: s["dgram_first"]].view(torch.int32), status=b["status"][: s["status"]],
            total=b["total"][:24].view(torch.int64), max_frames=max_frames, max_out_bytes=int(max_out_bytes))

    def host(self) -> dict:
        return {k: v.cpu().numpy().copy() for k, v in self.buf.items()}

    def untouched_past(self, frames: int) -> None:
        """Nothing past the emitted part of a per-frame array (d_first: past its
        closing entry), nothing past the end of the others."""
        h = self.host()
        for k, v in h.items():
            written = self.size[k] if k not in OUT_ELEM else OUT_ELEM[k] * frames + (4 if k == "first" else 0)
            before = self.hdr_shift if k == "hdr" else 0
            assert np.all(v[:before] == POISON) and np.all(v[before + written:] == POISON), (k, frames)


def _check(r, exp, off, msg=""):
    """Every output of a run against the expectation (synchronises)."""
    torch.cuda.synchronize()
    e = len(exp["frames"])
    assert r.totals() == exp["total"], msg
    assert r.frames_emitted() == e, msg
    assert np.array_equal(r.status.cpu().numpy(), exp["status"]), msg
    assert np.array_equal(r.dgram_first.cpu().numpy().view(np.uint32), exp["dgram_first"]), msg
    assert np.array_equal(r.first[: e + 1].cpu().numpy().view(np.uint32), exp["first"]), msg
    assert np.array_equal(r.out_off[:e].cpu().numpy().view(np.uint64), exp["out_off"]), msg
    assert np.array_equal(r.out_len[:e].cpu().numpy().view(np.uint32), exp["out_len"]), msg
    assert np.array_equal(r.hdr[: 20 * e].cpu().numpy(), exp["hdr"]), msg
    d = r.desc[: 32 * e].cpu().numpy().view(batch.DESC_DTYPE)
    f = np.arange(e, dtype=np.uint64)
    own = np.array([off[i] + np.uint64(o) for i, o in exp["owner"]], dtype=np.uint64)
    assert np.array_equal(d["src"][0::2], np.uint64(r.hdr.data_ptr()) + 20 * f), msg
    assert np.array_equal(d["dst_off"][0::2], exp["out_off"].astype(np.uint32)), msg
    assert np.all(d["len"][0::2] == 20), msg
    assert np.array_equal(d["src"][1::2], np.uint64(r.l4.data.data_ptr()) + own), msg
    assert np.array_equal(d["dst_off"][1::2], (exp["out_off"] + 20).astype(np.uint32)), msg
    assert np.array_equal(d["len"][1::2], exp["out_len"] - 20), msg
    packed = r.pack()
    torch.cuda.synchronize()
    assert packed.n == e and packed.bytes_len == exp["packed"].size, msg
    assert np.array_equal(packed.data.cpu().numpy()[: packed.bytes_len], exp["packed"]), msg
    assert np.array_equal(packed.off.cpu().numpy().view(np.uint64), exp["out_off"]), msg
    assert np.array_equal(packed.length.cpu().numpy().view(np.uint32), exp["out_len"]), msg


@pytest.mark.parametrize("mtu", [68, 576, 1500, 65535])
def test_parity(dev, mtu):
    rng = np.random.default_rng(0x5E4D + mtu)
    lens = rng.permutation(np.array(L4_LENS))
    protos = rng.permutation(np.resize([6, 17, 1, 47], lens.size))
    buf, off, lens, dst, proto, ids = _datagrams(rng, lens, protos=protos)
    assert np.any(off % 2 == 1)
    l4, d_dst, d_proto, d_ids = _dev_inputs(dev, buf, off, lens, dst, proto, ids)
    exp = expected_send(buf, off, lens, dst, proto, mtu, SRC, ids=ids)
    r = batch.ipv4_send(l4, d_dst, d_proto, mtu, SRC, ids=d_ids)
    _check(r, exp, off, f"mtu {mtu}")
    assert np.array_equal(l4.data.cpu().numpy()[: buf.size], buf)  # the datagrams are not written
    # ids=None: identification 0, what the reference writes
    r0 = batch.ipv4_send(l4, d_dst, d_proto, mtu, SRC)
    _check(r0, expected_send(buf, off, lens, dst, proto, mtu, SRC), off, f"mtu {mtu}, no ids")
    # twice into the same arrays: identical bytes in every output
    raw = Raw(dev, l4, d_dst, d_proto, d_ids, room=exp["total"][0] + 3)
    _check(raw.run(mtu), exp, off, f"mtu {mtu}, raw")
    raw.untouched_past(len(exp["frames"]))
    a = raw.host()
    raw.run(mtu)
    b = raw.host()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_header_array_at_any_alignment(dev, shift):
    """d_hdr is a byte array: at an address that is no multiple of 4 the
    headers are the same bytes, and the header descriptors point at them."""
    rng = np.random.default_rng(0x5E55 + shift)
    buf, off, lens, dst, proto, ids = _datagrams(rng, rng.permutation(np.array(L4_LENS)))
    l4, d_dst, d_proto, d_ids = _dev_inputs(dev, buf, off, lens, dst, proto, ids)
    exp = expected_send(buf, off, lens, dst, proto, 576, SRC, ids=ids)
    raw = Raw(dev, l4, d_dst, d_proto, d_ids, room=exp["total"][0] + 2, hdr_shift=shift)
    r = raw.run(576)
    assert r.hdr.data_ptr() % 4 == shift
    _check(r, exp, off, f"hdr shift {shift}")
    raw.untouched_past(len(exp["frames"]))


def test_existing_calls_consume_the_output(dev):
    """The emitted lists are arguments of the *_desc calls as they stand."""
    rng = np.random.default_rng(0x5E4E)
    sizes = [8, 100, 20, 1480, 1481, 2960, 4000, 9000, 65515, 1479, 30001, 64]
    protos = [17, 6, 6, 17, 6, 17, 6, 17, 6, 1, 17, 47]
    buf, off, lens, dst, proto, ids = _datagrams(rng, sizes, protos=protos, valid_l4=True)
    l4, d_dst, d_proto, d_ids = _dev_inputs(dev, buf, off, lens, dst, proto, ids)
    exp = expected_send(buf, off, lens, dst, proto, 1500, SRC, ids=ids)
    r = batch.ipv4_send(l4, d_dst, d_proto, 1500, SRC, ids=d_ids)
    desc, first, out_off, out_len, max_len = r.lists()
    e = int(out_off.numel())
    assert e == len(exp["frames"]) and max_len == 1500
    st = torch.empty(e, dtype=torch.uint8, device=dev)
    got = batch.ipv4_frames_desc(desc, first, out_off, out_len, max_len, status=st)
    torch.cuda.synchronize()
    want, want_st = oracle.batch_ipv4(exp["packed"], exp["out_off"], exp["out_len"])
    st = st.cpu().numpy()
    assert np.array_equal(batch.as_u16(got), want) and np.array_equal(st, want_st)
    df = exp["dgram_first"]
    for i in range(len(sizes)):
        idx = np.arange(df[i], df[i + 1])
        assert np.all(st[idx] & native.ST_OK)
        if idx.size > 1:
            assert np.all(st[idx] == native.ST_OK | native.ST_IPFRAG)
        elif protos[i] in (6, 17):
            assert st[idx[0]] == native.ST_OK | native.ST_L4_OK
    # every cut datagram, reassembled from its payload records with its pseudo-header seed, sums to 0
    d = r.desc[: 32 * e].cpu().numpy().view(batch.DESC_DTYPE)
    src_a, dst_off, flen, pfirst, doff, dlen, seeds = [], [], [], [0], [], [], []
    pos = 0
    for i in range(len(sizes)):
        if df[i + 1] - df[i] < 2 or protos[i] not in (6, 17):
            continue
        doff.append(pos)
        for f in range(df[i], df[i + 1]):
            src_a.append(int(d["src"][2 * f + 1]))
            dst_off.append(pos)
            flen.append(int(d["len"][2 * f + 1]))
            pos += flen[-1]
        pfirst.append(len(src_a))
        dlen.append(pos - doff[-1])
        assert dlen[-1] == sizes[i]
        seeds.append(oracle.pseudo_seed(SRC, int(dst[i]), protos[i], sizes[i]))
    assert len(doff) >= 5
    rec = torch.from_numpy(batch.make_desc(np.array(src_a, np.uint64), np.array(dst_off, np.uint32),
                                           np.array(flen, np.uint32)).view(np.uint8)).to(dev)
    sums = batch.spans_desc(rec, torch.from_numpy(np.array(pfirst, np.int32)).to(dev),
                            torch.from_numpy(np.array(doff, np.int64)).to(dev),
                            torch.from_numpy(np.array(dlen, np.int32)).to(dev), max(dlen),
                            seeds=torch.from_numpy(np.array(seeds, np.uint32).view(np.int32)).to(dev))
    torch.cuda.synchronize()
    assert np.all(batch.as_u16(sums) == 0)


def test_flags(dev):
    rng = np.random.default_rng(0x5E4F)
    buf, off, lens, dst, proto, ids = _datagrams(rng, [9000, 9000, 100, 3000], protos=[6, 17, 6, 1])
    l4, d_dst, d_proto, d_ids = _dev_inputs(dev, buf, off, lens, dst, proto, ids)
    for flags, counts in ((TSO, [1, 7, 1, 3]), (UFO, [7, 1, 1, 3]), (TSO | UFO, [1, 1, 1, 3]), (0, [7, 7, 1, 3])):
        exp = expected_send(buf, off, lens, dst, proto, 1500, SRC, ids=ids, flags=flags)
        assert np.diff(exp["dgram_first"].astype(np.int64)).tolist() == counts
        r = batch.ipv4_send(l4, d_dst, d_proto, 1500, SRC, ids=d_ids, flags=flags)
        _check(r, exp, off, f"flags {flags}")
    exp = expected_send(buf, off, lens, dst, proto, 1500, SRC, ids=ids, flags=NO_IP_CSUM | TSO)
    r = batch.ipv4_send(l4, d_dst, d_proto, 1500, SRC, ids=d_ids, flags=NO_IP_CSUM | TSO)
    _check(r, exp, off, "no ip csum")
    hdr = r.hdr[: 20 * r.frames_emitted()].cpu().numpy().reshape(-1, 20)
    assert hdr.shape[0] == 12 and np.all(hdr[:, 10:12] == 0)


def test_send_l4_stores_the_l4_values(dev):
    """SEND_L4 stores l4sum at UDP +6 / TCP +16 of emitted datagrams that hold
    the field, and writes nothing else into the datagram buffer."""
    rng = np.random.default_rng(0x5E50)
    sizes = [7, 8, 100, 19, 20, 300, 64, 64, 100, 2000, 40]
    protos = [17, 17, 17, 6, 6, 6, 1, 47, 17, 6, 17]
    buf, off, lens, dst, proto, ids = _datagrams(rng, sizes, protos=protos)
    off[8] = buf.size - 50  # refused: 100 bytes from 50 before the end
    sums = rng.integers(1, 65536, size=len(sizes)).astype(np.uint16)
    l4, d_dst, d_proto, d_ids = _dev_inputs(dev, buf, off, lens, dst, proto, ids)
    d_sums = torch.from_numpy(sums.view(np.int16).copy()).to(dev)
    # the last datagram is past the frame cap: not emitted, not written
    need = 9 + 2  # nine single frames (one refused datagram has none) + the 2000-byte TCP datagram's two
    want_buf = buf.copy()
    for i in (1, 2, 4, 5, 9):
        at = int(off[i]) + (6 if protos[i] == 17 else 16)
        want_buf[at:at + 2] = np.frombuffer(sums[i].tobytes(), np.uint8)
    exp = expected_send(want_buf, off, lens, dst, proto, 1500, SRC, ids=ids, flags=SEND_L4, max_frames=need - 1)
    assert exp["total"] == (need, int(np.delete(lens, 8).sum()) + 20 * need, 10)
    assert exp["status"].tolist() == [1] * 8 + [native.ST_RANGE, 1, 0]
    r = batch.ipv4_send(l4, d_dst, d_proto, 1500, SRC, ids=d_ids, l4sum=d_sums, flags=SEND_L4, max_frames=need - 1)
    _check(r, exp, off, "SEND_L4")
    assert np.array_equal(l4.data.cpu().numpy()[: buf.size], want_buf)


def test_tile_edges(dev):
    tile, emit_tile = _tiles()
    rng = np.random.default_rng(0x5E51)
    for n in (1, tile - 1, tile, tile + 1, 2 * tile + 3):
        lens = rng.choice([0, 0, 1, 47, 48, 49, 96, 97, 150], size=n)
        big = min(n - 1, tile - 1)  # the longest datagram ends the first tile, empty ones around it
        lens[max(big - 2, 0):big + 3] = 0
        lens[big] = 65515
        buf, off, lens, dst, proto, ids = _datagrams(rng, lens)
        l4, d_dst, d_proto, d_ids = _dev_inputs(dev, buf, off, lens, dst, proto, ids)
        exp = expected_send(buf, off, lens, dst, proto, 68, SRC, ids=ids)
        df = exp["dgram_first"].astype(np.int64)
        assert df[big + 1] - df[big] == 1365 and df[big] // emit_tile != (df[big + 1] - 1) // emit_tile
        raw = Raw(dev, l4, d_dst, d_proto, d_ids, room=exp["total"][0] + 1)
        _check(raw.run(68), exp, off, f"n {n}")
        raw.untouched_past(len(exp["frames"]))


def _need(opts, lens, proto):
    lib = native.load()
    frames = nbytes = 0
    for ln, p in zip(lens.tolist(), proto.tolist()):
        nf, nb = ctypes.c_uint32(), ctypes.c_uint64()
        assert lib.sccsum_ipv4_send_plan(ctypes.addressof(opts), ln, p, ctypes.byref(nf), ctypes.byref(nb)) == 0
        frames += nf.value
        nbytes += nb.value
    return frames, nbytes


@pytest.mark.parametrize("shape", ["one_tile", "second_tile"])
def test_caps(dev, shape):
    tile, _ = _tiles()
    rng = np.random.default_rng(0x5E52)
    if shape == "one_tile":
        mtu = 576
        lens = rng.choice([0, 8, 100, 556, 557, 1480, 2961, 5000], size=40)
        lens[-1] = 700  # the last datagram has two frames
    else:
        mtu = 68
        lens = rng.choice([0, 1, 40, 48, 49, 100], size=tile + 50)
    buf, off, lens, dst, proto, ids = _datagrams(rng, lens)
    l4, d_dst, d_proto, d_ids = _dev_inputs(dev, buf, off, lens, dst, proto, ids)
    need_f, need_b = _need(native.SendOpts(SRC, mtu, 0), lens, proto)
    full = expected_send(buf, off, lens, dst, proto, mtu, SRC, ids=ids)
    assert full["total"] == (need_f, need_b, lens.size)
    raw = Raw(dev, l4, d_dst, d_proto, d_ids, room=need_f + 8)
    mid = int(full["dgram_first"][lens.size - 20])  # a cap inside the batch (the second tile of the larger shape)
    mid_b = int(full["out_off"][mid]) + 7
    for max_frames, max_bytes in ((need_f - 1, 0xFFFFFFFF), (need_f + 8, need_b - 1), (mid + 1, 0xFFFFFFFF),
                                  (need_f + 8, mid_b), (0, 0xFFFFFFFF), (need_f + 8, 0)):
        exp = expected_send(buf, off, lens, dst, proto, mtu, SRC, ids=ids, max_frames=max_frames,
                            max_out_bytes=max_bytes)
        assert exp["total"][:2] == (need_f, need_b) and exp["total"][2] < lens.size
        r = raw.run(mtu, max_frames=max_frames, max_out_bytes=max_bytes)
        _check(r, exp, off, f"caps {max_frames} {max_bytes}")
        raw.untouched_past(len(exp["frames"]))
        # a rerun with the reported need emits everything
        got_f, got_b, _ = r.totals()
        _check(raw.run(mtu, max_frames=got_f, max_out_bytes=got_b), full, off, "rerun with the need")
        raw.untouched_past(need_f)


def test_refusals(dev):
    rng = np.random.default_rng(0x5E53)
    lens = np.array([100, 300, 200, 10, 65516, 50, 2**32 - 1, 1481, 0], dtype=np.uint32)
    buf, off, _, dst, proto, ids = _datagrams(rng, np.where(lens > 70000, 0, lens), tail=0)
    off[1] = buf.size - 299          # off + len one past the buffer
    off[3] = 2**32 + int(off[2])     # the low 32 bits would be in range
    assert int(off[4]) + 65516 <= buf.size
    bad = [1, 3, 4, 6]
    l4, d_dst, d_proto, d_ids = _dev_inputs(dev, buf, off, lens, dst, proto, ids)
    exp = expected_send(buf, off, lens, dst, proto, 1500, SRC, ids=ids)
    R, M = native.ST_RANGE, native.ST_MALFORMED
    assert exp["status"].tolist() == [1, R, 1, R, M, 1, R | M, 1, 1]
    assert np.all(np.diff(exp["dgram_first"].astype(np.int64))[bad] == 0)
    raw = Raw(dev, l4, d_dst, d_proto, d_ids, room=16)
    _check(raw.run(1500), exp, off, "refusals")
    raw.untouched_past(len(exp["frames"]))
    # the neighbours' frames are those of a run without the refused datagrams
    keep = np.setdiff1d(np.arange(lens.size), bad)
    l4k, dk, pk, ik = _dev_inputs(dev, buf, off[keep], lens[keep], dst[keep], proto[keep], ids[keep])
    rk = batch.ipv4_send(l4k, dk, pk, 1500, SRC, ids=ik)
    torch.cuda.synchronize()
    assert rk.totals() == (len(exp["frames"]), exp["packed"].size, keep.size)
    assert np.all(rk.status.cpu().numpy() == native.ST_OK)
    pk_ = rk.pack()
    torch.cuda.synchronize()
    assert np.array_equal(pk_.data.cpu().numpy()[: pk_.bytes_len], exp["packed"])
    assert np.array_equal(rk.dgram_first.cpu().numpy().view(np.uint32), exp["dgram_first"][np.append(keep, lens.size)])


def test_a_long_run_of_refused_datagrams(dev):
    """More refused datagrams in a row than an emit tile has frames: the frames
    on either side of the run find their datagrams across it."""
    _, emit_tile = _tiles()
    rng = np.random.default_rng(0x5E54)
    n = 3 * emit_tile + 40
    buf, off, lens, dst, proto, ids = _datagrams(rng, rng.choice([0, 8, 48, 49, 100], size=n))
    off[30:n - 25] += np.uint64(1 << 40)
    l4, d_dst, d_proto, d_ids = _dev_inputs(dev, buf, off, lens, dst, proto, ids)
    exp = expected_send(buf, off, lens, dst, proto, 68, SRC, ids=ids)
    assert exp["total"][2] == n and np.count_nonzero(exp["status"] == native.ST_RANGE) == n - 55
    raw = Raw(dev, l4, d_dst, d_proto, d_ids, room=exp["total"][0] + 2)
    _check(raw.run(68), exp, off, "refused run")
    raw.untouched_past(len(exp["frames"]))


def test_no_datagrams(dev):
    e = np.zeros(0, np.uint8)
    l4, d_dst, d_proto, d_ids = _dev_inputs(dev, e, np.zeros(0, np.uint64), np.zeros(0, np.uint32),
                                            np.zeros(0, np.uint32), e, np.zeros(0, np.uint16))
    r = batch.ipv4_send(l4, d_dst, d_proto, 1500, SRC, ids=d_ids)
    torch.cuda.synchronize()
    assert r.totals() == (0, 0, 0) and r.frames_emitted() == 0
    assert r.dgram_first.cpu().numpy().tolist() == [0] and r.first.cpu().numpy()[0] == 0
    p = r.pack()
    assert p.n == 0 and p.bytes_len == 0
    raw = Raw(dev, l4, d_dst, d_proto, d_ids, room=4)
    r = raw.run(1500)
    assert r.totals() == (0, 0, 0) and r.dgram_first.cpu().numpy().tolist() == [0]
    raw.untouched_past(0)
