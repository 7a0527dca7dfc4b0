"""The code of reasm.hip, send.hip and bucket_pass.h that only large batches
reach, against the vectorised expectations of tests/fast_models.py (pinned to
the per-record models by tests/test_fast_models.py).  Byte for byte, every
output with poisoned guard bytes, the workspace poisoned.

The carry kernels (rec_carry, seg_carry, dg_carry, st_carry, send_scan) are ONE
block of 1024 threads — the scan kernels' block size, equal to their tile — that
takes the per-tile values 1024 at a time: a second chunk needs more than 1024
tiles.  The radix sort's scan_row takes a digit's row of per-tile counts 256 at
a time.  N = 1024 tiles + 1 tile + 7 entries is 1026 scan tiles (two chunks)
and 513 sort tiles (three chunks, the last of one tile); each test asserts the
counts, so that another tile size fails the test instead of hollowing it."""
import numpy as np
import pytest
import torch

import fast_models
import oracle
import test_gpu_reasm as R
import test_gpu_send as S
from seastar_amd import batch, native, synth
from test_send_host import L4_LENS, expected_send

pytestmark = pytest.mark.gpu

CHUNK = 1024          # tiles per round of a carry kernel's loop: its block size
SORT_CHUNK = 256      # tiles per round of bucket_pass::scan_row
POISON = 0xA5


# ---------------------------------------------------------------- reassembly

def _reasm_n() -> int:
    sort, scan = R._tiles()
    n = CHUNK * scan + scan + 7
    assert -(-n // scan) > CHUNK and -(-n // sort) > 2 * SORT_CHUNK
    return n


@pytest.fixture(scope="module")
def reasm_input():
    """N plain UDP records (frame addresses relative to the payload buffer),
    the buffer, and the hashes of the datagrams they complete, in delivery order."""
    n = _reasm_n()
    rng = np.random.Generator(np.random.PCG64(0x5CA1E))
    recs, buf = fast_models.plain_udp_records(rng, n)
    exp = fast_models.reasm_plain(recs)
    st = exp["state"]
    # the input mix: mostly complete, a good share pending, and mix collisions alone supply host records
    assert np.count_nonzero(st == R.COMPLETE) >= n // 2 and np.count_nonzero(st == R.PENDING) >= n // 20
    assert np.count_nonzero(st == R.HOSTB) >= 2 and fast_models.reasm_plain(recs, mix=None)["total"][3] == 0
    # the frames the host would assemble (ip.cc:439-455), hashed by the oracle as test_gpu_reasm._check does
    D, K = exp["total"][:2]
    head = recs[exp["head"]]
    hdr = np.zeros((D, 20), np.uint8)
    synth.write_ipv4_header(hdr, 20 + exp["len"].astype(np.int64), 17, head["src"], head["dst"])
    flen = 20 + exp["len"].astype(np.int64)
    foff = np.concatenate([[0], np.cumsum(flen)])
    flat = np.zeros(int(foff[-1]), np.uint8)
    flat[(foff[:-1, None] + np.arange(20)).reshape(-1)] = hdr.reshape(-1)
    ln = exp["desc"]["len"].astype(np.int64)
    run = np.cumsum(ln)
    within = np.arange(int(run[-1]), dtype=np.int64) - np.repeat(run - ln, ln)
    dgram_of = np.repeat(np.arange(D), np.diff(exp["first"].astype(np.int64)))
    flat[np.repeat(exp["desc"]["dst_off"].astype(np.int64) + 20 * (dgram_of + 1), ln) + within] = \
        buf[np.repeat(exp["desc"]["src"].astype(np.int64), ln) + within]
    want_hash, _ = oracle.batch_ipv4_rss(flat, foff[:-1].astype(np.uint64), flen.astype(np.uint32), R.KEY,
                                         native.RSS_REASSEMBLED)
    return recs, buf, want_hash


def _check_reasm(h, recs, exp, want_hash, msg):
    m = recs.size
    D, K, P, H = exp["total"]
    assert h["total"][:32].view(np.uint64).tolist() == [D, K, P, H], msg
    assert np.array_equal(h["rec_state"][:m], exp["state"]), msg
    assert h["pending"][: 32 * P].tobytes() == exp["pending"].tobytes(), msg
    assert h["host"][: 32 * H].tobytes() == exp["host"].tobytes(), msg
    assert np.array_equal(h["dgram_first"][: 4 * (D + 1)].view(np.uint32), exp["first"]), msg
    assert np.array_equal(h["dgram_off"][: 8 * D].view(np.uint64), exp["off"]), msg
    for name in ("len", "head", "last", "seed"):
        assert np.array_equal(h["dgram_" + name][: 4 * D].view(np.uint32), exp[name]), (name, msg)
    assert h["desc"][: 16 * K].tobytes() == exp["desc"].tobytes(), msg
    assert np.array_equal(h["dgram_hash"][: 4 * D].view(np.uint32), want_hash[:D]), msg
    written = dict(desc=16 * K, dgram_first=4 * (D + 1), dgram_off=8 * D, dgram_len=4 * D, dgram_seed=4 * D,
                   dgram_head=4 * D, dgram_last=4 * D, dgram_hash=4 * D, pending=32 * P, host=32 * H, rec_state=m,
                   total=32)
    for name, w in written.items():
        assert np.all(h[name][w:] == POISON), (name, msg)


def _reasm_on_device(dev, reasm_input):
    recs0, buf, want_hash = reasm_input
    payload = torch.from_numpy(buf).to(dev)
    recs = recs0.copy()
    recs["frame"] += np.uint64(payload.data_ptr())
    rec_t = torch.from_numpy(recs.view(np.uint8)).to(dev)
    return recs, rec_t, payload, want_hash


def test_reassembly_of_more_than_one_carry_chunk(dev, reasm_input):
    recs, rec_t, payload, want_hash = _reasm_on_device(dev, reasm_input)
    assert recs.size == _reasm_n()                      # 1026 scan tiles, 513 sort tiles
    exp = fast_models.reasm_plain(recs)
    raw = R.Raw(dev, recs.size)
    _check_reasm(raw.run(rec_t), recs, exp, want_hash, "every datagram")
    del raw, rec_t, payload
    torch.cuda.empty_cache()


def test_reassembly_capacity_cut_in_the_second_carry_chunk(dev, reasm_input):
    """max_out_bytes one byte short of a datagram whose completing record lies
    in scan tile >= 1024: dg_carry finds the cut tile in its second chunk."""
    recs, rec_t, payload, want_hash = _reasm_on_device(dev, reasm_input)
    scan = R._tiles()[1]
    assert recs.size == _reasm_n()                      # 1026 scan tiles, 513 sort tiles
    every = fast_models.reasm_plain(recs)
    d = int(np.searchsorted(every["last"], CHUNK * scan)) + 300
    assert d < every["total"][0] - 1 and int(every["last"][d]) // scan >= CHUNK
    cap = int(every["off"][d]) + int(every["len"][d]) - 1
    exp = fast_models.reasm_plain(recs, cap=cap)
    assert exp["total"][0] == d and exp["total"][2] > every["total"][2]
    late = every["rows"][int(every["first"][d]):]                 # the records of the keys that do not fit
    assert late.size and np.all(exp["state"][late] == R.PENDING)
    raw = R.Raw(dev, recs.size)
    _check_reasm(raw.run(rec_t, max_out_bytes=cap), recs, exp, want_hash, f"cap {cap}")
    del raw, rec_t, payload
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- records

HOSTS = np.array([R.HOST, R.HOST ^ 0x100], np.uint32)


def _rx_frames_2d(rng, n, width=72):
    """n frames of `width` bytes with valid header checksums: whole datagrams
    and fragments, two destinations, ihl 5-15, IP total lengths at, below and
    past the frame's, offsets past 65535; and random status bytes."""
    f = rng.integers(0, 256, (n, width), dtype=np.uint8)
    ihl = rng.choice([5, 5, 5, 5, 6, 8, 15], n)
    ip_len = rng.choice([width, width, width, width - 4, 4 * 15 - 1, width + 4], n)   # trimmed, short of ihl 15, too long
    kind = rng.integers(0, 8, n)                      # 0-1 whole datagrams, 2-6 fragments, 7 an offset past 65535
    frag = np.where(kind < 2, 0, np.where(kind == 7, 0x1FFF, rng.integers(1, 0x1F00, n) | (rng.integers(0, 2, n) << 13)))
    frag[kind == 6] = 0x2000                          # the first fragment
    f[:, 0] = 0x40 | ihl
    f[:, 2], f[:, 3] = ip_len >> 8, ip_len & 0xFF
    f[:, 6], f[:, 7] = frag >> 8, frag & 0xFF
    dst = HOSTS[rng.integers(0, 2, n)]
    for k in range(4):
        f[:, 16 + k] = (dst >> (24 - 8 * k)) & 0xFF
    f[:, 10:12] = 0
    c = oracle.batch_spans(f.reshape(-1), width * np.arange(n, dtype=np.uint64), np.full(n, 20, np.uint32))
    f[:, 10:12] = c.view(np.uint8).reshape(n, 2)
    assert oracle.ip_checksum(f[n - 1, :20]) == 0
    off = width * np.arange(n, dtype=np.uint64)
    lens = np.full(n, width, np.uint32)
    return f, off, lens, rng.integers(0, 256, n, dtype=np.uint8)


def test_records_of_more_than_one_carry_chunk(dev):
    """rec_carry's second chunk; the status bytes are random, so the two masks
    decide on their own, through several mask pairs."""
    n = _reasm_n()
    f, off, lens, status = _rx_frames_2d(np.random.Generator(np.random.PCG64(0x5CA1F)), n)
    b = batch.PacketBatch.from_host(f.reshape(-1), off, lens, device=dev)
    d_status = torch.from_numpy(status).to(dev)
    base = b.data.data_ptr()
    ok, frg, bad = native.ST_OK, native.ST_IPFRAG, native.ST_MALFORMED | native.ST_RANGE
    counts = []
    for need, reject, host in ((ok | frg, bad, R.HOST), (0, 0, R.HOST), (0, bad, 0), (ok, 0, R.HOST),
                               (ok | native.ST_L4_OK | frg, 0xE0, R.HOST), (0x80, 0x7F, 0)):
        want, by_status, by_header = fast_models.frag_records_plain(f, off, lens, status, need, reject, host, base,
                                                                   0xC0DE0000 + need)
        assert 0 < want.size < n and np.any(by_status & ~by_header) and ((need | reject) == 0 or np.any(by_header & ~by_status))
        rec, count = R._records_raw(dev, b, d_status, n, host, 0xC0DE0000 + need, need=need, reject=reject)
        msg = f"need {need:#x} reject {reject:#x} host {host:#x}"
        assert int(count[:4].view(np.uint32)[0]) == want.size and np.all(count[4:] == POISON), msg
        assert rec[: 32 * want.size].tobytes() == want.tobytes(), msg
        assert np.all(rec[32 * want.size:] == POISON), msg
        counts.append(want.size)
        assert np.any(want["hdr_len"] > 20) and set(want["dst"].tolist()) == ({R.HOST} if host else set(HOSTS.tolist()))
    assert len(set(counts)) == len(counts)
    del b, d_status
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- send

def _send_n() -> int:
    tile = S._tiles()[0]
    n = CHUNK * tile + tile + 7
    assert -(-n // tile) > CHUNK
    return n


def _check_send(raw, r, exp, off, msg):
    """Every output of a Raw run against fast_models.send_plain's."""
    torch.cuda.synchronize()
    e = exp["emitted"]
    assert r.totals() == exp["total"] and r.frames_emitted() == e, msg
    h = raw.host()
    assert np.array_equal(h["status"][: raw.size["status"]], exp["status"]), msg
    assert np.array_equal(h["dgram_first"][: raw.size["dgram_first"]].view(np.uint32), exp["dgram_first"]), msg
    assert np.array_equal(h["first"][: 4 * (e + 1)].view(np.uint32), exp["first"]), msg
    assert np.array_equal(h["out_off"][: 8 * e].view(np.uint64), exp["out_off"]), msg
    assert np.array_equal(h["out_len"][: 4 * e].view(np.uint32), exp["out_len"]), msg
    assert np.array_equal(h["hdr"][: 20 * e], exp["hdr"].reshape(-1)), msg
    d = h["desc"][: 32 * e].view(batch.DESC_DTYPE)
    f = np.arange(e, dtype=np.uint64)
    assert np.array_equal(d["src"][0::2], np.uint64(r.hdr.data_ptr()) + 20 * f), msg
    assert np.array_equal(d["dst_off"][0::2], exp["out_off"].astype(np.uint32)), msg
    assert np.all(d["len"][0::2] == 20), msg
    assert np.array_equal(d["src"][1::2], np.uint64(r.l4.data.data_ptr()) + off[exp["owner"]]
                          + exp["piece_off"].astype(np.uint64)), msg
    assert np.array_equal(d["dst_off"][1::2], (exp["out_off"] + np.uint64(20)).astype(np.uint32)), msg
    assert np.array_equal(d["len"][1::2], exp["out_len"] - 20), msg
    for k, v in h.items():   # nothing past the emitted part of a per-frame array, nothing past the end of the others
        written = raw.size[k] if k not in S.OUT_ELEM else S.OUT_ELEM[k] * e + (4 if k == "first" else 0)
        assert np.all(v[written:] == POISON), (k, msg)


def test_send_of_more_than_one_scan_chunk(dev):
    """send_scan's second chunk, with both caps cutting in a tile >= 1024, then
    the rerun with the reported need."""
    n, tile = _send_n(), S._tiles()[0]
    rng = np.random.default_rng(0x5CA20)
    lens = rng.choice([0, 1, 40, 48, 49, 100], size=n).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    buf = rng.integers(0, 256, int(off[-1]) + int(lens[-1]) + 16, dtype=np.uint8)
    dst = rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    proto = rng.choice([6, 17, 1, 47], size=n).astype(np.uint8)
    ids = rng.integers(0, 65536, size=n).astype(np.uint16)
    l4, d_dst, d_proto, d_ids = S._dev_inputs(dev, buf, off, lens, dst, proto, ids)
    full = fast_models.send_plain(lens, dst, proto, ids, 68, S.SRC)
    need_f, need_b, prefix = full["total"]
    assert prefix == n and need_f > n
    raw = S.Raw(dev, l4, d_dst, d_proto, d_ids, room=need_f + 8)
    raw.ws.fill_(0x5A)
    _check_send(raw, raw.run(68), full, off, "no cap")
    cut = CHUNK * tile + 300                                   # the first datagram that does not fit: tile 1024
    cf = np.cumsum(np.diff(full["dgram_first"].astype(np.int64)))
    cb = cf * 20 + np.cumsum(lens.astype(np.int64))
    for max_frames, max_bytes in ((int(cf[cut]) - 1, 0xFFFFFFFF), (need_f + 8, int(cb[cut]) - 1)):
        exp = fast_models.send_plain(lens, dst, proto, ids, 68, S.SRC, max_frames, max_bytes)
        assert exp["total"] == (need_f, need_b, cut) and cut // tile >= CHUNK
        raw.ws.fill_(0x5A)
        r = raw.run(68, max_frames=max_frames, max_out_bytes=max_bytes)
        _check_send(raw, r, exp, off, f"caps {max_frames} {max_bytes}")
        got_f, got_b, _ = r.totals()
        _check_send(raw, raw.run(68, max_frames=got_f, max_out_bytes=got_b), full, off, "rerun with the need")
    del raw, l4, d_dst, d_proto, d_ids
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- the emit grid-stride

def send_plain_torch(lens, off, dst, proto, ids, mtu, src, hdr_ptr, l4_ptr) -> dict:
    """fast_models.send_plain restated in torch on the inputs' device, for
    batches whose outputs are too large to copy to the host: no cap, every
    datagram in range, (mtu - 20) % 8 == 0.  lens / off / dst / proto / ids:
    int64 tensors.  Returns dgram_first [n + 1], first [E + 1], out_off, out_len,
    hdr uint8 [E, 20] and desc int64 [E, 4] (the two records of a frame as four
    64-bit words)."""
    room = mtu - 20
    assert room % 8 == 0
    n = lens.numel()
    cut = lens + 20 > mtu
    nf = torch.where(cut, (lens + room - 1) // room, torch.ones_like(lens))
    dgram_first = torch.cat([torch.zeros(1, dtype=torch.int64, device=lens.device), torch.cumsum(nf, 0)])
    e = int(dgram_first[-1].item())
    owner = torch.repeat_interleave(torch.arange(n, device=lens.device), nf)
    k = torch.arange(e, device=lens.device) - dgram_first[owner]
    ln, c = lens[owner], cut[owner]
    o = torch.where(c, k * room, torch.zeros_like(k))
    piece = torch.where(c, torch.minimum(ln - o, torch.full_like(ln, room)), ln)
    frag = torch.where(c, torch.where(o + piece < ln, 0x2000, 0) | (o >> 3), torch.zeros_like(o))
    total_len = 20 + piece
    out_off = torch.cumsum(total_len, 0) - total_len
    d, p, ident = dst[owner], proto[owner], ids[owner]
    # RFC 1071 over the ten 16-bit words with a zero field (pinned to oracle.ip_checksum through expected_send)
    s = 0x4500 + total_len + ident + frag + ((64 << 8) | p) + (src >> 16) + (src & 0xFFFF) + (d >> 16) + (d & 0xFFFF)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    csum = ~s & 0xFFFF
    hdr = torch.empty((e, 20), dtype=torch.uint8, device=lens.device)
    cols = [0x45, 0, total_len >> 8, total_len, ident >> 8, ident, frag >> 8, frag, 64, p, csum >> 8, csum,
            src >> 24, src >> 16, src >> 8, src, d >> 24, d >> 16, d >> 8, d]
    for at, v in enumerate(cols):
        hdr[:, at] = v & 0xFF if isinstance(v, int) else (v & 0xFF).to(torch.uint8)
    f = torch.arange(e, device=lens.device)
    at32 = out_off & 0xFFFFFFFF
    desc = torch.stack([hdr_ptr + 20 * f, at32 | (20 << 32), l4_ptr + off[owner] + o,
                        ((at32 + 20) & 0xFFFFFFFF) | (piece << 32)], dim=1)
    return dict(dgram_first=dgram_first, first=2 * torch.arange(e + 1, device=lens.device), out_off=out_off,
                out_len=total_len, hdr=hdr, desc=desc, emitted=e, bytes=int((out_off[-1] + total_len[-1]).item()) if e else 0)


def _send_on_device(dev, buf, off, lens, dst, proto, ids, room):
    l4, d_dst, d_proto, d_ids = S._dev_inputs(dev, buf, off, lens, dst, proto, ids)
    raw = S.Raw(dev, l4, d_dst, d_proto, d_ids, room=room)
    raw.ws.fill_(0x5A)
    r = raw.run(68)
    as64 = [torch.from_numpy(a.astype(np.int64)).to(dev) for a in (lens, off, dst, proto, ids)]
    want = send_plain_torch(*as64, 68, S.SRC, r.hdr.data_ptr(), l4.data.data_ptr())
    return raw, r, want


def _same_on_device(raw, r, want, n, msg):
    e = want["emitted"]
    assert r.totals() == (e, want["bytes"], n), msg
    assert torch.equal(r.dgram_first.view(torch.int32).to(torch.int64) & 0xFFFFFFFF, want["dgram_first"]), msg
    assert torch.equal(r.first[: e + 1].to(torch.int64) & 0xFFFFFFFF, want["first"]), msg
    assert torch.equal(r.out_off[:e], want["out_off"]), msg
    assert torch.equal(r.out_len[:e].to(torch.int64), want["out_len"]), msg
    assert torch.equal(r.hdr[: 20 * e].view(e, 20), want["hdr"]), msg
    assert torch.equal(r.desc[: 32 * e].view(torch.int64).view(e, 4), want["desc"]), msg
    for k, t in raw.buf.items():
        written = raw.size[k] if k not in S.OUT_ELEM else S.OUT_ELEM[k] * e + (4 if k == "first" else 0)
        assert bool(torch.all(t[written:] == POISON).item()), (k, msg)


def test_send_emits_more_frames_than_the_emit_grid_has_slots(dev):
    """Past 16 384 blocks x one emit tile of frames send_emit's grid strides
    over the tiles: 12 292 datagrams of 65 515 bytes at MTU 68 (1365 frames
    each, all reading the same source bytes) and a few short ones are 1364 + a
    few frames more than that.  About 1.2 GB of outputs, compared on the device
    with send_plain_torch, which is first pinned to expected_send on L4_LENS."""
    emit_tile = S._tiles()[1]
    grid_frames = 16384 * emit_tile
    rng = np.random.default_rng(0x5CA21)
    # the restatement against the per-datagram model
    buf, off, lens, dst, proto, ids = S._datagrams(rng, rng.permutation(np.array(L4_LENS)))
    exp = expected_send(buf, off, lens, dst, proto, 68, S.SRC, ids=ids)
    e = len(exp["frames"])
    raw, r, want = _send_on_device(dev, buf, off, lens, dst, proto, ids, e + 3)
    _same_on_device(raw, r, want, lens.size, "L4_LENS")
    assert want["emitted"] == e and np.array_equal(want["hdr"].cpu().numpy().reshape(-1), exp["hdr"])
    assert np.array_equal(want["dgram_first"].cpu().numpy(), exp["dgram_first"])
    assert np.array_equal(want["out_off"].cpu().numpy(), exp["out_off"].astype(np.int64))
    assert np.array_equal(want["out_len"].cpu().numpy(), exp["out_len"])
    own = np.array([off[i] + np.uint64(o) for i, o in exp["owner"]], dtype=np.uint64)
    d = want["desc"].cpu().numpy()
    assert np.array_equal(d[:, 0], r.hdr.data_ptr() + 20 * np.arange(e))
    assert np.array_equal(d[:, 2], r.l4.data.data_ptr() + own.astype(np.int64))
    assert np.array_equal(d[:, 1], exp["out_off"].astype(np.int64) | (20 << 32))
    assert np.array_equal(d[:, 3], (exp["out_off"].astype(np.int64) + 20) | ((exp["out_len"].astype(np.int64) - 20) << 32))
    del raw, r, want
    torch.cuda.empty_cache()
    # the large batch
    big = -(-(grid_frames + emit_tile + 1) // 1365)
    lens = np.full(big + 9, 65515, np.uint32)
    short = np.array([0, 3, big // 2, big // 2 + 1, big + 4, big + 5, big + 6, big + 7, big + 8])
    lens[short] = [49, 0, 100, 1, 48, 0, 49, 100, 7]
    n = lens.size
    off = np.where(lens == 65515, 0, rng.integers(0, 60000, n)).astype(np.uint64)
    buf = rng.integers(0, 256, 65515 + 16, dtype=np.uint8)
    dst = rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    proto = rng.choice([6, 17, 1, 47], size=n).astype(np.uint8)
    ids = rng.integers(0, 65536, size=n).astype(np.uint16)
    frames = int(np.where(lens + 20 > 68, -(-lens.astype(np.int64) // 48), 1).sum())
    assert grid_frames + emit_tile < frames < grid_frames + 3 * emit_tile and frames > 16777216
    raw, r, want = _send_on_device(dev, buf, off, lens, dst, proto, ids, frames + 5)
    assert want["emitted"] == frames and want["bytes"] < 2**32
    _same_on_device(raw, r, want, n, "grid-stride")
    del raw, r, want
    torch.cuda.empty_cache()
