"""Rx steering on the device (sccsum_steer_run): every packet's shard, the
per-shard counts and the STABLE partition of the packet indices, compared
byte for byte with the numpy restatement of the reference in
tests/test_steer_host.py (np.argsort(kind="stable") + np.bincount).  Every
case compares all three outputs; nothing has a tolerance."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import oracle
from seastar_amd import batch, native, synth
from test_steer_host import (DISPATCH, EINVAL, HASH2CPU, make_steer, map_grid, rand_hashes, random_map, ref_dest,
                             ref_steer, src_cpus)

pytestmark = pytest.mark.gpu

GUARD = 16  # guard words / bytes on either side of every output
NEED, REJECT = native.ST_OK, native.ST_MALFORMED | native.ST_RANGE


@functools.lru_cache(maxsize=None)
def _tile() -> int:
    return int(native.load().sccsum_steer_tile_packets())


def _status(rng, n: int, drop: float = 0.1) -> np.ndarray:
    """Status bytes of which about `drop` fail need = ST_OK / reject = MALFORMED | RANGE,
    each in one of the ways a frame can."""
    st = np.full(n, native.ST_OK | native.ST_L4_OK, dtype=np.uint8)
    st[rng.random(n) < 0.3] = native.ST_OK                      # L4 bad: not dropped by this policy
    st[rng.random(n) < 0.1] |= native.ST_IPFRAG
    r = rng.random(n)
    st[r < drop] = 0                                            # header checksum bad
    st[r < drop * 0.6] = native.ST_OK | native.ST_MALFORMED
    st[r < drop * 0.3] = native.ST_RANGE
    return st


def _guarded(dev, numel: int, dtype, fill: int):
    t = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return t, t[GUARD:GUARD + numel]


def _guards_intact(t, numel: int, fill: int) -> bool:
    h = t.cpu().numpy()
    return bool(np.all(h[:GUARD] == fill) and np.all(h[GUARD + numel:] == fill))


def _run_and_check(dev, steer, m, h, st=None, need=0, reject=0, mode=HASH2CPU, src=0, want_cpu=True, want_order=True,
                   msg="", ws_after=None):
    """One run into guarded outputs, compared with the restatement; returns the host copies.
    A list given as `ws_after` gets the workspace's bytes as the run left them."""
    n = int(h.size)
    ncpu = m["ncpu"]
    d_h = torch.from_numpy(h.view(np.int32).copy()).to(dev)
    d_st = None if st is None else torch.from_numpy(st.copy()).to(dev)
    cpu_all, cpu = _guarded(dev, n, torch.uint8, 0xA5) if want_cpu else (None, None)
    ord_all, order = _guarded(dev, n, torch.int32, -7) if want_order else (None, None)
    first_all, first = _guarded(dev, ncpu + 2, torch.int32, -7)
    wsb = steer.workspace_bytes(n)
    ws_all, ws = _guarded(dev, wsb, torch.uint8, 0x5A)
    assert ws.data_ptr() % 16 == 0
    g_cpu, g_order, g_first = steer.run(d_h, d_st, need=need, reject=reject, mode=mode, src_cpu=src, cpu=cpu,
                                        order=order, first=first, workspace=ws, want_cpu=want_cpu,
                                        want_order=want_order)
    torch.cuda.synchronize()
    w_cpu, w_order, w_first = ref_steer(m, mode, src, h, st, need, reject)
    got_first = g_first.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_first, w_first), (msg, got_first, w_first)
    assert int(got_first[-1]) == n
    assert _guards_intact(first_all, ncpu + 2, -7), msg
    assert _guards_intact(ws_all, wsb, 0x5A), msg
    if ws_after is not None:
        ws_after.append(ws.cpu().numpy())
    got_cpu = got_order = None
    if want_cpu:
        got_cpu = g_cpu.cpu().numpy()
        assert np.array_equal(got_cpu, w_cpu), msg
        assert _guards_intact(cpu_all, n, 0xA5), msg
    else:
        assert g_cpu is None
    if want_order:
        got_order = g_order.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_order, w_order), msg
        assert _guards_intact(ord_all, n, -7), msg
    else:
        assert g_order is None
    return got_cpu, got_order, got_first


@pytest.fixture(scope="module")
def map16():
    m = random_map(np.random.default_rng(16), 16, 8, 128, 7, unset=False)
    assert set(np.unique(m["reta"])) == set(range(16))
    return m


@pytest.fixture(scope="module")
def steer16(dev, map16):
    s = make_steer(map16)
    yield s
    s.close()


def _sizes():
    t = _tile()
    return [0, 1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17, 300007]


@pytest.mark.parametrize("k", range(10))
def test_sizes(dev, steer16, map16, k):
    n = _sizes()[k]
    rng = np.random.default_rng(100 + k)
    h = rand_hashes(rng, n)
    st = _status(rng, n)
    cpu, _, first = _run_and_check(dev, steer16, map16, h, st, NEED, REJECT, msg=f"n={n}")
    if n > 1000:
        assert first[17] - first[16] > 0 and np.count_nonzero(cpu == 0xFF) == first[17] - first[16]


def test_tile_getter_is_what_the_workspace_is_sized_by(dev, steer16):
    t = _tile()
    per_tile = 4 * 17
    assert steer16.workspace_bytes(0) >= 16
    for n in (1, t, t + 1, 4 * t, 4 * t + 1, 300007):
        tiles = -(-n // t)
        w = steer16.workspace_bytes(n)
        assert w % 16 == 0 and per_tile * tiles <= w <= per_tile * (tiles + 3) + 1024  # + the bucket totals


def test_ncpu_1(dev):
    rng = np.random.default_rng(1)
    m = random_map(rng, 1, 3, 0, 0, unset=False)
    s = make_steer(m)
    n = _tile() + 65
    _run_and_check(dev, s, m, rand_hashes(rng, n), _status(rng, n), NEED, REJECT)
    _run_and_check(dev, s, m, rand_hashes(rng, n))
    s.close()


@pytest.mark.parametrize("ncpu", [31, 32])
def test_either_side_of_the_one_block_scan(dev, ncpu):
    """Up to 32 buckets (31 shards + the dropped) one block scans the counts;
    past that a block per bucket and a launch for the totals."""
    rng = np.random.default_rng(ncpu)
    m = random_map(rng, ncpu, 3, 0, 5, unset=False)
    s = make_steer(m)
    for n in (1, 3 * _tile() + 17):
        _run_and_check(dev, s, m, rand_hashes(rng, n), _status(rng, n), NEED, REJECT)
    _run_and_check(dev, s, m, rand_hashes(rng, 0))
    s.close()


@pytest.mark.parametrize("ncpu", [1, 31, 32, 255])
@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_tile_edge_on_either_scan_path(dev, ncpu, n):
    """One packet short of a tile, a whole tile, one packet into the second,
    with and without a status array, at 1, 31, 32 and 255 shards.  32 buckets
    (31 shards + the dropped) is the last case of the one-block scan, 33 the
    first that takes a block per bucket and a launch for the totals; that
    path leaves the bucket totals behind the workspace's rows of per-tile
    counts and the one-block scan leaves those bytes alone, which pins the
    switch."""
    assert _tile() == 2048
    rng = np.random.default_rng(1000 * ncpu + n)
    m = random_map(rng, ncpu, 3, 0, 5, unset=False)
    s = make_steer(m)
    tiles = -(-n // _tile())
    at = 4 * (ncpu + 1) * ((tiles + 3) & ~3)  # the rows [ncpu + 1][pitch] of 32-bit counts
    for st in (_status(rng, n), None):
        ws = []
        _, _, first = _run_and_check(dev, s, m, rand_hashes(rng, n), st, NEED if st is not None else 0,
                                     REJECT if st is not None else 0, msg=f"ncpu={ncpu} n={n}", ws_after=ws)
        behind = ws[0][at:at + 4 * (ncpu + 1)]
        if ncpu + 1 <= 32:
            assert np.all(behind == 0x5A)
        else:
            assert np.array_equal(behind.view(np.uint32), np.diff(first))
    s.close()


def test_ncpu_255_most_buckets_of_a_wave_distinct(dev):
    rng = np.random.default_rng(255)
    m = random_map(rng, 255, 256, 512, 9, unset=False)
    s = make_steer(m)
    n = 3 * _tile() + 17
    h = rand_hashes(rng, n)
    cpu, _, first = _run_and_check(dev, s, m, h, _status(rng, n), NEED, REJECT)
    assert np.unique(cpu[:64]).size > 40
    assert np.count_nonzero(np.diff(first.astype(np.int64)) > 0) > 250
    s.close()


@pytest.mark.parametrize("ncpu", [16, 255])
def test_more_tiles_than_one_scan_chunk(dev, ncpu):
    """The scan kernel takes a bucket's tiles 256 at a time and carries the sum
    from chunk to chunk: a batch of more than 256 tiles, whose last chunk is
    partly filled, through the one-block scan (16 shards) and the per-bucket
    blocks (255)."""
    rng = np.random.default_rng(256 + ncpu)
    m = random_map(rng, ncpu, 8, 128, 3, unset=False)
    s = make_steer(m)
    n = 256 * _tile() + _tile() + 9
    _run_and_check(dev, s, m, rand_hashes(rng, n), _status(rng, n), NEED, REJECT)
    s.close()


def test_every_packet_to_one_shard_and_every_packet_dropped(dev, steer16, map16):
    rng = np.random.default_rng(7)
    n = 2 * _tile() + 5
    # one shard: a map whose tables all name shard 11, and dispatch from a queue without a _sw_reta
    m = random_map(rng, 16, 8, 0, 0, unset=False)
    m["reta"][:] = 11
    s = make_steer(m)
    cpu, order, first = _run_and_check(dev, s, m, rand_hashes(rng, n))
    assert np.all(cpu == 11) and np.array_equal(order, np.arange(n, dtype=np.uint32))
    s.close()
    m = random_map(rng, 16, 8, 0, 0, unset=True)
    s = make_steer(m)
    for src in (0, 12):  # queue 0 has no _sw_reta; 12 is a proxy queue past hw_queues
        cpu, order, _ = _run_and_check(dev, s, m, rand_hashes(rng, n), mode=DISPATCH, src=src)
        assert np.all(cpu == src)
    s.close()
    # every packet dropped: by a need bit no status has, and by a reject bit all have
    h = rand_hashes(rng, n)
    st = np.full(n, native.ST_OK, dtype=np.uint8)
    cpu, order, first = _run_and_check(dev, steer16, map16, h, st, need=native.ST_L4_OK)
    assert np.all(cpu == 0xFF) and first[16] == 0 and np.array_equal(order, np.arange(n, dtype=np.uint32))
    _run_and_check(dev, steer16, map16, h, st, reject=native.ST_OK)


def test_nothing_dropped_and_an_empty_shard(dev):
    rng = np.random.default_rng(9)
    m = random_map(rng, 16, 8, 128, 7, unset=False)
    m["reta"][m["reta"] == 5] = 6  # no table entry names shard 5
    s = make_steer(m)
    n = _tile() + 700
    cpu, order, first = _run_and_check(dev, s, m, rand_hashes(rng, n))
    assert first[5] == first[6] and first[16] == first[17] == n and 0xFF not in cpu
    cpu, order, first = _run_and_check(dev, s, m, rand_hashes(rng, n), _status(rng, n), NEED, REJECT)
    assert first[5] == first[6] and first[16] < n
    s.close()


def test_map_forms(dev):
    """Both modes over the host test's whole map grid at n = 4097."""
    rng = np.random.default_rng(4097)
    n = 4097
    h = rand_hashes(rng, n)
    st = _status(rng, n)
    count = 0
    for m in map_grid():
        s = make_steer(m)
        tag = (m["ncpu"], m["hw_queues"], m["table_bits"], None if m["redir"] is None else m["redir"].size)
        _run_and_check(dev, s, m, h, st, NEED, REJECT, mode=HASH2CPU, msg=f"hash2cpu {tag}")
        for src in src_cpus(m, rng):
            _run_and_check(dev, s, m, h, st, NEED, REJECT, mode=DISPATCH, src=src, msg=f"dispatch {src} {tag}")
        s.close()
        count += 1
    assert count == 80


def test_optional_outputs(dev, steer16, map16):
    rng = np.random.default_rng(21)
    n = _tile() + 333
    h = rand_hashes(rng, n)
    st = _status(rng, n)
    for want_cpu, want_order in itertools.product((False, True), repeat=2):
        _run_and_check(dev, steer16, map16, h, st, NEED, REJECT, want_cpu=want_cpu, want_order=want_order)


def test_two_runs_give_identical_bytes(dev, steer16, map16):
    rng = np.random.default_rng(33)
    n = 300007
    d_h = torch.from_numpy(rand_hashes(rng, n).view(np.int32).copy()).to(dev)
    d_st = torch.from_numpy(_status(rng, n)).to(dev)
    runs = []
    for _ in range(2):
        cpu, order, first = steer16.run(d_h, d_st, need=NEED, reject=REJECT)
        torch.cuda.synchronize()
        runs.append((cpu.cpu().numpy().tobytes(), order.cpu().numpy().tobytes(), first.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]


def test_capture_and_replay(dev, steer16, map16):
    """One run under torch.cuda.graph (a single chain of kernels), replayed once."""
    rng = np.random.default_rng(44)
    n = _tile() + 1
    h = rand_hashes(rng, n)
    st = _status(rng, n)
    w_cpu, w_order, w_first = ref_steer(map16, HASH2CPU, 0, h, st, NEED, REJECT)
    d_h = torch.from_numpy(h.view(np.int32).copy()).to(dev)
    d_st = torch.from_numpy(st).to(dev)
    cpu = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    order = torch.full((n,), -7, dtype=torch.int32, device=dev)
    first = torch.full((18,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(steer16.workspace_bytes(n), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        steer16.run(d_h, d_st, need=NEED, reject=REJECT, cpu=cpu, order=order, first=first, workspace=ws,
                    stream=torch.cuda.current_stream())
    cpu.fill_(0xA5)
    order.fill_(-7)
    first.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(cpu.cpu().numpy(), w_cpu)
    assert np.array_equal(order.cpu().numpy().view(np.uint32), w_order)
    assert np.array_equal(first.cpu().numpy().view(np.uint32), w_first)
    e_cpu, e_order, e_first = steer16.run(d_h, d_st, need=NEED, reject=REJECT)
    torch.cuda.synchronize()
    assert torch.equal(e_cpu, cpu) and torch.equal(e_order, order) and torch.equal(e_first, first)


def _early_return(buf, off, lens) -> np.ndarray:
    """Frames ipv4::handle_received_packet returns early on (ip.cc:115-144):
    no whole ip_hdr, a header checksum that does not verify, fewer bytes than
    the IP total length, or fragment offset + length past 65535.  A header
    longer than the datagram (4 * ihl > total length) is counted too: the
    reference has no defined behaviour for it (its trim_front(ip_hdr_len),
    ip.cc:225, would pass the packet's end) and the library reports it as
    SCCSUM_ST_MALFORMED."""
    out = np.zeros(off.size, dtype=bool)
    for i in range(off.size):
        o, L = int(off[i]), int(lens[i])
        if L < 20:
            out[i] = True
            continue
        f = buf[o:o + L]
        ip_len = (int(f[2]) << 8) | int(f[3])
        frag_off = ((((int(f[6]) << 8) | int(f[7])) & 0x1FFF) * 8)
        out[i] = (oracle.ip_checksum(f[:20]) != 0 or L < ip_len or frag_off + min(L, ip_len) > 65535
                  or 4 * (int(f[0]) & 0xF) > ip_len)
    return out


def test_end_to_end_frames_rss_then_steer(dev):
    """rss_frames with valid IPv4 header checksums, about 2 % of the headers
    corrupted afterwards: ipv4_frames_rss, then steering by its hashes and
    status, against the oracle's status and hashes sent through the
    restatement."""
    rng = np.random.default_rng(77)
    buf, off, lens = synth.rss_frames(5000, seed=31)
    for i in range(off.size):
        o, L = int(off[i]), int(lens[i])
        if L >= 20:
            buf[o + 10:o + 12] = 0
            buf[o + 10:o + 12] = np.frombuffer(np.uint16(oracle.ip_checksum(buf[o:o + 20])).tobytes(), np.uint8)
    corrupt = np.flatnonzero((rng.random(off.size) < 0.02) & (lens >= 20))
    for i in corrupt:
        buf[int(off[i]) + 8] ^= 0x10  # ttl
    want2, want_st = oracle.batch_ipv4(buf, off, lens)
    want_h, _ = oracle.batch_ipv4_rss(buf, off, lens, key=batch.RSS_KEY_40, mode=native.RSS_DISPATCH)
    ok = (want_st & native.ST_OK) != 0
    assert 0 < np.count_nonzero(~ok[corrupt]) == corrupt.size and np.count_nonzero(ok) > 2000
    m = random_map(rng, 12, 4, 128, 0, unset=False)
    m["reta"][:] = np.stack([batch.build_reta({c: 1.0 + (c + q) % 3 for c in range(12)}) for q in range(4)])
    w_cpu, w_order, w_first = ref_steer(m, HASH2CPU, 0, want_h, want_st, NEED, REJECT)

    b = batch.PacketBatch.from_host(buf, off, lens, device=dev)
    st = torch.empty(b.n, dtype=torch.uint8, device=dev)
    out2, hashes = batch.ipv4_frames_rss(b, key=batch.RSS_KEY_40, mode=native.RSS_DISPATCH, status=st)
    s = make_steer(m)
    cpu, order, first = s.run(hashes, st, need=NEED, reject=REJECT, mode=HASH2CPU)
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), want_st)
    cpu, order, first = cpu.cpu().numpy(), order.cpu().numpy().view(np.uint32), first.cpu().numpy().view(np.uint32)
    assert np.array_equal(cpu, w_cpu)
    assert np.array_equal(first, w_first)
    assert np.array_equal(order, w_order)
    dropped = order[first[12]:first[13]]
    early = _early_return(buf, off, lens)
    assert dropped.size > corrupt.size and np.all(early[dropped])
    assert np.array_equal(np.sort(dropped), np.flatnonzero(early))  # and nothing the reference keeps is dropped
    kept = np.flatnonzero(~early)
    assert np.array_equal(cpu[kept], ref_dest(m, HASH2CPU, 0, want_h[kept]).astype(np.uint8))
    s.close()


@pytest.mark.parametrize("case", range(24))
def test_seeded_fuzz(dev, case):
    rng = np.random.default_rng(9000 + case)
    ncpu = int(rng.choice([1, 2, 3, 8, 16, 31, 64, 100, 200, 255]))
    hwq = int(rng.choice([1, 2, 3, 8, 16, 64, 255, 256]))
    rs = int(rng.choice([0, 0, 1, 2, 64, 128, 512]))
    m = random_map(rng, ncpu, hwq, rs, int(rng.integers(0, 32)), unset=bool(rng.integers(0, 2)))
    n = int(rng.integers(0, 20001))
    h = rand_hashes(rng, n)
    if rng.random() < 0.2:
        h[rng.random(n) < 0.5] = 0  # what unhashable frames get
    mode = int(rng.integers(0, 2))
    src = int(rng.choice(src_cpus(m, rng))) if mode == DISPATCH else int(rng.integers(0, 1 << 32))
    st, need, reject = None, 0, 0
    if rng.random() < 0.75:
        st = rng.integers(0, 32, size=n, dtype=np.int64).astype(np.uint8)
        need, reject = int(rng.integers(0, 4)), int(rng.integers(0, 32)) & ~3
    s = make_steer(m)
    _run_and_check(dev, s, m, h, st, need, reject, mode=mode, src=src,
                   msg=f"case {case}: ncpu {ncpu} hwq {hwq} redir {rs} bits {m['table_bits']} mode {mode} n {n}")
    s.close()


def test_run_argument_errors_on_a_real_object(dev, steer16):
    """The argument errors of tests/test_steer_host.py on an object that exists:
    each is SCCSUM_EINVAL and no output is touched."""
    lib = native.load()
    n = 256
    d_h = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    order = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    first = torch.full((19,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(steer16.workspace_bytes(n) + 16, dtype=torch.uint8, device=dev)
    H, S, O, F, W = (t.data_ptr() for t in (d_h, d_st, order, first, ws))
    stream = torch.cuda.current_stream().cuda_stream
    h = steer16._h

    def run(mode=HASH2CPU, src=0, dh=H, st=None, need=0, reject=0, nn=n, cpu=None, o=O, f=F, w=W):
        return lib.sccsum_steer_run(h, mode, src, dh, st, need, reject, nn, cpu, o, f, w, stream)

    assert run(st=None, need=1) == EINVAL and run(st=None, reject=4) == EINVAL
    assert run(f=None) == EINVAL
    assert run(dh=None) == EINVAL and run(w=None) == EINVAL
    assert run(dh=H + 2) == EINVAL and run(o=O + 2) == EINVAL and run(f=F + 2) == EINVAL and run(w=W + 8) == EINVAL
    assert run(nn=1 << 32) == EINVAL
    assert run(mode=2) == EINVAL and run(mode=-1) == EINVAL
    assert run(mode=DISPATCH, src=16) == EINVAL  # a proxy queue that is no shard
    assert run(nn=0, f=None) == 0
    torch.cuda.synchronize()
    assert torch.all(order == -7) and torch.all(first == -7)
    assert run(st=S, need=1, o=None) == 0  # counts only
    torch.cuda.synchronize()
    got = first.cpu().numpy()
    assert got[16] == 0 and got[17] == n and got[18] == -7 and torch.all(order == -7)
    if torch.cuda.device_count() > 1:
        other = torch.cuda.Stream(device=1)
        assert lib.sccsum_steer_run(h, HASH2CPU, 0, H, None, 0, 0, n, None, O, F, W, other.cuda_stream) == EINVAL
    assert ctypes.sizeof(native.SteerMap) == 40
