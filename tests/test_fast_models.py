"""tests/fast_models.py pinned to the per-record models on inputs small enough
for them: reasm_plain to reasm_model.buckets + reasm_model.run (through
test_gpu_reasm._expect), send_plain to test_send_host.expected_send,
frag_records_plain to test_gpu_reasm._expected_records.  No device needed."""
import numpy as np
import pytest

import fast_models
import oracle
from seastar_amd import batch, native
from test_gpu_reasm import HOST, _expect, _expected_records, _pack_frames, _rx_frames
from test_gpu_send import SRC, _datagrams
from test_reasm_host import key_mix
from test_send_host import L4_LENS, expected_send


def test_the_layouts_and_constants_are_the_interface_s():
    assert fast_models.REC_DTYPE == batch.REC_DTYPE and fast_models.DESC_DTYPE == batch.DESC_DTYPE
    assert (fast_models.COMPLETE, fast_models.PENDING, fast_models.HOST) == \
        (native.REASM_COMPLETE, native.REASM_PENDING, native.REASM_HOST)
    assert fast_models.ST_OK == native.ST_OK


def test_key_mix_and_seeds_match_the_scalar_forms():
    rng = np.random.Generator(np.random.PCG64(1))
    n = 400
    src = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    dst = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    ident = rng.integers(0, 65536, n).astype(np.uint32)
    proto = rng.choice([6, 17, 1, 255], n).astype(np.uint32)
    length = rng.integers(0, 70000, n).astype(np.uint32)
    src[:3], dst[:3], length[:3] = (0xFFFFFFFF, 0, 0xFFFF0000), (0xFFFFFFFF, 0, 0xFFFF), (0xFFFF, 0, 0)
    mix = fast_models.key_mix(src, dst, ident, proto)
    seeds = fast_models.pseudo_seeds(src, dst, proto, length)
    for i in range(n):
        k = (int(src[i]), int(dst[i]), int(ident[i]), int(proto[i]))
        assert int(mix[i]) == key_mix(*k)
        want = oracle.pseudo_seed(k[0], k[1], k[3], int(length[i])) if k[3] in (6, 17) else 0
        assert int(seeds[i]) == want, (k, int(length[i]))


def slow_reasm_outputs(recs, st, emitted) -> dict:
    """What test_gpu_reasm._check compares a run with, as arrays."""
    D = len(emitted)
    cnt = [len(d.pieces) for d in emitted]
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum([d.length for d in emitted])]).astype(np.uint64)[:D]
    desc = np.zeros(int(first[-1]), batch.DESC_DTYPE)
    k = 0
    for d, o in zip(emitted, off):
        pos = 0
        for r, frm, ln in d.pieces:
            desc[k] = (int(recs[r]["frame"]) + int(recs[r]["hdr_len"]) + frm, (int(o) + pos) & 0xFFFFFFFF, ln)
            pos += ln
            k += 1
    seeds = [oracle.pseudo_seed(d.key[0], d.key[1], d.key[3], d.length) if d.key[3] in (6, 17) else 0 for d in emitted]
    pend, host = recs[st == native.REASM_PENDING], recs[st == native.REASM_HOST]
    return dict(state=st, first=first, off=off, len=np.array([d.length for d in emitted], np.uint32),
                head=np.array([d.head for d in emitted], np.uint32), last=np.array([d.last for d in emitted], np.uint32),
                seed=np.array(seeds, np.uint32), desc=desc, pending=pend, host=host,
                total=(D, int(first[-1]), pend.size, host.size))


def _colliding_keys(rng):
    """Two distinct keys of one mix, found among 2^18 random ones."""
    n = 1 << 18
    src = rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    dst = rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    ident = rng.integers(0, 65536, n).astype(np.uint32)
    mix = fast_models.key_mix(src, dst, ident, np.full(n, 17, np.uint32))
    order = np.argsort(mix, kind="stable")
    same = np.flatnonzero(mix[order][1:] == mix[order][:-1])
    assert same.size
    a, b = int(order[same[0]]), int(order[same[0] + 1])
    return [(int(src[i]), int(dst[i]), int(ident[i])) for i in (a, b)]


@pytest.fixture(scope="module")
def small_records():
    rng = np.random.Generator(np.random.PCG64(0xFA57))
    recs, _ = fast_models.plain_udp_records(rng, 3000)
    recs["frame"] += np.uint64(0x7F0000000000)
    # two complete keys of several pieces get the addresses and ids of a colliding pair
    tags, counts = np.unique(recs["tag"], return_counts=True)
    full = [int(t) for t, c in zip(tags, counts) if c in (3, 5) and
            not recs["mf"][(recs["tag"] == t)][np.argmax(recs["offset"][recs["tag"] == t])]][:2]
    for t, (s, d, i) in zip(full, _colliding_keys(rng)):
        mine = recs["tag"] == t
        recs["src"][mine], recs["dst"][mine], recs["id"][mine] = s, d, i
    return recs, full


def _same(fast, slow, msg):
    assert fast["total"] == slow["total"], msg
    for name in ("state", "first", "off", "len", "head", "last", "seed"):
        assert fast[name].dtype == slow[name].dtype and np.array_equal(fast[name], slow[name]), (name, msg)
    for name in ("desc", "pending", "host"):
        assert fast[name].tobytes() == slow[name].tobytes(), (name, msg)


def test_reasm_plain_is_the_slow_model_on_3000_records(small_records):
    recs, pair = small_records
    st, emitted = _expect(recs, collisions=True)
    assert np.all(st[np.isin(recs["tag"], pair)] == native.REASM_HOST)
    assert np.count_nonzero(st == native.REASM_HOST) in (6, 8, 10)       # the pair, nobody else
    assert np.count_nonzero(st == native.REASM_PENDING) > 100 and len(emitted) > 500
    fast = fast_models.reasm_plain(recs)
    _same(fast, slow_reasm_outputs(recs, st, emitted), "no cap")
    assert np.array_equal(fast["rows"], [r for d in emitted for r, _, _ in d.pieces])
    # grouped by the full key alone the pair is delivered
    alone = fast_models.reasm_plain(recs, mix=None)
    assert alone["total"][3] == 0 and alone["total"][0] == len(emitted) + 2


def test_reasm_plain_applies_the_cap_as_the_slow_model_does(small_records):
    recs, _ = small_records
    _, every = _expect(recs, collisions=True)
    sums = np.cumsum([d.length for d in every])
    for cap, want in ((int(sums[400]), 401), (int(sums[400]) - 1, 400), (int(sums[-1]), len(every)),
                      (int(sums[-1]) - 1, len(every) - 1), (every[0].length - 1, 0), (0, 0)):
        st, emitted = _expect(recs, cap=cap, collisions=True)
        assert len(emitted) == want
        _same(fast_models.reasm_plain(recs, cap=cap), slow_reasm_outputs(recs, st, emitted), f"cap {cap}")


def test_reasm_plain_refuses_keys_that_are_not_plain():
    recs = np.zeros(2, fast_models.REC_DTYPE)
    recs["src"], recs["proto"], recs["mf"], recs["len"] = 5, 17, (1, 0), 16
    recs["offset"] = (0, 8)                                              # an overlap
    with pytest.raises(AssertionError, match="not plain"):
        fast_models.reasm_plain(recs)
    recs["offset"], recs["mf"] = (0, 16), (0, 1)                         # a record after the MF-clear one
    with pytest.raises(AssertionError, match="not plain"):
        fast_models.reasm_plain(recs)
    recs["mf"], recs["len"] = (1, 0), (16, 0)                            # an empty piece
    with pytest.raises(AssertionError, match="not plain"):
        fast_models.reasm_plain(recs)
    assert fast_models.reasm_plain(recs[:0])["total"] == (0, 0, 0, 0)


@pytest.mark.parametrize("mtu", [68, 1500])
def test_send_plain_is_expected_send(mtu):
    rng = np.random.default_rng(0xFA58 + mtu)
    lens = rng.permutation(np.array(L4_LENS))
    buf, off, lens, dst, proto, ids = _datagrams(rng, lens, protos=rng.permutation(np.resize([6, 17, 1, 47], lens.size)))
    full = expected_send(buf, off, lens, dst, proto, mtu, SRC, ids=ids)
    need_f, need_b, _ = full["total"]
    mid = int(full["dgram_first"][lens.size // 2])
    caps = [(0x7FFFFFFF, 0xFFFFFFFF), (need_f, need_b), (need_f - 1, 0xFFFFFFFF), (need_f, need_b - 1),
            (mid, 0xFFFFFFFF), (mid + 1, 0xFFFFFFFF), (need_f, int(full["out_off"][mid])),
            (need_f, int(full["out_off"][mid]) - 1), (0, 0xFFFFFFFF), (need_f, 0)]
    prefixes = set()
    for max_frames, max_bytes in caps:
        exp = expected_send(buf, off, lens, dst, proto, mtu, SRC, ids=ids, max_frames=max_frames, max_out_bytes=max_bytes)
        got = fast_models.send_plain(lens, dst, proto, ids, mtu, SRC, max_frames, max_bytes)
        msg = f"caps {max_frames} {max_bytes}"
        assert got["total"] == exp["total"] and got["emitted"] == len(exp["frames"]), msg
        for name in ("dgram_first", "status", "first", "out_off", "out_len"):
            assert got[name].dtype == exp[name].dtype and np.array_equal(got[name], exp[name]), (name, msg)
        assert np.array_equal(got["hdr"].reshape(-1), exp["hdr"]), msg
        assert list(zip(got["owner"].tolist(), got["piece_off"].tolist())) == exp["owner"], msg
        prefixes.add(exp["total"][2])
    assert len(prefixes) >= 5 and lens.size in prefixes and 0 in prefixes


def test_frag_records_plain_is_expected_records():
    rng = np.random.Generator(np.random.PCG64(0xFA59))
    frames = _rx_frames(rng, 1500)
    buf, offs, lens = _pack_frames(rng, frames)
    _, status = oracle.batch_ipv4(buf, offs, lens)
    width = max(int(lens.max()), 20)
    f2 = np.zeros((len(frames), width), np.uint8)
    for i, f in enumerate(frames):
        f2[i, : f.size] = f
    base = 0x7F1200000000
    want = _expected_records(frames, offs, base, 0xBEEF)
    assert 200 < want.size < 1200
    got, by_status, by_header = fast_models.frag_records_plain(f2, offs, lens, status, batch.FRAG_NEED,
                                                               batch.FRAG_REJECT, HOST, base, 0xBEEF)
    assert got.tobytes() == want.tobytes()
    # each of the two masks decides on its own: frames the status passes and the header refuses (another
    # host's), and the reverse (whole datagrams, wrong checksums)
    assert np.any(by_status & ~by_header) and np.any(by_header & ~by_status)
    # masks of 0 leave the header rules alone
    every, s0, h0 = fast_models.frag_records_plain(f2, offs, lens, status, 0, 0, HOST, base, 0xBEEF)
    assert np.all(s0) and np.array_equal(h0, by_header) and every.size == np.count_nonzero(by_header)
    # host 0 accepts every destination
    anyone, _, h1 = fast_models.frag_records_plain(f2, offs, lens, status, batch.FRAG_NEED, batch.FRAG_REJECT, 0, base, 1)
    assert anyone.size > want.size and set(anyone["dst"].tolist()) == {HOST, HOST ^ 0x100}
