"""Offsets and lengths past 2^31 / 2^32 in every entry point, against the oracle.

The C-ABI takes uint64_t bytes_len / d_off[], uint32_t d_len[] and absolute
64-bit src pointers in descriptors; the kernels split pointers into 32-bit
halves for readlane, re-base buffer resources with 32-bit extents and carry
some byte ranges as int.  Three parts:

  A  a 1 MiB buffer whose offset array holds, as every fourth entry, an ALIAS
     of a valid packet (k, L): k + 2^31, k + 2^32, k + 2^33, k + 2^63,
     k + 2^64 - 2^32, 2^64 - L, 2^64 - L + 1, 2^64 - 1 — offsets whose low 32
     bits, or whose wrapped end, look valid.  Each must give 0 +
     SCCSUM_ST_RANGE (RSS hash 0, nothing written), each valid entry exactly
     the oracle's value.  (For the descriptor calls k + 2^31 fits dst_off: it
     is a legitimate layout coordinate there, so those tests use the other
     seven.)
  B  one device buffer of W = 2^32 + 2^26 bytes with ~400 packets in six
     clusters: at offset 0, straddling offset 2^31, straddling offset 2^32,
     above 2^32, ending exactly at W, and straddling the absolute address in
     the buffer that is a multiple of 2^32.
  C  lengths at the 32-bit edges in the same buffer: frames whose d_len is
     2^31 - 1 .. 2^32 - 1 (their L4 range stays <= 65 535 B), and spans of
     2^31 - 1, 2^31, 2^31 + 1 and 2^32 - 1 bytes next to short ones.

The checker is the oracle on a compact host image (the same bytes at small
host offsets; the multi-GiB spans on the module's one host copy of the
buffer).  Every packet of every case is compared.

The stack layers that came later (steer, ipv4_send, reassembly, Ethernet,
UDP, TCP, tcp_rx_data, tcp_tx_data) see frames at such offsets in
tests/test_gpu_wide_stack.py, laid out by tests/wide_layout.py.

Not covered, here or there: a buffer crossing a 64 GiB-aligned address (the
wrap of the 16-byte unit index the flat kernel re-bases its buffer resources
with); a test cannot choose where an allocation lands.  A packed output of
more than 4 GiB: dst_off is 32-bit by contract.  Host pipelines and burst queues over
more than 4 GiB of host memory are out of scope (their offset checks are in
part A; burst batches are 32-bit by contract).
"""
import bisect
import contextlib
import types

import numpy as np
import pytest
import torch

import oracle
from seastar_amd import batch, devsynth, native, pipeline
from test_gpu_parity import FILL_MODES, _tx_frames

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
P31, P32 = 1 << 31, 1 << 32
T = 1 << 20
W = P32 + (1 << 26)
CAP = 65536 + 64  # a frame's bytes any entry point may touch: 4 * ihl + its L4 range <= 65 535
MODES = ["ip_l4_icmp_echo", "ip_pseudo_tso"]


@pytest.fixture(params=[0, 1, 2, 15, 16], ids=["default", "simple", "rows", "flat8_pipe", "flat16"])
def kernel_form(request, dev):
    """The default pick and each kernel family forced (in-place fills run the
    flat kernel whatever the form)."""
    lib = native.load()
    native.check(lib.sccsum_set_kernel_variant(request.param), "set variant")
    yield request.param
    native.check(lib.sccsum_set_kernel_variant(0), "reset variant")


def _t(a, dtype=None):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:  # torch takes the signed view
        a = a.view(a.dtype.str.replace("u", "i"))
    t = torch.from_numpy(a)
    return (t if dtype is None else t.view(dtype)).to("cuda:0")


def _pb(data, bytes_len, off, length, max_len):
    """A PacketBatch straight from device tensors (from_host would copy the buffer)."""
    return batch.PacketBatch(data=data, off=_t(np.asarray(off, np.uint64), torch.int64),
                             length=_t(np.asarray(length, np.uint32), torch.int32), bytes_len=bytes_len,
                             max_len=int(max_len))


def _marked(n, dtype, dev):
    """An output array no kernel result equals by accident: every element must be written."""
    return torch.full((max(n, 1),), 0x5A if dtype == torch.uint8 else 0x5A5A, dtype=dtype, device=dev)


def _u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ part A

ALIAS_KINDS = ["k+2^31", "k+2^32", "k+2^33", "k+2^63", "k+2^64-2^32", "2^64-L", "2^64-L+1", "2^64-1"]


def _alias(kind, k, L):
    return [k + P31, k + P32, k + (1 << 33), k + (1 << 63), k + (1 << 64) - P32, (1 << 64) - L, (1 << 64) - L + 1,
            (1 << 64) - 1][kind] & M64


def _alias_entries(off, length, kinds):
    """The packets with an alias of a valid packet (>= 20 B) after every third
    one: every fourth entry, inside the same 64-packet tiles and row groups."""
    e_off, e_len, e_src, e_kind = [], [], [], []
    na = 0
    for i in range(off.size):
        e_off.append(int(off[i]))
        e_len.append(int(length[i]))
        e_src.append(i)
        e_kind.append(-1)
        if i % 3 == 2:
            j = i
            while length[j] < 20:
                j -= 1
            kind = kinds[na % len(kinds)]
            na += 1
            e_off.append(_alias(kind, int(off[j]), int(length[j])))
            e_len.append(int(length[j]))
            e_src.append(j)
            e_kind.append(kind)
    E = types.SimpleNamespace(off=np.array(e_off, np.uint64), length=np.array(e_len, np.uint32),
                              src=np.array(e_src), kind=np.array(e_kind))
    E.valid = E.kind < 0
    E.n = E.off.size
    return E


def _assert_aliases(E, kinds, T_):
    """Every alias kind is present, every fourth entry is one, and each is out
    of range although its low 32 bits or its wrapped end are not."""
    assert np.array_equal(np.nonzero(~E.valid)[0] % 4, np.full(int((~E.valid).sum()), 3))
    for kind in kinds:
        idx = np.nonzero(E.kind == kind)[0]
        assert idx.size >= 8, (ALIAS_KINDS[kind], idx.size)
        for i in idx:
            o, L = int(E.off[i]), int(E.length[i])
            assert o > T_ or L > T_ - o  # out of range as the contract states it
            # and in range once truncated to 31 / 32 bits, or once its end wraps
            assert (o & 0x7FFFFFFF) + L <= T_ or (o & 0xFFFFFFFF) + L <= T_ or ((o + L) & M64) <= T_


@pytest.fixture(scope="module")
def small(dev):
    rng = np.random.default_rng(0xA11A5)
    buf, off, length = _tx_frames(rng, 256)
    assert buf.size < T
    buf = np.concatenate([buf, rng.integers(0, 256, size=T - buf.size, dtype=np.uint8)])
    s = types.SimpleNamespace(buf=buf, off=off, length=length, max_len=int(length.max()))
    s.E = _alias_entries(off, length, list(range(8)))
    s.D = _alias_entries(off, length, list(range(1, 8)))  # the descriptor calls
    s.seeds = rng.integers(0, 1 << 32, size=off.size, dtype=np.uint64).astype(np.uint32)
    s.want_spans = oracle.batch_spans(buf, off, length)
    s.want_seeded = oracle.batch_spans(buf, off, length, s.seeds)
    s.want2, s.want_st = oracle.batch_ipv4(buf, off, length)
    s.want_h, s.want_hst = oracle.batch_ipv4_rss(buf, off, length)
    s.fill = {m: oracle.batch_ipv4_fill(buf, off, length, FILL_MODES[m]) for m in MODES}
    s.d_data = torch.from_numpy(buf).to(dev)
    return s


def _check_spans(E, got, st, want):
    v = E.valid
    assert np.array_equal(got[v], want)
    assert np.array_equal(st[v], (want == 0).astype(np.uint8))
    assert np.all(got[~v] == 0) and np.all(st[~v] == native.ST_RANGE)


def _check_frames(E, got2, st, want2, want_st):
    v = E.valid
    if got2 is not None:
        assert np.array_equal(got2[v], want2)
        assert np.all(got2[~v] == 0)
    assert np.array_equal(st[v], want_st)
    assert np.all(st[~v] == native.ST_RANGE)


@pytest.mark.parametrize("seeded", [False, True], ids=["plain", "seeded"])
def test_alias_spans(dev, small, kernel_form, seeded):
    s, E = small, small.E
    _assert_aliases(E, range(8), T)
    b = _pb(s.d_data, T, E.off, E.length, s.max_len)
    out, st = _marked(E.n, torch.int16, dev), _marked(E.n, torch.uint8, dev)
    batch.spans(b, seeds=_t(s.seeds[E.src], torch.int32) if seeded else None, out=out, status=st)
    torch.cuda.synchronize()
    _check_spans(E, batch.as_u16(out), st.cpu().numpy(), s.want_seeded if seeded else s.want_spans)


@pytest.mark.parametrize("outputs", ["both", "status_alone"])
def test_alias_frames(dev, small, kernel_form, outputs):
    s, E = small, small.E
    _assert_aliases(E, range(8), T)
    b = _pb(s.d_data, T, E.off, E.length, s.max_len)
    st = _marked(E.n, torch.uint8, dev)
    got2 = None
    if outputs == "both":
        out2 = _marked(2 * E.n, torch.int16, dev)
        batch.ipv4_frames(b, out2=out2, status=st)
        torch.cuda.synchronize()
        got2 = batch.as_u16(out2).reshape(-1, 2)
    else:
        batch.verify_frames(b, st)
        torch.cuda.synchronize()
    _check_frames(E, got2, st.cpu().numpy(), s.want2, s.want_st)


def test_alias_multi(dev, small, kernel_form):
    """Two batches of this kind in one launch: the default pick takes the row
    kernel's several-batch form (<= 65 536 packets in total), the flat forms
    the flat kernel's queues, the per-packet forms one launch per batch."""
    s, E = small, small.E
    _assert_aliases(E, range(8), T)
    cut = (E.n // 2) | 1
    parts = [slice(0, cut), slice(cut, E.n)]
    bs = [_pb(s.d_data, T, E.off[p], E.length[p], s.max_len) for p in parts]
    sts = [_marked(b.n, torch.uint8, dev) for b in bs]
    outs = [_marked(2 * b.n, torch.int16, dev) for b in bs]
    batch.ipv4_frames_multi([(b, o, t) for b, o, t in zip(bs, outs, sts)])
    torch.cuda.synchronize()
    got2 = np.concatenate([batch.as_u16(o).reshape(-1, 2) for o in outs])
    _check_frames(E, got2, np.concatenate([t.cpu().numpy() for t in sts]), s.want2, s.want_st)
    sts = [_marked(b.n, torch.uint8, dev) for b in bs]
    outs = [_marked(b.n, torch.int16, dev) for b in bs]
    batch.spans_multi([(b, o, t, _t(s.seeds[E.src[p]], torch.int32)) for b, o, t, p in zip(bs, outs, sts, parts)])
    torch.cuda.synchronize()
    _check_spans(E, np.concatenate([batch.as_u16(o) for o in outs]), np.concatenate([t.cpu().numpy() for t in sts]),
                 s.want_seeded)


@pytest.mark.parametrize("mode", MODES)
def test_alias_fill(dev, small, kernel_form, fill_passes, mode):
    """The whole buffer is byte-identical to the oracle's fill of the valid entries alone."""
    s, E = small, small.E
    _assert_aliases(E, range(8), T)
    d = s.d_data.clone()
    b = _pb(d, T, E.off, E.length, s.max_len)
    out2, st = _marked(2 * E.n, torch.int16, dev), _marked(E.n, torch.uint8, dev)
    batch.ipv4_fill(b, FILL_MODES[mode], out2=out2, status=st)
    torch.cuda.synchronize()
    want_buf, want2, want_st = s.fill[mode]
    _check_frames(E, batch.as_u16(out2).reshape(-1, 2), st.cpu().numpy(), want2, want_st)
    bad = np.nonzero(d.cpu().numpy() != want_buf)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"


def test_alias_rss(dev, small, kernel_form):
    s, E = small, small.E
    _assert_aliases(E, range(8), T)
    v = E.valid
    b = _pb(s.d_data, T, E.off, E.length, s.max_len)
    st, h = _marked(E.n, torch.uint8, dev), _marked(E.n, torch.int32, dev)
    batch.ipv4_rss(b, hash_out=h, status=st)
    torch.cuda.synchronize()
    stn = st.cpu().numpy()
    assert np.array_equal(_u32(h)[v], s.want_h) and np.all(_u32(h)[~v] == 0)
    assert np.array_equal(stn[v] & native.ST_MALFORMED, s.want_hst & native.ST_MALFORMED)
    assert np.all((stn[v] & native.ST_RANGE) == 0) and np.all(stn[~v] == native.ST_RANGE)
    st, h, out2 = _marked(E.n, torch.uint8, dev), _marked(E.n, torch.int32, dev), _marked(2 * E.n, torch.int16, dev)
    batch.ipv4_frames_rss(b, out2=out2, status=st, hash_out=h)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(h)[v], s.want_h) and np.all(_u32(h)[~v] == 0)
    _check_frames(E, batch.as_u16(out2).reshape(-1, 2), st.cpu().numpy(), s.want2, s.want_st)


def _cut_fragments(rng, off, length, nmax=3):
    """Each packet as 1..nmax fragments (odd cuts; an empty packet is one
    empty fragment); returns the fragments' offsets and lengths and first[]."""
    f_off, f_len, first = [], [], [0]
    for o, L in zip(off.tolist(), length.tolist()):
        if L == 0:
            f_off.append(o), f_len.append(0)
        k = int(rng.integers(0, nmax)) if L >= 2 else 0
        edges = [0, *sorted(set(int(c) for c in rng.integers(1, max(L, 2), size=k))), L]
        for a, b_ in zip(edges[:-1], edges[1:]):
            if b_ > a:
                f_off.append(o + a)
                f_len.append(b_ - a)
        first.append(len(f_off))
    return np.array(f_off, np.uint64), np.array(f_len, np.uint32), np.array(first, np.uint32)


def test_alias_fragments(dev, small, kernel_form):
    """sccsum_fragments: one aliased d_frag_off makes its packet 0 + ST_RANGE."""
    s, E = small, small.E
    _assert_aliases(E, range(8), T)
    rng = np.random.default_rng(0xF4A6)
    f_off, f_len, first = _cut_fragments(rng, s.off[E.src], E.length)
    want = oracle.batch_fragments(s.buf, f_off, f_len, first, s.seeds[E.src])
    f_off = f_off.copy()
    for i in np.nonzero(~E.valid)[0]:
        j = int(first[i]) + int(rng.integers(0, int(first[i + 1]) - int(first[i])))
        f_off[j] = _alias(int(E.kind[i]), int(f_off[j]), int(f_len[j]))
    st = _marked(E.n, torch.uint8, dev)
    got = batch.fragments(s.d_data, T, _t(f_off, torch.int64), _t(f_len, torch.int32), _t(first, torch.int32),
                          seeds=_t(s.seeds[E.src], torch.int32), status=st, max_frag_len=s.max_len)
    torch.cuda.synchronize()
    _check_spans(E, batch.as_u16(got), st.cpu().numpy(), want[E.valid])


def _alias_desc(rng, s, E, base, nfrag):
    """One or two fragments per entry: d_off is the entry's offset (the alias),
    dst_off its low 32 bits (+ the cut), src the valid packet's bytes — or
    NULL, the bytes then lying at stage + dst_off for a valid entry."""
    src, dst, ln, first = [], [], [], [0]
    for i in range(E.n):
        o, L, k = int(E.off[i]), int(E.length[i]), int(s.off[E.src[i]])
        c = int(rng.integers(1, min(L, 40) if rng.random() < 0.3 else L)) if nfrag == 2 and L >= 2 else L
        for t, (a, l) in enumerate(((0, c), (c, L - c))):
            if l:
                src.append(0 if (i + t) % 3 == 0 else base + k + a)
                dst.append((o + a) & 0xFFFFFFFF)
                ln.append(l)
        first.append(len(ln))
    return batch.make_desc(np.array(src, np.uint64), np.array(dst, np.uint64), np.array(ln, np.uint32)), \
        np.array(first, np.int32)


@pytest.mark.parametrize("nfrag", [1, 2])
def test_alias_desc(dev, small, nfrag):
    """The tiling check refuses a d_off whose low 32 bits are the descriptor's
    dst_off: sccsum_spans_desc, sccsum_ipv4_frames_desc, and
    sccsum_ipv4_fill_desc with pool and stage untouched by the refused ones."""
    s, E = small, small.D
    _assert_aliases(E, range(1, 8), T)
    rng = np.random.default_rng(0xDE5C + nfrag)
    d = s.d_data.clone()  # pool and stage at once: src = its addresses, NULL src = stage + dst_off
    desc, first = _alias_desc(rng, s, E, d.data_ptr(), nfrag)
    args = (_t(desc.view(np.uint8)), _t(first), _t(E.off, torch.int64), _t(E.length, torch.int32), s.max_len)
    st, out = _marked(E.n, torch.uint8, dev), _marked(E.n, torch.int16, dev)
    batch.spans_desc(*args, seeds=_t(s.seeds[E.src], torch.int32), stage=d, out=out, status=st)
    torch.cuda.synchronize()
    _check_spans(E, batch.as_u16(out), st.cpu().numpy(), s.want_seeded)
    st, out2 = _marked(E.n, torch.uint8, dev), _marked(2 * E.n, torch.int16, dev)
    batch.ipv4_frames_desc(*args, stage=d, out2=out2, status=st)
    torch.cuda.synchronize()
    _check_frames(E, batch.as_u16(out2).reshape(-1, 2), st.cpu().numpy(), s.want2, s.want_st)
    assert torch.equal(d, s.d_data)
    for mode in MODES:
        d.copy_(s.d_data)
        st, out2 = _marked(E.n, torch.uint8, dev), _marked(2 * E.n, torch.int16, dev)
        batch.ipv4_fill_desc(*args, mode=FILL_MODES[mode], stage=d, out2=out2, status=st)
        torch.cuda.synchronize()
        want_buf, want2, want_st = s.fill[mode]
        _check_frames(E, batch.as_u16(out2).reshape(-1, 2), st.cpu().numpy(), want2, want_st)
        bad = np.nonzero(d.cpu().numpy() != want_buf)[0]
        assert bad.size == 0, f"{mode}: {bad.size} bytes differ, first at {bad[:8]}"


def test_alias_engine(dev, small):
    """submit and submit_fill steps of this kind: exact, and the run ends clean
    (finish / close raise on SCCSUM_EIDLE / SCCSUM_EFAULT)."""
    s, E = small, small.E
    _assert_aliases(E, range(8), T)
    mode = "ip_l4_icmp_echo"
    b = _pb(s.d_data, T, E.off, E.length, s.max_len)
    d = s.d_data.clone()
    bf = _pb(d, T, E.off, E.length, s.max_len)
    out2, st = _marked(2 * E.n, torch.int16, dev), _marked(E.n, torch.uint8, dev)
    out2f, stf = _marked(2 * E.n, torch.int16, dev), _marked(E.n, torch.uint8, dev)
    stv = _marked(E.n, torch.uint8, dev)
    outs, sts = _marked(E.n, torch.int16, dev), _marked(E.n, torch.uint8, dev)
    seeds = _t(s.seeds[E.src], torch.int32)
    stream = torch.cuda.Stream(device=dev)
    eng = batch.Engine(0, frames=True, fill=True, ring_slots=8, max_in_flight=2)
    torch.cuda.synchronize()
    eng.start(stream)
    eng.submit([(b, out2, st), (b, None, stv)], timeout_s=30.0)
    eng.submit_fill([(bf, out2f, stf)], FILL_MODES[mode], timeout_s=30.0)
    eng.finish(timeout_s=30.0)
    stream.synchronize()
    eng.close()
    eng = batch.Engine(0, frames=False, ring_slots=8, max_in_flight=2)
    eng.start(stream)
    eng.submit([(b, outs, sts, seeds)], timeout_s=30.0)
    eng.finish(timeout_s=30.0)
    stream.synchronize()
    eng.close()
    _check_frames(E, batch.as_u16(out2).reshape(-1, 2), st.cpu().numpy(), s.want2, s.want_st)
    _check_frames(E, None, stv.cpu().numpy(), s.want2, s.want_st)
    want_buf, want2, want_st = s.fill[mode]
    _check_frames(E, batch.as_u16(out2f).reshape(-1, 2), stf.cpu().numpy(), want2, want_st)
    assert np.array_equal(d.cpu().numpy(), want_buf)
    _check_spans(E, batch.as_u16(outs), sts.cpu().numpy(), s.want_seeded)


def test_alias_pipeline(dev, small):
    """sccsum_pipeline_run: one aliased host_off is SCCSUM_EINVAL in all four
    gather modes (checked on the host before anything of the chunk is queued),
    and the pipeline still runs afterwards."""
    s = small
    pinned = pipeline.pinned_empty(T)
    pinned[:] = s.buf
    j = next(i for i in range(3, s.off.size) if s.length[i] >= 20)
    pl = pipeline.HostPipeline(0, chunk_bytes=1 << 20, chunk_packets=64, depth=2)
    seen = 0
    for kind in range(8):
        off = s.off.copy()
        off[j] = _alias(kind, int(s.off[j]), int(s.length[j]))
        for gather in (native.GATHER_NONE, native.GATHER_HOST, native.GATHER_STRIDED, native.GATHER_ZERO_COPY):
            with pytest.raises(native.SccsumError) as e:
                pl.run(native.PIPE_IPV4 if kind % 2 else native.PIPE_SPANS, pinned, off, s.length, gather=gather,
                       max_len=s.max_len)
            assert e.value.code == native.SCCSUM_EINVAL, (ALIAS_KINDS[kind], gather)
            seen += 1
    assert seen == 32
    got, st = pl.run(native.PIPE_IPV4, pinned, s.off, s.length, status=True, gather=native.GATHER_ZERO_COPY,
                     max_len=s.max_len)
    pl.close()
    assert np.array_equal(got, s.want2) and np.array_equal(st, s.want_st)


# ------------------------------------------------------------------ parts B and C: the wide buffer

LENS6 = [P31 - 1, P31, P31 + 1, P32 - 31, P32 - 16, P32 - 1]
GIANT0 = 1 << 22  # the giant frames' headers: 128 KiB apart from here
# (offset, length) of the multi-GiB spans: each length at an even and at an odd start
GIANT_SPANS = [(2, P31 - 1), (P31 + 7, P31 - 1), (4, P31), (P31 + (1 << 20) + 1, P31), (8, P31 + 1),
               (P31 + (1 << 21) + 3, P31 + 1), (16, P32 - 1), ((1 << 26) + 1, P32 - 1)]


def _seq(rng, start, lengths, gaps=18):
    off, pos = [], start
    for L in lengths:
        off.append(pos)
        pos += int(L) + int(rng.integers(0, gaps))
    return off


def _wide_packets(rng, base):
    """(off, length, cluster, solo, straddler index) of part B's packets.
    Straddlers of one line overlap each other (they all hold the line), so an
    in-place fill takes the `solo` packets plus ONE straddler per line."""
    assert base % 16 == 0
    absx = (-base) % P32
    if absx < (1 << 24):
        absx += P32
    lines = [P31, P32] + ([absx] if absx not in (P31, P32) else [])
    off, length, cluster, solo, kidx = [], [], [], [], []

    def add(o, L, c, so, k=-1):
        off.extend(o), length.extend(L), cluster.extend([c] * len(o)), solo.extend([so] * len(o))
        kidx.extend(k if isinstance(k, list) else [k] * len(o))

    L0 = rng.integers(20, 9001, 70)
    add(_seq(rng, 0, L0), L0, 0, True)  # near offset 0 (the first at 0 itself)
    for c, X in enumerate(lines, start=1):
        so, sl = [], []
        for k in range(16):  # one straddler per start alignment
            st = ((X - 100 - 96 * k) & ~15) - 16 + k
            so.append(st)
            sl.append(X - st + int(rng.integers(1, 9000 - (X - st))))
        if X == P31:
            so.append(X - 66667), sl.append(200001)
        if X == P32:
            so.append(X - 30003), sl.append(65535)
        add(so, sl, c, False, list(range(len(so))))
        add([X - 4321, X], [4321, 3333], c, False)  # ending at the line, starting on it
        for start in (X - (1 << 19), X + (1 << 18) + 7):
            Lg = rng.integers(20, 9001, 25)
            add(_seq(rng, start, Lg), Lg, c, True)
    L3 = rng.integers(20, 9001, 70)
    add(_seq(rng, P32 + (1 << 25) + 5, L3), L3, 4, True)  # above 2^32
    L4 = np.concatenate([rng.integers(20, 9001, 49), [65535]])
    pos, o4 = W, []
    for L in L4[::-1]:
        o4.append(pos - int(L))
        pos = o4[-1] - int(rng.integers(0, 18))
    add(o4[::-1], L4, 5, True)  # the last ends exactly at W
    P = types.SimpleNamespace(off=np.array(off, np.uint64), length=np.array(length, np.uint32),
                              cluster=np.array(cluster), solo=np.array(solo), kidx=np.array(kidx), lines=lines,
                              absx=absx, n=len(off))
    # clusters keep to themselves (a line cluster spans its line +- 512 KiB)
    spans_ = sorted((int(P.off[P.cluster == c].min()), int((P.off + P.length)[P.cluster == c].max()))
                    for c in np.unique(P.cluster))
    assert all(a[1] <= b_[0] for a, b_ in zip(spans_[:-1], spans_[1:])), spans_
    assert int((P.off + P.length)[P.cluster == 0].max()) < GIANT0
    return P


def _giant_frames():
    """36 frames whose d_len is at a 32-bit edge: each length at head 0 and
    15, as UDP, TCP and ICMP echo; ip_len <= 65 535 whatever d_len says."""
    off, length, ip_len, proto, ihl = [], [], [], [], []
    for li, L in enumerate(LENS6):
        for hd in (0, 15):
            for pr in (17, 6, 1):
                j = len(off)
                off.append(GIANT0 + j * (1 << 17) + hd)
                length.append(L)
                ip_len.append([65535, 28 + 97 * j, 40000 + j][(j // 3) % 3])
                proto.append(pr)
                ihl.append(8 if j % 4 == 3 else 5)
    assert all(o + L <= W for o, L in zip(off, length))
    return types.SimpleNamespace(off=np.array(off, np.uint64), length=np.array(length, np.uint32),
                                 ip_len=np.array(ip_len), proto=np.array(proto), ihl=np.array(ihl), n=len(off))


def _write_headers(rng, data, off, length, ip_len=None, proto=None, ihl=None):
    """Valid IPv4 headers over the random bytes (the payload is what lies
    there): ihl 5..15, ip_len = the frame (a few padded, a few truncated),
    UDP / TCP / ICMP (echo requests mostly), DF or nothing in the fragment
    word (a few fragments)."""
    n = len(off)
    for i in range(n):
        o, L = int(off[i]), int(length[i])
        h = rng.integers(0, 256, size=20, dtype=np.uint8)
        il = int(ihl[i]) if ihl is not None else min(5 if rng.random() < 0.8 else int(rng.integers(6, 16)), L // 4)
        r = rng.random()
        pl = int(ip_len[i]) if ip_len is not None else min(
            65535, L - int(rng.integers(1, 40)) if r < 0.08 and L > 4 * il + 48 else (L + 9 if r > 0.97 else L))
        pr = int(proto[i]) if proto is not None else int(rng.choice([17, 6, 1]))
        fw = int(rng.choice([0, 0x4000])) if rng.random() < 0.92 else int(rng.choice([0x2000, 0x00B9, 0x2005]))
        h[0], h[2], h[3], h[6], h[7], h[9] = 0x40 | il, pl >> 8, pl & 0xFF, fw >> 8, fw & 0xFF, pr
        data[o:o + 20].copy_(torch.from_numpy(h))
        if pr == 1 and L > 4 * il and rng.random() < 0.8:
            data[o + 4 * il:o + 4 * il + 1].fill_(8)


def _compact(host, off, length, cap=None):
    """The packets' bytes at small host offsets (odd gaps): the oracle's image."""
    take = np.minimum(length, cap) if cap else length
    coff = np.empty(len(off), np.uint64)
    pos = 0
    for i in range(len(off)):
        pos += i % 4
        coff[i] = pos
        pos += int(take[i])
    img = np.empty(pos + 16, np.uint8)
    for i in range(len(off)):
        o, c, t = int(off[i]), int(coff[i]), int(take[i])
        img[c:c + t] = host[o:o + t]
    return img, coff


@pytest.fixture(scope="module")
def wide(dev):
    """The W-byte device buffer (random bytes generated on the device), its
    packets and giant frames, ONE host copy, and the oracle's values."""
    g = torch.Generator(device=dev)
    g.manual_seed(0x51DE)
    data = devsynth.random_bytes(W, g, dev)  # torch.empty inside: no room is an error, never a skip
    rng = np.random.default_rng(0xB16)
    w = types.SimpleNamespace(data=data, base=data.data_ptr())
    w.P = P = _wide_packets(rng, w.base)
    w.G = G = _giant_frames()
    _write_headers(rng, data, G.off, G.length, G.ip_len, G.proto, G.ihl)
    _write_headers(rng, data, P.off, P.length)
    torch.cuda.synchronize()
    w.host = np.empty(W, np.uint8)
    for a in range(0, W, 1 << 30):
        e = min(W, a + (1 << 30))
        w.host[a:e] = data[a:e].cpu().numpy()
    w.seeds = rng.integers(0, 1 << 32, size=P.n, dtype=np.uint64).astype(np.uint32)
    img, coff = _compact(w.host, P.off, P.length)
    w.want_spans = oracle.batch_spans(img, coff, P.length, nthreads=8)
    w.want_seeded = oracle.batch_spans(img, coff, P.length, w.seeds, nthreads=8)
    w.want2, w.want_st = oracle.batch_ipv4(img, coff, P.length, nthreads=8)
    w.want_h, w.want_hst = oracle.batch_ipv4_rss(img, coff, P.length)
    gimg, gcoff = _compact(w.host, G.off, G.length, CAP)
    w.g_want2, w.g_want_st = oracle.batch_ipv4(gimg, gcoff, G.length)
    # the multi-GiB spans: the oracle reads them in the host copy, where they lie
    w.S_off = np.array([o for o, _ in GIANT_SPANS], np.uint64)
    w.S_len = np.array([L for _, L in GIANT_SPANS], np.uint32)
    assert all(o + L <= W for o, L in GIANT_SPANS)
    w.S_seeds = rng.integers(0, 1 << 32, size=len(GIANT_SPANS), dtype=np.uint64).astype(np.uint32)
    w.S_want = oracle.batch_spans(w.host, w.S_off, w.S_len, nthreads=8)
    w.S_want_seeded = oracle.batch_spans(w.host, w.S_off, w.S_len, w.S_seeds, nthreads=8)
    w.orders = {"address": np.argsort(P.off, kind="stable"), "shuffled": np.random.default_rng(7).permutation(P.n)}
    return w


def _assert_clusters(w):
    """Every cluster is there, at least 8 packets start below each line and
    end above it, and the starts take all 16 alignments."""
    P = w.P
    end = P.off + P.length
    for c in range(6):
        if c == 3 and len(P.lines) == 2:
            continue  # the buffer starts on a multiple of 2^32: offset 2^32 is the absolute line too
        assert int((P.cluster == c).sum()) >= 50, c
    assert int(P.off.min()) == 0 and int(end.max()) == W
    assert int((P.off > P32).sum()) >= 70
    assert (w.base + P.absx) % P32 == 0 and 0 < P.absx < W
    for X in (P31, P32, P.absx):
        strad = (P.off < X) & (end > X)
        assert int(strad.sum()) >= 8, (X, int(strad.sum()))
        assert set((P.off[strad] % 16).tolist()) >= set(range(16))
    assert set((P.off % 16).tolist()) == set(range(16))
    assert sorted(P.length.tolist())[-3:] == [65535, 65535, 200001] and 320 <= P.n <= 460


@pytest.mark.parametrize("order", ["address", "shuffled"])
@pytest.mark.parametrize("seeded", [False, True], ids=["plain", "seeded"])
def test_wide_spans(dev, wide, kernel_form, order, seeded):
    w, P, ix = wide, wide.P, wide.orders[order]
    _assert_clusters(w)
    b = _pb(w.data, W, P.off[ix], P.length[ix], 200001)
    out, st = _marked(P.n, torch.int16, dev), _marked(P.n, torch.uint8, dev)
    batch.spans(b, seeds=_t(w.seeds[ix], torch.int32) if seeded else None, out=out, status=st)
    torch.cuda.synchronize()
    want = (w.want_seeded if seeded else w.want_spans)[ix]
    bad = np.nonzero(batch.as_u16(out) != want)[0]
    assert bad.size == 0, [(int(P.off[ix[i]]), int(P.length[ix[i]])) for i in bad[:6]]
    assert np.array_equal(st.cpu().numpy(), (want == 0).astype(np.uint8))


@pytest.mark.parametrize("order", ["address", "shuffled"])
@pytest.mark.parametrize("outputs", ["both", "status_alone"])
def test_wide_frames(dev, wide, kernel_form, order, outputs):
    w, P, ix = wide, wide.P, wide.orders[order]
    _assert_clusters(w)
    b = _pb(w.data, W, P.off[ix], P.length[ix], 200001)
    st = _marked(P.n, torch.uint8, dev)
    if outputs == "both":
        out2 = _marked(2 * P.n, torch.int16, dev)
        batch.ipv4_frames(b, out2=out2, status=st)
        torch.cuda.synchronize()
        bad = np.nonzero(np.any(batch.as_u16(out2).reshape(-1, 2) != w.want2[ix], axis=1))[0]
        assert bad.size == 0, [(int(P.off[ix[i]]), int(P.length[ix[i]])) for i in bad[:6]]
    else:
        batch.verify_frames(b, st)
        torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), w.want_st[ix])


def test_wide_multi(dev, wide, kernel_form):
    w, P, ix = wide, wide.P, wide.orders["shuffled"]
    _assert_clusters(w)
    parts = [ix[: P.n // 2 + 1], ix[P.n // 2 + 1:]]
    bs = [_pb(w.data, W, P.off[p], P.length[p], 200001) for p in parts]
    sts = [_marked(b.n, torch.uint8, dev) for b in bs]
    outs = [_marked(2 * b.n, torch.int16, dev) for b in bs]
    batch.ipv4_frames_multi([(b, o, t) for b, o, t in zip(bs, outs, sts)])
    torch.cuda.synchronize()
    for p, o, t in zip(parts, outs, sts):
        assert np.array_equal(batch.as_u16(o).reshape(-1, 2), w.want2[p])
        assert np.array_equal(t.cpu().numpy(), w.want_st[p])
    outs = [_marked(b.n, torch.int16, dev) for b in bs]
    batch.spans_multi([(b, o, None, _t(w.seeds[p], torch.int32)) for b, o, p in zip(bs, outs, parts)])
    torch.cuda.synchronize()
    for p, o in zip(parts, outs):
        assert np.array_equal(batch.as_u16(o), w.want_seeded[p])


def test_wide_rss(dev, wide, kernel_form):
    w, P, ix = wide, wide.P, wide.orders["shuffled"]
    _assert_clusters(w)
    b = _pb(w.data, W, P.off[ix], P.length[ix], 200001)
    st, h = _marked(P.n, torch.uint8, dev), _marked(P.n, torch.int32, dev)
    batch.ipv4_rss(b, hash_out=h, status=st)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(h), w.want_h[ix])
    assert np.array_equal(st.cpu().numpy() & native.ST_MALFORMED, w.want_hst[ix] & native.ST_MALFORMED)
    st, h, out2 = _marked(P.n, torch.uint8, dev), _marked(P.n, torch.int32, dev), _marked(2 * P.n, torch.int16, dev)
    batch.ipv4_frames_rss(b, out2=out2, status=st, hash_out=h)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(h), w.want_h[ix])
    assert np.array_equal(batch.as_u16(out2).reshape(-1, 2), w.want2[ix])
    assert np.array_equal(st.cpu().numpy(), w.want_st[ix])


@pytest.mark.parametrize("order", ["address", "shuffled"])
def test_wide_fragments(dev, wide, kernel_form, order):
    w, P, ix = wide, wide.P, wide.orders[order]
    _assert_clusters(w)
    f_off, f_len, first = _cut_fragments(np.random.default_rng(0xF7A6), P.off[ix], P.length[ix])
    st = _marked(P.n, torch.uint8, dev)
    got = batch.fragments(w.data, W, _t(f_off, torch.int64), _t(f_len, torch.int32), _t(first, torch.int32),
                          seeds=_t(w.seeds[ix], torch.int32), status=st, max_frag_len=200001)
    torch.cuda.synchronize()
    want = w.want_seeded[ix]  # a packet's fragments are contiguous here: the span's sum
    assert np.array_equal(batch.as_u16(got), want)
    assert np.array_equal(st.cpu().numpy(), (want == 0).astype(np.uint8))


def _wide_desc(w, off, length, nfrag, rng, cuts=None):
    """Descriptors over packets where they lie in the wide buffer.  A packet
    below 2^32 keeps its offset as its layout coordinate, so a fragment with a
    NULL src lies at stage + dst_off (dst_off up to 2^32 - 1: the second
    fragment of a straddler of 2^32 starts below the line); one above takes
    off - 2^32 and absolute src pointers."""
    src, dst, ln, first, lay = [], [], [], [0], []
    for i, (o, L) in enumerate(zip(off.tolist(), length.tolist())):
        lo = o if o < P32 else o - P32
        lay.append(lo)
        c = L
        if nfrag == 2 and L >= 2:
            c = int(cuts[i]) if cuts is not None and cuts[i] else int(rng.integers(1, L))
            if o < P32:
                c = min(c, P32 - 1 - o)
        for t, (a, l) in enumerate(((0, c), (c, L - c))):
            if l:
                stage = o < P32 and (i + t) % 3 == 0
                src.append(0 if stage else w.base + o + a)
                dst.append(lo + a)
                ln.append(l)
        first.append(len(ln))
    assert max(dst) < P32
    desc = batch.make_desc(np.array(src, np.uint64), np.array(dst, np.uint64), np.array(ln, np.uint32))
    return (_t(desc.view(np.uint8)), _t(np.array(first, np.int32)), _t(np.array(lay, np.uint64), torch.int64),
            _t(np.asarray(length, np.uint32), torch.int32)), desc


@pytest.mark.parametrize("nfrag", [1, 2])
def test_wide_desc(dev, wide, nfrag):
    """src pointers into the wide buffer (across the absolute 2^32 line too),
    stage fragments at dst_off up to 2^32 - 1."""
    w, P, ix = wide, wide.P, wide.orders["shuffled"]
    _assert_clusters(w)
    args, desc = _wide_desc(w, P.off[ix], P.length[ix], nfrag, np.random.default_rng(0xD0 + nfrag))
    absl = w.base + P.absx
    assert int(((desc["src"] != 0) & (desc["src"] < absl) & (desc["src"] + desc["len"] > absl)).sum()) >= 4
    near = (desc["src"] == 0) & (desc["dst_off"] > P32 - (1 << 19))
    assert int(near.sum()) >= 4 and int(desc["dst_off"][near].max()) > P32 - 2000
    st, out = _marked(P.n, torch.uint8, dev), _marked(P.n, torch.int16, dev)
    batch.spans_desc(*args, 200001, seeds=_t(w.seeds[ix], torch.int32), stage=w.data, out=out, status=st)
    torch.cuda.synchronize()
    assert np.array_equal(batch.as_u16(out), w.want_seeded[ix])
    st, out2 = _marked(P.n, torch.uint8, dev), _marked(2 * P.n, torch.int16, dev)
    batch.ipv4_frames_desc(*args, 200001, stage=w.data, out2=out2, status=st)
    torch.cuda.synchronize()
    assert np.array_equal(batch.as_u16(out2).reshape(-1, 2), w.want2[ix])
    assert np.array_equal(st.cpu().numpy(), w.want_st[ix])


# ---- in-place fills on the wide buffer: guard windows

def _regions(off, length):
    """Merged byte ranges to compare after a fill: each frame's reachable
    bytes and its end +- 64 B, and the same windows at off mod 2^32 and
    off mod 2^31, where a store through a truncated offset would land."""
    iv = []
    for o, L in zip(off.tolist(), length.tolist()):
        t = min(L, CAP)
        for s0 in {o, o % P32, o % P31}:
            iv.append((s0 - 64, s0 + t + 64))
            iv.append((s0 + L - 64, s0 + L + 64))
    iv = sorted((max(a, 0), min(b_, W)) for a, b_ in iv if a < W and b_ > 0)
    out = [list(iv[0])]
    for a, b_ in iv[1:]:
        if a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b_)
        else:
            out.append([a, b_])
    return out


def _restore(w, regions):
    for a, b_ in regions:
        w.data[a:b_].copy_(torch.from_numpy(w.host[a:b_]))
    torch.cuda.synchronize()


@contextlib.contextmanager
def _fill_guard(w, off, length):
    """Known bytes in every window before the launch (the host copy's), and
    the buffer as it was afterwards, whatever the test found."""
    regions = _regions(off, length)
    _restore(w, regions)
    try:
        yield regions
    finally:
        _restore(w, regions)


def _check_fill(w, regions, off, length, mode, out2, st):
    """Every window byte for byte: the oracle's fill of the frames, the host
    copy's bytes everywhere else."""
    img, coff = _compact(w.host, off, length, CAP)
    want_img, want2, want_st = oracle.batch_ipv4_fill(img, coff, length, mode)
    assert np.array_equal(batch.as_u16(out2).reshape(-1, 2)[: len(off)], want2)
    assert np.array_equal(st.cpu().numpy()[: len(off)], want_st)
    exp = [w.host[a:b_].copy() for a, b_ in regions]
    starts = [a for a, _ in regions]
    for o, L, c in zip(off.tolist(), length.tolist(), coff.tolist()):
        r = bisect.bisect_right(starts, o) - 1
        t = min(L, CAP)
        assert regions[r][0] <= o and o + t <= regions[r][1]
        exp[r][o - regions[r][0]: o - regions[r][0] + t] = want_img[c:c + t]
    assert int(((want_st & (native.ST_OK | native.ST_L4_OK)) != 0).sum()) > len(off) // 2  # fields were written
    for (a, b_), e in zip(regions, exp):
        got = w.data[a:b_].cpu().numpy()
        bad = np.nonzero(got != e)[0]
        assert bad.size == 0, f"window [{a}, {b_}): {bad.size} bytes differ, first at {a + int(bad[0])}"


def _fill_set(w, r):
    """Part B's packets for an in-place fill: the solo ones and one straddler
    per line (run r takes another one; r = 0 the 200 001 / 65 535-byte ones)."""
    P = w.P
    pick = P.solo.copy()
    for c in range(1, len(P.lines) + 1):
        ks = np.nonzero((P.cluster == c) & (P.kidx >= 0))[0]
        pick[ks[[ks.size - 1 if ks.size > 16 else 0, 5, 10, 15][r % 4]]] = True
    ix = np.nonzero(pick)[0]
    o, e = P.off[ix], P.off[ix] + P.length[ix]
    srt = np.argsort(o)
    assert np.all(e[srt][:-1] <= o[srt][1:])  # frames of a fill do not overlap
    for X in P.lines:
        assert int(((o < X) & (e > X)).sum()) == 1
    return np.random.default_rng(r).permutation(ix) if r % 2 else ix


@pytest.mark.parametrize("mode", MODES)
def test_wide_fill(dev, wide, kernel_form, fill_passes, mode):
    w, P = wide, wide.P
    _assert_clusters(w)
    ix = _fill_set(w, 2 * MODES.index(mode) + fill_passes - 1)
    off, length = P.off[ix], P.length[ix]
    b = _pb(w.data, W, off, length, 200001)
    out2, st = _marked(2 * b.n, torch.int16, dev), _marked(b.n, torch.uint8, dev)
    with _fill_guard(w, off, length) as regions:
        batch.ipv4_fill(b, FILL_MODES[mode], out2=out2, status=st)
        torch.cuda.synchronize()
        _check_fill(w, regions, off, length, FILL_MODES[mode], out2, st)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nfrag", [1, 2])
def test_wide_fill_desc(dev, wide, mode, nfrag):
    w, P = wide, wide.P
    _assert_clusters(w)
    ix = _fill_set(w, 2 * MODES.index(mode) + nfrag - 1)
    off, length = P.off[ix], P.length[ix]
    args, _ = _wide_desc(w, off, length, nfrag, np.random.default_rng(0xFD + nfrag))
    out2, st = _marked(2 * ix.size, torch.int16, dev), _marked(ix.size, torch.uint8, dev)
    with _fill_guard(w, off, length) as regions:
        batch.ipv4_fill_desc(*args, 200001, mode=FILL_MODES[mode], stage=w.data, out2=out2, status=st)
        torch.cuda.synchronize()
        _check_fill(w, regions, off, length, FILL_MODES[mode], out2, st)


def test_wide_engine(dev, wide):
    """Three sum steps and one fill step, each a slice of the wide buffer with
    bytes_len = W and a max_len hint; the run ends clean."""
    w, P = wide, wide.P
    _assert_clusters(w)
    ix = w.orders["shuffled"]
    parts = [ix[0::3], ix[1::3], ix[2::3]]
    bs = [_pb(w.data, W, P.off[p], P.length[p], 200001) for p in parts]
    outs = [_marked(2 * b.n, torch.int16, dev) for b in bs]
    sts = [_marked(b.n, torch.uint8, dev) for b in bs]
    fx = _fill_set(w, 3)
    foff, flen = P.off[fx], P.length[fx]
    bf = _pb(w.data, W, foff, flen, 65535)
    out2f, stf = _marked(2 * bf.n, torch.int16, dev), _marked(bf.n, torch.uint8, dev)
    mode = native.FILL_IP | native.FILL_L4
    stream = torch.cuda.Stream(device=dev)
    with _fill_guard(w, foff, flen) as regions:
        eng = batch.Engine(0, frames=True, fill=True, ring_slots=8, max_in_flight=2)
        torch.cuda.synchronize()
        eng.start(stream)
        for b, o, t in zip(bs, outs, sts):
            last = eng.submit([(b, o, t)], timeout_s=30.0)
        eng.wait(last, timeout_s=30.0)  # the fill writes frames the sum steps read
        for k in range(last):
            eng.wait(k, timeout_s=30.0)
        eng.submit_fill([(bf, out2f, stf)], mode, timeout_s=30.0)
        eng.finish(timeout_s=30.0)
        stream.synchronize()
        eng.close()
        for p, o, t in zip(parts, outs, sts):
            assert np.array_equal(batch.as_u16(o).reshape(-1, 2), w.want2[p])
            assert np.array_equal(t.cpu().numpy(), w.want_st[p])
        _check_fill(w, regions, foff, flen, mode, out2f, stf)


# ------------------------------------------------------------------ part C: lengths at the 32-bit edges

def _giant_mix(w):
    """The 36 giant frames among part B's 70 short frames at offset 0, shuffled."""
    P, G = w.P, w.G
    near = np.nonzero(P.cluster == 0)[0]
    off = np.concatenate([G.off, P.off[near]])
    length = np.concatenate([G.length, P.length[near]])
    want2 = np.concatenate([w.g_want2, w.want2[near]])
    want_st = np.concatenate([w.g_want_st, w.want_st[near]])
    ix = np.random.default_rng(0xC1).permutation(off.size)
    for L in LENS6:
        assert int((length == L).sum()) == 6 and {int(o) % 16 for o in off[length == L]} == {0, 15}
    assert int(((w.g_want_st & native.ST_MALFORMED) != 0).sum()) <= G.n // 3  # most have an L4 range to sum
    return off[ix], length[ix], want2[ix], want_st[ix]


def test_giant_frames(dev, wide, kernel_form):
    """Frames with d_len from 2^31 - 1 to 2^32 - 1 (head 0 and 15; UDP, TCP,
    ICMP echo) among short frames in one tile: values and status."""
    w = wide
    off, length, want2, want_st = _giant_mix(w)
    b = _pb(w.data, W, off, length, P32 - 1)
    out2, st = _marked(2 * b.n, torch.int16, dev), _marked(b.n, torch.uint8, dev)
    batch.ipv4_frames(b, out2=out2, status=st)
    torch.cuda.synchronize()
    got2 = batch.as_u16(out2).reshape(-1, 2)
    bad = np.nonzero(np.any(got2 != want2, axis=1) | (st.cpu().numpy() != want_st))[0]
    assert bad.size == 0, [(int(off[i]), int(length[i]), got2[i].tolist(), want2[i].tolist()) for i in bad[:6]]
    stv = _marked(b.n, torch.uint8, dev)
    batch.verify_frames(b, stv)
    torch.cuda.synchronize()
    assert np.array_equal(stv.cpu().numpy(), want_st)


def test_giant_frames_in_full_tiles(dev, wide, kernel_form):
    """The mix above is one packet per flat-kernel tile (a launch smaller than
    the grid).  Here the same frames are drawn 70 000 times under one block per
    CU, so the flat forms' tiles hold 64 packets: giant and short frames side
    by side in every tile (the per-packet forms just see more packets)."""
    w = wide
    off, length, want2, want_st = _giant_mix(w)
    rep = np.random.default_rng(0xC6).integers(0, off.size, 70000)
    assert int((length[rep] >= P31 - 1).sum()) > 20000
    b = _pb(w.data, W, off[rep], length[rep], P32 - 1)
    out2, st = _marked(2 * b.n, torch.int16, dev), _marked(b.n, torch.uint8, dev)
    lib = native.load()
    try:
        native.check(lib.sccsum_set_blocks_per_cu(1), "blocks")
        native.check(lib.sccsum_set_tile_bytes(0), "tile bytes")  # the plain 64-packet cap
        batch.ipv4_frames(b, out2=out2, status=st)
        torch.cuda.synchronize()
    finally:
        lib.sccsum_set_blocks_per_cu(8)
        lib.sccsum_set_tile_bytes(49152)
    got2 = batch.as_u16(out2).reshape(-1, 2)
    bad = np.nonzero(np.any(got2 != want2[rep], axis=1) | (st.cpu().numpy() != want_st[rep]))[0]
    assert bad.size == 0, (bad.size, [(int(off[rep[i]]), int(length[rep[i]])) for i in bad[:6]])


def _giant_cuts(off, length):
    """Two fragments: the first 2^31 + 1 bytes where the frame is longer, else
    a cut inside the IPv4 header or the L4 range."""
    return [P31 + 1 if L > P31 + 1 else ((7 if i % 2 else 4341) if L >= P31 - 1 else 0)
            for i, L in enumerate(length.tolist())]


@pytest.mark.parametrize("nfrag", [1, 2])
def test_giant_frames_desc(dev, wide, nfrag):
    w = wide
    off, length, want2, want_st = _giant_mix(w)
    args, desc = _wide_desc(w, off, length, nfrag, np.random.default_rng(0xC2), _giant_cuts(off, length))
    assert nfrag == 1 or int((desc["len"] == P31 + 1).sum()) == 18
    out2, st = _marked(2 * off.size, torch.int16, dev), _marked(off.size, torch.uint8, dev)
    batch.ipv4_frames_desc(*args, P32 - 1, stage=w.data, out2=out2, status=st)
    torch.cuda.synchronize()
    got2 = batch.as_u16(out2).reshape(-1, 2)
    bad = np.nonzero(np.any(got2 != want2, axis=1) | (st.cpu().numpy() != want_st))[0]
    assert bad.size == 0, [(int(off[i]), int(length[i]), got2[i].tolist(), want2[i].tolist()) for i in bad[:6]]


def _giant_fill_set(w, li, hd):
    """One giant frame (frames of a fill do not overlap, and its d_len covers
    most of the buffer) in the middle of every solo short frame outside it."""
    P, G = w.P, w.G
    j = li * 6 + hd * 3 + (2 * li + hd) % 3
    o, L = int(G.off[j]), int(G.length[j])
    assert L == LENS6[li] and o % 16 == 15 * hd
    end = P.off + P.length
    out = np.nonzero(P.solo & ((end <= o) | (P.off >= o + L)))[0]
    assert int((P.cluster[out] == 0).sum()) == 70 and out.size >= 100
    h = out.size // 2
    off = np.concatenate([P.off[out[:h]], [o], P.off[out[h:]]]).astype(np.uint64)
    length = np.concatenate([P.length[out[:h]], [L], P.length[out[h:]]]).astype(np.uint32)
    return off, length


GIANT_FILLS = [(li, hd) for li in range(6) for hd in (0, 1)]
GIANT_FILL_IDS = [f"{'2^31-1 2^31 2^31+1 2^32-31 2^32-16 2^32-1'.split()[li]}-head{15 * hd}" for li, hd in GIANT_FILLS]


@pytest.mark.parametrize("li,hd", GIANT_FILLS, ids=GIANT_FILL_IDS)
def test_giant_fill(dev, wide, li, hd):
    w = wide
    off, length = _giant_fill_set(w, li, hd)
    mode = FILL_MODES["ip_l4_icmp_echo"]
    b = _pb(w.data, W, off, length, P32 - 1)
    out2, st = _marked(2 * b.n, torch.int16, dev), _marked(b.n, torch.uint8, dev)
    with _fill_guard(w, off, length) as regions:
        batch.ipv4_fill(b, mode, out2=out2, status=st)
        torch.cuda.synchronize()
        _check_fill(w, regions, off, length, mode, out2, st)


@pytest.mark.parametrize("nfrag", [1, 2])
@pytest.mark.parametrize("li,hd", GIANT_FILLS, ids=GIANT_FILL_IDS)
def test_giant_fill_desc(dev, wide, li, hd, nfrag):
    w = wide
    off, length = _giant_fill_set(w, li, hd)
    mode = FILL_MODES["ip_l4_icmp_echo"]
    args, _ = _wide_desc(w, off, length, nfrag, np.random.default_rng(0xC3), _giant_cuts(off, length))
    out2, st = _marked(2 * off.size, torch.int16, dev), _marked(off.size, torch.uint8, dev)
    with _fill_guard(w, off, length) as regions:
        batch.ipv4_fill_desc(*args, P32 - 1, mode=mode, stage=w.data, out2=out2, status=st)
        torch.cuda.synchronize()
        _check_fill(w, regions, off, length, mode, out2, st)


def _span_mix(w, with_4g=True):
    """The multi-GiB spans among part B's packets, 40 entries apart: each on a
    wave of its own, side by side in one launch."""
    P = w.P
    keep = [g for g in range(len(GIANT_SPANS)) if with_4g or GIANT_SPANS[g][1] != P32 - 1]
    ix = w.orders["shuffled"]
    off, length, seeds, want, want_seeded = [], [], [], [], []
    at = 0
    for k, i in enumerate(ix.tolist()):
        if k % 40 == 20 and at < len(keep):
            g = keep[at]
            at += 1
            off.append(int(w.S_off[g])), length.append(int(w.S_len[g])), seeds.append(int(w.S_seeds[g]))
            want.append(int(w.S_want[g])), want_seeded.append(int(w.S_want_seeded[g]))
        off.append(int(P.off[i])), length.append(int(P.length[i])), seeds.append(int(w.seeds[i]))
        want.append(int(w.want_spans[i])), want_seeded.append(int(w.want_seeded[i]))
    assert at == len(keep)
    length = np.array(length, np.uint32)
    off = np.array(off, np.uint64)
    for L in (P31 - 1, P31, P31 + 1) + ((P32 - 1,) if with_4g else ()):
        assert sorted(int(o) % 2 for o in off[length == L]) == [0, 1]  # an even and an odd start address
    return (off, length, np.array(seeds, np.uint32), np.array(want, np.uint16), np.array(want_seeded, np.uint16))


def _span_report(off, length, got, want):
    bad = np.nonzero(got != want)[0]
    return [(int(off[i]), int(length[i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:10]]


def test_giant_spans(dev, wide, kernel_form):
    """Spans of 2^31 - 1, 2^31, 2^31 + 1 and 2^32 - 1 bytes, random bytes, at
    even and odd addresses, next to short ones, under every kernel form."""
    w = wide
    off, length, seeds, _, want = _span_mix(w)
    b = _pb(w.data, W, off, length, P32 - 1)
    out, st = _marked(b.n, torch.int16, dev), _marked(b.n, torch.uint8, dev)
    batch.spans(b, seeds=_t(seeds, torch.int32), out=out, status=st)
    torch.cuda.synchronize()
    got = batch.as_u16(out)
    assert np.array_equal(got, want), _span_report(off, length, got, want)
    assert np.array_equal(st.cpu().numpy(), (want == 0).astype(np.uint8))


@pytest.mark.parametrize("nfrag", [1, 2])
def test_giant_spans_desc(dev, wide, nfrag):
    """sccsum_spans_desc: one fragment (the contiguous-span path), and two with
    the first 2^31 + 1 bytes long (2^30 + 1 where the span is shorter)."""
    w = wide
    off, length, seeds, want, _ = _span_mix(w)
    cuts = [(P31 + 1 if L > P31 + 1 else (1 << 30) + 1) if L >= P31 - 1 else 0 for L in length.tolist()]
    args, desc = _wide_desc(w, off, length, nfrag, np.random.default_rng(0xC4), cuts)
    assert nfrag == 1 or (int((desc["len"] == P31 + 1).sum()) == 2 and int((desc["len"] >= (1 << 30)).sum()) == 12)
    out, st = _marked(off.size, torch.int16, dev), _marked(off.size, torch.uint8, dev)
    batch.spans_desc(*args, P32 - 1, stage=w.data, out=out, status=st)
    torch.cuda.synchronize()
    got = batch.as_u16(out)
    assert np.array_equal(got, want), _span_report(off, length, got, want)


def test_giant_spans_fragments(dev, wide):
    """sccsum_fragments: each multi-GiB span as two fragments (the first
    2^31 + 1 or 2^30 + 1 bytes long), short packets as one to three."""
    w = wide
    off, length, seeds, _, want = _span_mix(w)
    rng = np.random.default_rng(0xC5)
    f_off, f_len, first = [], [], [0]
    for o, L in zip(off.tolist(), length.tolist()):
        if L >= P31 - 1:
            c = P31 + 1 if L > P31 + 1 else (1 << 30) + 1
            f_off += [o, o + c]
            f_len += [c, L - c]
        else:
            fo, fl, _ = _cut_fragments(rng, np.array([o], np.uint64), np.array([L], np.uint32))
            f_off += fo.tolist()
            f_len += fl.tolist()
        first.append(len(f_off))
    st = _marked(off.size, torch.uint8, dev)
    got = batch.fragments(w.data, W, _t(np.array(f_off, np.uint64), torch.int64),
                          _t(np.array(f_len, np.uint32), torch.int32), _t(np.array(first, np.uint32), torch.int32),
                          seeds=_t(seeds, torch.int32), status=st, max_frag_len=P32 - 1)
    torch.cuda.synchronize()
    got = batch.as_u16(got)
    assert np.array_equal(got, want), _span_report(off, length, got, want)
