"""max_len is a hint: every kernel form it can pick, under true, wrong and
missing hints, against the oracle on the same bytes, bit for bit.

include/sccsum.h promises "0 = unknown; any value is correct, it only tunes
speed".  In seastar_amd/csrc/sccsum.hip the hint (and the diagnostics knob
sccsum_set_group_units) selects template instantiations whose later loop
passes a truthful hint never runs:

  launch_rows    units = (max_len + 30) / 16 (0: 128);  units <= 32 -> V 2,
                 <= 64 -> V 4, <= 96 -> V 6, else V 8  (csum_row_kernel<V>;
                 one pass of its g loop covers V * 256 bytes)
  units_class    sccsum_set_group_units(U) if set; max_len 0 -> 4; else
                 units <= 64 -> U 1, <= 128 -> U 2, <= 256 -> U 4, else U 8
                 (csum_kernel<U>: one step covers U * 1024 bytes)
  launch_desc    switch (units_class(max_len)): 1, 2, default 4
                 (csum_desc_kernel<U>; a forced 8 runs as 4)

(max_len + 30) / 16 <= u holds up to max_len = 16 u - 15, so the last hint
of each class is 497 / 1009 / 1521 (rows) and 1009 / 2033 / 4081 (units).

Section 1 sweeps every length at every start alignment through each of those
instantiations, past its first pass; section 2 runs one mixed batch and one
slot-shaped batch through every entry point under every hint."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import oracle
from seastar_amd import batch, native, pipeline, synth
from test_gpu_parity import FILL_MODES, _tx_frames

pytestmark = pytest.mark.gpu


def _last_hint(units):
    """The largest max_len with (max_len + 30) / 16 <= units (launch_rows, units_class)."""
    h = 16 * units - 15
    assert (h + 30) // 16 == units and (h + 1 + 30) // 16 == units + 1
    return h


ROW_LAST = {2: _last_hint(32), 4: _last_hint(64), 6: _last_hint(96)}   # 497, 1009, 1521; above: V 8
UNIT_LAST = {1: _last_hint(64), 2: _last_hint(128), 4: _last_hint(256)}  # 1009, 2033, 4081; above: U 8
# a hint well inside each class: units 1 / 39 / 70 / 251 (and 0 -> 128) for the rows,
# units 33 / 95 / 189 / 376 for units_class
ROW_HINTS = {2: (1,), 4: (600,), 6: (1100,), 8: (4000, 0)}
UNIT_HINTS = {1: 500, 2: 1500, 4: 3000, 8: 6000}
for _v, _hs in ROW_HINTS.items():
    for _h in _hs:
        _u = (_h + 30) // 16 if _h else 128
        assert (2 if _u <= 32 else 4 if _u <= 64 else 6 if _u <= 96 else 8) == _v
for _c, _h in UNIT_HINTS.items():
    _u = (_h + 30) // 16
    assert (1 if _u <= 64 else 2 if _u <= 128 else 4 if _u <= 256 else 8) == _c


@pytest.fixture
def knobs(dev):
    """Sets the diagnostics knobs of this thread; teardown puts back their
    defaults: variant 0, group units 0, native.FILL_SINGLE_MAX."""
    lib = native.load()

    def set_(variant=0, group_units=0, fill_single_max=native.FILL_SINGLE_MAX):
        native.check(lib.sccsum_set_kernel_variant(variant), "sccsum_set_kernel_variant")
        native.check(lib.sccsum_set_group_units(group_units), "sccsum_set_group_units")
        native.check(lib.sccsum_set_fill_single_max(fill_single_max), "sccsum_set_fill_single_max")

    yield set_
    set_()


def _hinted(b, hint):
    """The same device batch with max_len = hint."""
    return dataclasses.replace(b, max_len=int(hint))


def _t(a, dtype=None):
    t = torch.from_numpy(np.array(a))  # (a copy: the shared cases are read-only)
    return (t if dtype is None else t.view(dtype)).to("cuda:0")


def _write_headers(buf, off, lens):
    """An IPv4 header (ihl 5, ip_len = L, atomic, UDP or TCP by turns) over the
    first bytes of every packet of at least 20 bytes: with ip_len == L and no
    options a frame stays on the kernels' fast path, the one the hint shapes
    (options or a trimmed length go to the exact redo).  Shorter packets keep
    their raw bytes: MALFORMED."""
    f = np.nonzero(lens >= 20)[0]
    o = off[f].astype(np.int64)
    L = lens[f].astype(np.int64)
    assert L.size == 0 or int(L.max()) <= 65535
    buf[o] = 0x45
    buf[o + 2] = L >> 8
    buf[o + 3] = L & 0xFF
    buf[o + 6] = np.where(f % 3 == 0, 0x40, 0)  # DF alone is still atomic
    buf[o + 7] = 0
    buf[o + 9] = np.where(f % 2 == 0, 17, 6)


# ---------------------------------------------------------------- 1. sweeps

class Sweep:
    """Every length of `lengths` at all 16 start alignments, placed as
    test_every_length_every_alignment places them (each start = the next
    16-byte boundary + head); the same bytes as seeded spans and as frames."""

    def __init__(self, lengths, seed):
        rng = np.random.default_rng(seed)
        lengths = np.asarray(lengths, np.uint32)
        self.lengths = lengths
        self.lens = np.tile(lengths, 16)
        self.heads = np.repeat(np.arange(16, dtype=np.uint64), lengths.size)
        room = (self.heads + self.lens + np.uint64(15)) // np.uint64(16) * np.uint64(16)
        base = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.uint64)
        self.off = base + self.heads
        total = int(base[-1] + room[-1])
        self.buf = rng.integers(0, 256, size=total, dtype=np.uint8)
        _write_headers(self.buf, self.off, self.lens)
        self.seeds = rng.integers(0, 1 << 32, self.lens.size, dtype=np.uint64).astype(np.uint32)
        self.want_spans = oracle.batch_spans(self.buf, self.off, self.lens, self.seeds, nthreads=8)
        self.want_frames, self.want_st = oracle.batch_ipv4(self.buf, self.off, self.lens, nthreads=8)
        self.pairs = self.lens.size

    def device(self, dev):
        b = batch.PacketBatch.from_host(self.buf, self.off, self.lens, device=dev)
        assert int(((b.data.data_ptr() + self.off) % 16 != self.heads).sum()) == 0  # head = address mod 16
        return b, _t(self.seeds.view(np.int32))

    def check(self, what, got, want, idx=None):
        """Bit-exact, or the first mismatches as (length, head, got, want); returns the pairs compared."""
        idx = np.arange(self.pairs) if idx is None else idx
        want = want[idx]
        assert got.shape == want.shape, what
        ne = got != want
        bad = np.nonzero(ne.any(axis=1) if ne.ndim == 2 else ne)[0]
        assert bad.size == 0, f"{what}: {bad.size} of {idx.size} differ, first (length, head, got, want): " + str(
            [(int(self.lens[idx[i]]), int(self.heads[idx[i]]), got[i].tolist(), want[i].tolist()) for i in bad[:8]])
        return idx.size

    def check_spans(self, what, out, st, idx=None):
        c = self.check(what + " out", batch.as_u16(out), self.want_spans, idx)
        self.check(what + " status", st.cpu().numpy(), (self.want_spans == 0).astype(np.uint8), idx)
        return c

    def check_frames(self, what, out2, st, idx=None):
        c = self.check(what + " out2", batch.as_u16(out2).reshape(-1, 2), self.want_frames, idx)
        self.check(what + " status", st.cpu().numpy(), self.want_st, idx)
        return c


def _single(sw, b, sd, hint, what):
    """The sweep as one sccsum_spans and one sccsum_ipv4_frames launch; returns the pairs compared."""
    hb = _hinted(b, hint)
    st = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=b.device)
    out = batch.spans(hb, seeds=sd, status=st)
    torch.cuda.synchronize()
    c = sw.check_spans(f"{what} spans hint {hint}", out, st)
    st2 = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=b.device)
    out2 = batch.ipv4_frames(hb, status=st2)
    torch.cuda.synchronize()
    return c + sw.check_frames(f"{what} frames hint {hint}", out2, st2)


def _slice(b, idx_t, hint):
    """Packets idx_t of b as a batch of its own over the same bytes."""
    return batch.PacketBatch(data=b.data, off=b.off[idx_t].contiguous(), length=b.length[idx_t].contiguous(),
                             bytes_len=b.bytes_len, max_len=int(hint))


@functools.lru_cache(maxsize=1)
def _row_sweep(V):
    return Sweep(np.arange(0, 2 * V * 256 + 33), seed=0x5100 + V)


@pytest.mark.parametrize("V", [2, 4, 6, 8])
def test_row_kernel_every_length_every_alignment(dev, knobs, V):
    """csum_row_kernel<V, spans | frames> and its MQ form, V picked by the hint
    alone (launch_rows: `if (units <= 32) ... <= 64 ... <= 96`, units =
    (max_len + 30) / 16, 128 for 0): hints 1 / 600 / 1100 / 4000 and 0 give
    V 2 / 4 / 6 / 8 and 8.  Lengths 0 .. 2 V 256 + 32 at all 16 heads: one
    pass of the g loop, two, and the start of a third, which V 2, 4 and 6
    only take under an understated hint; the last unit (the `lastv` select,
    `lim >= 1 && lim <= 16 * V && ((lim - 1) & 15) == 0`) lands on every lane
    of a row, on every u, in every pass.  Single batch under variant 2
    (launch() -> launch_rows); then the lengths V 256 - 48 .. 2 V 256 + 32 as
    3 batches of one sccsum_*_multi launch under variant 0, at most
    kSmallRowsMax = 65 536 packets in all, which launch_multi gives to
    csum_row_kernel<V, ., MQ = true>."""
    sw = _row_sweep(V)
    b, sd = sw.device(dev)
    assert sw.pairs == 16 * (2 * V * 256 + 33)
    knobs(variant=2)
    for hint in ROW_HINTS[V]:
        assert _single(sw, b, sd, hint, f"row V {V}") == 2 * sw.pairs
    knobs(variant=0)
    sel = np.nonzero(sw.lens >= V * 256 - 48)[0]
    assert sel.size == 16 * (V * 256 + 32 + 49) and sel.size <= 65536
    parts = np.array_split(sel, 3)
    for hint in ROW_HINTS[V]:
        items, fitems = [], []
        for idx in parts:
            it = torch.from_numpy(idx).to(dev)
            sb = _slice(b, it, hint)
            items.append((sb, None, torch.full((sb.n,), 0xEE, dtype=torch.uint8, device=dev), sd[it].contiguous()))
            fitems.append((sb, None, torch.full((sb.n,), 0xEE, dtype=torch.uint8, device=dev)))
        outs = batch.spans_multi(items)
        fouts = batch.ipv4_frames_multi(fitems)
        torch.cuda.synchronize()
        compared = 0
        for idx, item, o, fitem, fo in zip(parts, items, outs, fitems, fouts):
            compared += sw.check_spans(f"row V {V} MQ spans hint {hint}", o, item[2], idx)
            compared += sw.check_frames(f"row V {V} MQ frames hint {hint}", fo, fitem[2], idx)
        assert compared == 2 * sel.size


def _unit_lengths(U):
    """Every length 0 .. U 1024 + 64 (one step of a U-unit kernel and the start
    of the next) plus k U 1024 +- 48 for k = 2, 3 (the second and third step's
    ends)."""
    step = U * 1024
    return np.concatenate([np.arange(0, step + 65)] + [np.arange(k * step - 48, k * step + 49) for k in (2, 3)])


@functools.lru_cache(maxsize=1)
def _unit_sweep(U):
    return Sweep(_unit_lengths(U), seed=0x5200 + U)


@pytest.mark.parametrize("U,how", [(1, "forced"), (1, "hint"), (2, "forced"), (4, "forced"), (8, "forced"),
                                   (8, "hint")])
def test_simple_kernel_every_length_every_alignment(dev, knobs, U, how):
    """csum_kernel<U, spans | frames> (variant 1; launch_simple's switch on
    units_class): U forced by sccsum_set_group_units (`if (forced) return
    forced`) under the true maximum, and U 1 / U 8 once more by hint alone
    (group units 0; hints 500 -> 33 units <= 64 -> U 1, 6000 -> 376 units > 256
    -> U 8).  One step of span_packet's loop covers U 1024 bytes: lengths
    0 .. U 1024 + 64 and k U 1024 +- 48 (k = 2, 3) at all 16 heads, so U 1
    meets packets of two, three and four steps."""
    sw = _unit_sweep(U)
    b, sd = sw.device(dev)
    assert sw.pairs == 16 * (U * 1024 + 65 + 2 * 97)
    knobs(variant=1, group_units=U if how == "forced" else 0)
    hint = b.max_len if how == "forced" else UNIT_HINTS[U]
    assert _single(sw, b, sd, hint, f"simple U {U} ({how})") == 2 * sw.pairs


class Lists:
    """Packets of a contiguous image cut at `cuts` (sorted positions inside
    each packet) into fragments placed in a pool in shuffled order, fragment j
    at source alignment j mod 16; the packet layout is the image's own
    (dst_off = off + position in the packet)."""

    def __init__(self, rng, buf, off, lens, cuts):
        n = lens.size
        self.buf, self.off, self.lens = buf, off, lens
        pk, pa, pl = [], [], []
        self.first = np.zeros(n + 1, np.int32)
        for i in range(n):
            edges = [0, *cuts[i], int(lens[i])]
            self.first[i] = len(pk)
            for a, z in zip(edges[:-1], edges[1:]):
                assert z >= a
                if z > a:  # (empty pieces dropped, as the burst queue drops them)
                    pk.append(i)
                    pa.append(a)
                    pl.append(z - a)
        self.first[n] = len(pk)
        self.pk, self.pa, self.pl = np.array(pk, np.int64), np.array(pa, np.int64), np.array(pl, np.int64)
        nd = self.pk.size
        self.pos = np.zeros(nd, np.int64)
        at = 0
        for j in rng.permutation(nd):
            at = (at + 15) // 16 * 16 + int(j) % 16
            self.pos[j] = at
            at += int(self.pl[j]) + int(rng.integers(0, 24))
        self.src_off = off[self.pk].astype(np.int64) + self.pa  # the pieces' bytes in the image
        self.pool = rng.integers(0, 256, size=at + 64, dtype=np.uint8)
        self.pool = self.image(buf)

    def image(self, frames):
        """The pool with every piece's bytes taken from `frames`."""
        pool = self.pool.copy()
        for p, s, ln in zip(self.pos.tolist(), self.src_off.tolist(), self.pl.tolist()):
            pool[p:p + ln] = frames[s:s + ln]
        return pool

    def device(self, dev):
        self.d_pool = torch.from_numpy(self.pool.copy()).to(dev)
        base = self.d_pool.data_ptr()
        desc = batch.make_desc(base + self.pos, self.src_off, self.pl)
        assert int(self.src_off.max(initial=0)) < 1 << 32
        self.aligns = set(((base + self.pos) % 16).tolist())
        # per packet, for the reports: its first fragment's source address mod 16
        f0 = np.minimum(self.first[:-1], self.pos.size - 1)
        self.heads = np.where(self.first[1:] > self.first[:-1], (base + self.pos[f0]) % 16, 0)
        self.args = (_t(desc.view(np.uint8)), _t(self.first), _t(self.off.astype(np.uint64).view(np.int64)),
                     _t(self.lens.astype(np.uint32).view(np.int32)))
        return self

    def restore(self):
        self.d_pool.copy_(torch.from_numpy(self.pool))

    def _pool_byte(self, x, got, want):
        """(length, head, got, want) of pool byte x; length -1: between the fragments."""
        j = np.nonzero((self.pos <= x) & (x < self.pos + self.pl))[0]
        i = int(self.pk[j[0]]) if j.size else -1
        return (int(self.lens[i]) if i >= 0 else -1, int(self.heads[i]) if i >= 0 else x % 16, int(got[x]),
                int(want[x]))

    def check(self, what, got, want):
        assert got.shape == want.shape, what
        ne = got != want
        bad = np.nonzero(ne.any(axis=1) if ne.ndim == 2 else ne)[0]
        assert bad.size == 0, f"{what}: {bad.size} of {want.shape[0]} differ, first (length, head, got, want): " + str(
            [(int(self.lens[i]), int(self.heads[i]), got[i].tolist(), want[i].tolist()) for i in bad[:8]])
        return want.shape[0]

    def run(self, what, hint, seeds_t, want_spans, want_frames, want_st, fill_mode, want_fill):
        """sccsum_spans_desc, sccsum_ipv4_frames_desc and sccsum_ipv4_fill_desc
        under one hint; returns the packets compared (three times n)."""
        dev = self.d_pool.device
        n = self.lens.size
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        out = batch.spans_desc(*self.args, hint, seeds=seeds_t, status=st)
        torch.cuda.synchronize()
        c = self.check(f"{what} spans_desc hint {hint} out", batch.as_u16(out), want_spans)
        self.check(f"{what} spans_desc hint {hint} status", st.cpu().numpy(), (want_spans == 0).astype(np.uint8))
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        out2 = batch.ipv4_frames_desc(*self.args, hint, status=st)
        torch.cuda.synchronize()
        c += self.check(f"{what} frames_desc hint {hint} out2", batch.as_u16(out2).reshape(-1, 2), want_frames)
        self.check(f"{what} frames_desc hint {hint} status", st.cpu().numpy(), want_st)
        filled, fill2, fill_st = want_fill
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        out2 = batch.ipv4_fill_desc(*self.args, hint, mode=fill_mode, status=st)
        torch.cuda.synchronize()
        c += self.check(f"{what} fill_desc hint {hint} out2", batch.as_u16(out2).reshape(-1, 2), fill2)
        self.check(f"{what} fill_desc hint {hint} status", st.cpu().numpy(), fill_st)
        got_pool, want_pool = self.d_pool.cpu().numpy(), self.image(filled)
        bad = np.nonzero(got_pool != want_pool)[0]  # the fragments' stored bytes, and every byte between them
        assert bad.size == 0, f"{what} fill_desc hint {hint}: {bad.size} pool bytes differ, first (length, head, " \
                              f"got, want): {[self._pool_byte(x, got_pool, want_pool) for x in bad[:8].tolist()]}"
        self.restore()
        return c


def _cuts(rng, lens, cutting):
    """one: no cut.  two_odd: one cut at an odd offset, so that the second
    fragment starts at odd packet parity (the swap16 of its partial sum).
    scatter: test_gpu_desc._scatter's 0-4 random cuts (1-5 pieces), every third
    packet with a cut inside its first 20 bytes."""
    out = []
    for i, L in enumerate(lens.tolist()):
        if cutting == "one" or L < 2:
            cuts = set()
        elif cutting == "two_odd":
            cuts = {1 + 2 * int(rng.integers(0, L // 2))}
        else:
            header_cut = L > 3 and i % 3 == 0
            cuts = set(int(c) for c in rng.integers(0, L + 1, size=int(rng.integers(0, 4 if header_cut else 5))))
            if header_cut:
                cuts.add(int(rng.integers(1, min(L, 20))))
        out.append(sorted(c for c in cuts if 0 < c < L))
    return out


@functools.lru_cache(maxsize=1)
def _desc_case(U):
    """The simple kernel's length set for U, each length once, packed with
    gaps of 0-3 bytes; headers as the sweeps'; the oracle's results."""
    rng = np.random.default_rng(0x5300 + U)
    lens = _unit_lengths(U).astype(np.uint32)
    off, total = synth.pack(lens, seed=0x5310 + U, max_gap=3)
    buf = rng.integers(0, 256, size=int(total) + 1, dtype=np.uint8)
    _write_headers(buf, off, lens)
    seeds = rng.integers(0, 1 << 32, lens.size, dtype=np.uint64).astype(np.uint32)
    mode = native.FILL_IP | native.FILL_L4
    return (buf, off, lens, seeds, oracle.batch_spans(buf, off, lens, seeds), *oracle.batch_ipv4(buf, off, lens),
            oracle.batch_ipv4_fill(buf, off, lens, mode))


@pytest.mark.parametrize("cutting", ["one", "two_odd", "scatter"])
@pytest.mark.parametrize("U", [1, 2, 4])
def test_desc_kernel_every_length(dev, knobs, U, cutting):
    """csum_desc_kernel<U, spans | frames | fill> with U by hint alone
    (launch_desc: `switch (sums ? units_class(max_len) : 1)`; hints 500 /
    1500 / 3000 -> U 1 / 2 / 4): lengths 0 .. U 1024 + 64 and k U 1024 +- 48
    (k = 2, 3), so under U 1 a 3 120-byte packet takes four passes of the unit
    loop (span_packet's for a one-fragment packet, the fragment loop's `for
    (g = c0; g < c1; g += U * kWave)` otherwise and for every fill).  Three
    cuttings (_cuts); the fragments' source addresses cover all 16 alignments
    over the set.  The fill (FILL_IP | FILL_L4) is compared as the whole pool
    against the oracle's filled frames scattered the same way, and as out2."""
    buf, off, lens, seeds, want_spans, want_frames, want_st, want_fill = _desc_case(U)
    rng = np.random.default_rng(0x5400 + 8 * U + len(cutting))
    lay = Lists(rng, buf, off, lens, _cuts(rng, lens, cutting)).device(dev)
    assert lay.aligns == set(range(16))
    npieces = np.diff(lay.first)
    if cutting == "one":
        assert int(npieces.max()) == 1
    elif cutting == "two_odd":
        assert np.all(npieces[lens >= 2] == 2) and np.all(lay.pa[lay.pa > 0] % 2 == 1)
    else:
        assert int(npieces.max()) == 5 and int(((lay.pa > 0) & (lay.pa < 20)).sum()) > lens.size // 4
    knobs()
    c = lay.run(f"desc U {U} {cutting}", UNIT_HINTS[U], _t(seeds.view(np.int32)), want_spans, want_frames, want_st,
                native.FILL_IP | native.FILL_L4, want_fill)
    assert c == 3 * (U * 1024 + 65 + 2 * 97)


# ---------------------------------------------------------------- 2. the hint matrix

class Case:
    """One batch of the matrix: host bytes, the oracle's answers (computed
    once, read-only) and the hints it runs under."""

    def __init__(self, name, buf, off, lens, extra=()):
        self.name, self.buf, self.off, self.lens = name, buf, off.astype(np.uint64), lens.astype(np.uint32)
        self.n = lens.size
        self.seeds = np.random.default_rng(0x5600 + self.n).integers(0, 1 << 32, self.n, dtype=np.uint64).astype(
            np.uint32)
        self.true_max = int(lens.max())
        hints = [0, 1, 20]
        for last in sorted(set(ROW_LAST.values()) | set(UNIT_LAST.values())):
            hints += [last, last + 1]  # the last hint of the smaller instantiation, the first of the larger
        self.hints = hints + [self.true_max, 1 << 20, 0xFFFFFFFF, *extra]
        self._memo = {}
        for a in (self.buf, self.off, self.lens, self.seeds):
            a.setflags(write=False)

    def want(self, key):
        if key not in self._memo:
            a = (self.buf, self.off, self.lens)
            if key == "spans":
                w = oracle.batch_spans(*a, self.seeds)
                self._memo[key] = (w, (w == 0).astype(np.uint8))
            elif key == "frames":
                self._memo[key] = oracle.batch_ipv4(*a)
            elif key[0] == "rss":
                self._memo[key] = oracle.batch_ipv4_rss(*a, mode=key[1])[0]
            else:
                self._memo[key] = oracle.batch_ipv4_fill(*a, key[1])
        return self._memo[key]

    def device(self, dev):
        """(a fresh device batch, its seeds)"""
        return batch.PacketBatch.from_host(self.buf, self.off, self.lens, device=dev), _t(self.seeds.view(np.int32))

    def shared(self, dev):
        """One device batch for the launches that only read it."""
        if "dev" not in self._memo:
            self._memo["dev"] = self.device(dev)
        return self._memo["dev"]


def _header(f, proto, ip_len=None):
    L = f.size if ip_len is None else ip_len
    f[0] = 0x45
    f[2], f[3] = L >> 8, L & 0xFF
    f[6], f[7] = 0, 0
    f[9] = proto


@functools.lru_cache(maxsize=None)
def _mixed_case():
    """About 3 000 packets: the tx generator's frames (test_gpu_parity._tx_frames:
    TCP / UDP / ICMP echo and other ICMP, IP options, fragments, padded,
    truncated, runts), Zipf UDP frames up to 9 000 bytes, some turned into
    protocol 47, hand-made ones of 0, 1, 19, 20, 27 and 28 bytes, a spread of
    2 048 .. 9 000, one of 70 000 and one of 140 000 bytes (over kExactMax =
    131 072); shuffled, packed from an odd offset with gaps of 0-40 bytes."""
    rng = np.random.default_rng(0x5500)
    b0, o0, l0 = _tx_frames(rng, 2300)
    frames = [b0[int(o):int(o) + int(L)].copy() for o, L in zip(o0, l0)]
    b1, o1, l1, _ = synth.mixed_udp_frames(650, seed=0x5501)
    for i, (o, L) in enumerate(zip(o1, l1)):
        f = b1[int(o):int(o) + int(L)].copy()
        if i % 5 == 0:
            f[9] = 47
        frames.append(f)
    for L in (0, 1, 19):
        frames.append(rng.integers(0, 256, size=L, dtype=np.uint8))
    for L, proto in ((20, 17), (27, 17), (28, 17), (28, 6), (2048, 6), (4096, 17), (8191, 6), (9000, 17)):
        f = rng.integers(0, 256, size=L, dtype=np.uint8)
        _header(f, proto)
        frames.append(f)
    order = rng.permutation(len(frames)).tolist()
    for L, at in ((70000, 1000), (140000, 2000)):  # hand-placed, inside the batch
        f = rng.integers(0, 256, size=L, dtype=np.uint8)
        _header(f, 17, ip_len=65535)
        frames.append(f)
        order.insert(at, len(frames) - 1)
    frames = [frames[i] for i in order]
    lens = np.array([f.size for f in frames], np.uint32)
    gaps = rng.integers(0, 41, size=lens.size)
    off = np.zeros(lens.size, np.uint64)
    pos = 1
    for i in range(lens.size):
        pos += int(gaps[i])
        off[i] = pos
        pos += int(lens[i])
    buf = rng.integers(0, 256, size=pos + 5, dtype=np.uint8)
    for o, f in zip(off.tolist(), frames):
        buf[o:o + f.size] = f
    assert 2900 <= lens.size <= 3100 and int(lens.max()) == 140000 and int((off % 2 == 1).sum()) > 1000
    return Case("mixed", buf, off, lens)


@functools.lru_cache(maxsize=None)
def _slot_case():
    """256 frames of at most 1 500 bytes in 2 304-byte slots, data at + 256
    (an mbuf pool): bytes_len / n = 2 304, so the hints 2 240 and 2 241 are
    the two sides of pick_variant's sparse rule, bytes_len / n >= max_len + 64."""
    rng = np.random.default_rng(0x5510)
    n, slot = 256, 2304
    lens = rng.integers(28, 1501, size=n).astype(np.uint32)
    lens[7] = 1500
    fb, fo, _, _ = synth.mixed_udp_frames(n, seed=0x5511, lengths=lens)
    off = np.arange(n, dtype=np.uint64) * slot + 256
    buf = rng.integers(0, 256, size=n * slot, dtype=np.uint8)
    for i in range(n):
        buf[int(off[i]):int(off[i]) + int(lens[i])] = fb[int(fo[i]):int(fo[i]) + int(lens[i])]
    assert buf.size // n == slot
    return Case("slots", buf, off, lens, extra=(buf.size // n - 64, buf.size // n - 63))


CASES = {"mixed": _mixed_case, "slots": _slot_case}


def _eq(what, got, want):
    assert got.shape == want.shape, what
    ne = got != want
    bad = np.nonzero(ne.any(axis=1) if ne.ndim == 2 else ne)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.shape[0]} differ, first (index, got, want): " + str(
        [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:8]])


@pytest.mark.parametrize("family", [0, 1, 2, 14, 15, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_hint_matrix_spans(dev, knobs, case, family):
    """sccsum_spans (seeded, with status) under every hint, per kernel family."""
    c = CASES[case]()
    b, sd = c.shared(dev)
    want, want_st = c.want("spans")
    knobs(variant=family)
    for hint in c.hints:
        st = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=dev)
        out = batch.spans(_hinted(b, hint), seeds=sd, status=st)
        torch.cuda.synchronize()
        _eq(f"{case} family {family} hint {hint} out", batch.as_u16(out), want)
        _eq(f"{case} family {family} hint {hint} status", st.cpu().numpy(), want_st)


@pytest.mark.parametrize("family", [0, 1, 2, 14, 15, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_hint_matrix_frames(dev, knobs, case, family):
    """sccsum_ipv4_frames, with out2 and status and verify-only (status alone)."""
    c = CASES[case]()
    b, _ = c.shared(dev)
    want, want_st = c.want("frames")
    knobs(variant=family)
    for hint in c.hints:
        hb = _hinted(b, hint)
        st = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=dev)
        out2 = batch.ipv4_frames(hb, status=st)
        st1 = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=dev)
        batch.verify_frames(hb, st1)
        torch.cuda.synchronize()
        _eq(f"{case} family {family} hint {hint} out2", batch.as_u16(out2).reshape(-1, 2), want)
        _eq(f"{case} family {family} hint {hint} status", st.cpu().numpy(), want_st)
        _eq(f"{case} family {family} hint {hint} status alone", st1.cpu().numpy(), want_st)


@pytest.mark.parametrize("family", [0, 1, 2, 15])
@pytest.mark.parametrize("case", list(CASES))
def test_hint_matrix_multi(dev, knobs, case, family):
    """sccsum_spans_multi / sccsum_ipv4_frames_multi: the batch cut into 3 and
    into 16 batches of one launch (under family 0 the row kernel's MQ form)."""
    c = CASES[case]()
    b, sd = c.shared(dev)
    ws, ws_st = c.want("spans")
    wf, wf_st = c.want("frames")
    knobs(variant=family)
    for nb in (3, 16):
        parts = np.array_split(np.arange(c.n), nb)
        for hint in c.hints:
            items, fitems = [], []
            for idx in parts:
                it = torch.from_numpy(idx).to(dev)
                sb = _slice(b, it, hint)
                items.append((sb, None, torch.full((sb.n,), 0xEE, dtype=torch.uint8, device=dev),
                              sd[it].contiguous()))
                fitems.append((sb, None, torch.full((sb.n,), 0xEE, dtype=torch.uint8, device=dev)))
            outs = batch.spans_multi(items)
            fouts = batch.ipv4_frames_multi(fitems)
            torch.cuda.synchronize()
            for k, (idx, item, o, fitem, fo) in enumerate(zip(parts, items, outs, fitems, fouts)):
                what = f"{case} family {family} hint {hint} batch {k} of {nb}"
                _eq(what + " spans out", batch.as_u16(o), ws[idx])
                _eq(what + " spans status", item[2].cpu().numpy(), ws_st[idx])
                _eq(what + " frames out2", batch.as_u16(fo).reshape(-1, 2), wf[idx])
                _eq(what + " frames status", fitem[2].cpu().numpy(), wf_st[idx])


@pytest.mark.parametrize("family", [0, 1, 15])
@pytest.mark.parametrize("case", list(CASES))
def test_hint_matrix_frames_rss(dev, knobs, case, family):
    """sccsum_ipv4_frames_rss, both hash modes: hash, out2 and status."""
    c = CASES[case]()
    b, _ = c.shared(dev)
    want, want_st = c.want("frames")
    knobs(variant=family)
    for mode in (native.RSS_DISPATCH, native.RSS_REASSEMBLED):
        want_h = c.want(("rss", mode))
        for hint in c.hints:
            st = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=dev)
            out2, h = batch.ipv4_frames_rss(_hinted(b, hint), mode=mode, status=st)
            torch.cuda.synchronize()
            what = f"{case} family {family} mode {mode} hint {hint}"
            _eq(what + " hash", h.cpu().numpy().view(np.uint32), want_h)
            _eq(what + " out2", batch.as_u16(out2).reshape(-1, 2), want)
            _eq(what + " status", st.cpu().numpy(), want_st)


@pytest.mark.parametrize("family", [0, 15, 16])
@pytest.mark.parametrize("passes", [1, 2], ids=["one_pass", "two_pass"])
@pytest.mark.parametrize("mode", list(FILL_MODES))
def test_hint_matrix_fill(dev, knobs, mode, passes, family):
    """sccsum_ipv4_fill, every mode, in one pass and in two
    (sccsum_set_fill_single_max, as conftest's fill_passes), both batches: the
    buffer is restored before each hint, then the whole buffer, out2 and the
    status are the oracle's.  The 140 000-byte frame: hints 0 and above
    kExactMax run the flat kernel (its exact redo); smaller hints, under
    family 0 in one pass, the row kernel's `FILL && huge` branch."""
    m = FILL_MODES[mode]
    knobs(variant=family, fill_single_max=1 << 30 if passes == 1 else 0)
    for case in CASES:
        c = CASES[case]()
        b, _ = c.device(dev)
        orig = b.data.clone()
        want_buf, want2, want_st = c.want(("fill", m))
        for hint in c.hints:
            b.data.copy_(orig)
            out2 = torch.full((2 * b.n,), -1, dtype=torch.int16, device=dev)
            st = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=dev)
            batch.ipv4_fill(_hinted(b, hint), m, out2=out2, status=st)
            torch.cuda.synchronize()
            what = f"{case} {mode} passes {passes} family {family} hint {hint}"
            _eq(what + " out2", batch.as_u16(out2).reshape(-1, 2), want2)
            _eq(what + " status", st.cpu().numpy(), want_st)
            _eq(what + " bytes", b.data.cpu().numpy()[: c.buf.size], want_buf)


@pytest.mark.parametrize("case", list(CASES))
def test_hint_matrix_desc(dev, knobs, case):
    """sccsum_spans_desc / sccsum_ipv4_frames_desc / sccsum_ipv4_fill_desc
    (FILL_IP | FILL_L4 | FILL_ICMP_ECHO) on the batch cut _scatter-style."""
    c = CASES[case]()
    rng = np.random.default_rng(0x5700 + c.n)
    lay = Lists(rng, c.buf, c.off, c.lens, _cuts(rng, c.lens, "scatter")).device(dev)
    m = FILL_MODES["ip_l4_icmp_echo"]
    knobs()
    sd = _t(c.seeds.view(np.int32))
    for hint in c.hints:
        lay.run(f"{case} desc", hint, sd, c.want("spans")[0], *c.want("frames"), m, c.want(("fill", m)))


def _engine_run(eng, stream, submit, steps):
    """Start, submit every step, wait for every step, stop; close() (the
    caller's) raises if the run left a step undone."""
    eng.start(stream)
    try:
        ids = [submit(s) for s in steps]
        for i in ids:
            eng.wait(i)
    finally:
        eng.stop()
        stream.synchronize()


@pytest.mark.parametrize("kind", ["spans", "frames"])
def test_hint_matrix_engine_submit(dev, knobs, kind):
    """sccsum_engine_submit: one run, one step per hint and batch, all waited.
    The header sets no length limit for a step's packets (the engine runs
    flat_body, whose phase D redoes a packet over kExactMax exactly), so the
    140 000-byte frame stays."""
    knobs()
    steps = []
    for case in CASES:
        c = CASES[case]()
        b, sd = c.shared(dev)
        for hint in c.hints:
            out = torch.full(((2 if kind == "frames" else 1) * b.n,), -1, dtype=torch.int16, device=dev)
            st = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=dev)
            item = (_hinted(b, hint), out, st) + ((sd,) if kind == "spans" else ())
            steps.append((f"{case} engine {kind} hint {hint}", c, item))
    torch.cuda.synchronize()
    eng = batch.Engine(0, frames=kind == "frames", ring_slots=64, max_in_flight=4)
    _engine_run(eng, torch.cuda.Stream(device=dev), lambda s: eng.submit([s[2]]), steps)
    for what, c, item in steps:
        want, want_st = c.want(kind)
        got = batch.as_u16(item[1])
        _eq(what + " out", got.reshape(-1, 2) if kind == "frames" else got, want)
        _eq(what + " status", item[2].cpu().numpy(), want_st)
    eng.close()


@pytest.mark.parametrize("passes", [1, 2], ids=["one_pass", "two_pass"])
def test_hint_matrix_engine_fill(dev, knobs, passes):
    """sccsum_engine_submit_fill (FILL_IP | FILL_L4 | FILL_ICMP_ECHO): one run,
    one fill per hint and batch, each on its own copy of the frames (the
    140 000-byte frame included)."""
    m = FILL_MODES["ip_l4_icmp_echo"]
    knobs(fill_single_max=1 << 30 if passes == 1 else 0)
    steps = []
    for case in CASES:
        c = CASES[case]()
        for hint in c.hints:
            b, _ = c.device(dev)
            out2 = torch.full((2 * b.n,), -1, dtype=torch.int16, device=dev)
            st = torch.full((b.n,), 0xEE, dtype=torch.uint8, device=dev)
            steps.append((f"{case} engine fill passes {passes} hint {hint}", c, (_hinted(b, hint), out2, st)))
    torch.cuda.synchronize()
    eng = batch.Engine(0, frames=True, fill=True, ring_slots=128, max_in_flight=4)
    _engine_run(eng, torch.cuda.Stream(device=dev), lambda s: eng.submit_fill([s[2]], m), steps)
    for what, c, (b, out2, st) in steps:
        want_buf, want2, want_st = c.want(("fill", m))
        _eq(what + " out2", batch.as_u16(out2).reshape(-1, 2), want2)
        _eq(what + " status", st.cpu().numpy(), want_st)
        _eq(what + " bytes", b.data.cpu().numpy()[: c.buf.size], want_buf)
    eng.close()


@pytest.mark.parametrize("gather", [native.GATHER_NONE, native.GATHER_ZERO_COPY], ids=["as_is", "zero_copy"])
@pytest.mark.parametrize("mode", [native.PIPE_SPANS, native.PIPE_IPV4], ids=["spans", "ipv4"])
@pytest.mark.parametrize("case", list(CASES))
def test_hint_matrix_pipeline(dev, knobs, case, mode, gather):
    """HostPipeline.run (sccsum_pipeline_run) from a pinned buffer: chunks copied
    as they lie, and read in place through the fragment-list kernel."""
    c = CASES[case]()
    knobs()
    host = pipeline.pinned_empty(c.buf.size + 64)[: c.buf.size]
    host[:] = c.buf
    want, want_st = c.want("spans" if mode == native.PIPE_SPANS else "frames")
    pl = pipeline.HostPipeline(0, chunk_bytes=1 << 20, chunk_packets=300, depth=3)
    try:
        for hint in c.hints:
            got, st = pl.run(mode, host, c.off, c.lens, seeds=c.seeds if mode == native.PIPE_SPANS else None,
                             status=True, gather=gather, max_len=hint)
            _eq(f"{case} pipeline mode {mode} gather {gather} hint {hint} out", got, want)
            _eq(f"{case} pipeline mode {mode} gather {gather} hint {hint} status", st, want_st)
    finally:
        pl.close()
