"""Where a test's frames lie in one device buffer of W = 2^32 + 2^26 bytes, so
that offsets and addresses with a non-zero high word reach every stack layer.
Host only: the frames' lengths in, (off u64[], length u32[]) and the byte
ranges to write out.  Nothing here holds W bytes.

The buffer has three lines: offset 2^31, offset 2^32, and the offset `absx` at
which the absolute address is a multiple of 2^32.  The clusters are
  0  from offset 0 upwards,
  1-3  about each line (a few hundred KiB on either side),
  4  above 2^32, from 2^32 + 2^25 upwards,
  5  downwards from W: its first frame ends exactly at W.

ONE byte belongs to ONE frame, so one layout holds one frame across each line
(or one that ends on it and one that starts on it).  The position of the line
inside that frame is the layout's *variant*: variant v takes slot (v + j) of
`slots` for line j, and the variants 0 .. len(slots) - 1 together put every
slot on every line.  tests/test_wide_layout.py asserts that, the GPU tests run
every variant.

Everything else is placed for these rules, which check() asserts:
  - the frame starts take all 16 alignments;
  - every 64 consecutive entries of the batch (and of any sub-batch a test
    names) hold offsets below 2^31, in [2^31, 2^32) and at 2^32 or above: no
    wave or tile is uniform in the high word.  The batch keeps the traffic's
    order; a frame's zone goes round-robin with its index;
  - at least 32 frames at o >= 2^32 have a different frame of the same kind
    at o - 2^32 (cluster 0 and the part of cluster 2 above the line are laid
    out in step), so an offset narrowed to 32 bits reads a plausible frame
    inside the buffer;
  - clusters do not overlap and nothing lies outside [0, W)."""
from __future__ import annotations

import types

import numpy as np

P31, P32 = 1 << 31, 1 << 32
W = P32 + (1 << 26)
SLACK = 1 << 24          # allocate W + SLACK bytes; base_shift() says where in them the buffer starts
HALF = 1 << 21           # a cluster keeps within HALF bytes of its anchor on either side
MARGIN = 64              # known bytes written around every cluster
C4 = P32 + (1 << 25)
FRAME_BYTES = (1, 14, 15, 34, 35, 42, 54)   # Ethernet | IP, IP | L4, the end of a UDP and of a 20-byte TCP header
PAIRS = 40


def absx_of(base: int) -> int:
    """The offset whose absolute address is a multiple of 2^32 (as tests/test_gpu_wide.py picks it)."""
    x = (-base) % P32
    return x + P32 if x < (1 << 24) else x


def base_shift(ptr: int) -> int:
    """The first s (a multiple of 4 MiB below SLACK) for which the absolute
    line of a buffer at ptr + s keeps 2 * HALF away from both offset lines."""
    for s in range(0, SLACK, 2 * HALF):
        x = absx_of(ptr + s)
        if min(abs(x - P31), abs(x - P32)) >= 2 * HALF:
            return s
    raise AssertionError("no shift keeps the absolute line apart")


def slots(strip: int = 0, head: int = 0, extra=()) -> list:
    """The places of a line in a frame, for a layer that takes its frames
    `strip` bytes behind the Ethernet frame's start: an int p puts the line in
    front of frame byte p (off = X - p; p = 0 starts on the line, p < 0 lies
    above it with the line in the headroom), "inside" in the payload, "last"
    in front of the last byte, "end" behind it; "edge" is "end" and 0 at once,
    which only frames without headroom can share."""
    pos = sorted({1} | {p - strip for p in FRAME_BYTES if p - strip > 0} | set(extra))
    return pos + ["inside", "last"] + (["edge"] if head == 0 else ["end", 0])


def _inside(length: int, strip: int) -> int:
    hdr = max(54 - strip, 1)
    return hdr + (length - hdr) // 2


def _fits(slot, length: int, strip: int) -> bool:
    if slot == "inside":
        return length - max(54 - strip, 1) >= 3
    if slot in ("last",):
        return length >= 2
    if slot in ("end", "edge"):
        return length >= 1
    return length > max(slot, 0)


class _Cursor:
    def __init__(self, at: int, up: bool, head: int, rng, tight: bool = False):
        self.at, self.up, self.head, self.rng, self.tight = at, up, head, rng, tight
        self.lo = self.hi = at

    def take(self, length: int) -> int:
        gap = 0 if self.tight else int(self.rng.integers(0, 18))
        self.tight = False
        if self.up:
            o = self.at + self.head + gap
            self.at = self.hi = o + length
        else:
            o = self.at - gap - length
            self.at = self.lo = o - self.head
        return o


def place(lengths, base: int, variant: int, slot_list, strip: int = 0, head: int = 0, kinds=None, prefer=None,
          seed: int = 0, none_len: int = 40):
    """lengths[i]: frame i's bytes, None for a frame the test wants past the
    buffer.  head: bytes kept free in front of every frame (tx headroom).
    kinds[i]: what an alias must share; prefer[i]: frames worth a line."""
    assert base % 16 == 0
    rng = np.random.default_rng(0x71DE + 977 * seed + variant)
    n = len(lengths)
    absx = absx_of(base)
    lines = [P31, P32, absx]
    assert min(abs(absx - P31), abs(absx - P32)) >= 2 * HALF, "shift the buffer by base_shift()"
    off = np.zeros(n, np.uint64)
    length = np.array([none_len if x is None else x for x in lengths], np.uint32)
    real = [i for i in range(n) if lengths[i] is not None]
    for i in range(n):
        if lengths[i] is None:
            off[i] = W + 1 + i
    kinds = [0] * n if kinds is None else kinds
    free = set(real)
    cand = [int(i) for i in rng.permutation(real)] if real else []
    if prefer is not None:
        cand = [i for i in cand if prefer[i]] + [i for i in cand if not prefer[i]]

    def pick(ok):
        for i in cand:
            if i in free and ok(i):
                free.discard(i)
                return i
        raise AssertionError("no frame left that fits")

    # ---- one slot per line
    special, occupied = {}, {}
    for j, X in enumerate(lines):
        slot = slot_list[(variant + j) % len(slot_list)]
        got, lo, hi = [], X, X
        if slot in ("end", "edge"):
            i = pick(lambda i: _fits("end", int(length[i]), strip))
            off[i] = X - int(length[i])
            got.append(i)
            lo = int(off[i]) - head
        if slot != "end":
            sl = 0 if slot == "edge" else slot
            i = pick(lambda i: _fits(sl, int(length[i]), strip))
            L = int(length[i])
            p = _inside(L, strip) if sl == "inside" else L - 1 if sl == "last" else sl
            off[i] = X - p
            got.append(i)
            lo, hi = min(lo, X - p - head), X - p + L
        special[X] = (slot, got)
        occupied[X] = (lo, hi)

    # ---- the frame at the buffer's start, then the alias pairs: cluster 0 and above 2^32 in step
    f0 = pick(lambda i: length[i] >= 1)
    off[f0] = head
    s = max(head + int(length[f0]), occupied[P32][1] - P32)
    pairs, waiting = [], {}
    for i in cand:
        if len(pairs) == PAIRS:
            break
        if i not in free or length[i] < 1:
            continue
        if kinds[i] in waiting:
            a = waiting.pop(kinds[i])
            free.discard(a), free.discard(i)
            o = s + head + int(rng.integers(0, 18))
            off[a], off[i] = o, P32 + o
            s = o + int(max(length[a], length[i]))
            pairs.append((a, i))
        else:
            waiting[kinds[i]] = i

    # ---- the rest, a zone after the other
    def cur(at, up, tight=False):
        return _Cursor(at, up, head, rng, tight)
    low0, up31, dn31 = cur(s, True), cur(occupied[P31][1], True), cur(occupied[P31][0], False)
    up32, dn32 = cur(P32 + s, True), cur(occupied[P32][0], False)
    upx, dnx = cur(occupied[absx][1], True), cur(occupied[absx][0], False)
    c4, tail = cur(C4, True), cur(W, False, tight=True)
    zones = [[low0, dn31], [up31, dn32], [up32, c4, tail]]
    zones[0 if absx < P31 else 1 if absx < P32 else 2] += [upx, dnx]
    zones[2] = [tail] + [c for c in zones[2] if c is not tail]      # the first frame of zone 2 ends at W
    count = [0, 0, 0]
    for k, i in enumerate(sorted(free)):
        z = k % 3
        c = zones[z][count[z] % len(zones[z])]
        count[z] += 1
        off[i] = c.take(int(length[i]))
    clusters = [(0, low0.hi), (dn31.lo, up31.hi), (dn32.lo, up32.hi), (dnx.lo, upx.hi), (C4, c4.hi), (tail.lo, W)]
    clusters = sorted((max(a - MARGIN, 0), min(b + MARGIN, W)) for a, b in clusters if b > a)
    return types.SimpleNamespace(off=off, length=length, real=np.array(real, np.int64), lines=lines, absx=absx,
                                 special=special, pairs=pairs, clusters=clusters, head=head, strip=strip, base=base,
                                 slot_list=slot_list, variant=variant, first=f0)


def zone(off) -> np.ndarray:
    off = np.asarray(off, np.uint64)
    return np.where(off >= W, -1, (off >= P31).astype(np.int64) + (off >= P32))


def mixed(off, width: int = 64) -> bool:
    """Every `width` consecutive entries hold all three zones (a batch shorter than that: all of it does)."""
    z = zone(off)
    if z.size < width:
        return True
    for v in range(3):
        c = np.concatenate([[0], np.cumsum(z == v)])
        if np.any(c[width:] - c[:-width] == 0):
            return False
    return True


def line_byte(lay, X: int) -> list:
    """What the line's frames show: for each, (place of the line in the frame, its length)."""
    _, got = lay.special[X]
    return [(X - int(lay.off[i]), int(lay.length[i])) for i in got]


def check(lay, sub=()) -> None:
    """The rules of the module docstring on one layout; `sub`: index arrays of the sub-batches a test hands on."""
    off, length, real = lay.off, lay.length, lay.real
    o, e = off[real].astype(np.int64), off[real].astype(np.int64) + length[real]
    assert o.min() - lay.head == 0 and e.max() == W
    # clusters apart, every frame (with its headroom) inside one, nothing shared between two frames
    cl = lay.clusters
    assert all(a[1] <= b[0] for a, b in zip(cl[:-1], cl[1:])), cl
    assert len(cl) == 6 and cl[0][0] == 0 and cl[-1][1] == W
    starts = np.array([a for a, _ in cl])
    at = np.searchsorted(starts, o - lay.head, side="right") - 1
    assert np.all(e <= np.array([b for _, b in cl])[at]) and np.all(at >= 0)
    for (a, b), X in zip(cl[1:4], sorted(lay.lines)):
        assert X - HALF < a < X < b < X + HALF, (a, X, b)
    srt = np.lexsort((e, o))                                   # an empty frame may start where its neighbour does
    assert np.all(e[srt][:-1] <= (o - lay.head)[srt][1:]), "two frames share a byte"
    assert set((o % 16).tolist()) == set(range(16))
    # one slot per line, as the variant says
    assert (lay.base + lay.absx) % P32 == 0 and lay.lines == [P31, P32, lay.absx]
    for j, X in enumerate(lay.lines):
        slot, got = lay.special[X]
        assert slot == lay.slot_list[(lay.variant + j) % len(lay.slot_list)]
        seen = line_byte(lay, X)
        if slot == "edge":
            assert [p == L for p, L in seen] == [True, False] and seen[1][0] == 0
        elif slot == "end":
            assert seen[0][0] == seen[0][1]
        elif slot == "last":
            assert seen[0][0] == seen[0][1] - 1 >= 1
        elif slot == "inside":
            assert max(54 - lay.strip, 1) < seen[0][0] < seen[0][1] - 1
        else:
            assert seen[0][0] == slot and (slot <= 0 or slot < seen[0][1])
        inner = [(p, L) for p, L in seen if 0 < p < L]
        assert len(inner) == (0 if slot in ("edge", "end", 0) or (isinstance(slot, int) and slot < 0) else 1)
        crossing = np.flatnonzero((o < X) & (e > X))
        assert crossing.size == len(inner)
    # aliases: another frame of the batch starts exactly 2^32 below
    assert len(lay.pairs) >= 32
    for a, b in lay.pairs:
        assert a != b and int(off[b]) >= P32 and int(off[b]) - P32 == int(off[a])
    # no wave or tile uniform in the high word
    assert mixed(off), "the whole batch"
    for k, ix in enumerate(sub):
        assert mixed(off[np.asarray(ix, np.int64)]), ("sub-batch", k)
    for z in range(3):
        assert int((zone(off) == z).sum()) >= 8


def images(lay, frames, seed: int = 0) -> list:
    """(start, bytes) of every cluster: random bytes with the frames in place."""
    rng = np.random.default_rng(0x1A6E + seed)
    out = [(a, rng.integers(0, 256, b - a, dtype=np.uint8)) for a, b in lay.clusters]
    starts = np.array([a for a, _ in out])
    for i in lay.real.tolist():
        o = int(lay.off[i])
        c = int(np.searchsorted(starts, o, side="right")) - 1
        a, img = out[c]
        img[o - a:o - a + len(frames[i])] = np.frombuffer(frames[i], np.uint8)
    return out


def variants(slot_list) -> range:
    return range(len(slot_list))
