"""A Python restatement of the reference's IPv4 reassembly, the expectation of
the rx reassembly tests (paths relative to the reference tree):

  packet_merger::merge            include/seastar/net/packet-util.hh:45-151, all six
                                  cases and the second pass, for any fragment sequence
  ipv4::frag::merge / is_complete src/net/ip.cc:412-437
  ipv4::handle_received_packet    src/net/ip.cc:164-220: a key's state, completion after
                                  every fragment, erase on completion

A packet is a list of pieces (record, from, len): bytes [from, from + len) of
record's payload.  tests/test_reasm_ref.py checks Merger against the reference's
own packet_merger (tests/cpp/reasm_ref.cc), tests/golden/reasm.json pins it
where the reference tree does not exist.  Nothing here reads the code under
test."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np


def plen(p) -> int:
    return sum(ln for _, _, ln in p)


def trim_front(p, n: int):
    """packet::trim_front: drop the first n bytes."""
    if n == 0:
        return p
    out = []
    for rec, frm, ln in p:
        if n > 0 and n >= ln:
            n -= ln
            continue
        out.append((rec, frm + n, ln - n))
        n = 0
    return out


class Merger:
    """packet_merger<uint32_t, Tag>: self.map[offset] = [packet, its length]
    (the length kept beside the pieces, so that a merge does not walk a long
    packet to measure it)."""

    def __init__(self):
        self.map = {}

    def merge(self, offset: int, p) -> None:
        p = list(p)
        n = plen(p)
        insert = True
        beg = offset
        end = beg + n
        for seg_beg in sorted(self.map):
            seg, seg_len = self.map[seg_beg]
            seg_end = seg_beg + seg_len
            if seg_beg <= beg and end <= seg_end:          # 1) we already have the data
                return
            elif beg <= seg_beg and seg_end <= end:        # 2) the new one holds more: replace
                del self.map[seg_beg]
                insert = True
                break
            elif beg < seg_beg and seg_beg <= end and end <= seg_end:   # 3) new + trimmed old
                trim = end - seg_beg
                p = p + list(trim_front(seg, trim))
                n += seg_len - trim
                del self.map[seg_beg]
                insert = True
                break
            elif seg_beg <= beg and beg <= seg_end and seg_end < end:   # 4) old + trimmed new
                trim = seg_end - beg
                seg.extend(trim_front(p, trim))
                self.map[seg_beg][1] = seg_len + n - trim
                insert = False
                break
            else:                                           # 5) / 6) apart: keep looking
                insert = True
        if insert and beg not in self.map:                  # map.emplace does not overwrite
            self.map[beg] = [p, n]
        # second pass: merge adjacent segments
        keys = sorted(self.map)
        it = 0
        while it + 1 < len(keys):
            seg_beg, nxt = keys[it], keys[it + 1]
            first = self.map[seg_beg]
            seg_end = seg_beg + first[1]
            q, q_len = self.map[nxt]
            b, e = nxt, nxt + q_len
            if seg_beg <= b and b <= seg_end and seg_end < e:
                trim = seg_end - b
                first[0].extend(trim_front(q, trim))
                first[1] += q_len - trim
                del self.map[nxt]
                del keys[it + 1]
            elif e <= seg_end:
                del self.map[nxt]
                del keys[it + 1]
            elif seg_end < b:
                it += 1
            else:
                raise AssertionError("packet_merger would abort")

    def segments(self):
        """[(offset, packet), ...] in offset order (copies)."""
        return [(k, list(self.map[k][0])) for k in sorted(self.map)]

    def whole(self):
        """The one packet at offset 0 when that is all the map holds, else None."""
        return self.map[0][0] if len(self.map) == 1 and 0 in self.map else None


@dataclass
class Datagram:
    key: tuple          # (src, dst, id, proto)
    pieces: list        # (record index, from, len) in datagram order
    head: int           # the record whose IP header frag::merge kept (the last offset-0 one)
    last: int           # the record that completed it
    length: int


@dataclass
class Frag:
    data: Merger = field(default_factory=Merger)
    last_frag_received: bool = False
    header: int = -1
    records: list = field(default_factory=list)


def run(records) -> tuple:
    """ip.cc:164-220 over records in arrival order; a record is any object or
    numpy row with src, dst, id, proto, mf, offset, len.  Returns (delivered
    datagrams in delivery order, {key: Frag} of what stays held)."""
    frags, out = {}, []
    for i, r in enumerate(records):
        key = (int(r["src"]), int(r["dst"]), int(r["id"]), int(r["proto"]))
        f = frags.setdefault(key, Frag())
        if not int(r["mf"]):
            f.last_frag_received = True
        off, ln = int(r["offset"]), int(r["len"])
        if off == 0:
            f.header = i
        f.records.append(i)
        f.data.merge(off, [(i, 0, ln)])
        whole = f.data.whole()
        if f.last_frag_received and whole is not None:   # is_complete
            out.append(Datagram(key, list(whole), f.header, i, plen(whole)))
            del frags[key]
    return out, frags


def buckets(records, mix=None) -> np.ndarray:
    """The bucket of every record by the interface's definition (sccsum.h, "Rx
    reassembly"): 1 complete, 2 pending, 3 host — from offsets, lengths and MF
    alone, not from a merge.  mix(key): keys of one mix are grouped together,
    and a group of more than one key is host whole."""
    by_key = {}
    for i, r in enumerate(records):
        by_key.setdefault((int(r["src"]), int(r["dst"]), int(r["id"]), int(r["proto"])), []).append(i)
    state = np.zeros(len(records), np.uint8)
    groups = {}
    for key in by_key:
        groups.setdefault(mix(key) if mix else key, []).append(key)
    for keys in groups.values():
        for key in keys:
            idx = sorted(by_key[key], key=lambda i: (int(records[i]["offset"]), i))
            beg = [int(records[i]["offset"]) for i in idx]
            end = [b + int(records[i]["len"]) for b, i in zip(beg, idx)]
            mf = [int(records[i]["mf"]) for i in idx]
            plain = (all(e > b for b, e in zip(beg, end)) and all(end[j] <= beg[j + 1] for j in range(len(idx) - 1))
                     and all(mf[:-1]))
            whole = beg[0] == 0 and all(end[j] == beg[j + 1] for j in range(len(idx) - 1)) and not mf[-1]
            state[idx] = 3 if (not plain or len(keys) > 1) else 1 if whole else 2
    return state


# ---------------------------------------------------------------- seeded merger sequences

def payload_byte(rec: int, pos: int) -> int:
    """Byte `pos` of record `rec`'s payload in the merger checks (the driver computes the same)."""
    return (((rec + 1) * 2654435761 + pos * 40503) >> 7) & 0xFF


def packet_bytes(p) -> bytes:
    return bytes(payload_byte(rec, frm + k) for rec, frm, ln in p for k in range(ln))


def crc(p) -> int:
    return zlib.crc32(packet_bytes(p))


def _cut(rng, total: int, pieces: int) -> list:
    """[0, total) cut at multiples of 8 into at most `pieces` (offset, len)."""
    marks = sorted({0, *(8 * int(x) for x in rng.integers(1, max(2, total // 8 + 1), size=pieces - 1)
                         if 0 < 8 * int(x) < total)})
    return [(a, b - a) for a, b in zip(marks, marks[1:] + [total])]


def seeded_sequences(seed: int, count: int) -> list:
    """(kind, [(offset, len, mf), ...]) merger inputs: plain ones (pieces that
    tile, or tile with a hole, in a random permutation) and every non-plain
    kind: overlapping, duplicate, nested, zero-length and late (data past the
    last fragment)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kinds = ("plain", "plain", "plain_hole", "overlap", "duplicate", "nested", "zero", "late")
    out = []
    for t in range(count):
        kind = kinds[t % len(kinds)]
        total = int(rng.integers(1, 25)) * 8 + int(rng.integers(0, 8))
        cuts = _cut(rng, total, int(rng.integers(1, 8)))
        seq = [(o, ln, 1 if o + ln < total else 0) for o, ln in cuts]
        if kind == "plain_hole" and len(seq) > 1:
            del seq[int(rng.integers(0, len(seq)))]
        elif kind == "overlap":
            for _ in range(int(rng.integers(1, 4))):
                o = 8 * int(rng.integers(0, total // 8 + 1))
                ln = int(rng.integers(1, 41))
                seq.append((o, ln, int(rng.integers(0, 2)) if o + ln >= total else 1))
        elif kind == "duplicate":
            for _ in range(int(rng.integers(1, 3))):
                seq.append(seq[int(rng.integers(0, len(seq)))])
        elif kind == "nested":
            o, ln, mf = seq[int(rng.integers(0, len(seq)))]
            if ln > 8:
                seq.append((o + 8 * int(rng.integers(0, ln // 8)), int(rng.integers(1, 9)), 1))
            seq.append((0, total, 0))
        elif kind == "zero":
            seq.append((8 * int(rng.integers(0, total // 8 + 2)), 0, int(rng.integers(0, 2))))
        elif kind == "late":
            seq.append((8 * ((total + 7) // 8) + 8 * int(rng.integers(0, 3)), int(rng.integers(1, 17)), 1))
        order = rng.permutation(len(seq))
        out.append((kind, [seq[int(k)] for k in order]))
    return out


def merge_trace(seq) -> list:
    """The merger's map after every fragment of seq: per step [(beg, packet), ...]."""
    m, steps = Merger(), []
    for i, (off, ln, _) in enumerate(seq):
        m.merge(off, [(i, 0, ln)])
        steps.append(m.segments())
    return steps


def trace_summary(steps) -> list:
    """A trace as recorded data: per step [[beg, len, crc32 of the bytes], ...]."""
    return [[[beg, plen(p), crc(p)] for beg, p in segs] for segs in steps]
