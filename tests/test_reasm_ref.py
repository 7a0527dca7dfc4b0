"""Pins tests/reasm_model.py, the expectation of the rx reassembly tests, to
the REFERENCE's own packet_merger (include/seastar/net/packet-util.hh:45-151,
used where it lies): tests/cpp/reasm_ref.cc feeds it seeded fragment sequences
and prints its map after every merge; the model must hold the same segments,
every length and every byte, after every merge.  Also asserts the claim the
device path rests on: a plain key's outcome is the same for every arrival
order.  CPU only; needs /root/reference (build container only)."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_reasm  # noqa: E402
import reasm_model  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(make_reasm.REF_INCLUDE),
                                reason="needs /root/reference (build container only)")

NSEQ = 2400


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("reasm_ref"))
    return make_reasm.build_driver(d), d


def _as_bytes(steps):
    return [[(beg, reasm_model.plen(p), reasm_model.packet_bytes(p)) for beg, p in segs] for segs in steps]


def test_model_matches_the_reference_merger(driver):
    exe, d = driver
    seqs = reasm_model.seeded_sequences(0x0DDBA11, NSEQ)
    kinds = {k for k, _ in seqs}
    assert {"plain", "plain_hole", "overlap", "duplicate", "nested", "zero", "late"} <= kinds
    traces = make_reasm.run_driver(exe, [s for _, s in seqs], d)
    for (kind, seq), want in zip(seqs, traces):
        assert _as_bytes(reasm_model.merge_trace(seq)) == want, (kind, seq)


def _records(seq):
    r = np.zeros(len(seq), dtype=[("src", "<u4"), ("dst", "<u4"), ("id", "<u2"), ("proto", "u1"), ("mf", "u1"),
                                  ("offset", "<u2"), ("len", "<u2")])
    for i, (o, ln, mf) in enumerate(seq):
        r[i] = (1, 2, 3, 17, mf, o, ln)
    return r


def test_plain_keys_do_not_depend_on_arrival_order(driver):
    """For a plain key, every permutation tried leaves the reference's merger
    with the same segments and bytes, and the restated ip.cc:164-220 delivers
    the same datagram (or none), at the last record to arrive."""
    exe, d = driver
    rng = np.random.Generator(np.random.PCG64(77))
    base = [s for k, s in reasm_model.seeded_sequences(0xA11CE, 400) if k in ("plain", "plain_hole")]
    assert len(base) >= 100
    perms, owner = [], []
    for b, seq in enumerate(base):
        seq = sorted(seq)
        assert reasm_model.buckets(_records(seq)).max() <= 2   # plain by the interface's definition
        orders = (list(itertools.permutations(range(len(seq)))) if len(seq) <= 4
                  else [rng.permutation(len(seq)) for _ in range(12)])
        for o in orders:
            perms.append(([seq[int(k)] for k in o], [int(k) for k in o]))
            owner.append(b)
    traces = make_reasm.run_driver(exe, [p for p, _ in perms], d)
    final, delivered = {}, {}
    for (p, order), trace, b in zip(perms, traces, owner):
        assert _as_bytes(reasm_model.merge_trace(p))[-1] == trace[-1]
        # the bytes by original record: the driver numbers records by arrival, so compare offsets and lengths
        segs = [(beg, ln) for beg, ln, _ in trace[-1]]
        assert final.setdefault(b, segs) == segs, p
        out, held = reasm_model.run(_records(p))
        got = None
        if out:
            assert len(out) == 1 and not held and out[0].last == len(p) - 1
            got = [(order[r], frm, ln) for r, frm, ln in out[0].pieces]
            assert all(frm == 0 for _, frm, _ in got)          # only the touching cases fire: nothing is trimmed
        assert delivered.setdefault(b, got) == got, p
        want = reasm_model.buckets(_records(p))
        assert (want == 1).all() == (got is not None)
    assert any(v is not None for v in delivered.values()) and any(v is None for v in delivered.values())
