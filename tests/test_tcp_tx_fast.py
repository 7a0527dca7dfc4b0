"""The closed form of the TCP transmit chain against the reference's loop
(tests/tcp_tx_model.py), and its numpy restatement for a batch
(tests/tcp_tx_fast.py) against both, on seeded sweeps.  No GPU, no library."""
import copy

import numpy as np
import pytest

import tcp_tx_fast as fast
import tcp_tx_model as tm
import tcp_tx_traffic as tr

HWS = [tm.Hw(1500), tm.Hw(68), tm.Hw(576), tm.Hw(9000), tm.Hw(1500, True, 65521), tm.Hw(65535), tm.Hw(1500, True, 41)]


def _small(rng) -> tm.Tcb:
    """A tcb whose every quantity is a handful of bytes: the corners meet often."""
    used = int(rng.integers(0, 40))
    nxt = int(rng.choice([5, tm.M32 - 3, tm.M32, 1 << 31]))
    t = tm.Tcb(snd_next=nxt, snd_unacknowledged=(nxt - used) & tm.M32, snd_window=int(rng.integers(0, 60)),
               cwnd=int(rng.integers(0, 25)), mss=int(rng.integers(0, 30)), rtx_armed=bool(rng.integers(0, 2)))
    return t.queue(bytes(rng.integers(0, 256, size=int(n), dtype=np.uint8))
                   for n in rng.integers(0, 12, size=int(rng.integers(0, 8))))


def _livelock(t: tm.Tcb, hw: tm.Hw) -> bool:
    """The reference's chain does not end: segments of no bytes with can_send() > 0 (mss == 0 without TSO)."""
    r = tm.closed_form(t, hw)
    return r.segs == 1 and r.bytes == 0 and min(t.cwnd, hw.seg_len(t.mss)) == 0 and copy.deepcopy(t).can_send() > 0


def _check(t: tm.Tcb, hw: tm.Hw):
    stream = b"".join(t.unsent)
    bufs = list(t.unsent)
    r = tm.closed_form(t, hw)
    if t.why_not_eligible():
        assert (r.segs, r.stop, r.next, r.flags) == (0, tm.STOP_INELIGIBLE, t.snd_next, 0)
        return "ineligible"
    after = copy.deepcopy(t)
    if _livelock(t, hw):
        segs, cut = tm.chain(after, hw, limit=5)
        assert cut and [len(s["payload"]) for s in segs] == [0] * 5 and after.snd_next == t.snd_next
        return "livelock"
    segs, cut = tm.chain(after, hw)
    assert not cut
    assert [s["seq"] for s in segs] == r.seq and [len(s["payload"]) for s in segs] == r.length
    assert b"".join(s["payload"] for s in segs) == stream[:r.bytes]
    assert after.snd_next == r.next and b"".join(after.unsent) == stream[r.bytes:]
    assert after.unsent_len == len(stream) - r.bytes
    assert after.rtx_armed == (t.rtx_armed or bool(r.flags & tm.RTX_ARM))
    assert any(s["armed_here"] for s in segs) == bool(r.flags & tm.RTX_ARM)
    assert after.data == t.data + [(s["seq"], s["payload"]) for s in segs if s["payload"]]
    assert r.stop == (tm.STOP_END if r.bytes == len(stream) else tm.STOP_WINDOW)
    at = 0
    for s in segs:
        assert s["pieces"] == tm.pieces_of(bufs, at, len(s["payload"]))
        assert (s["ack"], s["flags"], s["hdr_len"]) == (t.rcv_next, tm.ACK, 20)
        at += len(s["payload"])
    # the hand-off: the host that applies the record stands where the reference's own walk ends
    mine = tm.continue_from(t, tm.closed_form(t, hw))
    assert (mine.snd_next, mine.unsent_len, mine.rtx_armed, mine.data, b"".join(mine.unsent)) == (
        after.snd_next, after.unsent_len, after.rtx_armed, after.data, b"".join(after.unsent))
    return "pure_ack" if r.bytes == 0 else "data"


@pytest.mark.parametrize("seed", range(4))
def test_closed_form_is_the_loop_on_small_tcbs(seed):
    rng = np.random.default_rng(100 + seed)
    seen = {}
    for _ in range(1500):
        t, hw = _small(rng), HWS[int(rng.integers(0, len(HWS)))]
        k = _check(t, hw)
        seen[k] = seen.get(k, 0) + 1
    assert seen.get("livelock", 0) > 5 and min(seen.get(k, 0) for k in ("pure_ack", "data")) > 100, seen


@pytest.mark.parametrize("seed", range(3))
def test_closed_form_is_the_loop_on_the_traffic(seed):
    seen = set()
    for t in tr.mixed(seed, 400):
        for hw in HWS[:5]:
            seen.add(_check(t, hw))
    assert seen == {"ineligible", "pure_ack", "data"}


def test_ineligible_tcbs_do_something_else():
    """Why the premises are premises: each kind the host keeps leaves the closed form."""
    hw = tm.Hw(1500)
    t = tm.Tcb(dupacks=1, cwnd=1460, mss=1460).queue([bytes(6000)])
    t.data = [(0, bytes(4000))]                       # limited transmit: cwnd + 2 mss - flight, and it is recorded
    segs, _ = tm.chain(t, hw)
    assert [len(s["payload"]) for s in segs] == [380] and t.limited_transfer == 380
    t = tm.Tcb(dupacks=3).queue([bytes(6000)])        # dupacks >= 3: one segment, the chain is not continued
    assert [len(s["payload"]) for s in tm.chain(t, hw)[0]] == [1460]
    t = tm.Tcb(window_probe=True, snd_window=0).queue([bytes(100)])
    segs, cut = tm.chain(t, hw, limit=3)              # the probe: one byte against a closed window
    assert len(segs[0]["payload"]) == 1 and not cut
    t = tm.Tcb(state="FIN_WAIT_1")                    # the FIN rides on the empty segment
    assert tm.chain(t, hw)[0][0]["flags"] == tm.ACK | 0x01
    t = tm.Tcb(packetq=2).queue([bytes(10)])          # queued packets go first: nothing is cut on the first poll
    seg, again = t.get_packet(hw)
    assert seg is None and again
    for t in (tm.Tcb(dupacks=1), tm.Tcb(dupacks=2), tm.Tcb(dupacks=7), tm.Tcb(window_probe=True), tm.Tcb(packetq=1),
              tm.Tcb(state="FIN_WAIT_1"), tm.Tcb(state="SYN_SENT"), tm.Tcb(state="LAST_ACK")):
        assert t.why_not_eligible() and not t.flags() & tm.ELIGIBLE
    assert tm.Tcb().flags() == tm.ELIGIBLE and tm.Tcb(state=tm.CLOSE_WAIT, rtx_armed=True).flags() == 3


# ---------------------------------------------------------------- the numpy restatement

def _against_model(cases, hw, headroom, max_segs=0x7FFFFFFF, max_bytes=tm.M32):
    want = tr.expect(cases, hw, headroom, max_segs, max_bytes)
    a = tr.arrays(cases)
    f = lay = pieces = 0
    cut = False
    for c, t in enumerate(cases):
        r = tm.closed_form(t, hw)
        need = r.bytes + headroom * r.segs
        cut = cut or f + r.segs > max_segs or lay + need > max_bytes
        run = want["run"][c]
        if cut:
            assert (run["segs"], run["bytes"], run["seg_first"], run["next"], run["flags"], run["stop"]) == (
                0, 0, f, t.snd_next, 0, tm.STOP_CAPACITY)
            continue
        assert (run["segs"], run["bytes"], run["seg_first"], run["next"], run["flags"], run["stop"]) == (
            r.segs, r.bytes, f, r.next, r.flags, r.stop), c
        bufs, at = list(t.unsent), 0
        for k in range(r.segs):
            o = want["out"][f]
            assert want["off"][f] == lay + headroom and want["len"][f] == r.length[k] and want["seg_first"][f] == pieces
            assert (o["dst"], o["seq"], o["ack"], o["sport"], o["dport"], o["window"], o["flags"], o["hdr_len"],
                    o["mss"]) == (t.dst, r.seq[k], t.rcv_next, t.sport, t.dport, (t.rcv_window >> t.window_scale) & 0xFFFF,
                                  0x10, 20, t.mss)
            dst = lay + headroom
            for j, inner, n in tm.pieces_of(bufs, at, r.length[k]):
                assert (want["desc_buf"][pieces], want["desc_inner"][pieces], want["desc_dst"][pieces],
                        want["desc_len"][pieces]) == (a["buf_first"][c] + j, inner, dst, n)
                dst += n
                pieces += 1
            at += r.length[k]
            lay += headroom + r.length[k]
            f += 1
    assert want["total"][:3].tolist() == [f, lay, pieces] and want["seg_first"][f] == pieces
    assert want["total"][3] == sum(tm.closed_form(t, hw).bytes + headroom * tm.closed_form(t, hw).segs for t in cases)
    return want


@pytest.mark.parametrize("seed,hw,headroom", [(0, HWS[0], 20), (1, HWS[1], 24), (2, HWS[4], 64), (3, HWS[3], 20)])
def test_fast_is_the_model(seed, hw, headroom):
    cases = tr.mixed(seed, 300)
    want = _against_model(cases, hw, headroom)
    segs, lay = int(want["total"][0]), int(want["total"][1])
    for max_segs, max_bytes in ((segs, lay), (segs - 1, lay), (segs, lay - 1), (segs // 2, lay), (segs, lay // 3), (0, lay),
                                (segs, 0), (segs, headroom)):
        _against_model(cases, hw, headroom, max_segs, max_bytes)


def test_fast_on_small_tcbs():
    rng = np.random.default_rng(9)
    cases = [_small(rng) for _ in range(500)]
    for hw in HWS:
        _against_model(cases, hw, 20)


def test_queue_past_32_bits():
    snd = np.zeros(3, dtype=fast.SND_DTYPE)
    snd["flags"], snd["window"], snd["cwnd"], snd["mss"] = tm.ELIGIBLE, 3000, 1460, 1460
    buf_len = np.array([0xFFFFFFFF, 0xFFFFFFFF, 1, 5], dtype=np.uint32)
    r = fast.expect(snd, buf_len, np.array([0, 1, 3, 4], dtype=np.uint32), 1500, 20)
    assert r["run"]["stop"].tolist() == [tm.STOP_WINDOW, tm.STOP_QUEUE, tm.STOP_END]
    assert r["run"]["segs"].tolist() == [3, 0, 1] and r["len"].tolist() == [1460, 1460, 80, 5]
    assert r["desc_buf"].tolist() == [0, 0, 0, 3] and r["desc_inner"].tolist() == [0, 1460, 2920, 0]
    assert tm.closed_form(tm.Tcb(), tm.Hw(), unsent_len=1 << 32).stop == tm.STOP_QUEUE
