"""sccsum_tcp_rx_data past one chunk of its carry kernels: 1 049 607 records
(1 024 tiles + 1 tile + 7) in three layouts, compared with the whole-array
restatement tests/tcp_data_fast.py, which tests/test_tcp_data_fast.py pins to
the per-segment model.  The records are fabricated with numpy: runs in
sequence, every seventh one (and the long ones at a far segment) leaving the
straight path by a gap, a FIN, a new ACK or a pure ACK."""
import numpy as np
import pytest

import tcp_data_fast as fast
import tcp_data_traffic as tr
from test_gpu_tcp_data import BASE, check, run_data

pytestmark = pytest.mark.gpu

N = 1025 * tr.TILE + 7
M32 = 0xFFFFFFFF


def fabricate(lengths, seed: int) -> dict:
    """Runs of the given lengths as tcp_rx leaves them, run k of connection k."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    r, n0 = lengths.size, int(lengths.sum())
    start = np.cumsum(lengths) - lengths
    run_of = np.repeat(np.arange(r), lengths)
    rcv = np.zeros(r, dtype=tr.RCV_DTYPE)
    rcv["next"] = rng.integers(0, 1 << 32, r)
    rcv["room"] = 1 << 30
    rcv["cap"] = 29200 << 7
    rcv["window"] = rcv["cap"]
    rcv["snd_una"] = rng.integers(0, 1 << 32, r)
    rcv["mss"] = 1000
    rcv["flags"] = 1 | (rng.integers(0, 4, r) << 1)
    rcv["flags"][np.arange(r) % 41 == 40] &= 0xFE                    # not eligible
    seg = np.zeros(n0 + 3, dtype=tr.SEG_DTYPE)
    s = seg[:n0]
    s["pay_len"] = rng.choice([1000, 1000, 999, 1001, 1, 700], n0)   # under 2^30 in all: the room lasts
    s["conn"] = run_of
    s["flags"] = 0x10 | (rng.integers(0, 2, n0) << 3)
    s["ack"] = rcv["snd_una"][run_of]
    s["pay_off"] = np.cumsum(s["pay_len"].astype(np.uint64) + 3)
    # the departures: every seventh run, at a segment that depends on the run; the long runs far in
    odd = np.flatnonzero((np.arange(r) % 7 == 3) | (lengths > 100000))
    at = start[odd] + np.where(lengths[odd] > 100000, lengths[odd] - 12345, (odd // 7) % lengths[odd])
    kind = (odd // 7) % 4
    s["flags"][at[kind == 1]] |= 0x01
    s["ack"][at[kind == 2]] += 1
    s["pay_len"][at[kind == 3]] = 0
    length = s["pay_len"].astype(np.int64)
    cs = np.cumsum(length) - length
    s["seq"] = (rcv["next"].astype(np.int64)[run_of] + cs - cs[start][run_of]) & M32
    s["seq"][at[kind == 0]] += 5
    seg[n0:]["conn"] = 0xFFFFFFFF
    return dict(seg=seg, rcv=rcv, run_conn=np.arange(r, dtype=np.uint32),
                run_first=np.concatenate([start, [n0]]).astype(np.uint32),
                first=np.array([0, n0, n0 + 1, n0 + 3, n0 + 3], dtype=np.uint32), n=n0 + 3, n0=n0, nconns=r,
                rx_total=np.array([r, 2, 0, 0], dtype=np.uint64))


LAYOUTS = {
    "one_run": [N],
    "runs_of_3": [3] * (N // 3) + [N % 3 or 3],
    "long_between_short": [2, 5, 1, 1 << 20, 3, 1, 4] + [9] * ((N - (1 << 20) - 16) // 9) + [(N - (1 << 20) - 16) % 9 or 9],
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_a_million_records_against_the_restatement(dev, layout):
    lengths = LAYOUTS[layout]
    a = fabricate(lengths, len(layout))
    assert a["n0"] >= N and (a["n0"] + tr.TILE - 1) // tr.TILE > 1024    # the carry kernels' second chunk
    want = fast.rx_data(a["seg"], a["first"], a["run_conn"], a["run_first"], a["rcv"], M32, BASE)
    taken = int(want["total"][0])
    assert 0.3 * a["n0"] <= taken < a["n0"]
    if layout == "one_run":
        assert want["run"]["taken"].tolist() == [N - 12345] and want["run"]["stop"][0] == 3
    check(run_data(dev, a), want, layout)
    # the capacity in the far tiles: the cut behind the carry kernels' first chunk
    cap = int(want["total"][1]) - 50000
    if cap <= M32:
        check(run_data(dev, a, cap), fast.rx_data(a["seg"], a["first"], a["run_conn"], a["run_first"], a["rcv"], cap,
                                                  BASE), (layout, cap))
