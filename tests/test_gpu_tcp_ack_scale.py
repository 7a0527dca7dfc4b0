"""sccsum_tcp_rx_acks on about 2^20 + 1 031 ACKs in three layouts, against
the numpy restatement (tests/tcp_ack_fast.py) that tests/test_tcp_ack_host.py
pins to the per-segment model: one run, runs of three (more runs than one
chunk of the totals block, more queue entries than one chunk of the entry
scans' carry block), and one long run between short ones."""
import functools

import numpy as np
import pytest

import tcp_ack_fast as fast
import tcp_ack_model as am
import tcp_ack_traffic as tr
from test_gpu_tcp_ack import check, run_acks

pytestmark = pytest.mark.gpu

N = (1 << 20) + 1031
LAYOUTS = {
    "one_run": ([N], 0),
    "runs_of_three": ([3] * (N // 3) + [N % 3 or 3], 50),
    "one_long_run_between_short_ones": ([2, 5, 1] * 700 + [N - 2 * 8 * 700] + [2, 5, 1] * 700, 0),
}


@functools.lru_cache(maxsize=1)
def _layout(name: str):
    lengths, dup_every = LAYOUTS[name]
    a = tr.bulk(lengths, sorted(LAYOUTS).index(name), dup_every)
    return a, fast.expect(a)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_a_million_acks(dev, name):
    a, want = _layout(name)
    assert abs(a["n"] - N) <= 3 and int(want["total"][0]) == len(LAYOUTS[name][0])
    taken = int(want["total"][1])
    if name == "runs_of_three":
        assert a["nq"] > 1 << 20 and int(a["rx_total"][0]) > 65536            # the carry blocks' second chunks
        assert 0.9 * a["n"] < taken < a["n"] and am.STOP_ACK in want["run"]["stop"]
    else:
        assert taken == a["n"] and int(want["run"]["taken"].max()) > 1 << 19
    assert int(want["total"][2]) > a["n"] // 8                                # entries popped
    check(run_acks(dev, a), want, name)
