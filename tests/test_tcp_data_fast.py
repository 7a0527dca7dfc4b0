"""tests/tcp_data_fast.py (the whole-array restatement the scale test compares
with) pinned to the per-segment model on the traffic of the GPU tests."""
import numpy as np
import pytest

import tcp_data_fast as fast
import tcp_data_traffic as tr

M32 = 0xFFFFFFFF


def _same(got: dict, want: dict, what) -> None:
    assert got["total"].tolist() == want["total"].tolist(), what
    for name in tr.RUN_DTYPE.names:
        assert np.array_equal(got["run"][name], want["run"][name]), (what, name)
    assert got["desc"].tobytes() == want["desc"].tobytes(), what


def _fast(a: dict, max_bytes: int = M32, base: int = 0) -> dict:
    return fast.rx_data(a["seg"], a["first"], a["run_conn"], a["run_first"], a["rcv"], max_bytes, base)


@pytest.mark.parametrize("n", [0, 1, 65, 1024, 2 * tr.TILE + 7])
def test_fast_is_the_model_on_mixed_traffic(n):
    cases = tr.mixed(n % 5, n)
    a = tr.arrays(cases)
    free = tr.expect(cases, base=77)
    _same(_fast(a, base=77), free, n)
    total = int(free["total"][1])
    for max_bytes in (0, total // 3, total - 1, total):
        _same(_fast(a, max_bytes, 77), tr.expect(cases, max_bytes, base=77), (n, max_bytes))


def test_fast_is_the_model_on_long_and_single_runs():
    rng = np.random.default_rng(5)
    cases = [tr.stream(rng, 1, tr.KINDS[k % len(tr.KINDS)] if k % 2 else "none", 0, state=k) for k in range(600)]
    _same(_fast(tr.arrays(cases, spare=1, others=0)), tr.expect(cases), "each")
    cases = tr.by_lengths(1, [10, 3000, 3, 3], [None, 2500, None, 1])
    _same(_fast(tr.arrays(cases)), tr.expect(cases), "long")
    t, segs = tr.stream(rng, 20000, lens=[65535] * 20000)      # the room runs out: sums past 2^30
    cases = [(t, segs), tr.stream(rng, 5)]
    _same(_fast(tr.arrays(cases)), tr.expect(cases), "room")


def test_tables_compose_as_the_steps_do():
    """Every pair of steps from every state: the composed table is the two steps in turn."""
    tabs = np.stack([fast.OVER, fast.FULL, fast.SHORT, fast.IDENT])
    for a in tabs:
        for b in tabs:
            c = fast.compose(a[None, :], b[None, :])[0]
            for s in range(4):
                ea = int(a[s])
                eb = int(b[ea & 3])
                assert int(c[s]) == (eb & 3) | ((ea | eb) & 12)
    assert np.array_equal(fast.compose(fast.IDENT[None, :], fast.FULL[None, :])[0], fast.FULL)
    assert np.array_equal(fast.compose(fast.FULL[None, :], fast.IDENT[None, :])[0], fast.FULL)
