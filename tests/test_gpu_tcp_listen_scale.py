"""sccsum_tcp_listen on 2^18 SYNs of distinct peers and 2^10 scattered segments
that are no SYN, against the numpy restatement (tests/tcp_listen_fast.py).
The host test first pins that restatement, on the same generator's small
buckets, to the per-segment model byte for byte."""
import numpy as np
import pytest

import tcp_listen_fast as fast
import tcp_listen_model as lm
import tcp_listen_traffic as tr
from seastar_amd import native

NAMES = ("cls", "new", "synack", "sa_off", "sa_len", "sa_out", "rst", "rst_dst", "total")
# the interface's words for the model's: both tests here are about that interface
assert (native.TCP_LISTEN_NEW, native.TCP_LISTEN_RESET, native.TCP_LISTEN_DROP, native.TCP_LISTEN_LATER) == \
    (lm.NEW, lm.RESET, lm.DROP, lm.LATER)


@pytest.mark.parametrize("n_syn,n_other", [(1 << 11, 1 << 5), (3000, 100)])
def test_the_restatement_equals_the_model_on_small_buckets(n_syn, n_other):
    a, space = tr.scale_arrays(n_syn, n_other, seed=n_other)
    segs = tr.segs_of(a)
    assert len(segs) == n_syn + n_other and len({s.connid for s in segs}) == len(segs)
    for offload in (False, True):
        want = lm.expect(segs, space, tr.KEY, tr.ISN_M, tr.MTU, offload, strict=True)
        got = fast.expect(a, tr.space_array(space), tr.KEY, tr.ISN_M, tr.MTU, offload)
        for name in NAMES:
            assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    t = want["total"].tolist()
    assert t[0] == len(segs) and t[1] > n_syn // 2 and t[2] > n_syn // 4 and t[3] > n_other // 4
    assert len(set(want["new"]["flags"].tolist())) >= 4 and len({bytes(s) for s in want["synack"]}) == 3


@pytest.mark.gpu
def test_a_quarter_million_syns(dev):
    from test_gpu_tcp_listen import check, run_listen

    a, space = tr.scale_arrays(1 << 18, 1 << 10)
    want = fast.expect(a, tr.space_array(space), tr.KEY, tr.ISN_M, tr.MTU, True)
    t = want["total"].tolist()
    assert t[0] == (1 << 18) + (1 << 10) and t[1] > 1 << 17 and t[2] > 1 << 16 and t[3] > 1 << 8
    assert np.unique(want["new"]["iss"]).size > 0.99 * t[1]
    check(run_listen(dev, a, space, flags=1), want)
