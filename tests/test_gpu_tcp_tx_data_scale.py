"""sccsum_tcp_tx_data past one trip of the segment kernel's grid and past one
chunk of every one-block carry kernel: about 2^20 + 1 031 segments, and more
buffers than 1 024 tiles hold, against the numpy restatement
(tests/tcp_tx_fast.py), in three layouts."""
import numpy as np
import pytest

import tcp_tx_fast as fast
import tcp_tx_model as tm
from seastar_amd import native
from test_gpu_tcp_tx_data import _arrays_of, _expect, _one, check, run_tx

pytestmark = pytest.mark.gpu

SEGS = (1 << 20) + 1031


def _layout(name: str):
    if name == "one_connection":
        # a byte a segment, out of buffers of 0 to 2 bytes: more than 1 024 tiles of buffers too
        sizes = np.tile(np.array([1, 0, 1, 0, 2], dtype=np.uint32), SEGS // 4 + 1)
        return [_one(sizes.tolist(), cwnd=1, snd_window=SEGS)]
    if name == "three_segments_each":
        return [_one([2000, 1500], snd_window=3000 + c % 900) for c in range(SEGS // 3 + 1)]
    short = [_one([700, 700], snd_window=2000)] * 515
    return short + [_one([4096] * 257, cwnd=1, snd_window=1 << 20)] + short


@pytest.mark.parametrize("name", ["one_connection", "three_segments_each", "one_long_between_short"])
def test_past_one_trip_and_one_chunk(dev, name):
    a = _arrays_of(_layout(name))
    want = _expect(a)
    lib = native.load()
    assert want["total"][0] > lib.sccsum_tcp_tx_data_seg_tile() * lib.sccsum_tcp_tx_data_max_blocks()
    assert abs(int(want["total"][0]) - SEGS) < 1100
    if name == "one_connection":
        assert a["buf_len"].size > 1024 * 1024 and want["run"]["stop"][0] == tm.STOP_WINDOW
    check(run_tx(dev, a), want, name)
    cut = _expect(a, max_segs=SEGS // 2)
    check(run_tx(dev, a, max_segs=SEGS // 2), cut, name)
    assert (cut["run"]["stop"] == fast.STOP_CAPACITY).any()
