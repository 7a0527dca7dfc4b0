"""tests/wide_layout.py without a device: every rule of its docstring, on
made-up lengths and on the plans tests/test_gpu_wide_stack.py places, for every
variant and for buffers that start at awkward addresses."""
import numpy as np
import pytest

import test_gpu_wide_stack as ws
import wide_layout as wl
from test_stack_model import modelled
from wide_layout import P31, P32, W

# allocation addresses: a plain one; a multiple of 2^32; the absolute line 2 MiB
# below offset 2^32 and 1 MiB above offset 2^31 (both need the shift); 16 bytes
# below a multiple of 2^32
PTRS = [0x7F12_3456_0000, 0x7F00_0000_0000, 0x7F01_0020_0000, 0x7F00_7FF0_0000, 0x7EFF_FFFF_FFF0]


def _base(ptr: int) -> int:
    s = wl.base_shift(ptr)
    assert 0 <= s < wl.SLACK and s % 16 == 0
    return ptr + s


def _covered(slot_list, strip, lays) -> None:
    """Over the variants, every line saw every slot; the slots are the issue's list."""
    want = {1} | {p - strip for p in wl.FRAME_BYTES if p - strip > 0}
    assert want <= set(slot_list) and {"inside", "last"} <= set(slot_list)
    assert "edge" in slot_list or {"end", 0} <= set(slot_list)
    for j in range(3):
        assert {lay.special[lay.lines[j]][0] for lay in lays} == set(slot_list), j
    for lay in lays:
        for X in lay.lines:
            slot, _ = lay.special[X]
            for p, L in wl.line_byte(lay, X):      # the line really lies there: off + p is the line
                assert 0 <= p <= L or (isinstance(slot, int) and slot < 0 and p == slot)


def test_the_frame_slots_are_the_header_boundaries():
    assert wl.slots() == [1, 14, 15, 34, 35, 42, 54, "inside", "last", "edge"]
    assert wl.slots(14) == [1, 20, 21, 28, 40, "inside", "last", "edge"]       # a layer that takes IP packets
    assert wl.slots(42, 8, extra=(-4,)) == [-4, 1, 12, "inside", "last", "end", 0]
    assert wl.slots(54) == [1, "inside", "last", "edge"]


@pytest.mark.parametrize("ptr", PTRS)
def test_base_shift_keeps_the_lines_apart(ptr):
    base = _base(ptr)
    x = wl.absx_of(base)
    assert (base + x) % P32 == 0 and (1 << 24) <= x < W
    assert min(abs(x - P31), abs(x - P32)) >= 2 * wl.HALF


@pytest.mark.parametrize("ptr", PTRS)
@pytest.mark.parametrize("head", [0, 8, 60])
def test_made_up_lengths(ptr, head):
    rng = np.random.default_rng(head)
    lengths = [int(x) for x in rng.integers(0, 1515, 400)]
    for k in (7, 130, 399):
        lengths[k] = None
    strip = {0: 0, 8: 42, 60: 54}[head]
    slot_list = wl.slots(strip, head, extra=(-4,) if head else ())
    lays = []
    for v in wl.variants(slot_list):
        lay = wl.place(lengths, _base(ptr), v, slot_list, strip=strip, head=head)
        wl.check(lay)
        assert np.all(lay.off[[7, 130, 399]] > W) and lay.length[7] == 40
        lays.append(lay)
    _covered(slot_list, strip, lays)


def _plan_layouts(plan, ptr, slot_list=ws.RX_SLOTS):
    lays = []
    for v in wl.variants(slot_list):
        lay = ws.lay_of(plan, _base(ptr), v, slot_list)
        wl.check(lay, plan.sub)
        lays.append(lay)
    _covered(slot_list, 0, lays)
    return lays


@pytest.mark.parametrize("ptr", PTRS[:3])
@pytest.mark.parametrize("name", ["stack_plan", "udp_plan", "tcp_plan", "tcp_data_plan"])
def test_rx_plans(name, ptr):
    plan = getattr(ws, name)()
    lays = _plan_layouts(plan, ptr)
    for lay in lays:
        # the frames on the lines are frames the layers take: IPv4, with an L4 header
        for X in lay.lines:
            for i in lay.special[X][1]:
                assert plan.prefer[i]
        for a, b in lay.pairs:
            assert plan.kinds[a] == plan.kinds[b] and plan.frames[a] != plan.frames[b]
        imgs = wl.images(lay, plan.frames)
        assert [(a, a + img.size) for a, img in imgs] == lay.clusters
        assert sum(img.size for _, img in imgs) < 8 << 20
        for i in (lay.first, lay.pairs[0][1], lay.special[P32][1][0]):
            a, img = next((a, img) for a, img in imgs if a <= int(lay.off[i]) < a + img.size)
            o = int(lay.off[i]) - a
            assert img[o:o + len(plan.frames[i])].tobytes() == plan.frames[i]


@pytest.mark.parametrize("ptr", PTRS[:2])
def test_stack_plan_has_datagrams_across_2_32(ptr):
    """At least 8 delivered datagrams have fragments on both sides of offset 2^32, in every variant."""
    plan = ws.stack_plan()
    _, outs, _ = modelled(ws.STACK_SEED)
    for lay in _plan_layouts(plan, ptr):
        where = {}
        for o in outs:
            for (b, k), key, *_ in o["frags"]:
                where.setdefault(key, []).append(int(lay.off[int(plan.starts[b]) + k]))
        done = [(d["src"], d["dst"], d["id"], d["proto"]) for o in outs for d in o["delivered"] if d["plain"]]
        across = sum(1 for key in done if key in where and min(where[key]) < P32 <= max(where[key]))
        assert across >= 8, across


@pytest.mark.parametrize("ptr", PTRS[:2])
def test_tx_plans(ptr):
    for plan, slot_list, strip, head in ((ws.udp_send_plan(), ws.UDP_TX_SLOTS, 42, 8),
                                         (ws.tcp_send_plan(), ws.TCP_TX_SLOTS, 54, 60),
                                         (ws.tx_data_plan(), ws.BUF_SLOTS, 54, 0)):
        lays = []
        for v in wl.variants(slot_list):
            lay = ws.lay_of(plan, _base(ptr), v, slot_list, strip=strip, head=head)
            wl.check(lay, plan.sub)
            lays.append(lay)
        _covered(slot_list, strip, lays)
        if head:
            # a payload that starts on each line (its header below it), one 4 bytes above (its header across it)
            for X in lays[0].lines:
                rel = {int(lay.off[i]) - X for lay in lays for i in lay.special[X][1]}
                assert {0, 4} <= rel
        assert set(np.concatenate([lay.off[lay.real] % 16 for lay in lays]).tolist()) == set(range(16))
