"""Every sccsum_*_workspace function that needs no device handle returns the
byte count pinned here.  A caller allocates exactly that many bytes and the
kernels index the arrays a layer lays out inside them, so a change of any
figure is a change of the allocation contract.

EXPECTED was recorded from the library built at the commit before the host
side's workspace layouts moved to host_launch::Carver (the parent of that
commit), by calling every function below on the argument tuples of cases();
the literals never come from the code under test.  A layer that changes its
workspace on purpose records its own new figures the same way, in the commit
that changes it."""
import re

import pytest

from seastar_amd import native

# n: the sizes around one and two tiles of every layer, two large ones
COMMON = (0, 1, 1023, 1024, 1025, 2047, 2049, 1 << 18, 1 << 20)
U32, I31 = (1 << 32) - 1, (1 << 31) - 1
CONNS = native.TCP_MAX_CONNS

# function -> the documented maximum of each argument (include/sccsum.h)
LIMITS = {
    "sccsum_fragments_workspace": (U32,),
    "sccsum_ipv4_send_workspace": (U32,),
    "sccsum_ipv4_reasm_workspace": (I31,),
    "sccsum_eth_rx_workspace": (U32,),
    "sccsum_arp_learn_workspace": (I31,),
    "sccsum_eth_send_workspace": (U32,),
    "sccsum_udp_rx_workspace": (U32,),
    "sccsum_udp_rx_reasm_workspace": (I31,),
    "sccsum_tcp_rx_workspace": (U32, CONNS),
    "sccsum_tcp_rx_data_workspace": (U32, CONNS),
    "sccsum_tcp_tx_data_workspace": (CONNS, 1 << 31),
    "sccsum_tcp_rx_acks_workspace": (U32, CONNS, 1 << 31),
    "sccsum_tcp_listen_workspace": (1 << 30,),
}
# for the functions of several arguments: sizes that differ per argument, either way round
MIXED = {
    "sccsum_tcp_rx_workspace": ((1025, 3), (3, 1025), (1 << 18, 1 << 20)),
    "sccsum_tcp_rx_data_workspace": ((1025, 3), (3, 1025), (1 << 18, 1 << 20)),
    "sccsum_tcp_tx_data_workspace": ((3, 2049), (2049, 3), (1 << 20, 1), (1, 1 << 20), (1025, 0), (0, 1025)),
    "sccsum_tcp_rx_acks_workspace": ((3, 1025, 2049), (1025, 3, 2049), (2049, 1025, 3), (1 << 20, 1, 1 << 18),
                                     (1, 1 << 20, 1 << 18), (0, 1025, 7), (1025, 0, 7), (1025, 7, 0)),
}


def cases(name: str) -> list:
    """The argument tuples of one function: every COMMON size in all arguments
    at once (an argument's own maximum where the size is past it), each
    argument at its maximum and one past it with the others at 1025, and the
    MIXED tuples."""
    limits = LIMITS[name]
    out = [tuple(min(n, m) for m in limits) for n in COMMON]
    for k, m in enumerate(limits):
        for v in (m, m + 1):
            out.append(tuple(v if j == k else 1025 for j in range(len(limits))))
    out += MIXED.get(name, ())
    return list(dict.fromkeys(out))


EXPECTED = {
    "sccsum_fragments_workspace": {
        (0,): 16,
        (1,): 33,
        (1023,): 3087,
        (1024,): 3088,
        (1025,): 3105,
        (2047,): 6159,
        (2049,): 6177,
        (262144,): 786448,
        (1048576,): 3145744,
        (4294967295,): 12884901903,
        (4294967296,): 12884901904,
    },
    "sccsum_ipv4_send_workspace": {
        (0,): 16,
        (1,): 48,
        (1023,): 8224,
        (1024,): 8224,
        (1025,): 8256,
        (2047,): 16432,
        (2049,): 16464,
        (262144,): 2101264,
        (1048576,): 8405008,
        (4294967295,): 34426847248,
        (4294967296,): 34426847248,
    },
    "sccsum_ipv4_reasm_workspace": {
        (0,): 1040,
        (1,): 5424,
        (1023,): 71744,
        (1024,): 71744,
        (1025,): 72016,
        (2047,): 138336,
        (2049,): 138624,
        (262144,): 17180688,
        (1048576,): 68719632,
        (2147483647,): 140735677456,
        (2147483648,): 140735677456,
    },
    "sccsum_eth_rx_workspace": {
        (0,): 16,
        (1,): 160,
        (1023,): 160,
        (1024,): 160,
        (1025,): 160,
        (2047,): 160,
        (2049,): 160,
        (262144,): 9232,
        (1048576,): 36880,
        (4294967295,): 150994960,
        (4294967296,): 150994960,
    },
    "sccsum_arp_learn_workspace": {
        (0,): 16,
        (1,): 32,
        (1023,): 32,
        (1024,): 32,
        (1025,): 32,
        (2047,): 32,
        (2049,): 32,
        (262144,): 1040,
        (1048576,): 4112,
        (2147483647,): 8388624,
        (2147483648,): 8388624,
    },
    "sccsum_eth_send_workspace": {
        (0,): 32,
        (1,): 64,
        (1023,): 64,
        (1024,): 64,
        (1025,): 96,
        (2047,): 96,
        (2049,): 128,
        (262144,): 8224,
        (1048576,): 32800,
        (4294967295,): 134217760,
        (4294967296,): 134217760,
    },
    "sccsum_udp_rx_workspace": {
        (0,): 1024,
        (1,): 5088,
        (1023,): 21440,
        (1024,): 21456,
        (1025,): 21472,
        (2047,): 37824,
        (2049,): 37856,
        (262144,): 4454400,
        (1048576,): 17814528,
        (4294967295,): 72964113392,
        (4294967296,): 72964113408,
    },
    "sccsum_udp_rx_reasm_workspace": {
        (0,): 1024,
        (1,): 5088,
        (1023,): 21440,
        (1024,): 21456,
        (1025,): 21472,
        (2047,): 37824,
        (2049,): 37856,
        (262144,): 4454400,
        (1048576,): 17814528,
        (2147483647,): 36482057200,
        (2147483648,): 36482057216,
    },
    "sccsum_tcp_rx_workspace": {
        (0, 0): 1040,
        (1, 1): 5216,
        (1023, 1023): 62448,
        (1024, 1024): 62496,
        (1025, 1025): 62560,
        (2047, 2047): 119792,
        (2049, 2049): 119904,
        (262144, 262144): 14944272,
        (1048576, 1048576): 59773968,
        (4294967295, 1025): 244829914080,
        (4294967296, 1025): 244829914128,
        (1025, 1048576): 62560,
        (1025, 1048577): 62560,
        (1025, 3): 62560,
        (3, 1025): 5328,
        (262144, 1048576): 14944272,
    },
    "sccsum_tcp_rx_data_workspace": {
        (0, 0): 96,
        (1, 1): 176,
        (1023, 1023): 176,
        (1024, 1024): 176,
        (1025, 1025): 256,
        (2047, 2047): 256,
        (2049, 2049): 336,
        (262144, 262144): 20576,
        (1048576, 1048576): 82016,
        (4294967295, 1025): 335544416,
        (4294967296, 1025): 335544416,
        (1025, 1048576): 256,
        (1025, 1048577): 256,
        (1025, 3): 256,
        (3, 1025): 176,
        (262144, 1048576): 20576,
    },
    "sccsum_tcp_tx_data_workspace": {
        (0, 0): 80,
        (1, 1): 160,
        (1023, 1023): 36944,
        (1024, 1024): 36992,
        (1025, 1025): 37056,
        (2047, 2047): 73856,
        (2049, 2049): 73952,
        (262144, 262144): 9446480,
        (1048576, 1048576): 37785680,
        (1048576, 1025): 25202816,
        (1048577, 1025): 25202864,
        (1025, 2147483648): 25794994336,
        (1025, 2147483649): 25794994352,
        (3, 2049): 24800,
        (2049, 3): 49376,
        (1048576, 1): 25190512,
        (1, 1048576): 12595328,
        (1025, 0): 24736,
        (0, 1025): 12416,
    },
    "sccsum_tcp_rx_acks_workspace": {
        (0, 0, 0): 48,
        (1, 1, 1): 112,
        (1023, 1023, 1023): 20624,
        (1024, 1024, 1024): 20640,
        (1025, 1025, 1025): 20704,
        (2047, 2047, 2047): 41216,
        (2049, 2049, 2049): 41280,
        (262144, 262144, 262144): 5270576,
        (1048576, 1048576, 1048576): 21082160,
        (4294967295, 1025, 1025): 34359750864,
        (4294967296, 1025, 1025): 34359750864,
        (1025, 1048576, 1025): 20704,
        (1025, 1048577, 1025): 20704,
        (1025, 1025, 2147483648): 25794977968,
        (1025, 1025, 2147483649): 25794978000,
        (3, 1025, 2049): 24720,
        (1025, 3, 2049): 32896,
        (2049, 1025, 3): 16608,
        (1048576, 1, 262144): 11537488,
        (1, 1048576, 262144): 3148880,
        (0, 1025, 7): 144,
        (1025, 0, 7): 8352,
        (1025, 7, 0): 8272,
    },
    "sccsum_tcp_listen_workspace": {
        (0,): 263296,
        (1,): 267520,
        (1023,): 320592,
        (1024,): 320608,
        (1025,): 328896,
        (2047,): 373840,
        (2049,): 390336,
        (262144,): 14158912,
        (1048576,): 55845952,
        (1073741824,): 56916968512,
        (1073741825,): 0,
    },
}


def test_every_handle_free_workspace_function_is_pinned():
    declared = set(re.findall(r"uint64_t (sccsum_\w*workspace)\(", open(native.HEADER_PATH).read()))
    assert declared - {"sccsum_steer_workspace"} == set(LIMITS) == set(EXPECTED)
    for name in LIMITS:
        assert list(EXPECTED[name]) == cases(name), name


@pytest.mark.parametrize("name", sorted(LIMITS))
def test_workspace_bytes(name):
    fn = getattr(native.load(), name)
    got = {args: int(fn(*args)) for args in cases(name)}
    assert got == EXPECTED[name]
