"""ctypes binding of the C-ABI in include/sccsum.h (libsccsum.so).

There is no fallback: if the library is missing or fails to load, every entry
point raises.  torch is imported before the library is opened so that both
share one HIP runtime (torch ships its own libamdhip64.so.7; our library's
NEEDED entry then resolves to the already-loaded copy).
"""
from __future__ import annotations

import ctypes
import os
import re

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, "lib", "libsccsum.so")
HEADER_PATH = os.path.join(REPO_DIR, "include", "sccsum.h")
DIAG_HEADER_PATH = os.path.join(REPO_DIR, "include", "sccsum_diag.h")

SCCSUM_OK = 0
SCCSUM_EINVAL = -1
SCCSUM_ENODEV = -2
SCCSUM_EBUSY = -3
SCCSUM_EIDLE = -4
SCCSUM_EFAULT = -5
ST_OK = 0x01
ST_L4_OK = 0x02
ST_MALFORMED = 0x04
ST_RANGE = 0x08
ST_IPFRAG = 0x10
FILL_IP = 0x01
FILL_L4 = 0x02
FILL_L4_PSEUDO = 0x04
FILL_TSO = 0x08
FILL_ICMP_ECHO = 0x10
ABI_VERSION = 4


class SccsumError(RuntimeError):
    def __init__(self, code: int, what: str):
        self.code = code
        msg = what
        try:
            msg = f"{what}: {load().sccsum_strerror(code).decode()} ({code})"
        except Exception:  # noqa: BLE001 - best effort message
            msg = f"{what}: error {code}"
        super().__init__(msg)


_LIB = None

_u64 = ctypes.c_uint64
_u32 = ctypes.c_uint32
_vp = ctypes.c_void_p

_PROTOS = {
    "sccsum_abi_version": (ctypes.c_int, []),
    "sccsum_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "sccsum_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "sccsum_device_numa_node": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "sccsum_init": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_pseudo_seed": (_u32, [_u32, _u32, ctypes.c_uint8, ctypes.c_uint16]),
    "sccsum_spans": (ctypes.c_int, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp]),
    "sccsum_ipv4_frames": (ctypes.c_int, [_vp, _u64, _vp, _vp, _vp, _vp, _u64, _u32, _vp]),
    "sccsum_spans_multi": (ctypes.c_int, [_vp, _u32, _u32, _vp]),
    "sccsum_ipv4_frames_multi": (ctypes.c_int, [_vp, _u32, _u32, _vp]),
    "sccsum_sync": (ctypes.c_int, [_vp]),
    "sccsum_fragments": (ctypes.c_int, [_vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp]),
    "sccsum_fragments_workspace": (_u64, [_u64]),
    "sccsum_ipv4_fill": (ctypes.c_int, [_vp, _u64, _vp, _vp, _vp, _vp, _u64, _u32, _u32, _vp]),
    "sccsum_ipv4_rss": (ctypes.c_int, [_vp, _u64, _vp, _vp, _vp, _u32, ctypes.c_int, _vp, _vp, _u64, _vp]),
    "sccsum_ipv4_frames_rss": (ctypes.c_int, [_vp, _u64, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _u32, ctypes.c_int,
                                               _vp, _vp]),
    "sccsum_set_kernel_variant": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_blocks_per_cu": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_group_units": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_tile_packets": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_dynamic_tiles": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_tile_bytes": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_tail_split": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "sccsum_set_out_policy": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_engine_write_through": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_short_chunks": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_run_align": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_read_probe": (ctypes.c_int, [_vp, _u64, _vp, _vp]),
    "sccsum_read_probe_blocks": (ctypes.c_int, []),
    "sccsum_pipeline_create": (ctypes.c_int, [ctypes.c_int, _u64, _u32, ctypes.c_int, ctypes.POINTER(_vp)]),
    "sccsum_pipeline_run": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, _u64, _vp, _vp, _vp, _u64, _u32,
                                           _vp, _vp]),
    "sccsum_pipeline_destroy": (ctypes.c_int, [_vp]),
    "sccsum_burst_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _u64, _u32, _u64, ctypes.c_int, _vp, _vp,
                                           ctypes.POINTER(_vp)]),
    "sccsum_burst_submit": (ctypes.c_int, [_vp, _vp, _u32, _u32, ctypes.POINTER(_u64)]),
    "sccsum_burst_submit_mapped": (ctypes.c_int, [_vp, _vp, _u32, _u32, ctypes.POINTER(_u64)]),
    "sccsum_gather": (ctypes.c_int, [_vp, _u64, _vp, _vp]),
    "sccsum_spans_desc": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp]),
    "sccsum_ipv4_frames_desc": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp]),
    "sccsum_ipv4_fill_desc": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _u32, _vp]),
    "sccsum_burst_set_fill": (ctypes.c_int, [_vp, _u32]),
    "sccsum_set_burst_fused": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_burst_poll": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    "sccsum_burst_drain": (ctypes.c_int, [_vp]),
    "sccsum_burst_destroy": (ctypes.c_int, [_vp]),
    "sccsum_host_alloc": (ctypes.c_int, [ctypes.POINTER(_vp), _u64]),
    "sccsum_host_free": (ctypes.c_int, [_vp]),
    "sccsum_engine_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _u32, _u32, ctypes.POINTER(_vp)]),
    "sccsum_engine_create_opts": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "sccsum_engine_start": (ctypes.c_int, [_vp, _vp]),
    "sccsum_engine_submit": (ctypes.c_int, [_vp, _vp, _u32, _u32, _u64, ctypes.POINTER(_u64)]),
    "sccsum_engine_submit_fill": (ctypes.c_int, [_vp, _vp, _u32, _u32, _u32, _u64, ctypes.POINTER(_u64)]),
    "sccsum_set_engine_idle_ms": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_engine_sync_every": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_set_fill_single_max": (ctypes.c_int, [ctypes.c_int]),
    "sccsum_engine_wait": (ctypes.c_int, [_vp, _u64, _u64]),
    "sccsum_engine_stop": (ctypes.c_int, [_vp]),
    "sccsum_engine_destroy": (ctypes.c_int, [_vp]),
    "sccsum_steer_create": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "sccsum_steer_destroy": (ctypes.c_int, [_vp]),
    "sccsum_steer_workspace": (_u64, [_vp, _u64]),
    "sccsum_steer_run": (ctypes.c_int, [_vp, ctypes.c_int, _u32, _vp, _vp, _u32, _u32, _u64, _vp, _vp, _vp, _vp,
                                        _vp]),
    "sccsum_steer_dest": (_u32, [_vp, ctypes.c_int, _u32, _u32]),
    "sccsum_steer_build_reta": (ctypes.c_int, [_vp, _vp, _u32, _vp]),
    "sccsum_steer_tile_packets": (ctypes.c_int, []),
    "sccsum_ipv4_send_plan": (ctypes.c_int, [_vp, _u32, ctypes.c_uint8, ctypes.POINTER(_u32), ctypes.POINTER(_u64)]),
    "sccsum_ipv4_send_workspace": (_u64, [_u64]),
    "sccsum_ipv4_send": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sccsum_send_tile_datagrams": (ctypes.c_int, []),
    "sccsum_send_emit_tile_frames": (ctypes.c_int, []),
    "sccsum_ipv4_frag_records": (ctypes.c_int, [_vp, _u64, _vp, _vp, _vp, _u32, _u32, _u64, _u32, _u32, _vp, _vp, _vp,
                                                _vp]),
    "sccsum_ipv4_reasm_workspace": (_u64, [_u64]),
    "sccsum_ipv4_reasm": (ctypes.c_int, [_vp, _u64, _u64, _vp, _u32, _vp, _vp, _vp]),
    "sccsum_reasm_key_mix": (_u32, [_u32, _u32, ctypes.c_uint16, ctypes.c_uint8]),
    "sccsum_reasm_sort_tile_records": (ctypes.c_int, []),
    "sccsum_reasm_scan_tile_records": (ctypes.c_int, []),
    "sccsum_arp_table_create": (ctypes.c_int, [ctypes.c_int, _vp, _u32, ctypes.POINTER(_vp)]),
    "sccsum_arp_table_create_host": (ctypes.c_int, [_vp, _u32, ctypes.POINTER(_vp)]),
    "sccsum_arp_table_destroy": (ctypes.c_int, [_vp]),
    "sccsum_arp_table_lookup": (ctypes.c_int, [_vp, _u32, ctypes.POINTER(_u64)]),
    "sccsum_arp_table_slot": (_u32, [_u32, _u32]),
    "sccsum_arp_table_bits": (_u32, [_vp]),
    "sccsum_eth_tile_packets": (ctypes.c_int, []),
    "sccsum_eth_rx_workspace": (_u64, [_u64]),
    "sccsum_eth_rx": (ctypes.c_int, [_vp, _u64, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sccsum_arp_learn_workspace": (_u64, [_u64]),
    "sccsum_arp_learn_records": (ctypes.c_int, [_vp, _u64, _vp, _vp, _vp, _u32, _u32, _vp, _u64, _u32, _u32, _vp, _vp,
                                                _vp, _vp, _vp]),
    "sccsum_eth_send_workspace": (_u64, [_u64]),
    "sccsum_eth_send": (ctypes.c_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sccsum_udp_ports_create": (ctypes.c_int, [ctypes.c_int, _vp, _u32, ctypes.POINTER(_vp)]),
    "sccsum_udp_ports_create_host": (ctypes.c_int, [_vp, _u32, ctypes.POINTER(_vp)]),
    "sccsum_udp_ports_destroy": (ctypes.c_int, [_vp]),
    "sccsum_udp_ports_lookup": (ctypes.c_int, [_vp, ctypes.c_uint16]),
    "sccsum_udp_ports_channels": (_u32, [_vp]),
    "sccsum_udp_rx_workspace": (_u64, [_u64]),
    "sccsum_udp_rx": (ctypes.c_int, [_vp, _u64, _vp, _vp, _u64, _vp, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp]),
    "sccsum_udp_rx_reasm_workspace": (_u64, [_u64]),
    "sccsum_udp_rx_reasm": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _u32, _vp, _vp,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sccsum_udp_send": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp]),
    "sccsum_tcp_conns_create": (ctypes.c_int, [ctypes.c_int, _vp, _u32, _vp, _u32, ctypes.POINTER(_vp)]),
    "sccsum_tcp_conns_create_host": (ctypes.c_int, [_vp, _u32, _vp, _u32, ctypes.POINTER(_vp)]),
    "sccsum_tcp_conns_destroy": (ctypes.c_int, [_vp]),
    "sccsum_tcp_conns_lookup": (ctypes.c_int64, [_vp, _u32, _u32, ctypes.c_uint16, ctypes.c_uint16]),
    "sccsum_tcp_conns_listening": (ctypes.c_int, [_vp, ctypes.c_uint16]),
    "sccsum_tcp_conns_slot": (_u32, [_u32, _u32, ctypes.c_uint16, ctypes.c_uint16, _u32]),
    "sccsum_tcp_conns_bits": (_u32, [_vp]),
    "sccsum_tcp_conns_count": (_u32, [_vp]),
    "sccsum_tcp_rx_workspace": (_u64, [_u64, _u32]),
    "sccsum_tcp_rx": (ctypes.c_int, [_vp, _u64, _vp, _vp, _u64, _vp, _u32, _u32, _u32, _vp, _vp, _u64, _u32, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sccsum_tcp_send": (ctypes.c_int, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp]),
    "sccsum_tcp_rx_data_workspace": (_u64, [_u64, _u32]),
    "sccsum_tcp_rx_data": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _u32, _u64, _vp, _vp, _vp, _vp,
                                          _vp]),
    "sccsum_tcp_tx_data_workspace": (_u64, [_u32, _u64]),
    "sccsum_tcp_tx_data_seg_tile": (ctypes.c_int, []),
    "sccsum_tcp_tx_data_max_blocks": (ctypes.c_int, []),
    "sccsum_tcp_tx_data": (ctypes.c_int, [_vp, _vp, _u32, _vp, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp, _vp]),
    "sccsum_tcp_rx_acks_workspace": (_u64, [_u64, _u32, _u64]),
    "sccsum_tcp_rx_acks": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _u64,
                                          ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "sccsum_tcp_listen_workspace": (_u64, [_u64]),
    # the first argument, sccsum_tcp_listen_opts by value, is put in front where TcpListenOpts is defined
    "sccsum_tcp_listen": (ctypes.c_int, [_vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _vp, _vp, _vp]),
}
PIPE_SPANS = 0
PIPE_IPV4 = 1
ENGINE_FILL = 0x100
GATHER_NONE = 0
GATHER_HOST = 1
GATHER_STRIDED = 2
GATHER_ZERO_COPY = 3
RSS_DISPATCH = 0
RSS_REASSEMBLED = 1


class Batch(ctypes.Structure):
    """sccsum_batch: one batch of a multi-batch launch."""
    _fields_ = [("d_bytes", ctypes.c_void_p), ("bytes_len", ctypes.c_uint64), ("d_off", ctypes.c_void_p),
                ("d_len", ctypes.c_void_p), ("d_seed", ctypes.c_void_p), ("d_out", ctypes.c_void_p),
                ("d_status", ctypes.c_void_p), ("n", ctypes.c_uint64)]


MAX_BATCHES = 16
FILL_SINGLE_MAX = 524288  # in-place fills of at most this many frames run in one pass (sccsum_diag.h)
ENGINE_MAX_BATCHES = 4


class EngineOpts(ctypes.Structure):
    """sccsum_engine_opts: a resident engine's limits (0 = the default)."""
    _fields_ = [("ring_slots", ctypes.c_uint32), ("max_in_flight", ctypes.c_uint32), ("idle_ms", ctypes.c_uint32),
                ("dep_ms", ctypes.c_uint32), ("producer_in_flight", ctypes.c_uint32)]


STEER_DISPATCH = 0
STEER_HASH2CPU = 1
STEER_DROPPED = 0xFF  # d_cpu of a dropped packet
RETA_SIZE = 128


class SteerMap(ctypes.Structure):
    """sccsum_steer_map: the tables rx steering sends a hash through (host memory)."""
    _fields_ = [("ncpu", ctypes.c_uint32), ("hw_queues", ctypes.c_uint32), ("table_bits", ctypes.c_uint32),
                ("redir_size", ctypes.c_uint32), ("redir", ctypes.c_void_p), ("sw_reta", ctypes.c_void_p),
                ("sw_reta_set", ctypes.c_void_p)]


SEND_TSO = 0x01
SEND_UFO = 0x02
SEND_NO_IP_CSUM = 0x04
SEND_L4 = 0x08
SEND_L4_MAX = 65515  # the longest L4 datagram ipv4::send takes (ip_packet_len_max - 20)


class SendOpts(ctypes.Structure):
    """sccsum_send_opts: what ipv4::send takes from its interface (source address, MTU, offload flags)."""
    _fields_ = [("src_host", ctypes.c_uint32), ("mtu", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


REASM_COMPLETE = 1
REASM_PENDING = 2
REASM_HOST = 3
REASM_MAX_RECORDS = 0x7FFFFFFF


class FragRec(ctypes.Structure):
    """sccsum_frag_rec: one IPv4 fragment as rx reassembly takes it (32 bytes)."""
    _fields_ = [("frame", ctypes.c_void_p), ("src", ctypes.c_uint32), ("dst", ctypes.c_uint32),
                ("id", ctypes.c_uint16), ("proto", ctypes.c_uint8), ("mf", ctypes.c_uint8),
                ("offset", ctypes.c_uint16), ("hdr_len", ctypes.c_uint16), ("len", ctypes.c_uint16),
                ("reserved", ctypes.c_uint16), ("tag", ctypes.c_uint32)]


class ReasmOut(ctypes.Structure):
    """sccsum_reasm_out: the device arrays sccsum_ipv4_reasm writes."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("d_desc", "d_dgram_first", "d_dgram_off", "d_dgram_len", "d_dgram_seed", "d_dgram_head",
                 "d_dgram_last", "d_dgram_hash", "d_pending", "d_host", "d_rec_state", "d_total")]


ST_NOARP = 0x20       # eth_send: the next hop has no ARP entry
ETH_UNKNOWN = 0xFF    # eth_rx classes of dropped frames
ETH_SHORT = 0xFE
ETH_RANGE = 0xFD
ETH_MAX_PROTOS = 8
ETH_HDR = 14          # sizeof(eth_hdr)
ARP_MAX_ENTRIES = 1 << 20
MAC_MAX = (1 << 48) - 1


class ArpEntry(ctypes.Structure):
    """sccsum_arp_entry: one (ip, mac) pair of an ARP table (16 bytes)."""
    _fields_ = [("ip", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("mac", ctypes.c_uint64)]


class EthOpts(ctypes.Structure):
    """sccsum_eth_opts: what eth_send takes from the interface and its ipv4 (addresses in host order)."""
    _fields_ = [("hw_address", ctypes.c_uint64), ("host", ctypes.c_uint32), ("netmask", ctypes.c_uint32),
                ("gw", ctypes.c_uint32), ("eth_proto", ctypes.c_uint16)]


UDP_NOPORT = 0xFF     # udp_rx classes of dropped frames / datagrams
UDP_SHORT = 0xFE
UDP_SKIP = 0xFD
UDP_MAX_CHANNELS = 252
UDP_HDR = 8           # sizeof(udp_hdr)
UDP_CSUM_OFFLOAD = 0x01
UDP_UFO = 0x02
UDP_PAYLOAD_MAX = SEND_L4_MAX - UDP_HDR  # 65507
UDP_QUEUE_SIZE = 1024  # ipv4_udp::default_queue_size


class UdpOpts(ctypes.Structure):
    """sccsum_udp_opts: what ipv4_udp::send takes from its ipv4 (source address, MTU, offload flags)."""
    _fields_ = [("src_host", ctypes.c_uint32), ("mtu", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


TCP_CONN = 0          # tcp_rx classes: a known connection, a listening port, answered with a RST
TCP_LISTEN = 1
TCP_RESET = 2
TCP_NOCONN = 3        # ... and of dropped frames: a RST nobody owns, a bad header, not the TCP layer's
TCP_SHORT = 0xFE
TCP_SKIP = 0xFD
TCP_MAX_CONNS = 1 << 20
TCP_HDR = 20          # tcp_hdr::len
TCP_CSUM_OFFLOAD = 0x01
TCP_TSO = 0x02
TCP_NO_CONN = 0xFFFFFFFF  # sccsum_tcp_seg.conn outside bucket 0
TCP_RCV_ELIGIBLE = 0x01     # sccsum_tcp_rcv.flags: the tcb may take the straight path
TCP_RCV_NR_FULL = 0x02      # ... and sccsum_tcp_rcv_run.flags: _nr_full_seg_received
TCP_RCV_ACK_ARMED = 0x04    # _delayed_ack.armed()
TCP_RCV_ACK_REARMED = 0x08  # run records only: arm(200 ms) was called during the stretch
TCP_RCV_ACK_NOW = 0x10      # run records only: output() was called at least once
TCP_STOP_END = 0            # sccsum_tcp_rcv_run.stop: why segment `taken` was not taken
TCP_STOP_INELIGIBLE = 1
TCP_STOP_WINDOW = 2
TCP_STOP_SEQ = 3
TCP_STOP_FLAGS = 4
TCP_STOP_ACK = 5
TCP_STOP_EMPTY = 6
TCP_STOP_CAPACITY = 7


class TcpConn(ctypes.Structure):
    """sccsum_tcp_conn: one connid of the connection table (12 bytes, host order)."""
    _fields_ = [("local_ip", ctypes.c_uint32), ("foreign_ip", ctypes.c_uint32), ("local_port", ctypes.c_uint16),
                ("foreign_port", ctypes.c_uint16)]


class TcpSeg(ctypes.Structure):
    """sccsum_tcp_seg: one parsed segment of tcp_rx's grouped order (32 bytes)."""
    _fields_ = [("pay_off", ctypes.c_uint64), ("pay_len", ctypes.c_uint32), ("seq", ctypes.c_uint32),
                ("ack", ctypes.c_uint32), ("conn", ctypes.c_uint32), ("window", ctypes.c_uint16),
                ("sport", ctypes.c_uint16), ("dport", ctypes.c_uint16), ("flags", ctypes.c_uint8),
                ("hdr_len", ctypes.c_uint8)]


class TcpOut(ctypes.Structure):
    """sccsum_tcp_out: what output_one puts into one segment's header (24 bytes)."""
    _fields_ = [("dst", ctypes.c_uint32), ("seq", ctypes.c_uint32), ("ack", ctypes.c_uint32),
                ("sport", ctypes.c_uint16), ("dport", ctypes.c_uint16), ("window", ctypes.c_uint16),
                ("flags", ctypes.c_uint8), ("hdr_len", ctypes.c_uint8), ("mss", ctypes.c_uint32)]


class TcpOpts(ctypes.Structure):
    """sccsum_tcp_opts: what output_one takes from its ipv4 (source address, MTU, offload flags)."""
    _fields_ = [("src_host", ctypes.c_uint32), ("mtu", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


TCP_SND_ELIGIBLE = 0x01     # sccsum_tcp_snd.flags: the tcb's transmit chain is the closed form
TCP_SND_RTX_ARMED = 0x02    # _retransmit.armed()
TCP_SND_RTX_ARM = 0x04      # sccsum_tcp_snd_run.flags: arm the retransmit timer now
TCP_STOP_QUEUE = 8          # sccsum_tcp_snd_run.stop: a queue of more than 2^32 - 1 bytes
TCP_TX_MAX_BUFS = 1 << 31
TCP_TX_MAX_SEGS = 0x7FFFFFFF


class TcpTxOpts(ctypes.Structure):
    """sccsum_tcp_tx_opts: what get_transmit_packet takes from hw_features(), and the layout's headroom."""
    _fields_ = [("src_host", ctypes.c_uint32), ("mtu", ctypes.c_uint32), ("max_packet_len", ctypes.c_uint32),
                ("headroom", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


TCP_ACK_ELIGIBLE = 0x01     # sccsum_tcp_ack.flags: the tcb may take the advancing-ACK path
TCP_ACK_CLOSE_WAIT = 0x02   # the state is CLOSE_WAIT: no closing output()
TCP_ACK_FIRST_SAMPLE = 0x04  # ... and sccsum_tcp_ack_run.flags: _snd.first_rto_sample
TCP_ACK_ALL_ACKED = 0x08    # run records only: the queue is empty, stop the timer, signal_all_data_acked
TCP_ACK_RTX_REARM = 0x10    # run records only: rearm the retransmit timer at now + rto
TCP_ACK_POLL = 0x20         # run records only: clear_delayed_ack(); output()
TCP_STOP_DATA = 9           # sccsum_tcp_ack_run.stop: the segment carries text
TCP_STOP_WL = 10            # ... or fails the SND.WL1 / WL2 test at the run's head
TCP_ACK_MAX_ENTRIES = 1 << 31


class TcpAck(ctypes.Structure):
    """sccsum_tcp_ack: the send-side state of one tcb as tcp_rx_acks takes it (64 bytes)."""
    _fields_ = [("una", ctypes.c_uint32), ("next", ctypes.c_uint32), ("window", ctypes.c_uint32),
                ("wl1", ctypes.c_uint32), ("wl2", ctypes.c_uint32), ("cwnd", ctypes.c_uint32),
                ("ssthresh", ctypes.c_uint32), ("unsent_len", ctypes.c_uint32), ("rcv_next", ctypes.c_uint32),
                ("rto", ctypes.c_uint32), ("srtt", ctypes.c_int64), ("rttvar", ctypes.c_int64),
                ("mss", ctypes.c_uint16), ("window_scale", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("reserved", ctypes.c_uint32)]


class TcpAckRun(ctypes.Structure):
    """sccsum_tcp_ack_run: what one run's taken ACKs did to its tcb (64 bytes)."""
    _fields_ = [("taken", ctypes.c_uint32), ("una", ctypes.c_uint32), ("acked", ctypes.c_uint32),
                ("popped", ctypes.c_uint32), ("trim", ctypes.c_uint32), ("queue_freed", ctypes.c_uint32),
                ("window", ctypes.c_uint32), ("cwnd", ctypes.c_uint32), ("srtt", ctypes.c_int64),
                ("rttvar", ctypes.c_int64), ("rto", ctypes.c_uint32), ("flags", ctypes.c_uint8),
                ("stop", ctypes.c_uint8), ("pad", ctypes.c_uint16), ("reserved", ctypes.c_uint32 * 2)]


TCP_LISTEN_NEW = 0          # tcp_listen classes: a created connection (a record and a SYN-ACK)
TCP_LISTEN_RESET = 1        # answered with a RST: the port is full, or an ACK in LISTEN
TCP_LISTEN_DROP = 2         # discarded: a RST, or no RST / ACK / SYN
TCP_LISTEN_LATER = 3        # at or behind `taken`: the host walks it with its real _tcbs
TCP_LISTEN_MAX = 1 << 30
TCP_NEW_MSS = 0x01          # sccsum_tcp_new.flags: _mss_received
TCP_NEW_WSCALE = 0x02       # _win_scale_received
TCP_NEW_SACK = 0x04         # _sack_received
TCP_NEW_WSCALE_BIG = 0x08   # snd_wscale > 14: snd_window and ssthresh are unshifted
TCP_RCV_WINDOW = 29200      # get_default_receive_window_size before the shift


class TcpNew(ctypes.Structure):
    """sccsum_tcp_new: one connection tcp_listen created (64 bytes)."""
    _fields_ = [("local_ip", ctypes.c_uint32), ("foreign_ip", ctypes.c_uint32), ("local_port", ctypes.c_uint16),
                ("foreign_port", ctypes.c_uint16), ("pos", ctypes.c_uint32), ("irs", ctypes.c_uint32),
                ("iss", ctypes.c_uint32), ("snd_window", ctypes.c_uint32), ("cwnd", ctypes.c_uint32),
                ("ssthresh", ctypes.c_uint32), ("rcv_window", ctypes.c_uint32), ("wl1", ctypes.c_uint32),
                ("wl2", ctypes.c_uint32), ("snd_mss", ctypes.c_uint16), ("local_mss", ctypes.c_uint16),
                ("snd_wscale", ctypes.c_uint8), ("rcv_wscale", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("pad", ctypes.c_uint8), ("reserved", ctypes.c_uint32 * 2)]


class TcpListenOpts(ctypes.Structure):
    """sccsum_tcp_listen_opts: the ISN secret and clock, the MTU, the flags; passed by value (76 bytes)."""
    _fields_ = [("isn_key", ctypes.c_uint32 * 16), ("isn_m", ctypes.c_uint32), ("mtu", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


_PROTOS["sccsum_tcp_listen"] = (ctypes.c_int, [TcpListenOpts] + _PROTOS["sccsum_tcp_listen"][1])


class Fragment(ctypes.Structure):
    """sccsum_fragment: the layout of seastar::net::fragment (packet.hh:43-46)."""
    _fields_ = [("base", ctypes.c_void_p), ("size", ctypes.c_size_t)]


def header_symbols() -> list[str]:
    """Every function declared in include/sccsum.h and include/sccsum_diag.h."""
    text = open(HEADER_PATH).read() + open(DIAG_HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sccsum_[a-z0-9_]+)\s*\(", text)))


def load():
    """Open libsccsum.so (raises if it is missing: there is no CPU fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    import torch  # noqa: F401  -- share torch's HIP runtime (see module doc)

    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    # SCCSUM_LIB: diagnostic override (A/B builds of the same ABI); still a native library, never a fallback
    lib = ctypes.CDLL(os.environ.get("SCCSUM_LIB", LIB_PATH), mode=ctypes.RTLD_GLOBAL)
    # SCCSUM_ABI_ANY=1: diagnostic A/B against an older build (another ABI version; entry points it
    # lacks stay unbound); only ever set together with SCCSUM_LIB by tools/gpu_session.sh's lib: step
    any_abi = bool(os.environ.get("SCCSUM_ABI_ANY")) and "SCCSUM_LIB" in os.environ
    for name, (res, args) in _PROTOS.items():
        if any_abi and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.sccsum_abi_version() != ABI_VERSION and not any_abi:
        raise RuntimeError(f"libsccsum ABI version {lib.sccsum_abi_version()} != {ABI_VERSION}: rebuild it")
    _LIB = lib
    return lib


def check(code: int, what: str) -> None:
    if code != SCCSUM_OK:
        raise SccsumError(code, what)
