"""sccsum_tcp_listen on the GPU against the per-segment model
(tests/tcp_listen_model.py): every output array, exactly, for the buckets
written out by hand (every row of the table, the duplicate connids, every
option layout), seeded buckets around the tile, 300 listening ports, connids
that collide and wrap in the de-duplication table; the recipe from wire frames
to the SYN-ACKs on the wire; determinism, graph replay and the C++ class.
Every raw call writes into outputs with guard words on both sides."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import stack_model as sm
import tcp_listen_model as lm
import tcp_listen_traffic as tr
import tcp_model as tm
import tcp_traffic
from seastar_amd import batch, native
from test_gpu_eth import Out, _dev

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = tr.TILE
NAMES = ("cls", "new", "synack", "sa_off", "sa_len", "sa_out", "rst", "rst_dst", "total")
POISON = 0x5B


def _inputs(dev, a: dict, space) -> list:
    """The device arrays of tcp_listen_traffic.arrays' dict, in the call's order."""
    buf = np.zeros((a["buf"].size + 15) // 16 * 16 + 16, dtype=np.uint8)
    buf[:a["buf"].size] = a["buf"]
    sp = tr.space_array(space) if isinstance(space, dict) else space
    return [_dev(dev, buf), _dev(dev, a["off"].view(np.int64)), _dev(dev, a["first"].view(np.int32)),
            _dev(dev, a["order"].view(np.int32)), _dev(dev, a["seg"].view(np.int64)), _dev(dev, a["src"].view(np.int32)),
            _dev(dev, sp.view(np.int32))]


def _opts(flags: int = 0, key: bytes = tr.KEY, isn_m: int = tr.ISN_M, mtu: int = tr.MTU):
    return native.TcpListenOpts((ctypes.c_uint32 * 16)(*np.frombuffer(key, dtype="<u4").tolist()), isn_m, mtu, flags)


def _call(lib, a: dict, ins: list, m_max: int, flags: int, p: dict) -> int:
    return lib.sccsum_tcp_listen(_opts(flags), ins[0].data_ptr(), int(a["buf"].size), ins[1].data_ptr(), a["nbatch"],
                                 ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(), ins[5].data_ptr(), m_max,
                                 ins[6].data_ptr(), p["cls"], p["rec"], p["synack"], p["sa_off"], p["sa_len"], p["sa_out"],
                                 p["rst"], p["rst_dst"], p["total"], p["ws"], torch.cuda.current_stream().cuda_stream)


def run_listen(dev, a: dict, space, m_max: int | None = None, flags: int = 0, shift: int = 0) -> dict:
    """sccsum_tcp_listen on arrays as tcp_rx leaves them into guarded outputs; returns their host copies."""
    lib = native.load()
    m = a["m"]
    m_max = m if m_max is None else m_max
    ins = _inputs(dev, a, space)
    o = dict(cls=Out(dev, m_max, torch.uint8, POISON, shift), rec=Out(dev, 8 * m_max, torch.int64, -7, shift),
             synack=Out(dev, 8 * m_max, torch.int32, -7, shift), sa_off=Out(dev, m_max, torch.int64, -7, shift),
             sa_len=Out(dev, m_max, torch.int32, -7, shift), sa_out=Out(dev, 6 * m_max, torch.int32, -7, shift),
             rst=Out(dev, 5 * m_max, torch.int32, -7, shift), rst_dst=Out(dev, m_max, torch.int32, -7, shift),
             total=Out(dev, 4, torch.int64, -7, shift),
             ws=Out(dev, int(lib.sccsum_tcp_listen_workspace(m_max)) // 16, torch.complex128, 3.0, shift))
    assert o["ws"].ptr % 16 == 0 and o["rec"].ptr % 16 == 0
    rc = _call(lib, a, ins, m_max, flags, {k: v.ptr for k, v in o.items()})
    assert rc == 0, rc
    torch.cuda.synchronize()
    o["ws"].host()
    t = o["total"].host().view(np.uint64)
    k, r = int(t[1]), int(t[2])
    assert int(t[0]) <= min(m, m_max) and k + r <= int(t[0])
    slots = o["synack"].host(8 * k).reshape(k, 8)
    assert np.all(slots[:, :5] == -7)                        # the twenty bytes in front are tcp_send's
    staged = np.ascontiguousarray(slots[:, 5:]).view(np.uint8).reshape(k, 12)
    return dict(cls=o["cls"].host(min(m, m_max)), new=o["rec"].host(8 * k).view(lm.NEW_DTYPE), synack=staged,
                sa_off=o["sa_off"].host(k).view(np.uint64), sa_len=o["sa_len"].host(k).view(np.uint32),
                sa_out=o["sa_out"].host(6 * k).view(lm.OUT_DTYPE), rst=o["rst"].host(5 * r).view(np.uint8),
                rst_dst=o["rst_dst"].host(r).view(np.uint32), total=t)


def check(got: dict, want: dict, what="") -> None:
    assert got["total"].tolist() == want["total"].tolist(), what
    assert got["cls"].tolist() == want["cls"].tolist(), what
    for name in lm.NEW_DTYPE.names:
        ne = got["new"][name] != want["new"][name]
        bad = np.flatnonzero(ne if ne.ndim == 1 else ne.any(axis=1))
        assert bad.size == 0, (what, name, bad[:5], got["new"][bad[:5]], want["new"][bad[:5]])
    for name in NAMES:
        assert got[name].tobytes() == want[name].tobytes(), (what, name)


def _expect(segs, space, offload=False) -> dict:
    return lm.expect(segs, space, tr.KEY, tr.ISN_M, tr.MTU, offload)


# ---------------------------------------------------------------- written out by hand

@pytest.mark.parametrize("flags", [0, native.TCP_CSUM_OFFLOAD])
def test_every_row_of_the_table(dev, flags):
    segs, space, classes = tr.table_case()
    got = run_listen(dev, tr.arrays(segs), space, flags=flags)
    assert got["cls"].tolist() == classes
    check(got, _expect(segs, space, bool(flags)))


@pytest.mark.parametrize("name", sorted(tr.duplicate_cases()))
def test_duplicate_connids(dev, name):
    segs, space, taken, classes = tr.duplicate_cases()[name]
    got = run_listen(dev, tr.arrays(segs, lead=0, trail=0), space)
    assert int(got["total"][0]) == taken and got["cls"].tolist() == classes + [lm.LATER] * (len(segs) - taken)
    check(got, _expect(segs, space), name)


def test_option_layouts_mss_bands_and_shifts(dev):
    segs, space, names = tr.option_case()
    tr.check_strict(segs, names)
    want = _expect(segs, space)
    got = run_listen(dev, tr.arrays(segs), space)
    for k, name in enumerate(names):
        assert got["new"][k].tobytes() == want["new"][k].tobytes(), (name, got["new"][k], want["new"][k])
        assert got["synack"][k].tobytes() == want["synack"][k].tobytes(), name
    check(got, want)
    rec = dict(zip(names, got["new"]))
    assert [int(rec[f"mss_{v}"]["cwnd"]) for v in tr.MSS_VALUES] == [2144, 4380, 3288, 6570, 4382]
    assert int(rec["shift_14"]["flags"]) == lm.F_WSCALE and int(rec["shift_15"]["flags"]) == lm.F_WSCALE | lm.F_BIG


def test_options_at_the_buffers_edges_are_not_read_past(dev):
    """The last frame's options end at the buffer's last byte, and a record
    whose options would start before the buffer is read as having none."""
    segs = [tr.syn(1, options=tr.OPTION_LAYOUTS["forty"]), tr.syn(2, options=tr.OPTION_LAYOUTS["kind_last"])]
    a = tr.arrays(segs, lead=0, trail=0)
    last = int(np.argmax(a["off"]))                           # the frame that ends the buffer
    p = int(np.flatnonzero(a["order"] == last)[0])
    assert int(a["seg"]["pay_off"][p]) == a["buf"].size       # no payload: the options are the last bytes
    want = _expect(segs, {80: 9})
    check(run_listen(dev, a, {80: 9}), want)
    a["seg"]["pay_off"][0] = 30                               # 40 option bytes cannot lie in front of offset 30
    a["seg"]["hdr_len"][0] = 60
    got = run_listen(dev, a, {80: 9})
    assert (int(got["new"][0]["snd_mss"]), int(got["new"][0]["flags"]), int(got["sa_out"][0]["hdr_len"])) == (536, 0, 20)
    a["seg"]["pay_off"][0] = a["buf"].size + 1                # ... nor behind the buffer
    got = run_listen(dev, a, {80: 9})
    assert (int(got["new"][0]["snd_mss"]), int(got["new"][0]["flags"])) == (536, 0)


# ---------------------------------------------------------------- seeded buckets

@functools.lru_cache(maxsize=None)
def _mixed(m: int, stop_at=None):
    segs, space = tr.mixed(m % 5, m, stop_at=stop_at)
    return segs, space, tr.arrays(segs, seed=m), _expect(segs, space, bool(m % 2))


@pytest.mark.parametrize("m", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 7])
def test_seeded_buckets_against_the_model(dev, m):
    segs, space, a, want = _mixed(m)
    assert int(want["total"][0]) == m
    check(run_listen(dev, a, space, flags=m % 2), want)


def test_a_stop_behind_the_first_tile_and_a_bound_above_the_size(dev):
    segs, space, a, want = _mixed(2 * TILE + 7, 1500)
    assert want["total"].tolist()[0] == 1500
    got = run_listen(dev, a, space, flags=1)
    check(got, want)
    assert got["cls"][1500:].tolist() == [lm.LATER] * (len(segs) - 1500)
    # m_max above the size: sizes the table and the grids, changes nothing
    got = run_listen(dev, a, space, m_max=3 * TILE + 1, flags=1)
    check(got, want)
    # m_max below it: the bucket read as cut there
    segs, space, a, _ = _mixed(2 * TILE + 7)
    cut = 2 * TILE - 3
    check(run_listen(dev, a, space, m_max=cut, flags=1), _expect(segs[:cut], space, True))


def test_empty_bucket_and_no_segments(dev):
    a = tr.arrays([], lead=4, trail=3)
    got = run_listen(dev, a, {80: 5}, m_max=7)
    assert got["total"].tolist() == [0, 0, 0, 0] and got["cls"].size == 0
    lib = native.load()
    total = Out(dev, 4, torch.int64, -7)
    ws = Out(dev, max(int(lib.sccsum_tcp_listen_workspace(0)) // 16, 1), torch.complex128, 3.0)
    rc = lib.sccsum_tcp_listen(_opts(), None, 0, None, 0, None, None, None, None, 0, None, None, None, None, None, None,
                               None, None, None, total.ptr, ws.ptr, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert total.host().tolist() == [0, 0, 0, 0]


def test_three_hundred_listening_ports(dev):
    """Both digits of the port take part in the rank: 300 ports, each with room for all but its last SYN."""
    segs, space = tr.many_ports(0)
    want = _expect(segs, space)
    assert want["total"].tolist() == [1200, 900, 300, 0]
    check(run_listen(dev, tr.arrays(segs), space), want)


def test_colliding_and_wrapping_connids(dev):
    segs, space = tr.colliding(64)
    want = _expect(segs, space)
    assert int(want["total"][0]) == len(segs) - 1
    check(run_listen(dev, tr.arrays(segs, lead=0, trail=0), space, m_max=64), want)


def test_deterministic(dev):
    """Two runs into outputs at other addresses give identical bytes."""
    segs, space, a, _ = _mixed(2 * TILE + 7, 1500)
    x, y = run_listen(dev, a, space), run_listen(dev, a, space, shift=3)
    for name in x:
        assert x[name].tobytes() == y[name].tobytes(), name


def test_capturable(dev):
    """The launches replay from a graph: no allocation, no synchronisation inside the call."""
    segs, space, a, want = _mixed(2 * TILE + 7)
    lib = native.load()
    m = a["m"]
    ins = _inputs(dev, a, space)
    outs = dict(cls=torch.empty(m, dtype=torch.uint8, device=dev), rec=torch.empty(8 * m, dtype=torch.int64, device=dev),
                synack=torch.empty(8 * m, dtype=torch.int32, device=dev), sa_off=torch.empty(m, dtype=torch.int64, device=dev),
                sa_len=torch.empty(m, dtype=torch.int32, device=dev), sa_out=torch.empty(6 * m, dtype=torch.int32, device=dev),
                rst=torch.empty(5 * m, dtype=torch.int32, device=dev), rst_dst=torch.empty(m, dtype=torch.int32, device=dev),
                total=torch.empty(4, dtype=torch.int64, device=dev))
    ws = torch.empty(int(lib.sccsum_tcp_listen_workspace(m)), dtype=torch.uint8, device=dev)

    def launch():
        rc = _call(lib, a, ins, m, 1, dict({k: v.data_ptr() for k, v in outs.items()}, ws=ws.data_ptr()))
        assert rc == 0, rc

    for v in outs.values():
        v.fill_(0x5A)
    launch()
    torch.cuda.synchronize()
    keep = {k: v.clone() for k, v in outs.items()}
    t = keep["total"].cpu().numpy().view(np.uint64)
    k, r = int(t[1]), int(t[2])
    got = dict(cls=keep["cls"].cpu().numpy(), new=keep["rec"].cpu().numpy()[:8 * k].view(lm.NEW_DTYPE),
               synack=keep["synack"].cpu().numpy()[:8 * k].view(np.uint8).reshape(k, 32)[:, 20:].copy(),
               sa_off=keep["sa_off"].cpu().numpy()[:k].view(np.uint64), sa_len=keep["sa_len"].cpu().numpy()[:k].view(np.uint32),
               sa_out=keep["sa_out"].cpu().numpy()[:6 * k].view(lm.OUT_DTYPE),
               rst=keep["rst"].cpu().numpy()[:5 * r].view(np.uint8), rst_dst=keep["rst_dst"].cpu().numpy()[:r].view(np.uint32),
               total=t)
    check(got, want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for v in outs.values():
        v.fill_(0x5A)
    ws.fill_(0xC3)
    g.replay()
    torch.cuda.synchronize()
    for name, v in outs.items():
        assert torch.equal(v, keep[name]), name


# ---------------------------------------------------------------- from wire frames to the SYN-ACKs on the wire

def test_recipe_from_wire_frames_to_the_syn_acks(dev):
    """frames -> eth_rx -> ipv4_frames -> tcp_rx -> tcp_listen -> tcp_send ->
    spans -> ipv4_send -> eth_send -> pack(), through the wrappers: every
    SYN-ACK on the wire is what stack_model.tx makes of output_one's segment."""
    segs, space = tr.mixed(3, 400, stop_at=350)
    want = _expect(segs, space)
    frames = tr.frames(segs)
    length = np.array([len(f) for f in frames], dtype=np.uint32)
    off = (np.cumsum(length + 3, dtype=np.uint64) - length).astype(np.uint64)
    buf = np.zeros(int(off[-1] + length[-1]), dtype=np.uint8)
    for o, f in zip(off.tolist(), frames):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    wire = batch.PacketBatch.from_host(buf, off, length, device=dev)
    ip = batch.eth_rx(wire, (sm.IPV4, sm.ARP)).bucket(0)
    status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
    batch.ipv4_frames(ip, status=status)
    conns = batch.TcpConns(tcp_traffic.conn_array(0), sorted(space), device=dev.index)
    rx = batch.tcp_rx(ip, status, conns, sm.HOST)
    ls = batch.tcp_listen(rx, ip, space, tr.KEY, tr.ISN_M, tr.MTU)
    torch.cuda.synchronize()
    assert rx.bounds().tolist() == [0, 0, len(segs), len(segs), len(segs)]
    assert ls.totals() == tuple(int(x) for x in want["total"]) and ls.totals()[0] == 350
    assert ls.classes().cpu().numpy().tolist() == want["cls"].tolist()
    assert ls.new().tobytes() == want["new"].tobytes()
    # the room per port as a device tensor instead of a dict: the same bytes
    lt = batch.tcp_listen(rx, ip, _dev(dev, tr.space_array(space).view(np.int32)), tr.KEY, tr.ISN_M, tr.MTU)
    assert lt.totals() == ls.totals() and lt.new().tobytes() == ls.new().tobytes()
    assert torch.equal(lt.classes(), ls.classes()) and torch.equal(lt.synacks[1], ls.synacks[1])
    later = ls.later().cpu().numpy().reshape(-1).view(batch.TCP_SEG_DTYPE)
    assert later["seq"].tolist() == [s.seq for s in segs[350:]]
    l4, rst_dst = ls.resets
    assert l4.data.cpu().numpy()[:want["rst"].size].tobytes() == want["rst"].tobytes()
    assert rst_dst.cpu().numpy().view(np.uint32).tolist() == want["rst_dst"].tolist()
    # the SYN-ACKs
    k = ls.totals()[1]
    pay, out = ls.synacks
    assert out.cpu().numpy().reshape(-1).view(lm.OUT_DTYPE).tobytes() == want["sa_out"].tobytes()
    u = batch.tcp_send(pay, out, sm.HOST, tr.MTU)
    dst = _dev(dev, want["sa_out"]["dst"].view(np.int32))
    ids = [(31 * j + 5) & 0xFFFF for j in range(k)]
    l4sum = batch.spans(u.sum_batch, seeds=u.seeds)
    r = batch.ipv4_send(u.l4, dst, u.proto, tr.MTU, sm.HOST, ids=_dev(dev, np.array(ids, dtype=np.uint16).view(np.int16)),
                        l4sum=l4sum, flags=native.SEND_L4)
    arp = {d: sm.peer_mac(d) for d in sm.ON_LINK}
    arp[sm.GW] = sm.GW_MAC
    table = batch.ArpTable(arp)
    sent = batch.eth_send(r, dst, table, sm.HW, sm.HOST, sm.NETMASK, sm.GW).pack()
    torch.cuda.synchronize()
    assert u.status.cpu().numpy().tolist() == [native.ST_OK] * k
    model = [tm.send(b"", t.synack, sm.HOST, t.synack["options"]) for _, t in want["walk"]["created"]]
    assert {len(m["l4"]) for m in model} == {20, 24, 28}
    cfg = dict(host=sm.HOST, netmask=sm.NETMASK, gw=sm.GW, hw=sm.HW, mtu=tr.MTU, arp=arp)
    t = sm.tx([(m["zero"], sm.TCP, int(d), i) for m, d, i in zip(model, want["sa_out"]["dst"].tolist(), ids)], cfg)
    data, w_off, w_len = sent.data.cpu().numpy(), sent.off.cpu().numpy(), sent.length.cpu().numpy()
    assert sent.n == len(t["frames"]) == k
    for j, f in enumerate(t["frames"]):
        assert data[int(w_off[j]):int(w_off[j]) + int(w_len[j])].tobytes() == f, ("wire frame", j)
    table.close()
    conns.close()


def test_cpp_class_on_gpu(tmp_path):
    """Native host program (tests/cpp/tcp_listen_gpu.cc): tcp_listen against the
    C call it forwards to, on the same inputs into separately poisoned
    outputs; every array byte-equal."""
    exe = str(tmp_path / "tcp_listen_gpu")
    lib_dir = os.path.join(REPO, "seastar_amd", "lib")
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "tcp_listen_gpu.cc"), "-L", lib_dir, "-lsccsum", "-Wl,-rpath," + lib_dir,
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tcp_listen_gpu: OK" in r.stdout
    print(r.stdout)
