"""Device-resident packet batches and the launch wrappers over the C-ABI.

A batch is the layout the kernels consume (DESIGN.md "Data layout in HBM"):
one byte buffer holding every packet back to back (any alignment), padded to
a multiple of 16 bytes, plus an offset (u64) / length (u32) array.  torch
tensors only hold the device memory and give the stream; the arithmetic is in
libsccsum.so.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import native


def _round16(n: int) -> int:
    return (n + 15) & ~15


@dataclass
class PacketBatch:
    data: torch.Tensor  # uint8, len >= round16(bytes_len), device
    off: torch.Tensor  # int64 [n], device
    length: torch.Tensor  # int32 [n], device
    bytes_len: int
    max_len: int

    def __post_init__(self):
        # the kernels trust these: a short buffer or a mistyped array would be
        # read (or, for in-place fill, written) past its end on the device
        d, o, ln = self.data, self.off, self.length
        if d.dtype != torch.uint8 or d.dim() != 1 or not d.is_contiguous():
            raise ValueError("PacketBatch.data must be a contiguous 1-D uint8 tensor")
        if not (0 <= int(self.bytes_len) and _round16(int(self.bytes_len)) <= d.numel()):
            raise ValueError(f"PacketBatch.data holds {d.numel()} bytes; bytes_len {self.bytes_len} needs "
                             f"{_round16(int(self.bytes_len))} (padded to 16)")
        if o.dtype != torch.int64 or o.dim() != 1 or not o.is_contiguous():
            raise ValueError("PacketBatch.off must be a contiguous 1-D int64 tensor")
        if ln.dtype != torch.int32 or ln.dim() != 1 or not ln.is_contiguous() or ln.numel() != o.numel():
            raise ValueError("PacketBatch.length must be a contiguous 1-D int32 tensor with one entry per offset")
        if o.device != d.device or ln.device != d.device:
            raise ValueError("PacketBatch tensors must be on one device")
        if int(self.max_len) < 0:
            raise ValueError("PacketBatch.max_len must be >= 0 (0 = unknown)")

    @property
    def n(self) -> int:
        return int(self.off.numel())

    @property
    def device(self) -> torch.device:
        return self.data.device

    @staticmethod
    def from_host(buf: np.ndarray, off: np.ndarray, length: np.ndarray, device="cuda") -> "PacketBatch":
        buf = np.ascontiguousarray(buf, dtype=np.uint8).ravel()
        bytes_len = int(buf.size)
        padded = np.zeros(_round16(bytes_len) or 16, dtype=np.uint8)
        padded[:bytes_len] = buf
        off = np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)
        length = np.ascontiguousarray(length, dtype=np.uint32).view(np.int32)
        max_len = int(length.view(np.uint32).max()) if length.size else 0
        return PacketBatch(
            data=torch.from_numpy(padded).to(device),
            off=torch.from_numpy(off.copy()).to(device),
            length=torch.from_numpy(length.copy()).to(device),
            bytes_len=bytes_len,
            max_len=max_len,
        )


def _ptr(t):
    return None if t is None else ctypes_ptr(t)


def _need(t: torch.Tensor | None, numel: int, dtype: torch.dtype, what: str, device: torch.device) -> None:
    """A caller-supplied array the kernel reads or writes numel elements of."""
    if t is None:
        return
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < numel or t.device != device:
        raise ValueError(f"{what}: need a contiguous {dtype} tensor of >= {numel} elements on {device}, got "
                         f"{t.dtype} x {t.numel()} on {t.device}")


def ctypes_ptr(t: torch.Tensor) -> int:
    if not t.is_cuda:
        raise ValueError("sccsum kernels need device tensors")
    return t.data_ptr()


def _stream(stream) -> int | None:
    s = torch.cuda.current_stream() if stream is None else stream
    return s.cuda_stream


def _scratch(numel: int, device, stream, dtype=torch.uint8) -> torch.Tensor:
    """A buffer the library fills or reads for kernels queued on `stream`
    (scratch, or an output the caller did not pass).  It is allocated on
    `stream` itself, so the caching allocator hands out a block whose earlier
    users on that stream are ordered before the launch (a block freed on
    another stream could still be read there when the kernel overwrites it,
    ADVICE r03), and it is recorded on torch's current stream, where the
    caller reads the results, so it is not reused before that stream is done
    with it either."""
    if stream is None or not torch.device(device).type == "cuda":
        return torch.empty(numel, dtype=dtype, device=device)
    with torch.cuda.stream(stream):
        t = torch.empty(numel, dtype=dtype, device=device)
    cur = torch.cuda.current_stream(t.device)
    if cur != stream:
        t.record_stream(cur)
    return t


def spans(batch: PacketBatch, seeds: torch.Tensor | None = None, out: torch.Tensor | None = None,
          status: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """sccsum_spans: one network-order uint16 checksum per span (int16 tensor)."""
    lib = native.load()
    n = batch.n
    if out is None:
        out = _scratch(max(n, 1), batch.device, stream, torch.int16)
    _need(out, n, torch.int16, "out", batch.device)
    _need(seeds, n, torch.int32, "seeds", batch.device)
    _need(status, n, torch.uint8, "status", batch.device)
    code = lib.sccsum_spans(
        ctypes_ptr(batch.data), batch.bytes_len, ctypes_ptr(batch.off), ctypes_ptr(batch.length),
        _ptr(seeds), ctypes_ptr(out), _ptr(status), n, batch.max_len, _stream(stream),
    )
    native.check(code, "sccsum_spans")
    return out[:n]


def ipv4_frames(batch: PacketBatch, out2: torch.Tensor | None = None, status: torch.Tensor | None = None,
                stream=None) -> torch.Tensor:
    """sccsum_ipv4_frames: [n, 2] int16 (IPv4 header checksum, L4 checksum)."""
    lib = native.load()
    n = batch.n
    if out2 is None:
        out2 = _scratch(max(2 * n, 2), batch.device, stream, torch.int16)
    _need(out2, 2 * n, torch.int16, "out2", batch.device)
    _need(status, n, torch.uint8, "status", batch.device)
    code = lib.sccsum_ipv4_frames(
        ctypes_ptr(batch.data), batch.bytes_len, ctypes_ptr(batch.off), ctypes_ptr(batch.length),
        ctypes_ptr(out2), _ptr(status), n, batch.max_len, _stream(stream),
    )
    native.check(code, "sccsum_ipv4_frames")
    return _pairs(out2, n)


def verify_frames(batch: PacketBatch, status: torch.Tensor, stream=None) -> torch.Tensor:
    """sccsum_ipv4_frames in verify-only form (no d_out2): per-frame status
    bits only — what the reference's verify keeps of the sum (ip.cc:121-127,
    tcp.hh:876-883: drop when get() != 0).  Returns status[:n]."""
    lib = native.load()
    n = batch.n
    if status is None:
        raise ValueError("verify_frames needs a status tensor")
    _need(status, n, torch.uint8, "status", batch.device)
    code = lib.sccsum_ipv4_frames(
        ctypes_ptr(batch.data), batch.bytes_len, ctypes_ptr(batch.off), ctypes_ptr(batch.length),
        None, ctypes_ptr(status), n, batch.max_len, _stream(stream),
    )
    native.check(code, "sccsum_ipv4_frames")
    return status[:n]


def _pairs(out2: torch.Tensor, n: int) -> torch.Tensor:
    """The [n, 2] view of a frames output (IPv4 header checksum, L4 checksum)."""
    return out2[: 2 * n].view(n, 2)


def _batch_array(items, width, seeds_ok, alloc_out, fill=False, stream=None):
    """The native.Batch array of items [(PacketBatch, out | None, status | None[, seeds]), ...]
    and their outputs.  width: out values per packet; seeds_ok: spans may carry
    seeds; alloc_out: a missing out is allocated on `stream`, else it stands for
    a verify-only batch, which needs its status; fill: every batch needs out."""
    rows = []
    for i, it in enumerate(items):  # every item is checked before any address is taken
        b, out, status = it[0], it[1], it[2]
        seeds = it[3] if len(it) > 3 else None
        if seeds is not None and not seeds_ok:
            raise ValueError("frames take no seeds")
        if fill and out is None:
            raise ValueError(f"batch {i}: a fill step needs out2 (the values pass through it)")
        if out is None and status is None and not alloc_out:
            raise ValueError(f"batch {i}: give out, status or both")
        _need(out, width * b.n, torch.int16, f"batch {i} out", b.device)
        _need(status, b.n, torch.uint8, f"batch {i} status", b.device)
        _need(seeds, b.n, torch.int32, f"batch {i} seeds", b.device)
        rows.append((b, out, status, seeds))
    arr = (native.Batch * max(len(rows), 1))()
    outs = []
    for i, (b, out, status, seeds) in enumerate(rows):
        if out is None and alloc_out:
            out = _scratch(max(width * b.n, width), b.device, stream, torch.int16)
        arr[i] = native.Batch(ctypes_ptr(b.data), b.bytes_len, ctypes_ptr(b.off), ctypes_ptr(b.length), _ptr(seeds),
                              _ptr(out), _ptr(status), b.n)
        outs.append(out)
    return arr, outs


def _multi(fn, name, items, max_len, stream, width, with_seed):
    if len(items) > native.MAX_BATCHES:
        raise ValueError(f"at most {native.MAX_BATCHES} batches per launch")
    arr, outs = _batch_array(items, width, with_seed, True, stream=stream)
    native.check(fn(ctypes.cast(arr, ctypes.c_void_p), len(items), max_len, _stream(stream)), name)
    return outs


def ipv4_frames_multi(items, stream=None) -> list:
    """sccsum_ipv4_frames_multi: items = [(PacketBatch, out2 | None, status | None), ...]
    (<= 16) in ONE launch; returns the [n, 2] int16 outputs per batch."""
    ml = max((it[0].max_len for it in items), default=0)
    outs = _multi(native.load().sccsum_ipv4_frames_multi, "sccsum_ipv4_frames_multi", items, ml, stream, 2, False)
    return [_pairs(o, it[0].n) for o, it in zip(outs, items)]


def prepare_ipv4_frames_multi(items):
    """A prebuilt sccsum_ipv4_frames_multi launch over fixed batches and
    outputs: returns launch(stream) that only crosses the C-ABI (no argument
    marshalling per call), for callers that relaunch the same batch set."""
    lib = native.load()
    if not items or len(items) > native.MAX_BATCHES:
        raise ValueError(f"1..{native.MAX_BATCHES} batches per launch")
    arr, _ = _batch_array(items, 2, False, False)  # out None: a verify-only batch (status bits only)
    ml = max(it[0].max_len for it in items)
    fn, ptr, nb = lib.sccsum_ipv4_frames_multi, ctypes.cast(arr, ctypes.c_void_p), len(items)

    def launch(stream):
        code = fn(ptr, nb, ml, stream.cuda_stream)
        if code:
            native.check(code, "sccsum_ipv4_frames_multi")

    launch.keep = (arr, items)  # the descriptors and tensors outlive the closure's callers
    return launch


def prepare_call(name: str, *args):
    """A prebuilt C-ABI call: tensors become device addresses once; the
    returned launch(stream) appends the stream handle and calls `name`."""
    lib = native.load()
    fn = getattr(lib, name)
    conv = tuple(ctypes_ptr(a) if isinstance(a, torch.Tensor) else a for a in args)

    def launch(stream):
        code = fn(*conv, stream.cuda_stream)
        if code:
            native.check(code, name)

    launch.keep = args
    return launch


def spans_multi(items, stream=None) -> list:
    """sccsum_spans_multi: items = [(PacketBatch, out | None, status | None[, seeds int32]), ...]."""
    ml = max((it[0].max_len for it in items), default=0)
    outs = _multi(native.load().sccsum_spans_multi, "sccsum_spans_multi", items, ml, stream, 1, True)
    return [o[: it[0].n] for o, it in zip(outs, items)]


def ipv4_fill(batch: PacketBatch, mode: int = native.FILL_IP | native.FILL_L4, out2: torch.Tensor | None = None,
              status: torch.Tensor | None = None, stream=None) -> torch.Tensor | None:
    """sccsum_ipv4_fill: generate checksums and store them in batch.data in
    place.  FILL_L4 / FILL_ICMP_ECHO read every byte: up to 524 288 frames
    (sccsum_set_fill_single_max) in one pass whose tiles store the fields
    themselves, a larger fill as two kernels on the stream (the generate pass
    into out2, then the field-store pass); the header-only modes read only
    the headers.  out2 / status are optional reports of what was stored;
    without out2 the generate pass's words go through a scratch buffer from
    torch's caching allocator (not the library's stream-ordered hipMallocAsync,
    which sits outside torch's pool and can fail when torch has cached most of
    HBM).  Returns the [n, 2] values stored when out2 is given
    (else None)."""
    lib = native.load()
    n = batch.n
    _need(out2, 2 * n, torch.int16, "out2", batch.device)
    _need(status, n, torch.uint8, "status", batch.device)
    vals = out2
    if vals is None and mode & (native.FILL_L4 | native.FILL_ICMP_ECHO) and n:
        vals = _scratch(2 * n, batch.device, stream, torch.int16)
    code = lib.sccsum_ipv4_fill(
        ctypes_ptr(batch.data), batch.bytes_len, ctypes_ptr(batch.off), ctypes_ptr(batch.length),
        _ptr(vals), _ptr(status), n, batch.max_len, mode, _stream(stream),
    )
    native.check(code, "sccsum_ipv4_fill")
    return None if out2 is None else _pairs(out2, n)


# The reference's default RSS key (Mellanox driver key, toeplitz.hh:52-58).
RSS_KEY_40 = bytes.fromhex("d181c62cf7f4db5b1983a2fc943e1adbd9389e6bd1039c2ca74499ad593d56d9f3253c062adc1ffc")


def _key(key: bytes):
    kb = bytes(key)
    return (ctypes.c_uint8 * len(kb)).from_buffer_copy(kb), len(kb)


def ipv4_rss(batch: PacketBatch, key: bytes = RSS_KEY_40, mode: int = native.RSS_DISPATCH,
             hash_out: torch.Tensor | None = None, status: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """sccsum_ipv4_rss: the Toeplitz RSS hash of every frame (int32 tensor [n])."""
    lib = native.load()
    n = batch.n
    if hash_out is None:
        hash_out = _scratch(max(n, 1), batch.device, stream, torch.int32)
    _need(hash_out, n, torch.int32, "hash_out", batch.device)
    _need(status, n, torch.uint8, "status", batch.device)
    kb, kl = _key(key)
    code = lib.sccsum_ipv4_rss(ctypes_ptr(batch.data), batch.bytes_len, ctypes_ptr(batch.off),
                               ctypes_ptr(batch.length), ctypes.addressof(kb), kl, mode, ctypes_ptr(hash_out),
                               _ptr(status), n, _stream(stream))
    native.check(code, "sccsum_ipv4_rss")
    return hash_out[:n]


def ipv4_frames_rss(batch: PacketBatch, key: bytes = RSS_KEY_40, mode: int = native.RSS_DISPATCH,
                    out2: torch.Tensor | None = None, status: torch.Tensor | None = None,
                    hash_out: torch.Tensor | None = None, stream=None):
    """sccsum_ipv4_frames_rss: ([n, 2] int16 checksums, [n] int32 RSS hashes) in one pass."""
    lib = native.load()
    n = batch.n
    if out2 is None:
        out2 = _scratch(max(2 * n, 2), batch.device, stream, torch.int16)
    if hash_out is None:
        hash_out = _scratch(max(n, 1), batch.device, stream, torch.int32)
    _need(out2, 2 * n, torch.int16, "out2", batch.device)
    _need(hash_out, n, torch.int32, "hash_out", batch.device)
    _need(status, n, torch.uint8, "status", batch.device)
    kb, kl = _key(key)
    code = lib.sccsum_ipv4_frames_rss(
        ctypes_ptr(batch.data), batch.bytes_len, ctypes_ptr(batch.off), ctypes_ptr(batch.length), ctypes_ptr(out2),
        _ptr(status), n, batch.max_len, ctypes.addressof(kb), kl, mode, ctypes_ptr(hash_out), _stream(stream))
    native.check(code, "sccsum_ipv4_frames_rss")
    return _pairs(out2, n), hash_out[:n]


def fragments(data: torch.Tensor, bytes_len: int, frag_off: torch.Tensor, frag_len: torch.Tensor,
              pkt_first: torch.Tensor, seeds: torch.Tensor | None = None, out: torch.Tensor | None = None,
              status: torch.Tensor | None = None, max_frag_len: int = 0, stream=None) -> torch.Tensor:
    """sccsum_fragments: one checksum per fragment-list packet (int16 tensor)."""
    lib = native.load()
    n = int(pkt_first.numel()) - 1
    nfrag = int(frag_off.numel())
    if out is None:
        out = _scratch(max(n, 1), data.device, stream, torch.int16)
    dev = data.device
    if n < 0:
        raise ValueError("pkt_first needs n + 1 entries")
    _need(frag_off, nfrag, torch.int64, "frag_off", dev)
    _need(frag_len, nfrag, torch.int32, "frag_len", dev)
    _need(pkt_first, n + 1, torch.int32, "pkt_first", dev)
    _need(seeds, n, torch.int32, "seeds", dev)
    _need(out, n, torch.int16, "out", dev)
    _need(status, n, torch.uint8, "status", dev)
    ws = _scratch(int(lib.sccsum_fragments_workspace(nfrag)), data.device, stream)
    code = lib.sccsum_fragments(
        ctypes_ptr(data), bytes_len, ctypes_ptr(frag_off), ctypes_ptr(frag_len), nfrag, ctypes_ptr(pkt_first),
        _ptr(seeds), ctypes_ptr(out), _ptr(status), n, max_frag_len, ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_fragments")
    return out[:n]


DESC_DTYPE = np.dtype([("src", "<u8"), ("dst_off", "<u4"), ("len", "<u4")])  # sccsum_gather_desc


def make_desc(src, dst_off, length) -> np.ndarray:
    """sccsum_gather_desc records: src = absolute device-readable addresses
    (0 = in the stage buffer at dst_off), dst_off = the fragment's position in
    the packet layout (packet offset + offset inside the packet), length."""
    d = np.zeros(len(length), dtype=DESC_DTYPE)
    d["src"] = src
    d["dst_off"] = dst_off
    d["len"] = length
    return d


def _desc_call(name, desc, first, off, length, max_len, width, seeds, stage, out, status, stream):
    lib = native.load()
    n = int(off.numel())
    dev = off.device
    if int(first.numel()) != n + 1 or first.dtype != torch.int32 or (desc is not None and desc.dtype != torch.uint8):
        raise ValueError(f"{name}: first must be int32 [n + 1] and desc uint8 records (or None: no fragments)")
    if out is None:
        out = _scratch(max(width * n, width), dev, stream, torch.int16)
    _need(length, n, torch.int32, "length", dev)
    _need(seeds, n, torch.int32, "seeds", dev)
    _need(out, width * n, torch.int16, "out", dev)
    _need(status, n, torch.uint8, "status", dev)
    args = [_ptr(desc), ctypes_ptr(first), ctypes_ptr(off), ctypes_ptr(length)]
    if width == 1:
        args.append(_ptr(seeds))
    args += [None if stage is None else ctypes_ptr(stage), ctypes_ptr(out), _ptr(status), n, max_len, _stream(stream)]
    native.check(getattr(lib, name)(*args), name)
    return out


def spans_desc(desc: torch.Tensor, first: torch.Tensor, off: torch.Tensor, length: torch.Tensor, max_len: int,
               seeds: torch.Tensor | None = None, stage: torch.Tensor | None = None, out: torch.Tensor | None = None,
               status: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """sccsum_spans_desc: packets as fragment lists summed where the fragments
    lie (desc = make_desc records as a uint8 device tensor, first = int32
    [n + 1]); one int16 checksum per packet."""
    n = int(off.numel())
    return _desc_call("sccsum_spans_desc", desc, first, off, length, max_len, 1, seeds, stage, out, status,
                      stream)[:n]


def ipv4_frames_desc(desc: torch.Tensor, first: torch.Tensor, off: torch.Tensor, length: torch.Tensor, max_len: int,
                     stage: torch.Tensor | None = None, out2: torch.Tensor | None = None,
                     status: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """sccsum_ipv4_frames_desc: frames as fragment lists; [n, 2] int16."""
    n = int(off.numel())
    out2 = _desc_call("sccsum_ipv4_frames_desc", desc, first, off, length, max_len, 2, None, stage, out2, status,
                      stream)
    return _pairs(out2, n)


def ipv4_fill_desc(desc: torch.Tensor, first: torch.Tensor, off: torch.Tensor, length: torch.Tensor, max_len: int,
                   mode: int = native.FILL_IP | native.FILL_L4, stage: torch.Tensor | None = None,
                   out2: torch.Tensor | None = None, status: torch.Tensor | None = None,
                   stream=None) -> torch.Tensor:
    """sccsum_ipv4_fill_desc: generate the checksums of frames given as
    fragment lists and store them where the fragments lie (the memory behind
    the descriptors, or `stage`, is written).  Returns the values stored,
    [n, 2] int16 (IP, L4; 0 where nothing was stored)."""
    lib = native.load()
    name = "sccsum_ipv4_fill_desc"
    n = int(off.numel())
    dev = off.device
    if int(first.numel()) != n + 1 or first.dtype != torch.int32 or (desc is not None and desc.dtype != torch.uint8):
        raise ValueError(f"{name}: first must be int32 [n + 1] and desc uint8 records (or None: no fragments)")
    _need(off, n, torch.int64, "off", dev)
    _need(length, n, torch.int32, "length", dev)
    _need(first, n + 1, torch.int32, "first", dev)
    _need(desc, 0, torch.uint8, "desc", dev)
    _need(stage, 0, torch.uint8, "stage", dev)
    _need(out2, 2 * n, torch.int16, "out2", dev)
    _need(status, n, torch.uint8, "status", dev)
    if out2 is None:
        out2 = _scratch(max(2 * n, 2), dev, stream, torch.int16)
    native.check(lib.sccsum_ipv4_fill_desc(_ptr(desc), ctypes_ptr(first), ctypes_ptr(off), ctypes_ptr(length),
                                           _ptr(stage), ctypes_ptr(out2), _ptr(status), n, max_len, mode,
                                           _stream(stream)), name)
    return _pairs(out2, n)


def read_probe(buf: torch.Tensor, nbytes: int, sink: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Stream-read nbytes of buf with the kernels' load shape (HBM ceiling probe)."""
    lib = native.load()
    if sink is None:
        sink = torch.zeros(lib.sccsum_read_probe_blocks(), dtype=torch.int64, device=buf.device)
    native.check(lib.sccsum_read_probe(ctypes_ptr(buf), nbytes & ~15, ctypes_ptr(sink), _stream(stream)),
                 "sccsum_read_probe")
    return sink


def as_u16(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.uint16)


def pseudo_seed(src_host: int, dst_host: int, proto: int, length: int) -> int:
    return int(native.load().sccsum_pseudo_seed(src_host, dst_host, proto, length & 0xFFFF))


def build_reta(weights: dict) -> np.ndarray:
    """sccsum_steer_build_reta: qp::build_sw_reta (net.cc:214-231) for a
    {cpu: weight} map, iterated in ascending cpu order like the reference's
    std::map; the 128-entry table as uint8."""
    cpus = sorted(int(c) for c in weights)
    if not cpus or cpus[0] < 0:
        raise ValueError("build_reta: need at least one cpu >= 0")
    c = np.array(cpus, dtype=np.uint32)
    w = np.array([weights[k] for k in sorted(weights, key=int)], dtype=np.float32)
    out = np.zeros(native.RETA_SIZE, dtype=np.uint8)
    native.check(native.load().sccsum_steer_build_reta(c.ctypes.data, w.ctypes.data, len(cpus), out.ctypes.data),
                 "sccsum_steer_build_reta")
    return out


def _steer_map(ncpu, sw_reta, hw_queues, redir, table_bits, sw_reta_set):
    """(native.SteerMap, the numpy arrays it points into)."""
    reta = np.ascontiguousarray(sw_reta, dtype=np.uint8)
    if reta.ndim == 1:
        reta = reta.reshape(1, -1)
    if hw_queues is None:
        hw_queues = reta.shape[0]
    if reta.ndim != 2 or reta.shape != (int(hw_queues), native.RETA_SIZE):
        raise ValueError(f"sw_reta: need [hw_queues={hw_queues}][{native.RETA_SIZE}] uint8 entries, got {reta.shape}")
    rd = None if redir is None else np.ascontiguousarray(redir, dtype=np.uint8).ravel()
    has = None if sw_reta_set is None else np.ascontiguousarray(sw_reta_set, dtype=np.uint8).ravel()
    if has is not None and has.size != int(hw_queues):
        raise ValueError(f"sw_reta_set: need {hw_queues} entries, got {has.size}")
    m = native.SteerMap(int(ncpu), int(hw_queues), int(table_bits), 0 if rd is None else int(rd.size),
                        None if rd is None else rd.ctypes.data, reta.ctypes.data,
                        None if has is None else has.ctypes.data)
    return m, (reta, rd, has)


def steer_dest(hash_value: int, ncpu: int, sw_reta, hw_queues: int | None = None, redir=None, table_bits: int = 0,
               sw_reta_set=None, mode: int = native.STEER_HASH2CPU, src_cpu: int = 0) -> int:
    """sccsum_steer_dest: one hash through the map on the host (device::hash2cpu /
    forward_dst, net.hh:291-305)."""
    m, keep = _steer_map(ncpu, sw_reta, hw_queues, redir, table_bits, sw_reta_set)
    d = int(native.load().sccsum_steer_dest(ctypes.addressof(m), int(mode), int(src_cpu), int(hash_value) & 0xFFFFFFFF))
    del keep
    if d == 0xFFFFFFFF:
        raise ValueError("steer_dest: bad map or mode")
    return d


class _DeviceObject:
    """What every object that owns a C-ABI handle does with it: `handle` for
    the calls (an error once closed), close(), and a __del__ that stays quiet
    at interpreter shutdown.  A subclass names its destroy call and itself as
    error messages do, and once its create call has succeeded hands the handle
    and its device to _own()."""
    _destroy = ""   # the C-ABI call that frees the handle
    _a = ""         # the class with its article: "an ArpTable"
    _h = None
    device = None   # torch.device, or None for a host-only table

    def __init__(self):
        self._lib = native.load()

    def _own(self, h, device) -> None:
        self._h = h
        self.device = None if device is None else torch.device("cuda", int(device))

    @property
    def handle(self):
        if self._h is None:
            raise ValueError(f"{type(self).__name__} is closed")
        return self._h

    def close(self) -> None:
        h, self._h = self._h, None
        if h is not None:
            native.check(getattr(self._lib, self._destroy)(h), self._destroy)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def _device_handle(obj, cls, dev, what: str, optional: bool = False):
    """The handle of a table of class `cls` for a call on data that lives on `dev`."""
    if obj is None and optional:
        return None
    if not isinstance(obj, cls):
        raise ValueError(f"{what}: need {cls._a}")
    if obj.device != dev:
        raise ValueError(f"{what}: the table lives on {obj.device}, the data on {dev}")
    return obj.handle


class Steer(_DeviceObject):
    """sccsum_steer_*: rx steering of a batch on the device (include/sccsum.h,
    "Rx steering"): every packet's destination shard from its RSS hash, and the
    batch's packet indices grouped by shard in arrival order.

        st = Steer(ncpu=16, sw_reta=build_reta({c: 1.0 for c in range(16)}))
        cpu, order, first = st.run(hashes, status, need=ST_OK, reject=ST_MALFORMED | ST_RANGE)
        # shard c's packets: order[first[c]:first[c + 1]]; the dropped ones: order[first[ncpu]:first[ncpu + 1]]

    sw_reta is [hw_queues][128] (one row may be given flat); sw_reta_set marks
    the queues that have one (None: all).  The object is immutable and may be
    run from any thread on any stream of its device."""
    _destroy, _a = "sccsum_steer_destroy", "a Steer"

    def __init__(self, ncpu: int, sw_reta, hw_queues: int | None = None, redir=None, table_bits: int = 0,
                 sw_reta_set=None, device: int = 0):
        super().__init__()
        m, keep = _steer_map(ncpu, sw_reta, hw_queues, redir, table_bits, sw_reta_set)
        h = ctypes.c_void_p()
        native.check(self._lib.sccsum_steer_create(int(device), ctypes.addressof(m), ctypes.byref(h)),
                     "sccsum_steer_create")
        del keep
        self._own(h, device)
        self.ncpu = int(ncpu)

    @staticmethod
    def check_args(dev, ncpu, hashes, status, need, reject, cpu, order, first) -> int:
        """What run() refuses before any launch (the kernels trust the sizes); returns n."""
        if (not isinstance(hashes, torch.Tensor) or hashes.dtype != torch.int32 or hashes.dim() != 1
                or not hashes.is_contiguous() or hashes.device != dev):
            raise ValueError(f"hashes: need a contiguous 1-D int32 tensor on {dev}")
        n = int(hashes.numel())
        _need(status, n, torch.uint8, "status", dev)
        if status is None and (need or reject):
            raise ValueError("need / reject masks without a status array")
        _need(cpu, n, torch.uint8, "cpu", dev)
        _need(order, n, torch.int32, "order", dev)
        _need(first, ncpu + 2, torch.int32, "first", dev)
        return n

    def workspace_bytes(self, n: int) -> int:
        return int(self._lib.sccsum_steer_workspace(self._h, int(n)))

    def run(self, hashes: torch.Tensor, status: torch.Tensor | None = None, need: int = 0, reject: int = 0,
            mode: int = native.STEER_HASH2CPU, src_cpu: int = 0, stream=None, cpu: torch.Tensor | None = None,
            order: torch.Tensor | None = None, first: torch.Tensor | None = None,
            workspace: torch.Tensor | None = None, want_cpu: bool = True, want_order: bool = True):
        """(cpu uint8 [n], order int32 [n], first int32 [ncpu + 2]); cpu / order
        are None when want_cpu / want_order is False and no tensor was passed.
        Indices and counts are uint32 values in int32 tensors."""
        handle = self.handle
        dev = self.device
        n = self.check_args(dev, self.ncpu, hashes, status, need, reject, cpu, order, first)
        if cpu is None and want_cpu:
            cpu = _scratch(max(n, 1), dev, stream, torch.uint8)
        if order is None and want_order:
            order = _scratch(max(n, 1), dev, stream, torch.int32)
        if first is None:
            first = _scratch(self.ncpu + 2, dev, stream, torch.int32)
        ws_bytes = self.workspace_bytes(n)
        if workspace is None:
            workspace = _scratch(ws_bytes, dev, stream)
        _need(workspace, ws_bytes, torch.uint8, "workspace", dev)
        if n == 0:  # an empty tensor has no address: nothing to drop, only first is written
            status, need, reject = None, 0, 0
        code = self._lib.sccsum_steer_run(handle, int(mode), int(src_cpu), ctypes_ptr(hashes), _ptr(status),
                                          int(need), int(reject), n, _ptr(cpu), _ptr(order), ctypes_ptr(first),
                                          ctypes_ptr(workspace), _stream(stream))
        native.check(code, "sccsum_steer_run")
        return (None if cpu is None else cpu[:n]), (None if order is None else order[:n]), first[: self.ncpu + 2]


@dataclass
class SendResult:
    """What sccsum_ipv4_send wrote (include/sccsum.h, "Tx send").  The per-frame
    tensors have room for max_frames frames; frames_emitted() of them are
    written.  (desc, first, out_off, out_len) sliced to the emitted frames are
    the arguments of the *_desc calls; lists() returns them so."""
    l4: PacketBatch          # the datagrams (the payload descriptors point into l4.data)
    hdr: torch.Tensor        # uint8 [20 * max_frames]
    desc: torch.Tensor       # uint8 [32 * max_frames]: two sccsum_gather_desc records per frame
    first: torch.Tensor      # int32 [max_frames + 1]: 2f, and the closing entry
    out_off: torch.Tensor    # int64 [max_frames]: the frame's position in the packed layout
    out_len: torch.Tensor    # int32 [max_frames]
    dgram_first: torch.Tensor  # int32 [n + 1]: datagram i's first frame
    status: torch.Tensor     # uint8 [n]
    total: torch.Tensor      # int64 [3]: frames needed, bytes needed, datagrams emitted
    max_frames: int
    max_out_bytes: int

    def totals(self) -> tuple:
        """(frames needed, layout bytes needed, datagrams emitted); synchronises."""
        t = self.total.cpu().numpy()
        return int(t[0]), int(t[1]), int(t[2])

    def frames_emitted(self) -> int:
        """Frames written (synchronises)."""
        return int(self.dgram_first[-1].item()) & 0xFFFFFFFF

    def lists(self) -> tuple:
        """(desc, first, out_off, out_len, max_len) of the emitted frames, as
        ipv4_frames_desc / ipv4_fill_desc / spans_desc take them; synchronises."""
        e = self.frames_emitted()
        ln = self.out_len[:e]
        return self.desc[: 32 * e], self.first[: e + 1], self.out_off[:e], ln, (int(ln.max().item()) if e else 0)

    def pack(self, stream=None) -> PacketBatch:
        """The packed wire frames: sccsum_gather of every header and piece into
        a new buffer (the one pass that moves payload bytes); synchronises to
        size it."""
        desc, _, off, ln, max_len = self.lists()
        e = int(off.numel())
        nbytes = int((off[-1] + ln[-1]).item()) if e else 0
        data = _scratch(_round16(nbytes) or 16, self.l4.device, stream)
        if e:
            native.check(native.load().sccsum_gather(ctypes_ptr(desc), 2 * e, ctypes_ptr(data), _stream(stream)),
                         "sccsum_gather")
        return PacketBatch(data=data, off=off, length=ln, bytes_len=nbytes, max_len=max_len)


def send_check(l4: PacketBatch, dst, proto, mtu, src_host, ids, l4sum, flags, max_frames, max_out_bytes) -> tuple:
    """What ipv4_send refuses before any launch (the kernels trust the sizes);
    returns (n, max_frames, max_out_bytes) with the default caps filled in:
    every datagram needs at most ceil(len / (mtu - 20)) + 1 frames, so datagrams
    that do not overlap need at most bytes_len // (mtu - 20) + 2 n."""
    if not isinstance(l4, PacketBatch):
        raise ValueError("l4: need a PacketBatch of L4 datagrams")
    dev, n = l4.device, l4.n
    if not 68 <= int(mtu) <= 65535:
        raise ValueError(f"mtu: need 68..65535, got {mtu}")
    if int(flags) & ~(native.SEND_TSO | native.SEND_UFO | native.SEND_NO_IP_CSUM | native.SEND_L4):
        raise ValueError(f"flags: unknown bits in {int(flags):#x}")
    if not 0 <= int(src_host) <= 0xFFFFFFFF:
        raise ValueError("src_host: need a host-order IPv4 address, 0..2^32-1")
    if n > 0xFFFFFFFF:
        raise ValueError("l4: at most 2^32-1 datagrams")
    for t, dtype, what in ((dst, torch.int32, "dst"), (proto, torch.uint8, "proto")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError(f"{what}: need a 1-D {dtype} tensor of one entry per datagram")
        _need(t, n, dtype, what, dev)
    for t, what in ((ids, "ids"), (l4sum, "l4sum")):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 1):
            raise ValueError(f"{what}: need a 1-D int16 tensor of one entry per datagram")
        _need(t, n, torch.int16, what, dev)
    if bool(int(flags) & native.SEND_L4) != (l4sum is not None):
        raise ValueError("l4sum: needed with SEND_L4, and only with it")
    if max_frames is None:
        max_frames = min(0x7FFFFFFF, 2 * n + l4.bytes_len // (int(mtu) - 20))
    if max_out_bytes is None:
        max_out_bytes = min(0xFFFFFFFF, l4.bytes_len + 20 * int(max_frames))
    if not 0 <= int(max_frames) <= 0x7FFFFFFF:
        raise ValueError("max_frames: need 0..2^31-1")
    if not 0 <= int(max_out_bytes) <= 0xFFFFFFFF:
        raise ValueError("max_out_bytes: need 0..2^32-1 (descriptor offsets are 32-bit)")
    return n, int(max_frames), int(max_out_bytes)


def ipv4_send(l4: PacketBatch, dst: torch.Tensor, proto: torch.Tensor, mtu: int, src_host: int,
              ids: torch.Tensor | None = None, l4sum: torch.Tensor | None = None, flags: int = 0,
              max_frames: int | None = None, max_out_bytes: int | None = None, stream=None) -> SendResult:
    """sccsum_ipv4_send: ipv4::send (ip.cc:244-299) for a batch of L4 datagrams
    on the device — every frame's IPv4 header and, past the MTU, the cut into
    fragments, as header + payload fragment lists; no payload byte moves.

        seeds = ...pseudo_seed(src, dst, proto, len) per datagram, fields zero
        l4sum = spans(l4, seeds=seeds)
        r = ipv4_send(l4, dst, proto, 1500, src, ids=ids, l4sum=l4sum, flags=native.SEND_L4)
        frames = r.pack()                      # or ipv4_fill_desc(*r.lists()[:4], r.lists()[4]) where they lie

    dst: int32 [n] (host-order addresses as uint32 values), proto: uint8 [n],
    ids / l4sum: int16 [n].  Capacity is a prefix rule: r.totals() reports the
    full need and how many datagrams were emitted."""
    lib = native.load()
    n, max_frames, max_out_bytes = send_check(l4, dst, proto, mtu, src_host, ids, l4sum, flags, max_frames,
                                              max_out_bytes)
    dev = l4.device
    hdr = _scratch(20 * max(max_frames, 1), dev, stream)
    desc = _scratch(32 * max(max_frames, 1), dev, stream)
    first = _scratch(max_frames + 1, dev, stream, torch.int32)
    out_off = _scratch(max(max_frames, 1), dev, stream, torch.int64)
    out_len = _scratch(max(max_frames, 1), dev, stream, torch.int32)
    dgram_first = _scratch(n + 1, dev, stream, torch.int32)
    status = _scratch(max(n, 1), dev, stream, torch.uint8)
    total = _scratch(3, dev, stream, torch.int64)
    ws = _scratch(int(lib.sccsum_ipv4_send_workspace(n)), dev, stream)
    opts = native.SendOpts(int(src_host), int(mtu), int(flags))
    empty = n == 0  # an empty tensor has no address
    code = lib.sccsum_ipv4_send(
        ctypes.addressof(opts), ctypes_ptr(l4.data), l4.bytes_len, None if empty else ctypes_ptr(l4.off),
        None if empty else ctypes_ptr(l4.length), None if empty else ctypes_ptr(dst),
        None if empty else ctypes_ptr(proto), None if empty else _ptr(ids), None if empty else _ptr(l4sum), n,
        max_frames, max_out_bytes, ctypes_ptr(hdr), ctypes_ptr(desc), ctypes_ptr(first), ctypes_ptr(out_off),
        ctypes_ptr(out_len), ctypes_ptr(dgram_first), ctypes_ptr(status), ctypes_ptr(total), ctypes_ptr(ws),
        _stream(stream))
    native.check(code, "sccsum_ipv4_send")
    return SendResult(l4=l4, hdr=hdr, desc=desc, first=first, out_off=out_off[:max_frames],
                      out_len=out_len[:max_frames], dgram_first=dgram_first, status=status[:n], total=total,
                      max_frames=max_frames, max_out_bytes=max_out_bytes)


# sccsum_frag_rec
REC_DTYPE = np.dtype([("frame", "<u8"), ("src", "<u4"), ("dst", "<u4"), ("id", "<u2"), ("proto", "u1"), ("mf", "u1"),
                      ("offset", "<u2"), ("hdr_len", "<u2"), ("len", "<u2"), ("reserved", "<u2"), ("tag", "<u4")])
REC_BYTES = REC_DTYPE.itemsize  # 32
FRAG_NEED = native.ST_OK | native.ST_IPFRAG          # the fragments ip.cc:121-144 lets through
FRAG_REJECT = native.ST_MALFORMED | native.ST_RANGE


def _status_masks(need, reject) -> None:
    for v, what in ((need, "need"), (reject, "reject")):
        if not 0 <= int(v) <= 0xFF:
            raise ValueError(f"{what}: need a mask of status bits, 0..0xFF")


def frag_records_check(b: PacketBatch, status, need, reject, host_address, tag) -> int:
    """What frag_records refuses before any launch; returns n."""
    if not isinstance(b, PacketBatch):
        raise ValueError("b: need a PacketBatch of IPv4 frames")
    n = b.n
    if n > native.REASM_MAX_RECORDS:
        raise ValueError("b: at most 2^31-1 frames")
    if not isinstance(status, torch.Tensor) or status.dim() != 1:
        raise ValueError("status: need the 1-D uint8 tensor the frames call wrote, one entry per frame")
    _need(status, n, torch.uint8, "status", b.device)
    _status_masks(need, reject)
    for v, what in ((host_address, "host_address"), (tag, "tag")):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{what}: need 0..2^32-1")
    return n


def frag_records(b: PacketBatch, status: torch.Tensor, need: int = FRAG_NEED, reject: int = FRAG_REJECT,
                 host_address: int = 0, tag: int = 0, stream=None) -> torch.Tensor:
    """sccsum_ipv4_frag_records: the accepted frames of a frames batch as
    sccsum_frag_rec records (REC_DTYPE), in arrival order: a uint8 tensor of 32
    bytes per record.  Synchronises to size it.  The records point into b.data,
    which must stay alive while one of them is pending."""
    lib = native.load()
    n = frag_records_check(b, status, need, reject, host_address, tag)
    dev = b.device
    rec = _scratch(REC_BYTES * max(n, 1), dev, stream)
    count = _scratch(1, dev, stream, torch.int32)
    ws = _scratch(int(lib.sccsum_ipv4_reasm_workspace(n)), dev, stream)
    empty = n == 0  # an empty tensor has no address
    code = lib.sccsum_ipv4_frag_records(
        ctypes_ptr(b.data), b.bytes_len, None if empty else ctypes_ptr(b.off), None if empty else ctypes_ptr(b.length),
        None if empty else ctypes_ptr(status), int(need), int(reject), n, int(host_address), int(tag),
        ctypes_ptr(rec), ctypes_ptr(count), ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_ipv4_frag_records")
    if stream is not None:
        stream.synchronize()
    return rec[: REC_BYTES * (int(count.item()) & 0xFFFFFFFF)]


@dataclass
class ReasmResult:
    """What sccsum_ipv4_reasm wrote (include/sccsum.h, "Rx reassembly").  Every
    tensor has room for m entries; totals() says how many are written."""
    records: torch.Tensor      # uint8 [32 m]: the input
    desc: torch.Tensor         # uint8 [16 m]: one sccsum_gather_desc per record of an emitted datagram
    dgram_first: torch.Tensor  # int32 [m + 1]: CSR index into desc, and the closing entry
    dgram_off: torch.Tensor    # int64 [m]: the datagram's position in the packed layout
    dgram_len: torch.Tensor    # int32 [m]
    dgram_seed: torch.Tensor   # int32 [m]: the pseudo-header seed (0: not TCP / UDP)
    dgram_head: torch.Tensor   # int32 [m]: index of the offset-0 record
    dgram_last: torch.Tensor   # int32 [m]: index of the completing record
    dgram_hash: torch.Tensor | None  # int32 [m] when a key was given
    pending_buf: torch.Tensor  # uint8 [32 m]
    host_buf: torch.Tensor     # uint8 [32 m]
    rec_state: torch.Tensor    # uint8 [m]: native.REASM_COMPLETE / _PENDING / _HOST
    total: torch.Tensor        # int64 [4]
    m: int

    def totals(self) -> tuple:
        """(datagrams, descriptors, pending records, host records); synchronises."""
        t = self.total.cpu().numpy()
        return int(t[0]), int(t[1]), int(t[2]), int(t[3])

    def lists(self) -> tuple:
        """(desc, first, off, length, seeds, max_len) of the delivered
        datagrams, as spans_desc takes them; synchronises."""
        d, k, _, _ = self.totals()
        ln = self.dgram_len[:d]
        return (self.desc[: 16 * k], self.dgram_first[: d + 1], self.dgram_off[:d], ln, self.dgram_seed[:d],
                (int(ln.max().item()) if d else 0))

    @property
    def hashes(self) -> torch.Tensor | None:
        """The delivered datagrams' RSS hashes, as Steer.run takes them; synchronises."""
        return None if self.dgram_hash is None else self.dgram_hash[: self.totals()[0]]

    @property
    def pending(self) -> torch.Tensor:
        """The records to put in front of the next call's; synchronises."""
        return self.pending_buf[: REC_BYTES * self.totals()[2]]

    @property
    def host(self) -> torch.Tensor:
        """The records of the keys the host replays through the reference's merger; synchronises."""
        return self.host_buf[: REC_BYTES * self.totals()[3]]

    def pack(self, stream=None) -> PacketBatch:
        """The delivered datagrams packed back to back: sccsum_gather of every
        piece into a new buffer (the one pass that moves payload bytes);
        synchronises to size it."""
        desc, _, off, ln, _, max_len = self.lists()
        d = int(off.numel())
        nbytes = int((off[-1] + ln[-1]).item()) if d else 0
        data = _scratch(_round16(nbytes) or 16, self.records.device, stream)
        if d:
            native.check(native.load().sccsum_gather(ctypes_ptr(desc), int(desc.numel()) // 16, ctypes_ptr(data),
                                                     _stream(stream)), "sccsum_gather")
        return PacketBatch(data=data, off=off, length=ln, bytes_len=nbytes, max_len=max_len)


def reasm_check(records, key, max_out_bytes) -> int:
    """What reassemble refuses before any launch; returns m."""
    if (not isinstance(records, torch.Tensor) or records.dtype != torch.uint8 or records.dim() != 1
            or not records.is_contiguous() or records.numel() % REC_BYTES):
        raise ValueError("records: need a contiguous 1-D uint8 tensor of 32-byte sccsum_frag_rec records")
    if not records.is_cuda:
        raise ValueError("records: need a device tensor")
    m = int(records.numel()) // REC_BYTES
    if m > native.REASM_MAX_RECORDS:
        raise ValueError("records: at most 2^31-1 records")
    if m and records.data_ptr() % 8:
        raise ValueError("records: need 8-byte alignment")
    if key is not None and len(bytes(key)) < 4:
        raise ValueError("key: need at least 4 bytes")
    if not 0 <= int(max_out_bytes) <= 0xFFFFFFFF:
        raise ValueError("max_out_bytes: need 0..2^32-1 (descriptor offsets are 32-bit)")
    return m


def reassemble(records: torch.Tensor, key: bytes | None = None, max_out_bytes: int = 0xFFFFFFFF,
               stream=None) -> ReasmResult:
    """sccsum_ipv4_reasm: ipv4::handle_received_packet's reassembly branch
    (ip.cc:164-220) for a batch of fragment records on the device — complete
    datagrams as fragment lists in completion order, and the pending and host
    buckets; no payload byte moves.

        status = torch.empty(b.n, dtype=torch.uint8, device=dev)
        _, hashes = ipv4_frames_rss(b, key, status=status)
        recs = frag_records(b, status, host_address=me, tag=now)
        r = reassemble(torch.cat([carry, recs]), key=key)
        desc, first, off, length, seeds, max_len = r.lists()
        l4 = spans_desc(desc, first, off, length, max_len, seeds=seeds)      # 0 = the L4 checksum verifies
        steer.run(r.hashes)
        carry = r.pending.clone()
    """
    lib = native.load()
    m = reasm_check(records, key, max_out_bytes)
    dev = records.device
    k = max(m, 1)
    t = dict(desc=_scratch(16 * k, dev, stream), dgram_first=_scratch(m + 1, dev, stream, torch.int32),
             dgram_off=_scratch(k, dev, stream, torch.int64), dgram_len=_scratch(k, dev, stream, torch.int32),
             dgram_seed=_scratch(k, dev, stream, torch.int32), dgram_head=_scratch(k, dev, stream, torch.int32),
             dgram_last=_scratch(k, dev, stream, torch.int32),
             dgram_hash=None if key is None else _scratch(k, dev, stream, torch.int32),
             pending_buf=_scratch(REC_BYTES * k, dev, stream), host_buf=_scratch(REC_BYTES * k, dev, stream),
             rec_state=_scratch(k, dev, stream, torch.uint8), total=_scratch(4, dev, stream, torch.int64))
    ws = _scratch(int(lib.sccsum_ipv4_reasm_workspace(m)) or 16, dev, stream)
    out = native.ReasmOut(*[_ptr(t[name]) for name in
                            ("desc", "dgram_first", "dgram_off", "dgram_len", "dgram_seed", "dgram_head", "dgram_last",
                             "dgram_hash", "pending_buf", "host_buf", "rec_state", "total")])
    kb, kl = (None, 0) if key is None else _key(key)
    code = lib.sccsum_ipv4_reasm(ctypes_ptr(records) if m else None, m, int(max_out_bytes),
                                 None if kb is None else ctypes.addressof(kb), kl, ctypes.addressof(out),
                                 ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_ipv4_reasm")
    return ReasmResult(records=records, desc=t["desc"], dgram_first=t["dgram_first"], dgram_off=t["dgram_off"][:m],
                       dgram_len=t["dgram_len"][:m], dgram_seed=t["dgram_seed"][:m], dgram_head=t["dgram_head"][:m],
                       dgram_last=t["dgram_last"][:m],
                       dgram_hash=None if t["dgram_hash"] is None else t["dgram_hash"][:m],
                       pending_buf=t["pending_buf"], host_buf=t["host_buf"], rec_state=t["rec_state"][:m],
                       total=t["total"], m=m)


# sccsum_arp_rec, sccsum_eth_unresolved
ARP_REC_DTYPE = np.dtype([("ip", "<u4"), ("index", "<u4"), ("mac", "<u8")])
ARP_REC_BYTES = ARP_REC_DTYPE.itemsize  # 16
UNRESOLVED_DTYPE = np.dtype([("dgram", "<u4"), ("next_hop", "<u4")])
LEARN_NEED = native.ST_OK                               # what ip.cc:121-144 lets through, fragments included
LEARN_REJECT = native.ST_MALFORMED | native.ST_RANGE


def mac_int(mac) -> int:
    """A MAC as the interface takes it: the six wire bytes as a big-endian
    number.  Accepts that number, six bytes, or 'aa:bb:cc:dd:ee:ff'."""
    if isinstance(mac, str):
        parts = mac.split(":")
        if len(parts) != 6:
            raise ValueError(f"mac: need six ':'-separated bytes, got {mac!r}")
        mac = bytes(int(p, 16) for p in parts)
    if isinstance(mac, (bytes, bytearray)):
        if len(mac) != 6:
            raise ValueError("mac: need six bytes")
        mac = int.from_bytes(bytes(mac), "big")
    mac = int(mac)
    if not 0 <= mac <= native.MAC_MAX:
        raise ValueError("mac: bits 48-63 must be 0")
    return mac


class ArpTable(_DeviceObject):
    """sccsum_arp_table_*: an immutable copy of the stack's ARP table for the
    device calls below (include/sccsum.h, "Link layer").  `mapping` is a dict
    {ip: mac} or a sequence of (ip, mac) pairs, where a later pair for the same
    ip wins; ips in host order, macs as mac_int takes them.  device=None makes
    a host-only table (lookup alone).  A changed table is a new object."""
    _destroy, _a = "sccsum_arp_table_destroy", "an ArpTable"

    def __init__(self, mapping=(), device: int | None = 0):
        super().__init__()
        pairs = list(mapping.items()) if hasattr(mapping, "items") else list(mapping)
        if len(pairs) > native.ARP_MAX_ENTRIES:
            raise ValueError("mapping: at most 2^20 entries")
        arr = (native.ArpEntry * max(len(pairs), 1))()
        for k, (ip, mac) in enumerate(pairs):
            if not 0 <= int(ip) <= 0xFFFFFFFF:
                raise ValueError("mapping: an ip is a host-order IPv4 address, 0..2^32-1")
            arr[k].ip, arr[k].mac = int(ip), mac_int(mac)
        h = ctypes.c_void_p()
        entries = ctypes.addressof(arr) if pairs else None
        if device is None:
            code = self._lib.sccsum_arp_table_create_host(entries, len(pairs), ctypes.byref(h))
        else:
            code = self._lib.sccsum_arp_table_create(int(device), entries, len(pairs), ctypes.byref(h))
        native.check(code, "sccsum_arp_table_create")
        self._own(h, device)

    @property
    def bits(self) -> int:
        return int(self._lib.sccsum_arp_table_bits(self.handle))

    def lookup(self, ip: int):
        """The MAC the table maps ip to, or None (host arithmetic)."""
        mac = ctypes.c_uint64()
        hit = self._lib.sccsum_arp_table_lookup(self.handle, int(ip) & 0xFFFFFFFF, ctypes.byref(mac))
        return int(mac.value) if hit else None


class _Grouped:
    """A result whose entries are grouped by bucket: `first` holds the bucket
    bases, and the class names its buckets (_noun) and the tuple with one entry
    per bucket that is not the dropped one (_keys)."""
    _noun = ""
    _keys = ""

    def bounds(self) -> np.ndarray:
        """first on the host (synchronises once)."""
        if self._bounds is None:
            self._bounds = self.first.cpu().numpy().view(np.uint32).astype(np.int64)
        return self._bounds

    def _range(self, k: int) -> tuple:
        last = len(getattr(self, self._keys))
        if not 0 <= int(k) <= last:
            raise ValueError(f"{self._noun}: need 0..{last}")
        b = self.bounds()
        return int(b[k]), int(b[k + 1])


@dataclass
class EthRxResult(_Grouped):
    """What sccsum_eth_rx wrote (include/sccsum.h, "Link layer"): the batch's
    frames grouped by registered protocol, bucket len(protos) the dropped ones."""
    frames: PacketBatch       # the wire frames
    protos: tuple
    order: torch.Tensor       # int32 [n]: frame indices grouped by bucket, arrival order inside one
    first: torch.Tensor       # int32 [K + 2]: bucket bases, the last entry n
    l3_off: torch.Tensor      # int64 [n], grouped order: off + 14 (dropped: off)
    l3_len: torch.Tensor      # int32 [n], grouped order: len - 14 (dropped: 0)
    src_mac_all: torch.Tensor  # int64 [n], grouped order (dropped: 0)
    cls: torch.Tensor | None  # uint8 [n], arrival order: k, or native.ETH_UNKNOWN / ETH_SHORT / ETH_RANGE
    _bounds: np.ndarray | None = None
    _noun, _keys = "bucket", "protos"

    def bucket(self, k: int) -> PacketBatch:
        """Bucket k's frames behind their Ethernet header, a frames batch for
        ipv4_frames* as it stands (no copy)."""
        a, e = self._range(k)
        return PacketBatch(data=self.frames.data, off=self.l3_off[a:e], length=self.l3_len[a:e],
                           bytes_len=self.frames.bytes_len,
                           max_len=max(self.frames.max_len - native.ETH_HDR, 0) if self.frames.max_len else 0)

    def src_mac(self, k: int) -> torch.Tensor:
        a, e = self._range(k)
        return self.src_mac_all[a:e]

    def indices(self, k: int) -> torch.Tensor:
        """Bucket k's frame indices into the batch, in arrival order."""
        a, e = self._range(k)
        return self.order[a:e]


def eth_rx_check(b: PacketBatch, protos, cls=None) -> tuple:
    """What eth_rx refuses before any launch; returns (n, protos as a tuple)."""
    if not isinstance(b, PacketBatch):
        raise ValueError("b: need a PacketBatch of wire frames")
    protos = tuple(int(p) for p in protos)
    if not 1 <= len(protos) <= native.ETH_MAX_PROTOS:
        raise ValueError("protos: need 1..8 registered eth_proto values")
    if len(set(protos)) != len(protos) or any(not 0 <= p <= 0xFFFF for p in protos):
        raise ValueError("protos: need distinct 16-bit values")
    if b.n > 0xFFFFFFFF:
        raise ValueError("b: at most 2^32-1 frames")
    if cls is not None and (not isinstance(cls, torch.Tensor) or cls.dim() != 1):
        raise ValueError("cls: need a 1-D uint8 tensor of one entry per frame")
    _need(cls, b.n, torch.uint8, "cls", b.device)
    return b.n, protos


def eth_rx(b: PacketBatch, protos=(0x0800, 0x0806), want_class: bool = True, cls: torch.Tensor | None = None,
           stream=None) -> EthRxResult:
    """sccsum_eth_rx: interface::dispatch_packet (net.cc:324-357) for a batch of
    wire frames — the class of every frame by its eth_proto, a stable partition
    by class and the 14-byte trim; no byte moves.

        r = eth_rx(wire, (0x0800, 0x0806))
        ip = r.bucket(0)                              # a frames batch behind the Ethernet headers
        status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
        ipv4_frames(ip, status=status)
        recs = arp_learn_records(ip, status, r.src_mac(0), host, netmask, table)
        arp_frames = r.indices(1).cpu()               # the short list the host's ARP code takes
    """
    lib = native.load()
    n, protos = eth_rx_check(b, protos, cls)
    dev = b.device
    k = len(protos)
    if cls is None and want_class:
        cls = _scratch(max(n, 1), dev, stream, torch.uint8)
    order = _scratch(max(n, 1), dev, stream, torch.int32)
    first = _scratch(k + 2, dev, stream, torch.int32)
    l3_off = _scratch(max(n, 1), dev, stream, torch.int64)
    l3_len = _scratch(max(n, 1), dev, stream, torch.int32)
    src_mac = _scratch(max(n, 1), dev, stream, torch.int64)
    ws = _scratch(int(lib.sccsum_eth_rx_workspace(n)), dev, stream)
    arr = (ctypes.c_uint16 * k)(*protos)
    empty = n == 0  # an empty tensor has no address
    code = lib.sccsum_eth_rx(ctypes_ptr(b.data), b.bytes_len, None if empty else ctypes_ptr(b.off),
                             None if empty else ctypes_ptr(b.length), n, ctypes.addressof(arr), k, _ptr(cls),
                             ctypes_ptr(first), ctypes_ptr(order), ctypes_ptr(l3_off), ctypes_ptr(l3_len),
                             ctypes_ptr(src_mac), ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_eth_rx")
    return EthRxResult(frames=b, protos=protos, order=order[:n], first=first, l3_off=l3_off[:n], l3_len=l3_len[:n],
                       src_mac_all=src_mac[:n], cls=None if cls is None else cls[:n])


def arp_learn_check(b: PacketBatch, status, src_mac, host, netmask, table, need, reject) -> int:
    """What arp_learn_records refuses before any launch; returns n."""
    if not isinstance(b, PacketBatch):
        raise ValueError("b: need a PacketBatch of IPv4 frames (an eth_rx bucket)")
    n = b.n
    if n > 0x7FFFFFFF:
        raise ValueError("b: at most 2^31-1 frames")
    for t, dtype, what in ((status, torch.uint8, "status"), (src_mac, torch.int64, "src_mac")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError(f"{what}: need a 1-D {dtype} tensor of one entry per frame")
        _need(t, n, dtype, what, b.device)
    _status_masks(need, reject)
    for v, what in ((host, "host"), (netmask, "netmask")):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{what}: need 0..2^32-1")
    _device_handle(table, ArpTable, b.device, "table", optional=True)
    return n


def arp_learn_records(b: PacketBatch, status: torch.Tensor, src_mac: torch.Tensor, host: int, netmask: int,
                      table: ArpTable | None = None, need: int = LEARN_NEED, reject: int = LEARN_REJECT,
                      stream=None) -> torch.Tensor:
    """sccsum_arp_learn_records: the frames of an IPv4 bucket whose (source
    ip, source MAC) the stack's _arp.learn (ip.cc:147-149) has to be told, as
    sccsum_arp_rec records (ARP_REC_DTYPE) in arrival order: a uint8 tensor of
    16 bytes per record; empty in the steady state.  Repeats of one new pair
    inside the batch are not removed.  Synchronises to size it."""
    lib = native.load()
    n = arp_learn_check(b, status, src_mac, host, netmask, table, need, reject)
    dev = b.device
    rec = _scratch(ARP_REC_BYTES * max(n, 1), dev, stream)
    count = _scratch(1, dev, stream, torch.int32)
    ws = _scratch(int(lib.sccsum_arp_learn_workspace(n)), dev, stream)
    empty = n == 0  # an empty tensor has no address
    code = lib.sccsum_arp_learn_records(
        ctypes_ptr(b.data), b.bytes_len, None if empty else ctypes_ptr(b.off), None if empty else ctypes_ptr(b.length),
        None if empty else ctypes_ptr(status), int(need), int(reject), None if empty else ctypes_ptr(src_mac), n,
        int(host), int(netmask), None if table is None else table.handle, ctypes_ptr(rec), ctypes_ptr(count),
        ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_arp_learn_records")
    if stream is not None:
        stream.synchronize()
    return rec[: ARP_REC_BYTES * (int(count.item()) & 0xFFFFFFFF)]


@dataclass
class EthSendResult:
    """What sccsum_eth_send wrote (include/sccsum.h, "Link layer").  The
    per-frame tensors have room for every input frame; totals() and emitted()
    say how many are written."""
    eth: torch.Tensor          # uint8 [14 F]: the Ethernet headers
    desc: torch.Tensor         # uint8 [16 (D + F)]: sccsum_gather_desc records
    first: torch.Tensor        # int32 [F + 1]: CSR index into desc, and the closing entry
    out_off: torch.Tensor      # int64 [F]: the frame's position in the packed layout
    out_len: torch.Tensor      # int32 [F]: the input frame's length + 14
    frame_src: torch.Tensor    # int32 [F]: the input frame an emitted frame was made of
    status: torch.Tensor       # uint8 [n]: native.ST_OK, native.ST_NOARP or 0
    unresolved_buf: torch.Tensor  # uint8 [8 n]: sccsum_eth_unresolved records
    total: torch.Tensor        # int64 [6]
    keep: tuple                # the input lists the payload descriptors came from

    def _total(self) -> np.ndarray:
        return self.total.cpu().numpy()

    def totals(self) -> tuple:
        """(frames needed, layout bytes needed, datagrams taken, unresolved among them); synchronises."""
        t = self._total()
        return int(t[0]), int(t[1]), int(t[2]), int(t[3])

    def emitted(self) -> tuple:
        """(frames, descriptors) written; synchronises."""
        t = self._total()
        return int(t[4]), int(t[5])

    def lists(self) -> tuple:
        """(desc, first, out_off, out_len, max_len) of the emitted frames, as
        the *_desc calls and the mapped burst form take them; synchronises."""
        e, d = self.emitted()
        ln = self.out_len[:e]
        return self.desc[: 16 * d], self.first[: e + 1], self.out_off[:e], ln, (int(ln.max().item()) if e else 0)

    def unresolved(self) -> np.ndarray:
        """The datagrams without an ARP entry as a host array of
        UNRESOLVED_DTYPE {dgram, next_hop}, in order: the ARP queries to send;
        synchronises."""
        u = self.totals()[3]
        return self.unresolved_buf[: 8 * u].cpu().numpy().view(UNRESOLVED_DTYPE).copy()

    def pack(self, stream=None) -> PacketBatch:
        """The packed wire frames: sccsum_gather of every header and piece
        into a new buffer (the one pass that moves payload bytes);
        synchronises to size it."""
        desc, _, off, ln, max_len = self.lists()
        e = int(off.numel())
        nbytes = int((off[-1] + ln[-1]).item()) if e else 0
        data = _scratch(_round16(nbytes) or 16, self.eth.device, stream)
        if e:
            native.check(native.load().sccsum_gather(ctypes_ptr(desc), int(desc.numel()) // 16, ctypes_ptr(data),
                                                     _stream(stream)), "sccsum_gather")
        return PacketBatch(data=data, off=off, length=ln, bytes_len=nbytes, max_len=max_len)


def eth_send_check(lists, dst, dgram_first, table, hw_address, host, netmask, gw, eth_proto, max_out_bytes) -> tuple:
    """What eth_send refuses before any launch (the kernels trust the sizes);
    returns (n, F, D): datagrams, frames, descriptors."""
    if not isinstance(lists, (tuple, list)) or len(lists) < 4:
        raise ValueError("lists: need (desc, first, off, length[, max_len]) as SendResult.lists() returns them")
    desc, first, off, length = lists[:4]
    for t, what in ((desc, "desc"), (first, "first"), (off, "off"), (length, "length"), (dst, "dst")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError(f"{what}: need a 1-D tensor")
    dev = off.device
    nframes = int(off.numel())
    if nframes > 0x7FFFFFFF:
        raise ValueError("lists: at most 2^31-1 frames")
    _need(off, nframes, torch.int64, "off", dev)
    _need(length, nframes, torch.int32, "length", dev)
    _need(first, nframes + 1, torch.int32, "first", dev)
    _need(desc, 0, torch.uint8, "desc", dev)
    if int(first.numel()) != nframes + 1 or int(length.numel()) != nframes or int(desc.numel()) % 16:
        raise ValueError("lists: first must have one entry more than off / length, desc 16-byte records")
    n = int(dst.numel())
    if n > 0xFFFFFFFF:
        raise ValueError("dst: at most 2^32-1 datagrams")
    _need(dst, n, torch.int32, "dst", dev)
    if dgram_first is None:
        if n != nframes:
            raise ValueError("dst: without dgram_first there is one frame per datagram")
    else:
        if not isinstance(dgram_first, torch.Tensor) or dgram_first.dim() != 1 or int(dgram_first.numel()) != n + 1:
            raise ValueError("dgram_first: need a 1-D int32 tensor of n + 1 entries")
        _need(dgram_first, n + 1, torch.int32, "dgram_first", dev)
    _device_handle(table, ArpTable, dev, "table")
    mac_int(hw_address)
    for v, what in ((host, "host"), (netmask, "netmask"), (gw, "gw")):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{what}: need a host-order IPv4 value, 0..2^32-1")
    if not 0 <= int(eth_proto) <= 0xFFFF:
        raise ValueError("eth_proto: need a 16-bit value")
    if max_out_bytes is not None and not 0 <= int(max_out_bytes) <= 0xFFFFFFFF:
        raise ValueError("max_out_bytes: need 0..2^32-1 (descriptor offsets are 32-bit)")
    return n, nframes, int(desc.numel()) // 16


def eth_send(send, dst: torch.Tensor, table: ArpTable, hw_address, host: int, netmask: int, gw: int,
             eth_proto: int = 0x0800, dgram_first: torch.Tensor | None = None, max_out_bytes: int | None = None,
             stream=None) -> EthSendResult:
    """sccsum_eth_send: ipv4::get_l2_dst_address (ip.cc:231-242) and the
    interface's Ethernet header (net.cc:266-284) for frames given as fragment
    lists — a SendResult (after its checksum fills) or a (desc, first, off,
    length) tuple with dgram_first (None: one frame per datagram).  dst: int32
    [n], the datagrams' destinations (host-order addresses as uint32 values).

        r = ipv4_send(l4, dst, proto, 1500, me)
        ipv4_fill_desc(*r.lists()[:4], r.lists()[4], mode=native.FILL_IP)
        e = eth_send(r, dst, table, hw, me, netmask, gw)
        wire = e.pack()                 # or hand e.lists() to the mapped burst form
        for q in e.unresolved(): ...    # arp queries for q["next_hop"], then resubmit datagram q["dgram"]
    """
    lib = native.load()
    if isinstance(send, SendResult):
        lists = send.lists()
        dgram_first = send.dgram_first
    else:
        lists = send
    n, nframes, ndesc = eth_send_check(lists, dst, dgram_first, table, hw_address, host, netmask, gw, eth_proto,
                                       max_out_bytes)
    desc, first, off, length = lists[:4]
    dev = off.device
    if max_out_bytes is None:
        need = (int(length.to(torch.int64).sum().item()) if nframes else 0) + native.ETH_HDR * nframes
        max_out_bytes = min(0xFFFFFFFF, need)
    f1 = max(nframes, 1)
    eth = _scratch(native.ETH_HDR * f1, dev, stream)
    desc_out = _scratch(16 * max(ndesc + nframes, 1), dev, stream)
    first_out = _scratch(nframes + 1, dev, stream, torch.int32)
    out_off = _scratch(f1, dev, stream, torch.int64)
    out_len = _scratch(f1, dev, stream, torch.int32)
    frame_src = _scratch(f1, dev, stream, torch.int32)
    status = _scratch(max(n, 1), dev, stream, torch.uint8)
    unresolved = _scratch(8 * max(n, 1), dev, stream)
    total = _scratch(6, dev, stream, torch.int64)
    ws = _scratch(int(lib.sccsum_eth_send_workspace(n)), dev, stream)
    opts = native.EthOpts(mac_int(hw_address), int(host), int(netmask), int(gw), int(eth_proto))
    no_dg, no_fr = n == 0, nframes == 0  # an empty tensor has no address
    code = lib.sccsum_eth_send(
        ctypes.addressof(opts), table.handle, None if no_dg else ctypes_ptr(dst), _ptr(dgram_first), n,
        None if no_fr or not ndesc else ctypes_ptr(desc), None if no_fr else ctypes_ptr(first),
        None if no_fr else ctypes_ptr(off), None if no_fr else ctypes_ptr(length), nframes, int(max_out_bytes),
        ctypes_ptr(eth), ctypes_ptr(desc_out), ctypes_ptr(first_out), ctypes_ptr(out_off), ctypes_ptr(out_len),
        ctypes_ptr(frame_src), ctypes_ptr(status), ctypes_ptr(unresolved), ctypes_ptr(total), ctypes_ptr(ws),
        _stream(stream))
    native.check(code, "sccsum_eth_send")
    return EthSendResult(eth=eth, desc=desc_out, first=first_out, out_off=out_off[:nframes], out_len=out_len[:nframes],
                         frame_src=frame_src[:nframes], status=status[:n], unresolved_buf=unresolved, total=total,
                         keep=(send, dst))


UDP_NEED = native.ST_OK                  # what ip.cc:121-144 lets through; the reference verifies no UDP checksum on rx
UDP_REJECT = native.ST_MALFORMED | native.ST_RANGE | native.ST_IPFRAG


class UdpPorts(_DeviceObject):
    """sccsum_udp_ports_*: the immutable port -> channel table of the UDP layer
    (include/sccsum.h, "UDP layer").  `ports` are distinct host-order ports,
    at most 252; channel k is ports[k].  device=None makes a host-only table
    (lookup alone).  A changed set of channels is a new object."""
    _destroy, _a = "sccsum_udp_ports_destroy", "a UdpPorts"

    def __init__(self, ports=(), device: int | None = 0):
        super().__init__()
        ports = tuple(int(p) for p in ports)
        if len(ports) > native.UDP_MAX_CHANNELS:
            raise ValueError("ports: at most 252 channels")
        if any(not 0 <= p <= 0xFFFF for p in ports) or len(set(ports)) != len(ports):
            raise ValueError("ports: need distinct 16-bit values")
        arr = (ctypes.c_uint16 * max(len(ports), 1))(*ports)
        h = ctypes.c_void_p()
        where = ctypes.addressof(arr) if ports else None
        if device is None:
            code = self._lib.sccsum_udp_ports_create_host(where, len(ports), ctypes.byref(h))
        else:
            code = self._lib.sccsum_udp_ports_create(int(device), where, len(ports), ctypes.byref(h))
        native.check(code, "sccsum_udp_ports_create")
        self._own(h, device)
        self.ports = ports

    @property
    def channels(self) -> int:
        return int(self._lib.sccsum_udp_ports_channels(self.handle))

    def lookup(self, port: int):
        """The channel bound to port, or None (host arithmetic)."""
        k = int(self._lib.sccsum_udp_ports_lookup(self.handle, int(port) & 0xFFFF))
        return None if k < 0 else k


@dataclass
class UdpRxResult(_Grouped):
    """What sccsum_udp_rx / sccsum_udp_rx_reasm wrote (include/sccsum.h, "UDP
    layer"): the call's frames (datagrams) grouped by channel, bucket
    len(ports) everything dropped."""
    source: object            # the frames batch, or the ReasmResult whose datagrams these are
    ports: tuple
    order: torch.Tensor       # int32 [n]: batch frame (datagram) indices grouped by bucket, arrival order inside one
    first: torch.Tensor       # int32 [C + 2]: bucket bases, the last entry n
    pay_off: torch.Tensor | None  # int64 [n], grouped order: off + 4 ihl + 8 (dropped: off); None for datagrams
    pay_len: torch.Tensor     # int32 [n], grouped order (dropped: 0)
    src_all: torch.Tensor     # int32 [n], grouped order: the source address
    sport_all: torch.Tensor   # int16 [n], grouped order: the source port
    cls: torch.Tensor | None  # uint8 [n], arrival order: k, or native.UDP_SKIP / UDP_SHORT / UDP_NOPORT
    _bounds: np.ndarray | None = None
    _noun, _keys = "channel", "ports"

    def count(self, k: int) -> int:
        a, e = self._range(k)
        return e - a

    def taken(self, k: int, room: int = native.UDP_QUEUE_SIZE) -> int:
        """How many of channel k's datagrams _queue.push accepts with `room`
        free slots: the partition is stable, so they are the first taken(k,
        room) of the bucket (queue.hh:184-192)."""
        if int(room) < 0:
            raise ValueError("room: need >= 0")
        return min(self.count(k), int(room))

    def channel(self, k: int) -> PacketBatch:
        """Channel k's payloads where they lie, a spans batch as it stands (no
        copy).  Reassembled datagrams have no such batch: their payload is the
        fragment list's bytes from +8 (indices(k), payload_len(k))."""
        if self.pay_off is None:
            raise ValueError("channel: reassembled datagrams are fragment lists; use indices(k) and payload_len(k)")
        a, e = self._range(k)
        ml = self.source.max_len
        return PacketBatch(data=self.source.data, off=self.pay_off[a:e], length=self.pay_len[a:e],
                           bytes_len=self.source.bytes_len, max_len=max(ml - 28, 0) if ml else 0)

    def indices(self, k: int) -> torch.Tensor:
        a, e = self._range(k)
        return self.order[a:e]

    def payload_len(self, k: int) -> torch.Tensor:
        a, e = self._range(k)
        return self.pay_len[a:e]

    def src(self, k: int) -> torch.Tensor:
        a, e = self._range(k)
        return self.src_all[a:e]

    def sport(self, k: int) -> torch.Tensor:
        a, e = self._range(k)
        return self.sport_all[a:e]


def _rx_filter(host, need, reject) -> None:
    """What the UDP and TCP rx calls take of a frame: the status masks and the host address."""
    _status_masks(need, reject)
    if not 0 <= int(host) <= 0xFFFFFFFF:
        raise ValueError("host: need a host-order IPv4 address, 0..2^32-1")


def udp_rx_check(b: PacketBatch, status, ports, host, need, reject, index=None, cls=None) -> tuple:
    """What udp_rx refuses before any launch; returns (n, nbatch)."""
    if not isinstance(b, PacketBatch):
        raise ValueError("b: need a PacketBatch of IPv4 frames (an eth_rx bucket)")
    nbatch = b.n
    if nbatch > 0xFFFFFFFF:
        raise ValueError("b: at most 2^32-1 frames")
    if not isinstance(status, torch.Tensor) or status.dim() != 1:
        raise ValueError("status: need the 1-D uint8 tensor the frames call wrote, one entry per frame")
    _need(status, nbatch, torch.uint8, "status", b.device)
    _rx_filter(host, need, reject)
    n = nbatch
    if index is not None:
        if not isinstance(index, torch.Tensor) or index.dim() != 1:
            raise ValueError("index: need a 1-D int32 tensor of batch frame indices")
        n = int(index.numel())
        if n > 0xFFFFFFFF:
            raise ValueError("index: at most 2^32-1 entries")
        _need(index, n, torch.int32, "index", b.device)
    if cls is not None and (not isinstance(cls, torch.Tensor) or cls.dim() != 1):
        raise ValueError("cls: need a 1-D uint8 tensor of one entry per frame")
    _need(cls, n, torch.uint8, "cls", b.device)
    _device_handle(ports, UdpPorts, b.device, "ports")
    return n, nbatch


def _udp_rx_outputs(n, channels, dev, stream, want_class, cls, with_off):
    if cls is None and want_class:
        cls = _scratch(max(n, 1), dev, stream, torch.uint8)
    k = max(n, 1)
    return dict(cls=cls, order=_scratch(k, dev, stream, torch.int32), first=_scratch(channels + 2, dev, stream, torch.int32),
                pay_off=_scratch(k, dev, stream, torch.int64) if with_off else None,
                pay_len=_scratch(k, dev, stream, torch.int32), src=_scratch(k, dev, stream, torch.int32),
                sport=_scratch(k, dev, stream, torch.int16))


def udp_rx(b: PacketBatch, status: torch.Tensor, ports: UdpPorts, host: int, need: int = UDP_NEED,
           reject: int = UDP_REJECT, index: torch.Tensor | None = None, want_class: bool = True,
           cls: torch.Tensor | None = None, stream=None) -> UdpRxResult:
    """sccsum_udp_rx: the end of ipv4::handle_received_packet (ip.cc:159-162,
    222-227) and ipv4_udp::received (udp.cc:45-53, 164-173) for the
    non-fragment frames of an IPv4 bucket — for us? UDP? the trim to the IP
    length, both headers dropped, the channel by destination port; a stable
    partition by channel, no byte moves.

        ip = eth_rx(wire).bucket(0)
        status = torch.empty(ip.n, dtype=torch.uint8, device=dev)
        ipv4_frames(ip, status=status)
        r = udp_rx(ip, status, ports, me)             # index=: a shard's slice of Steer.run's order
        spans(r.channel(k))                            # channel k's payloads, r.src(k), r.sport(k)
        r.taken(k, room)                               # how many of them the channel's queue accepts

    The reference verifies no UDP checksum on rx; need=ST_OK | ST_L4_OK does."""
    lib = native.load()
    n, nbatch = udp_rx_check(b, status, ports, host, need, reject, index, cls)
    dev = b.device
    t = _udp_rx_outputs(n, len(ports.ports), dev, stream, want_class, cls, True)
    ws = _scratch(int(lib.sccsum_udp_rx_workspace(n)), dev, stream)
    empty = nbatch == 0  # an empty tensor has no address
    code = lib.sccsum_udp_rx(
        ctypes_ptr(b.data), b.bytes_len, None if empty else ctypes_ptr(b.off), None if empty else ctypes_ptr(b.length),
        nbatch, None if empty else ctypes_ptr(status), int(need), int(reject), int(host), ports.handle,
        None if index is None or n == 0 else ctypes_ptr(index), n, _ptr(t["cls"]), ctypes_ptr(t["first"]),
        ctypes_ptr(t["order"]), ctypes_ptr(t["pay_off"]), ctypes_ptr(t["pay_len"]), ctypes_ptr(t["src"]),
        ctypes_ptr(t["sport"]), ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_udp_rx")
    return UdpRxResult(source=b, ports=ports.ports, order=t["order"][:n], first=t["first"], pay_off=t["pay_off"][:n],
                       pay_len=t["pay_len"][:n], src_all=t["src"][:n], sport_all=t["sport"][:n],
                       cls=None if t["cls"] is None else t["cls"][:n])


def udp_rx_reasm_check(r, records, ports, host, l4_status, need, reject, cls=None) -> tuple:
    """What udp_rx_reassembled refuses before any launch; returns (m, nrec):
    the delivered datagrams (synchronises to count them) and the records."""
    if not isinstance(r, ReasmResult):
        raise ValueError("r: need the ReasmResult of reassemble()")
    nrec = reasm_check(records, None, 0)
    dev = records.device
    m = r.totals()[0]
    _rx_filter(host, need, reject)
    if l4_status is None:
        if int(need) or int(reject):
            raise ValueError("need / reject: masks need l4_status")
    else:
        if not isinstance(l4_status, torch.Tensor) or l4_status.dim() != 1:
            raise ValueError("l4_status: need the 1-D uint8 tensor spans_desc wrote, one entry per datagram")
        _need(l4_status, m, torch.uint8, "l4_status", dev)
    if cls is not None and (not isinstance(cls, torch.Tensor) or cls.dim() != 1):
        raise ValueError("cls: need a 1-D uint8 tensor of one entry per datagram")
    _need(cls, m, torch.uint8, "cls", dev)
    _device_handle(ports, UdpPorts, dev, "ports")
    return m, nrec


def udp_rx_reassembled(r: ReasmResult, records: torch.Tensor, ports: UdpPorts, host: int,
                       l4_status: torch.Tensor | None = None, need: int = 0, reject: int = 0, want_class: bool = True,
                       cls: torch.Tensor | None = None, stream=None) -> UdpRxResult:
    """sccsum_udp_rx_reasm: udp_rx's demux for the datagrams reassemble()
    delivered; `records` is the tensor reassemble() took.  The UDP header is
    read through the fragment list; the payload is the list's bytes from +8.

        r = reassemble(recs)
        desc, first, off, length, seeds, max_len = r.lists()
        st = torch.empty(off.numel(), dtype=torch.uint8, device=dev)
        spans_desc(desc, first, off, length, max_len, seeds=seeds, status=st)
        u = udp_rx_reassembled(r, recs, ports, me)     # l4_status=st, need=ST_OK: verified datagrams only
        u.indices(k), u.payload_len(k), u.src(k), u.sport(k)
    """
    lib = native.load()
    m, nrec = udp_rx_reasm_check(r, records, ports, host, l4_status, need, reject, cls)
    dev = records.device
    t = _udp_rx_outputs(m, len(ports.ports), dev, stream, want_class, cls, False)
    ws = _scratch(int(lib.sccsum_udp_rx_reasm_workspace(m)), dev, stream)
    empty = m == 0  # an empty tensor has no address
    code = lib.sccsum_udp_rx_reasm(
        None if empty else ctypes_ptr(r.desc), None if empty else ctypes_ptr(r.dgram_first),
        None if empty else ctypes_ptr(r.dgram_off), None if empty else ctypes_ptr(r.dgram_len),
        None if empty else ctypes_ptr(r.dgram_head), m, ctypes_ptr(records) if nrec else None, nrec,
        None if empty else _ptr(l4_status), int(need), int(reject), int(host), ports.handle, _ptr(t["cls"]),
        ctypes_ptr(t["first"]), ctypes_ptr(t["order"]), ctypes_ptr(t["pay_len"]), ctypes_ptr(t["src"]),
        ctypes_ptr(t["sport"]), ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_udp_rx_reasm")
    return UdpRxResult(source=r, ports=ports.ports, order=t["order"][:m], first=t["first"], pay_off=None,
                       pay_len=t["pay_len"][:m], src_all=t["src"][:m], sport_all=t["sport"][:m],
                       cls=None if t["cls"] is None else t["cls"][:m])


@dataclass
class UdpSendResult:
    """What sccsum_udp_send wrote (include/sccsum.h, "UDP layer"): the headers
    lie in the payloads' headroom, in payloads.data itself."""
    l4: PacketBatch            # header + payload per datagram: what ipv4_send takes
    sum_batch: PacketBatch     # the spans whose results (with seeds) are ipv4_send's l4sum
    seeds: torch.Tensor        # int32 [n]
    proto: torch.Tensor        # uint8 [n]: 17
    needs_csum: torch.Tensor   # uint8 [n]: offload_info::needs_csum
    status: torch.Tensor       # uint8 [n]: native.ST_OK, or ST_RANGE / ST_MALFORMED (no header written)


def udp_send_check(payloads: PacketBatch, dst, dport, sport, src_host, mtu, flags) -> int:
    """What udp_send refuses before any launch; returns n."""
    if not isinstance(payloads, PacketBatch):
        raise ValueError("payloads: need a PacketBatch of UDP payloads, each with 8 bytes of headroom")
    dev, n = payloads.device, payloads.n
    if n > 0xFFFFFFFF:
        raise ValueError("payloads: at most 2^32-1 datagrams")
    if not 68 <= int(mtu) <= 65535:
        raise ValueError(f"mtu: need 68..65535, got {mtu}")
    if int(flags) & ~(native.UDP_CSUM_OFFLOAD | native.UDP_UFO):
        raise ValueError(f"flags: unknown bits in {int(flags):#x}")
    if not 0 <= int(src_host) <= 0xFFFFFFFF:
        raise ValueError("src_host: need a host-order IPv4 address, 0..2^32-1")
    for t, dtype, what in ((dst, torch.int32, "dst"), (dport, torch.int16, "dport"), (sport, torch.int16, "sport")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError(f"{what}: need a 1-D {dtype} tensor of one entry per datagram")
        _need(t, n, dtype, what, dev)
    return n


def udp_send(payloads: PacketBatch, dst: torch.Tensor, dport: torch.Tensor, sport: torch.Tensor, src_host: int,
             mtu: int, flags: int = 0, stream=None) -> UdpSendResult:
    """sccsum_udp_send: ipv4_udp::send's header (udp.cc:175-197) into the 8
    bytes in front of every payload — the caller's headroom, which must not
    overlap another payload — and the checksum pass's spans and seeds.

        u = udp_send(payloads, dst, dport, sport, me, 1500)
        l4sum = spans(u.sum_batch, seeds=u.seeds)
        r = ipv4_send(u.l4, dst, u.proto, 1500, me, ids=ids, l4sum=l4sum, flags=native.SEND_L4)
        ipv4_fill_desc(*r.lists()[:4], r.lists()[4], mode=native.FILL_IP)    # unless SEND computed it
        wire = eth_send(r, dst, table, hw, me, netmask, gw).pack()

    dst: int32 [n], dport / sport: int16 [n] (uint32 / uint16 values).  With
    native.UDP_CSUM_OFFLOAD a datagram that needs no cut gets the folded
    pseudo-header sum in its field and needs_csum = 1."""
    lib = native.load()
    n = udp_send_check(payloads, dst, dport, sport, src_host, mtu, flags)
    dev = payloads.device
    k = max(n, 1)
    l4_off = _scratch(k, dev, stream, torch.int64)
    l4_len = _scratch(k, dev, stream, torch.int32)
    sum_len = _scratch(k, dev, stream, torch.int32)
    seeds = _scratch(k, dev, stream, torch.int32)
    proto = _scratch(k, dev, stream, torch.uint8)
    needs_csum = _scratch(k, dev, stream, torch.uint8)
    status = _scratch(k, dev, stream, torch.uint8)
    opts = native.UdpOpts(int(src_host), int(mtu), int(flags))
    empty = n == 0  # an empty tensor has no address
    code = lib.sccsum_udp_send(
        ctypes.addressof(opts), ctypes_ptr(payloads.data), payloads.bytes_len,
        None if empty else ctypes_ptr(payloads.off), None if empty else ctypes_ptr(payloads.length),
        None if empty else ctypes_ptr(dst), None if empty else ctypes_ptr(dport), None if empty else ctypes_ptr(sport),
        n, ctypes_ptr(l4_off), ctypes_ptr(l4_len), ctypes_ptr(sum_len), ctypes_ptr(seeds), ctypes_ptr(proto),
        ctypes_ptr(needs_csum), ctypes_ptr(status), _stream(stream))
    native.check(code, "sccsum_udp_send")
    ml = payloads.max_len + native.UDP_HDR if payloads.max_len else 0
    l4 = PacketBatch(data=payloads.data, off=l4_off[:n], length=l4_len[:n], bytes_len=payloads.bytes_len, max_len=ml)
    sums = PacketBatch(data=payloads.data, off=l4_off[:n], length=sum_len[:n], bytes_len=payloads.bytes_len, max_len=ml)
    return UdpSendResult(l4=l4, sum_batch=sums, seeds=seeds[:n], proto=proto[:n], needs_csum=needs_csum[:n],
                         status=status[:n])


TCP_NEED = native.ST_OK | native.ST_L4_OK   # the reference verifies the TCP checksum on rx (tcp.hh:876-883)
TCP_REJECT = native.ST_MALFORMED | native.ST_RANGE | native.ST_IPFRAG
TCP_SEG_DTYPE = np.dtype([("pay_off", "<u8"), ("pay_len", "<u4"), ("seq", "<u4"), ("ack", "<u4"), ("conn", "<u4"),
                          ("window", "<u2"), ("sport", "<u2"), ("dport", "<u2"), ("flags", "u1"), ("hdr_len", "u1")])
TCP_OUT_DTYPE = np.dtype([("dst", "<u4"), ("seq", "<u4"), ("ack", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
                          ("window", "<u2"), ("flags", "u1"), ("hdr_len", "u1"), ("mss", "<u4")])


class TcpConns(_DeviceObject):
    """sccsum_tcp_conns_*: the immutable connection table of the TCP layer
    (include/sccsum.h, "TCP layer").  `conns` are distinct (local_ip,
    foreign_ip, local_port, foreign_port) in host order, at most 2^20;
    connection c is conns[c].  `listen` are the distinct listening ports.
    device=None makes a host-only table (lookup alone).  A changed set of
    connections is a new object."""
    _destroy, _a = "sccsum_tcp_conns_destroy", "a TcpConns"

    def __init__(self, conns=(), listen=(), device: int | None = 0):
        super().__init__()
        arr = np.asarray(conns, dtype=np.int64).reshape(-1, 4)
        listen = np.asarray(listen, dtype=np.int64).reshape(-1)
        if arr.shape[0] > native.TCP_MAX_CONNS:
            raise ValueError("conns: at most 2^20 connections")
        if arr.size and (arr.min() < 0 or arr[:, :2].max() > 0xFFFFFFFF or arr[:, 2:].max() > 0xFFFF):
            raise ValueError("conns: need (local_ip, foreign_ip, local_port, foreign_port), 32- and 16-bit values")
        if listen.size > 65536 or (listen.size and (listen.min() < 0 or listen.max() > 0xFFFF)):
            raise ValueError("listen: need at most 65536 16-bit ports")
        if np.unique(listen).size != listen.size:
            raise ValueError("listen: need distinct ports")
        packed = np.zeros(max(arr.shape[0], 1), dtype=np.dtype([("l", "<u4"), ("f", "<u4"), ("lp", "<u2"), ("fp", "<u2")]))
        if arr.shape[0]:
            packed["l"], packed["f"], packed["lp"], packed["fp"] = arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3]
        ports = np.ascontiguousarray(listen.astype(np.uint16)) if listen.size else np.zeros(1, np.uint16)
        h = ctypes.c_void_p()
        a = packed.ctypes.data if arr.shape[0] else None
        b = ports.ctypes.data if listen.size else None
        if device is None:
            code = self._lib.sccsum_tcp_conns_create_host(a, arr.shape[0], b, listen.size, ctypes.byref(h))
        else:
            code = self._lib.sccsum_tcp_conns_create(int(device), a, arr.shape[0], b, listen.size, ctypes.byref(h))
        # every other cause of SCCSUM_EINVAL (a count past its limit, a value out of range, a port given
        # twice) was refused above, so what is left is a connid given twice; a check dropped above
        # would make this message wrong
        if code == native.SCCSUM_EINVAL:
            raise ValueError("conns: a connection given twice")
        native.check(code, "sccsum_tcp_conns_create")
        self._own(h, device)
        self.nconns = int(arr.shape[0])

    @property
    def count(self) -> int:
        return int(self._lib.sccsum_tcp_conns_count(self.handle))

    @property
    def bits(self) -> int:
        return int(self._lib.sccsum_tcp_conns_bits(self.handle))

    def lookup(self, local_ip: int, foreign_ip: int, local_port: int, foreign_port: int):
        """The connection of a connid, or None (host arithmetic)."""
        c = int(self._lib.sccsum_tcp_conns_lookup(self.handle, int(local_ip) & 0xFFFFFFFF, int(foreign_ip) & 0xFFFFFFFF,
                                                  int(local_port) & 0xFFFF, int(foreign_port) & 0xFFFF))
        return None if c < 0 else c

    def listening(self, port: int) -> bool:
        return bool(self._lib.sccsum_tcp_conns_listening(self.handle, int(port) & 0xFFFF))


@dataclass
class TcpRxResult(_Grouped):   # bounds() alone: its four buckets have no names to range over
    """What sccsum_tcp_rx wrote (include/sccsum.h, "TCP layer"): the call's
    segments grouped by bucket (0 a known connection, 1 a listening port, 2
    answered with a RST, 3 dropped), bucket 0 by connection."""
    source: PacketBatch
    order: torch.Tensor       # int32 [n]: batch frame indices in grouped order
    first: torch.Tensor       # int32 [5]: bucket bases, the last entry n
    seg: torch.Tensor         # uint8 [n, 32]: sccsum_tcp_seg records, grouped order (TCP_SEG_DTYPE on the host)
    src_all: torch.Tensor     # int32 [n], grouped order: the source address
    run_conn: torch.Tensor    # int32 [>= R]: the connection of run r
    run_first: torch.Tensor   # int32 [>= R + 1]: where run r starts in bucket 0
    rst: torch.Tensor         # uint8 [>= 20 n]: the RST answers of bucket 2, 20 bytes each
    rst_dst: torch.Tensor     # int32 [n]: their destinations
    total: torch.Tensor       # int64 [4]: R, resets
    cls: torch.Tensor | None  # uint8 [n], arrival order: native.TCP_*
    _bounds: np.ndarray | None = None
    _totals: tuple | None = None

    def totals(self) -> tuple:
        """(R, resets) on the host (synchronises once)."""
        if self._totals is None:
            t = self.total.cpu().numpy()
            self._totals = (int(t[0]), int(t[1]))
        return self._totals

    def runs(self) -> tuple:
        """(run_conn [R], run_first [R + 1]): run r is connection run_conn[r],
        positions run_first[r] .. run_first[r + 1] of the grouped order."""
        r = self.totals()[0]
        return self.run_conn[:r], self.run_first[:r + 1]

    def segs(self, conn_run: int) -> torch.Tensor:
        """The records of run conn_run, a connection's segments in arrival order (a view)."""
        r = self.totals()[0]
        if not 0 <= int(conn_run) < r:
            raise ValueError(f"conn_run: need 0..{r - 1}")
        rf = self.run_first[int(conn_run):int(conn_run) + 2].cpu().numpy().view(np.uint32)
        return self.seg[int(rf[0]):int(rf[1])]

    @property
    def resets(self) -> tuple:
        """(l4, dst): the RST answers as an L4 batch of 20-byte segments and
        their destinations, what ipv4_send takes with proto 6 (no SEND_L4)."""
        k = self.totals()[1]
        dev = self.rst.device
        off = torch.arange(k, dtype=torch.int64, device=dev) * 20
        length = torch.full((k,), 20, dtype=torch.int32, device=dev)
        return (PacketBatch(data=self.rst, off=off, length=length, bytes_len=20 * k, max_len=20 if k else 0),
                self.rst_dst[:k])

    def taken(self, space: int) -> int:
        """How many of the answers send_packet_without_tcb accepts with
        `space` bytes of _queue_space: the list is stable, so they are the
        first taken(space) of it (tcp.hh:946-953)."""
        if int(space) < 0:
            raise ValueError("space: need >= 0")
        return min(self.totals()[1], int(space) // 20)


def tcp_rx_check(b: PacketBatch, status, conns, host, need, reject, index=None, cls=None, flags=0) -> tuple:
    """What tcp_rx refuses before any launch; returns (n, nbatch)."""
    if not isinstance(b, PacketBatch):
        raise ValueError("b: need a PacketBatch of IPv4 frames (an eth_rx bucket)")
    nbatch = b.n
    if nbatch > 0xFFFFFFFF:
        raise ValueError("b: at most 2^32-1 frames")
    if not isinstance(status, torch.Tensor) or status.dim() != 1:
        raise ValueError("status: need the 1-D uint8 tensor the frames call wrote, one entry per frame")
    _need(status, nbatch, torch.uint8, "status", b.device)
    _rx_filter(host, need, reject)
    if int(flags) & ~native.TCP_CSUM_OFFLOAD:
        raise ValueError(f"flags: unknown bits in {int(flags):#x}")
    n = nbatch
    if index is not None:
        if not isinstance(index, torch.Tensor) or index.dim() != 1:
            raise ValueError("index: need a 1-D int32 tensor of batch frame indices")
        n = int(index.numel())
        if n > 0xFFFFFFFF:
            raise ValueError("index: at most 2^32-1 entries")
        _need(index, n, torch.int32, "index", b.device)
    if cls is not None and (not isinstance(cls, torch.Tensor) or cls.dim() != 1):
        raise ValueError("cls: need a 1-D uint8 tensor of one entry per frame")
    _need(cls, n, torch.uint8, "cls", b.device)
    # not _device_handle: the check never asked for the handle, so a closed table is tcp_rx's to refuse
    if not isinstance(conns, TcpConns):
        raise ValueError(f"conns: need {TcpConns._a}")
    if conns.device != b.device:
        raise ValueError(f"conns: the table lives on {conns.device}, the data on {b.device}")
    return n, nbatch


def tcp_rx(b: PacketBatch, status: torch.Tensor, conns: TcpConns, host: int, need: int = TCP_NEED,
           reject: int = TCP_REJECT, index: torch.Tensor | None = None, flags: int = 0, want_class: bool = True,
           cls: torch.Tensor | None = None, stream=None) -> TcpRxResult:
    """sccsum_tcp_rx: the stateless part of tcp::received (tcp.hh:865-942) for
    the non-fragment frames of an IPv4 bucket — for us? TCP? the header and
    its data_offset, the connid looked up, then the listening ports, then the
    RST of respond_with_reset — ending in segments grouped per connection.

        r = tcp_rx(ip, status, conns, me)              # index=: a shard's slice of Steer.run's order
        run_conn, run_first = r.runs()
        r.segs(k)                                      # run k's records, arrival order: one tcb's input
        l4, dst = r.resets                             # -> ipv4_send(l4, dst, proto 6, ...) -> eth_send
        r.taken(space)                                 # how many of them _queue_space accepts

    flags=native.TCP_CSUM_OFFLOAD: the answers carry the folded pseudo-header
    sum instead of the full checksum."""
    lib = native.load()
    n, nbatch = tcp_rx_check(b, status, conns, host, need, reject, index, cls, flags)
    dev = b.device
    if cls is None and want_class:
        cls = _scratch(max(n, 1), dev, stream, torch.uint8)
    k = max(n, 1)
    runs = min(n, conns.nconns) + 1
    first = _scratch(5, dev, stream, torch.int32)
    order = _scratch(k, dev, stream, torch.int32)
    seg = _scratch(4 * k, dev, stream, torch.int64)
    src = _scratch(k, dev, stream, torch.int32)
    run_conn = _scratch(runs, dev, stream, torch.int32)
    run_first = _scratch(runs, dev, stream, torch.int32)
    rst = _scratch(5 * k + 3, dev, stream, torch.int32)   # 20 n bytes, padded to 16 for the batch it becomes
    rst_dst = _scratch(k, dev, stream, torch.int32)
    total = _scratch(4, dev, stream, torch.int64)
    ws = _scratch(int(lib.sccsum_tcp_rx_workspace(n, conns.nconns)), dev, stream)
    empty = nbatch == 0  # an empty tensor has no address
    code = lib.sccsum_tcp_rx(
        ctypes_ptr(b.data), b.bytes_len, None if empty else ctypes_ptr(b.off), None if empty else ctypes_ptr(b.length),
        nbatch, None if empty else ctypes_ptr(status), int(need), int(reject), int(host), conns.handle,
        None if index is None or n == 0 else ctypes_ptr(index), n, int(flags), _ptr(cls), ctypes_ptr(first),
        ctypes_ptr(order), ctypes_ptr(seg), ctypes_ptr(src), ctypes_ptr(run_conn), ctypes_ptr(run_first),
        ctypes_ptr(rst), ctypes_ptr(rst_dst), ctypes_ptr(total), ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_tcp_rx")
    return TcpRxResult(source=b, order=order[:n], first=first, seg=seg.view(torch.uint8).view(-1, 32)[:n],
                       src_all=src[:n], run_conn=run_conn, run_first=run_first, rst=rst.view(torch.uint8),
                       rst_dst=rst_dst[:n], total=total, cls=None if cls is None else cls[:n])


TCP_RCV_DTYPE = np.dtype([("next", "<u4"), ("window", "<u4"), ("room", "<u4"), ("cap", "<u4"), ("snd_una", "<u4"),
                          ("mss", "<u2"), ("flags", "u1"), ("pad", "u1"), ("reserved", "<u4", (2,))])
TCP_RCV_RUN_DTYPE = np.dtype([("taken", "<u4"), ("bytes", "<u4"), ("next", "<u4"), ("window", "<u4"), ("room", "<u4"),
                              ("desc_first", "<u4"), ("dst_off", "<u4"), ("flags", "u1"), ("stop", "u1"),
                              ("pad", "<u2")])


class _RunRecords:
    """A result with one record per run (or polled connection) in `run` and
    its counts in `total`: both on the host, fetched once.  The classes keep
    totals() and runs_host() themselves, for what their docstrings say."""

    def _totals_host(self) -> tuple:
        if self._totals is None:
            self._totals = tuple(int(x) for x in self.total.cpu().numpy().view(np.uint64))
        return self._totals

    def _runs_host(self, dtype) -> np.ndarray:
        if self._runs is None:
            self._runs = self.runs.cpu().numpy().reshape(-1).view(dtype)
        return self._runs


class _RxRunRecords(_RunRecords):
    """The run records of a fast path over tcp_rx's bucket 0 (`rx`): one per
    run of rx, the first `taken` segments of each dealt with."""

    @property
    def runs(self) -> torch.Tensor:
        """The R run records (a view)."""
        return self.run[:self.rx.totals()[0]]

    def rest(self, conn_run: int) -> torch.Tensor:
        """The records of run conn_run the host still has to walk with its
        tcb, from the state in the run record: segs(conn_run)[taken:]."""
        segs = self.rx.segs(conn_run)
        return segs[int(self.runs_host()["taken"][int(conn_run)]):]


@dataclass
class TcpRxDataResult(_RxRunRecords):
    """What sccsum_tcp_rx_data wrote (include/sccsum.h, "TCP receive fast
    path"): the leading in-sequence stretch of every run of tcp_rx's bucket 0."""
    rx: TcpRxResult
    run: torch.Tensor          # uint8 [>= R, 32]: sccsum_tcp_rcv_run records (TCP_RCV_RUN_DTYPE on the host)
    desc: torch.Tensor         # uint8 [16 n]: one sccsum_gather_desc per taken segment, grouped by run
    total: torch.Tensor        # int64 [4]: taken, bytes as emitted; the bytes needed without max_bytes
    _totals: tuple | None = None
    _runs: np.ndarray | None = None

    def totals(self) -> tuple:
        """(taken, bytes, needed) on the host (synchronises once)."""
        if self._totals is None:   # not _totals_host: three of the four words, read as the int64 they are
            t = self.total.cpu().numpy()
            self._totals = (int(t[0]), int(t[1]), int(t[2]))
        return self._totals

    def runs_host(self) -> np.ndarray:
        """The run records on the host as TCP_RCV_RUN_DTYPE (synchronises once)."""
        return self._runs_host(TCP_RCV_RUN_DTYPE)

    @property
    def descs(self) -> torch.Tensor:
        """The descriptors of the taken segments, uint8 [taken, 16] (DESC_DTYPE on the host)."""
        return self.desc.view(-1, 16)[:self.totals()[0]]

    def pack(self, stream=None) -> torch.Tensor:
        """Every connection's new in-order bytes packed back to back: run k's
        lie at [dst_off, dst_off + bytes) of the returned uint8 buffer."""
        taken, nbytes, _ = self.totals()
        data = _scratch(_round16(nbytes) or 16, self.desc.device, stream)
        if taken:
            native.check(native.load().sccsum_gather(ctypes_ptr(self.desc), taken, ctypes_ptr(data), _stream(stream)),
                         "sccsum_gather")
        return data


def _conn_records(t, width: int, name: str, struct: str, dev=None, rx=None) -> int:
    """A fast path's per-connection state: a uint8 [nconns, width] tensor of
    sccsum_tcp_<struct> records on `dev` (its own device when None), 16-byte
    aligned; with `rx`, for no more connections than tcp_rx's table had.
    Returns nconns."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f"{name}: need a uint8 [nconns, {width}] tensor of sccsum_tcp_{struct} records "
                         f"(TCP_{struct.upper()}_DTYPE)")
    nconns = int(t.shape[0])
    if nconns > native.TCP_MAX_CONNS:
        raise ValueError(f"{name}: at most 2^20 connections")
    _need(t, width * nconns, torch.uint8, name, t.device if dev is None else dev)
    if nconns and t.data_ptr() % 16:
        raise ValueError(f"{name}: need a 16-byte aligned tensor")
    if rx is not None and int(rx.run_conn.numel()) < min(int(rx.seg.shape[0]), nconns) + 1:
        raise ValueError(f"{name}: {nconns} connections, but rx was made with a table of fewer")
    return nconns


def _flat_tensors(dev, *named) -> None:
    """Every (name, tensor, dtype) is a contiguous 1-D tensor of that dtype on dev."""
    for what, t, dtype in named:
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError(f"{what}: need a 1-D {dtype} tensor")
        _need(t, t.numel(), dtype, what, dev)


def tcp_rx_data_check(rx, rcv, max_bytes) -> tuple:
    """What tcp_rx_data refuses before any launch; returns (n, nconns)."""
    if not isinstance(rx, TcpRxResult):
        raise ValueError("rx: need the TcpRxResult of tcp_rx")
    dev = rx.seg.device
    n = int(rx.seg.shape[0])
    nconns = _conn_records(rcv, 32, "rcv", "rcv", dev, rx)
    if not 0 <= int(max_bytes) <= 0xFFFFFFFF:
        raise ValueError("max_bytes: need 0..2^32-1")
    return n, nconns


def tcp_rx_data(rx: TcpRxResult, rcv: torch.Tensor, max_bytes: int = 0xFFFFFFFF, stream=None) -> TcpRxDataResult:
    """sccsum_tcp_rx_data: header prediction for a batch — the leading stretch
    of every connection's run that is acceptable, exactly at RCV.NXT, carries
    data, no control flag besides ACK / PSH and acknowledges nothing new: step
    4.7 of tcb::input_handle_other_state (tcp.hh:1497-1521) and nothing else.

        d = tcp_rx_data(r, rcv)                        # rcv: TCP_RCV_DTYPE records as uint8 [nconns, 32]
        buf = d.pack()                                 # the new in-order bytes of every connection
        for k, run in enumerate(d.runs_host()):        # one record per connection: next, window, room, the ACK
            ...                                        # buf[run.dst_off : run.dst_off + run.bytes] -> _rcv.data
            d.rest(k)                                  # what the tcb still walks itself, from that state

    Runs are taken while their packed text fits max_bytes; the runs from the
    first that does not fit onward take nothing (stop = TCP_STOP_CAPACITY)."""
    lib = native.load()
    n, nconns = tcp_rx_data_check(rx, rcv, max_bytes)
    dev = rx.seg.device
    k = max(n, 1)
    run = _scratch(4 * (min(n, nconns) + 1), dev, stream, torch.int64)
    desc = _scratch(2 * k, dev, stream, torch.int64)
    total = _scratch(4, dev, stream, torch.int64)
    ws = _scratch(int(lib.sccsum_tcp_rx_data_workspace(n, nconns)), dev, stream)
    empty = n == 0  # an empty tensor has no address
    code = lib.sccsum_tcp_rx_data(
        ctypes_ptr(rx.source.data), None if empty else ctypes_ptr(rx.seg), ctypes_ptr(rx.first),
        ctypes_ptr(rx.run_conn), ctypes_ptr(rx.run_first), ctypes_ptr(rx.total), n,
        ctypes_ptr(rcv) if nconns else None, nconns, int(max_bytes), ctypes_ptr(run), ctypes_ptr(desc),
        ctypes_ptr(total), ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_tcp_rx_data")
    return TcpRxDataResult(rx=rx, run=run.view(torch.uint8).view(-1, 32), desc=desc.view(torch.uint8)[:16 * n],
                           total=total)


@dataclass
class TcpSendResult:
    """What sccsum_tcp_send wrote (include/sccsum.h, "TCP layer"): the headers
    lie in the payloads' headroom, in payloads.data itself."""
    l4: PacketBatch            # header + payload per segment: what ipv4_send takes
    sum_batch: PacketBatch     # the spans whose results (with seeds) are ipv4_send's l4sum
    seeds: torch.Tensor        # int32 [n]
    proto: torch.Tensor        # uint8 [n]: 6
    needs_csum: torch.Tensor   # uint8 [n]: offload_info::needs_csum
    tso_seg: torch.Tensor      # int16 [n]: offload_info::tso_seg_size
    status: torch.Tensor       # uint8 [n]: native.ST_OK, or ST_RANGE / ST_MALFORMED (no header written)


def tcp_send_check(payloads: PacketBatch, out, src_host, mtu, flags) -> int:
    """What tcp_send refuses before any launch; returns n."""
    if not isinstance(payloads, PacketBatch):
        raise ValueError("payloads: need a PacketBatch of TCP payloads, each with hdr_len bytes of headroom")
    dev, n = payloads.device, payloads.n
    if n > 0xFFFFFFFF:
        raise ValueError("payloads: at most 2^32-1 segments")
    if not 68 <= int(mtu) <= 65535:
        raise ValueError(f"mtu: need 68..65535, got {mtu}")
    if int(flags) & ~(native.TCP_CSUM_OFFLOAD | native.TCP_TSO):
        raise ValueError(f"flags: unknown bits in {int(flags):#x}")
    if not 0 <= int(src_host) <= 0xFFFFFFFF:
        raise ValueError("src_host: need a host-order IPv4 address, 0..2^32-1")
    if not isinstance(out, torch.Tensor) or out.dim() != 2 or out.shape[1] != 24:
        raise ValueError("out: need a uint8 [n, 24] tensor of sccsum_tcp_out records (TCP_OUT_DTYPE)")
    _need(out, 24 * n, torch.uint8, "out", dev)
    return n


def tcp_send(payloads: PacketBatch, out: torch.Tensor, src_host: int, mtu: int, flags: int = 0,
             stream=None) -> TcpSendResult:
    """sccsum_tcp_send: tcb::output_one's header (tcp.hh:1620-1698) into the
    hdr_len bytes in front of every payload — the caller's headroom, whose
    last hdr_len - 20 bytes already hold the options — and the checksum
    pass's spans and seeds.

        t = tcp_send(payloads, out, me, 1500)          # out: TCP_OUT_DTYPE records as uint8 [n, 24]
        l4sum = spans(t.sum_batch, seeds=t.seeds)
        r = ipv4_send(t.l4, dst, t.proto, 1500, me, ids=ids, l4sum=l4sum, flags=native.SEND_L4)
        wire = eth_send(r, dst, table, hw, me, netmask, gw).pack()

    With native.TCP_CSUM_OFFLOAD the field gets the folded pseudo-header sum
    and needs_csum = 1; with native.TCP_TSO too a payload longer than its mss
    gets a pseudo-header of length 0 and tso_seg = mss."""
    lib = native.load()
    n = tcp_send_check(payloads, out, src_host, mtu, flags)
    dev = payloads.device
    k = max(n, 1)
    l4_off = _scratch(k, dev, stream, torch.int64)
    l4_len = _scratch(k, dev, stream, torch.int32)
    sum_len = _scratch(k, dev, stream, torch.int32)
    seeds = _scratch(k, dev, stream, torch.int32)
    tso = _scratch(k, dev, stream, torch.int16)
    proto = _scratch(k, dev, stream, torch.uint8)
    needs_csum = _scratch(k, dev, stream, torch.uint8)
    status = _scratch(k, dev, stream, torch.uint8)
    opts = native.TcpOpts(int(src_host), int(mtu), int(flags))
    empty = n == 0  # an empty tensor has no address
    code = lib.sccsum_tcp_send(
        ctypes.addressof(opts), ctypes_ptr(payloads.data), payloads.bytes_len,
        None if empty else ctypes_ptr(payloads.off), None if empty else ctypes_ptr(payloads.length),
        None if empty else ctypes_ptr(out), n, ctypes_ptr(l4_off), ctypes_ptr(l4_len), ctypes_ptr(sum_len),
        ctypes_ptr(seeds), ctypes_ptr(tso), ctypes_ptr(proto), ctypes_ptr(needs_csum), ctypes_ptr(status),
        _stream(stream))
    native.check(code, "sccsum_tcp_send")
    ml = payloads.max_len + 60 if payloads.max_len else 0
    l4 = PacketBatch(data=payloads.data, off=l4_off[:n], length=l4_len[:n], bytes_len=payloads.bytes_len, max_len=ml)
    sums = PacketBatch(data=payloads.data, off=l4_off[:n], length=sum_len[:n], bytes_len=payloads.bytes_len, max_len=ml)
    return TcpSendResult(l4=l4, sum_batch=sums, seeds=seeds[:n], proto=proto[:n], needs_csum=needs_csum[:n],
                         tso_seg=tso[:n], status=status[:n])


TCP_SND_DTYPE = np.dtype([("dst", "<u4"), ("next", "<u4"), ("una", "<u4"), ("window", "<u4"), ("cwnd", "<u4"),
                          ("rcv_next", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("mss", "<u2"), ("wnd", "<u2"),
                          ("flags", "u1"), ("pad", "u1", (3,)), ("reserved", "<u4", (3,))])
TCP_SND_RUN_DTYPE = np.dtype([("segs", "<u4"), ("bytes", "<u4"), ("seg_first", "<u4"), ("next", "<u4"), ("flags", "u1"),
                              ("stop", "u1"), ("pad", "<u2"), ("reserved", "<u4", (3,))])


@dataclass
class TcpTxDataResult(_RunRecords):   # no rx behind it: every record is a polled connection's
    """What sccsum_tcp_tx_data wrote (include/sccsum.h, "TCP transmit fast
    path"): every polled connection's unsent queue cut into segments."""
    run: torch.Tensor          # uint8 [P, 32]: sccsum_tcp_snd_run records (TCP_SND_RUN_DTYPE on the host)
    off: torch.Tensor          # int64 [max_segs]: the payload's place in the packed layout
    length: torch.Tensor       # int32 [max_segs]
    out: torch.Tensor          # uint8 [max_segs, 24]: sccsum_tcp_out records (TCP_OUT_DTYPE on the host)
    seg_first: torch.Tensor    # int32 [max_segs + 1]: segment f's descriptors are [seg_first[f], seg_first[f + 1])
    desc: torch.Tensor         # uint8 [16 (max_segs + nbuf)]: one sccsum_gather_desc per (segment, buffer) overlap
    total: torch.Tensor        # int64 [4]: segments, layout bytes, descriptors emitted; the layout bytes needed
    max_len: int               # no payload is longer
    _totals: tuple | None = None
    _runs: np.ndarray | None = None

    def totals(self) -> tuple:
        """(segments, layout bytes, descriptors, layout bytes needed) on the host (synchronises once)."""
        return self._totals_host()

    def runs_host(self) -> np.ndarray:
        """The run records on the host as TCP_SND_RUN_DTYPE (synchronises once)."""
        return self._runs_host(TCP_SND_RUN_DTYPE)

    @property
    def runs(self) -> torch.Tensor:
        """The P run records (a view)."""
        return self.run

    @property
    def descs(self) -> torch.Tensor:
        """The descriptors emitted, uint8 [pieces, 16] (DESC_DTYPE on the host)."""
        return self.desc.view(-1, 16)[:self.totals()[2]]

    def pack(self, stream=None) -> tuple:
        """Gathers every segment's payload into a new staging buffer, behind
        its headroom, and returns (payloads, out) as tcp_send takes them.  The
        staging copy is the segments' _snd.data clone: the queues' buffers are
        free once it has run."""
        nsegs, nbytes, pieces, _ = self.totals()
        data = _scratch(_round16(nbytes) or 16, self.desc.device, stream)
        if pieces:
            native.check(native.load().sccsum_gather(ctypes_ptr(self.desc), pieces, ctypes_ptr(data), _stream(stream)),
                         "sccsum_gather")
        payloads = PacketBatch(data=data, off=self.off[:nsegs], length=self.length[:nsegs], bytes_len=nbytes,
                               max_len=self.max_len)
        return payloads, self.out[:nsegs]

    def segs(self, k: int) -> tuple:
        """Connection k's slice (off, length, out): its new _snd.data entries, in stream order."""
        r = self.runs_host()[int(k)]
        lo, hi = int(r["seg_first"]), int(r["seg_first"]) + int(r["segs"])
        return self.off[lo:hi], self.length[lo:hi], self.out[lo:hi]


def tcp_tx_data_check(snd, buf_src, buf_len, buf_first, src_host, mtu, headroom, flags, max_packet_len, max_segs,
                      max_out_bytes) -> tuple:
    """What tcp_tx_data refuses before any launch; returns (nconns, nbuf)."""
    nconns = _conn_records(snd, 48, "snd", "snd")
    _flat_tensors(snd.device, ("buf_src", buf_src, torch.int64), ("buf_len", buf_len, torch.int32),
                  ("buf_first", buf_first, torch.int32))
    nbuf = int(buf_src.numel())
    if int(buf_len.numel()) != nbuf:
        raise ValueError("buf_len: need one length per buffer address")
    if nbuf > native.TCP_TX_MAX_BUFS:
        raise ValueError("buf_src: at most 2^31 buffers")
    if int(buf_first.numel()) != nconns + 1:
        raise ValueError("buf_first: need nconns + 1 entries")
    if not 68 <= int(mtu) <= 65535:
        raise ValueError(f"mtu: need 68..65535, got {mtu}")
    if not 20 <= int(headroom) <= 65535:
        raise ValueError(f"headroom: need 20..65535, got {headroom}")
    if int(flags) & ~native.TCP_TSO:
        raise ValueError(f"flags: unknown bits in {int(flags):#x}")
    if int(flags) & native.TCP_TSO and not 41 <= int(max_packet_len) <= 65535:
        raise ValueError(f"max_packet_len: need 41..65535, got {max_packet_len}")
    if not 0 <= int(src_host) <= 0xFFFFFFFF:
        raise ValueError("src_host: need a host-order IPv4 address, 0..2^32-1")
    if not 0 <= int(max_segs) <= native.TCP_TX_MAX_SEGS:
        raise ValueError("max_segs: need 0..2^31-1")
    if not 0 <= int(max_out_bytes) <= 0xFFFFFFFF:
        raise ValueError("max_out_bytes: need 0..2^32-1")
    return nconns, nbuf


def tcp_tx_data(snd: torch.Tensor, buf_src: torch.Tensor, buf_len: torch.Tensor, buf_first: torch.Tensor,
                src_host: int, mtu: int, max_segs: int, max_out_bytes: int = 0xFFFFFFFF, headroom: int = 20,
                flags: int = 0, max_packet_len: int = 65535, stream=None) -> TcpTxDataResult:
    """sccsum_tcp_tx_data: the cut tcb::get_packet's chain makes of every
    polled connection's unsent queue (can_send, get_transmit_packet and
    output_one's seq, tcp.hh:515-549, 1578-1606, 1635-1645), for the tcbs on
    the straight path; the others come back untouched (TCP_STOP_INELIGIBLE).

        d = tcp_tx_data(snd, src, length, first, me, 1500, max_segs=1 << 16)   # snd: TCP_SND_DTYPE as uint8 [P, 48]
        payloads, out = d.pack()                       # the staging copy: the queues' buffers are free
        t = tcp_send(payloads, out, me, 1500)          # and on as tcp_send's recipe goes
        for k, run in enumerate(d.runs_host()):        # one record per connection: pop run.bytes, next, the timer
            ...                                        # d.segs(k): its new _snd.data entries

    Connections are taken while their segments fit max_segs and their layout
    bytes max_out_bytes; from the first that does not fit onward they take
    nothing (stop = TCP_STOP_CAPACITY)."""
    lib = native.load()
    nconns, nbuf = tcp_tx_data_check(snd, buf_src, buf_len, buf_first, src_host, mtu, headroom, flags, max_packet_len,
                                     max_segs, max_out_bytes)
    dev = snd.device
    k = max(int(max_segs), 1)
    run = _scratch(4 * max(nconns, 1), dev, stream, torch.int64)
    off = _scratch(k, dev, stream, torch.int64)
    length = _scratch(k, dev, stream, torch.int32)
    out = _scratch(3 * k, dev, stream, torch.int64)
    seg_first = _scratch(k + 1, dev, stream, torch.int32)
    desc = _scratch(2 * (k + nbuf), dev, stream, torch.int64)
    total = _scratch(4, dev, stream, torch.int64)
    ws = _scratch(int(lib.sccsum_tcp_tx_data_workspace(nconns, nbuf)), dev, stream)
    opts = native.TcpTxOpts(int(src_host), int(mtu), int(max_packet_len), int(headroom), int(flags))
    code = lib.sccsum_tcp_tx_data(
        ctypes.addressof(opts), ctypes_ptr(snd) if nconns else None, nconns, ctypes_ptr(buf_src) if nbuf else None,
        ctypes_ptr(buf_len) if nbuf else None, ctypes_ptr(buf_first), nbuf, int(max_segs), int(max_out_bytes),
        ctypes_ptr(run), ctypes_ptr(off), ctypes_ptr(length), ctypes_ptr(out), ctypes_ptr(seg_first), ctypes_ptr(desc),
        ctypes_ptr(total), ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_tcp_tx_data")
    bound = int(max_packet_len) - 40 if int(flags) & native.TCP_TSO else int(mtu) - 40
    return TcpTxDataResult(run=run.view(torch.uint8).view(-1, 32)[:nconns], off=off[:int(max_segs)],
                           length=length[:int(max_segs)], out=out.view(torch.uint8).view(-1, 24)[:int(max_segs)],
                           seg_first=seg_first[:int(max_segs) + 1],
                           desc=desc.view(torch.uint8)[:16 * (int(max_segs) + nbuf)], total=total, max_len=bound)


TCP_ACK_DTYPE = np.dtype([("una", "<u4"), ("next", "<u4"), ("window", "<u4"), ("wl1", "<u4"), ("wl2", "<u4"),
                          ("cwnd", "<u4"), ("ssthresh", "<u4"), ("unsent_len", "<u4"), ("rcv_next", "<u4"),
                          ("rto", "<u4"), ("srtt", "<i8"), ("rttvar", "<i8"), ("mss", "<u2"), ("window_scale", "u1"),
                          ("flags", "u1"), ("reserved", "<u4")])
TCP_ACK_RUN_DTYPE = np.dtype([("taken", "<u4"), ("una", "<u4"), ("acked", "<u4"), ("popped", "<u4"), ("trim", "<u4"),
                              ("queue_freed", "<u4"), ("window", "<u4"), ("cwnd", "<u4"), ("srtt", "<i8"),
                              ("rttvar", "<i8"), ("rto", "<u4"), ("flags", "u1"), ("stop", "u1"), ("pad", "<u2"),
                              ("reserved", "<u4", (2,))])


@dataclass
class TcpAckQueues:
    """The retransmit queues (_snd.data) of every connection as a CSR:
    connection c's entries are [first[c], first[c + 1])."""
    first: torch.Tensor        # int32 [nconns + 1]
    length: torch.Tensor       # int32 [nq]: the entry's current p.len()
    meta: torch.Tensor         # int32 [nq]: data_len | (nr_transmits != 0) << 16
    tx: torch.Tensor           # int64 [nq]: tx_time in ns of now_ns's clock


@dataclass
class TcpRxAcksResult(_RxRunRecords):
    """What sccsum_tcp_rx_acks wrote (include/sccsum.h, "TCP ACK fast path"):
    the leading stretch of advancing pure ACKs of every run of tcp_rx's bucket 0."""
    rx: TcpRxResult
    run: torch.Tensor          # uint8 [>= R, 64]: sccsum_tcp_ack_run records (TCP_ACK_RUN_DTYPE on the host)
    total: torch.Tensor        # int64 [4]: R, taken ACKs, popped entries, acked bytes
    _totals: tuple | None = None
    _runs: np.ndarray | None = None

    def totals(self) -> tuple:
        """(R, taken, popped, acked) on the host (synchronises once)."""
        return self._totals_host()

    def runs_host(self) -> np.ndarray:
        """The run records on the host as TCP_ACK_RUN_DTYPE (synchronises once)."""
        return self._runs_host(TCP_ACK_RUN_DTYPE)


def tcp_rx_acks_check(rx, ack_state, queue, now_ns) -> tuple:
    """What tcp_rx_acks refuses before any launch; returns (n, nconns, nq)."""
    if not isinstance(rx, TcpRxResult):
        raise ValueError("rx: need the TcpRxResult of tcp_rx")
    dev = rx.seg.device
    n = int(rx.seg.shape[0])
    nconns = _conn_records(ack_state, 64, "ack_state", "ack", dev, rx)
    if not isinstance(queue, TcpAckQueues):
        raise ValueError("queue: need a TcpAckQueues")
    _flat_tensors(dev, ("queue.first", queue.first, torch.int32), ("queue.length", queue.length, torch.int32),
                  ("queue.meta", queue.meta, torch.int32), ("queue.tx", queue.tx, torch.int64))
    nq = int(queue.length.numel())
    if nq > native.TCP_ACK_MAX_ENTRIES:
        raise ValueError("queue.length: at most 2^31 entries")
    if int(queue.meta.numel()) != nq:
        raise ValueError("queue.meta: need one word per entry")
    if int(queue.tx.numel()) != nq:
        raise ValueError("queue.tx: need one time per entry")
    if int(queue.first.numel()) != nconns + 1:
        raise ValueError("queue.first: need nconns + 1 entries")
    if not -(1 << 63) <= int(now_ns) < (1 << 63):
        raise ValueError("now_ns: need a signed 64-bit count of nanoseconds")
    return n, nconns, nq


def tcp_rx_acks(rx: TcpRxResult, ack_state: torch.Tensor, queue: TcpAckQueues, now_ns: int,
                stream=None) -> TcpRxAcksResult:
    """sccsum_tcp_rx_acks: the sender half of header prediction for a batch —
    the leading stretch of every connection's run that is pure ACKs advancing
    SND.UNA: data_segment_acked with update_rto and update_cwnd, the window
    update and the closing can_send() (tcp.hh:1336-1400, 1026-1055, 1570-1574).

        a = tcp_rx_acks(r, ack_state, queues, now_ns)  # ack_state: TCP_ACK_DTYPE records as uint8 [nconns, 64]
        for k, run in enumerate(a.runs_host()):        # one record per connection: all the tcb takes over
            ...                                        # pop run.popped entries, trim run.trim, una, window, cwnd, rto
            a.rest(k)                                  # what the tcb still walks itself, from that state

    The next tcp_tx_data record (una, window, cwnd) follows from the run
    record without touching a segment."""
    lib = native.load()
    n, nconns, nq = tcp_rx_acks_check(rx, ack_state, queue, now_ns)
    dev = rx.seg.device
    run = _scratch(8 * (min(n, nconns) + 1), dev, stream, torch.int64)
    total = _scratch(4, dev, stream, torch.int64)
    ws = _scratch(int(lib.sccsum_tcp_rx_acks_workspace(n, nconns, nq)), dev, stream)
    empty = n == 0  # an empty tensor has no address
    code = lib.sccsum_tcp_rx_acks(
        None if empty else ctypes_ptr(rx.seg), ctypes_ptr(rx.first), ctypes_ptr(rx.run_conn),
        ctypes_ptr(rx.run_first), ctypes_ptr(rx.total), n, ctypes_ptr(ack_state) if nconns else None, nconns,
        ctypes_ptr(queue.first), ctypes_ptr(queue.length) if nq else None, ctypes_ptr(queue.meta) if nq else None,
        ctypes_ptr(queue.tx) if nq else None, nq, int(now_ns), ctypes_ptr(run), ctypes_ptr(total), ctypes_ptr(ws),
        _stream(stream))
    native.check(code, "sccsum_tcp_rx_acks")
    return TcpRxAcksResult(rx=rx, run=run.view(torch.uint8).view(-1, 64), total=total)


TCP_NEW_DTYPE = np.dtype([("local_ip", "<u4"), ("foreign_ip", "<u4"), ("local_port", "<u2"), ("foreign_port", "<u2"),
                          ("pos", "<u4"), ("irs", "<u4"), ("iss", "<u4"), ("snd_window", "<u4"), ("cwnd", "<u4"),
                          ("ssthresh", "<u4"), ("rcv_window", "<u4"), ("wl1", "<u4"), ("wl2", "<u4"), ("snd_mss", "<u2"),
                          ("local_mss", "<u2"), ("snd_wscale", "u1"), ("rcv_wscale", "u1"), ("flags", "u1"),
                          ("pad", "u1"), ("reserved", "<u4", (2,))])
TCP_PORTS = 65536


@dataclass
class TcpListenResult:
    """What sccsum_tcp_listen wrote (include/sccsum.h, "TCP passive open"):
    the LISTEN bucket of a tcp_rx up to the first segment that needs a tcb
    this very batch created."""
    rx: TcpRxResult
    cls: torch.Tensor          # uint8 [m_max]: native.TCP_LISTEN_* per position of the bucket
    rec: torch.Tensor          # uint8 [m_max, 64]: sccsum_tcp_new records (TCP_NEW_DTYPE on the host)
    synack: torch.Tensor       # uint8 [32 m_max]: the SYN-ACK staging, 32 bytes a created connection
    sa_off: torch.Tensor       # int64 [m_max]: 32 k + hdr_len
    sa_len: torch.Tensor       # int32 [m_max]: 0
    sa_out: torch.Tensor       # uint8 [m_max, 24]: sccsum_tcp_out records
    rst: torch.Tensor          # uint8 [>= 20 m_max]: the RST answers, 20 bytes each
    rst_dst: torch.Tensor      # int32 [m_max]: their destinations
    total: torch.Tensor        # int64 [4]: taken, created, resets, dropped
    _totals: tuple | None = None
    _new: np.ndarray | None = None

    def totals(self) -> tuple:
        """(taken, created, resets, dropped) on the host (synchronises once)."""
        if self._totals is None:
            self._totals = tuple(int(x) for x in self.total.cpu().numpy().view(np.uint64))
        return self._totals

    def new(self) -> np.ndarray:
        """The records of the created connections on the host as TCP_NEW_DTYPE, in arrival order."""
        if self._new is None:
            k = self.totals()[1]
            self._new = self.rec[:k].cpu().numpy().reshape(-1).view(TCP_NEW_DTYPE)
        return self._new

    def classes(self) -> torch.Tensor:
        """The class of every position of the bucket (a view; positions from
        totals()[0] on are TCP_LISTEN_LATER: the host's to walk, in order)."""
        b = self.rx.bounds()
        return self.cls[:min(int(b[2] - b[1]), int(self.cls.numel()))]

    @property
    def synacks(self) -> tuple:
        """(payloads, out): what tcp_send takes for the SYN-ACKs — empty
        payloads behind hdr_len bytes of headroom whose options are written,
        and their sccsum_tcp_out records."""
        k = self.totals()[1]
        return (PacketBatch(data=self.synack, off=self.sa_off[:k], length=self.sa_len[:k], bytes_len=32 * k, max_len=0),
                self.sa_out[:k])

    @property
    def resets(self) -> tuple:
        """(l4, dst): the RST answers as TcpRxResult.resets gives tcp_rx's."""
        k = self.totals()[2]
        dev = self.rst.device
        off = torch.arange(k, dtype=torch.int64, device=dev) * 20
        length = torch.full((k,), 20, dtype=torch.int32, device=dev)
        return (PacketBatch(data=self.rst, off=off, length=length, bytes_len=20 * k, max_len=20 if k else 0),
                self.rst_dst[:k])

    def later(self) -> torch.Tensor:
        """The records of the positions the host still walks, in order: segs of the bucket from `taken` on."""
        b = self.rx.bounds()
        return self.rx.seg[int(b[1]) + self.totals()[0]:int(b[2])]


def _isn_key(key) -> tuple:
    if isinstance(key, (bytes, bytearray)):
        if len(key) != 64:
            raise ValueError("key: need the 64 bytes of isn_secret::key")
        return tuple(int(x) for x in np.frombuffer(bytes(key), dtype="<u4"))
    words = [int(x) for x in key]
    if len(words) != 16 or any(not 0 <= w <= 0xFFFFFFFF for w in words):
        raise ValueError("key: need 64 bytes or sixteen 32-bit words")
    return tuple(words)


def tcp_listen_check(rx, b, space, key, isn_m, mtu, flags=0, m_max=None) -> tuple:
    """What tcp_listen refuses before any launch; returns (m_max, nbatch, key words)."""
    if not isinstance(rx, TcpRxResult):
        raise ValueError("rx: need the TcpRxResult of tcp_rx")
    if not isinstance(b, PacketBatch):
        raise ValueError("b: need the PacketBatch tcp_rx was given")
    dev = rx.seg.device
    if b.device != dev:
        raise ValueError(f"b: the frames live on {b.device}, rx on {dev}")
    nbatch = b.n
    if nbatch > 0xFFFFFFFF:
        raise ValueError("b: at most 2^32-1 frames")
    n = int(rx.seg.shape[0])
    m = n if m_max is None else int(m_max)
    if not 0 <= m <= min(n, native.TCP_LISTEN_MAX):
        raise ValueError(f"m_max: need 0..{min(n, native.TCP_LISTEN_MAX)} (the segments of rx, at most 2^30)")
    if isinstance(space, dict):
        for port, room in space.items():
            if not 0 <= int(port) < TCP_PORTS or not 0 <= int(room) <= 0xFFFFFFFF:
                raise ValueError(f"space: need {{port 0..65535: room 0..2^32-1}}, got {port}: {room}")
    elif not isinstance(space, torch.Tensor) or space.dim() != 1 or int(space.numel()) != TCP_PORTS:
        raise ValueError("space: need a {port: room} dict or a 1-D int32 tensor of 65536 entries")
    else:
        _need(space, TCP_PORTS, torch.int32, "space", dev)
    words = _isn_key(key)
    if not 0 <= int(isn_m) <= 0xFFFFFFFF:
        raise ValueError("isn_m: need microseconds / 4 truncated to 32 bits")
    if not 68 <= int(mtu) <= 65535:
        raise ValueError(f"mtu: need 68..65535, got {mtu}")
    if int(flags) & ~native.TCP_CSUM_OFFLOAD:
        raise ValueError(f"flags: unknown bits in {int(flags):#x}")
    return m, nbatch, words


def tcp_listen(rx: TcpRxResult, b: PacketBatch, space, key, isn_m: int, mtu: int, flags: int = 0, stream=None,
               m_max: int | None = None) -> TcpListenResult:
    """sccsum_tcp_listen: the passive open for the LISTEN bucket of a tcp_rx —
    listener->full(), the RST / ACK / SYN triage, and for every new connection
    the options parsed, the ISN, its record and its SYN-ACK (tcp.hh:888-929,
    1079-1141, 2067-2086; tcp.cc:34-138).

        ls = tcp_listen(r, ip, {80: 128}, secret, now_us // 4, 1500)   # space: room left per listening port
        for c in ls.new(): ...                         # make the tcb, inc_pending
        pay, out = ls.synacks                          # -> tcp_send(pay, out, me, 1500) -> spans -> ipv4_send
        l4, dst = ls.resets                            # -> ipv4_send(l4, dst, proto 6, ...)
        ls.later()                                     # the host walks these with its real _tcbs, in order

    m_max (default: every segment of rx) bounds the bucket's size without a
    host synchronisation; it sizes the outputs and the workspace."""
    lib = native.load()
    m, nbatch, words = tcp_listen_check(rx, b, space, key, isn_m, mtu, flags, m_max)
    dev = rx.seg.device
    if isinstance(space, dict):
        host = np.zeros(TCP_PORTS, dtype=np.uint32)
        for port, room in space.items():
            host[int(port)] = int(room)
        space = torch.from_numpy(host.view(np.int32)).to(dev)
    k = max(m, 1)
    cls = _scratch(k, dev, stream, torch.uint8)
    rec = _scratch(8 * k, dev, stream, torch.int64)
    synack = _scratch(4 * k, dev, stream, torch.int64)
    sa_off = _scratch(k, dev, stream, torch.int64)
    sa_len = _scratch(k, dev, stream, torch.int32)
    sa_out = _scratch(6 * k, dev, stream, torch.int32)
    rst = _scratch(5 * k + 3, dev, stream, torch.int32)
    rst_dst = _scratch(k, dev, stream, torch.int32)
    total = _scratch(4, dev, stream, torch.int64)
    ws = _scratch(int(lib.sccsum_tcp_listen_workspace(m)), dev, stream)
    opts = native.TcpListenOpts((ctypes.c_uint32 * 16)(*words), int(isn_m), int(mtu), int(flags))
    empty = m == 0  # an empty tensor has no address
    code = lib.sccsum_tcp_listen(
        opts, ctypes_ptr(b.data), b.bytes_len, None if nbatch == 0 else ctypes_ptr(b.off), nbatch,
        ctypes_ptr(rx.first), None if empty else ctypes_ptr(rx.order), None if empty else ctypes_ptr(rx.seg),
        None if empty else ctypes_ptr(rx.src_all), m, ctypes_ptr(space), ctypes_ptr(cls), ctypes_ptr(rec),
        ctypes_ptr(synack), ctypes_ptr(sa_off), ctypes_ptr(sa_len), ctypes_ptr(sa_out), ctypes_ptr(rst),
        ctypes_ptr(rst_dst), ctypes_ptr(total), ctypes_ptr(ws), _stream(stream))
    native.check(code, "sccsum_tcp_listen")
    return TcpListenResult(rx=rx, cls=cls[:m], rec=rec.view(torch.uint8).view(-1, 64)[:m], synack=synack.view(torch.uint8),
                           sa_off=sa_off[:m], sa_len=sa_len[:m], sa_out=sa_out.view(torch.uint8).view(-1, 24)[:m],
                           rst=rst.view(torch.uint8), rst_dst=rst_dst[:m], total=total)


class Engine:
    """sccsum_engine_*: ONE resident grid that takes steps (up to 4 batches
    each: a step's tx and rx halves, a shard's rx queues) while it runs, so the
    launch's ramp, drain and kernel boundary are paid once per run instead of
    once per step (include/sccsum.h, "Resident engine").

        eng = Engine(device=0, frames=True, ring_slots=1024, max_in_flight=2)
        eng.start(stream)
        step = eng.submit([(tx, out2, None), (rx, None, status)])   # like prepare_ipv4_frames_multi's items
        eng.wait(step)                                               # results readable by a D2H copy
        eng.finish(); stream.synchronize()                           # wait on the last step, then stop

    A run takes any number of steps: their descriptors cycle through a ring
    of ring_slots slots (max_steps is its old name).  Any number of threads
    may submit into a running engine and wait on its steps (the shards of one
    GPU); start / stop / finish / close belong to its owner.  max_in_flight
    is shared by every producer; producer_in_flight (0: none) also limits each
    submitting thread's own steps not yet done.

    fill=True (frames): the run also takes in-place fills, each as a generate
    step and a store step (sccsum_engine_submit_fill):
        step = eng.submit_fill([(frames, out2, status)], FILL_IP | FILL_L4)

    A step's tensors must stay alive (and unmodified) until its wait returns;
    submit keeps a reference until then.  One engine runs per device at a time
    (start raises SccsumError(SCCSUM_EBUSY) while another engine's run holds
    it); while it runs, every other kernel on the device waits for its stop."""

    def __init__(self, device: int = 0, frames: bool = True, max_steps: int | None = None, max_in_flight: int = 2,
                 fill: bool = False, ring_slots: int | None = None, idle_ms: int = 0, dep_ms: int = 0,
                 producer_in_flight: int = 0):
        import threading

        self._lib = native.load()
        h = ctypes.c_void_p()
        mode = (native.PIPE_IPV4 if frames else native.PIPE_SPANS) | (native.ENGINE_FILL if fill else 0)
        ring = ring_slots if ring_slots is not None else (max_steps if max_steps is not None else 1024)
        opts = native.EngineOpts(int(ring), int(max_in_flight), int(idle_ms), int(dep_ms), int(producer_in_flight))
        if ring <= 0 or max_in_flight <= 0:  # (0 would mean "the default" to the C-ABI)
            raise ValueError("ring_slots and max_in_flight must be >= 1")
        if hasattr(self._lib, "sccsum_engine_create_opts"):
            native.check(self._lib.sccsum_engine_create_opts(int(device), mode, ctypes.byref(opts), ctypes.byref(h)),
                         "sccsum_engine_create_opts")
        else:  # an ABI 3 build under A/B (SCCSUM_LIB + SCCSUM_ABI_ANY): its runs end at ring_slots steps
            native.check(self._lib.sccsum_engine_create(int(device), mode, int(ring), int(max_in_flight),
                                                         ctypes.byref(h)), "sccsum_engine_create")
        self._h = h
        self.frames = frames
        self.fill = fill
        self.max_in_flight = int(max_in_flight)
        self._keep: dict[int, tuple] = {}
        self._mu = threading.Lock()  # _keep and _last: producers may be several threads
        self._last = -1  # the run's latest step
        self._stream = None

    def start(self, stream=None):
        s = torch.cuda.current_stream() if stream is None else stream
        native.check(self._lib.sccsum_engine_start(self._h, s.cuda_stream), "sccsum_engine_start")
        self._stream = s
        with self._mu:
            self._keep.clear()
            self._last = -1

    def prepare(self, items, fill_mode: int = 0):
        """A step's descriptor array, checked once (items as for
        prepare_ipv4_frames_multi: (PacketBatch, out | None, status | None
        [, seeds])); submit_prepared(prep) then only crosses the C-ABI.
        fill_mode != 0: an in-place fill of the items (out2 required)."""
        if not items or len(items) > native.ENGINE_MAX_BATCHES:
            raise ValueError(f"1..{native.ENGINE_MAX_BATCHES} batches per step")
        if fill_mode and not self.fill:
            raise ValueError("fill steps need Engine(..., fill=True)")
        arr, _ = _batch_array(items, 2 if self.frames else 1, not self.frames, False, fill=bool(fill_mode))
        return (arr, len(items), max(it[0].max_len for it in items), items, int(fill_mode))

    def submit_prepared(self, prep, timeout_s: float = 10.0) -> int:
        arr, nb, ml, items, fill_mode = prep
        step = ctypes.c_uint64()
        if fill_mode:
            native.check(self._lib.sccsum_engine_submit_fill(self._h, ctypes.cast(arr, ctypes.c_void_p), nb, ml,
                                                              fill_mode, int(timeout_s * 1e9), ctypes.byref(step)),
                         "sccsum_engine_submit_fill")
        else:
            native.check(self._lib.sccsum_engine_submit(self._h, ctypes.cast(arr, ctypes.c_void_p), nb, ml,
                                                         int(timeout_s * 1e9), ctypes.byref(step)),
                         "sccsum_engine_submit")
        s = step.value
        with self._mu:
            self._keep[s] = prep
            self._last = max(self._last, s)
            if len(self._keep) > 4 * self.max_in_flight + 8:
                # done: a step max_in_flight (+ 1 for a fill's pair) before the newest was waited for by a submit
                for k in [k for k in self._keep if k + self.max_in_flight + 1 < self._last]:
                    del self._keep[k]
        return s

    def submit(self, items, timeout_s: float = 10.0) -> int:
        return self.submit_prepared(self.prepare(items), timeout_s)

    def submit_fill(self, items, mode: int = native.FILL_IP | native.FILL_L4, timeout_s: float = 10.0) -> int:
        """In-place fill of items [(PacketBatch, out2, status | None), ...]:
        returns the store step, done once the frames hold their checksums."""
        return self.submit_prepared(self.prepare(items, fill_mode=mode), timeout_s)

    def wait(self, step: int, timeout_s: float = 10.0) -> None:
        native.check(self._lib.sccsum_engine_wait(self._h, int(step), int(timeout_s * 1e9)), "sccsum_engine_wait")

    @property
    def last_step(self) -> int:
        """The run's latest submitted step (-1: none yet)."""
        return self._last

    def stop(self) -> None:
        native.check(self._lib.sccsum_engine_stop(self._h), "sccsum_engine_stop")

    def finish(self, timeout_s: float = 10.0) -> None:
        """Stop the run, then wait until its latest step is done: a give-up
        (EIDLE) or fault (EFAULT) raises here instead of passing unseen
        (a timed run that only stopped never looked).  The stop
        comes first because the grid leaves once its published steps are done:
        stopped after the wait, it left ~20 us later per run, the time for a
        waiting wave to poll the host and see the stop
        (profiles/r06_run_cost.log)."""
        self.stop()
        if self._last >= 0:
            self.wait(self._last, timeout_s)

    def close(self) -> None:
        """Destroy the engine (stopping and synchronising a running one).
        Raises SccsumError when its last run left a published step undone
        (SCCSUM_EIDLE / SCCSUM_EFAULT from sccsum_engine_destroy)."""
        if self._h:
            h, self._h = self._h, None
            self._keep.clear()
            native.check(self._lib.sccsum_engine_destroy(h), "sccsum_engine_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
