"""Sample ingest / framing front-end and UDP frame emitter (row N2).

Stands where the XADC + acquisition sequencer stand (imp/dsp_system_top.vhd:412-435,
imp/sequencer_dsp.vhd): a continuous int16 sample stream is cut into 16384-sample frames and moved
host -> device through two pinned staging buffers so the copy of batch k+1 overlaps the processing of
batch k.  This is where PCIe (63 GB/s, ~0.48 M frames/s of int16... 1.9 M) rather than HBM becomes the
limit; the benchmark keeps inputs resident in HBM and never includes this stage.
"""
from __future__ import annotations

import socket
from typing import Iterable, Iterator, Optional

import numpy as np
import torch

from . import frames

N = frames.FFT_SIZE
P12_FRAME_BYTES = 3 * N // 2       # SA_P12_FRAME_BYTES (include/specan.h): 24576


def pack12(samples) -> np.ndarray:
    """Pack 12-bit samples, two to three bytes, along the last axis (the "p12" format of include/specan.h): sample n
    occupies bits [12n, 12n+12) of the row read as a little-endian bit stream.  ``samples``: integers in [-2048, 2047]
    (``ValueError`` otherwise), last axis of even length n; returns uint8 with last axis 3n/2.

    For tests, tools and files, not for the hot path: at 30 G samples/s no host packer keeps up.  The format pays when
    the source (a digitiser, a capture file) delivers it."""
    s = np.asarray(samples)
    if s.dtype.kind not in "iu":
        raise ValueError("samples must be integers")
    if s.shape[-1] % 2:
        raise ValueError("the last axis must hold an even number of samples")
    if s.size and (s.min() < -2048 or s.max() > 2047):
        raise ValueError("samples do not fit 12 bits")
    u = s.astype(np.int32) & 0xFFF
    u0, u1 = u[..., 0::2], u[..., 1::2]
    out = np.empty(s.shape[:-1] + (s.shape[-1] // 2, 3), np.uint8)
    out[..., 0] = u0 & 0xFF
    out[..., 1] = (u0 >> 8) | ((u1 & 0xF) << 4)
    out[..., 2] = u1 >> 4
    return out.reshape(s.shape[:-1] + (3 * (s.shape[-1] // 2),))


def unpack12(packed) -> np.ndarray:
    """The inverse of :func:`pack12` along the last axis (a multiple of 3 bytes, ``ValueError`` otherwise): uint8 -> int16,
    sign-extended.  Every bit pattern is valid.  For tests, tools and files, like :func:`pack12`."""
    b = np.asarray(packed)
    if b.dtype != np.uint8:
        raise ValueError("packed samples must be uint8")
    if b.shape[-1] % 3:
        raise ValueError("the last axis must hold a multiple of 3 bytes")
    t = b.reshape(b.shape[:-1] + (b.shape[-1] // 3, 3)).astype(np.int16)
    out = np.empty(b.shape[:-1] + (b.shape[-1] // 3, 2), np.int16)
    out[..., 0] = t[..., 0] | ((t[..., 1] & 0xF) << 8)
    out[..., 1] = (t[..., 1] >> 4) | (t[..., 2] << 4)
    out = (out ^ 0x800) - 0x800                              # sign extension of 12 bits
    return out.reshape(b.shape[:-1] + (2 * (b.shape[-1] // 3),))


class FrameCutter:
    """Cut an arbitrary sequence of int16 sample blocks into frames of 16384 samples.

    ``hop`` < 16384 gives overlapping frames (hop = 16384 reproduces the FPGA: back-to-back
    acquisitions, no overlap).  Samples are kept as delivered (the XADC delivers 12-bit values
    sign-extended to int16, imp/dsp_system_top.vhd:435).

    ``packed=True``: the stream is the packed 12-bit byte stream (:func:`pack12`), pushed in chunks of any length
    (a chunk may end inside a pair of samples), and the frames come out packed, [k, 24576] uint8.  ``hop`` must then
    be even, so that every frame starts on a whole byte."""

    def __init__(self, hop: int = N, packed: bool = False):
        if not 0 < hop <= N:
            raise ValueError("hop must be in 1..16384")
        if packed and hop % 2:
            raise ValueError("hop must be even for a packed stream (frames start on whole bytes)")
        self.hop = hop
        self.packed = bool(packed)
        self._buf = np.empty(0, np.uint8 if packed else np.int16)

    def _cut(self, new: np.ndarray, row: int, hop: int) -> np.ndarray:
        """Append `new` to the buffer and take out every complete frame: `row` elements of the buffer each, `hop` apart."""
        self._buf = np.concatenate([self._buf, new.reshape(-1)])
        n = self._buf.size
        if n < row:
            return np.empty((0, row), self._buf.dtype)
        k = (n - row) // hop + 1
        idx = np.arange(k)[:, None] * hop + np.arange(row)[None, :]
        out = self._buf[idx]
        self._buf = self._buf[k * hop:]
        return out

    def push(self, samples) -> np.ndarray:
        """Append samples; return the frames that became complete, shape [k, 16384] (k may be 0).
        Packed: append bytes of the packed stream; the frames are [k, 24576] uint8."""
        if self.packed:
            b = (np.frombuffer(samples, np.uint8) if isinstance(samples, (bytes, bytearray, memoryview))
                 else np.asarray(samples))
            if b.dtype != np.uint8:
                raise ValueError("a packed stream is pushed as uint8 / bytes")
            return self._cut(b, P12_FRAME_BYTES, 3 * self.hop // 2)          # in bytes
        s = np.asarray(samples)
        if s.dtype != np.int16:
            if np.any(s < -32768) or np.any(s > 32767):
                raise ValueError("samples do not fit int16")
            s = s.astype(np.int16)
        return self._cut(s, N, self.hop)

    @property
    def pending(self) -> int:
        """Samples (packed: bytes) waiting for the rest of their frame."""
        return int(self._buf.size)


class StreamCutter:
    """Cut a sample stream into 1-D blocks for the device-side framing of ``SpectrumChain.process_q15(x, hop=...)``: every
    block holds exactly ``frames`` frames' worth of the stream, (frames - 1) * hop + 16384 samples, and consecutive blocks
    start frames * hop samples apart -- so each block repeats the last 16384 - hop samples of the one before it (carried
    here, on the host), and every other sample crosses the link once instead of 16384 / hop times.  The frames of the
    blocks, in order, are the frames :class:`FrameCutter` ``(hop)`` cuts from the same stream, once each.

    ``hop``: a multiple of 8 in 8..16384, what the device call takes (``ValueError`` otherwise).  ``packed=True``: the
    stream is the packed 12-bit byte stream (:func:`pack12`), pushed in chunks of any length (a chunk may end inside a
    pair of samples), and the blocks are uint8, 3/2 bytes per sample."""

    def __init__(self, hop: int, frames: int, packed: bool = False):
        if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or not 8 <= hop <= N or hop % 8:
            raise ValueError("hop must be a multiple of 8 in 8..16384")
        if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or frames < 1:
            raise ValueError("frames must be a positive integer")
        self.hop, self.frames, self.packed = int(hop), int(frames), bool(packed)
        self._row, self._dtype = (P12_FRAME_BYTES, np.uint8) if packed else (N, np.int16)
        self._step = self._row * self.hop // N                      # elements of the buffer per hop
        self._buf = np.empty(0, self._dtype)

    @property
    def block_size(self) -> int:
        """Elements (samples; packed: bytes) of a full block."""
        return (self.frames - 1) * self._step + self._row

    def push(self, samples) -> list:
        """Append samples (packed: bytes of the packed stream); return the blocks that became complete, a list of 1-D
        arrays of ``block_size`` elements (possibly empty)."""
        if self.packed:
            s = (np.frombuffer(samples, np.uint8) if isinstance(samples, (bytes, bytearray, memoryview))
                 else np.asarray(samples))
            if s.dtype != np.uint8:
                raise ValueError("a packed stream is pushed as uint8 / bytes")
        else:
            s = np.asarray(samples)
            if s.dtype != np.int16:
                if np.any(s < -32768) or np.any(s > 32767):
                    raise ValueError("samples do not fit int16")
                s = s.astype(np.int16)
        self._buf = np.concatenate([self._buf, s.reshape(-1)])
        size, advance = self.block_size, self.frames * self._step
        k = 0 if self._buf.size < size else (self._buf.size - size) // advance + 1
        out = [self._buf[i * advance:i * advance + size].copy() for i in range(k)]
        self._buf = self._buf[k * advance:]
        return out

    def flush(self):
        """A last block of the complete frames that remain (fewer than ``frames``), or None.  What is left after it is
        less than a frame beyond the last hop; pushing may go on."""
        if self._buf.size < self._row:
            return None
        k = (self._buf.size - self._row) // self._step + 1
        out = self._buf[:(k - 1) * self._step + self._row].copy()
        self._buf = self._buf[k * self._step:]
        return out

    @property
    def pending(self) -> int:
        """Samples (packed: bytes) held for the next block."""
        return int(self._buf.size)


class DeviceFeeder:
    """Buffered host -> device mover: ``feed(batch_iter)`` yields device tensors [B,16384] int16
    (``packed``: [B,24576] uint8) while the next batch is already in flight on a side stream.

    Two pinned staging buffers, two device buffers, and FOUR events created once (a "copied" and a
    "consumed" event per slot).  Measured (profiles/r2_ingest.txt): 1.42 M frames/s = 46.5 GB/s end to end
    against 55 GB/s for the bare pinned copy, i.e. PCIe-bound, with the copy of batch k+1 under the kernels of
    batch k.  The staging copy numpy -> pinned runs on torch's intra-op thread pool: on a host that exposes
    more cores than the job may use (a 16-CPU share of a 256-core box) the default pool stalls it for 50-100 ms
    every dozen batches -- pass ``host_threads`` (or call torch.set_num_threads yourself).

    ``packed=True``: the batches are packed 12-bit frames, [B,24576] uint8 (what a packed :class:`FrameCutter` cuts), and
    so are the staging and device buffers and the tensors handed out: three quarters of the bytes per frame on the link.
    ``SpectrumChain.process_f32`` takes them as they are.

    ``stream=True``: the batches are 1-D blocks of a sample stream (what :class:`StreamCutter` cuts; packed or not), of at
    most ``max_batch`` x 16384 samples.  They are staged, copied and handed out 1-D, for
    ``SpectrumChain.process_q15(x, hop=...)``, which cuts the overlapping frames on the device.

    **The consumer's contract.**  The tensor handed out for batch k is a view of a slot's device buffer.  The consumer
    enqueues its work on the stream that was current when ``feed`` started, between taking batch k and asking for
    batch k+1, and the feeder rewrites a slot -- its pinned and its device buffer -- only after the consumer's work on
    it is ordered on that stream and has run there (a host wait on the slot's "consumed" event).

    ``consumer_depth`` (1..4) says how far the consumer's reads lag behind its calls.  1 (the default): the work on
    batch k is on the current stream when the consumer asks for batch k+1 -- any stream-ordered consumer, a
    ``SpectrumChain`` at overlap depth 1.  d > 1: the consumer is a chain with ``set_overlap(d)`` (or anything that
    follows the overlap contract of include/specan.h): call k runs on a stream of the library's and the current stream
    joins it only when call k+d-1 is made, so the slot of batch k counts as consumed from that call on, and the feeder
    keeps d+1 slots (d batches lent to the consumer, one being filled) where depth 1 keeps two.  A feeder whose
    ``consumer_depth`` is smaller than the chain's overlap depth rewrites buffers under running kernels.

    **At the end of a feed** -- the iterator is exhausted, or the consumer stops early -- the last d-1 calls of an
    overlapped consumer are not joined by anything: call ``SpectrumChain.flush()`` on the same current stream before
    the results are read there AND before the next ``feed()`` of this feeder is started; the next ``feed()`` takes
    everything enqueued on the current stream at its start as the end of the earlier consumers' work.  With
    ``consumer_depth`` 1 nothing is to be done.

    **Refused** (``ValueError``): a ``consumer_depth`` outside 1..4, a batch of more than ``max_batch`` frames (``stream``:
    a block of more than ``max_batch`` frames' elements).
    ``RuntimeError``: going on with an iterator of an earlier ``feed()`` after a new ``feed()`` of the same feeder has
    started -- one feed at a time; an abandoned iterator needs no closing."""

    MAX_CONSUMER_DEPTH = 4              # sa_set_overlap's largest depth (include/specan.h)

    def __init__(self, device: torch.device | int = 0, max_batch: int = 256, host_threads: Optional[int] = None,
                 packed: bool = False, consumer_depth: int = 1, stream: bool = False):
        if not 1 <= int(consumer_depth) <= self.MAX_CONSUMER_DEPTH:
            raise ValueError("consumer_depth must be in 1..4 (the overlap depths of SpectrumChain.set_overlap)")
        if host_threads is not None:
            torch.set_num_threads(int(host_threads))
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.max_batch = max_batch
        self.packed = bool(packed)
        self.consumer_depth = int(consumer_depth)
        self.stream = bool(stream)
        self._row, self._np_dtype = (P12_FRAME_BYTES, np.uint8) if packed else (N, np.int16)
        dt = torch.uint8 if packed else torch.int16
        ns = self._nslots = 2 if self.consumer_depth == 1 else self.consumer_depth + 1
        # a slot holds max_batch rows: frames, or in stream mode the same room as one row of elements
        self._shape = (max_batch * self._row,) if self.stream else (max_batch, self._row)
        self._pinned = [torch.empty(self._shape, dtype=dt).pin_memory() for _ in range(ns)]
        self._dev = [torch.empty(self._shape, dtype=dt, device=self.device) for _ in range(ns)]
        self._copy_stream = torch.cuda.Stream(self.device)
        self._copied = [torch.cuda.Event() for _ in range(ns)]      # slot's host->device copy has run
        self._consumed = [torch.cuda.Event() for _ in range(ns)]    # slot's consumer work is ordered on the stream and has run
        self._used = [False] * ns
        self._copying = [False] * ns    # a copy into the slot was enqueued and the slot not handed out since (abandoned feed)
        self._lent = []                 # slots handed out and not yet recorded as consumed, oldest first
        self._feed = 0                  # serial number of the feed() that owns the feeder

    def _retire(self, cur, keep: int):
        """Record "consumed" on `cur` for all but the newest `keep` lent slots: the consumer's latest call joined the
        one made consumer_depth-1 calls before it, and a new feed() starts behind the consumer's flush."""
        while len(self._lent) > keep:
            s = self._lent.pop(0)
            self._consumed[s].record(cur)
            self._used[s] = True

    def feed(self, batches: Iterable[np.ndarray]) -> Iterator[torch.Tensor]:
        cur = torch.cuda.current_stream(self.device)
        self._feed += 1
        me = self._feed
        # what an earlier feed left lent (an overlapped consumer's last calls, a batch taken from an abandoned iterator):
        # the consumer has flushed onto `cur` by now (class docstring)
        self._retire(cur, 0)
        pend = None                                             # (slot, n_frames) handed out next
        for i, b in enumerate(batches):
            b = np.ascontiguousarray(b, self._np_dtype).reshape((-1,) + self._shape[1:])
            n = b.shape[0]                                      # frames; stream mode: elements
            if n > self._shape[0]:
                raise ValueError("batch larger than max_batch")
            slot = i % self._nslots
            if self._used[slot]:
                self._consumed[slot].synchronize()              # the slot's previous consumer is done with it
            if self._copying[slot]:
                self._copied[slot].synchronize()                # an abandoned feed's copy still reads the pinned buffer
            self._pinned[slot][:n].copy_(torch.from_numpy(b))
            with torch.cuda.stream(self._copy_stream):
                self._dev[slot][:n].copy_(self._pinned[slot][:n], non_blocking=True)
                self._copied[slot].record(self._copy_stream)
            self._copying[slot] = True
            if pend is not None:
                ps, pn = pend
                self._copying[ps] = False
                self._lent.append(ps)
                yield self._dev[ps][:pn]                        # the consumer enqueues its work on `cur` here
                if me != self._feed:
                    raise RuntimeError("DeviceFeeder: this iterator was superseded by a later feed()")
                self._retire(cur, self.consumer_depth - 1)
            cur.wait_event(self._copied[slot])
            pend = (slot, n)
        if pend is not None:
            ps, pn = pend
            self._copying[ps] = False
            self._lent.append(ps)
            yield self._dev[ps][:pn]
            if me != self._feed:
                raise RuntimeError("DeviceFeeder: this iterator was superseded by a later feed()")
            self._retire(cur, self.consumer_depth - 1)


def udp_emit(frame_bytes: bytes, addr: tuple[str, int], sock: Optional[socket.socket] = None,
             src_port: Optional[int] = None) -> int:
    """Send one 65536-byte frame as the FPGA MAC does: 64 datagrams of 1 index byte + 1024 data bytes
    (gui.py:48-50, 318-339; the board sends from port 5005 to port 6006, imp/head_data.mif:27-38).
    Returns the number of datagrams sent."""
    own = sock is None
    if own:
        sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        if src_port is not None:
            sock.bind(("", src_port))
    try:
        n = 0
        for p in frames.frame_to_udp_payloads(frame_bytes):
            sock.sendto(p, addr)
            n += 1
        return n
    finally:
        if own:
            sock.close()
