"""Host-side mirror of the reference's signal-path contract, over the C ABI.

``SpectrumChain`` is the "virtual FPGA" seen from the host: it takes the same command bytes
(scripts/fft_analyzer_gui.py:28-37), the same ``0xF1`` + 12 x int8 coefficient upload
(gui.py:591-613 -> new/rx_filter_coeff.vhd:41-66) and produces the same 65536-byte frames
(imp/sequ2.vhd:153, gui.py:250-260) -- batched over thousands of frames resident in HBM.
PyTorch is used only for device memory and streams.  The handle, the control plane and the process calls are here; the
reductions of the handle-less libraries are the mixin of reductions.py.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import abi, frames, holds, reductions
from .abi import (SA_FILTER_CUSTOM, SA_FILTER_DEFAULT, SA_FILTER_NONE, SA_FILTER_WIDE, SA_N, SA_P12_FRAME_BYTES,
                  SA_OUT_MAG_FULL, SA_OUT_MAG_HALF, SA_OUT_MARKER, SA_OUT_SPEC_HALF, SA_OUT_TIME, SA_PRECISION_F32,
                  SA_PRECISION_F64_STATE, SA_Q15_OUT_IQ, SA_Q15_OUT_MAG, SA_Q15_OUT_MARKER, SpecanError)

# command bytes, same names as gui.py:28-37
UART_REQUEST_CMD = 0xA5
FPGA_RESET_CMD = 0xFF
ETHERNET_MODE_CMD = 0xEF
UART_MODE_CMD = 0xFE
START_COMMAND = 0x55
FILTER_UPDATE_CMD = 0xF1
FILTER_DEFAULT_CMD = 0x00
FILTER_CUSTOM_CMD = 0xA1
FILTER_NONE_CMD = 0xB1
FILTER_WIDE_CMD = 0xA2          # build extension

FRAME_SIZE_BYTES = 65536        # gui.py:42
SAMPLES_PER_FRAME = 16384       # gui.py:43
FFT_SIZE = 16384                # gui.py:44
FS_HZ = 1_000_000.0             # gui.py:45

_PRECISIONS = {"f32": SA_PRECISION_F32, "f64": SA_PRECISION_F64_STATE}


# C entry point -> (takes scale, takes out_kind): the argument lists of include/specan.h, `..., batch[, kind], stream`
_ARGS = {"sa_process_f32": (False, True), "sa_process_f32_i16": (True, True), "sa_process_f32_p12": (True, True),
         "sa_process_q15": (False, False), "sa_process_q15_out": (False, True), "sa_process_q15_p12": (False, True),
         "sa_filter_q15": (False, False), "sa_filter_q15_p12": (False, False)}
# C entry point -> the ints behind batch: the argument lists of include/specan_ext.h, `..., batch, log2a[, hop], stream` (no
# scale, no out_kind)
_EXT_ARGS = {"sa_spectra_q15": ("log2a", "hop"), "sa_spectra_q15_p12": ("log2a", "hop"), "sa_fold_iq_q15": ("log2a",)}


class _Chain(NamedTuple):
    """What a process call has to know about one chain.  A new input form is one row of ``inputs``, a new output kind one
    row of ``outputs``."""
    outputs: dict   # out_kind -> (C code, shape of one row of the output, torch dtype[, frames per row]): a row is one frame's
                    # output, or, where the fourth entry names an A > 1, that of A consecutive frames (B a multiple of A)
    inputs: dict    # torch dtype of x -> _form(...); the first dtype stands in the message for an x that is no tensor of a
                    # listed dtype
    streams: dict = {}  # the same for a call with ``hop``: x is ONE 1-D stream, frame b its `row` elements from element
                        # b * row * hop / 16384 on, and the hop goes out inside the kind word, SA_Q15_HOP_KIND(code, hop), or
                        # as the entry point's own argument (_EXT_ARGS).  Empty: the chain takes frames only.

    def output(self, out_kind) -> tuple:
        """(C code, shape of one row, torch dtype, frames per row) of ``out_kind``."""
        if out_kind not in self.outputs:
            raise SpecanError(abi.SA_EINVAL, f"out_kind must be one of {sorted(self.outputs)}")
        return (self.outputs[out_kind] + (1,))[:4]

    def rows(self, out_kind, B: int) -> int:
        """The rows of the output of a call on ``B`` frames: SA_ESHAPE where B is no multiple of the frames per row."""
        per_row = self.output(out_kind)[3]
        if B % per_row:
            raise SpecanError(abi.SA_ESHAPE, f"the batch ({B} frames) must be a multiple of {per_row}")
        return B // per_row


def _form(row, outputs: dict, name: str, **other) -> tuple:
    """One input form: (row of x -- its length, or its shape as a tuple --, {out_kind: (C entry point, takes scale, takes
    out_kind)}).  The entry point is ``name``, or what ``other`` names for that out_kind; one of _EXT_ARGS takes neither."""
    return row, {k: (other.get(k, name),) + _ARGS.get(other.get(k, name), (False, False)) for k in outputs}


_HALF = SA_N // 2 + 1
_FLOAT_OUT = {"mag_full": (SA_OUT_MAG_FULL, (SA_N,), torch.float32),
              "mag_half": (SA_OUT_MAG_HALF, (_HALF,), torch.float32),
              "spec_half": (SA_OUT_SPEC_HALF, (_HALF,), torch.complex64),
              "time": (SA_OUT_TIME, (SA_N,), torch.float32),
              "marker": (SA_OUT_MARKER, (4,), torch.int32)}
FLOAT_CHAIN = _Chain(_FLOAT_OUT, {torch.float32: _form(SA_N, _FLOAT_OUT, "sa_process_f32"),
                                  torch.int16: _form(SA_N, _FLOAT_OUT, "sa_process_f32_i16"),
                                  torch.uint8: _form(SA_P12_FRAME_BYTES, _FLOAT_OUT, "sa_process_f32_p12")})
_Q15_OUT = {"iq": (SA_Q15_OUT_IQ, (SA_N, 2), torch.int16),
            "mag": (SA_Q15_OUT_MAG, (SA_N,), torch.float32),
            "marker": (SA_Q15_OUT_MARKER, (4,), torch.int32)}
def _q15_streams(outputs: dict) -> dict:
    """The stream forms of the Q15 chain: the two entry points whose out_kind word carries the hop."""
    return {torch.int16: _form(SA_N, outputs, "sa_process_q15_out"),
            torch.uint8: _form(SA_P12_FRAME_BYTES, outputs, "sa_process_q15_p12")}


Q15_CHAIN = _Chain(_Q15_OUT, {torch.int16: _form(SA_N, _Q15_OUT, "sa_process_q15_out", iq="sa_process_q15"),
                              torch.uint8: _form(SA_P12_FRAME_BYTES, _Q15_OUT, "sa_process_q15_p12")},
                   _q15_streams(_Q15_OUT))
# the Q15 chain's display trace (traces_q15): one output per bucket width W = 2^k, named by W; a table of its own, so that
# process_q15(out_kind=...) keeps the three kinds it has
_TRACE_OUT = {1 << k: (abi.SA_Q15_TRACE_KIND(k), (SA_N >> k, 2), torch.float32)
              for k in range(abi.SA_Q15_TRACE_LOG2W_MIN, abi.SA_Q15_TRACE_LOG2W_MAX + 1)}
Q15_TRACE_CHAIN = _Chain(_TRACE_OUT, {torch.int16: _form(SA_N, _TRACE_OUT, "sa_process_q15_out"),
                                      torch.uint8: _form(SA_P12_FRAME_BYTES, _TRACE_OUT, "sa_process_q15_p12")},
                         _q15_streams(_TRACE_OUT))
# the trace over groups of A = 2^a consecutive frames (traces_q15(group=A)): one output per (W, A), one row per group
_TRACE_AVG_OUT = {(1 << k, 1 << a): (abi.SA_Q15_TRACE_AVG_KIND(k, a), (SA_N >> k, 2), torch.float32, 1 << a)
                  for k in range(abi.SA_Q15_TRACE_LOG2W_MIN, abi.SA_Q15_TRACE_LOG2W_MAX + 1)
                  for a in range(abi.SA_Q15_TRACE_LOG2A_MIN, abi.SA_Q15_TRACE_LOG2A_MAX + 1)}
TRACE_GROUPS = tuple(1 << a for a in range(abi.SA_Q15_TRACE_LOG2A_MIN, abi.SA_Q15_TRACE_LOG2A_MAX + 1))
Q15_TRACE_AVG_CHAIN = _Chain(_TRACE_AVG_OUT, {torch.int16: _form(SA_N, _TRACE_AVG_OUT, "sa_process_q15_out"),
                                              torch.uint8: _form(SA_P12_FRAME_BYTES, _TRACE_AVG_OUT, "sa_process_q15_p12")},
                             _q15_streams(_TRACE_AVG_OUT))
# the Q15 chain without its FFT (filter_q15): one output, which has no name
_WINDOW_OUT = {None: (SA_Q15_OUT_IQ, (SA_N,), torch.int16)}
Q15_WINDOW_CHAIN = _Chain(_WINDOW_OUT, {torch.int16: _form(SA_N, _WINDOW_OUT, "sa_filter_q15"),
                                        torch.uint8: _form(SA_P12_FRAME_BYTES, _WINDOW_OUT, "sa_filter_q15_p12")})
# the calls of include/specan_ext.h: one record per bin and group of A frames (spectra_q15), one output per A, named by A;
# and the fold alone (fold_iq_q15), whose input rows are the IQ frames themselves
_SPECTRA_OUT = {A: (SA_Q15_OUT_IQ, (SA_N, 2), torch.float32, A) for A in TRACE_GROUPS}
_SPECTRA_IN = {torch.int16: _form(SA_N, _SPECTRA_OUT, "sa_spectra_q15"),
               torch.uint8: _form(SA_P12_FRAME_BYTES, _SPECTRA_OUT, "sa_spectra_q15_p12")}
Q15_SPECTRA_CHAIN = _Chain(_SPECTRA_OUT, _SPECTRA_IN, _SPECTRA_IN)
Q15_FOLD_CHAIN = _Chain(_SPECTRA_OUT, {torch.int16: _form((SA_N, 2), _SPECTRA_OUT, "sa_fold_iq_q15")})
# the fold of float magnitudes (include/specan_fold.h; fold_mag_f32, spectra_f32): a call of libspecan_fold.so, which takes
# no handle and is no row of the tables above -- the float chain's own call writes the magnitudes it reads
FOLD_GROUPS, FOLD_BUCKETS = frames.FOLD_GROUPS, frames.FOLD_BUCKETS         # 1 .. 128 and 1 .. 64: the mirror's, defined once
_HARM_WORDS = reductions.HARM_WORDS


def output_spec(chain: _Chain, out_kind: Optional[str], B: int) -> tuple:
    """``(shape, dtype)`` of the output of a process call on ``B`` frames (no handle, no GPU)."""
    _, frame, dtype, _ = chain.output(out_kind)
    return (chain.rows(out_kind, B),) + frame, dtype


def _sized_export(fn, head: tuple, dtype, what: str) -> np.ndarray:
    """The exports that are called twice: ``fn(*head, NULL, 0)`` returns the number of elements (negative: an error code),
    ``fn(*head, out, n)`` fills them."""
    n = fn(*head, None, 0)
    if n < 0:
        raise SpecanError(n, what)
    out = np.zeros(n, dtype)
    fn(*head, out.ctypes.data_as(fn.argtypes[-2]), n)
    return out


def _command_buffer(data: bytes):
    return (C.c_uint8 * len(data)).from_buffer_copy(bytes(data)) if len(data) else (C.c_uint8 * 1)()


class SpectrumChain(reductions.Reductions, holds.Holds):
    """One handle = one (GPU, stream) instance of window -> IIR -> 16K FFT.

    Not thread-safe (same rule as the C ABI).  All process calls are asynchronous on the current
    torch stream of the handle's device.

    Overlap mode (:meth:`set_overlap` with depth d > 1): a call runs on an internal stream of the library that torch's
    caching allocator knows nothing about, and the C contract lends the call's input and output tensors to the library
    until d-1 further calls have been made or :meth:`flush` is called.  The wrapper therefore keeps a reference to the
    tensors of the last d-1 calls (a temporary passed as input, or a result that is dropped, would otherwise be
    recycled by the allocator under the running kernel) and releases them at the join, in :meth:`flush` and in
    :meth:`set_overlap`.  A result returned by a process call in this mode holds valid data on the current stream
    only after those d-1 further calls or after :meth:`flush`.
    """

    def __init__(self, device: Optional[int | torch.device | str] = None):
        self._lib = abi.lib()
        if device is None:
            dev = torch.cuda.current_device() if torch.cuda.is_available() else 0
        else:
            d = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
            dev = d.index if d.index is not None else 0
        self.device = torch.device("cuda", dev)
        h = C.c_void_p()
        rc = self._lib.sa_create(dev, C.byref(h))
        if rc != abi.SA_OK:
            raise SpecanError(rc, self._lib.sa_last_error(None).decode())
        self._h = h
        self.control_generation = 0        # bumped by every call that changes what the path computes (virtual_fpga.py)
        self._depth = 1                    # launches in flight (sa_set_overlap)
        self._lent = collections.deque()   # (input, output) of the overlapped calls the caller's stream has not joined
        self._fold_work = None             # float32 [B,16384] of the largest spectra_f32 call made without `work`

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int):
        if rc != abi.SA_OK:
            raise SpecanError(rc, self._lib.sa_last_error(self._h).decode())

    def _ctl(self, rc: int):
        """_check for the calls that change what the path computes: virtual_fpga.py drops frames computed ahead."""
        self._check(rc)
        self.control_generation += 1

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sa_destroy(self._h)        # waits on the host for the handle's own work
            self._h = None
            self._lent.clear()
            self._fold_work = None

    def _lend(self, x: torch.Tensor, out: torch.Tensor):
        """Overlap mode: the call just made owns (x, out) until depth-1 further calls have been made."""
        if self._depth > 1:
            self._lent.append((x, out))
            while len(self._lent) > self._depth - 1:   # this call enqueued the join of the call made depth-1 calls ago
                self._lent.popleft()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check_in(self, x: torch.Tensor, dtype: torch.dtype, row, hop: Optional[int] = None) -> int:
        """The number of frames in ``x``: its rows (of length ``row``, or of that shape where it is a tuple), or with ``hop``
        the frames of `row` elements that the 1-D stream holds row * hop / 16384 elements apart."""
        if not isinstance(x, torch.Tensor) or x.dtype != dtype:
            raise SpecanError(abi.SA_EINVAL, f"input must be a {dtype} tensor")
        if x.device != self.device:
            raise SpecanError(abi.SA_EINVAL, f"input must live on {self.device}")
        if hop is not None:
            step = row * hop // SA_N
            if x.dim() != 1 or not x.is_contiguous() or x.shape[0] < row or (x.shape[0] - row) % step:
                raise SpecanError(abi.SA_ESHAPE, f"with hop={hop} the input must be a contiguous 1-D stream of "
                                                 f"{row} + k * {step} elements")
            return (x.shape[0] - row) // step + 1
        shape = row if isinstance(row, tuple) else (row,)
        if x.dim() != 1 + len(shape) or tuple(x.shape[1:]) != shape or not x.is_contiguous():
            raise SpecanError(abi.SA_ESHAPE, f"input must be a contiguous [B, {', '.join(map(str, shape))}] tensor")
        return x.shape[0]

    def _form_in(self, x, forms: dict, hop: Optional[int] = None) -> tuple:
        """``(number of frames in x, the calls of its input form)``: ``x`` by its dtype among ``forms``, checked as
        :meth:`_check_in` does; what is no tensor of a listed dtype is refused in the name of the first."""
        dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype in forms else next(iter(forms))
        row, calls = forms[dtype]
        return self._check_in(x, dtype, row, hop), calls

    def _float_frames(self, x) -> int:
        """The number of frames in ``x``, an input of :meth:`process_f32` (float32, int16 or packed uint8), or its refusal:
        the input check of every reduction that runs the float chain first."""
        return self._form_in(x, FLOAT_CHAIN.inputs)[0]

    def _process(self, chain: _Chain, x, out, out_kind, scale=None, hop=None):
        """Every process call: ``x`` by its dtype to the chain's entry point for it, into ``out`` (allocated when None).
        ``hop``: ``x`` is one sample stream and the frames are cut from it on the device (the chain's ``streams``)."""
        code, frame, dt, per_row = chain.output(out_kind)
        forms = chain.inputs
        if hop is not None:
            if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or not 8 <= hop <= SA_N or hop % 8:
                raise SpecanError(abi.SA_EINVAL, "hop must be an int, a multiple of 8 in 8..16384")
            hop, forms = int(hop), chain.streams
        B, calls = self._form_in(x, forms, hop)
        shape = (chain.rows(out_kind, B),) + frame
        if out is None:
            out = torch.empty(shape, dtype=dt, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != dt or out.device != self.device or not out.is_contiguous():
            raise SpecanError(abi.SA_ESHAPE, f"out must be a contiguous {dt} tensor of shape {shape}")
        name, takes_scale, takes_kind = calls[out_kind]
        if takes_kind:                     # the kind word, which carries the hop
            tail = (abi.SA_Q15_HOP_KIND(code, hop or 0),)
        else:                              # nothing, or the ints of _EXT_ARGS
            tail = tuple({"log2a": per_row.bit_length() - 1, "hop": hop or 0}[k] for k in _EXT_ARGS.get(name, ()))
        args = (self._h, x.data_ptr()) + ((float(scale),) if takes_scale else ()) + (out.data_ptr(), B) + tail
        self._check(getattr(self._lib, name)(*args, self._stream()))
        self._lend(x, out)
        return out

    # ------------------------------------------------------------------ control plane
    def set_filter_mode(self, cmd: int):
        """0x00 default / 0xA1 custom / 0xB1 none (new/command_control.vhd:53-58); 0xA2 wide."""
        if not 0 <= int(cmd) <= 255:
            raise SpecanError(abi.SA_EINVAL, "filter command must be one byte")
        self._ctl(self._lib.sa_set_filter_mode(self._h, int(cmd)))

    @property
    def filter_mode(self) -> int:
        v = C.c_uint8()
        self._check(self._lib.sa_get_filter_mode(self._h, C.byref(v)))
        return v.value

    def load_coeffs_q7(self, coeffs: Sequence[int]):
        """12 int8 in wire order [b0,b1,b2,a0,a1,a2] x 2 (gui.py:598-605)."""
        a = np.asarray(coeffs).reshape(-1)
        if a.size != 12:
            raise SpecanError(abi.SA_EINVAL, "expected 12 coefficients (2 sections x 6)")
        a = a.astype(np.int64)
        if a.min() < -128 or a.max() > 127:
            raise SpecanError(abi.SA_EINVAL, "coefficients must fit int8")
        a8 = np.ascontiguousarray(a.astype(np.int8))
        self._ctl(self._lib.sa_load_coeffs_q7(self._h, a8.ctypes.data_as(C.POINTER(C.c_int8))))

    def coeffs_q7(self) -> np.ndarray:
        a = np.zeros(12, np.int8)
        self._check(self._lib.sa_get_coeffs_q7(self._h, a.ctypes.data_as(C.POINTER(C.c_int8))))
        return a

    def feed_command_bytes(self, data: bytes) -> int:
        """Push raw UART bytes through the RX state machine; returns the number of UART read requests
        (0xA5, imp/sequ2.vhd:216) seen outside coefficient uploads."""
        n = C.c_int(0)
        self._ctl(self._lib.sa_feed_command_bytes(self._h, _command_buffer(data), len(data), C.byref(n)))
        return n.value

    def feed_command_bytes_ex(self, data: bytes) -> "abi.CmdEvents":
        """The same, reporting everything a transport shim needs (sa_cmd_events of include/specan.h)."""
        ev = abi.CmdEvents()
        self._check(self._lib.sa_feed_command_bytes_ex(self._h, _command_buffer(data), len(data), C.byref(ev)))
        if ev.control_changed:
            self.control_generation += 1
        return ev

    @property
    def transport(self) -> int:
        """0xEF (Ethernet, the reset state: imp/sequ2.vhd:85-86) or 0xFE (UART)."""
        v = C.c_uint8()
        self._check(self._lib.sa_get_transport(self._h, C.byref(v)))
        return v.value

    def send_filter_coefficients(self, quantized_sections) -> bytes:
        """Same wire bytes as UartReceiver.send_filter_coefficients (gui.py:591-613): 0xF1 then the
        12 coefficients of exactly two sections, each ``int(c) & 0xFF``.  Returns the bytes sent."""
        secs = [list(s) for s in quantized_sections]
        if len(secs) != 2 or any(len(s) != 6 for s in secs):
            raise SpecanError(abi.SA_EINVAL, "exactly two sections of six coefficients (gui.py:1186-1192)")
        payload = bytes([FILTER_UPDATE_CMD]) + bytes(int(c) & 0xFF for s in secs for c in s)
        self.feed_command_bytes(payload)
        return payload

    def load_sos(self, sos):
        """Wide float format: up to 6 sections, scipy rows [b0,b1,b2,a0,a1,a2] (float64)."""
        s = np.ascontiguousarray(np.asarray(sos, np.float64).reshape(-1, 6))
        self._ctl(self._lib.sa_load_sos_f64(self._h, s.ctypes.data_as(C.POINTER(C.c_double)), s.shape[0]))

    def load_sos_f32(self, sos):
        s = np.ascontiguousarray(np.asarray(sos, np.float32).reshape(-1, 6))
        self._ctl(self._lib.sa_load_sos_f32(self._h, s.ctypes.data_as(C.POINTER(C.c_float)), s.shape[0]))

    def load_sos_q14(self, sos_q14):
        s = np.ascontiguousarray(np.asarray(sos_q14, np.int16).reshape(-1, 6))
        self._ctl(self._lib.sa_load_sos_q14(self._h, s.ctypes.data_as(C.POINTER(C.c_int16)), s.shape[0]))

    def set_window_q15(self, rom: Optional[np.ndarray]):
        if rom is None:
            self._ctl(self._lib.sa_set_window_q15(self._h, None))
            return
        r = np.ascontiguousarray(rom, np.int16)
        if r.shape != (SA_N,):
            raise SpecanError(abi.SA_ESHAPE, "window ROM must have 16384 entries")
        self._ctl(self._lib.sa_set_window_q15(self._h, r.ctypes.data_as(C.POINTER(C.c_int16))))

    def window_q15(self) -> np.ndarray:
        r = np.zeros(SA_N, np.int16)
        self._check(self._lib.sa_get_window_q15(self._h, r.ctypes.data_as(C.POINTER(C.c_int16))))
        return r

    def set_window_f32(self, w: Optional[np.ndarray]):
        if w is None:
            self._ctl(self._lib.sa_set_window_f32(self._h, None))
            return
        a = np.ascontiguousarray(w, np.float32)
        if a.shape != (SA_N,):
            raise SpecanError(abi.SA_ESHAPE, "window must have 16384 entries")
        self._ctl(self._lib.sa_set_window_f32(self._h, a.ctypes.data_as(C.POINTER(C.c_float))))

    def set_window_mode_q15(self, mode: int):
        self._ctl(self._lib.sa_set_window_mode_q15(self._h, int(mode)))

    def reserve(self, max_batch: int):
        self._check(self._lib.sa_reserve(self._h, int(max_batch)))

    def set_overlap(self, depth: int):
        """Opt-in overlapped launches (include/specan.h, sa_set_overlap): with depth d > 1 the results of a
        process call are visible on the current stream after d-1 further calls or after :meth:`flush`, and the
        call's input and output tensors belong to the library until then (the wrapper holds them: class docstring).
        1 = strictly stream-ordered."""
        self._check(self._lib.sa_set_overlap(self._h, int(depth)))
        if int(depth) != self._depth:            # a change of depth waited on the host for everything in flight;
            self._depth = int(depth)             # the same depth returns at once, with the lent tensors still in use
            self._lent.clear()

    @property
    def overlap(self) -> int:
        v = C.c_int()
        self._check(self._lib.sa_get_overlap(self._h, C.byref(v)))
        return v.value

    def overlap_streams_side_by_side(self) -> bool:
        """Tests: re-run the library's probe on the handle's internal streams and the current stream
        (sa_debug_overlap_streams)."""
        v = C.c_int()
        self._check(self._lib.sa_debug_overlap_streams(self._h, self._stream(), C.byref(v)))
        return bool(v.value)

    def flush(self):
        """Make the current stream wait for every outstanding overlapped call (no host wait)."""
        self._check(self._lib.sa_flush(self._h, self._stream()))
        self._lent.clear()

    def set_profiling(self, ring: int):
        """Launch timing (include/specan.h, sa_set_profiling): keep the device times of the last ``ring`` stream-ordered
        process calls (0 = off).  The events ride on the dispatch packets; a train of calls runs as it does untimed."""
        self._check(self._lib.sa_set_profiling(self._h, int(ring)))

    def profile_read(self, n: int) -> list:
        """Device time in ms of up to ``n`` of the most recent timed calls, oldest first (waits for them)."""
        buf = (C.c_float * max(1, int(n)))()
        got = self._lib.sa_profile_read(self._h, buf, int(n))
        if got < 0:
            self._check(got)
        return [float(buf[i]) for i in range(got)]

    def iir_plan(self) -> np.ndarray:
        return _sized_export(self._lib.sa_debug_iir_plan_f32, (self._h,), np.float32, "sa_debug_iir_plan_f32")

    def set_precision(self, precision: str):
        """'f32' (the default) or 'f64': window, inter-section signal and cascade of the float path in float64
        (include/specan.h, sa_set_precision).  Applies to later :meth:`process_f32` calls in filter modes 0x00 and 0xA1."""
        if precision not in _PRECISIONS:
            raise SpecanError(abi.SA_EINVAL, f"precision must be one of {sorted(_PRECISIONS)}")
        self._ctl(self._lib.sa_set_precision(self._h, _PRECISIONS[precision]))

    @property
    def precision(self) -> str:
        v = C.c_int()
        self._check(self._lib.sa_get_precision(self._h, C.byref(v)))
        return {code: name for name, code in _PRECISIONS.items()}[v.value]

    def iir_plan_f64(self) -> np.ndarray:
        """The float64 plan the handle would launch in its current filter mode (sa_debug_iir_plan_f64)."""
        return _sized_export(self._lib.sa_debug_iir_plan_f64, (self._h,), np.float64, "sa_debug_iir_plan_f64")

    def set_marker_range(self, lo: int, hi: int):
        """The full-spectrum bins [lo, hi) that ``out_kind='marker'`` covers (include/specan.h, sa_set_marker_range):
        0 <= lo < hi <= 16384, [0, 16384) by default.  frames.bin_range_from_permille maps the gui's per-mille range.
        Stream-ordered; the 0xFF reset leaves it alone."""
        self._ctl(self._lib.sa_set_marker_range(self._h, int(lo), int(hi)))

    @property
    def marker_range(self) -> tuple:
        lo, hi = C.c_int(), C.c_int()
        self._check(self._lib.sa_get_marker_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    # ------------------------------------------------------------------ data plane
    def process_f32(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, out_kind: str = "mag_full",
                    scale: float = 1.0 / 2048.0):
        """[B,16384] float32 -> per ``out_kind``: 'mag_full' [B,16384] f32, 'mag_half' [B,8193] f32,
        'spec_half' [B,8193] complex64, 'time' [B,16384] f32, 'marker' [B,4] int32 (one sa_marker per frame:
        peak_mag as float32 bits, peak_bin, band_power as float32 bits, 0; see :meth:`markers`).

        An int16 tensor (the ADC's samples, what the ingest front-end delivers) takes the same float path through
        sa_process_f32_i16: x = float(sample) * ``scale``, rounded once, no conversion pass; ``scale`` is ignored for
        float32 input.

        A uint8 tensor [B,24576] holds the same samples packed to 12 bits, two samples in three bytes (include/specan.h,
        "p12"; ingest.pack12 is the host packer): it goes to sa_process_f32_p12, is unpacked in the stage-in and gives
        the results of the int16 tensor of the same samples bit for bit, from three quarters of the input bytes.  Its
        data pointer must be 16-byte aligned (any tensor torch allocates is, and so is every whole-frame slice of one).

        Pointer contract (include/specan.h; checked by the C entry point, SA_EINVAL): the data pointer of ``x`` is 16-byte
        aligned, and so is that of ``out`` except for 'mag_half' (4 bytes) and 'spec_half' (8 bytes), which are aligned to
        their element: every row slice ``big[a:a+B]`` of such a tensor is a valid ``out``.  The bytes read through ``x``
        and the bytes written through ``out`` are disjoint: no call works in place (``out=x``); buffers that merely touch
        are fine.  A contiguous view that starts one element into a buffer is not aligned."""
        return self._process(FLOAT_CHAIN, x, out, out_kind, scale)

    def markers(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, scale: float = 1.0 / 2048.0):
        """Peak search and band power over the marker range, per frame: ``(peak_mag float32 [B], peak_bin int32 [B],
        band_power float32 [B])``, views of the [B,4] int32 record tensor (``out``, allocated when None) that
        ``process_f32(x, out, 'marker', scale)`` fills.  peak_mag is the 'mag_full' value at peak_bin, bit for bit.
        ``x`` is float32, int16 or packed uint8 as for :meth:`process_f32`."""
        rec = self.process_f32(x, out, out_kind="marker", scale=scale)
        f = rec.view(torch.float32)
        return f[:, 0], rec[:, 1], f[:, 2]

    def process_q15(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, out_kind: str = "iq",
                    hop: Optional[int] = None) -> torch.Tensor:
        """[B,16384] int16 -> per ``out_kind``: 'iq' (the default) [B,16384,2] int16 (re, im), B frames of 65536 bytes;
        'mag' [B,16384] float32, frames.decode_mag_16iq_le of each of those frames bit for bit (gui.py:250-260);
        'marker' [B,4] int32, one sa_marker_q15 per frame over the marker range (peak_mag as float32 bits, peak_bin,
        band_power as the two halves of an int64; see :meth:`markers_q15`).

        A uint8 tensor [B,24576] holds the same samples packed to 12 bits (include/specan.h, "p12"; ingest.pack12 is the
        host packer): it goes to sa_process_q15_p12, is unpacked inside the kernels that read the samples and gives the
        results of the int16 tensor of the same samples bit for bit, from three quarters of the input bytes.  Its data
        pointer must be 16-byte aligned (any tensor torch allocates is, and so is every whole-frame slice of one).

        ``hop`` (a multiple of 8 in 8..16384; include/specan.h, SA_Q15_HOP_KIND): overlapping frames cut on the device.
        ``x`` is then ONE 1-D stream -- (B-1) * hop + 16384 int16 samples, or 3/2 as many packed bytes -- frame b is its
        samples [b * hop, b * hop + 16384), and the result is that of the plain call on those B frames copied out
        (``ingest.FrameCutter(hop)``), bit for bit, with every sample sent to the device once (``ingest.StreamCutter`` cuts
        such streams).  The data pointer must be 16-byte aligned for both dtypes.  ``hop=None`` is the call on frames.

        Pointer contract (include/specan.h; checked by the C entry point, SA_EINVAL): the data pointers of ``x`` and of
        ``out`` are 16-byte aligned for every ``out_kind``, and the bytes read through ``x`` -- with ``hop`` the stream, not
        B whole frames -- and the bytes written through ``out`` are disjoint; buffers that merely touch are fine."""
        return self._process(Q15_CHAIN, x, out, out_kind, hop=hop)

    def markers_q15(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, hop: Optional[int] = None):
        """Peak search and band power of the integer chain's frames over the marker range: ``(peak_mag float32 [B],
        peak_bin int32 [B], band_power int64 [B])``, views of the [B,4] int32 record tensor (``out``, allocated when
        None) that ``process_q15(x, out, 'marker')`` fills.  peak_mag is the 'mag' value at peak_bin, bit for bit, and
        band_power the exact integer sum of re^2 + im^2 over the range.  ``x`` is int16 or packed uint8 as for
        :meth:`process_q15`, and with ``hop`` a 1-D stream as there."""
        rec = self.process_q15(x, out, out_kind="marker", hop=hop)
        return rec.view(torch.float32)[:, 0], rec[:, 1], rec.view(torch.int64)[:, 1]

    def traces_q15(self, x: torch.Tensor, bucket: int = 16, out: Optional[torch.Tensor] = None,
                   hop: Optional[int] = None, group: Optional[int] = None) -> torch.Tensor:
        """The display trace of the integer chain's frames: [B, 16384 // bucket, 2] float32, one sa_trace_point_q15 per
        bucket of ``bucket`` consecutive bins of the full spectrum (include/specan.h, SA_Q15_TRACE_KIND).  ``[..., 0]`` is
        the peak, the largest 'mag' value of the bucket bit for bit; ``[..., 1]`` the power, the exact integer sum of
        re^2 + im^2 over the bucket rounded once to float32 (frames.trace_of_frame is the numpy mirror).  ``bucket`` is
        2, 4, 8, 16, 32 or 64 -- anything else is SA_EINVAL before any device call; the marker range plays no part.
        ``x`` is int16 or packed uint8 as for :meth:`process_q15`, and with ``hop`` a 1-D stream as there.

        ``group=A`` (2, 4, ..., 128; include/specan.h, SA_Q15_TRACE_AVG_KIND) reduces groups of A consecutive frames as well:
        [B // A, 16384 // bucket, 2] float32, record (g, j) over the bucket j of the frames gA .. gA + A - 1 -- with ``hop``
        the frames of the stream.  ``[..., 0]`` is the largest of the A frames' peaks, bit for bit (max hold); ``[..., 1]``
        the exact integer sum of re^2 + im^2 over bucket x A frames (at most 2^44), rounded once to float32.  It is the
        SUM: the mean is ``power / A``, exactly.  frames.trace_of_frames is the numpy mirror.  Any other ``group`` (a
        bool or a float included) is SA_EINVAL, a B that is no multiple of A SA_ESHAPE, both before any device call.
        The call keeps B * (16384 // bucket) * 16 bytes of workspace in the handle, grown by the call itself and never by
        :meth:`reserve`: before capturing such a call into a graph, make one of the same bucket and batch outside it
        (SA_ESTATE otherwise).  ``group=None`` is the call on single frames."""
        if isinstance(bucket, bool) or not isinstance(bucket, (int, np.integer)) or int(bucket) not in _TRACE_OUT:
            raise SpecanError(abi.SA_EINVAL, f"bucket must be one of {sorted(_TRACE_OUT)}")
        if group is None:
            return self._process(Q15_TRACE_CHAIN, x, out, int(bucket), hop=hop)
        self._log2_group(group)
        return self._process(Q15_TRACE_AVG_CHAIN, x, out, (int(bucket), int(group)), hop=hop)

    @staticmethod
    def _log2_group(group) -> int:
        """The one validation of a ``group`` argument: a of A = 2^a, or SA_EINVAL."""
        if isinstance(group, bool) or not isinstance(group, (int, np.integer)) or int(group) not in TRACE_GROUPS:
            raise SpecanError(abi.SA_EINVAL, f"group must be one of {TRACE_GROUPS}")
        return int(group).bit_length() - 1

    def spectra_q15(self, x: torch.Tensor, group: int, out: Optional[torch.Tensor] = None,
                    hop: Optional[int] = None) -> torch.Tensor:
        """Max hold and summed power of the integer chain's frames over groups of ``group`` consecutive frames, at the full
        resolution of 16384 bins: [B // group, 16384, 2] float32, one sa_trace_point_q15 per bin and group
        (include/specan_ext.h, sa_spectra_q15).  ``[..., 0]`` is the largest 'mag' value of the bin over the group's frames,
        bit for bit; ``[..., 1]`` the exact integer sum of re^2 + im^2 over them (at most 2^38) rounded once to float32.  It
        is the SUM: the mean is ``power / group``, exactly -- a Welch estimate where the frames overlap (``hop``).
        frames.spectrum_of_frames is the numpy mirror of one row; the marker range plays no part.

        ``group`` is 2, 4, ..., 128; anything else (a bool or a float included) is SA_EINVAL, a B that is no multiple of it
        SA_ESHAPE, both before any device call.  ``x`` is int16 or packed uint8 as for :meth:`process_q15`, and with ``hop``
        a 1-D stream as there.  The call is :meth:`process_q15` ``(out_kind='iq')`` into a workspace of the handle, 64 KiB
        per frame, and one more launch that folds it; the workspace is grown by the call itself and never by
        :meth:`reserve`: before capturing such a call into a graph, make one of the same batch outside it (SA_ESTATE
        otherwise).  The pointer contract is that of :meth:`process_q15`, on (B // group) * 131072 bytes written."""
        self._log2_group(group)
        return self._process(Q15_SPECTRA_CHAIN, x, out, int(group), hop=hop)

    def fold_iq_q15(self, iq: torch.Tensor, group: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The fold of :meth:`spectra_q15` alone, on frames the caller already has: ``iq`` is an int16 [B,16384,2] device
        tensor, the result of ``process_q15(out_kind='iq')`` (include/specan_ext.h, sa_fold_iq_q15); the result is
        [B // group, 16384, 2] float32 as there.  One launch, no workspace: it captures into a graph at any time."""
        self._log2_group(group)
        return self._process(Q15_FOLD_CHAIN, iq, out, int(group))

    def filter_q15(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Window (+ integer IIR) only: the FFT input stream, [B,16384] int16.  ``x`` is [B,16384] int16 or the same
        samples packed, [B,24576] uint8 (sa_filter_q15_p12), as for :meth:`process_q15`.

        Pointer contract (include/specan.h; checked by the C entry point, SA_EINVAL): the data pointers of ``x`` and of
        ``out`` are 16-byte aligned, and the bytes read through ``x`` and written through ``out`` are disjoint: the call
        does not work in place (``out=x``), although the sizes would match; buffers that merely touch are fine."""
        return self._process(Q15_WINDOW_CHAIN, x, out, None)

    def frames_bytes(self, iq: torch.Tensor) -> list[bytes]:
        """Device IQ tensor -> list of 65536-byte frames exactly as sequ2 emits them.  In overlap mode the current
        stream first joins the outstanding calls (the tensor may be the result of one of them)."""
        if self._depth > 1:
            self.flush()
        host = iq.detach().to("cpu").contiguous().numpy().astype("<i2", copy=False)
        return [host[i].tobytes() for i in range(host.shape[0])]


def iir_plan_from_sos(sos) -> np.ndarray:
    """Host-only: the float IIR plan (no GPU needed); see include/specan.h sa_iir_plan_from_sos."""
    s = np.ascontiguousarray(np.asarray(sos, np.float64).reshape(-1, 6))
    return _sized_export(abi.lib().sa_iir_plan_from_sos, (s.ctypes.data_as(C.POINTER(C.c_double)), s.shape[0]), np.float32,
                         "sa_iir_plan_from_sos: bad SOS")


def iir_plan_f64_from_sos(sos) -> np.ndarray:
    """Host-only: the float64-state plan (no GPU needed); see include/specan.h sa_iir_plan_from_sos_f64."""
    s = np.ascontiguousarray(np.asarray(sos, np.float64).reshape(-1, 6))
    return _sized_export(abi.lib().sa_iir_plan_from_sos_f64, (s.ctypes.data_as(C.POINTER(C.c_double)), s.shape[0]), np.float64,
                         "sa_iir_plan_from_sos_f64: bad SOS")


def pack_frame(iq_host: np.ndarray) -> bytes:
    L = abi.lib()
    a = np.ascontiguousarray(iq_host, np.int16).reshape(SA_N, 2)
    buf = (C.c_uint8 * FRAME_SIZE_BYTES)()
    rc = L.sa_pack_frame(a.ctypes.data_as(C.POINTER(C.c_int16)), buf)
    if rc != abi.SA_OK:
        raise SpecanError(rc, "sa_pack_frame")
    return bytes(buf)
