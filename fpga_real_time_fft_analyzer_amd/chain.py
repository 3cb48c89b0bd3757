"""Host-side mirror of the reference's signal-path contract, over the C ABI.

``SpectrumChain`` is the "virtual FPGA" seen from the host: it takes the same command bytes
(scripts/fft_analyzer_gui.py:28-37), the same ``0xF1`` + 12 x int8 coefficient upload
(gui.py:591-613 -> new/rx_filter_coeff.vhd:41-66) and produces the same 65536-byte frames
(imp/sequ2.vhd:153, gui.py:250-260) -- batched over thousands of frames resident in HBM.
PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import abi, frames
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
# find_peaks(field=...) -> the `field` of include/specan_peaks.h: plain magnitudes, or one float of (peak, power) records
_PEAK_FIELDS = {None: abi.SA_PEAKS_IN_MAG, "peak": abi.SA_PEAKS_IN_POINT_PEAK, "power": abi.SA_PEAKS_IN_POINT_POWER}
# order_stats(field=...) -> the `field` of include/specan_rank.h: the same three layouts
_RANK_FIELDS = {None: abi.SA_RANK_IN_MAG, "peak": abi.SA_RANK_IN_POINT_PEAK, "power": abi.SA_RANK_IN_POINT_POWER}
# band_power(field=...) -> the `field` of include/specan_bands.h: the same three layouts
_BANDS_FIELDS = {None: abi.SA_BANDS_IN_MAG, "peak": abi.SA_BANDS_IN_POINT_PEAK, "power": abi.SA_BANDS_IN_POINT_POWER}
# mask_test(field=...) -> the `field` of include/specan_mask.h: the same three layouts
_MASK_FIELDS = {None: abi.SA_MASK_IN_MAG, "peak": abi.SA_MASK_IN_POINT_PEAK, "power": abi.SA_MASK_IN_POINT_POWER}
# harmonics(field=...) -> the `field` of include/specan_harm.h: the same three layouts
_HARM_FIELDS = {None: abi.SA_HARM_IN_MAG, "peak": abi.SA_HARM_IN_POINT_PEAK, "power": abi.SA_HARM_IN_POINT_POWER}
_HARM_WORDS = C.sizeof(abi.HarmRow) // 4                                      # an sa_harm_row as int32 words: 42


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


class SpectrumChain:
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

    def _process(self, chain: _Chain, x, out, out_kind, scale=None, hop=None):
        """Every process call: ``x`` by its dtype to the chain's entry point for it, into ``out`` (allocated when None).
        ``hop``: ``x`` is one sample stream and the frames are cut from it on the device (the chain's ``streams``)."""
        code, frame, dt, per_row = chain.output(out_kind)
        forms = chain.inputs
        if hop is not None:
            if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or not 8 <= hop <= SA_N or hop % 8:
                raise SpecanError(abi.SA_EINVAL, "hop must be an int, a multiple of 8 in 8..16384")
            hop, forms = int(hop), chain.streams
        dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype in forms else next(iter(forms))
        row, calls = forms[dtype]
        B = self._check_in(x, dtype, row, hop)
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

    @staticmethod
    def _log2_fold(group, bucket) -> tuple:
        """The one validation of the ``group`` and ``bucket`` of the float fold: (a, k) of A = 2^a and W = 2^k, or SA_EINVAL."""
        for name, v, allowed in (("group", group, FOLD_GROUPS), ("bucket", bucket, FOLD_BUCKETS)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) not in allowed:
                raise SpecanError(abi.SA_EINVAL, f"{name} must be one of {allowed}")
        if int(group) == 1 and int(bucket) == 1:
            raise SpecanError(abi.SA_EINVAL, "group = bucket = 1 folds nothing")
        return int(group).bit_length() - 1, int(bucket).bit_length() - 1

    def _fold_out(self, B: int, group: int, bucket: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``out`` of the float fold of ``B`` frames, allocated when None: SA_ESHAPE where B is no multiple of the group or
        ``out`` is not the contiguous float32 [B // group, 16384 // bucket, 2] tensor on the handle's device."""
        if B % group:
            raise SpecanError(abi.SA_ESHAPE, f"the batch ({B} frames) must be a multiple of {group}")
        shape = (B // group, SA_N // bucket, 2)
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32
                or out.device != self.device or not out.is_contiguous()):
            raise SpecanError(abi.SA_ESHAPE, f"out must be a contiguous torch.float32 tensor of shape {shape}")
        return out

    def fold_mag_f32(self, mag: torch.Tensor, group: int = 1, bucket: int = 1,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Max hold and summed power of float32 magnitudes over groups of ``group`` consecutive frames and buckets of
        ``bucket`` adjacent bins (include/specan_fold.h, sa_fold_mag_f32): ``mag`` is a float32 [B,16384] device tensor, what
        ``process_f32(out_kind='mag_full')`` or ``process_q15(out_kind='mag')`` wrote; the result is float32
        [B // group, 16384 // bucket, 2], one sa_fold_point per bucket and group.  ``[..., 0]`` is the peak: the input whose
        bits with the sign cleared are largest as an integer -- the float maximum of the chain's non-negative values, bit for
        bit; a NaN shows, -0.0 reads as +0.0, no denormal is flushed.  ``[..., 1]`` is the power: the float64 sum of the exact
        squares, per bin over the frames in ascending order and then across the bucket's bins by a balanced pair tree,
        rounded once to float32.  It is the SUM: the mean is ``power / (group * bucket)``, exactly.  frames.fold_of_mags is
        the numpy mirror, bit for bit.

        ``group`` is 1, 2, ..., 128 and ``bucket`` 1, 2, ..., 64, not both 1; anything else (a bool or a float included) is
        SA_EINVAL, a B that is no multiple of ``group`` SA_ESHAPE, both before any device call.  One launch on the current
        stream of the handle's device, no handle state, no workspace: it captures into a graph at any time.  Where ``mag`` is
        the result of a call made in overlap mode, call :meth:`flush` first.  Pointer contract (checked by the C entry
        point, SA_EINVAL): both data pointers are 16-byte aligned and the B * 65536 bytes read and the
        (B // group) * (16384 // bucket) * 8 bytes written are disjoint; buffers that merely touch are fine."""
        a, k = self._log2_fold(group, bucket)
        B = self._check_in(mag, torch.float32, SA_N)
        out = self._fold_out(B, int(group), int(bucket), out)
        L = abi.fold_lib()
        with torch.cuda.device(self.device):         # the C call launches on the calling thread's current device
            rc = L.sa_fold_mag_f32(mag.data_ptr(), out.data_ptr(), B, a, k, self._stream())
        if rc != abi.SA_OK:
            raise SpecanError(rc, L.sa_fold_last_error().decode())
        return out

    def spectra_f32(self, x: torch.Tensor, group: int, bucket: int = 1, out: Optional[torch.Tensor] = None,
                    scale: float = 1.0 / 2048.0, work: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Max hold and summed power of the float chain's spectra over groups of ``group`` consecutive frames and buckets of
        ``bucket`` adjacent bins: float32 [B // group, 16384 // bucket, 2], the records of :meth:`fold_mag_f32` of
        ``process_f32(x, out_kind='mag_full', scale=scale)``, bit for bit -- the input of a Welch estimate (``[..., 1] /
        group``) or a max-hold display, from (2 / (group * bucket)) of the full spectrum's bytes.  ``x`` is float32, int16 or
        packed uint8 exactly as for :meth:`process_f32`; every filter mode and both precisions apply, because the call is
        that call, unchanged, into a float32 [B,16384] workspace, followed by one fold launch on the current stream.

        The workspace is ``work`` (float32, contiguous, [B,16384] or more rows, on the handle's device; 16-byte aligned),
        or, when None, a tensor cached on this object and regrown when B grows: allocate it by one call of the largest batch
        before capturing the call into a graph, and give calls made on different streams a ``work`` each.  In overlap mode
        (:meth:`set_overlap` with depth > 1) the call joins every outstanding call of the handle on the device, as
        :meth:`flush` does and with no host wait, between its two launches: the result is valid on the current stream when
        the call returns, and ``x`` and the workspace are free again then -- the call lends nothing.  ``group``, ``bucket``,
        ``out`` and a B that is no multiple of ``group`` are refused as by :meth:`fold_mag_f32`, before anything is
        launched."""
        self._log2_fold(group, bucket)
        forms = FLOAT_CHAIN.inputs
        dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype in forms else next(iter(forms))
        B = self._check_in(x, dtype, forms[dtype][0])
        out = self._fold_out(B, int(group), int(bucket), out)
        mag = self._mag_full_in_work(x, B, scale, work)
        return self.fold_mag_f32(mag, group, bucket, out)

    def _mag_full_in_work(self, x: torch.Tensor, B: int, scale: float, work: Optional[torch.Tensor]) -> torch.Tensor:
        """``process_f32(x, 'mag_full')`` of B frames into ``work`` or, when None, the cached workspace (regrown when B grows),
        joined with the current stream where overlap is on: what :meth:`spectra_f32` and :meth:`peak_table_f32` reduce."""
        if work is None:
            if self._fold_work is None or self._fold_work.shape[0] < B:
                self._fold_work = None               # released before the larger one is taken
                self._fold_work = torch.empty((B, SA_N), dtype=torch.float32, device=self.device)
            work = self._fold_work
        elif (not isinstance(work, torch.Tensor) or work.dtype != torch.float32 or work.device != self.device or work.dim() != 2
              or work.shape[1] != SA_N or work.shape[0] < B or not work.is_contiguous()):
            raise SpecanError(abi.SA_ESHAPE, f"work must be a contiguous torch.float32 tensor of shape [{B} or more, {SA_N}]")
        mag = self.process_f32(x, out=work[:B], out_kind="mag_full", scale=scale)
        if self._depth > 1:
            self.flush()                             # the reduction reads what an internal stream of the library writes
        return mag

    @staticmethod
    def _peaks_args(k, threshold, lo, hi, min_sep, field) -> int:
        """The one validation of the arguments of the peak table: the ``field`` code of include/specan_peaks.h, or SA_EINVAL."""
        for name, v in (("k", k), ("lo", lo), ("hi", hi), ("min_sep", min_sep)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise SpecanError(abi.SA_EINVAL, f"{name} must be an int")
        if not 1 <= int(k) <= abi.SA_PEAKS_K_MAX:
            raise SpecanError(abi.SA_EINVAL, f"k must be 1..{abi.SA_PEAKS_K_MAX}")
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
            raise SpecanError(abi.SA_EINVAL, "threshold must be a number")
        if int(np.array([threshold], np.float32).view(np.uint32)[0]) > 0x7F800000:
            raise SpecanError(abi.SA_EINVAL, "threshold must be +0.0 .. +inf: no NaN, no sign bit")
        if not 0 <= int(lo) < int(hi) <= SA_N:
            raise SpecanError(abi.SA_EINVAL, f"the range must be 0 <= lo < hi <= {SA_N}")
        if not 1 <= int(min_sep) <= SA_N:
            raise SpecanError(abi.SA_EINVAL, f"min_sep must be 1..{SA_N}")
        if not (field is None or isinstance(field, str)) or field not in _PEAK_FIELDS:
            raise SpecanError(abi.SA_EINVAL, "field must be None, 'peak' or 'power'")
        return _PEAK_FIELDS[field]

    def _peaks_out(self, R: int, k: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``out`` of the peak table of ``R`` rows, allocated when None: SA_ESHAPE where it is not the contiguous int32 [R, k, 2]
        tensor on the handle's device."""
        shape = (R, k, 2)
        if out is None:
            return torch.empty(shape, dtype=torch.int32, device=self.device)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.int32
                or out.device != self.device or not out.is_contiguous()):
            raise SpecanError(abi.SA_ESHAPE, f"out must be a contiguous torch.int32 tensor of shape {shape}")
        return out

    def find_peaks(self, t: torch.Tensor, k: int = 8, threshold: float = 0.0, lo: int = 0, hi: int = SA_N, min_sep: int = 1,
                   field: Optional[str] = None, out: Optional[torch.Tensor] = None) -> tuple:
        """The peak table of each row of ``t`` (include/specan_peaks.h, sa_peaks_f32): the ``k`` strongest local maxima with
        their bins.  ``t`` is a float32 [R,16384] device tensor -- what ``process_f32(out_kind='mag_full')`` or
        ``process_q15(out_kind='mag')`` wrote -- or, with ``field='peak'`` or ``field='power'``, float32 [R,16384,2], the
        records of :meth:`fold_mag_f32` at bucket 1, :meth:`spectra_f32` or :meth:`spectra_q15`, of which that float is the
        point.  Returns ``(mag float32 [R,k], bin int32 [R,k], count int32 [R])``: mag and bin are views of the [R,k,2] int32
        record tensor (``out``, allocated when None; one sa_peak per slot), count is allocated by the call.

        A point's key is its bits with the sign cleared, as an integer: the float order of the chains' non-negative values; a
        NaN shows above +inf, -0.0 reads as +0.0, no denormal is flushed.  Bin i is a candidate when ``lo <= i < hi``, its key
        is not 0 and not below that of ``threshold``, above that of bin i-1 and not below that of bin i+1 (the row's
        neighbours, in the range or not; bins 0 and 16383 lack one, which then agrees): a plateau gives its lowest bin.  The
        candidates are walked by larger key, then lower bin, and one is accepted when it lies ``min_sep`` or more bins from
        every one accepted before; the first ``k`` accepted are the records, in that order, the unused slots (+0.0, -1).
        ``count`` is the number of candidates before suppression and truncation.  frames.peaks_of_rows is the numpy mirror,
        bit for bit.  With k = 1, threshold 0 and the full range the record is (peak_mag, peak_bin) of :meth:`markers` /
        :meth:`markers_q15` on the same frames, wherever that peak is not zero.

        ``k`` is 1..32, ``threshold`` not negative and no NaN, ``0 <= lo < hi <= 16384``, ``min_sep`` 1..16384; k, lo, hi and
        min_sep take ints only (a bool or a float is SA_EINVAL); a wrong dtype is SA_EINVAL and a wrong shape SA_ESHAPE, all
        before any device call.  One launch on the current stream of the handle's device, no handle state, no workspace: it
        captures into a graph at any time (count then lives in the graph's pool, like an ``out`` the call allocates).  Where
        ``t`` is the result of a call made in overlap mode, call :meth:`flush` first.  Pointer contract
        (checked by the C entry point, SA_EINVAL): ``t`` is 16-byte aligned, and the bytes read and the R * k * 8 and R * 4
        bytes written are disjoint; buffers that merely touch are fine."""
        code = self._peaks_args(k, threshold, lo, hi, min_sep, field)
        R = self._check_in(t, torch.float32, (SA_N, 2) if code else SA_N)
        out = self._peaks_out(R, int(k), out)
        count = torch.empty((R,), dtype=torch.int32, device=self.device)
        L = abi.peaks_lib()
        with torch.cuda.device(self.device):         # the C call launches on the calling thread's current device
            rc = L.sa_peaks_f32(t.data_ptr(), code, out.data_ptr(), count.data_ptr(), R, int(k), float(threshold), int(lo),
                                int(hi), int(min_sep), self._stream())
        if rc != abi.SA_OK:
            raise SpecanError(rc, L.sa_peaks_last_error().decode())
        return out.view(torch.float32)[..., 0], out[..., 1], count

    def peak_table_f32(self, x: torch.Tensor, k: int = 8, threshold: float = 0.0, lo: int = 0, hi: int = SA_N,
                       min_sep: int = 1, group: Optional[int] = None, scale: float = 1.0 / 2048.0,
                       work: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> tuple:
        """The peak table of the float chain's spectra, without the spectra leaving the device: ``(mag float32 [R,k], bin
        int32 [R,k], count int32 [R])`` as :meth:`find_peaks` returns them.  ``x`` is float32, int16 or packed uint8 exactly
        as for :meth:`process_f32`; every filter mode and both precisions apply.

        Without ``group`` (R = B) the call is ``process_f32(x, out_kind='mag_full', scale=scale)`` into the workspace of
        :meth:`spectra_f32` followed by :meth:`find_peaks`: the peaks of every frame's magnitudes.  With ``group=A`` (2, 4,
        ..., 128; R = B // A) it is ``spectra_f32(x, group=A, scale=scale, work=work)`` followed by ``find_peaks(...,
        field='power')``: the peaks of the summed power of every A consecutive frames, the Welch estimate times A (mag is that
        sum).

        The workspace is ``work`` or the cached tensor, as for :meth:`spectra_f32`, and in overlap mode the call joins every
        outstanding call of the handle on the device (as :meth:`flush` does) before the find: the result is valid on the
        current stream when the call returns, and the call lends nothing.  The arguments of the find and ``out`` are refused
        as by :meth:`find_peaks`, ``group`` and a B that is no multiple of it as by :meth:`spectra_f32`, all before anything
        is launched, and so is a wrong ``work``."""
        self._peaks_args(k, threshold, lo, hi, min_sep, None)
        if group is not None:
            self._log2_fold(group, 1)
        forms = FLOAT_CHAIN.inputs
        dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype in forms else next(iter(forms))
        B = self._check_in(x, dtype, forms[dtype][0])
        if group is not None:
            if B % int(group):
                raise SpecanError(abi.SA_ESHAPE, f"the batch ({B} frames) must be a multiple of {int(group)}")
            out = self._peaks_out(B // int(group), int(k), out)      # refused here, before the chain is launched
            rec = self.spectra_f32(x, group, 1, scale=scale, work=work)
            return self.find_peaks(rec, k, threshold, lo, hi, min_sep, field="power", out=out)
        out = self._peaks_out(B, int(k), out)
        return self.find_peaks(self._mag_full_in_work(x, B, scale, work), k, threshold, lo, hi, min_sep, out=out)

    @staticmethod
    def _rank_args(ranks, lo, hi, field) -> tuple:
        """The one validation of the arguments of the order statistics: ``(field code of include/specan_rank.h, the ranks as a
        tuple of ints)``, or SA_EINVAL."""
        for name, v in (("lo", lo), ("hi", hi)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise SpecanError(abi.SA_EINVAL, f"{name} must be an int")
        if not 0 <= int(lo) < int(hi) <= SA_N:
            raise SpecanError(abi.SA_EINVAL, f"the range must be 0 <= lo < hi <= {SA_N}")
        if isinstance(ranks, (str, bytes)) or not hasattr(ranks, "__len__") or not 1 <= len(ranks) <= abi.SA_RANK_Q_MAX:
            raise SpecanError(abi.SA_EINVAL, f"ranks must be a sequence of 1..{abi.SA_RANK_Q_MAX} ints")
        m = int(hi) - int(lo)
        for v in ranks:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < m:
                raise SpecanError(abi.SA_EINVAL, f"a rank must be an int in 0..{m - 1}")
        if not (field is None or isinstance(field, str)) or field not in _RANK_FIELDS:
            raise SpecanError(abi.SA_EINVAL, "field must be None, 'peak' or 'power'")
        return _RANK_FIELDS[field], tuple(int(v) for v in ranks)

    @staticmethod
    def _quantile_ranks(q, lo, hi) -> tuple:
        """``q``, a number in 0..1 or a sequence of 1..8 of them, as the ranks of those lower quantiles among the hi - lo bins
        (frames.rank_of_quantile), or SA_EINVAL; ``lo`` and ``hi`` have been checked."""
        qs = q if hasattr(q, "__len__") and not isinstance(q, (str, bytes)) else (q,)
        if not 1 <= len(qs) <= abi.SA_RANK_Q_MAX:
            raise SpecanError(abi.SA_EINVAL, f"q must be a number or a sequence of 1..{abi.SA_RANK_Q_MAX} numbers")
        try:
            return tuple(frames.rank_of_quantile(v, int(hi) - int(lo)) for v in qs)
        except ValueError as e:
            raise SpecanError(abi.SA_EINVAL, str(e)) from None

    def _rank_out(self, R: int, q: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``out`` of the order statistics of ``R`` rows, allocated when None: SA_ESHAPE where it is not the contiguous float32
        [R, q] tensor on the handle's device."""
        shape = (R, q)
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32
                or out.device != self.device or not out.is_contiguous()):
            raise SpecanError(abi.SA_ESHAPE, f"out must be a contiguous torch.float32 tensor of shape {shape}")
        return out

    def order_stats(self, t: torch.Tensor, ranks: Sequence[int], lo: int = 0, hi: int = SA_N, field: Optional[str] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Order statistics of each row of ``t`` (include/specan_rank.h, sa_rank_f32): float32 [R, q], ``[r, j]`` the value at
        rank ``ranks[j]`` of the ascending sort of the bins ``[lo, hi)`` of row r.  Rank 0 is the minimum of the range, rank
        ``hi - lo - 1`` its maximum; frames.rank_of_quantile gives the rank of a quantile.  ``t`` is a float32 [R,16384]
        device tensor -- what ``process_f32(out_kind='mag_full')`` or ``process_q15(out_kind='mag')`` wrote -- or, with
        ``field='peak'`` or ``field='power'``, float32 [R,16384,2], the records of :meth:`fold_mag_f32` at bucket 1,
        :meth:`spectra_f32` or :meth:`spectra_q15`, of which that float is the point.

        A point's key is its bits with the sign cleared, as an integer: the float order of the chains' non-negative values; a
        NaN ranks above +inf, -0.0 reads as +0.0, no denormal is flushed; the result is those bits.  frames.ranks_of_rows is
        the numpy mirror, bit for bit.  The maximum over a range is peak_mag of :meth:`markers` / :meth:`markers_q15` with that
        marker range on the same frames.  The cost is linear in the number of ranks.

        ``ranks`` is a sequence of 1..8 ints, each ``0 <= rank < hi - lo``, in any order, repeats allowed;
        ``0 <= lo < hi <= 16384``; ints only (a bool or a float is SA_EINVAL); a wrong dtype is SA_EINVAL and a wrong shape
        SA_ESHAPE, all before any device call.  One launch on the current stream of the handle's device -- the ranks travel
        in the launch's arguments -- no handle state, no workspace: it captures into a graph at any time.  Where ``t`` is the
        result of a call made in overlap mode, call :meth:`flush` first.  Pointer contract (checked by the C entry point,
        SA_EINVAL): ``t`` is 16-byte aligned, and the bytes read and the R * q * 4 bytes written are disjoint; buffers that
        merely touch are fine."""
        code, ranks = self._rank_args(ranks, lo, hi, field)
        R = self._check_in(t, torch.float32, (SA_N, 2) if code else SA_N)
        out = self._rank_out(R, len(ranks), out)
        L = abi.rank_lib()
        with torch.cuda.device(self.device):         # the C call launches on the calling thread's current device
            rc = L.sa_rank_f32(t.data_ptr(), code, out.data_ptr(), R, len(ranks), (C.c_int32 * len(ranks))(*ranks), int(lo),
                               int(hi), self._stream())
        if rc != abi.SA_OK:
            raise SpecanError(rc, L.sa_rank_last_error().decode())
        return out

    def noise_floor_f32(self, x: torch.Tensor, q=0.5, lo: int = 0, hi: int = SA_N, group: Optional[int] = None,
                        scale: float = 1.0 / 2048.0, work: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The noise floor of the float chain's spectra, without the spectra leaving the device: float32 [R, len(q)], the lower
        quantiles ``q`` (a number in 0..1, which gives [R, 1], or a sequence of 1..8 of them; 0.5 is the lower median) of the
        bins ``[lo, hi)`` of every row, each the order statistic of rank ``frames.rank_of_quantile(q, hi - lo)``.  ``x`` is
        float32, int16 or packed uint8 exactly as for :meth:`process_f32`; every filter mode and both precisions apply.

        Without ``group`` (R = B) the call is ``process_f32(x, out_kind='mag_full', scale=scale)`` into the workspace of
        :meth:`spectra_f32` followed by :meth:`order_stats`: the floor of every frame's magnitudes.  With ``group=A`` (2, 4,
        ..., 128; R = B // A) it is ``spectra_f32(x, group=A, scale=scale, work=work)`` followed by ``order_stats(...,
        field='power')``: the floor of the summed power of every A consecutive frames, the Welch estimate times A.

        The workspace is ``work`` or the cached tensor, as for :meth:`spectra_f32`, and in overlap mode the call joins every
        outstanding call of the handle on the device (as :meth:`flush` does) before the selection: the result is valid on
        the current stream when the call returns, and the call lends nothing.  ``q``, the range and ``out`` are refused as by
        :meth:`order_stats`, ``group`` and a B that is no multiple of it as by :meth:`spectra_f32`, all before anything is
        launched, and so is a wrong ``work``."""
        self._rank_args((0,), lo, hi, None)
        ranks = self._quantile_ranks(q, lo, hi)
        if group is not None:
            self._log2_fold(group, 1)
        forms = FLOAT_CHAIN.inputs
        dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype in forms else next(iter(forms))
        B = self._check_in(x, dtype, forms[dtype][0])
        if group is not None:
            if B % int(group):
                raise SpecanError(abi.SA_ESHAPE, f"the batch ({B} frames) must be a multiple of {int(group)}")
            out = self._rank_out(B // int(group), len(ranks), out)   # refused here, before the chain is launched
            rec = self.spectra_f32(x, group, 1, scale=scale, work=work)
            return self.order_stats(rec, ranks, lo, hi, field="power", out=out)
        out = self._rank_out(B, len(ranks), out)
        return self.order_stats(self._mag_full_in_work(x, B, scale, work), ranks, lo, hi, out=out)

    @staticmethod
    def _hist_args(edges, group, bucket, lo, hi) -> tuple:
        """The one validation of the arguments of the level histogram: ``(log2 of the bucket, the edges as a tuple of float32
        values)``, or SA_EINVAL.  ``group`` may be None (all rows)."""
        for name, v in (("bucket", bucket), ("lo", lo), ("hi", hi)) + ((("group", group),) if group is not None else ()):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise SpecanError(abi.SA_EINVAL, f"{name} must be an int")
        if group is not None and not 1 <= int(group) <= frames.HIST_GROUP_MAX:
            raise SpecanError(abi.SA_EINVAL, f"group must be 1..{frames.HIST_GROUP_MAX}")
        if int(bucket) not in frames.HIST_BUCKETS:
            raise SpecanError(abi.SA_EINVAL, f"bucket must be one of {frames.HIST_BUCKETS}")
        try:
            keys = frames._hist_edge_keys(edges)
        except ValueError as e:
            raise SpecanError(abi.SA_EINVAL, str(e)) from None
        if not 0 <= int(lo) < int(hi) <= SA_N or int(lo) % int(bucket) or int(hi) % int(bucket):
            raise SpecanError(abi.SA_EINVAL, f"the range must be 0 <= lo < hi <= {SA_N}, both multiples of the bucket")
        return int(bucket).bit_length() - 1, tuple(float(v) for v in keys.view(np.float32))

    def _hist_out(self, R: int, group, bucket: int, lo: int, hi: int, L: int, out: Optional[torch.Tensor]) -> tuple:
        """``(group, out)`` of the level histogram of ``R`` rows, ``group`` None meaning all of them and ``out`` allocated when
        None: SA_ESHAPE where R is no multiple of the group or ``out`` is not the contiguous uint32 [G, C, L] tensor on the
        handle's device."""
        A = max(R, 1) if group is None else int(group)
        if A > frames.HIST_GROUP_MAX:
            raise SpecanError(abi.SA_EINVAL, f"group must be 1..{frames.HIST_GROUP_MAX}")
        if R % A:
            raise SpecanError(abi.SA_ESHAPE, f"the rows ({R}) must be a multiple of {A}")
        shape = (R // A, (int(hi) - int(lo)) // int(bucket), L)
        if out is None:
            return A, torch.empty(shape, dtype=torch.uint32, device=self.device)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.uint32
                or out.device != self.device or not out.is_contiguous()):
            raise SpecanError(abi.SA_ESHAPE, f"out must be a contiguous torch.uint32 tensor of shape {shape}")
        return A, out

    def level_hist(self, t: torch.Tensor, edges: Sequence[float], group: Optional[int] = None, bucket: int = 1, lo: int = 0,
                   hi: int = SA_N, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The level histogram of the rows of ``t`` (include/specan_hist.h, sa_hist_f32), the data of a persistence display:
        uint32 [G, C, L], ``[g, c, l]`` the number of points of group g (``group`` consecutive rows; None: all rows, G = 1)
        and column c (the bins ``[lo + c bucket, lo + (c + 1) bucket)``) whose level is l.  ``t`` is a float32 [R,16384]
        device tensor: what ``process_f32(out_kind='mag_full')`` or ``process_q15(out_kind='mag')`` wrote.

        A point's key is its bits with the sign cleared, as an integer: the float order of the chains' non-negative values; a
        NaN is above +inf, -0.0 reads as +0.0, no denormal is flushed.  Its level is the number of ``edges`` whose key is not
        above its own, 0..L-1 with L = len(edges) + 1: a value equal to an edge is in the level above it.  The L counters of
        a cell column sum to ``group * bucket``; the counts add across calls, so a longer persistence is a sum (or a decayed
        sum) of these small images on the host.  frames.hist_of_rows is the numpy mirror, bit for bit; frames.level_edges_db
        makes edges evenly spaced in dB.

        ``edges`` is a sequence of 1..63 numbers, each +0.0 .. +inf as a float32 and none below the one before; ``group`` is
        1..2^24 and divides R; ``bucket`` is 1, 2, 4, ..., 64; ``0 <= lo < hi <= 16384``, both multiples of ``bucket``; ints
        only (a bool or a float is SA_EINVAL); a wrong dtype is SA_EINVAL and a wrong shape SA_ESHAPE, all before any
        device call.  One launch on the current stream of the handle's device (two, the first zeroing ``out``, where there
        are fewer than 256 pairs of a group and a 256-bin tile and ``group`` is 64 or more) -- the edges travel in the
        launch's arguments, every counter is written (``out`` needs no zeroing) -- no handle state, no workspace: it captures
        into a graph at any time.  Where ``t`` is the result of a call made in overlap mode, call :meth:`flush` first.  Pointer
        contract (checked by the C entry point, SA_EINVAL): ``t`` is 16-byte aligned, and the bytes read and the G * C * L * 4
        bytes written are disjoint; buffers that merely touch are fine."""
        log2w, edges = self._hist_args(edges, group, bucket, lo, hi)
        R = self._check_in(t, torch.float32, SA_N)
        A, out = self._hist_out(R, group, int(bucket), lo, hi, len(edges) + 1, out)
        L = abi.hist_lib()
        with torch.cuda.device(self.device):         # the C call launches on the calling thread's current device
            rc = L.sa_hist_f32(t.data_ptr(), out.data_ptr(), R, A, log2w, len(edges) + 1, (C.c_float * len(edges))(*edges),
                               int(lo), int(hi), self._stream())
        if rc != abi.SA_OK:
            raise SpecanError(rc, L.sa_hist_last_error().decode())
        return out

    def persistence_f32(self, x: torch.Tensor, edges: Sequence[float], group: Optional[int] = None, bucket: int = 16,
                        lo: int = 0, hi: int = SA_N, scale: float = 1.0 / 2048.0, work: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The level histogram of the float chain's spectra, without the spectra leaving the device: uint32 [G, C, L] as
        :meth:`level_hist` returns it.  ``x`` is float32, int16 or packed uint8 exactly as for :meth:`process_f32`; every
        filter mode and both precisions apply.  The call is ``process_f32(x, out_kind='mag_full', scale=scale)`` into the
        workspace of :meth:`spectra_f32` followed by :meth:`level_hist`.

        The workspace is ``work`` or the cached tensor, as for :meth:`spectra_f32`, and in overlap mode the call joins every
        outstanding call of the handle on the device (as :meth:`flush` does) before the count: the result is valid on the
        current stream when the call returns, and the call lends nothing.  The edges, ``group`` (None: the whole batch),
        ``bucket``, the range and ``out`` are refused as by :meth:`level_hist`, all before anything is launched, and so is
        a wrong ``work``."""
        log2w, keys = self._hist_args(edges, group, bucket, lo, hi)
        forms = FLOAT_CHAIN.inputs
        dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype in forms else next(iter(forms))
        B = self._check_in(x, dtype, forms[dtype][0])
        A, out = self._hist_out(B, group, int(bucket), lo, hi, len(keys) + 1, out)     # refused here, before the chain is launched
        return self.level_hist(self._mag_full_in_work(x, B, scale, work), edges, A, bucket, lo, hi, out=out)

    @staticmethod
    def _bands_args(bands, fracs, field) -> tuple:
        """The one validation of the arguments of the band power: ``(field code of include/specan_bands.h, the bands as a
        tuple of (lo, hi) int pairs, the fractions as a tuple of floats)``, or SA_EINVAL."""
        try:
            bands, fracs = frames._bands_args(bands, fracs, field)
        except ValueError as e:
            raise SpecanError(abi.SA_EINVAL, str(e)) from None
        return _BANDS_FIELDS[field], bands, fracs

    def _bands_out(self, R: int, nb: int, nq: int, power: Optional[torch.Tensor], cross: Optional[torch.Tensor]) -> tuple:
        """``(power, cross)`` of the band power of ``R`` rows, each allocated when None: SA_ESHAPE where ``power`` is not the
        contiguous float64 [R, nb] tensor or ``cross`` not the contiguous int32 [R, nb, nq] tensor on the handle's device.
        Without fractions ``cross`` is handed back as it came and never looked at."""
        for name, t, shape, dtype in (("power", power, (R, nb), torch.float64), ("cross", cross, (R, nb, nq), torch.int32)):
            if t is None or (name == "cross" and nq == 0):
                continue
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device
                    or not t.is_contiguous()):
                raise SpecanError(abi.SA_ESHAPE, f"{name} must be a contiguous {dtype} tensor of shape {shape}")
        if power is None:
            power = torch.empty((R, nb), dtype=torch.float64, device=self.device)
        if cross is None and nq:
            cross = torch.empty((R, nb, nq), dtype=torch.int32, device=self.device)
        return power, cross

    def band_power(self, t: torch.Tensor, bands: Sequence, fracs: Sequence[float] = (), field: Optional[str] = None,
                   power: Optional[torch.Tensor] = None, cross: Optional[torch.Tensor] = None) -> tuple:
        """Band power and occupied bandwidth of each row of ``t`` (include/specan_bands.h, sa_bands_f32): ``(power float64
        [R, nb], cross int32 [R, nb, nq])``, or ``(power, None)`` without fractions.  ``power[r, j]`` is the sum of the power
        of the bins ``[lo_j, hi_j)`` of row r in float64; ``cross[r, j, q]`` the bin of that band at which its cumulative
        power reaches ``fracs[q]`` of it, or -1 where the band holds a NaN.  ``t`` is a float32 [R,16384] device tensor --
        what ``process_f32(out_kind='mag_full')`` or ``process_q15(out_kind='mag')`` wrote, squared bin by bin -- or, with
        ``field='peak'`` (squared) or ``field='power'`` (taken as it is: a power sum already), float32 [R,16384,2], the
        records of :meth:`fold_mag_f32` at bucket 1, :meth:`spectra_f32` or :meth:`spectra_q15`.  Of ``spectra_f32(group=A)``
        the power is the sum over A frames: the Welch mean is ``power / A`` on the host.

        A point's value is the float with its sign cleared, widened to float64 (denormals kept); a band's sum is the balanced
        tree of adjacent pairs over the row with +0.0 outside the band -- the tree of :meth:`fold_mag_f32` across a bucket,
        continued -- and a crossing a 14-step descent of that tree; frames.bands_of_rows is the numpy mirror, bit for bit.
        Channel power and ACPR are a main band and its neighbours (frames.channel_bands); occupied bandwidth at 99 % is
        ``fracs=(0.005, 0.995)``; the power median of a band is 0.5.

        ``bands`` is a sequence of 1..16 (lo, hi) pairs of ints, ``0 <= lo < hi <= 16384``, in any order, overlapping or
        repeated; ``fracs`` a sequence of 0..4 numbers in [0, 1 - 2^-32]; a bool or a float where an int belongs is
        SA_EINVAL; a wrong dtype is SA_EINVAL and a wrong shape SA_ESHAPE, all before any device call.  One launch on the
        current stream of the handle's device -- the bands and fractions travel in the launch's arguments -- no atomics, no
        handle state, no workspace: it captures into a graph at any time.  Where ``t`` is the result of a call made in
        overlap mode, call :meth:`flush` first.  Pointer contract (checked by the C entry point, SA_EINVAL): ``t`` is 16-byte
        aligned, and the bytes read, the R * nb * 8 bytes of ``power`` and the R * nb * nq * 4 bytes of ``cross`` are
        pairwise disjoint; buffers that merely touch are fine."""
        code, bands, fracs = self._bands_args(bands, fracs, field)
        R = self._check_in(t, torch.float32, (SA_N, 2) if code else SA_N)
        nb, nq = len(bands), len(fracs)
        power, cross = self._bands_out(R, nb, nq, power, cross)
        L = abi.bands_lib()
        c_bands = (abi.Band * nb)(*(abi.Band(lo, hi) for lo, hi in bands))
        c_fracs = (C.c_double * nq)(*fracs) if nq else None
        with torch.cuda.device(self.device):         # the C call launches on the calling thread's current device
            rc = L.sa_bands_f32(t.data_ptr(), code, power.data_ptr(), cross.data_ptr() if nq else None, R, nb, c_bands, nq,
                                c_fracs, self._stream())
        if rc != abi.SA_OK:
            raise SpecanError(rc, L.sa_bands_last_error().decode())
        return power, cross if nq else None

    def channel_power_f32(self, x: torch.Tensor, bands: Sequence, fracs: Sequence[float] = (), group: Optional[int] = None,
                          scale: float = 1.0 / 2048.0, work: Optional[torch.Tensor] = None,
                          power: Optional[torch.Tensor] = None, cross: Optional[torch.Tensor] = None) -> tuple:
        """Band power and occupied bandwidth of the float chain's spectra, without the spectra leaving the device: ``(power
        float64 [R, nb], cross int32 [R, nb, nq] or None)`` as :meth:`band_power` returns them.  ``x`` is float32, int16 or
        packed uint8 exactly as for :meth:`process_f32`; every filter mode and both precisions apply.

        Without ``group`` (R = B) the call is ``process_f32(x, out_kind='mag_full', scale=scale)`` into the workspace of
        :meth:`spectra_f32` followed by :meth:`band_power`: the band powers of every frame.  With ``group=A`` (2, 4, ...,
        128; R = B // A) it is ``spectra_f32(x, group=A, scale=scale, work=work)`` followed by ``band_power(...,
        field='power')``: the band powers of the summed power of every A consecutive frames, the Welch estimate times A.

        The workspace is ``work`` or the cached tensor, as for :meth:`spectra_f32`, and in overlap mode the call joins every
        outstanding call of the handle on the device (as :meth:`flush` does) before the sums: the result is valid on the
        current stream when the call returns, and the call lends nothing.  The bands, the fractions, ``power`` and ``cross``
        are refused as by :meth:`band_power`, ``group`` and a B that is no multiple of it as by :meth:`spectra_f32`, all
        before anything is launched, and so is a wrong ``work``."""
        _, bands, fracs = self._bands_args(bands, fracs, None)
        if group is not None:
            self._log2_fold(group, 1)
        forms = FLOAT_CHAIN.inputs
        dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype in forms else next(iter(forms))
        B = self._check_in(x, dtype, forms[dtype][0])
        if group is not None:
            if B % int(group):
                raise SpecanError(abi.SA_ESHAPE, f"the batch ({B} frames) must be a multiple of {int(group)}")
            power, cross = self._bands_out(B // int(group), len(bands), len(fracs), power, cross)      # refused here, before the chain
            rec = self.spectra_f32(x, group, 1, scale=scale, work=work)
            return self.band_power(rec, bands, fracs, field="power", power=power, cross=cross)
        power, cross = self._bands_out(B, len(bands), len(fracs), power, cross)
        return self.band_power(self._mag_full_in_work(x, B, scale, work), bands, fracs, power=power, cross=cross)

    @staticmethod
    def _mask_args(upper, lower, lo, hi, field) -> int:
        """The one validation of the scalar arguments of the mask test: the ``field`` code of include/specan_mask.h, or
        SA_EINVAL.  The limits are only counted here; :meth:`_mask_limits` looks at them."""
        for name, v in (("lo", lo), ("hi", hi)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise SpecanError(abi.SA_EINVAL, f"{name} must be an int")
        if not 0 <= int(lo) < int(hi) <= SA_N:
            raise SpecanError(abi.SA_EINVAL, f"the range must be 0 <= lo < hi <= {SA_N}")
        if not (field is None or isinstance(field, str)) or field not in _MASK_FIELDS:
            raise SpecanError(abi.SA_EINVAL, "field must be None, 'peak' or 'power'")
        if upper is None and lower is None:
            raise SpecanError(abi.SA_EINVAL, "upper and lower are both None: no limit at all")
        return _MASK_FIELDS[field]

    def _mask_limits(self, upper, lower) -> None:
        """SA_ESHAPE where a limit is neither None nor a contiguous float32 [16384] tensor on the handle's device."""
        for name, v in (("upper", upper), ("lower", lower)):
            if v is not None and (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != (SA_N,)
                                  or v.device != self.device or not v.is_contiguous()):
                raise SpecanError(abi.SA_ESHAPE, f"{name} must be None or a contiguous torch.float32 tensor of shape ({SA_N},)")

    def _mask_out(self, R: int, out: Optional[torch.Tensor], summary) -> tuple:
        """``(out, summary)`` of the mask test of ``R`` rows: ``out`` allocated when None, ``summary`` allocated when True and
        None when False or None: SA_ESHAPE where ``out`` is not the contiguous int32 [R, 10] tensor or a given ``summary`` not
        the contiguous int32 [4] tensor on the handle's device."""
        for name, t, shape in (("out", out, (R, 10)), ("summary", summary, (4,))):
            if t is None or isinstance(t, bool):
                continue
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != self.device
                    or not t.is_contiguous()):
                raise SpecanError(abi.SA_ESHAPE, f"{name} must be a contiguous torch.int32 tensor of shape {shape}")
        if out is None:
            out = torch.empty((R, 10), dtype=torch.int32, device=self.device)
        if summary is True:
            summary = torch.empty((4,), dtype=torch.int32, device=self.device)
        return out, (None if summary is False else summary)

    def mask_test(self, t: torch.Tensor, upper: Optional[torch.Tensor], lower: Optional[torch.Tensor] = None, lo: int = 0,
                  hi: int = SA_N, field: Optional[str] = None, out: Optional[torch.Tensor] = None, summary=False) -> tuple:
        """The spectral mask test of each row of ``t`` (include/specan_mask.h, sa_mask_f32): ``(ints int32 [R, 6], floats
        float32 [R, 4], summary int32 [4] or None)``.  ``ints[r]`` is (over, under, first, last, up_bin, lo_bin) and
        ``floats[r]`` (up_val, up_lim, lo_val, lo_lim) of row r, both views of the [R, 10] int32 record tensor (``out``,
        allocated when None; one sa_mask_row per row, frames.MASK_ROW on the host).  ``t`` is a float32 [R,16384] device
        tensor -- what ``process_f32(out_kind='mag_full')`` or ``process_q15(out_kind='mag')`` wrote -- or, with
        ``field='peak'`` or ``field='power'``, float32 [R,16384,2], the records of :meth:`fold_mag_f32` at bucket 1,
        :meth:`spectra_f32` or :meth:`spectra_q15`, of which that float is the point.  Nothing is squared: the limits are in
        the unit of the points, powers for ``field='power'``.

        ``upper`` and ``lower`` are float32 [16384] device tensors shared by all rows, or None (not both; the same tensor may
        be both); bin i has that limit where the value is finite and above 0 and ``lo <= i < hi`` -- 0, a negative value,
        an infinity or a NaN leaves a gap.  ``over`` counts the limited bins where the point, its sign cleared, is above the
        upper limit or a NaN, ``under`` those below the lower limit or a NaN; ``first`` and ``last`` are the lowest and
        highest such bin or -1.  ``up_bin`` is the bin whose point / limit is largest and ``lo_bin`` the one where it is
        smallest, by the exact ratio of the two float32 values, equal ratios to the lowest bin; the floats are the point and
        the limit there (frames.mask_margin_db turns them into dB), -1 and +0.0 without a limited bin.  ``summary=True`` (or
        an int32 [4] tensor to write into) adds the trigger: the rows with over > 0, the rows with under > 0, the first row
        with either or -1 and the last.  frames.mask_of_rows is the numpy mirror, bit for bit.

        ``lo`` and ``hi`` take ints only (a bool or a float is SA_EINVAL); a wrong dtype of ``t`` is SA_EINVAL and a wrong
        shape SA_ESHAPE, all before any device call.  One launch on the current stream of the handle's device, and one more
        of a single workgroup for the summary -- no atomics, nothing zeroed, no handle state, no workspace: it captures into a
        graph at any time and every replay gives the summary of its own input.  Where ``t`` is the result of a call made in
        overlap mode, call :meth:`flush` first.  Pointer contract (checked by the C entry point, SA_EINVAL): ``t`` and the
        limits are 16-byte aligned, and the bytes read, the R * 40 bytes of the records and the 16 of the summary are
        pairwise disjoint; buffers that merely touch are fine."""
        code = self._mask_args(upper, lower, lo, hi, field)
        R = self._check_in(t, torch.float32, (SA_N, 2) if code else SA_N)
        self._mask_limits(upper, lower)
        out, summary = self._mask_out(R, out, summary)
        L = abi.mask_lib()
        with torch.cuda.device(self.device):         # the C call launches on the calling thread's current device
            rc = L.sa_mask_f32(t.data_ptr(), code, None if upper is None else upper.data_ptr(),
                               None if lower is None else lower.data_ptr(), int(lo), int(hi), out.data_ptr(),
                               None if summary is None else summary.data_ptr(), R, self._stream())
        if rc != abi.SA_OK:
            raise SpecanError(rc, L.sa_mask_last_error().decode())
        return out[:, :6], out.view(torch.float32)[:, 6:], summary

    def mask_trigger_f32(self, x: torch.Tensor, upper: Optional[torch.Tensor], lower: Optional[torch.Tensor] = None, lo: int = 0,
                         hi: int = SA_N, group: Optional[int] = None, scale: float = 1.0 / 2048.0,
                         work: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                         summary: Optional[torch.Tensor] = None) -> tuple:
        """The frequency-mask trigger on the float chain's spectra, without the spectra leaving the device: ``(ints int32
        [R, 6], floats float32 [R, 4], summary int32 [4])`` as :meth:`mask_test` returns them with the summary -- which rows
        left the mask, the first and last of them, and every row's worst bins.  ``x`` is float32, int16 or packed uint8
        exactly as for :meth:`process_f32`; every filter mode and both precisions apply.

        Without ``group`` (R = B) the call is ``process_f32(x, out_kind='mag_full', scale=scale)`` into the workspace of
        :meth:`spectra_f32` followed by :meth:`mask_test`: every frame's magnitudes against limits in amplitude.  With
        ``group=A`` (2, 4, ..., 128; R = B // A) it is ``spectra_f32(x, group=A, scale=scale, work=work)`` followed by
        ``mask_test(..., field='power')``: the summed power of every A consecutive frames, the Welch estimate times A,
        against limits in that unit.

        The workspace is ``work`` or the cached tensor, as for :meth:`spectra_f32`, and in overlap mode the call joins every
        outstanding call of the handle on the device (as :meth:`flush` does) before the test: the result is valid on the
        current stream when the call returns, and the call lends nothing.  The limits, the range, ``out`` and ``summary``
        (a tensor to write into, allocated when None) are refused as by :meth:`mask_test`, ``group`` and a B that is no
        multiple of it as by :meth:`spectra_f32`, all before anything is launched, and so is a wrong ``work``."""
        self._mask_args(upper, lower, lo, hi, None)
        if group is not None:
            self._log2_fold(group, 1)
        forms = FLOAT_CHAIN.inputs
        dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype in forms else next(iter(forms))
        B = self._check_in(x, dtype, forms[dtype][0])
        self._mask_limits(upper, lower)
        if isinstance(summary, bool):
            raise SpecanError(abi.SA_ESHAPE, "summary must be None or a contiguous torch.int32 tensor of shape (4,)")
        if group is not None:
            if B % int(group):
                raise SpecanError(abi.SA_ESHAPE, f"the batch ({B} frames) must be a multiple of {int(group)}")
            out, summary = self._mask_out(B // int(group), out, True if summary is None else summary)      # before the chain
            rec = self.spectra_f32(x, group, 1, scale=scale, work=work)
            return self.mask_test(rec, upper, lower, lo, hi, field="power", out=out, summary=summary)
        out, summary = self._mask_out(B, out, True if summary is None else summary)
        return self.mask_test(self._mag_full_in_work(x, B, scale, work), upper, lower, lo, hi, out=out, summary=summary)

    @staticmethod
    def _harm_args(order, span, lo, hi, fund, dc, top, field) -> tuple:
        """The one validation of the arguments of the harmonic analysis: ``(field code of include/specan_harm.h, the
        sa_harm_cfg with the defaults filled in)``, or SA_EINVAL."""
        try:
            cfg = frames._harm_args(order, span, lo, hi, fund, dc, top, field)
        except ValueError as e:
            raise SpecanError(abi.SA_EINVAL, str(e)) from None
        return _HARM_FIELDS[field], abi.HarmCfg(*cfg)

    def _harm_out(self, R: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """The record tensor of the harmonic analysis of ``R`` rows, allocated when None: SA_ESHAPE where ``out`` is not the
        contiguous int32 [R, 42] tensor on the handle's device."""
        if out is None:
            return torch.empty((R, _HARM_WORDS), dtype=torch.int32, device=self.device)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != (R, _HARM_WORDS) or out.dtype != torch.int32
                or out.device != self.device or not out.is_contiguous()):
            raise SpecanError(abi.SA_ESHAPE, f"out must be a contiguous torch.int32 tensor of shape ({R}, {_HARM_WORDS})")
        return out

    def harmonics(self, t: torch.Tensor, order: int = 5, span: int = 3, lo: Optional[int] = None, hi: Optional[int] = None,
                  fund: Optional[int] = None, dc: Optional[int] = None, top: int = frames.HARM_TOP_MAX,
                  field: Optional[str] = None, out: Optional[torch.Tensor] = None) -> tuple:
        """The harmonic analysis of each row of ``t`` (include/specan_harm.h, sa_harm_f32): ``(sums float64 [R, 13], bins
        int32 [R, 10], levels float32 [R, 3], marks int32 [R, 3])``, all views of the [R, 42] int32 record tensor (``out``,
        allocated when None; one sa_harm_row of 168 bytes per row: ``out.cpu().numpy().view(frames.HARM_ROW)[:, 0]`` is what
        frames.harm_metrics turns into SFDR, THD, SINAD, SNR and ENOB).  ``sums[r]`` is (power[0..9], dist, nad, noise),
        ``bins[r]`` the fundamental's bin and the bins harmonics 2..order alias to (-1 in the unused slots), ``levels[r]``
        (fund, spur, nonharm) and ``marks[r]`` (spur_bin, nonharm_bin, n_noise).  ``t`` is a float32 [R,16384] device tensor
        -- what ``process_f32(out_kind='mag_full')`` or ``process_q15(out_kind='mag')`` wrote, squared bin by bin in the sums
        -- or, with ``field='peak'`` (squared) or ``field='power'`` (taken as it is), float32 [R,16384,2], the records of
        :meth:`fold_mag_f32` at bucket 1, :meth:`spectra_f32` or :meth:`spectra_q15`.

        The analysed bins are ``[dc, top)`` (``dc`` defaults to ``span + 1``, ``top`` to 8193: a real input's spectrum).  The
        fundamental is bin ``fund`` where given (coherent sampling), else the largest point of ``[lo, hi)`` (default: all
        analysed bins), equal points to the lowest bin.  Harmonic h = 2..``order`` aliases to ``(h * k1) mod 16384`` folded
        about 8192; a tone's band reaches ``span`` bins to either side, clipped to the analysed bins.  ``power[0]`` is the
        float64 power of the fundamental's band F, ``power[h - 1]`` that of harmonic h's band less F, ``dist`` that of their
        union, ``nad`` that of all analysed bins less F and ``noise`` that less the harmonics too, each the balanced pair tree
        of :meth:`band_power`; ``spur`` is the largest point outside F and ``nonharm`` the largest that is in no harmonic's
        band either.  frames.harm_of_rows is the numpy mirror, bit for bit.

        The integers take ints only (a bool or a float is SA_EINVAL), ``order`` 1..10, ``span`` 0..64, ``0 <= dc < top <=
        8193``, ``dc <= lo < hi <= top``; a wrong dtype of ``t`` is SA_EINVAL and a wrong shape SA_ESHAPE, all before any
        device call.  One launch on the current stream of the handle's device -- the parameters travel in the launch's
        arguments -- no atomics, nothing zeroed, no handle state, no workspace: it captures into a graph at any time.  Where
        ``t`` is the result of a call made in overlap mode, call :meth:`flush` first.  Pointer contract (checked by the C
        entry point, SA_EINVAL): ``t`` is 16-byte aligned, and the bytes of ``t`` and the R * 168 bytes of the records are
        disjoint; buffers that merely touch are fine."""
        code, cfg = self._harm_args(order, span, lo, hi, fund, dc, top, field)
        R = self._check_in(t, torch.float32, (SA_N, 2) if code else SA_N)
        out = self._harm_out(R, out)
        L = abi.harm_lib()
        with torch.cuda.device(self.device):         # the C call launches on the calling thread's current device
            rc = L.sa_harm_f32(t.data_ptr(), code, out.data_ptr(), R, C.byref(cfg), self._stream())
        if rc != abi.SA_OK:
            raise SpecanError(rc, L.sa_harm_last_error().decode())
        return out.view(torch.float64)[:, :13], out[:, 26:36], out.view(torch.float32)[:, 36:39], out[:, 39:]

    def harmonics_f32(self, x: torch.Tensor, order: int = 5, span: int = 3, lo: Optional[int] = None, hi: Optional[int] = None,
                      fund: Optional[int] = None, dc: Optional[int] = None, top: int = frames.HARM_TOP_MAX,
                      group: Optional[int] = None, scale: float = 1.0 / 2048.0, work: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> tuple:
        """The harmonic analysis of the float chain's spectra, without the spectra leaving the device: ``(sums, bins, levels,
        marks)`` as :meth:`harmonics` returns them.  ``x`` is float32, int16 or packed uint8 exactly as for
        :meth:`process_f32`; every filter mode and both precisions apply.

        Without ``group`` (R = B) the call is ``process_f32(x, out_kind='mag_full', scale=scale)`` into the workspace of
        :meth:`spectra_f32` followed by :meth:`harmonics`: the figures of every frame.  With ``group=A`` (2, 4, ..., 128;
        R = B // A) it is ``spectra_f32(x, group=A, scale=scale, work=work)`` followed by ``harmonics(..., field='power')``:
        the figures of the summed power of every A consecutive frames, where averaging has lowered the noise's variance
        (frames.harm_metrics with ``unit='power'``).

        The workspace is ``work`` or the cached tensor, as for :meth:`spectra_f32`, and in overlap mode the call joins every
        outstanding call of the handle on the device (as :meth:`flush` does) before the analysis: the result is valid on the
        current stream when the call returns, and the call lends nothing.  The parameters and ``out`` are refused as by
        :meth:`harmonics`, ``group`` and a B that is no multiple of it as by :meth:`spectra_f32`, all before anything is
        launched, and so is a wrong ``work``."""
        self._harm_args(order, span, lo, hi, fund, dc, top, None)
        if group is not None:
            self._log2_fold(group, 1)
        forms = FLOAT_CHAIN.inputs
        dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype in forms else next(iter(forms))
        B = self._check_in(x, dtype, forms[dtype][0])
        if group is not None:
            if B % int(group):
                raise SpecanError(abi.SA_ESHAPE, f"the batch ({B} frames) must be a multiple of {int(group)}")
            out = self._harm_out(B // int(group), out)             # refused here, before the chain is launched
            rec = self.spectra_f32(x, group, 1, scale=scale, work=work)
            return self.harmonics(rec, order, span, lo, hi, fund, dc, top, field="power", out=out)
        out = self._harm_out(B, out)
        return self.harmonics(self._mag_full_in_work(x, B, scale, work), order, span, lo, hi, fund, dc, top, out=out)

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
