"""The reductions of ``SpectrumChain``: the calls of the handle-less libraries of abi.LIBRARIES -- the fold of float
magnitudes, the peak table, the order statistics, the level histogram, the band power, the mask test, the harmonic
analysis, the signal list and the CFAR normalisation -- on tensors the caller has (``fold_mag_f32``, ``find_peaks``, ...) and
composed with the float chain, the spectra never leaving the device (``spectra_f32``, ``peak_table_f32``, ...).

``Reductions`` is a mixin of ``SpectrumChain`` (chain.py, which this module does not import): it reaches the handle through
``self`` -- ``device``, ``_stream``, ``_check_in``, ``_float_frames``, ``process_f32``, ``flush`` -- and keeps one copy of
what every reduction does: allocate-or-refuse of the outputs (``_outs``), the C call (``_call``) and the body of the composed
calls (``_of_spectra``).  The rules of the scalar arguments are those of the numpy mirrors, stated once in frames.py
(``frames._x_args``): ``_rules`` runs one and turns its ValueError into SA_EINVAL with the same text, so that a wrapper and
its mirror refuse the same calls in the same words.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import abi, frames
from .abi import SA_N, SpecanError

# field=... -> the `field` of include/specan_{peaks,rank,bands,mask,harm,signals,cfar}.h: plain magnitudes, or one float of
# (peak, power) records; the seven headers number the three layouts alike (SA_X_IN_MAG, SA_X_IN_POINT_PEAK, SA_X_IN_POINT_POWER)
FIELDS = {None: 0, "peak": 1, "power": 2}
HARM_WORDS = C.sizeof(abi.HarmRow) // 4                                       # an sa_harm_row as int32 words: 42
SIGNAL_WORDS = C.sizeof(abi.Signal) // 4                                      # an sa_signal as int32 words: 6


def _rules(rule, *args):
    """``rule(*args)``, a rule function of frames.py, its ValueError re-raised as SA_EINVAL with the same text."""
    try:
        return rule(*args)
    except ValueError as e:
        raise SpecanError(abi.SA_EINVAL, str(e)) from None


class Reductions:
    """The reduction methods of ``SpectrumChain`` (module docstring)."""

    # ------------------------------------------------------------------ the skeleton
    def _outs(self, *specs) -> list:
        """The output tensors of a call, one per ``(name, tensor or None, shape, dtype)``: the tensor, allocated when None.
        SA_ESHAPE where a given one is not the contiguous ``dtype`` tensor of ``shape`` on the handle's device; every given
        one is looked at before the first is allocated."""
        for name, t, shape, dtype in specs:
            if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype
                                  or t.device != self.device or not t.is_contiguous()):
                raise SpecanError(abi.SA_ESHAPE, f"{name} must be a contiguous {dtype} tensor of shape {shape}")
        return [torch.empty(shape, dtype=dtype, device=self.device) if t is None else t for _, t, shape, dtype in specs]

    def _call(self, L: C.CDLL, entry: str, *args) -> None:
        """``entry(*args, stream)`` of the library ``L``, sa_<library>_...: a launch on the current stream of the handle's
        device, or the SpecanError of its code and the library's last error."""
        with torch.cuda.device(self.device):         # the C call launches on the calling thread's current device
            rc = getattr(L, entry)(*args, self._stream())
        if rc != abi.SA_OK:
            sa_last_error = getattr(L, f"sa_{entry.split('_')[1]}_last_error")
            raise SpecanError(rc, sa_last_error().decode())

    def _of_spectra(self, x, group, scale, work, outputs, reduce, after_input=None):
        """The body of every composed call: ``reduce(t, field, outputs(R))`` on the float chain's spectra of ``x``.  Without
        ``group``, ``t`` is the magnitudes of the B frames in the workspace, ``field`` None and R = B; with ``group=A`` it is
        ``spectra_f32(x, A)``, ``field`` 'power' and R = B // A.  ``outputs(R)`` prepares or refuses the caller's output
        tensors; it and ``after_input()``, the checks a call makes between the input's and the batch's, run before anything
        is launched."""
        if group is not None:
            self._log2_fold(group, 1)
        B = self._float_frames(x)
        if after_input is not None:
            after_input()
        if group is None:
            outs = outputs(B)
            return reduce(self._mag_full_in_work(x, B, scale, work), None, outs)
        if B % int(group):
            raise SpecanError(abi.SA_ESHAPE, f"the batch ({B} frames) must be a multiple of {int(group)}")
        outs = outputs(B // int(group))              # refused here, before the chain is launched
        return reduce(self.spectra_f32(x, group, 1, scale=scale, work=work), "power", outs)

    # ------------------------------------------------------------------ the fold
    @staticmethod
    def _log2_fold(group, bucket) -> tuple:
        """The one validation of the ``group`` and ``bucket`` of the float fold: (a, k) of A = 2^a and W = 2^k, or SA_EINVAL."""
        group, bucket = _rules(frames._fold_args, group, bucket)
        return group.bit_length() - 1, bucket.bit_length() - 1

    def _fold_out(self, B: int, group: int, bucket: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``out`` of the float fold of ``B`` frames, allocated when None: SA_ESHAPE where B is no multiple of the group or
        ``out`` is not the contiguous float32 [B // group, 16384 // bucket, 2] tensor on the handle's device."""
        if B % group:
            raise SpecanError(abi.SA_ESHAPE, f"the batch ({B} frames) must be a multiple of {group}")
        return self._outs(("out", out, (B // group, SA_N // bucket, 2), torch.float32))[0]

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
        self._call(abi.fold_lib(), "sa_fold_mag_f32", mag.data_ptr(), out.data_ptr(), B, a, k)
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
        B = self._float_frames(x)
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
        _rules(frames._peaks_args, k, threshold, lo, hi, min_sep, field)
        return FIELDS[field]

    def _peaks_out(self, R: int, k: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``out`` of the peak table of ``R`` rows, allocated when None: SA_ESHAPE where it is not the contiguous int32 [R, k, 2]
        tensor on the handle's device."""
        return self._outs(("out", out, (R, k, 2), torch.int32))[0]

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
        self._call(abi.peaks_lib(), "sa_peaks_f32", t.data_ptr(), code, out.data_ptr(), count.data_ptr(), R, int(k),
                   float(threshold), int(lo), int(hi), int(min_sep))
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
        return self._of_spectra(x, group, scale, work, lambda R: self._peaks_out(R, int(k), out),
                                lambda t, field, out: self.find_peaks(t, k, threshold, lo, hi, min_sep, field, out))

    @staticmethod
    def _rank_args(ranks, lo, hi, field) -> tuple:
        """The one validation of the arguments of the order statistics: ``(field code of include/specan_rank.h, the ranks as a
        tuple of ints)``, or SA_EINVAL."""
        ranks, _, _ = _rules(frames._rank_args, ranks, lo, hi, field)
        return FIELDS[field], ranks

    @staticmethod
    def _quantile_ranks(q, lo, hi) -> tuple:
        """``q``, a number in 0..1 or a sequence of 1..8 of them, as the ranks of those lower quantiles among the hi - lo bins
        (frames.rank_of_quantile), or SA_EINVAL; ``lo`` and ``hi`` have been checked."""
        qs = q if hasattr(q, "__len__") and not isinstance(q, (str, bytes)) else (q,)
        if not 1 <= len(qs) <= abi.SA_RANK_Q_MAX:
            raise SpecanError(abi.SA_EINVAL, f"q must be a number or a sequence of 1..{abi.SA_RANK_Q_MAX} numbers")
        return tuple(_rules(frames.rank_of_quantile, v, int(hi) - int(lo)) for v in qs)

    def _rank_out(self, R: int, q: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``out`` of the order statistics of ``R`` rows, allocated when None: SA_ESHAPE where it is not the contiguous float32
        [R, q] tensor on the handle's device."""
        return self._outs(("out", out, (R, q), torch.float32))[0]

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
        self._call(abi.rank_lib(), "sa_rank_f32", t.data_ptr(), code, out.data_ptr(), R, len(ranks),
                   (C.c_int32 * len(ranks))(*ranks), int(lo), int(hi))
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
        return self._of_spectra(x, group, scale, work, lambda R: self._rank_out(R, len(ranks), out),
                                lambda t, field, out: self.order_stats(t, ranks, lo, hi, field, out))

    @staticmethod
    def _hist_args(edges, group, bucket, lo, hi) -> tuple:
        """The one validation of the arguments of the level histogram: ``(log2 of the bucket, the edges as a tuple of float32
        values)``, or SA_EINVAL.  ``group`` may be None (all rows)."""
        keys, _, bucket, _, _ = _rules(frames._hist_args, edges, group, bucket, lo, hi)
        return bucket.bit_length() - 1, tuple(float(v) for v in keys.view(np.float32))

    def _hist_out(self, R: int, group, bucket: int, lo: int, hi: int, L: int, out: Optional[torch.Tensor]) -> tuple:
        """``(group, out)`` of the level histogram of ``R`` rows, ``group`` None meaning all of them and ``out`` allocated when
        None: SA_ESHAPE where R is no multiple of the group or ``out`` is not the contiguous uint32 [G, C, L] tensor on the
        handle's device."""
        A = max(R, 1) if group is None else int(group)
        if A > frames.HIST_GROUP_MAX:
            raise SpecanError(abi.SA_EINVAL, f"group must be 1..{frames.HIST_GROUP_MAX}")
        if R % A:
            raise SpecanError(abi.SA_ESHAPE, f"the rows ({R}) must be a multiple of {A}")
        return A, self._outs(("out", out, (R // A, (int(hi) - int(lo)) // int(bucket), L), torch.uint32))[0]

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
        self._call(abi.hist_lib(), "sa_hist_f32", t.data_ptr(), out.data_ptr(), R, A, log2w, len(edges) + 1,
                   (C.c_float * len(edges))(*edges), int(lo), int(hi))
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
        _, keys = self._hist_args(edges, group, bucket, lo, hi)
        # no spectra_f32 branch: the group divides the rows of the magnitudes, inside _hist_out
        return self._of_spectra(x, None, scale, work, lambda B: self._hist_out(B, group, int(bucket), lo, hi, len(keys) + 1, out),
                                lambda t, field, A_out: self.level_hist(t, edges, A_out[0], bucket, lo, hi, A_out[1]))

    @staticmethod
    def _bands_args(bands, fracs, field) -> tuple:
        """The one validation of the arguments of the band power: ``(field code of include/specan_bands.h, the bands as a
        tuple of (lo, hi) int pairs, the fractions as a tuple of floats)``, or SA_EINVAL."""
        bands, fracs = _rules(frames._bands_args, bands, fracs, field)
        return FIELDS[field], bands, fracs

    def _bands_out(self, R: int, nb: int, nq: int, power: Optional[torch.Tensor], cross: Optional[torch.Tensor]) -> tuple:
        """``(power, cross)`` of the band power of ``R`` rows, each allocated when None: SA_ESHAPE where ``power`` is not the
        contiguous float64 [R, nb] tensor or ``cross`` not the contiguous int32 [R, nb, nq] tensor on the handle's device.
        Without fractions ``cross`` is handed back as it came and never looked at."""
        if nq == 0:
            return self._outs(("power", power, (R, nb), torch.float64))[0], cross
        return tuple(self._outs(("power", power, (R, nb), torch.float64), ("cross", cross, (R, nb, nq), torch.int32)))

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
        c_bands = (abi.Band * nb)(*(abi.Band(lo, hi) for lo, hi in bands))
        c_fracs = (C.c_double * nq)(*fracs) if nq else None
        self._call(abi.bands_lib(), "sa_bands_f32", t.data_ptr(), code, power.data_ptr(), cross.data_ptr() if nq else None, R, nb,
                   c_bands, nq, c_fracs)
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
        return self._of_spectra(x, group, scale, work, lambda R: self._bands_out(R, len(bands), len(fracs), power, cross),
                                lambda t, field, outs: self.band_power(t, bands, fracs, field, *outs))

    @staticmethod
    def _mask_args(upper, lower, lo, hi, field) -> int:
        """The one validation of the scalar arguments of the mask test: the ``field`` code of include/specan_mask.h, or
        SA_EINVAL.  The limits are only counted here; :meth:`_mask_limits` looks at them."""
        _rules(frames._mask_args, upper, lower, lo, hi, field)
        return FIELDS[field]

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
        if summary is None or summary is False:
            return self._outs(("out", out, (R, 10), torch.int32))[0], None
        return tuple(self._outs(("out", out, (R, 10), torch.int32),
                                ("summary", None if summary is True else summary, (4,), torch.int32)))

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
        self._call(abi.mask_lib(), "sa_mask_f32", t.data_ptr(), code, None if upper is None else upper.data_ptr(),
                   None if lower is None else lower.data_ptr(), int(lo), int(hi), out.data_ptr(),
                   None if summary is None else summary.data_ptr(), R)
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

        def limits_and_summary():                    # after the input's check, before the batch's
            self._mask_limits(upper, lower)
            if isinstance(summary, bool):
                raise SpecanError(abi.SA_ESHAPE, "summary must be None or a contiguous torch.int32 tensor of shape (4,)")

        return self._of_spectra(x, group, scale, work, lambda R: self._mask_out(R, out, True if summary is None else summary),
                                lambda t, field, outs: self.mask_test(t, upper, lower, lo, hi, field, *outs),
                                after_input=limits_and_summary)

    @staticmethod
    def _harm_args(order, span, lo, hi, fund, dc, top, field) -> tuple:
        """The one validation of the arguments of the harmonic analysis: ``(field code of include/specan_harm.h, the
        sa_harm_cfg with the defaults filled in)``, or SA_EINVAL."""
        cfg = _rules(frames._harm_args, order, span, lo, hi, fund, dc, top, field)
        return FIELDS[field], abi.HarmCfg(*cfg)

    def _harm_out(self, R: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """The record tensor of the harmonic analysis of ``R`` rows, allocated when None: SA_ESHAPE where ``out`` is not the
        contiguous int32 [R, 42] tensor on the handle's device."""
        return self._outs(("out", out, (R, HARM_WORDS), torch.int32))[0]

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
        self._call(abi.harm_lib(), "sa_harm_f32", t.data_ptr(), code, out.data_ptr(), R, C.byref(cfg))
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
        return self._of_spectra(x, group, scale, work, lambda R: self._harm_out(R, out),
                                lambda t, field, out: self.harmonics(t, order, span, lo, hi, fund, dc, top, field, out))


    @staticmethod
    def _signals_args(k, threshold, lo, hi, gap, min_width, field) -> int:
        """The one validation of the arguments of the signal list: the ``field`` code of include/specan_signals.h, or
        SA_EINVAL.  Of a threshold per row only the dtype is looked at here; :meth:`_signals_out` looks at the rest."""
        _rules(frames._signals_args, k, lo, hi, gap, min_width, field)
        if not isinstance(threshold, torch.Tensor):
            _rules(frames._threshold_key, threshold)
        elif threshold.dtype != torch.float32:
            raise SpecanError(abi.SA_EINVAL, "a threshold per row must be a torch.float32 tensor")
        return FIELDS[field]

    @staticmethod
    def _as_float32(v) -> float:
        """The number ``v`` rounded to float32, as a Python float; what is too large is inf."""
        with np.errstate(over="ignore"):
            return float(np.float32(v))

    def _signals_out(self, R: int, k: int, threshold, out: Optional[torch.Tensor], stats: Optional[torch.Tensor]) -> tuple:
        """``(out, stats)`` of the signal list of ``R`` rows, each allocated when None: SA_ESHAPE where a threshold per row is
        not the contiguous float32 [R] tensor, ``out`` not the contiguous int32 [R, k, 6] tensor or ``stats`` not the contiguous
        int32 [R, 3] tensor on the handle's device."""
        if isinstance(threshold, torch.Tensor) and (tuple(threshold.shape) != (R,) or threshold.device != self.device
                                                    or not threshold.is_contiguous()):
            raise SpecanError(abi.SA_ESHAPE, f"a threshold per row must be a contiguous torch.float32 tensor of shape ({R},)")
        return tuple(self._outs(("out", out, (R, k, SIGNAL_WORDS), torch.int32), ("stats", stats, (R, 3), torch.int32)))

    def find_signals(self, t: torch.Tensor, k: int = 16, threshold=0.0, lo: int = 0, hi: int = SA_N, gap: int = 0,
                     min_width: int = 1, field: Optional[str] = None, out: Optional[torch.Tensor] = None,
                     stats: Optional[torch.Tensor] = None) -> tuple:
        """The signal list of each row of ``t`` (include/specan_signals.h, sa_signals_f32): the runs of bins that stand above
        a threshold.  Returns ``(bounds int32 [R,k,2], peak float32 [R,k], peak_bin int32 [R,k], power float64 [R,k], stats
        int32 [R,3])``: the first four are views of the [R,k,6] int32 record tensor (``out``, allocated when None; one
        sa_signal of 24 bytes per slot, frames.SIGNAL on the host), ``stats`` is allocated when None.  ``t`` is a float32
        [R,16384] device tensor -- what ``process_f32(out_kind='mag_full')`` or ``process_q15(out_kind='mag')`` wrote, squared
        bin by bin in the power -- or, with ``field='peak'`` (squared) or ``field='power'`` (taken as it is), float32
        [R,16384,2], the records of :meth:`fold_mag_f32` at bucket 1, :meth:`spectra_f32` or :meth:`spectra_q15`.

        A point's key is its bits with the sign cleared, as an integer; bin i is on when ``lo <= i < hi``, its key is not 0
        and not below the threshold's.  ``threshold`` is a number (+0.0 .. +inf) for all rows or a contiguous float32 [R]
        tensor on the handle's device, one per row and keyed like a point -- the noise floor of :meth:`order_stats` times a
        factor, say, made on the device.  Off runs of at most ``gap`` bins between two on bins are bridged; the runs
        ``[start, stop)`` of on or bridged bins that are ``min_width`` or more wide are the segments, and the first ``k`` in
        ascending order the records: ``bounds`` (start, stop), the largest point with its bin (equal ones to the lowest), and
        the float64 power of the band ``[start, stop)`` by the balanced pair tree of :meth:`band_power`; the unused slots are
        (-1, -1, +0.0, -1, +0.0).  ``stats[r]`` is (segments kept before the truncation to k, on bins, bins of all kept
        segments).  frames.signals_of_rows is the numpy mirror, bit for bit.

        ``k`` is 1..32, ``0 <= lo < hi <= 16384``, ``gap`` 0..16383, ``min_width`` 1..16384, ints only (a bool or a float is
        SA_EINVAL); a wrong dtype is SA_EINVAL and a wrong shape SA_ESHAPE, all before any device call.  One launch on the
        current stream of the handle's device -- the parameters travel in the launch's arguments -- no atomics, nothing
        zeroed, no handle state, no workspace: it captures into a graph at any time.  Where ``t`` is the result of a call made
        in overlap mode, call :meth:`flush` first.  Pointer contract (checked by the C entry point, SA_EINVAL): ``t`` is
        16-byte aligned, and the R * k * 24 bytes of the records and the R * 12 of ``stats`` meet neither each other nor the
        bytes read; buffers that merely touch are fine."""
        code = self._signals_args(k, threshold, lo, hi, gap, min_width, field)
        R = self._check_in(t, torch.float32, (SA_N, 2) if code else SA_N)
        out, stats = self._signals_out(R, int(k), threshold, out, stats)
        per_row = isinstance(threshold, torch.Tensor)
        self._call(abi.signals_lib(), "sa_signals_f32", t.data_ptr(), code, threshold.data_ptr() if per_row else None,
                   0.0 if per_row else float(threshold), out.data_ptr(), stats.data_ptr(), R, int(k), int(lo), int(hi), int(gap),
                   int(min_width))
        return out[..., :2], out.view(torch.float32)[..., 2], out[..., 3], out.view(torch.float64)[..., 2], stats

    def signals_f32(self, x: torch.Tensor, k: int = 16, threshold=None, factor=None, q=0.5, lo: int = 0, hi: int = SA_N,
                    gap: int = 0, min_width: int = 1, group: Optional[int] = None, scale: float = 1.0 / 2048.0,
                    work: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    stats: Optional[torch.Tensor] = None) -> tuple:
        """The signal list of the float chain's spectra, without the spectra leaving the device: ``(bounds, peak, peak_bin,
        power, stats, thr)``, the five values of :meth:`find_signals` and the threshold per row, float32 [R], or None where the
        threshold is absolute.  ``x`` is float32, int16 or packed uint8 exactly as for :meth:`process_f32`; every filter mode
        and both precisions apply.

        Exactly one of ``threshold`` and ``factor`` is given.  ``threshold`` is absolute, as for :meth:`find_signals`.
        ``factor``, a finite number above 0, makes the threshold ride on the noise: it is ``order_stats(t,
        [frames.rank_of_quantile(q, hi - lo)], lo, hi, field)[:, 0] * float32(factor)`` -- the lower quantile ``q`` of the
        bins ``[lo, hi)`` of each row (0.5: the median) times the factor, one float32 multiply on the current stream -- of the
        very rows the signals are then found in.

        Without ``group`` (R = B) the rows are ``process_f32(x, out_kind='mag_full', scale=scale)`` in the workspace of
        :meth:`spectra_f32`: the signals of every frame.  With ``group=A`` (2, 4, ..., 128; R = B // A) they are
        ``spectra_f32(x, group=A, scale=scale, work=work)`` with ``field='power'``: the signals of the summed power of every A
        consecutive frames, the Welch estimate times A, the threshold in that unit.

        The workspace is ``work`` or the cached tensor, as for :meth:`spectra_f32`, and in overlap mode the call joins every
        outstanding call of the handle on the device (as :meth:`flush` does) before the search: the result is valid on the
        current stream when the call returns, and the call lends nothing.  The parameters, ``out`` and ``stats`` are refused
        as by :meth:`find_signals`, ``q`` as by :meth:`noise_floor_f32` (one number), ``group`` and a B that is no multiple
        of it as by :meth:`spectra_f32`, all before anything is launched, and so is a wrong ``work``."""
        self._signals_args(k, 0.0 if threshold is None else threshold, lo, hi, gap, min_width, None)
        if (threshold is None) == (factor is None):
            raise SpecanError(abi.SA_EINVAL, "exactly one of threshold and factor must be given")
        if factor is not None:
            if not frames._is_number(factor) or not 0.0 < self._as_float32(factor) < float("inf"):
                raise SpecanError(abi.SA_EINVAL, "factor must be a finite number above 0 as a float32")
            rank = _rules(frames.rank_of_quantile, q, int(hi) - int(lo))

        def reduce(t, field, outs):
            thr = threshold
            if factor is not None:
                thr = self.order_stats(t, (rank,), lo, hi, field)[:, 0] * self._as_float32(factor)
            return (*self.find_signals(t, k, thr, lo, hi, gap, min_width, field, *outs), thr if factor is not None else None)

        return self._of_spectra(x, group, scale, work, lambda R: self._signals_out(R, int(k), threshold, out, stats), reduce)

    # ------------------------------------------------------------------ the CFAR normalisation
    @staticmethod
    def _cfar_args(train, guard, mode, what, lo, hi, field) -> tuple:
        """The one validation of the arguments of the CFAR normalisation: ``(field code, log2_train, mode code, what code)``
        of include/specan_cfar.h, or SA_EINVAL."""
        t, _, m, w, _, _ = _rules(frames._cfar_args, train, guard, mode, what, lo, hi, field)
        return FIELDS[field], t, m, w

    def _cfar_out(self, R: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``out`` of the CFAR normalisation of ``R`` rows, allocated when None: SA_ESHAPE where it is not the contiguous
        float32 [R, 16384] tensor on the handle's device."""
        return self._outs(("out", out, (R, SA_N), torch.float32))[0]

    def cfar(self, t: torch.Tensor, train: int = 16, guard: int = 2, mode: str = "ca", what: str = "ratio", lo: int = 0,
             hi: int = SA_N, field: Optional[str] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Every bin of each row of ``t`` against its local noise floor (include/specan_cfar.h, sa_cfar_f32): float32
        [R,16384] (``out``, allocated when None), a cell-averaging CFAR.  ``t`` is a float32 [R,16384] device tensor -- what
        ``process_f32(out_kind='mag_full')`` or ``process_q15(out_kind='mag')`` wrote, squared bin by bin -- or, with
        ``field='peak'`` (squared) or ``field='power'`` (taken as it is), float32 [R,16384,2], the records of
        :meth:`fold_mag_f32` at bucket 1, :meth:`spectra_f32` or :meth:`spectra_q15`.

        The floor of bin i is the mean power of the ``train`` cells below it and the ``train`` cells above it, ``guard`` cells
        left out on either side, of which only those inside ``[lo, hi)`` count (``mode='ca'``); ``'go'`` takes the side with
        the larger mean, which holds the false alarms down at a step of the floor, and ``'so'`` the side with the smaller,
        which keeps a neighbouring emission from masking a bin.  ``what='ratio'`` gives the bin's power over that floor, a
        pure number that :meth:`find_signals`, :meth:`find_peaks`, :meth:`mask_test` and :meth:`level_hist` take as
        magnitudes with a threshold such as ``frames.cfar_alpha(pfa, 2 * train)``; ``what='floor'`` the floor itself, a
        power.  Bins outside ``[lo, hi)`` are +0.0.  Every sum is a float64 balanced pair tree in bin order, the quotient a
        float64 division rounded once to float32: frames.cfar_of_rows is the numpy mirror, bit for bit.

        ``train`` is 1, 2, 4, ..., 64, ``guard`` 0..64, ``0 <= lo < hi <= 16384`` with ``hi - lo >= 2 * guard + 2``, ints only
        (a bool or a float is SA_EINVAL); ``mode`` is 'ca', 'go' or 'so' and ``what`` 'ratio' or 'floor'; a wrong dtype is
        SA_EINVAL and a wrong shape SA_ESHAPE, all before any device call.  One launch on the current stream of the handle's
        device -- the parameters travel in the launch's arguments -- no atomics, nothing zeroed, no handle state, no
        workspace: it captures into a graph at any time.  Where ``t`` is the result of a call made in overlap mode, call
        :meth:`flush` first.  Pointer contract (checked by the C entry point, SA_EINVAL): ``t`` and ``out`` are 16-byte
        aligned and the R * 65536 bytes written do not meet the bytes read; buffers that merely touch are fine."""
        code, log2_train, m, w = self._cfar_args(train, guard, mode, what, lo, hi, field)
        R = self._check_in(t, torch.float32, (SA_N, 2) if code else SA_N)
        out = self._cfar_out(R, out)
        self._call(abi.cfar_lib(), "sa_cfar_f32", t.data_ptr(), code, out.data_ptr(), R, log2_train, int(guard), m, w, int(lo),
                   int(hi))
        return out

    def cfar_f32(self, x: torch.Tensor, train: int = 16, guard: int = 2, mode: str = "ca", what: str = "ratio", lo: int = 0,
                 hi: int = SA_N, group: Optional[int] = None, scale: float = 1.0 / 2048.0,
                 work: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The CFAR normalisation of the float chain's spectra, without the spectra leaving the device: float32 [R,16384],
        the value of :meth:`cfar`.  ``x`` is float32, int16 or packed uint8 exactly as for :meth:`process_f32`; every filter
        mode and both precisions apply.

        Without ``group`` (R = B) the rows are ``process_f32(x, out_kind='mag_full', scale=scale)`` in the workspace of
        :meth:`spectra_f32`: every frame against its own floor.  With ``group=A`` (2, 4, ..., 128; R = B // A) they are
        ``spectra_f32(x, group=A, scale=scale, work=work)`` with ``field='power'``: the summed power of every A consecutive
        frames against its floor -- a smoother floor, to which ``frames.cfar_alpha`` does not apply.

        The workspace is ``work`` or the cached tensor, as for :meth:`spectra_f32`, and in overlap mode the call joins every
        outstanding call of the handle on the device (as :meth:`flush` does) before the normalisation: the result is valid on
        the current stream when the call returns, and the call lends nothing.  The parameters and ``out`` are refused as by
        :meth:`cfar`, ``group`` and a B that is no multiple of it as by :meth:`spectra_f32`, all before anything is launched,
        and so is a wrong ``work``."""
        self._cfar_args(train, guard, mode, what, lo, hi, None)
        return self._of_spectra(x, group, scale, work, lambda R: self._cfar_out(R, out),
                                lambda t, field, o: self.cfar(t, train, guard, mode, what, lo, hi, field, o))
