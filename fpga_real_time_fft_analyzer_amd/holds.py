"""The percentile traces of ``SpectrumChain``: the calls of libspecan_hold.so (include/specan_hold.h) -- per bin the values at
given ranks of the sorted frames of every group of A rows: the min hold, a median or percentile trace, the max hold -- on a
tensor the caller has (``hold_ranks``) and composed with the float chain, the spectra never leaving the device
(``hold_f32``).

``Holds`` is a mixin of ``SpectrumChain`` beside ``reductions.Reductions``, whose skeleton it uses through ``self``:
``_outs``, ``_call``, ``_mag_full_in_work``, and ``_check_in`` and ``_float_frames`` of the chain.  The rules of the scalar
arguments are those of the numpy mirror, stated once in frames.py (``frames._hold_args``) and turned into SA_EINVAL with the
same text by ``reductions._rules``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import abi, frames
from .abi import SA_N, SpecanError
from .reductions import FIELDS, _rules


class Holds:
    """The percentile-trace methods of ``SpectrumChain`` (module docstring)."""

    @staticmethod
    def _hold_args(ranks, group, field) -> tuple:
        """The one validation of the arguments of the percentile traces: ``(field code of include/specan_hold.h, the ranks as
        a tuple of ints, the group)``, or SA_EINVAL."""
        ranks, group = _rules(frames._hold_args, ranks, group, field)
        return FIELDS[field], ranks, group

    @staticmethod
    def _hold_quantile_ranks(q, group) -> tuple:
        """``q``, a number in 0..1 or a sequence of 1..8 of them, as the ranks of those lower quantiles among ``group`` frames
        (frames.rank_of_quantile), or SA_EINVAL; ``group`` has been checked."""
        qs = q if hasattr(q, "__len__") and not isinstance(q, (str, bytes)) else (q,)
        if not 1 <= len(qs) <= abi.SA_HOLD_Q_MAX:
            raise SpecanError(abi.SA_EINVAL, f"q must be a number or a sequence of 1..{abi.SA_HOLD_Q_MAX} numbers")
        return tuple(_rules(frames.rank_of_quantile, v, group) for v in qs)

    def _hold_out(self, R: int, group: int, q: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``out`` of the percentile traces of ``R`` rows, allocated when None: SA_ESHAPE where R is no multiple of the group
        or ``out`` is not the contiguous float32 [R // group, q, 16384] tensor on the handle's device."""
        if R % group:
            raise SpecanError(abi.SA_ESHAPE, f"the rows ({R}) must be a multiple of {group}")
        return self._outs(("out", out, (R // group, q, SA_N), torch.float32))[0]

    def hold_ranks(self, t: torch.Tensor, ranks: Sequence[int], group: int, field: Optional[str] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Percentile traces of the rows of ``t`` (include/specan_hold.h, sa_hold_f32): float32 [R // group, q, 16384],
        ``[g, j, i]`` the value at rank ``ranks[j]`` of the ascending sort of bin i over the ``group`` consecutive rows of
        group g.  Rank 0 is the min hold, rank ``group - 1`` the max hold, rank ``(group - 1) // 2`` the lower median;
        frames.rank_of_quantile gives the rank of a quantile.  ``t`` is a float32 [R,16384] device tensor -- what
        ``process_f32(out_kind='mag_full')`` or ``process_q15(out_kind='mag')`` wrote -- or, with ``field='peak'`` or
        ``field='power'``, float32 [R,16384,2], the records of :meth:`fold_mag_f32` at bucket 1, :meth:`spectra_f32` or
        :meth:`spectra_q15`, of which that float is the point.  Every ``[g, j]`` of the result is a row of magnitudes that
        :meth:`find_peaks`, :meth:`order_stats`, :meth:`mask_test`, :meth:`find_signals` and :meth:`cfar` take as it is
        (``out.view(-1, 16384)``).

        A point's key is its bits with the sign cleared, as an integer: the float order of the chains' non-negative values; a
        NaN ranks above +inf, -0.0 reads as +0.0, no denormal is flushed; the result is those bits.  frames.holds_of_rows is
        the numpy mirror, bit for bit.  Rank ``group - 1`` is ``[..., 0]`` of :meth:`fold_mag_f32` at the same group and
        bucket 1.  All ranks come from one sort: the cost hardly depends on their number.

        ``group`` is an int in 2..128, any, not only a power of two; ``ranks`` a sequence of 1..8 ints, each
        ``0 <= rank < group``, in any order, repeats allowed; ints only (a bool or a float is SA_EINVAL); a wrong dtype is
        SA_EINVAL, a wrong shape and an R that is no multiple of ``group`` SA_ESHAPE, all before any device call.  One launch
        on the current stream of the handle's device -- the ranks travel in the launch's arguments -- no handle state, no
        workspace: it captures into a graph at any time.  Where ``t`` is the result of a call made in overlap mode, call
        :meth:`flush` first.  Pointer contract (checked by the C entry point, SA_EINVAL): both tensors are 16-byte aligned,
        and the bytes read and the (R // group) * q * 65536 bytes written are disjoint; buffers that merely touch are
        fine."""
        code, ranks, group = self._hold_args(ranks, group, field)
        R = self._check_in(t, torch.float32, (SA_N, 2) if code else SA_N)
        out = self._hold_out(R, group, len(ranks), out)
        self._call(abi.hold_lib(), "sa_hold_f32", t.data_ptr(), code, out.data_ptr(), R, group, len(ranks),
                   (C.c_int32 * len(ranks))(*ranks))
        return out

    def hold_f32(self, x: torch.Tensor, q=0.5, group: int = 16, scale: float = 1.0 / 2048.0,
                 work: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Percentile traces of the float chain's spectra, without the spectra leaving the device: float32
        [B // group, len(q), 16384], per bin the lower quantiles ``q`` (a number in 0..1, which gives one trace, or a sequence
        of 1..8 of them; 0.0 is the min hold, 0.5 the lower median, 1.0 the max hold) of the magnitudes of every ``group``
        consecutive frames, each the order statistic of rank ``frames.rank_of_quantile(q, group)``.  ``x`` is float32, int16
        or packed uint8 exactly as for :meth:`process_f32`; every filter mode and both precisions apply.  The call is
        ``process_f32(x, out_kind='mag_full', scale=scale)`` into the workspace of :meth:`spectra_f32` followed by
        :meth:`hold_ranks`.

        The workspace is ``work`` or the cached tensor, as for :meth:`spectra_f32`, and in overlap mode the call joins every
        outstanding call of the handle on the device (as :meth:`flush` does) before the sort: the result is valid on the
        current stream when the call returns, and the call lends nothing.  ``q``, ``group``, a B that is no multiple of it
        and ``out`` are refused as by :meth:`hold_ranks`, all before anything is launched -- the arguments, then the input,
        then the batch, then ``out`` -- and so is a wrong ``work``."""
        _, _, group = self._hold_args((0,), group, None)
        ranks = self._hold_quantile_ranks(q, group)
        B = self._float_frames(x)
        out = self._hold_out(B, group, len(ranks), out)
        return self.hold_ranks(self._mag_full_in_work(x, B, scale, work), ranks, group, None, out)
